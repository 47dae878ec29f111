// multi_cplx.hpp -- what the complex multi-vector product (csr_multi_cplx.hip) and the batched complex loops
// (solvers_multi_cplx.hip) share.  Not installed.
//
// A block of k complex vectors is ONE array of n * k interleaved (re, im) pairs, row-major: column j of row i is the 16-byte piece
// i * k + j (doubles 2 (i k + j) and 2 (i k + j) + 1); k = 2, 4, 8; the base 16-byte aligned.  DESIGN.md section 18.
#pragma once

#include "multi.hpp"

namespace lcgh {

constexpr int CMM_W = 1536;     // entries per LDS window of k_cspmm: 30,720 B of staging (16 B value + 4 B column), five blocks per CU

// a CSR handle this path serves: complex128, whole (not sharded), not dense (0, or LCG_HIP_E_ARG with the text)
int cmulti_handle(const char *entry, const lcg_hip_csr *A);

// Y = A.X for the k complex columns in one launch (P's plain CSR arrays, val = interleaved (re, im): no plan is built or used).  With
// U: column j's UNCONJUGATED sum (A.X)_j . U_j is left as *slots <= MM_MG partial sums, re at dots[(2 j) * MM_MG ...], im at
// dots[(2 j + 1) * MM_MG ...], to be added in index order.  `big` holds the per-workgroup sums of a matrix with more than MM_MG row
// blocks on their way there (cspmm_big_doubles(P, k) doubles; may be null where that is 0).  multi.hpp's frame with two table rows per
// column.
int cspmm_launch(const CsrPart &P, int k, const double *X, double *Y, hipStream_t s, const int *done, const double *U = nullptr,
                 double *big = nullptr, double *dots = nullptr, int *slots = nullptr);
inline size_t cspmm_big_doubles(const CsrPart &P, int k) { return multi_big_doubles(P, 2 * k); }

} // namespace lcgh
