// multi_c64.hpp -- what the complex64 multi-vector product (csr_multi_c64.hip) and the batched complex64 loops
// (solvers_multi_c64.hip) share.  Not installed.
//
// A block of k complex64 vectors is ONE array of n * k interleaved (re, im) float pairs, row-major: column j of row i is floats
// 2 (i k + j) and 2 (i k + j) + 1; k = 2, 4, 8; the base 16-byte aligned, so a row is k / 2 aligned 16-byte pieces, each holding two
// neighbouring columns.  DESIGN.md section 21.
//
// The product's fma order, per entry a of the row and column x, the same as lcg_hip_spmv_c64's (csr_c64.hip: c64_mac):
//     re = fma(a.re, x.re, re); re = fma(-a.im, x.im, re); im = fma(a.re, x.im, im); im = fma(a.im, x.re, im)
// in fp32; a lane adds its entries in entry order, the T lanes of a row are added in slot order.
#pragma once

#include "multi.hpp"

namespace lcgh {

// entries per LDS window of k_cspmm_c64: 27,648 B of staging (8 B value + 4 B column), five blocks per CU; the row-sum exchange of
// k = 8 (256 lanes x 8 float pairs = 2048 value slots) fits the value window in one round, and 64 rows of 33 entries fit one window
constexpr int C64MM_W = 2304;

// a CSR handle this path serves: complex64, whole (not sharded), not dense (0, or LCG_HIP_E_ARG with the text)
int c64multi_handle(const char *entry, const lcg_hip_csr *A);

// Y = A.X for the k complex64 columns in one launch (P's plain CSR arrays, val = interleaved (re, im) floats: no plan is built or used),
// summed in fp32.  With U: column j's UNCONJUGATED sum (A.X)_j . U_j, exact fp64 products summed in fp64, is left as *slots <= MM_MG
// partial sums, re at dots[(2 j) * MM_MG ...], im at dots[(2 j + 1) * MM_MG ...], to be added in index order.  `big` holds the
// per-workgroup sums of a matrix with more than MM_MG row blocks on their way there (cspmm_c64_big_doubles(P, k) doubles; may be null
// where that is 0).  multi.hpp's frame with two table rows per column.
int cspmm_c64_launch(const CsrPart &P, int k, const float *X, float *Y, hipStream_t s, const int *done, const float *U = nullptr,
                     double *big = nullptr, double *dots = nullptr, int *slots = nullptr);
inline size_t cspmm_c64_big_doubles(const CsrPart &P, int k) { return multi_big_doubles(P, 2 * k); }

} // namespace lcgh
