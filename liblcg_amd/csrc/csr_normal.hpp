// csr_normal.hpp -- the normal state of a real fp64 CSR handle K (M x N): what lcg_hip_csr_build_normal leaves beside the matrix so
// that K^T.x and K^T.(K.x) are products of the kernels the library has (csr_normal.hip).  Not installed.
#pragma once

#include "internal.hpp"
#include "lcg_hip_staging_csr_normal.h"

namespace lcgh {

struct CsrNormal {
    CsrPart T;                  // K^T: N rows, M columns, rows sorted by source row, duplicates in K's own entry order; owned, padded
    double *t = nullptr;        // K.x on its way to K^T: M doubles
    double *tk = nullptr;       // the same for a block of kmax vectors: M x kmax doubles, reserved before a batched loop starts
    int kmax = 0;
    double *invdiag = nullptr;  // 1 / sum_i K(i,c)^2, N doubles (lcg_hip_csr_build_jacobi_normal); the handle's invdiag stays the square diagonal's
    bool stale = false;         // the handle's arrays may have been rewritten since the build (csr.hip: op_copies_free)
    int longest = 0;            // entries of the longest column of K = of the longest row of K^T
    double build_ms = 0.0;      // host time of the latest build of K^T
};

// The checks every entry of csr_normal.hip begins with.  A dense, complex, complex64 or sharded handle: LCG_HIP_E_ARG before the device
// is touched.  Then the device; then a null handle or (need_state) one without the normal state: LCG_HIP_E_ARG.  A stale state is
// built again here.  0: K->normal may be used.
int normal_kind(const char *entry, const lcg_hip_csr *K);                   // the first part alone: touches nothing
int normal_ready(const char *entry, lcg_hip_csr *K, bool need_state = true);
// the M x k block of a batched loop or a k-wide entry: the first call at a k larger than any before allocates, later ones do nothing
int normal_reserve(lcg_hip_csr *K, int k);

} // namespace lcgh
