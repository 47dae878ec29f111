/*
 * lcg_hip_staging_dense_c64.h -- the complex64 dense entries of liblcg_hip.so, waiting for their place in lcg_hip.h.
 *
 * The rule is lcg_hip_staging.h's: every entry that lcg_hip.h declares has a line in the stream-coverage table of the test suite
 * (tests/stream_cases.py), and a feature pull request does not edit existing tests, so an entry that such a pull request adds is
 * declared outside lcg_hip.h, with its full contract, exported by the library and bound by the Python front like any other; the test
 * pull request that gives it its table line (tests/dense_c64_cases.py holds the lines ready) moves its declaration, word for word,
 * into lcg_hip.h -- it moves into lcg_hip.h with its stream-coverage line.
 *
 * Why a file of its own: the suite pins the other staging headers to the names they held when their own tests were written, so a
 * further staged entry cannot join any of them without editing those tests.  These entries are bound in
 * liblcg_amd._lib.STAGING_DENSE_C64_SIGNATURES.  Nothing else distinguishes them: the ABI rules, codes, memory convention and types
 * are lcg_hip.h's.
 *
 * A complex64 dense handle is a lcg_hip_dense_t whose element type is complex64.  lcg_hip_dense_rows, _cols, _destroy,
 * _last_kernel, _multi_last_kernel and _set_kernel serve it (set_kernel: AUTO, ROW, ROW_SPLIT and COL; the K^T.K variants return
 * LCG_HIP_E_ARG).  Every other entry for real or complex128 dense handles returns LCG_HIP_E_ARG before the device is touched, with
 * "complex64" in lcg_hip_last_error() and its outputs untouched; the entries below answer a real or complex128 dense handle, and
 * every CSR handle, the same way.  All products are fp32 throughout, every multiply-add an explicit fused one, every sum added in an
 * order the shape and the forced variant fix: the same bits from call to call.  No atomics.
 */
#ifndef LCG_HIP_STAGING_DENSE_C64_H
#define LCG_HIP_STAGING_DENSE_C64_H

#include "lcg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An M x N complex64 matrix resident in HBM.  val: row-major interleaved (re, im) float pairs, row i at val + 2 * i * ld floats (ld
 * counted in entries, ld >= N), living where `mem` says; it is copied.  The checks and codes are lcg_hip_dense_create's.  Storage:
 * rows padded to whole 16-byte packs of two entries (columns 2p and 2p + 1), ceil(N / 2) packs per row, pads zero, 64 bytes of slack:
 * 8 bytes per entry where a complex128 handle holds 16. */
int lcg_hip_dense_create_c64(lcg_hip_dense_t *K, int m_rows, int n_cols, const float *val, int64_t ld, int mem);

/* y = K.x (layout 0, conjugate 0), conj(K).x (0, 1), K^T.x (1, 0) or K^H.x (1, 1): x and y device vectors of interleaved float
 * pairs, N (layout 1: M) and M (N) entries.  Per entry the fused multiply-adds of lcg_hip_spmv_c64 in its order; a row's (a
 * column's) terms are added in an order fixed by the shape and the forced variant.  k_cdn_row: W lanes per row; k_cdn_row_split:
 * the row cut into strips, fp32 partial sums in slots added by k_cdn_fold in one fixed order; k_cdn_col: a lane owns a pack of
 * columns and walks a strip of rows.  LCG_HIP_E_ARG: the handle is not a complex64 dense one, x or y is NULL or the same vector,
 * layout or conjugate is neither 0 nor 1.  Inside a solve the product falls through once the solve has stopped. */
int clcg_hip_dense_matvec_c64(lcg_hip_dense_t K, const float *x, float *y, int layout, int conjugate);

/* clcg_hip_axfunc_c64_ptr callbacks for clcg_hip_solver_c64 / clcg_hip_solver_preconditioned_c64 with instance = the handle:
 * clcg_hip_dense_ax_c64 is clcg_hip_dense_matvec_c64 on a square K (BiCG asks for K^H, BiCG-sym and PCG for K alone);
 * clcg_hip_dense_jacobi_mx_c64 is z = x .* (1 / diag) after lcg_hip_dense_build_jacobi_c64, layout / conjugate ignored.  A failure
 * (not a complex64 dense handle, not square, n_size differs from N, no reciprocals built) ends the solve with LCG_HIP_E_ARG, nothing
 * written, as the other built-in callbacks do. */
void clcg_hip_dense_ax_c64(void *instance, const float *x, float *prod_Ax, const int n_size, int layout, int conjugate);
void clcg_hip_dense_jacobi_mx_c64(void *instance, const float *x, float *prod_Mx, const int n_size, int layout, int conjugate);

/* The reciprocals 1 / K(i,i) of a square K, formed on the device by the scaled division the complex64 loops use (cuCdivf's
 * formula), kept with the handle for clcg_hip_dense_jacobi_mx_c64 and clcg_hip_dense_lpcg_multi_c64.  diag_out (device, N float
 * pairs, or NULL) receives the diagonal itself.  LCG_HIP_E_ARG: not a complex64 dense handle, not square, or a diagonal entry that
 * is zero or not finite (no reciprocals are kept then). */
int lcg_hip_dense_build_jacobi_c64(lcg_hip_dense_t K, float *diag_out);

/* Y = K.X (conjugate 0) or conj(K).X (1) for k = 2, 4 or 8 complex64 vectors with K read ONCE for all of them.  X (N x k) and Y
 * (M x k) are blocks in clcg_hip_spmm_c64's layout: column j of row i is floats 2 (i k + j) and 2 (i k + j) + 1, the base 16-byte
 * aligned; device memory.  One kernel for every k, k_cdnm_mfma, on the fp32 matrix instruction (v_mfma_f32_16x16x4_f32, whose
 * result is a k-ordered chain of fp32 fused multiply-adds): a wavefront multiplies 16 rows of K by a tile whose 16 columns are the
 * re and im outputs of 8 block columns; at k = 2 and 4 the missing columns are zeros and are not stored, so column j's sums are the
 * same instructions, and the same bits, whatever k is, wherever the column stands and whatever the other columns hold (NaN and Inf
 * included), from call to call.  Rows cut into strips (k_cdnm_mfma_split) leave fp32 partial sums in slots that k_cdn_fold adds in
 * one fixed order.  LCG_HIP_E_ARG before the device is touched, Y untouched: k not 2, 4 or 8; a null or misaligned X / Y; not a
 * complex64 dense handle; conjugate neither 0 nor 1; X and Y overlap. */
int clcg_hip_dense_matmat_c64(lcg_hip_dense_t K, int k, const float *X, float *Y, int conjugate);

/* Y = K.X on a square K as above and, with U (a third block), dots[2 j], dots[2 j + 1] (host array of 2 k doubles) = re, im of the
 * UNCONJUGATED sum_i Y_ij U_ij: exact fp64 products of the fp32 values added in fp64 as one binary tree that does not depend on k
 * (k_cdnm_dot) -- what the batched complex64 loops take after their product.  U NULL: the product alone (dots must be NULL too).
 * LCG_HIP_E_ARG as clcg_hip_dense_matmat_c64's, and: K not square; Y overlaps X or U; dots without U. */
int clcg_hip_dense_op_multi_dot_c64(lcg_hip_dense_t K, int k, const float *X, float *Y, const float *U, double *dots);

/* clcg_hip_lbicg_sym_multi_c64 and clcg_hip_lpcg_multi_c64 on a square complex-symmetric complex64 dense handle: the same loops,
 * arguments, stop rule, NaN rule, frozen columns and codes, with K read once per iteration for all k columns by
 * clcg_hip_dense_op_multi_dot_c64's kernels.  Column j's iterate, count, residual and code are the same bits whatever k is, wherever
 * the column stands, whatever the other columns hold and from call to call.  PCG uses the reciprocals of
 * lcg_hip_dense_build_jacobi_c64 and returns LCG_NULL_PRECONDITION_MATRIX without them.  LCG_HIP_E_ARG, ret untouched: k, a null or
 * misaligned M / B, not a complex64 dense handle, a K that is not square, mem. */
int clcg_hip_dense_lbicg_sym_multi_c64(lcg_hip_dense_t K, int k, float *M, const float *B, const clcg_para *param,
                                       int *ret, int *iterations, double *residual, int mem);
int clcg_hip_dense_lpcg_multi_c64(lcg_hip_dense_t K, int k, float *M, const float *B, const clcg_para *param,
                                  int *ret, int *iterations, double *residual, int mem);

/* Entry `index` of the complex64 dense kernel names (k_cdn_row, k_cdn_row_split, k_cdn_col, k_cdnm_mfma, k_cdnm_mfma_split: what
 * lcg_hip_dense_last_kernel and lcg_hip_dense_multi_last_kernel report for such a handle), or NULL past the end. */
const char *clcg_hip_dense_kernel_name_c64(int index);

#ifdef __cplusplus
}
#endif
#endif /* LCG_HIP_STAGING_DENSE_C64_H */
