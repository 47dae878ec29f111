/*
 * lcg_hip_staging_csr_normal.h -- sparse least squares on a rectangular CSR matrix: the entries of liblcg_hip.so that multiply by
 * K^T and by K^T.K and run the batched loops on K^T.K, waiting for their place in lcg_hip.h.
 *
 * The rule is lcg_hip_staging.h's: every entry that lcg_hip.h declares has a line in the stream-coverage table of the test suite
 * (tests/stream_cases.py), and a feature pull request does not edit existing tests, so an entry that such a pull request adds is
 * declared outside lcg_hip.h, with its full contract, exported by the library and bound by the Python front like any other; the test
 * pull request that gives it its table line (tests/csr_normal_cases.py holds the lines ready) moves its declaration, word for word,
 * into lcg_hip.h -- it moves into lcg_hip.h with its stream-coverage line.
 *
 * Why a file of its own: the suite pins the earlier staging headers to the names they held when their own tests were written, so a
 * further staged entry cannot join any of them without editing those tests.  These entries are bound in
 * liblcg_amd._lib.STAGING_CSR_NORMAL_SIGNATURES.  Nothing else distinguishes them: the ABI rules, codes, memory convention and types
 * are lcg_hip.h's.
 *
 * The workload.  liblcg's first sample solves K^T.K m = K^T d through a callback that multiplies by K and then by K^T, and the one
 * sparse product the reference ships, lcg_matvec_coo (algebra.cpp:195-221), takes an M x N matrix in both orientations for it.
 * lcg_hip_dense_ata_ax and the dense batched loops serve a dense K; these entries serve a sparse one: K is a real fp64 CSR handle of
 * M = lcg_hip_csr_rows(K) rows and N = lcg_hip_csr_cols(K) columns on one GPU (lcg_hip_csr_create takes n_rows != n_cols), and
 * K^T.K is never formed -- with t entries per row of K it would hold about t^2 per row.
 *
 * One application of K^T.K is two products, t = K.x over the handle's arrays and y = K^T.t over a copy of K^T that
 * lcg_hip_csr_build_normal materialises (12 bytes per entry of extra memory), both by the kernels of lcg_hip_spmv / lcg_hip_spmm:
 * no atomics, the same bits from call to call.  There is no damping argument: K^T.K + lambda I is K'^T.K' with K' = [K; sqrt(lambda) I],
 * so a damped problem stacks N one-entry rows under K (and N zeros under d).
 *
 * Refusals common to every entry below but the query lcg_hip_csr_cols, in this order.  Before the device is touched, LCG_HIP_E_ARG
 * with nothing written and lcg_hip_last_error() naming the entry and the reason: a dense, complex, complex64 or sharded handle (a
 * handle sharded after its normal state was built is refused like any other).  Then the entry's own argument
 * checks, where it has any (LCG_HIP_E_ARG, still nothing touched).  Then the device (LCG_HIP_E_NO_DEVICE where there is none).  Then
 * LCG_HIP_E_ARG for a null handle and -- every entry but lcg_hip_csr_cols and lcg_hip_csr_build_normal -- for a handle without the
 * normal state, the text naming lcg_hip_csr_build_normal.  The batched loops then return the reference's parameter codes in the
 * reference's order.
 *
 * The rewrite protocol.  lcg_hip_csr_set_packed / _set_tiled / _set_binned / _set_ranges (K, 0) announce that the handle's arrays may be
 * rewritten.  The normal state survives them: it is marked stale, and the next entry below that needs it builds K^T (and the
 * reciprocals of lcg_hip_csr_build_jacobi_normal, if they were built) again from the arrays as they are then, before it does its work.
 */
#ifndef LCG_HIP_STAGING_CSR_NORMAL_H
#define LCG_HIP_STAGING_CSR_NORMAL_H

#include "lcg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- build and queries ---- */

/* N, the number of columns the handle was created with (lcg_hip_csr_rows gives M); 0 for a null handle.  A query answered on the host
 * for every CSR handle -- complex, complex64 and sharded ones too: of the common refusals only the dense handle's applies
 * (LCG_HIP_E_ARG, as lcg_hip_csr_rows). */
int lcg_hip_csr_cols(lcg_hip_csr_t A);

/* Builds the normal state of K on the device: K^T as a CSR matrix of N rows and M columns with the slack and alignment of the
 * library's own arrays, and the M doubles between the two products.  Idempotent: a second call does nothing (a stale state is built
 * again).  LCG_HIP_E_ARG, with nothing kept, if a column index of K lies outside [0, N).
 * The order inside K^T: a row of K^T holds the entries of a column of K sorted by source row, and entries of equal (row, column) stand
 * in K's own entry order -- K^T is the stable sort of K's entries by column.  The order depends on the matrix alone, not on its values:
 * the same matrix gives the same three arrays bit for bit on every build.
 * Cost: one thread sorts a column of up to 32 entries; a longer one is sorted by workgroups, 8192 entries at a time in LDS, and merged
 * beyond that, so a column of L entries costs about L log L, not L^2.  The call drains the stream. */
int lcg_hip_csr_build_normal(lcg_hip_csr_t K);

/* What the build left (any pointer may be NULL): the entries of the longest column of K; the bytes the normal state holds beside the
 * matrix (K^T's arrays, the M doubles, the M x k block of the k-wide entries once one has run, the N reciprocals once built); the host
 * time of the latest build of K^T in milliseconds.  Not counted: the kernel plans (packed columns, tiles, bins, row ranges) that the
 * single-vector products may build for K^T at their first use, as they do for K itself -- lcg_hip_csr_plan_info reports K's, K^T's
 * have no query; they are freed with the state. */
int lcg_hip_csr_normal_info(lcg_hip_csr_t K, int *longest_column, int64_t *extra_bytes, double *build_ms);

/* Device pointers of K^T -- rowptr[N + 1], col[nnz], val[nnz] -- as lcg_hip_csr_arrays gives K's.  They belong to the handle and are
 * replaced when a stale state is built again. */
int lcg_hip_csr_normal_arrays(lcg_hip_csr_t K, const int **rowptr, const int **col, const double **val);

/* ---- single-vector products (device pointers, on the library's stream) ---- */

/* y[N] = K^T.x[M]: how b = K^T.d is formed.  LCG_HIP_E_ARG for a null x or y.  Like lcg_hip_spmv it takes device vectors, and the
 * library has no entry that allocates device memory: the caller brings it (hipMalloc, a torch tensor).  A program built without
 * the HIP headers forms b on the host; the solvers and the batched loops take host vectors (LCG_HIP_MEM_HOST), the products do not. */
int lcg_hip_spmv_t(lcg_hip_csr_t K, const double *x, double *y);

/* y[N] = K^T.(K.x[N]): lcg_hip_spmv's launch on K into the state's M doubles, then on K^T -- each matrix chooses its own kernel
 * family.  x and y may be the same vector.  LCG_HIP_E_ARG for a null x or y. */
int lcg_hip_csr_ata(lcg_hip_csr_t K, const double *x, double *y);

/* lcg_hip_csr_ata as the Afp callback of lcg_hip_solver (CG, CGS, BiCGStab, BiCGStab2), lcg_hip_solver_preconditioned (PCG) and
 * lcg_hip_solver_constrained (PG, SPG) with instance = K and n_size = N: the loops run on K^T.K unchanged.  Inside a solve both launches
 * fall through once the loop has stopped, like lcg_hip_csr_ax's, and both are counted as products by lcg_hip_last_launches.  The
 * callback returns nothing: a refusal (n_size not N among them) is parked and ends the solve with its code, as lcg_hip_dense_ata_ax's. */
void lcg_hip_csr_ata_ax(void *instance, const double *x, double *prod_Ax, const int n_size);

/* ---- Jacobi ---- */

/* The Jacobi preconditioner of K^T.K: d_c = sum_i K(i,c)^2, each column's squares added in a fixed order over its row of K^T, and
 * the reciprocals 1 / d_c kept beside -- not in -- the reciprocals of lcg_hip_csr_build_jacobi, which stay the square diagonal's.
 * diag_out (device, N doubles, or NULL) receives d.  A column of K without a positive finite sum of squares is a model parameter
 * that no datum sees, and K^T.K is singular: LCG_HIP_E_ARG, the text naming the first such column, and nothing is stored (earlier
 * reciprocals stay).  The call drains the stream. */
int lcg_hip_csr_build_jacobi_normal(lcg_hip_csr_t K, double *diag_out);

/* prod_Mx = x .* (1 / d) as the Mfp callback of lcg_hip_solver_preconditioned beside lcg_hip_csr_ata_ax (instance = K, n_size = N).
 * Refusals are parked: those above, n_size not N, the reciprocals not built. */
void lcg_hip_csr_jacobi_normal_mx(void *instance, const double *x, double *prod_Mx, const int n_size);

/* ---- k-wide products: k = 2, 4 or 8 vectors as one row-major block, lcg_hip_spmm's layout and alignment rules ---- */

/* Y[N x k] = K^T.X[M x k].  LCG_HIP_E_ARG as lcg_hip_spmm: k, a null or misaligned block. */
int lcg_hip_spmm_t(lcg_hip_csr_t K, int k, const double *X, double *Y);

/* Y[N x k] = K^T.(K.X[N x k]): lcg_hip_spmm's launch on K into the state's M x k block (allocated at the first call with a k larger
 * than any before), then on K^T; both matrices are read once for all k columns. */
int lcg_hip_csr_ata_multi(lcg_hip_csr_t K, int k, const double *X, double *Y);

/* The same product with the sum the batched loops take after it carried by the second launch: dots[j] = Y_j . U_j (host array of k),
 * U an N x k block.  The call waits for the result.
 * For all three: column j of Y, and dots[j], are the same bits whatever k is, wherever the column stands, whatever the other columns
 * hold (NaN and Inf included), from call to call. */
int lcg_hip_csr_ata_multi_dot(lcg_hip_csr_t K, int k, const double *X, double *Y, const double *U, double *dots);

/* ---- batched loops on K^T.K ---- */

/* lcg_hip_dense_lcg_multi(normal = 1) and lcg_hip_dense_lpcg_multi(normal = 1) on a sparse K: batched CG and PCG (Jacobi, the
 * reciprocals of lcg_hip_csr_build_jacobi_normal) over k = 2, 4 or 8 right-hand sides, M (in/out) and B N x k blocks living where
 * `mem` says.  The contract is the dense entries': every column runs the reference's recurrence as if it were alone -- its own
 * scalars, stop test, count, residual and code; a column that has stopped is final and never stored to again; a NaN stays in its
 * column; returns 0 when the loop ran, whatever the columns' verdicts.  Column j's iterate, count, residual and code are the same bits
 * whatever k is, wherever the column stands and whatever the other columns hold, from call to call.  No loop allocates: the M x k
 * block is reserved before it starts.  Every application of K^T.K counts as two products in lcg_hip_last_launches.
 * Refusals after the common ones: k, a null or misaligned M / B, mem (LCG_HIP_E_ARG); a handle without the normal state; then
 * LCG_INVILAD_MAX_ITERATIONS, LCG_INVILAD_EPSILON; then, PCG without the reciprocals, LCG_NULL_PRECONDITION_MATRIX. */
int lcg_hip_csr_normal_lcg_multi(lcg_hip_csr_t K, int k, double *M, const double *B, const lcg_para *param, int *ret, int *iterations, double *residual, int mem);
int lcg_hip_csr_normal_lpcg_multi(lcg_hip_csr_t K, int k, double *M, const double *B, const lcg_para *param, int *ret, int *iterations, double *residual, int mem);

/* lcg_hip_dense_solver_constrained_multi(normal = 1) on a sparse K: batched PG (solver_id other than LCG_SPG) and SPG between the
 * bounds low, hig (N doubles each, shared by the columns).  The contract, the three stated deviations (breakdown, NaN sums, no progress
 * callback), `products` and the codes are lcg_hip_staging_box_multi.h's; the independence of a column from k, its position and its
 * neighbours is as above.  Refusals after the common ones: k, M / B, a null low / hig, mem; a handle without the normal state; then
 * the reference's parameter codes per solver, then maxi_m > 64 (LCG_HIP_E_ARG). */
int lcg_hip_csr_normal_solver_constrained_multi(lcg_hip_csr_t K, int k, int solver_id, double *M, const double *B, const double *low, const double *hig, const lcg_para *param, int *ret, int *iterations, int *products, double *residual, int mem);

#ifdef __cplusplus
}
#endif
#endif /* LCG_HIP_STAGING_CSR_NORMAL_H */
