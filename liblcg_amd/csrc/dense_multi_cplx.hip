// dense_multi_cplx.hip -- complex128 dense operators over k = 2, 4, 8 right-hand sides: K.X, conj(K).X, K^T.X, K^H.X with K read ONCE
// for all k columns, and the operator of the batched complex loops (solvers_multi_cplx.hip: clcg_hip_dense_lbicg_sym_multi,
// clcg_hip_dense_lpcg_multi) with the unconjugated sum they take after it.  One GPU.  DESIGN.md section 20.
//
// Blocks of vectors are multi_cplx.hpp's: column j of row i is the 16-byte piece i * k + j, the base 16-byte aligned.  This unit holds
// the complex entries and their checks.  The kernels and the host flow under them are dense_multi.hip's, shared with the real handles:
// one 16-byte pack per entry (NP = N, the single stored copy), the SAME plans (dense.hpp: functions of the shape and the forced
// variant, never of k):
//
//   k_zdnm_row<K, W, CONJ>  Y(i,:) = sum_j op(K(i,j)) X(j,:)   W lanes per group of zrr(K) = 4 rows; per pack a lane loads one entry of K per row
//                           and row j of X (16 k contiguous bytes) once for its rows; k complex accumulators per row; butterfly
//                           over the W lanes; whole rows of Y.  Columns cut into strips over gridDim.y (k_zdnm_row_split): one slot
//                           of M * 2k doubles per strip
//   k_dnm_col<DnCplx<K, CONJ>, K>  ("k_zdnm_col": the real column form's template with the complex element trait)  Y(j,:) = sum_i
//                           op(K(i,j)) X(i,:)   thread (cp, rg) owns one column and walks a strip of rows, reading the k complex values
//                           X(i,:) per row (one address for all lanes of a row group); k accumulators; the row groups meet in LDS in rg
//                           order; one slot of N * 2k doubles per strip of rows
//   k_dnm_fold              the slots added in its fixed order -- it adds doubles and does not care what they are
//   k_dnm_dot<K, true>      column j's unconjugated sum_i Y_ij U_ij left as <= MM_MG partial sums per component in the table format
//                           cspmm_launch leaves (re: row 2 j, im: row 2 j + 1), one launch over the two N x k blocks: no pass over K
//
// Every complex multiply-add is zfma's pair of explicit fmas per component (the conjugated forms flip signs and nothing else) and every
// sum is added in an order fixed by the shape alone, so column j's bits depend on K, the handle's forced variant and column j of X (and
// U) -- not on k, not on what the other columns hold, not on the call.  No atomics.  Every kernel falls through when the batch has
// stopped (`done`).
#include "dense.hpp"
#include "multi_cplx.hpp"

using namespace lcgh;

extern "C" {

int clcg_hip_dense_matmat(lcg_hip_dense_t K, int k, const double *X, double *Y, int layout, int conjugate)
{
    const char *entry = "clcg_hip_dense_matmat";
    TRY(multi_args(entry, k, X, Y));
    lcg_hip_dense *D = dnm_handle(entry, K, true);
    if (!D) return LCG_HIP_E_ARG;
    if (layout < 0 || layout > 1 || conjugate < 0 || conjugate > 1)
        return arg_error("%s: layout = %d, conjugate = %d (layout 0: K.X, 1: K^T.X; conjugate 0 / 1)", entry, layout, conjugate);
    const size_t nx = (size_t)(layout ? D->M : D->N) * k, ny = (size_t)(layout ? D->N : D->M) * k;
    if (overlap(X, 16 * nx, Y, 16 * ny)) return arg_error("%s: X and Y overlap", entry);
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    int launches = 0;
    return layout ? dnm_col_product(D, k, X, Y, conjugate, ctx().stream, nullptr, &launches)
                  : dnm_row_product(D, k, X, Y, conjugate, D->variant, ctx().stream, nullptr, &launches);
}

int clcg_hip_dense_op_multi_dot(lcg_hip_dense_t K, int k, const double *X, double *Y, const double *U, double *dots)
{
    const char *entry = "clcg_hip_dense_op_multi_dot";
    TRY(multi_args(entry, k, X, Y, U ? (const void *)U : (const void *)16));
    lcg_hip_dense *D = dnm_handle(entry, K, true);
    if (!D) return LCG_HIP_E_ARG;
    if (D->M != D->N) return arg_error("%s: the matrix is %d x %d: the loops' operator needs a square one", entry, D->M, D->N);
    const size_t nv = 16 * (size_t)D->N * k;
    if (overlap(X, nv, Y, nv) || (U && overlap(U, nv, Y, nv))) return arg_error("%s: Y overlaps X or U", entry);
    if (dots && !U) return arg_error("%s: dots without U", entry);
    return dnm_op_dot_run(D, k, 0, X, Y, U, dots);
}

const char *clcg_hip_dense_multi_kernel_name(int index) { return dnm_kernel_name(true, index); }

} // extern "C"
