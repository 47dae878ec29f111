// csr_ilu0.hip -- incomplete LU with zero fill, ILU(0): the preconditioner of sample11.cu (cusparseZcsrilu02 and two
// cusparseZcsrsv2_solve, unit-lower L then U, sample11.cu's cudaMx_ILU as Mfp of CLCG_PCG) and of the Eigen back-end's
// lcg_incomplete_LU / clcg_incomplete_LU (preconditioner_eigen.h:109-119).  No square root: it serves symmetric indefinite
// and non-symmetric matrices, which IC(0) (csr_ic0.hip) refuses or cannot express.  DESIGN 13.
//
// build: all of A's entries, duplicates summed, one explicit zero on every diagonal, rows sorted (extract_rows, csr_tri.hpp).
// One host pass over the downloaded pattern finds every row's diagonal, the level sets of L (forward, from the strictly lower
// pattern) and of U (backward, from U's own pattern: it is not L^T's when A's pattern is not symmetric) and the row pointers
// of the two triangles.  The factor runs on the device in place over the forward schedule (IluFactorRow on the level walker),
// one thread per row in IKJ order: for each k < i of row i, ascending, L(i,k) = w(i,k) / U(k,k), then row k's upper part is
// merged into the rest of row i (both sorted).  Every entry so receives
//     w(i,j) = A(i,j) - sum_{k < min(i,j)} L(i,k).U(k,j)      one accumulator, one product subtracted at a time, k ascending
//     U(i,j) = w(i,j) (j >= i),   L(i,j) = w(i,j) / U(j,j) (j < i),   L(i,i) = 1, not stored
// unconjugated for complex A.  Row i needs the rows k < i of its own pattern final: exactly what L's forward solve needs.
// The combined rows are then split into L (CSR, sorted rows, no diagonal) and U (CSR, sorted rows, diagonal first).
//
// The result is a TriFactor whose lower triangle has a unit diagonal that is not stored; its solves, sweeps and the host
// surface behind the entries below are csr_tri.hip's, shared with IC(0).  U divides once by its diagonal, L does not divide;
// for L the first sweep from y = 0 is y = x, so its second sweep reads x and a k-sweep apply of L is k - 1 launches (one copy
// when k = 1).
#include <cmath>

#include "csr_tri.hpp"

namespace lcgh {

// ------------------------------------------------------------------------------------------ factor
__device__ __forceinline__ bool ilu_pivot_fails(double d) { return d == 0.0 || !isfinite(d); }
__device__ __forceinline__ bool ilu_pivot_fails(double2 d) { return (d.x == 0.0 && d.y == 0.0) || !isfinite(d.x) || !isfinite(d.y); }

// Row i of the combined factor in place (val holds A's row on entry; dg[i] is the position of its diagonal).  Rows k < i of
// its pattern are final (earlier levels); nothing but row i is written.
template <class V>
struct IluFactorRow {
    const int *rowptr, *col, *dg;
    V *val;
    int *zp;
    __device__ __forceinline__ void operator()(int i) const
    {
        const int s = rowptr[i], d = dg[i], e = rowptr[i + 1];
        for (int p = s; p < d; p++) {
            const int k = col[p], dk = dg[k];
            const V l = ic_div(val[p], val[dk]);
            val[p] = l;
            int r = p + 1, q = dk + 1;
            const int qe = rowptr[k + 1];
            while (r < e && q < qe) {
                const int cr = col[r], cq = col[q];
                if (cr == cq) { val[r] = vsub(val[r], ic_mul(l, val[q])); r++; q++; }
                else if (cr < cq) r++;
                else q++;
            }
        }
        if (ilu_pivot_fails(val[d])) atomicMin(zp, i);
    }
};

// the combined rows into L (the entries before the diagonal) and U (the diagonal and what follows)
template <class V>
__global__ void k_ilu_split(int n, const int *rowptr, const int *col, const V *val, const int *dg, const int *rpL, int *colL, V *valL,
                            const int *rpU, int *colU, V *valU)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = rowptr[i], d = dg[i], e = rowptr[i + 1];
    for (int p = s, q = rpL[i]; p < d; p++, q++) { colL[q] = col[p]; valL[q] = val[p]; }
    for (int p = d, q = rpU[i]; p < e; p++, q++) { colU[q] = col[p]; valU[q] = val[p]; }
}

// --------------------------------------------------------------------------------------------- host
constexpr TriSlot ILU0 = &lcg_hip_csr::ilu0;
constexpr const char *ILU0_BUILDER = "lcg_hip_csr_build_ilu0";

template <class V>
static int ilu0_build(lcg_hip_csr *A, TriFactor *F, hipStream_t s)
{
    const int n = A->n_rows;
    CsrPart LU;                                         // the combined rows, factored in place, then split
    int *dg = nullptr;
    auto bail = [&](int rc) { free_part(LU); if (dg) hipFree(dg); return rc; };
    int rc = extract_rows<V, false>(A, LU, F->cplx, s);
    if (rc) return bail(rc);
    const long nnz = LU.nnz;
    std::vector<int> rp((size_t)n + 1), col((size_t)nnz);
    if (hipMemcpy(rp.data(), LU.rowptr, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(col.data(), LU.col, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost) != hipSuccess)
        return bail(fail(hipErrorUnknown, "ilu0 pattern download", __FILE__, __LINE__));
    // one pass over the pattern: the diagonal's position, the two triangles' row pointers, the level sets.  Forward: level(i) =
    // 1 + max level(k) over k < i in row i.  Backward, rows descending: level(i) = 1 + max level(j) over j > i in row i of U.
    std::vector<int> dgh((size_t)n), rpL((size_t)n + 1, 0), rpU((size_t)n + 1, 0), lf((size_t)n, 0), lb((size_t)n, 0);
    int nf = 0, nb = 0;
    for (int i = 0; i < n; i++) {
        int p = rp[(size_t)i], l = 0;
        for (; col[(size_t)p] < i; p++) l = std::max(l, lf[(size_t)col[(size_t)p]] + 1);   // (the diagonal is there: the loop ends on it)
        dgh[(size_t)i] = p;
        rpL[(size_t)i + 1] = rpL[(size_t)i] + (p - rp[(size_t)i]);
        rpU[(size_t)i + 1] = rpU[(size_t)i] + (rp[(size_t)i + 1] - p);
        lf[(size_t)i] = l; nf = std::max(nf, l + 1);
    }
    for (int i = n - 1; i >= 0; i--) {
        int l = 0;
        for (int p = dgh[(size_t)i] + 1; p < rp[(size_t)i + 1]; p++) l = std::max(l, lb[(size_t)col[(size_t)p]] + 1);
        lb[(size_t)i] = l; nb = std::max(nb, l + 1);
    }
    rc = tri_schedule(F, lf, nf, lb, nb); if (rc) return bail(rc);
    if (hipMalloc(&dg, sizeof(int) * (size_t)std::max(n, 1)) != hipSuccess)
        return bail(fail(hipErrorOutOfMemory, "ilu0 diagonal positions", __FILE__, __LINE__));
    if (hipMemcpyAsync(dg, dgh.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess)
        return bail(fail(hipErrorUnknown, "ilu0 diagonal positions", __FILE__, __LINE__));
    // factor in place on the forward schedule
    rc = pivot_arm(F, s); if (rc) return bail(rc);
    rc = run_levels(F->fw, IluFactorRow<V>{LU.rowptr, LU.col, dg, reinterpret_cast<V *>(LU.val), F->zp}, nullptr, s); if (rc) return bail(rc);
    rc = pivot_read(F, s); if (rc) return bail(rc);
    // the two triangles as their own CSR
    rc = alloc_part(F->lo, n, rpL[(size_t)n], F->cplx); if (rc) return bail(rc);
    rc = alloc_part(F->up, n, rpU[(size_t)n], F->cplx); if (rc) return bail(rc);
    F->lo.n_cols = F->up.n_cols = n;
    if (hipMemcpyAsync(F->lo.rowptr, rpL.data(), sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(F->up.rowptr, rpU.data(), sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice, s) != hipSuccess)
        return bail(fail(hipErrorUnknown, "ilu0 row pointers", __FILE__, __LINE__));
    if (n > 0)
        hipLaunchKernelGGL((k_ilu_split<V>), dim3((unsigned)((n + VB - 1) / VB)), dim3(VB), 0, s, n, LU.rowptr, LU.col,
                           reinterpret_cast<const V *>(LU.val), dg, F->lo.rowptr, F->lo.col, reinterpret_cast<V *>(F->lo.val), F->up.rowptr,
                           F->up.col, reinterpret_cast<V *>(F->up.val));
    if (hipGetLastError() != hipSuccess || hipMalloc(&F->tmp, sizeof(V) * (size_t)std::max(n, 1)) != hipSuccess ||
        hipMalloc(&F->w, sizeof(V) * (size_t)std::max(n, 1)) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return bail(fail(hipErrorUnknown, "ilu0 split", __FILE__, __LINE__));
    return bail(0);
}

static int ilu0_call(void *A, bool cplx, int which, const double *x, double *y, long n_size)
{
    return tri_call(static_cast<lcg_hip_csr *>(A), ILU0, "ILU(0)", ILU0_BUILDER, cplx, false, which, x, y, n_size);
}

// y = A.(U^-1 L^-1 x): the apply into the factor's own vector, then the handle's ordinary product
static int ilu0_ax(void *instance, bool cplx, const double *x, double *y, long n_size)
{
    lcg_hip_csr *A = static_cast<lcg_hip_csr *>(instance);
    if (!A || !x || !y) return LCG_HIP_E_ARG;
    const TriFactor *F = nullptr;
    int rc = tri_check(A, ILU0, "ILU(0)", ILU0_BUILDER, cplx, false, n_size, 2, x, nullptr, &F);
    if (rc) return rc;
    rc = tri_apply(F, 2, x, F->w, ctx().stream, ax_flag(ctx()));
    return rc ? rc : lcg_hip_spmv(A, F->w, y);
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_csr_build_ilu0(lcg_hip_csr_t A)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_build_ilu0");
    return tri_build(A, ILU0, "ILU(0)", 2, "zero or not finite", [](lcg_hip_csr *A, TriFactor *F, hipStream_t s) {
        return F->cplx ? ilu0_build<double2>(A, F, s) : ilu0_build<double>(A, F, s);
    });
}

int lcg_hip_csr_ilu0_info(lcg_hip_csr_t A, int *levels_L, int *levels_U, int *launches_per_apply, int *zero_pivot, double *build_ms,
                          int64_t *bytes)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return tri_info(A, ILU0, levels_L, levels_U, launches_per_apply, zero_pivot, build_ms, bytes);
}

int lcg_hip_csr_ilu0_set_sweeps(lcg_hip_csr_t A, int sweeps)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return tri_set_sweeps(A, ILU0, __func__, ILU0_BUILDER, sweeps);
}

int lcg_hip_csr_ilu0_get_sweeps(lcg_hip_csr_t A, int *sweeps)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return tri_get_sweeps(A, ILU0, __func__, ILU0_BUILDER, sweeps);
}

int lcg_hip_csr_ilu0_factor(lcg_hip_csr_t A, int which, const int **rowptr, const int **col, const double **val)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return tri_arrays(A, ILU0, which, rowptr, col, val);
}

int lcg_hip_ilu0_solve(lcg_hip_csr_t A, int which, const double *x, double *y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return LCG_HIP_E_ARG;
    return ilu0_call(A, A->is_complex, which, x, y, -1);
}

int lcg_hip_csr_ilu0_schedule_for_test(lcg_hip_csr_t A, int max_merged_rows)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return tri_schedule_for_test(A, ILU0, max_merged_rows);
}

// The callback types return void (lcg.h:37-38, clcg.h:40-41): a failure is parked in Ctx::ax_rc (park, csr_tri.hip).
void lcg_hip_ilu0_mx(void *instance, const double *x, double *prod_Mx, const int n_size)
{
    NOT_DENSE_CB(instance);
    park(ilu0_call(instance, false, 2, x, prod_Mx, n_size));
}

void clcg_hip_ilu0_mx(void *instance, const double *x, double *prod_Mx, const int n_size, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    park(layout || conjugate ? arg_error("ILU(0): layout = 1 and conjugate = 1 are not offered (M = L.U is not symmetric)")
                             : ilu0_call(instance, true, 2, x, prod_Mx, n_size));
}

void lcg_hip_csr_ax_ilu0(void *instance, const double *x, double *prod_Ax, const int n_size)
{
    NOT_DENSE_CB(instance);
    park(ilu0_ax(instance, false, x, prod_Ax, n_size));
}

void clcg_hip_csr_ax_ilu0(void *instance, const double *x, double *prod_Ax, const int n_size, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    park(layout || conjugate ? arg_error("ILU(0): the right-preconditioned product offers (layout, conjugate) = (0, 0) only")
                             : ilu0_ax(instance, true, x, prod_Ax, n_size));
}

} // extern "C"
