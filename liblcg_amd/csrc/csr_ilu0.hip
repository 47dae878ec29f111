// csr_ilu0.hip -- incomplete LU with zero fill, ILU(0): the preconditioner of sample11.cu (cusparseZcsrilu02 and two
// cusparseZcsrsv2_solve, unit-lower L then U, sample11.cu's cudaMx_ILU as Mfp of CLCG_PCG) and of the Eigen back-end's
// lcg_incomplete_LU / clcg_incomplete_LU (preconditioner_eigen.h:109-119).  No square root: it serves symmetric indefinite
// and non-symmetric matrices, which IC(0) (csr_ic0.hip) refuses or cannot express.  DESIGN 13.
//
// build: all of A's entries, duplicates summed, one explicit zero on every diagonal, rows sorted (extract_rows, csr_tri.hpp).
// One host pass over the downloaded pattern finds every row's diagonal, the level sets of L (forward, from the strictly lower
// pattern) and of U (backward, from U's own pattern: it is not L^T's when A's pattern is not symmetric) and the row pointers
// of the two triangles.  The factor runs on the device in place over the forward schedule, one thread per row in IKJ order:
// for each k < i of row i, ascending, L(i,k) = w(i,k) / U(k,k), then row k's upper part is merged into the rest of row i
// (both sorted).  Every entry so receives
//     w(i,j) = A(i,j) - sum_{k < min(i,j)} L(i,k).U(k,j)      one accumulator, one product subtracted at a time, k ascending
//     U(i,j) = w(i,j) (j >= i),   L(i,j) = w(i,j) / U(j,j) (j < i),   L(i,i) = 1, not stored
// unconjugated for complex A.  Row i needs the rows k < i of its own pattern final: exactly what L's forward solve needs.
// The combined rows are then split into L (CSR, sorted rows, no diagonal) and U (CSR, sorted rows, diagonal first).
//
// solves, schedule, sweeps: as IC(0)'s (csr_ic0.hip) -- wide levels one grid launch, runs of narrow levels one workgroup with a
// barrier between levels; a row is one accumulator from x_i, products subtracted in column order; U divides once by its
// diagonal, L does not divide.  k Jacobi sweeps per triangle on request (k_ic_sweep, csr_tri.hpp); for L the first sweep from
// y = 0 is y = x, so its second sweep reads x and a k-sweep apply of L is k - 1 launches (one copy when k = 1).
#include <chrono>
#include <cmath>

#include "csr_tri.hpp"

namespace lcgh {

struct Ilu0 {
    int n = 0;
    bool cplx = false, ok = false;
    CsrPart L, U;               // L: rows sorted, no diagonal; U: rows sorted, diagonal first
    IcTri fw, bw;
    double *tmp = nullptr;      // L^-1 x of the full apply (n values of the factor's type)
    double *w = nullptr;        // U^-1 L^-1 x of the right-preconditioned product (lcg_hip_csr_ax_ilu0)
    int sweeps = 0;             // 0: exact level-scheduled solves; k >= 1: k Jacobi sweeps per triangle
    double *sw[2] = {nullptr, nullptr};     // the sweeps' two intermediate vectors (n values each, held while sweeps >= 1)
    int *zp = nullptr;          // device: smallest row whose pivot failed (INT_MAX: none)
    int zero_pivot = -1;
    int max_merged = IC_WG;     // widest level a narrow group takes (lcg_hip_csr_ilu0_schedule_for_test)
    double build_ms = 0.0;
};

// ------------------------------------------------------------------------------------------ factor
__device__ __forceinline__ bool ilu_pivot_fails(double d) { return d == 0.0 || !isfinite(d); }
__device__ __forceinline__ bool ilu_pivot_fails(double2 d) { return (d.x == 0.0 && d.y == 0.0) || !isfinite(d.x) || !isfinite(d.y); }

// Row i of the combined factor in place (val holds A's row on entry; dg[i] is the position of its diagonal).  Rows k < i of
// its pattern are final (earlier levels); nothing but row i is written.
template <class V>
__device__ __forceinline__ void ilu_factor_row(int i, const int *rowptr, const int *col, const int *dg, V *val, int *zp)
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
template <class V>
__global__ __launch_bounds__(IC_WB) void k_ilu_factor_wide(const int *ord, int b, int e, const int *rowptr, const int *col, const int *dg,
                                                          V *val, int *zp)
{
    const int pos = b + blockIdx.x * blockDim.x + threadIdx.x;
    if (pos < e) ilu_factor_row(ord[pos], rowptr, col, dg, val, zp);
}
template <class V>
__global__ __launch_bounds__(IC_WG) void k_ilu_factor_narrow(const int *ord, const int *lvl, int l0, int l1, const int *rowptr,
                                                            const int *col, const int *dg, V *val, int *zp)
{
    for (int l = l0; l < l1; l++) {
        for (int pos = lvl[l] + threadIdx.x; pos < lvl[l + 1]; pos += blockDim.x) ilu_factor_row(ord[pos], rowptr, col, dg, val, zp);
        __syncthreads();
    }
}

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

// ------------------------------------------------------------------------------------------- solves
// UP = false: y_i = x_i - sum_k L(i,k) y_k (unit diagonal); true: y_i = (x_i - sum_{k>i} U(i,k) y_k) / U(i,i).  Column order.
template <class V, bool UP>
__device__ __forceinline__ void ilu_solve_row(int i, const int *rowptr, const int *col, const V *val, const V *x, V *y)
{
    const int s = rowptr[i], e = rowptr[i + 1];
    V acc = x[i];
    for (int p = UP ? s + 1 : s; p < e; p++) acc = vsub(acc, ic_mul(val[p], y[col[p]]));
    y[i] = UP ? ic_div(acc, val[s]) : acc;
}
template <class V, bool UP>
__global__ __launch_bounds__(IC_WB) void k_ilu_solve_wide(const int *ord, int b, int e, const int *rowptr, const int *col, const V *val,
                                                         const V *x, V *y, const int *done)
{
    if (done && *done) return;
    const int pos = b + blockIdx.x * blockDim.x + threadIdx.x;
    if (pos < e) ilu_solve_row<V, UP>(ord[pos], rowptr, col, val, x, y);
}
template <class V, bool UP>
__global__ __launch_bounds__(IC_WG) void k_ilu_solve_narrow(const int *ord, const int *lvl, int l0, int l1, const int *rowptr,
                                                           const int *col, const V *val, const V *x, V *y, const int *done)
{
    if (done && *done) return;
    for (int l = l0; l < l1; l++) {
        for (int pos = lvl[l] + threadIdx.x; pos < lvl[l + 1]; pos += blockDim.x) ilu_solve_row<V, UP>(ord[pos], rowptr, col, val, x, y);
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------------- host
static void ilu0_release(Ilu0 *F)
{
    free_part(F->L); free_part(F->U);
    tri_free(F->fw); tri_free(F->bw);
    if (F->tmp) hipFree(F->tmp);
    if (F->w) hipFree(F->w);
    for (double *&p : F->sw) if (p) hipFree(p);
    if (F->zp) hipFree(F->zp);
    delete F;
}

template <class V, bool UP>
static int ilu_solve(const Ilu0 *F, const double *x, double *y, hipStream_t s, const int *done)
{
    const IcTri &t = UP ? F->bw : F->fw;
    const CsrPart &T = UP ? F->U : F->L;
    const V *xv = reinterpret_cast<const V *>(x), *val = reinterpret_cast<const V *>(T.val);
    V *yv = reinterpret_cast<V *>(y);
    for (const IcSeg &g : t.segs) {
        if (g.narrow)
            hipLaunchKernelGGL((k_ilu_solve_narrow<V, UP>), dim3(1), dim3(IC_WG), 0, s, t.ord, t.lvl, g.l0, g.l1, T.rowptr, T.col, val,
                               xv, yv, done);
        else {
            const int b = t.lvl_h[(size_t)g.l0], e = t.lvl_h[(size_t)g.l1];
            hipLaunchKernelGGL((k_ilu_solve_wide<V, UP>), dim3((unsigned)((e - b + IC_WB - 1) / IC_WB)), dim3(IC_WB), 0, s, t.ord, b, e,
                               T.rowptr, T.col, val, xv, yv, done);
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// launches of a k-sweep apply of one triangle: U scales and sweeps k - 1 times; L's first sweep is y = x, which its second reads
// in place of a vector of its own (k = 1: one copy)
static int ilu_sweep_launches(bool up, int k) { return up ? k : std::max(k - 1, 1); }

template <class V, bool UP>
static int ilu_sweeps(const Ilu0 *F, const double *x, double *y, hipStream_t s, const int *done)
{
    constexpr int DG = UP ? 1 : 2;
    const CsrPart &T = UP ? F->U : F->L;
    const V *xv = reinterpret_cast<const V *>(x), *val = reinterpret_cast<const V *>(T.val);
    V *const buf[2] = {reinterpret_cast<V *>(F->sw[0]), reinterpret_cast<V *>(F->sw[1])};
    V *yv = reinterpret_cast<V *>(y);
    const int k = F->sweeps;
    const dim3 grid((unsigned)((F->n + IC_SR - 1) / IC_SR));
    if (F->n == 0) return 0;
    const V *in = xv;                                   // L: y(1) = x itself
    if (UP || k == 1) {
        V *out = k == 1 ? yv : buf[0];
        hipLaunchKernelGGL((k_ic_scale<V, DG>), grid, dim3(IC_SR), 0, s, F->n, T.rowptr, val, xv, out, done);
        in = out;
    }
    for (int j = 2; j <= k; j++) {
        V *out = j == k ? yv : buf[in == buf[0] ? 1 : 0];
        hipLaunchKernelGGL((k_ic_sweep<V, DG>), grid, dim3(IC_SR), 0, s, F->n, T.rowptr, T.col, val, xv, in, out, done);
        in = out;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

template <class V, bool UP>
static int ilu_tri_apply(const Ilu0 *F, const double *x, double *y, hipStream_t s, const int *done)
{
    return F->sweeps > 0 ? ilu_sweeps<V, UP>(F, x, y, s, done) : ilu_solve<V, UP>(F, x, y, s, done);
}

template <class V>
static int ilu0_apply(const Ilu0 *F, int which, const double *x, double *y, hipStream_t s, const int *done)
{
    if (which == 0) return ilu_tri_apply<V, false>(F, x, y, s, done);
    if (which == 1) return ilu_tri_apply<V, true>(F, x, y, s, done);
    int rc = ilu_tri_apply<V, false>(F, x, F->tmp, s, done);
    return rc ? rc : ilu_tri_apply<V, true>(F, F->tmp, y, s, done);
}

template <class V>
static int factor_launch(const Ilu0 *F, const CsrPart &LU, const int *dg, hipStream_t s)
{
    const IcTri &t = F->fw;
    V *val = reinterpret_cast<V *>(LU.val);
    for (const IcSeg &g : t.segs) {
        if (g.narrow)
            hipLaunchKernelGGL((k_ilu_factor_narrow<V>), dim3(1), dim3(IC_WG), 0, s, t.ord, t.lvl, g.l0, g.l1, LU.rowptr, LU.col, dg, val, F->zp);
        else {
            const int b = t.lvl_h[(size_t)g.l0], e = t.lvl_h[(size_t)g.l1];
            hipLaunchKernelGGL((k_ilu_factor_wide<V>), dim3((unsigned)((e - b + IC_WB - 1) / IC_WB)), dim3(IC_WB), 0, s, t.ord, b, e,
                               LU.rowptr, LU.col, dg, val, F->zp);
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

template <class V>
static int ilu0_build(lcg_hip_csr *A, Ilu0 *F, hipStream_t s)
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
    rc = tri_levels(F->fw, lf, nf); if (rc) return bail(rc);
    rc = tri_levels(F->bw, lb, nb); if (rc) return bail(rc);
    tri_segments(F->fw, F->max_merged);
    tri_segments(F->bw, F->max_merged);
    const int big = 0x7fffffff;
    if (hipMalloc(&dg, sizeof(int) * (size_t)std::max(n, 1)) != hipSuccess || hipMalloc(&F->zp, sizeof(int)) != hipSuccess)
        return bail(fail(hipErrorOutOfMemory, "ilu0 diagonal positions", __FILE__, __LINE__));
    if (hipMemcpyAsync(dg, dgh.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(F->zp, &big, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess)
        return bail(fail(hipErrorUnknown, "ilu0 diagonal positions", __FILE__, __LINE__));
    // factor in place on the forward schedule
    rc = factor_launch<V>(F, LU, dg, s); if (rc) return bail(rc);
    int zp = big;
    if (hipMemcpyAsync(&zp, F->zp, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return bail(fail(hipErrorUnknown, "ilu0 factor", __FILE__, __LINE__));
    F->zero_pivot = zp == big ? -1 : zp;
    // the two triangles as their own CSR
    rc = alloc_part(F->L, n, rpL[(size_t)n], F->cplx); if (rc) return bail(rc);
    rc = alloc_part(F->U, n, rpU[(size_t)n], F->cplx); if (rc) return bail(rc);
    F->L.n_cols = F->U.n_cols = n;
    if (hipMemcpyAsync(F->L.rowptr, rpL.data(), sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(F->U.rowptr, rpU.data(), sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice, s) != hipSuccess)
        return bail(fail(hipErrorUnknown, "ilu0 row pointers", __FILE__, __LINE__));
    if (n > 0)
        hipLaunchKernelGGL((k_ilu_split<V>), dim3((unsigned)((n + VB - 1) / VB)), dim3(VB), 0, s, n, LU.rowptr, LU.col,
                           reinterpret_cast<const V *>(LU.val), dg, F->L.rowptr, F->L.col, reinterpret_cast<V *>(F->L.val), F->U.rowptr,
                           F->U.col, reinterpret_cast<V *>(F->U.val));
    if (hipGetLastError() != hipSuccess || hipMalloc(&F->tmp, sizeof(V) * (size_t)std::max(n, 1)) != hipSuccess ||
        hipMalloc(&F->w, sizeof(V) * (size_t)std::max(n, 1)) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return bail(fail(hipErrorUnknown, "ilu0 split", __FILE__, __LINE__));
    return bail(0);
}

static Ilu0 *ilu0_of(const lcg_hip_csr *A) { return static_cast<Ilu0 *>(A->ilu0); }

void ilu0_free(lcg_hip_csr *A)
{
    if (A->ilu0) ilu0_release(ilu0_of(A));
    A->ilu0 = nullptr;
}

static int arg_error(const char *fmt, long v = 0)
{
    char buf[256];
    std::snprintf(buf, sizeof buf, fmt, v);
    ctx().err = buf;
    return LCG_HIP_E_ARG;
}

// the checks every apply makes (callbacks and solve entries): 0 and *out = the factor, or LCG_HIP_E_ARG with the reason
static int ilu0_check(lcg_hip_csr *A, bool cplx, long n_size, const Ilu0 **out)
{
    if (!A) return arg_error("ILU(0): the handle is NULL");
    TRY_C64(A, "ILU(0) apply");
    const Ilu0 *F = ilu0_of(A);
    if (!F || !F->ok) return arg_error("ILU(0): the handle has no factor (lcg_hip_csr_build_ilu0)");
    if (F->cplx != cplx) return arg_error(cplx ? "ILU(0): complex callback on a real factor" : "ILU(0): real callback on a complex factor");
    if (n_size >= 0 && n_size != F->n) return arg_error("ILU(0): n_size differs from the factor's %ld rows", F->n);
    *out = F;
    return 0;
}

// the apply behind the callbacks and the solve entry: checks, then the triangular solves (or sweeps) on the library's stream
static int ilu0_call(lcg_hip_csr *A, bool cplx, int which, const double *x, double *y, long n_size)
{
    if (!A || !x || !y) return LCG_HIP_E_ARG;
    const Ilu0 *F = nullptr;
    const int rc = ilu0_check(A, cplx, n_size, &F);
    if (rc) return rc;
    if (which < 0 || which > 2) return arg_error("ILU(0): which = %ld (0, 1 or 2)", which);
    const size_t bytes = sizeof(double) * (cplx ? 2 : 1) * (size_t)F->n;
    if ((const char *)x < (const char *)y + bytes && (const char *)y < (const char *)x + bytes)
        return arg_error("ILU(0): x and y overlap");
    Ctx &c = ctx();
    return cplx ? ilu0_apply<double2>(F, which, x, y, c.stream, ax_flag(c)) : ilu0_apply<double>(F, which, x, y, c.stream, ax_flag(c));
}

// y = A.(U^-1 L^-1 x): the apply into the factor's own vector, then the handle's ordinary product
static int ilu0_ax(lcg_hip_csr *A, bool cplx, const double *x, double *y, long n_size)
{
    if (!A || !x || !y) return LCG_HIP_E_ARG;
    const Ilu0 *F = nullptr;
    int rc = ilu0_check(A, cplx, n_size, &F);
    if (rc) return rc;
    Ctx &c = ctx();
    rc = cplx ? ilu0_apply<double2>(F, 2, x, F->w, c.stream, ax_flag(c)) : ilu0_apply<double>(F, 2, x, F->w, c.stream, ax_flag(c));
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
    if (A->distributed) return arg_error("ILU(0): not available on a sharded matrix");
    if (A->n_cols != A->n_rows) return arg_error("ILU(0): the matrix is not square");
    int rc = ensure_init(); if (rc) return rc;
    Ctx &c = ctx();
    const auto t0 = std::chrono::steady_clock::now();
    int max_merged = IC_WG;
    if (A->ilu0) { max_merged = ilu0_of(A)->max_merged; ilu0_free(A); }
    Ilu0 *F = new Ilu0();
    F->n = A->n_rows; F->cplx = A->is_complex; F->max_merged = max_merged;
    A->ilu0 = F;
    rc = F->cplx ? ilu0_build<double2>(A, F, c.stream) : ilu0_build<double>(A, F, c.stream);
    F->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc) { ilu0_free(A); return rc; }
    if (F->zero_pivot >= 0) return arg_error("ILU(0): the pivot of row %ld is not usable (zero or not finite)", F->zero_pivot);
    F->ok = true;
    return 0;
}

int lcg_hip_csr_ilu0_info(lcg_hip_csr_t A, int *levels_L, int *levels_U, int *launches_per_apply, int *zero_pivot, double *build_ms,
                          int64_t *bytes)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || !A->ilu0) return LCG_HIP_E_ARG;
    const Ilu0 *F = ilu0_of(A);
    if (levels_L) *levels_L = F->fw.levels;
    if (levels_U) *levels_U = F->bw.levels;
    if (launches_per_apply)
        *launches_per_apply = F->sweeps > 0 ? ilu_sweep_launches(false, F->sweeps) + ilu_sweep_launches(true, F->sweeps)
                                            : (int)(F->fw.segs.size() + F->bw.segs.size());
    if (zero_pivot) *zero_pivot = F->zero_pivot;
    if (build_ms) *build_ms = F->build_ms;
    if (bytes) {
        const int64_t vw = F->cplx ? 16 : 8;
        *bytes = 2 * 4 * ((int64_t)F->n + 1) + (4 + vw) * ((int64_t)F->L.nnz + (int64_t)F->U.nnz)      // L and U
               + 2 * 4 * (int64_t)F->n + 4 * ((int64_t)F->fw.levels + F->bw.levels + 2)               // level orders
               + 2 * vw * F->n + 4;                                                                   // two work vectors, pivot word
        if (F->sweeps > 0) *bytes += 2 * vw * F->n;                                                   // the sweeps' two intermediate vectors
    }
    return 0;
}

int lcg_hip_csr_ilu0_set_sweeps(lcg_hip_csr_t A, int sweeps)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return arg_error("lcg_hip_csr_ilu0_set_sweeps: the handle is NULL");
    Ilu0 *F = ilu0_of(A);
    if (!F || !F->ok) return arg_error("lcg_hip_csr_ilu0_set_sweeps: the handle has no factor (lcg_hip_csr_build_ilu0)");
    if (sweeps < 0) return arg_error("lcg_hip_csr_ilu0_set_sweeps: sweeps = %ld (0: the exact solves, k >= 1: k sweeps per triangle)", sweeps);
    if (sweeps > 0 && !F->sw[0]) {
        const size_t bytes = sizeof(double) * (F->cplx ? 2 : 1) * (size_t)std::max(F->n, 1);
        for (double *&p : F->sw) {
            if (hipMalloc(&p, bytes) == hipSuccess) continue;
            for (double *&q : F->sw) { if (q) hipFree(q); q = nullptr; }
            return fail(hipErrorOutOfMemory, "ilu0 sweep vectors", __FILE__, __LINE__);
        }
    }
    if (sweeps == 0)                            // (hipFree waits for the applies still on the stream)
        for (double *&p : F->sw) { if (p) hipFree(p); p = nullptr; }
    F->sweeps = sweeps;
    return 0;
}

int lcg_hip_csr_ilu0_get_sweeps(lcg_hip_csr_t A, int *sweeps)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return arg_error("lcg_hip_csr_ilu0_get_sweeps: the handle is NULL");
    const Ilu0 *F = ilu0_of(A);
    if (!F || !F->ok) return arg_error("lcg_hip_csr_ilu0_get_sweeps: the handle has no factor (lcg_hip_csr_build_ilu0)");
    if (!sweeps) return arg_error("lcg_hip_csr_ilu0_get_sweeps: sweeps is NULL");
    *sweeps = F->sweeps;
    return 0;
}

int lcg_hip_csr_ilu0_factor(lcg_hip_csr_t A, int which, const int **rowptr, const int **col, const double **val)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || !A->ilu0 || which < 0 || which > 1) return LCG_HIP_E_ARG;
    const CsrPart &T = which ? ilu0_of(A)->U : ilu0_of(A)->L;
    if (!T.rowptr) return LCG_HIP_E_ARG;
    if (rowptr) *rowptr = T.rowptr;
    if (col) *col = T.col;
    if (val) *val = T.val;
    return 0;
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
    if (!A || !A->ilu0 || max_merged_rows < -1 || max_merged_rows > IC_WG) return LCG_HIP_E_ARG;
    Ilu0 *F = ilu0_of(A);
    F->max_merged = max_merged_rows < 0 ? IC_WG : max_merged_rows;
    tri_segments(F->fw, F->max_merged);
    tri_segments(F->bw, F->max_merged);
    return 0;
}

// The callback types return void (lcg.h:37-38, clcg.h:40-41): a failure is parked in Ctx::ax_rc (driver.hpp: checked_mx).
static void ilu_park(int rc) { if (rc && !ctx().ax_rc) ctx().ax_rc = rc; }

void lcg_hip_ilu0_mx(void *instance, const double *x, double *prod_Mx, const int n_size)
{
    NOT_DENSE_CB(instance);
    ilu_park(ilu0_call(static_cast<lcg_hip_csr *>(instance), false, 2, x, prod_Mx, n_size));
}

void clcg_hip_ilu0_mx(void *instance, const double *x, double *prod_Mx, const int n_size, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    ilu_park(layout || conjugate ? arg_error("ILU(0): layout = 1 and conjugate = 1 are not offered (M = L.U is not symmetric)")
                                 : ilu0_call(static_cast<lcg_hip_csr *>(instance), true, 2, x, prod_Mx, n_size));
}

void lcg_hip_csr_ax_ilu0(void *instance, const double *x, double *prod_Ax, const int n_size)
{
    NOT_DENSE_CB(instance);
    ilu_park(ilu0_ax(static_cast<lcg_hip_csr *>(instance), false, x, prod_Ax, n_size));
}

void clcg_hip_csr_ax_ilu0(void *instance, const double *x, double *prod_Ax, const int n_size, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    ilu_park(layout || conjugate ? arg_error("ILU(0): the right-preconditioned product offers (layout, conjugate) = (0, 0) only")
                                 : ilu0_ax(static_cast<lcg_hip_csr *>(instance), true, x, prod_Ax, n_size));
}

} // extern "C"
