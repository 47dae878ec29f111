// csr_ic0.hip -- incomplete Cholesky IC(0) with zero fill: the preconditioner of sample8.cu's PCG leg (csric02 + two csrsv2
// solves, sample8.cu:105-119,183-238) and of the complex samples' L.L^T (unconjugated, principal square root:
// clcg_incomplete_Cholesky_cuda_full, preconditioner_cuda.cu:207-259).  DESIGN 11.
//
// build: the lower triangle of A (diagonal included, duplicates summed, upper triangle ignored) is extracted on the device
// (count, scan, fill, row sort, then a second count / scan / fill that sums duplicate columns), the level sets of L (forward)
// and L^T (backward) are found by one host pass over the downloaded pattern, and the rows are listed level by level.  The
// factor itself runs on the device over the forward schedule: row i needs exactly the rows its forward solve needs.  L^T is
// then made by the transpose path of op(A) (k_tr_count / k_tr_fill / k_row_sort).
//
// schedule: a level wider than one workgroup is one grid launch; a run of consecutive levels that each fit in one workgroup is
// ONE launch of one workgroup that walks those levels with a barrier between them (workgroup-scope visibility only: no flag,
// no wait on another workgroup).  Every row is computed by one thread in one fixed order -- s = x_i, minus L(i,k).y_k in
// column order, divided by L(i,i) -- so results are the same bits from call to call and under every grouping of the levels.
//
// value types: double (real), double2 (complex128) and float2 (complex64: clcg_incomplete_Cholesky_cuda_half's cuComplex
// overload, preconditioner_cuda.cu, and the two cusparseSpSV solves with CUDA_C_32F of sample14.cu).  The complex64 factor and
// solves are fp32 throughout: products by c64_mul, quotients by c64_div (cuCdivf's scaled formula, c64common.hpp), the
// principal root by csqrt_principal_f, in the same order of operations as the other two types.  Its values are 8 bytes, so
// the build moves them with the real type's helpers as opaque 8-byte words (alloc_part / row_sort_launch / transpose_launch with
// cplx = false).  k_row_sort breaks ties between duplicate (row, column) entries on those words: duplicates are summed in a
// fixed order unless an imaginary part is Inf / NaN.  (L^T has no duplicate columns.)
//
// sweeps (lcg_hip_csr_ic0_set_sweeps, k >= 1): a triangle T = D + N is not solved but approximated by k Jacobi sweeps
// y <- D^-1 (x - N.y) from y = 0: the first is y = x / diag (k_ic_scale), each later one a sparse triangular product over ALL
// rows at once (k_ic_sweep: no level, no dependency between rows, one launch).  A sweep reads one vector and writes another,
// so its result does not depend on which row runs first; a row is summed exactly as ic_solve_row sums it, so a row whose
// inputs are final has the exact solve's bits, and after `levels` sweeps every row has.  2k launches per full apply.
#include <chrono>
#include <cmath>
#include <numeric>

#include "csr_tri.hpp"

namespace lcgh {

struct Ic0 {
    int n = 0;
    bool cplx = false, ok = false;
    bool c64 = false;           // complex64 values (8 bytes: cplx stays false, so the build moves them as real words)
    CsrPart L, LT;              // L: rows sorted, diagonal last; L^T: rows sorted, diagonal first
    IcTri fw, bw;
    double *tmp = nullptr;      // L^-1 x of the full apply (n values of the factor's type)
    int sweeps = 0;             // 0: exact level-scheduled solves; k >= 1: k Jacobi sweeps per triangle
    double *sw[2] = {nullptr, nullptr};     // the sweeps' two intermediate vectors (n values each, held while sweeps >= 1)
    int *zp = nullptr;          // device: smallest row whose pivot failed (INT_MAX: none)
    int zero_pivot = -1;
    int max_merged = IC_WG;     // widest level a narrow group takes (lcg_hip_csr_ic0_schedule_for_test)
    double build_ms = 0.0;
};


// ------------------------------------------------------------------------------------------ factor
__device__ __forceinline__ double2 csqrt_principal(double2 z)
{
    if (z.x == 0.0 && z.y == 0.0) return make_double2(0.0, z.y);
    const double r = hypot(z.x, z.y);
    if (z.x >= 0.0) {
        const double t = sqrt(0.5 * (r + z.x));
        return make_double2(t, z.y / (2.0 * t));
    }
    const double t = sqrt(0.5 * (r - z.x));
    return make_double2(fabs(z.y) / (2.0 * t), copysign(t, z.y));
}
__device__ __forceinline__ float2 csqrt_principal_f(float2 z)     // the same branches in fp32 (std::sqrt(std::complex<float>))
{
    if (z.x == 0.0f && z.y == 0.0f) return make_float2(0.0f, z.y);
    const float r = hypotf(z.x, z.y);
    if (z.x >= 0.0f) {
        const float t = sqrtf(0.5f * (r + z.x));
        return make_float2(t, z.y / (2.0f * t));
    }
    const float t = sqrtf(0.5f * (r - z.x));
    return make_float2(fabsf(z.y) / (2.0f * t), copysignf(t, z.y));
}
__device__ __forceinline__ double ic_sqrt(double d) { return sqrt(d); }
__device__ __forceinline__ double2 ic_sqrt(double2 d) { return csqrt_principal(d); }
__device__ __forceinline__ float2 ic_sqrt(float2 d) { return csqrt_principal_f(d); }
__device__ __forceinline__ bool pivot_fails(double d) { return !(d > 0.0) || !isfinite(d); }
__device__ __forceinline__ bool pivot_fails(double2 d) { return (d.x == 0.0 && d.y == 0.0) || !isfinite(d.x) || !isfinite(d.y); }
__device__ __forceinline__ bool pivot_fails(float2 d) { return (d.x == 0.0f && d.y == 0.0f) || !isfinite(d.x) || !isfinite(d.y); }

// Row i of L in place (val holds A's lower triangle on entry).  L(i,j) = (A(i,j) - sum_{k<j} L(i,k) L(j,k)) / L(j,j) by a sorted
// merge of row i's prefix with row j, then L(i,i) = sqrt(A(i,i) - sum_k L(i,k)^2).  Rows j < i are final (earlier levels).
template <class V>
__device__ __forceinline__ void ic_factor_row(int i, const int *rowptr, const int *col, V *val, int *zp)
{
    const int s = rowptr[i], e = rowptr[i + 1] - 1;     // e: the diagonal
    for (int p = s; p < e; p++) {
        const int j = col[p];
        V v = val[p];
        int r = s, q = rowptr[j];
        const int qe = rowptr[j + 1] - 1;
        while (r < p && q < qe) {
            const int cr = col[r], cq = col[q];
            if (cr == cq) { v = vsub(v, ic_mul(val[r], val[q])); r++; q++; }
            else if (cr < cq) r++;
            else q++;
        }
        val[p] = ic_div(v, val[qe]);
    }
    V d = val[e];
    for (int p = s; p < e; p++) d = vsub(d, ic_mul(val[p], val[p]));
    if (pivot_fails(d)) atomicMin(zp, i);
    val[e] = ic_sqrt(d);
}
template <class V>
__global__ __launch_bounds__(IC_WB) void k_ic_factor_wide(const int *ord, int b, int e, const int *rowptr, const int *col, V *val, int *zp)
{
    const int pos = b + blockIdx.x * blockDim.x + threadIdx.x;
    if (pos < e) ic_factor_row(ord[pos], rowptr, col, val, zp);
}
template <class V>
__global__ __launch_bounds__(IC_WG) void k_ic_factor_narrow(const int *ord, const int *lvl, int l0, int l1, const int *rowptr,
                                                           const int *col, V *val, int *zp)
{
    for (int l = l0; l < l1; l++) {
        for (int pos = lvl[l] + threadIdx.x; pos < lvl[l + 1]; pos += blockDim.x) ic_factor_row(ord[pos], rowptr, col, val, zp);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------- solves
// y_i = (x_i - sum_k T(i,k) y_k) / T(i,i), the sum in column order.  UP = false: T = L (diagonal last), true: T = L^T (first).
template <class V, bool UP>
__device__ __forceinline__ void ic_solve_row(int i, const int *rowptr, const int *col, const V *val, const V *x, V *y)
{
    const int s = rowptr[i], e = rowptr[i + 1];
    const int b = UP ? s + 1 : s, f = UP ? e : e - 1;
    V acc = x[i];
    for (int p = b; p < f; p++) acc = vsub(acc, ic_mul(val[p], y[col[p]]));
    y[i] = ic_div(acc, val[UP ? s : e - 1]);
}
template <class V, bool UP>
__global__ __launch_bounds__(IC_WB) void k_ic_solve_wide(const int *ord, int b, int e, const int *rowptr, const int *col, const V *val,
                                                        const V *x, V *y, const int *done)
{
    if (done && *done) return;
    const int pos = b + blockIdx.x * blockDim.x + threadIdx.x;
    if (pos < e) ic_solve_row<V, UP>(ord[pos], rowptr, col, val, x, y);
}
template <class V, bool UP>
__global__ __launch_bounds__(IC_WG) void k_ic_solve_narrow(const int *ord, const int *lvl, int l0, int l1, const int *rowptr,
                                                          const int *col, const V *val, const V *x, V *y, const int *done)
{
    if (done && *done) return;
    for (int l = l0; l < l1; l++) {
        for (int pos = lvl[l] + threadIdx.x; pos < lvl[l + 1]; pos += blockDim.x) ic_solve_row<V, UP>(ord[pos], rowptr, col, val, x, y);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------- sweeps
// k_ic_scale and k_ic_sweep (csr_tri.hpp, shared with ILU(0)): DG = UP, the diagonal last (L) or first (L^T).

// --------------------------------------------------------------------------------------------- host
static void ic0_release(Ic0 *F)
{
    free_part(F->L); free_part(F->LT);
    tri_free(F->fw); tri_free(F->bw);
    if (F->tmp) hipFree(F->tmp);
    for (double *&p : F->sw) if (p) hipFree(p);
    if (F->zp) hipFree(F->zp);
    delete F;
}


template <class V>
static int factor_launch(Ic0 *F, hipStream_t s)
{
    const IcTri &t = F->fw;
    V *val = reinterpret_cast<V *>(F->L.val);
    for (const IcSeg &g : t.segs) {
        if (g.narrow)
            hipLaunchKernelGGL((k_ic_factor_narrow<V>), dim3(1), dim3(IC_WG), 0, s, t.ord, t.lvl, g.l0, g.l1, F->L.rowptr, F->L.col, val, F->zp);
        else {
            const int b = t.lvl_h[(size_t)g.l0], e = t.lvl_h[(size_t)g.l1];
            hipLaunchKernelGGL((k_ic_factor_wide<V>), dim3((unsigned)((e - b + IC_WB - 1) / IC_WB)), dim3(IC_WB), 0, s, t.ord, b, e,
                               F->L.rowptr, F->L.col, val, F->zp);
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

template <class V, bool UP>
static int tri_solve(const Ic0 *F, const double *x, double *y, hipStream_t s, const int *done)
{
    const IcTri &t = UP ? F->bw : F->fw;
    const CsrPart &T = UP ? F->LT : F->L;
    const V *xv = reinterpret_cast<const V *>(x), *val = reinterpret_cast<const V *>(T.val);
    V *yv = reinterpret_cast<V *>(y);
    for (const IcSeg &g : t.segs) {
        if (g.narrow)
            hipLaunchKernelGGL((k_ic_solve_narrow<V, UP>), dim3(1), dim3(IC_WG), 0, s, t.ord, t.lvl, g.l0, g.l1, T.rowptr, T.col, val,
                               xv, yv, done);
        else {
            const int b = t.lvl_h[(size_t)g.l0], e = t.lvl_h[(size_t)g.l1];
            hipLaunchKernelGGL((k_ic_solve_wide<V, UP>), dim3((unsigned)((e - b + IC_WB - 1) / IC_WB)), dim3(IC_WB), 0, s, t.ord, b, e,
                               T.rowptr, T.col, val, xv, yv, done);
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// k sweeps on one triangle: y(1) = x / diag, then y(j+1) from y(j) between the two intermediate vectors; the last one writes y
template <class V, bool UP>
static int tri_sweeps(const Ic0 *F, const double *x, double *y, hipStream_t s, const int *done)
{
    const CsrPart &T = UP ? F->LT : F->L;
    const V *xv = reinterpret_cast<const V *>(x), *val = reinterpret_cast<const V *>(T.val);
    V *const buf[2] = {reinterpret_cast<V *>(F->sw[0]), reinterpret_cast<V *>(F->sw[1])};
    V *yv = reinterpret_cast<V *>(y);
    const int k = F->sweeps;
    const dim3 grid((unsigned)((F->n + IC_SR - 1) / IC_SR));
    if (F->n == 0) return 0;
    hipLaunchKernelGGL((k_ic_scale<V, UP>), grid, dim3(IC_SR), 0, s, F->n, T.rowptr, val, xv, k == 1 ? yv : buf[0], done);
    for (int j = 2, cur = 0; j <= k; j++, cur ^= 1)
        hipLaunchKernelGGL((k_ic_sweep<V, UP>), grid, dim3(IC_SR), 0, s, F->n, T.rowptr, T.col, val, xv, buf[cur], j == k ? yv : buf[cur ^ 1],
                           done);
    HIPCHK(hipGetLastError());
    return 0;
}

template <class V, bool UP>
static int tri_apply(const Ic0 *F, const double *x, double *y, hipStream_t s, const int *done)
{
    return F->sweeps > 0 ? tri_sweeps<V, UP>(F, x, y, s, done) : tri_solve<V, UP>(F, x, y, s, done);
}

template <class V>
static int ic0_apply(const Ic0 *F, int which, const double *x, double *y, hipStream_t s, const int *done)
{
    if (which == 0) return tri_apply<V, false>(F, x, y, s, done);
    if (which == 1) return tri_apply<V, true>(F, x, y, s, done);
    int rc = tri_apply<V, false>(F, x, F->tmp, s, done);
    return rc ? rc : tri_apply<V, true>(F, F->tmp, y, s, done);
}

// lower triangle of A, duplicates summed, one diagonal per row: into F->L (sorted rows) -- csr_tri.hpp
template <class V>
static int extract_lower(const lcg_hip_csr *A, Ic0 *F, hipStream_t s) { return extract_rows<V, true>(A, F->L, F->cplx, s); }

template <class V>
static int ic0_build(lcg_hip_csr *A, Ic0 *F, hipStream_t s)
{
    const int n = A->n_rows;
    int rc = extract_lower<V>(A, F, s);
    if (rc) return rc;
    // level sets from the pattern: forward level(i) = 1 + max over j < i in row i; backward over L^T, in reverse row order
    const long nnz = F->L.nnz;
    std::vector<int> rp((size_t)n + 1), col((size_t)nnz);
    HIPCHK(hipMemcpy(rp.data(), F->L.rowptr, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(col.data(), F->L.col, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost));
    std::vector<int> lf((size_t)n, 0), lb((size_t)n, 0);
    int nf = 0, nb = 0;
    for (int i = 0; i < n; i++) {
        int l = 0;
        for (int p = rp[(size_t)i]; p < rp[(size_t)i + 1] - 1; p++) l = std::max(l, lf[(size_t)col[(size_t)p]] + 1);
        lf[(size_t)i] = l; nf = std::max(nf, l + 1);
    }
    for (int i = n - 1; i >= 0; i--) {
        const int l = lb[(size_t)i];
        nb = std::max(nb, l + 1);
        for (int p = rp[(size_t)i]; p < rp[(size_t)i + 1] - 1; p++) { int &o = lb[(size_t)col[(size_t)p]]; o = std::max(o, l + 1); }
    }
    rc = tri_levels(F->fw, lf, nf); if (rc) return rc;
    rc = tri_levels(F->bw, lb, nb); if (rc) return rc;
    tri_segments(F->fw, F->max_merged);
    tri_segments(F->bw, F->max_merged);
    // factor in place on the forward schedule
    const int big = 0x7fffffff;
    HIPCHK(hipMalloc(&F->zp, sizeof(int)));
    HIPCHK(hipMemcpyAsync(F->zp, &big, sizeof(int), hipMemcpyHostToDevice, s));
    rc = factor_launch<V>(F, s); if (rc) return rc;
    int zp = big;
    HIPCHK(hipMemcpyAsync(&zp, F->zp, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    F->zero_pivot = zp == big ? -1 : zp;
    // L^T by the transpose path of op(A)
    rc = alloc_part(F->LT, n, nnz, F->cplx); if (rc) return rc;
    F->LT.n_cols = n;
    int *cnt = nullptr;
    HIPCHK(hipMalloc(&cnt, sizeof(int) * (size_t)n));
    rc = transpose_launch(n, n, nnz, F->L.rowptr, F->L.col, F->L.val, F->LT.rowptr, F->LT.col, F->LT.val, F->cplx, 0, cnt, s);
    hipFree(cnt);
    if (rc) return rc;
    HIPCHK(hipMalloc(&F->tmp, sizeof(V) * (size_t)n));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

static Ic0 *ic0_of(const lcg_hip_csr *A) { return static_cast<Ic0 *>(A->ic0); }

void ic0_free(lcg_hip_csr *A)
{
    if (A->ic0) ic0_release(ic0_of(A));
    A->ic0 = nullptr;
}

static int arg_error(const char *fmt, long v = 0)
{
    char buf[256];
    std::snprintf(buf, sizeof buf, fmt, v);
    ctx().err = buf;
    return LCG_HIP_E_ARG;
}

// the apply behind the callbacks and the solve entries: checks, then two triangular solves on the library's stream.
// c64: the complex64 entries (a complex64 handle only); otherwise cplx picks the fp64 or the complex128 factor.
static int ic0_call(lcg_hip_csr *A, bool cplx, bool c64, int which, const double *x, double *y, long n_size)
{
    if (!A || !x || !y) return LCG_HIP_E_ARG;
    if (!c64) TRY_C64(A, "IC(0) apply");
    else if (!A->c64) return arg_error("IC(0): a complex64 entry on a fp64 / complex128 handle (lcg_hip_ic0_solve, lcg_hip_ic0_mx, clcg_hip_ic0_mx)");
    const Ic0 *F = ic0_of(A);
    if (!F || !F->ok) return arg_error(c64 ? "IC(0): the handle has no factor (lcg_hip_csr_build_ic0_c64)" : "IC(0): the handle has no factor (lcg_hip_csr_build_ic0)");
    if (F->c64 != c64) return arg_error("IC(0): the factor's value type differs from the entry's");
    if (F->cplx != cplx) return arg_error(cplx ? "IC(0): complex callback on a real factor" : "IC(0): real callback on a complex factor");
    if (n_size >= 0 && n_size != F->n) return arg_error("IC(0): n_size differs from the factor's %ld rows", F->n);
    if (which < 0 || which > 2) return arg_error("IC(0): which = %ld (0, 1 or 2)", which);
    const size_t bytes = (c64 ? sizeof(float2) : sizeof(double) * (cplx ? 2 : 1)) * (size_t)F->n;
    if ((const char *)x < (const char *)y + bytes && (const char *)y < (const char *)x + bytes)
        return arg_error("IC(0): x and y overlap");
    Ctx &c = ctx();
    if (c64) return ic0_apply<float2>(F, which, x, y, c.stream, ax_flag(c));
    return cplx ? ic0_apply<double2>(F, which, x, y, c.stream, ax_flag(c)) : ic0_apply<double>(F, which, x, y, c.stream, ax_flag(c));
}

// the build behind lcg_hip_csr_build_ic0 and lcg_hip_csr_build_ic0_c64 (the handle's type already checked)
static int ic0_build_entry(lcg_hip_csr *A)
{
    if (A->distributed) return arg_error("IC(0): not available on a sharded matrix");
    if (A->n_cols != A->n_rows) return arg_error("IC(0): the matrix is not square");
    int rc = ensure_init(); if (rc) return rc;
    Ctx &c = ctx();
    const auto t0 = std::chrono::steady_clock::now();
    int max_merged = IC_WG;
    if (A->ic0) { max_merged = ic0_of(A)->max_merged; ic0_free(A); }
    Ic0 *F = new Ic0();
    F->n = A->n_rows; F->cplx = A->is_complex; F->c64 = A->c64; F->max_merged = max_merged;
    A->ic0 = F;
    rc = F->c64 ? ic0_build<float2>(A, F, c.stream) : F->cplx ? ic0_build<double2>(A, F, c.stream) : ic0_build<double>(A, F, c.stream);
    F->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc) { ic0_free(A); return rc; }
    if (F->zero_pivot >= 0) return arg_error("IC(0): the pivot of row %ld is not usable (zero, negative or not finite)", F->zero_pivot);
    F->ok = true;
    return 0;
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_csr_build_ic0(lcg_hip_csr_t A)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_build_ic0");
    return ic0_build_entry(A);
}

int lcg_hip_csr_build_ic0_c64(lcg_hip_csr_t A)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    int rc = ensure_init(); if (rc) return rc;
    if (!A) return LCG_HIP_E_ARG;
    if (!A->c64) return arg_error("lcg_hip_csr_build_ic0_c64: the handle is not a complex64 matrix (lcg_hip_csr_create_c64; "
                                  "fp64 / complex128 handles: lcg_hip_csr_build_ic0)");
    return ic0_build_entry(A);
}

int lcg_hip_csr_ic0_info(lcg_hip_csr_t A, int *levels_lower, int *levels_upper, int *launches_per_apply, int *zero_pivot,
                         double *build_ms, int64_t *bytes)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || !A->ic0) return LCG_HIP_E_ARG;
    const Ic0 *F = ic0_of(A);
    if (levels_lower) *levels_lower = F->fw.levels;
    if (levels_upper) *levels_upper = F->bw.levels;
    if (launches_per_apply) *launches_per_apply = F->sweeps > 0 ? 2 * F->sweeps : (int)(F->fw.segs.size() + F->bw.segs.size());
    if (zero_pivot) *zero_pivot = F->zero_pivot;
    if (build_ms) *build_ms = F->build_ms;
    if (bytes) {
        const int64_t vw = F->cplx ? 16 : 8;                                     // (complex64: 8, one float pair)
        *bytes = 2 * (4 * ((int64_t)F->n + 1) + (4 + vw) * F->L.nnz)               // L and L^T
               + 2 * 4 * (int64_t)F->n + 4 * ((int64_t)F->fw.levels + F->bw.levels + 2)   // level orders
               + vw * F->n + 4;                                                  // work vector, pivot word
        if (F->sweeps > 0) *bytes += 2 * vw * F->n;                              // the sweeps' two intermediate vectors
    }
    return 0;
}

int lcg_hip_csr_ic0_set_sweeps(lcg_hip_csr_t A, int sweeps)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return arg_error("lcg_hip_csr_ic0_set_sweeps: the handle is NULL");
    Ic0 *F = ic0_of(A);
    if (!F || !F->ok) return arg_error("lcg_hip_csr_ic0_set_sweeps: the handle has no factor (lcg_hip_csr_build_ic0, lcg_hip_csr_build_ic0_c64)");
    if (sweeps < 0) return arg_error("lcg_hip_csr_ic0_set_sweeps: sweeps = %ld (0: the exact solves, k >= 1: k sweeps per triangle)", sweeps);
    if (sweeps > 0 && !F->sw[0]) {
        const size_t bytes = (F->c64 ? sizeof(float2) : sizeof(double) * (F->cplx ? 2 : 1)) * (size_t)std::max(F->n, 1);
        for (double *&p : F->sw) {
            if (hipMalloc(&p, bytes) == hipSuccess) continue;
            for (double *&q : F->sw) { if (q) hipFree(q); q = nullptr; }
            return fail(hipErrorOutOfMemory, "ic0 sweep vectors", __FILE__, __LINE__);
        }
    }
    if (sweeps == 0)                            // (hipFree waits for the applies still on the stream)
        for (double *&p : F->sw) { if (p) hipFree(p); p = nullptr; }
    F->sweeps = sweeps;
    return 0;
}

int lcg_hip_csr_ic0_get_sweeps(lcg_hip_csr_t A, int *sweeps)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return arg_error("lcg_hip_csr_ic0_get_sweeps: the handle is NULL");
    const Ic0 *F = ic0_of(A);
    if (!F || !F->ok) return arg_error("lcg_hip_csr_ic0_get_sweeps: the handle has no factor (lcg_hip_csr_build_ic0, lcg_hip_csr_build_ic0_c64)");
    if (!sweeps) return arg_error("lcg_hip_csr_ic0_get_sweeps: sweeps is NULL");
    *sweeps = F->sweeps;
    return 0;
}

int lcg_hip_csr_ic0_factor(lcg_hip_csr_t A, const int **rowptr, const int **col, const double **val)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || !A->ic0) return LCG_HIP_E_ARG;
    const Ic0 *F = ic0_of(A);
    if (rowptr) *rowptr = F->L.rowptr;
    if (col) *col = F->L.col;
    if (val) *val = F->L.val;
    return 0;
}

int lcg_hip_ic0_solve(lcg_hip_csr_t A, int which, const double *x, double *y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return LCG_HIP_E_ARG;
    return ic0_call(A, A->is_complex, false, which, x, y, -1);
}

int lcg_hip_ic0_solve_c64(lcg_hip_csr_t A, int which, const float *x, float *y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    int rc = ensure_init(); if (rc) return rc;
    if (!A) return LCG_HIP_E_ARG;
    return ic0_call(A, false, true, which, reinterpret_cast<const double *>(x), reinterpret_cast<double *>(y), -1);
}

int lcg_hip_csr_ic0_schedule_for_test(lcg_hip_csr_t A, int max_merged_rows)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || !A->ic0 || max_merged_rows < -1 || max_merged_rows > IC_WG) return LCG_HIP_E_ARG;
    Ic0 *F = ic0_of(A);
    F->max_merged = max_merged_rows < 0 ? IC_WG : max_merged_rows;
    tri_segments(F->fw, F->max_merged);
    tri_segments(F->bw, F->max_merged);
    return 0;
}

// The callback types return void (lcg.h:37-38, clcg.h:40-41): a failure is parked in Ctx::ax_rc (driver.hpp: checked_mx).
void lcg_hip_ic0_mx(void *instance, const double *x, double *prod_Mx, const int n_size)
{
    NOT_DENSE_CB(instance);
    const int rc = ic0_call(static_cast<lcg_hip_csr *>(instance), false, false, 2, x, prod_Mx, n_size);
    if (rc && !ctx().ax_rc) ctx().ax_rc = rc;
}

void clcg_hip_ic0_mx(void *instance, const double *x, double *prod_Mx, const int n_size, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    (void)layout;       // M = L.L^T is complex-symmetric: M^T = M
    const int rc = conjugate ? arg_error("IC(0): conjugate = 1 is not offered (M^H != M)")
                             : ic0_call(static_cast<lcg_hip_csr *>(instance), true, false, 2, x, prod_Mx, n_size);
    if (rc && !ctx().ax_rc) ctx().ax_rc = rc;
}

void clcg_hip_ic0_mx_c64(void *instance, const float *x, float *prod_Mx, const int n_size, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    (void)layout;       // M = L.L^T is complex-symmetric: M^T = M
    const int rc = conjugate ? arg_error("IC(0): conjugate = 1 is not offered (M^H != M)")
                             : ic0_call(static_cast<lcg_hip_csr *>(instance), false, true, 2, reinterpret_cast<const double *>(x),
                                        reinterpret_cast<double *>(prod_Mx), n_size);
    if (rc && !ctx().ax_rc) ctx().ax_rc = rc;
}

} // extern "C"
