// csr_tri.hip -- the one triangular-factor core behind IC(0) (csr_ic0.hip) and ILU(0) (csr_ilu0.hip): a triangle's level
// schedule, its exact solve (TriSolveRow on the level walker of csr_tri.hpp), its k Jacobi sweeps (k_ic_scale, k_ic_sweep), the
// apply that chooses between them, the pivot word, and the host surface the two files' exported entries forward into.  What a
// factor IS -- its pattern, its factor row, its pivot rule, how its upper triangle is made -- stays with its file.  DESIGN 11, 13.
//
// Every row of a solve is computed by one thread in one fixed order -- s = x_i, minus T(i,k).y_k in column order, divided by
// T(i,i) unless the diagonal is unit -- so results are the same bits from call to call and under every grouping of the levels.
// A sweep sums a row exactly so, reads one vector and writes another: a row whose inputs are final has the exact solve's bits,
// and after `levels` sweeps every row has.
#include <chrono>

#include "csr_tri.hpp"

namespace lcgh {

typedef int ic_v4i __attribute__((ext_vector_type(4)));
typedef double ic_v2d __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------- sweeps
// One Jacobi sweep over a whole triangle: yout_i = (x_i - sum_p T(i,c_p) yin_{c_p}) / T(i,i) for every row i in ONE launch.
// Row i is summed as the exact solve's row sums it (one accumulator from x_i, the products subtracted in column order, one
// ic_div).  DG says where the row keeps its diagonal: 0 last (IC(0)'s L), 1 first (IC(0)'s L^T, ILU(0)'s U), 2 nowhere -- a
// unit diagonal that is not stored and not divided by (ILU(0)'s L).
// The rows of a factor are short (half of A's row), so a thread per row straight out of CSR would read col / val at a stride
// of the row length.  Instead (the row-block A.x kernels' shape, csr.hip) the workgroup's IC_SR consecutive rows own one
// contiguous slice of col / val: it is loaded 16 bytes per lane into LDS, every load issued before the first LDS store, then
// thread r walks row r out of LDS with up to four gathers of yin in flight, and yout is written coalesced.  A workgroup whose
// slice does not fit the window (a dense row among its rows) walks its rows out of global memory: the same sums.
template <class V, int DG>
static __global__ __launch_bounds__(IC_SR) void k_ic_scale(int n, const int *__restrict__ rowptr, const V *__restrict__ val,
                                                          const V *__restrict__ x, V *__restrict__ y, const int *done)
{   // the first sweep, from y = 0: y = x / diag
    if (done && *done) return;
    const int i = blockIdx.x * IC_SR + threadIdx.x;
    if (i < n) y[i] = DG == 2 ? x[i] : ic_div(x[i], val[DG == 1 ? rowptr[i] : rowptr[i + 1] - 1]);
}

template <class V, int DG>
static __global__ __launch_bounds__(IC_SR) void k_ic_sweep(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                          const V *__restrict__ val, const V *__restrict__ x, const V *__restrict__ yin,
                                                          V *__restrict__ yout, const int *done)
{
    constexpr int NRND = IC_SCH / (IC_SR * 4);          // 4-entry units per lane
    constexpr int VU = sizeof(V) / 4;                   // 16-byte pieces of val per 4 entries
    constexpr int UNR = 4;                              // gathers of yin in flight per lane
    __shared__ __attribute__((aligned(16))) V sval[IC_SCH];
    __shared__ __attribute__((aligned(16))) int scol[IC_SCH];
    if (done && *done) return;
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * IC_SR;
    const int nrows = min(IC_SR, n - row0);
    const int base = rowptr[row0] & ~3;
    const int cnt = rowptr[row0 + nrows] - base;
    // this lane's row bounds and x_i, requested before the slice's stream (vmcnt counts in order)
    const int rsafe = tid < nrows ? tid : 0;
    const int rs = rowptr[row0 + rsafe], re = rowptr[row0 + rsafe + 1];
    V acc = x[row0 + rsafe];
    const int b = DG == 1 ? rs + 1 : rs, f = DG == 0 ? re - 1 : re, dg = DG == 1 ? rs : re - 1;     // (dg is not read when DG == 2)
    if (cnt > IC_SCH) {                                 // (uniform over the workgroup)
        if (tid >= nrows) return;
        for (int p = b; p < f; p++) acc = vsub(acc, ic_mul(val[p], yin[col[p]]));
        yout[row0 + tid] = DG == 2 ? acc : ic_div(acc, val[dg]);
        return;
    }
    ic_v4i pc[NRND]; ic_v2d pv[NRND * VU];
#pragma unroll
    for (int r = 0; r < NRND; r++) {
        const int u = tid * 4 + r * IC_SR * 4;
        // branch-free: lanes past the slice re-read its first unit.  col / val carry 64 bytes of slack (alloc_part), so the
        // slice's last unit may reach up to three entries past nnz.
        const long g = (long)base + (u < cnt ? u : 0);
        pc[r] = *reinterpret_cast<const ic_v4i *>(col + g);
#pragma unroll
        for (int q = 0; q < VU; q++) pv[r * VU + q] = reinterpret_cast<const ic_v2d *>(val + g)[q];
    }
    __builtin_amdgcn_sched_barrier(0);                  // every load above every LDS store
#pragma unroll
    for (int r = 0; r < NRND; r++) {
        const int u = tid * 4 + r * IC_SR * 4;
        if (u < cnt) {
            *reinterpret_cast<ic_v4i *>(scol + u) = pc[r];
#pragma unroll
            for (int q = 0; q < VU; q++) reinterpret_cast<ic_v2d *>(sval + u)[q] = pv[r * VU + q];
        }
    }
    __syncthreads();
    if (tid >= nrows) return;
    int p = b - base;
    const int fe = f - base;
    for (; p + UNR <= fe; p += UNR) {
        V a[UNR], yv[UNR];
#pragma unroll
        for (int q = 0; q < UNR; q++) { a[q] = sval[p + q]; yv[q] = yin[scol[p + q]]; }
#pragma unroll
        for (int q = 0; q < UNR; q++) acc = vsub(acc, ic_mul(a[q], yv[q]));
    }
    {   // the row's last 0..3 entries, their gathers in flight together as well
        V a[UNR - 1], yv[UNR - 1];
        const int m = fe - p;
#pragma unroll
        for (int q = 0; q < UNR - 1; q++) if (q < m) { a[q] = sval[p + q]; yv[q] = yin[scol[p + q]]; }
#pragma unroll
        for (int q = 0; q < UNR - 1; q++) if (q < m) acc = vsub(acc, ic_mul(a[q], yv[q]));
    }
    yout[row0 + tid] = DG == 2 ? acc : ic_div(acc, sval[dg - base]);
}

// ------------------------------------------------------------------------------------------- solves
// y_i = (x_i - sum_k T(i,k) y_k) / T(i,i), the sum in column order, the diagonal where DG says (2: unit, no division)
template <class V, int DG>
struct TriSolveRow {
    const int *rowptr, *col;
    const V *val, *x;
    V *y;
    __device__ __forceinline__ void operator()(int i) const
    {
        const int s = rowptr[i], e = rowptr[i + 1];
        const int b = DG == 1 ? s + 1 : s, f = DG == 0 ? e - 1 : e;
        V acc = x[i];
        for (int p = b; p < f; p++) acc = vsub(acc, ic_mul(val[p], y[col[p]]));
        y[i] = DG == 2 ? acc : ic_div(acc, val[DG == 1 ? s : e - 1]);
    }
};

// launches of a k-sweep apply of one triangle: a stored diagonal scales and sweeps k - 1 times; a unit one's first sweep is
// y = x, which its second reads in place of a vector of its own (k = 1: one copy)
static int tri_sweep_launches(int dg, int k) { return dg == 2 ? std::max(k - 1, 1) : k; }

// k sweeps on one triangle: y(1) = x / diag, then y(j+1) from y(j) between the two intermediate vectors; the last one writes y
template <class V, int DG>
static int tri_sweeps(const TriFactor *F, const CsrPart &T, const V *x, V *y, hipStream_t s, const int *done)
{
    const V *val = reinterpret_cast<const V *>(T.val);
    V *const buf[2] = {reinterpret_cast<V *>(F->sw[0]), reinterpret_cast<V *>(F->sw[1])};
    const int k = F->sweeps;
    const dim3 grid((unsigned)((F->n + IC_SR - 1) / IC_SR));
    if (F->n == 0) return 0;
    const V *in = x;                                    // unit diagonal: y(1) = x itself
    if (DG != 2 || k == 1) {
        V *out = k == 1 ? y : buf[0];
        hipLaunchKernelGGL((k_ic_scale<V, DG>), grid, dim3(IC_SR), 0, s, F->n, T.rowptr, val, x, out, done);
        in = out;
    }
    for (int j = 2; j <= k; j++) {
        V *out = j == k ? y : buf[in == buf[0] ? 1 : 0];
        hipLaunchKernelGGL((k_ic_sweep<V, DG>), grid, dim3(IC_SR), 0, s, F->n, T.rowptr, T.col, val, x, in, out, done);
        in = out;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

template <class V, int DG>
static int tri_apply_one(const TriFactor *F, bool up, const double *x, double *y, hipStream_t s, const int *done)
{
    const CsrPart &T = up ? F->up : F->lo;
    const V *xv = reinterpret_cast<const V *>(x);
    V *yv = reinterpret_cast<V *>(y);
    if (F->sweeps > 0) return tri_sweeps<V, DG>(F, T, xv, yv, s, done);
    return run_levels(up ? F->bw : F->fw, TriSolveRow<V, DG>{T.rowptr, T.col, reinterpret_cast<const V *>(T.val), xv, yv}, done, s);
}

template <class V, int DGLO, int DGUP>
static int tri_apply(const TriFactor *F, int which, const double *x, double *y, hipStream_t s, const int *done)
{
    if (which == 0) return tri_apply_one<V, DGLO>(F, false, x, y, s, done);
    if (which == 1) return tri_apply_one<V, DGUP>(F, true, x, y, s, done);
    const int rc = tri_apply_one<V, DGLO>(F, false, x, F->tmp, s, done);
    return rc ? rc : tri_apply_one<V, DGUP>(F, true, F->tmp, y, s, done);
}

int tri_apply(const TriFactor *F, int which, const double *x, double *y, hipStream_t s, const int *done)
{
    if (F->dg[0] == 2) return F->cplx ? tri_apply<double2, 2, 1>(F, which, x, y, s, done) : tri_apply<double, 2, 1>(F, which, x, y, s, done);
    if (F->c64) return tri_apply<float2, 0, 1>(F, which, x, y, s, done);
    return F->cplx ? tri_apply<double2, 0, 1>(F, which, x, y, s, done) : tri_apply<double, 0, 1>(F, which, x, y, s, done);
}

// ---------------------------------------------------------------------------------------- schedule
static void tri_free(IcTri &t)
{
    if (t.ord) hipFree(t.ord);
    if (t.lvl) hipFree(t.lvl);
    t = IcTri();
}

// level sets -> rows level by level (a counting sort by level: rows ascend inside a level)
static int tri_levels(IcTri &t, const std::vector<int> &level, int nlev)
{
    const int n = (int)level.size();
    t.levels = nlev;
    t.lvl_h.assign((size_t)nlev + 1, 0);
    for (int i = 0; i < n; i++) t.lvl_h[(size_t)level[i] + 1]++;
    for (int l = 0; l < nlev; l++) t.lvl_h[(size_t)l + 1] += t.lvl_h[(size_t)l];
    std::vector<int> ord((size_t)n), next(t.lvl_h.begin(), t.lvl_h.end() - 1);
    for (int i = 0; i < n; i++) ord[(size_t)next[(size_t)level[i]]++] = i;
    HIPCHK(hipMalloc(&t.ord, sizeof(int) * (size_t)n));
    HIPCHK(hipMalloc(&t.lvl, sizeof(int) * ((size_t)nlev + 1)));
    HIPCHK(hipMemcpy(t.ord, ord.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.lvl, t.lvl_h.data(), sizeof(int) * ((size_t)nlev + 1), hipMemcpyHostToDevice));
    return 0;
}
// launches: every level wider than max_merged alone, every run of narrower ones together
static void tri_segments(IcTri &t, int max_merged)
{
    t.segs.clear();
    for (int l = 0; l < t.levels;) {
        const int w = t.lvl_h[(size_t)l + 1] - t.lvl_h[(size_t)l];
        if (w > max_merged) { t.segs.push_back({l, l + 1, false}); l++; continue; }
        int m = l + 1;
        while (m < t.levels && t.lvl_h[(size_t)m + 1] - t.lvl_h[(size_t)m] <= max_merged) m++;
        t.segs.push_back({l, m, true});
        l = m;
    }
}

int tri_schedule(TriFactor *F, const std::vector<int> &level_fw, int nfw, const std::vector<int> &level_bw, int nbw)
{
    int rc = tri_levels(F->fw, level_fw, nfw); if (rc) return rc;
    rc = tri_levels(F->bw, level_bw, nbw); if (rc) return rc;
    tri_segments(F->fw, F->max_merged);
    tri_segments(F->bw, F->max_merged);
    return 0;
}

// ------------------------------------------------------------------------------------------- pivots
static const int NO_PIVOT = 0x7fffffff;

int pivot_arm(TriFactor *F, hipStream_t s)
{
    HIPCHK(hipMalloc(&F->zp, sizeof(int)));
    HIPCHK(hipMemcpyAsync(F->zp, &NO_PIVOT, sizeof(int), hipMemcpyHostToDevice, s));
    return 0;
}
int pivot_read(TriFactor *F, hipStream_t s)
{
    int zp = NO_PIVOT;
    HIPCHK(hipMemcpyAsync(&zp, F->zp, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    F->zero_pivot = zp == NO_PIVOT ? -1 : zp;
    return 0;
}

// --------------------------------------------------------------------------------------------- host
void tri_factor_free(TriFactor *&F)
{
    if (!F) return;
    free_part(F->lo); free_part(F->up);
    tri_free(F->fw); tri_free(F->bw);
    if (F->tmp) hipFree(F->tmp);
    if (F->w) hipFree(F->w);
    for (double *&p : F->sw) if (p) hipFree(p);
    for (double *&p : F->mw) if (p) hipFree(p);
    if (F->zp) hipFree(F->zp);
    delete F;
    F = nullptr;
}

void park(int rc) { if (rc && !ctx().ax_rc) ctx().ax_rc = rc; }

int tri_build(lcg_hip_csr *A, TriSlot slot, const char *name, int dg_lo, const char *pivot_rule,
              int (*build)(lcg_hip_csr *, TriFactor *, hipStream_t))
{
    if (A->distributed) return arg_error("%s: not available on a sharded matrix", name);
    if (A->n_cols != A->n_rows) return arg_error("%s: the matrix is not square", name);
    int rc = ensure_init(); if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    int max_merged = IC_WG;
    if (A->*slot) { max_merged = (A->*slot)->max_merged; tri_factor_free(A->*slot); }
    TriFactor *F = A->*slot = new TriFactor();
    F->name = name; F->dg[0] = dg_lo;
    F->n = A->n_rows; F->cplx = A->is_complex; F->c64 = A->c64; F->max_merged = max_merged;
    rc = build(A, F, ctx().stream);
    F->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc) { tri_factor_free(A->*slot); return rc; }
    if (F->zero_pivot >= 0) return arg_error("%s: the pivot of row %d is not usable (%s)", name, F->zero_pivot, pivot_rule);
    F->ok = true;
    return 0;
}

static size_t value_bytes(const TriFactor *F) { return F->c64 ? sizeof(float2) : sizeof(double) * (F->cplx ? 2 : 1); }

int tri_check(lcg_hip_csr *A, TriSlot slot, const char *name, const char *builder, bool cplx, bool c64, long n_size, int which,
              const double *x, const double *y, const TriFactor **out)
{
    if (!c64) TRY_C64(A, (std::string(name) + " apply").c_str());
    else if (!A->c64) return arg_error("%s: a complex64 entry on a fp64 / complex128 handle (lcg_hip_ic0_solve, lcg_hip_ic0_mx, clcg_hip_ic0_mx)", name);
    const TriFactor *F = A->*slot;
    if (!F || !F->ok) return arg_error("%s: the handle has no factor (%s)", name, builder);
    if (F->c64 != c64) return arg_error("%s: the factor's value type differs from the entry's", name);
    if (F->cplx != cplx) return arg_error(cplx ? "%s: complex callback on a real factor" : "%s: real callback on a complex factor", name);
    if (n_size >= 0 && n_size != F->n) return arg_error("%s: n_size differs from the factor's %d rows", name, F->n);
    if (which < 0 || which > 2) return arg_error("%s: which = %d (0, 1 or 2)", name, which);
    const size_t bytes = value_bytes(F) * (size_t)F->n;
    if (y && (const char *)x < (const char *)y + bytes && (const char *)y < (const char *)x + bytes)
        return arg_error("%s: x and y overlap", name);
    *out = F;
    return 0;
}

int tri_call(lcg_hip_csr *A, TriSlot slot, const char *name, const char *builder, bool cplx, bool c64, int which, const double *x,
             double *y, long n_size)
{
    if (!A || !x || !y) return LCG_HIP_E_ARG;
    const TriFactor *F = nullptr;
    const int rc = tri_check(A, slot, name, builder, cplx, c64, n_size, which, x, y, &F);
    return rc ? rc : tri_apply(F, which, x, y, ctx().stream, ax_flag(ctx()));
}

int tri_apply_launches(const TriFactor *F, int which)
{
    int l = 0;
    if (which != 1) l += F->sweeps > 0 ? tri_sweep_launches(F->dg[0], F->sweeps) : (int)F->fw.segs.size();
    if (which != 0) l += F->sweeps > 0 ? tri_sweep_launches(F->dg[1], F->sweeps) : (int)F->bw.segs.size();
    return l;
}

int tri_info(lcg_hip_csr *A, TriSlot slot, int *levels_lo, int *levels_up, int *launches_per_apply, int *zero_pivot, double *build_ms,
             int64_t *bytes)
{
    if (!A || !(A->*slot)) return LCG_HIP_E_ARG;
    const TriFactor *F = A->*slot;
    if (levels_lo) *levels_lo = F->fw.levels;
    if (levels_up) *levels_up = F->bw.levels;
    if (launches_per_apply) *launches_per_apply = tri_apply_launches(F, 2);
    if (zero_pivot) *zero_pivot = F->zero_pivot;
    if (build_ms) *build_ms = F->build_ms;
    if (bytes) {
        const int64_t vw = (int64_t)value_bytes(F), n = F->n;
        const int vectors = (F->tmp != nullptr) + (F->w != nullptr) + (F->sw[0] != nullptr) + (F->sw[1] != nullptr)
                          + F->mk * ((F->mw[0] != nullptr) + (F->mw[1] != nullptr) + (F->mw[2] != nullptr));      // (a k-wide one counts k)
        *bytes = 2 * 4 * (n + 1) + (4 + vw) * ((int64_t)F->lo.nnz + (int64_t)F->up.nnz)      // the two triangles
               + 2 * 4 * n + 4 * ((int64_t)F->fw.levels + F->bw.levels + 2)                   // level orders
               + vectors * vw * n + 4;                                                        // work and sweep vectors held, pivot word
    }
    return 0;
}

// what the two sweeps entries refuse before they look at their own argument (0: A holds a usable factor)
static int sweeps_refusal(lcg_hip_csr *A, TriSlot slot, const char *entry, const char *builders)
{
    if (!A) return arg_error("%s: the handle is NULL", entry);
    if (!(A->*slot) || !(A->*slot)->ok) return arg_error("%s: the handle has no factor (%s)", entry, builders);
    return 0;
}

int tri_set_sweeps(lcg_hip_csr *A, TriSlot slot, const char *entry, const char *builders, int sweeps)
{
    if (const int rc = sweeps_refusal(A, slot, entry, builders)) return rc;
    if (sweeps < 0) return arg_error("%s: sweeps = %d (0: the exact solves, k >= 1: k sweeps per triangle)", entry, sweeps);
    TriFactor *F = A->*slot;
    if (sweeps > 0 && !F->sw[0]) {
        const size_t bytes = value_bytes(F) * (size_t)std::max(F->n, 1);
        for (double *&p : F->sw) {
            if (hipMalloc(&p, bytes) == hipSuccess) continue;
            for (double *&q : F->sw) { if (q) hipFree(q); q = nullptr; }
            return fail(hipErrorOutOfMemory, "sweep vectors", __FILE__, __LINE__);
        }
    }
    if (sweeps == 0)                            // (hipFree waits for the applies still on the stream)
        for (double *&p : F->sw) { if (p) hipFree(p); p = nullptr; }
    F->sweeps = sweeps;
    return 0;
}

int tri_get_sweeps(lcg_hip_csr *A, TriSlot slot, const char *entry, const char *builders, int *sweeps)
{
    if (const int rc = sweeps_refusal(A, slot, entry, builders)) return rc;
    if (!sweeps) return arg_error("%s: sweeps is NULL", entry);
    *sweeps = (A->*slot)->sweeps;
    return 0;
}

int tri_schedule_for_test(lcg_hip_csr *A, TriSlot slot, int max_merged_rows)
{
    if (!A || !(A->*slot) || max_merged_rows < -1 || max_merged_rows > IC_WG) return LCG_HIP_E_ARG;
    TriFactor *F = A->*slot;
    F->max_merged = max_merged_rows < 0 ? IC_WG : max_merged_rows;
    tri_segments(F->fw, F->max_merged);
    tri_segments(F->bw, F->max_merged);
    return 0;
}

int tri_arrays(lcg_hip_csr *A, TriSlot slot, int which, const int **rowptr, const int **col, const double **val)
{
    if (!A || !(A->*slot) || which < 0 || which > 1) return LCG_HIP_E_ARG;
    const CsrPart &T = which ? (A->*slot)->up : (A->*slot)->lo;
    if (!T.rowptr) return LCG_HIP_E_ARG;
    if (rowptr) *rowptr = T.rowptr;
    if (col) *col = T.col;
    if (val) *val = T.val;
    return 0;
}

} // namespace lcgh
