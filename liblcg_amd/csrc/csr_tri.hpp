// csr_tri.hpp -- what the incomplete factorisations share (csr_ic0.hip: IC(0), csr_ilu0.hip: ILU(0)): the
// device-side extraction of a factor's pattern from A (count, scan, fill, row sort, then a second count / scan / fill that sums
// duplicate columns), a triangle's level schedule (rows level by level, wide / narrow launch segments) and the element
// arithmetic of the three value types.  The kernels and host helpers are `static`: each translation unit has its own copy.
#pragma once

#include <algorithm>
#include <vector>

#include "devcommon.hpp"
#include "c64common.hpp"

namespace lcgh {

constexpr int IC_WG = 1024;     // threads of a narrow-group launch = widest level it takes in production
constexpr int IC_WB = 256;      // threads per block of a wide-level launch
constexpr int IC_SR = 256;      // rows of a sweep's workgroup = its threads
constexpr int IC_SCH = 2048;    // its LDS window in entries (8 per row; 24 KiB with 8-byte values, 40 KiB with 16-byte ones)
typedef int ic_v4i __attribute__((ext_vector_type(4)));
typedef double ic_v2d __attribute__((ext_vector_type(2)));

struct IcSeg { int l0, l1; bool narrow; };      // levels [l0, l1): one launch
struct IcTri {                                  // one triangle's schedule
    int *ord = nullptr;         // device: rows level by level (ascending row inside a level)
    int *lvl = nullptr;         // device: level l's rows are ord[lvl[l] .. lvl[l+1])
    std::vector<int> lvl_h;
    std::vector<IcSeg> segs;
    int levels = 0;
};

__device__ __forceinline__ double ic_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double2 ic_mul(double2 a, double2 b) { return cmul(a, b); }
__device__ __forceinline__ float2 ic_mul(float2 a, float2 b) { return c64_mul(a, b); }
__device__ __forceinline__ double ic_div(double a, double b) { return a / b; }
__device__ __forceinline__ double2 ic_div(double2 a, double2 b) { return cdiv(a, b); }
__device__ __forceinline__ float2 ic_div(float2 a, float2 b) { return c64_div(a, b); }

// ---------------------------------------------------------------------------------------- analysis
// LOWER: the entries on or below the diagonal (IC(0)); otherwise every entry (ILU(0)).  Either way plus one explicit zero on
// the diagonal: every row of the factor has its diagonal.
template <bool LOWER>
static __global__ void k_ic_low_count(int n, const int *rowptr, const int *col, int *cnt)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int k = 1;
    for (int p = rowptr[i]; p < rowptr[i + 1]; p++) k += !LOWER || col[p] <= i;
    cnt[i] = k;
}
template <class V, bool LOWER>
static __global__ void k_ic_low_fill(int n, const int *rowptr, const int *col, const V *val, const int *rpL, int *colL, V *valL)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int q = rpL[i];
    for (int p = rowptr[i]; p < rowptr[i + 1]; p++)
        if (!LOWER || col[p] <= i) { colL[q] = col[p]; valL[q] = val[p]; q++; }
    colL[q] = i; valL[q] = vzero(V());
}
static __global__ void k_ic_uniq_count(int n, const int *rowptr, const int *col, int *cnt)
{   // distinct columns of a sorted row
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int k = 0;
    for (int p = rowptr[i]; p < rowptr[i + 1]; p++) k += p == rowptr[i] || col[p] != col[p - 1];
    cnt[i] = k;
}
template <class V>
static __global__ void k_ic_uniq_fill(int n, const int *rowptr, const int *col, const V *val, const int *rpU, int *colU, V *valU)
{   // duplicate columns summed in their sorted order
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int q = rpU[i] - 1;
    for (int p = rowptr[i]; p < rowptr[i + 1]; p++) {
        if (p == rowptr[i] || col[p] != col[p - 1]) { q++; colU[q] = col[p]; valU[q] = val[p]; }
        else valU[q] = vadd(valU[q], val[p]);
    }
}

// A's lower triangle (LOWER) or all of A, duplicates summed, one diagonal per row: into `out` (sorted rows).  cplx: 16-byte
// values (complex64's 8-byte pairs travel as real words).  Drains the stream.
template <class V, bool LOWER>
static int extract_rows(const lcg_hip_csr *A, CsrPart &out, bool cplx, hipStream_t s)
{
    const int n = A->n_rows;
    const unsigned g = (unsigned)((n + VB - 1) / VB);
    int *cnt = nullptr;
    CsrPart R;                                          // the entries as they come, duplicates included
    auto bail = [&](int rc) { if (cnt) hipFree(cnt); free_part(R); return rc; };
    if (hipMalloc(&cnt, sizeof(int) * (size_t)std::max(n, 1)) != hipSuccess) return bail(fail(hipErrorOutOfMemory, "factor pattern counts", __FILE__, __LINE__));
    hipLaunchKernelGGL((k_ic_low_count<LOWER>), dim3(g), dim3(VB), 0, s, n, A->main.rowptr, A->main.col, cnt);
    int *rp = nullptr;
    if (hipMalloc(&rp, sizeof(int) * ((size_t)n + 1)) != hipSuccess) return bail(fail(hipErrorOutOfMemory, "factor pattern rowptr", __FILE__, __LINE__));
    long total = 0;
    int rc = device_exclusive_scan(n, cnt, rp, s, &total);
    if (rc) { hipFree(rp); return bail(rc); }
    rc = alloc_part(R, n, total, cplx);
    hipFree(R.rowptr); R.rowptr = rp;
    if (rc) return bail(rc);
    hipLaunchKernelGGL((k_ic_low_fill<V, LOWER>), dim3(g), dim3(VB), 0, s, n, A->main.rowptr, A->main.col,
                       reinterpret_cast<const V *>(A->main.val), R.rowptr, R.col, reinterpret_cast<V *>(R.val));
    row_sort_launch(n, R.rowptr, R.col, R.val, cplx, s);
    hipLaunchKernelGGL(k_ic_uniq_count, dim3(g), dim3(VB), 0, s, n, R.rowptr, R.col, cnt);
    HIPCHK(hipGetLastError());
    if (hipMalloc(&rp, sizeof(int) * ((size_t)n + 1)) != hipSuccess) return bail(fail(hipErrorOutOfMemory, "factor pattern rowptr", __FILE__, __LINE__));
    rc = device_exclusive_scan(n, cnt, rp, s, &total);
    if (rc) { hipFree(rp); return bail(rc); }
    rc = alloc_part(out, n, total, cplx);
    hipFree(out.rowptr); out.rowptr = rp;
    if (rc) return bail(rc);
    out.n_cols = n;
    hipLaunchKernelGGL((k_ic_uniq_fill<V>), dim3(g), dim3(VB), 0, s, n, R.rowptr, R.col, reinterpret_cast<const V *>(R.val), out.rowptr,
                       out.col, reinterpret_cast<V *>(out.val));
    HIPCHK(hipGetLastError());
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return bail(fail(e, "factor pattern", __FILE__, __LINE__));
    return bail(0);
}

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

} // namespace lcgh
