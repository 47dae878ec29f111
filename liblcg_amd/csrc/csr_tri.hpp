// csr_tri.hpp -- what the incomplete factorisations share (csr_ic0.hip: IC(0), csr_ilu0.hip: ILU(0)).  Here, compiled
// into both: the factor's struct, the device-side extraction of a factor's pattern from A (count, scan, fill, row sort, then a
// second count / scan / fill that sums duplicate columns), the element arithmetic of the three value types and the level
// walker -- a triangle's schedule turned into launches over a row functor (each build's factor row, the solve's row).  In
// csr_tri.hip, compiled once and declared below: the schedule itself, the two triangular applies (exact solves and Jacobi
// sweeps), the pivot word, and the host surface behind both factors' exported entries.
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
constexpr int IC_MT = 256;      // threads of a batched sweep's workgroup (csr_tri_multi.hip): k / 2 neighbouring lanes per row
constexpr int IC_MCH = 2048;    // its LDS window in entries (24 KiB: six workgroups per CU; 8, 16, 32 per row for k = 2, 4, 8)
constexpr int ic_mrows(int k) { return IC_MT * 2 / k; }    // rows of its workgroup: 256, 128, 64 for k = 2, 4, 8

struct IcSeg { int l0, l1; bool narrow; };      // levels [l0, l1): one launch
struct IcTri {                                  // one triangle's schedule
    int *ord = nullptr;         // device: rows level by level (ascending row inside a level)
    int *lvl = nullptr;         // device: level l's rows are ord[lvl[l] .. lvl[l+1])
    std::vector<int> lvl_h;
    std::vector<IcSeg> segs;
    int levels = 0;
};

// An incomplete factor of A as two triangles with sorted rows.  IC(0): lo = L (diagonal last), up = L^T (diagonal first).
// ILU(0): lo = L (unit diagonal, not stored), up = U (diagonal first).
struct TriFactor {
    const char *name = "";      // "IC(0)" / "ILU(0)": how messages call it
    int dg[2] = {0, 1};         // where a row of lo / up keeps its diagonal: 0 last, 1 first, 2 nowhere (unit) -- the DG of the kernels
    int n = 0;
    bool cplx = false, ok = false;
    bool c64 = false;           // complex64 values (8 bytes: cplx stays false, so the build moves them as real words)
    CsrPart lo, up;
    IcTri fw, bw;               // lo's schedule (forward), up's (backward)
    double *tmp = nullptr;      // lo^-1 x of the full apply (n values of the factor's type)
    double *w = nullptr;        // ILU(0) only: U^-1 L^-1 x of the right-preconditioned product (lcg_hip_csr_ax_ilu0)
    int sweeps = 0;             // 0: exact level-scheduled solves; k >= 1: k Jacobi sweeps per triangle
    double *sw[2] = {nullptr, nullptr};     // the sweeps' two intermediate vectors (n values each, held while sweeps >= 1)
    double *mw[3] = {nullptr, nullptr, nullptr};    // batched applies: lo^-1 X and the two sweep vectors, n * mk doubles each (tri_multi_reserve)
    int mk = 0;                 // the largest k a batched apply has asked for so far
    int *zp = nullptr;          // device: smallest row whose pivot failed (INT_MAX: none)
    int zero_pivot = -1;
    int max_merged = IC_WG;     // widest level a narrow group takes (lcg_hip_csr_{ic0,ilu0}_schedule_for_test)
    double build_ms = 0.0;
};
typedef TriFactor *lcg_hip_csr::*TriSlot;       // which of a handle's two factors: &lcg_hip_csr::ic0 or &lcg_hip_csr::ilu0

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

// ------------------------------------------------------------------------------------- level walker
// A schedule's launches over `row`, a small functor passed by value whose operator()(i) computes row i from rows of earlier
// levels.  A level wider than max_merged is one grid launch (k_lvl_wide); a run of narrower ones is ONE launch of one workgroup
// that walks them with a barrier between levels (k_lvl_narrow: workgroup-scope visibility only, no flag, no wait on another
// workgroup).  done: the solver's flag (a finished solve's launches fall through); the factor passes nullptr.
template <class Row>
__global__ __launch_bounds__(IC_WB) void k_lvl_wide(const int *ord, int b, int e, Row row, const int *done)
{
    if (done && *done) return;
    const int pos = b + blockIdx.x * blockDim.x + threadIdx.x;
    if (pos < e) row(ord[pos]);
}
template <class Row>
__global__ __launch_bounds__(IC_WG) void k_lvl_narrow(const int *ord, const int *lvl, int l0, int l1, Row row, const int *done)
{
    if (done && *done) return;
    for (int l = l0; l < l1; l++) {
        for (int pos = lvl[l] + threadIdx.x; pos < lvl[l + 1]; pos += blockDim.x) row(ord[pos]);
        __syncthreads();
    }
}
template <class Row>
static int run_levels(const IcTri &t, Row row, const int *done, hipStream_t s)
{
    for (const IcSeg &g : t.segs) {
        if (g.narrow)
            hipLaunchKernelGGL((k_lvl_narrow<Row>), dim3(1), dim3(IC_WG), 0, s, t.ord, t.lvl, g.l0, g.l1, row, done);
        else {
            const int b = t.lvl_h[(size_t)g.l0], e = t.lvl_h[(size_t)g.l1];
            hipLaunchKernelGGL((k_lvl_wide<Row>), dim3((unsigned)((e - b + IC_WB - 1) / IC_WB)), dim3(IC_WB), 0, s, t.ord, b, e, row, done);
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// --------------------------------------------------------------------------------------- csr_tri.hip
// build side.  tri_build: the body of the build entries once the handle's type is checked -- a fresh factor in A's slot (the
// grouping set for test survives a rebuild), `build` run on the library's stream, the pivot's verdict (`pivot_rule`: what the
// message says a usable pivot is not).  tri_schedule: both triangles' level sets into their schedules.  pivot_arm / pivot_read:
// the pivot word before the factor's launches, and F->zero_pivot after them (drains the stream).
int tri_build(lcg_hip_csr *A, TriSlot slot, const char *name, int dg_lo, const char *pivot_rule,
              int (*build)(lcg_hip_csr *, TriFactor *, hipStream_t));
int tri_schedule(TriFactor *F, const std::vector<int> &level_fw, int nfw, const std::vector<int> &level_bw, int nbw);
int pivot_arm(TriFactor *F, hipStream_t s);
int pivot_read(TriFactor *F, hipStream_t s);
// apply side.  tri_check: what every apply checks, in this order -- complex64 handle against entry, the factor's presence
// (`builder`: the entry the message names), its type, n_size (< 0: not given), which, x against y (y == nullptr: the result goes
// to a vector of the factor's own).  tri_apply: which = 0 lo^-1 x, 1 up^-1 x, 2 both, by exact solves or F->sweeps sweeps.
// tri_call: x, y, tri_check, tri_apply on the library's stream.  park: a void callback's failure into Ctx::ax_rc (driver.hpp:
// checked_mx).
int tri_check(lcg_hip_csr *A, TriSlot slot, const char *name, const char *builder, bool cplx, bool c64, long n_size, int which,
              const double *x, const double *y, const TriFactor **out);
int tri_apply(const TriFactor *F, int which, const double *x, double *y, hipStream_t s, const int *done);
int tri_call(lcg_hip_csr *A, TriSlot slot, const char *name, const char *builder, bool cplx, bool c64, int which, const double *x,
             double *y, long n_size);
void park(int rc);
// batched apply (csr_tri_multi.hip): a block of k = 2, 4, 8 vectors in multi.hpp's layout, column j with the bits of tri_apply on
// column j alone.  tri_multi_reserve: the factor's k-wide work vectors for such an apply (may allocate and wait; a call that finds
// them does neither) -- before tri_apply_multi, which only launches.  tri_apply_launches: launches of one apply of `which`.
int tri_multi_reserve(TriFactor *F, int k, int which);
int tri_apply_multi(const TriFactor *F, int k, int which, const double *X, double *Y, hipStream_t s, const int *done);
int tri_apply_launches(const TriFactor *F, int which);
// the bodies of lcg_hip_csr_{ic0,ilu0}_info / _set_sweeps / _get_sweeps / _schedule_for_test / _factor (`entry`: the exported
// name, `builders`: the build entries a "no factor" message names)
int tri_info(lcg_hip_csr *A, TriSlot slot, int *levels_lo, int *levels_up, int *launches_per_apply, int *zero_pivot, double *build_ms,
             int64_t *bytes);
int tri_set_sweeps(lcg_hip_csr *A, TriSlot slot, const char *entry, const char *builders, int sweeps);
int tri_get_sweeps(lcg_hip_csr *A, TriSlot slot, const char *entry, const char *builders, int *sweeps);
int tri_schedule_for_test(lcg_hip_csr *A, TriSlot slot, int max_merged_rows);
int tri_arrays(lcg_hip_csr *A, TriSlot slot, int which, const int **rowptr, const int **col, const double **val);

} // namespace lcgh
