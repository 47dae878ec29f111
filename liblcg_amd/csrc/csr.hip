// csr.hip -- CSR matrices in HBM: the plain row-block A.x kernels, the choice of a kernel family per part (ax_choose) and its
// dispatch, the handle's C ABI.  (Ingest, Jacobi diagonal, op(A), generators: csr_build.hip.  The packed row-block product -- its
// plan, k_spmv_ldsp, k_spmv_run1 / run1d, its setters and queries: csr_packed.hip, behind the interface in csr_plan.hpp.)
//
// A.x is the kernel the whole path is judged on: >= 80 % of the bytes of a CG iteration.
// It is HBM-bound (0.17 flop/byte): no MFMA.  The row-block kernels (this file unless said otherwise):
//
//  k_spmv_lds1<R>   (default)  One 256-thread block owns R consecutive rows (R*T = 256).
//      Stage 1: the block's contiguous slice of val/col streams from HBM into LDS with
//      16-byte-per-lane coalesced loads, ALL issued before the first LDS store (the CSR
//      arrays are read exactly once, at full width, whatever the row lengths).  Stage 2: lane (row = tid % R, j = tid / R) walks
//      its row's entries j, j+T, ... out of LDS and gathers x; consecutive lanes hold
//      consecutive ROWS, so for matrices with diagonal / stencil structure the x gather of a
//      wavefront is one contiguous run, and for arbitrary columns it is no worse than any
//      other mapping.  The T partial sums of a row meet in LDS; y is written coalesced.
//  k_spmv_ldsp      (csr_packed.hip) the same mapping for large real matrices with packed block-relative columns (18 / 21 bits) and,
//      where a 64-row block's columns advance by one per row, RUN blocks: row 0's columns only, x gathers sent out with the value
//      stream (the headline's kernel: DESIGN.md section 3.1a).  <DOT>: carries the dot that follows the product.
//  k_spmv_run1      (csr_packed.hip) short rows (stencils) whose blocks are runs: one wavefront per 64-row block, no barrier.
//  k_spmv_lds1d     small systems: the plain body + the dot that follows the product (two launches per CG iteration).
//  k_spmv_wave<T>   T consecutive lanes share a row (T = 64: wavefront per row), partial
//      sums folded with __shfl_down.  Better for long rows (> ~100 entries).
// (csr_tiled.hip, csr_binned.hip: the products for columns that do not run along diagonals.)
//
// Algorithmic bytes: 12*nnz + 4*(N+1) + 8*N (x) + 8*N (y), real.
#include <algorithm>
#include <type_traits>
#include <cstring>
#include <functional>
#include <numeric>

#include <chrono>

#include "csr_plan.hpp"

namespace lcgh {

// ------------------------------------------------------------------- wave-per-row family
// PUSH: the first pp.nblocks blocks of the grid do not multiply; they carry this rank's boundary
// entries of x to the neighbours (devcommon.hpp: push_block) while the rest of the grid works.
template <class V, int T, bool ACC, bool PUSH = false>
__global__ __launch_bounds__(VB) void k_spmv_wave(int n, const int *__restrict__ rowptr,
                                                  const int *__restrict__ col, const V *__restrict__ val,
                                                  const V *__restrict__ x, V *__restrict__ y,
                                                  const int *done, PushPlan pp)
{
    if (PUSH && (int)blockIdx.x < pp.nblocks) { push_block(pp, blockIdx.x); return; }
    if (PUSH && pp.nrecv > 0 && (int)blockIdx.x >= (int)gridDim.x - pp.nrecv) { recv_block(pp, (int)blockIdx.x - ((int)gridDim.x - pp.nrecv)); return; }
    const int bid = PUSH ? blockIdx.x - pp.nblocks : blockIdx.x;
    if (done && *done) return;
    const int sub = threadIdx.x % T;
    const long row = ((long)bid * VB + threadIdx.x) / T;
    V acc = vzero(V());
    if (row < n) {
        const int s = rowptr[row], e = rowptr[row + 1];
        int k = s + sub;
        // two independent gathers in flight per lane
        for (; k + T < e; k += 2 * T) {
            const int c0 = col[k], c1 = col[k + T];
            const V a0 = val[k], a1 = val[k + T];
            acc = mac(a0, x[c0], acc);
            acc = mac(a1, x[c1], acc);
        }
        if (k < e) acc = mac(val[k], x[col[k]], acc);
    }
#pragma unroll
    for (int off = T / 2; off > 0; off >>= 1) acc = vadd(acc, shfl_down_v(acc, off, T));
    if (sub == 0 && row < n) y[row] = ACC ? vadd(y[row], acc) : acc;
}

// ----------------------------------------------------------------------- LDS-staged family
// LDS budget per block: 26,880 B of staging (6 blocks fit a CU's 160 KiB; registers currently
// admit 5).  The row-sum exchange buffer aliases the staging buffer.
// (LdsCfg<V>::CH, the largest window, and the native vector types v4i / v2d: csr_plan.hpp)

// largest slice (entries from the 4-aligned start of a block's first row to the end of its last
// row) over all blocks of R rows: decides once per matrix whether every block fits one window
__global__ void k_max_slice(int n, int R, const int *rowptr, int *out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const long row0 = (long)b * R;
    if (row0 >= n) return;
    const int r1 = (int)min((long)n, row0 + R);
    atomicMax(out, rowptr[r1] - (rowptr[row0] & ~3));
}
void launch_max_slice(int n, int R, const int *rowptr, int *out, hipStream_t s)
{
    const int nb = (n + R - 1) / R;
    hipLaunchKernelGGL(k_max_slice, dim3((nb + VB - 1) / VB), dim3(VB), 0, s, n, R, rowptr, out);
}

// ---- one-window kernel: the host has verified (k_max_slice) that every block's slice fits one
// LDS window.  ALL of the block's HBM loads are issued before the first LDS store, 16 B per
// lane per access (~25 KB in flight per block); then every lane keeps UNR gathers of x in flight.
// The work of one row block, shared by the plain kernel and the one that carries a dot (below).  Returns the finished y
// of row row0 + tid % R on the lanes that wrote it (`mine`).
template <class V, int R, bool ACC, int CHE = LdsCfg<V>::CH>
__device__ __forceinline__ V lds1_block(int bid, int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                        const V *__restrict__ val, const V *__restrict__ x, V *__restrict__ y, V *sval, int *scol,
                                        bool &mine)
{
    constexpr int T = VB / R;
    constexpr int CH = CHE;                                 // entries per LDS window (multiple of 4)
    constexpr int NRND = (CH + VB * 4 - 1) / (VB * 4);      // 4-entry units per lane
    constexpr int VU = sizeof(V) / 4;                       // 16-byte pieces of val per 4 entries
    constexpr int UNR = 4;                                  // x gathers in flight per lane
    static_assert(T * R <= CH, "row-sum exchange must fit the staging buffer");
    V(*sred)[R] = reinterpret_cast<V(*)[R]>(sval);

    const int tid = threadIdx.x;
    const int row0 = bid * R;
    const int nrows = min(R, n - row0);
    const int rl = tid % R, j0 = tid / R;
    const int base = rowptr[row0] & ~3;
    const int cnt = rowptr[row0 + nrows] - base;
    // this lane's row bounds, requested BEFORE the block's stream: behind the fence below they would be issued when the stream has
    // arrived and cost the gather phase a memory latency of its own (vmcnt counts in order)
    const int rsafe = rl < nrows ? rl : 0;              // (branch-free, like the stream loads below)
    int rs = rowptr[row0 + rsafe], re = rowptr[row0 + rsafe + 1];
    if (rl >= nrows) { rs = 0; re = 0; }

    v4i pc[NRND]; v2d pv[NRND * VU];
#pragma unroll
    for (int r = 0; r < NRND; r++) {
        const int u = tid * 4 + r * VB * 4;
        // branch-free: lanes past the slice re-read its first unit (an L1 hit) instead of being
        // masked off -- a conditional load makes the compiler drain vmcnt at every join, which
        // serialises the rounds.  col/val carry >= 64 B of slack (CsrPart::padded): no tail case.
        const long g = (long)base + (u < cnt ? u : 0);
        pc[r] = *reinterpret_cast<const v4i *>(col + g);
#pragma unroll
        for (int q = 0; q < VU; q++) pv[r * VU + q] = reinterpret_cast<const v2d *>(val + g)[q];
    }
    // keep every load above every LDS store below: without this fence the scheduler pairs each
    // load with its store to save registers and the block has a third of the bytes in flight
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < NRND; r++) {
        const int u = tid * 4 + r * VB * 4;
        if (u < cnt) {
            *reinterpret_cast<v4i *>(scol + u) = pc[r];
#pragma unroll
            for (int q = 0; q < VU; q++) reinterpret_cast<v2d *>(sval + u)[q] = pv[r * VU + q];
        }
    }
    __syncthreads();
    // lane (row rl, slot j0) takes entries rs+j0, rs+j0+T, ... of its row
    V acc = vzero(V());
    int k = rs + j0;
    for (; k + (UNR - 1) * T < re; k += UNR * T) {
        int c[UNR]; V a[UNR], xv[UNR];
#pragma unroll
        for (int q = 0; q < UNR; q++) { c[q] = scol[k + q * T - base]; a[q] = sval[k + q * T - base]; }
#pragma unroll
        for (int q = 0; q < UNR; q++) xv[q] = x[c[q]];
#pragma unroll
        for (int q = 0; q < UNR; q++) acc = mac(a[q], xv[q], acc);
    }
    for (; k < re; k += T) acc = mac(sval[k - base], x[scol[k - base]], acc);
    __syncthreads();
    // the T partial sums of a row meet in LDS (staging buffer reused); y written coalesced
    mine = j0 == 0 && rl < nrows;
    if (T > 1) {
        sred[j0][rl] = acc;
        __syncthreads();
        if (mine) {
            V v = sred[0][rl];
#pragma unroll
            for (int j = 1; j < T; j++) v = vadd(v, sred[j][rl]);
            acc = ACC ? vadd(y[row0 + rl], v) : v;
            y[row0 + rl] = acc;
        }
    } else if (mine) {
        if (ACC) acc = vadd(y[row0 + rl], acc);
        y[row0 + rl] = acc;
    }
    return acc;
}

// CHE: the LDS window in entries (12 bytes each for real matrices); smaller where every block of the matrix fits -- more workgroups
// per CU (pk_window, csr_packed.hip: the ladder of k_spmv_ldsp)
template <class V, int R, bool ACC, bool PUSH = false, int CHE = LdsCfg<V>::CH>
__global__ __launch_bounds__(VB) void k_spmv_lds1(int n, long nnz, const int *__restrict__ rowptr,
                                                  const int *__restrict__ col, const V *__restrict__ val,
                                                  const V *__restrict__ x, V *__restrict__ y,
                                                  const int *done, PushPlan pp)
{
    if (PUSH && (int)blockIdx.x < pp.nblocks) { push_block(pp, blockIdx.x); return; }
    if (PUSH && pp.nrecv > 0 && (int)blockIdx.x >= (int)gridDim.x - pp.nrecv) { recv_block(pp, (int)blockIdx.x - ((int)gridDim.x - pp.nrecv)); return; }
    const int bid = PUSH ? blockIdx.x - pp.nblocks : blockIdx.x;
    constexpr int CH = CHE;
    __shared__ __attribute__((aligned(16))) V sval[CH];
    __shared__ __attribute__((aligned(16))) int scol[CH];
    if (done && *done) return;
    bool mine;
    (void)lds1_block<V, R, ACC, CHE>(bid, n, rowptr, col, val, x, y, sval, scol, mine);
}

// ---- the same product carrying a dot: the Krylov loops follow every A.x with y.u (CG / PCG: d.Ad, CGS / BiCGStab: Ap.r0,
// As.s and As.As; lcg.cpp:234, 389, 548-552, 720-724, 735-740) -- a pass of its own over two vectors and, on small systems, a
// launch of its own on the critical path.  Here the lanes that write y multiply it with u on the way out (u is requested
// before the block's stream, so the load hides behind it) and the workgroup leaves ONE partial sum per running sum in its
// slot of Ctx::ax_partials, which the consuming scalar step adds up in index order (devcommon.hpp: reduce_partials,
// PartCount) -- no atomics, the same bits from call to call.  y itself is bit-identical to the plain kernel's.
template <int R>
__global__ __launch_bounds__(VB) void k_spmv_lds1d(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                   const double *__restrict__ val, const double *__restrict__ x,
                                                   double *__restrict__ y, const int *done, DotPlan dp)
{
    constexpr int CH = LdsCfg<double>::CH;
    __shared__ __attribute__((aligned(16))) double sval[CH];
    __shared__ __attribute__((aligned(16))) int scol[CH];
    __shared__ double wsum[2][VB / 64];
    if (done && *done) return;
    const int rl = threadIdx.x % R, j0 = threadIdx.x / R;
    const long row = (long)blockIdx.x * R + rl;
    const double uv = dp.u[(j0 == 0 && row < n) ? row : 0];
    bool mine;
    const double v = lds1_block<double, R, false>(blockIdx.x, n, rowptr, col, val, x, y, sval, scol, mine);
    double a0 = mine ? v * uv : 0.0, a1 = mine ? v * v : 0.0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int NW = R >= 64 ? R / 64 : 1;        // wavefronts that hold finished rows
    if (w < NW) {
        a0 = wave_sum(a0); a1 = wave_sum(a1);
        if (lane == WSUM_LANE) { wsum[0][w] = a0; wsum[1][w] = a1; }
    }
    if (NW > 1) __syncthreads();
    if (threadIdx.x < 2 && (threadIdx.x == 0 || dp.yy)) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < NW; q++) t += wsum[threadIdx.x][q];
        dp.part[threadIdx.x * AXP_CAP + blockIdx.x] = t;
    }
}

// ---- windowed kernel: some block's rows are too long for one window; the slice is walked
// window by window (same mapping, general row clipping)
template <class V, int R, bool ACC, bool PUSH = false>
__global__ __launch_bounds__(VB) void k_spmv_ldsw(int n, long nnz, const int *__restrict__ rowptr,
                                                  const int *__restrict__ col, const V *__restrict__ val,
                                                  const V *__restrict__ x, V *__restrict__ y,
                                                  const int *done, PushPlan pp)
{
    if (PUSH && (int)blockIdx.x < pp.nblocks) { push_block(pp, blockIdx.x); return; }
    if (PUSH && pp.nrecv > 0 && (int)blockIdx.x >= (int)gridDim.x - pp.nrecv) { recv_block(pp, (int)blockIdx.x - ((int)gridDim.x - pp.nrecv)); return; }
    const int bid = PUSH ? blockIdx.x - pp.nblocks : blockIdx.x;
    constexpr int T = VB / R;
    constexpr int CH = LdsCfg<V>::CH;
    constexpr int VU = sizeof(V) / 4;
    __shared__ __attribute__((aligned(16))) V sval[CH];
    __shared__ __attribute__((aligned(16))) int scol[CH];
    V(*sred)[R] = reinterpret_cast<V(*)[R]>(sval);
    if (done && *done) return;

    const int tid = threadIdx.x;
    const int row0 = bid * R;
    const int nrows = min(R, n - row0);
    const int rl = tid % R, j0 = tid / R;
    const int s = rowptr[row0], e = rowptr[row0 + nrows];
    int rs = 0, re = 0;
    if (rl < nrows) { rs = rowptr[row0 + rl]; re = rowptr[row0 + rl + 1]; }
    V acc = vzero(V());
    for (int base = s & ~3; base < e; base += CH) {
        const int cnt = min(CH, e - base);
        for (int u = tid * 4; u < cnt; u += VB * 4) {
            const long g = (long)base + u;
            if (g + 3 < nnz) {
                *reinterpret_cast<v4i *>(scol + u) = *reinterpret_cast<const v4i *>(col + g);
#pragma unroll
                for (int q = 0; q < VU; q++) reinterpret_cast<v2d *>(sval + u)[q] = reinterpret_cast<const v2d *>(val + g)[q];
            } else {
                for (int q = 0; q < 4 && g + q < nnz; q++) { scol[u + q] = col[g + q]; sval[u + q] = val[g + q]; }
            }
        }
        __syncthreads();
        const int lo = max(rs, base), hi = min(re, base + cnt);
        int k = rs + j0;
        if (k < lo) k += ((lo - k + T - 1) / T) * T;
        for (; k + T < hi; k += 2 * T) {
            const int c0 = scol[k - base], c1 = scol[k + T - base];
            const V a0 = sval[k - base], a1 = sval[k + T - base];
            acc = mac(a0, x[c0], acc);
            acc = mac(a1, x[c1], acc);
        }
        if (k < hi) acc = mac(sval[k - base], x[scol[k - base]], acc);
        __syncthreads();
    }
    if (T > 1) {
        sred[j0][rl] = acc;
        __syncthreads();
        if (j0 == 0 && rl < nrows) {
            V v = sred[0][rl];
#pragma unroll
            for (int j = 1; j < T; j++) v = vadd(v, sred[j][rl]);
            y[row0 + rl] = ACC ? vadd(y[row0 + rl], v) : v;
        }
    } else if (rl < nrows) {
        y[row0 + rl] = ACC ? vadd(y[row0 + rl], acc) : acc;
    }
}

// rows per block of the LDS-staged kernels so that R*mean_row entries fit one LDS window, and whether EVERY block's slice
// does (blocks whose slice exceeds the window take the window-by-window kernel); scanned once per (matrix, R)
template <class V>
static int lds_shape(const CsrPart &P, int variant, double mean_row, hipStream_t s, int *R_out, bool *onewin)
{
    const int n = P.n_rows;
    const double cap = LdsCfg<V>::CH - 64;
    const int R = variant < -1 ? -variant
                               : (256 * mean_row <= cap ? 256 : 128 * mean_row <= cap ? 128 : 64 * mean_row <= cap ? 64
                                  : 32 * mean_row <= cap ? 32 : 16);
    if (P.slice_R != R) {
        int *d = nullptr, h = 0;
        HIPCHK(hipMalloc(&d, sizeof(int)));
        HIPCHK(hipMemsetAsync(d, 0, sizeof(int), s));
        const int nb = (n + R - 1) / R;
        hipLaunchKernelGGL(k_max_slice, dim3((nb + VB - 1) / VB), dim3(VB), 0, s, n, R, P.rowptr, d);
        hipError_t e = hipMemcpyAsync(&h, d, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        hipFree(d);
        if (e != hipSuccess) return fail(e, "slice scan", __FILE__, __LINE__);
        P.slice_R = R; P.max_slice = h;
    }
    *R_out = R;
    *onewin = P.padded && P.max_slice <= LdsCfg<V>::CH;
    return 0;
}

// (Ax, AxChoice: what one part's A.x runs -- csr_plan.hpp)
enum class AxAsk { product, dot, part_dot };        // who asks: spmv_dispatch, csr_ax_dot, csr_part_ax_dot

// The kernel a part's A.x takes: DESIGN 3.6's rules in order, the first that holds decides.  `push`: a shard's pushing blocks ride
// in front.  The dot askers then map the choice to the dot forms they take (csr_ax_dot, part_dot_launch); anything else: no dot.
// The plans below are built by the first call that consults them and are fixed from then on, so each is consulted under the same
// conditions and in the same order as always -- these accidents included (kept on purpose):
//  - packed_build is one-shot: the first of runs-only (R = 256 / 128, run1) and full (packed_ready: R = 64 or 32 / 16) fixes
//    pk_state.  So are the slice scan of lds_shape (slice_R), ranges_chosen, binned_chosen, tiled_chosen (and ensure_dot_part).
//  - a part's dot consults neither lr_mode nor ranges, nor tries run1 or the long-row packed form; with pushing blocks neither it
//    nor the product consults binned: tiled is tried directly.  The single-GPU dot does not consult lr_mode.
//  - the dot askers leave at > 160 entries per row or misaligned arrays before binned, and where a slice exceeds the window
//    before packed_build.
//  - plain k_spmv_run1 takes rows of up to 30 entries, its dot form run1d up to 15 (csr_ax_dot).
//  - plain k_spmv_lds1 takes a smaller window only if real, not accumulating, one-window and >= 2^22 entries; lds1d never.
//  - long-row packed blocks, windowed, wave, binned, ranges and complex matrices never carry the dot.
// Nothing is cached across calls (set_kernel, set_packed and ranges_free would have to invalidate it).
template <class V, bool ACC>
static int ax_choose(const CsrPart &P, int variant, double mean_row, bool push, AxAsk ask, hipStream_t s, AxChoice &c)
{
    c = AxChoice();
    const bool dot = ask != AxAsk::product;
    const bool automatic = variant == 0 || variant == -1;
    if (P.n_rows <= 0 || (dot && !automatic)) return 0;
    const bool al16 = (((uintptr_t)P.val | (uintptr_t)P.col) & 15) == 0;
    const bool whole = !push && ask != AxAsk::part_dot;      // a whole matrix (or one of its ranges), not a shard's part
    if constexpr (sizeof(V) == 8 && !ACC) {
        if (ask == AxAsk::product && whole && P.lr_mode == 1) { c.family = Ax::long_rows; return 0; }    // a range of long rows (ranges_chosen, class 3)
        if (whole && automatic && ranges_chosen(P, s)) { c.family = Ax::ranges; return 0; }
        if (dot && (mean_row > 160.0 || !al16)) return 0;
        if (!push && automatic && binned_chosen(P, s)) { c.family = Ax::binned; return 0; }
        if (automatic && tiled_chosen(P, s)) { c.family = Ax::tiled; return 0; }
    }
    if (variant == 0) variant = (!al16 || mean_row > 160.0) ? (mean_row > 48 ? 64 : (mean_row > 24 ? 32 : (mean_row > 12 ? 16 : 8))) : -1;
    if (variant > 0) { c.family = Ax::wave; c.T = variant; return 0; }
    if (!al16) return fail(hipErrorInvalidValue, "LDS-staged A.x needs 16-byte aligned col/val", __FILE__, __LINE__);
    { int rc = lds_shape<V>(P, variant, mean_row, s, &c.R, &c.onewin); if (rc) return rc; }
    const int R = c.R;
    c.family = c.onewin ? Ax::lds1 : Ax::ldsw;
    c.win = LdsCfg<V>::CH;
    if constexpr (sizeof(V) == 8 && !ACC) {
        if (dot && !c.onewin) return 0;
        // short rows whose blocks of 64 are mostly runs: one wavefront per block, no staging (k_spmv_run1)
        // (its wavefront-private LDS is dynamic: 4 wavefronts x 64 rows x LP doubles must stay within the 64 KB a launch
        //  may ask for without further ado -- rows of up to 30 entries)
        if (whole && variant == -1 && (R == 256 || R == 128) && packed_build(P, s, true) && packed_maxrow(P) <= 30) { c.family = Ax::run1; return 0; }
        if ((R == PK_R && c.onewin && packed_ready(P, s)) ||
            (whole && (R == 32 || R == 16) && c.onewin && packed_ready(P, s, R))) {     // (long rows: ldsp_ns)
            c.family = R == PK_R ? Ax::ldsp : Ax::ldsp_long; c.ns = ldsp_ns(P, R); c.bits = packed_bits(P);
            c.win = pk_window(P.max_slice);                 // the smallest LDS window every block fits: more workgroups per CU
            return 0;
        }
        // (real matrices, large enough for the memory system to matter: the smallest LDS window every block fits -- 27-point stencil
        //  x 3 unknowns, 16 rows of 81 entries per block: 625 us with five workgroups per CU -> see DESIGN 3.1)
        if (c.onewin && P.nnz >= (1 << 22)) c.win = pk_window(P.max_slice);
    }
    return 0;
}

template <class V, bool ACC, bool PUSH = false>
static int spmv_dispatch(const CsrPart &P, int variant, double mean_row, const V *x, V *y, hipStream_t s,
                         const int *done, const PushPlan &pp = PushPlan())
{
    const int n = P.n_rows;
    const unsigned xb = PUSH ? (unsigned)(pp.nblocks + pp.nrecv) : 0u;       // pushing blocks in front of the grid, receiving blocks behind it
    const V *val = reinterpret_cast<const V *>(P.val);
    if (n == 0) {
        if (PUSH && xb > 0) {       // nothing to multiply, but the neighbours still wait for x and the flags
            hipLaunchKernelGGL((k_spmv_wave<V, 1, ACC, PUSH>), dim3(xb), dim3(VB), 0, s, 0, P.rowptr, P.col, val, x, y, done, pp);
            HIPCHK(hipGetLastError());
        }
        return 0;
    }
    AxChoice c;
    { int rc = ax_choose<V, ACC>(P, variant, mean_row, PUSH, AxAsk::product, s, c); if (rc) return rc; }
    if constexpr (sizeof(V) == 8 && !ACC) {
        const double *xd = reinterpret_cast<const double *>(x);
        double *yd = reinterpret_cast<double *>(y);
        switch (c.family) {
        case Ax::long_rows: return long_rows_launch(P, xd, yd, s, done);
        case Ax::ranges: {
            RangePlan *R = static_cast<RangePlan *>(P.rg_plan);
            bool changed = false;
            for (size_t i = 0; i < R->parts.size(); i++) {
                const CsrPart &Q = R->parts[i];
                int rc = spmv_dispatch<V, false, false>(Q, variant, Q.n_rows ? (double)Q.nnz / Q.n_rows : 0.0, x, y + R->r0[i], s, done);
                if (rc) return rc;
                if (Q.last_kernel != R->seen[i]) { R->seen[i] = Q.last_kernel; changed = true; }
            }
            if (changed) {
                R->desc.clear();
                for (size_t i = 0; i < R->parts.size(); i++) {
                    char buf[64];
                    std::snprintf(buf, sizeof buf, "%srows [%d, %d): ", i ? " | " : "", R->r0[i], R->r0[i] + R->parts[i].n_rows);
                    R->desc += buf; R->desc += R->parts[i].last_kernel;
                }
            }
            P.last_kernel = R->desc.c_str();
            return 0;
        }
        case Ax::binned:
            P.last_kernel = "k_bin_expand + k_bin_reduce (two-pass binned product, x and row sums in LDS)";
            return binned_launch(P, xd, yd, s, done);
        case Ax::tiled:     // (sharded rows, direct exchange: the tiled product carries the pushing blocks too)
            P.last_kernel = PUSH ? "k_tile_spmv (one-pass tiled product: x tiles and row sums in LDS) + pushing blocks"
                                 : "k_tile_spmv (one-pass tiled product: x tiles and row sums in LDS)";
            return tiled_launch(P, xd, yd, s, done, PUSH ? &pp : nullptr);
        case Ax::run1: return packed_run1_launch(P, c, xd, yd, s, done);
        case Ax::ldsp: return packed_ldsp_launch(P, c, xd, yd, s, done, PUSH ? &pp : nullptr);
        case Ax::ldsp_long:
            if constexpr (!PUSH) return packed_ldsp_long_launch(P, c, xd, yd, s, done);
            break;
        default: break;
        }
    }
    if (c.family == Ax::wave) {
        const bool ok = pick<1, 2, 4, 8, 16, 32, 64>(c.T, [&](auto T) {
            constexpr int TT = decltype(T)::value;
            hipLaunchKernelGGL((k_spmv_wave<V, TT, ACC, PUSH>), dim3((unsigned)(((long)n * TT + VB - 1) / VB) + xb), dim3(VB), 0, s,
                               n, P.rowptr, P.col, val, x, y, done, pp);
        });
        if (!ok) return fail(hipErrorInvalidValue, "bad A.x lanes-per-row", __FILE__, __LINE__);
        P.last_kernel = "k_spmv_wave (lanes per row, shuffle reduction)";
    } else {
        const long nnz = P.end_abs >= 0 ? P.end_abs : P.nnz;
        const bool ok = pick<256, 128, 64, 32, 16>(c.R, [&](auto R) {
            constexpr int RR = decltype(R)::value;
            const dim3 g((n + RR - 1) / RR + xb);
            if (!c.onewin)
                hipLaunchKernelGGL((k_spmv_ldsw<V, RR, ACC, PUSH>), g, dim3(VB), 0, s, n, nnz, P.rowptr, P.col, val, x, y, done, pp);
            else if constexpr (sizeof(V) == 8 && !ACC)
                pick<PK_CH_8, PK_CH_7, PK_CH_SMALL, LdsCfg<double>::CH>(c.win, [&](auto win) {
                    hipLaunchKernelGGL((k_spmv_lds1<V, RR, ACC, PUSH, decltype(win)::value>), g, dim3(VB), 0, s, n, nnz, P.rowptr, P.col,
                                       val, x, y, done, pp);
                });
            else
                hipLaunchKernelGGL((k_spmv_lds1<V, RR, ACC, PUSH>), g, dim3(VB), 0, s, n, nnz, P.rowptr, P.col, val, x, y, done, pp);
        });
        if (!ok) return fail(hipErrorInvalidValue, "bad LDS A.x rows-per-block", __FILE__, __LINE__);
        P.last_kernel = c.onewin ? "k_spmv_lds1 (LDS-staged CSR)" : "k_spmv_ldsw (LDS-staged CSR, windowed)";
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int spmv_launch(const CsrPart &P, bool is_complex, int variant, double mean_row, const double *x, double *y,
                bool accumulate, hipStream_t s, const int *done)
{
    if (is_complex) {
        auto xv = reinterpret_cast<const double2 *>(x);
        auto yv = reinterpret_cast<double2 *>(y);
        return accumulate ? spmv_dispatch<double2, true>(P, variant, mean_row, xv, yv, s, done)
                          : spmv_dispatch<double2, false>(P, variant, mean_row, xv, yv, s, done);
    }
    return accumulate ? spmv_dispatch<double, true>(P, variant, mean_row, x, y, s, done)
                      : spmv_dispatch<double, false>(P, variant, mean_row, x, y, s, done);
}

int spmv_launch_push(const CsrPart &P, bool is_complex, int variant, double mean_row, const double *x, double *y,
                     hipStream_t s, const int *done, const PushPlan &pp)
{
    if (is_complex)
        return spmv_dispatch<double2, false, true>(P, variant, mean_row, reinterpret_cast<const double2 *>(x),
                                                   reinterpret_cast<double2 *>(y), s, done, pp);
    return spmv_dispatch<double, false, true>(P, variant, mean_row, x, y, s, done, pp);
}

// The packed kernel (csr_packed.hip: packed_ldsp_dot_launch) or the tiled one carrying y.u (and y.y): one partial per block of 64 rows
// (per chunk) into a buffer of the part's own, folded to <= 512 sums by a second small kernel (dot_part_fold) into part[0 .. *slots)
// (y.y: part[AXP_CAP ..)) -- together they replace a pass over two vectors of the part's height.  pp != nullptr: the product of a row shard with its pushing blocks in front (comm.hip).  1 = launched, 0 = this
// part does not take the packed kernel (nothing was launched), < 0 failure.
// nofold != nullptr: the second stage is left to the caller (comm.hip folds the per-block sums in the kernel that finishes the
// shard's product anyway): *nofold = number of per-block sums waiting in P.dot_part, nothing is written to `part`.
bool ensure_dot_part(const CsrPart &P, long count)
{   // (the packed kernel leaves a sum per 64 rows, the tiled one per 1024: a part that changes family needs the larger buffer)
    if (P.dot_part && P.dot_cap >= count) return true;
    if (P.dot_part) { if (ctx().inited) (void)hipDeviceSynchronize(); (void)hipFree(P.dot_part); P.dot_part = nullptr; P.dot_cap = 0; }
    if (hipMalloc(&P.dot_part, sizeof(double) * 2 * (size_t)count) != hipSuccess) { (void)hipGetLastError(); P.dot_part = nullptr; return false; }
    P.dot_cap = count;
    return true;
}

// the dot forms a part's own buffer takes: the tiled product or k_spmv_ldsp<DOT>, as chosen
static int part_dot_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, const double *u, int yy, double *part,
                           int *slots, hipStream_t s, const int *done, const PushPlan *pp, int *nofold)
{
    int nsum = 0;
    if (c.family == Ax::tiled) {
        // the tiled product: one sum per chunk of 1024 rows (per consumer wavefront), folded like the packed kernel's per-block sums
        nsum = tiled_chunks(P);
        if (nsum <= 0 || !ensure_dot_part(P, nsum)) return 0;
        DotPlan dp; dp.u = u; dp.part = P.dot_part; dp.yy = yy; dp.stride = nsum;
        int rc = tiled_launch(P, x, y, s, done, pp, &dp);
        if (rc) return rc;
        P.last_kernel = pp ? "k_tile_spmv (one-pass tiled product: x tiles and row sums in LDS) + pushing blocks, carrying the dot that follows the product"
                           : "k_tile_spmv (one-pass tiled product: x tiles and row sums in LDS) carrying the dot that follows the product";
    } else if (c.family == Ax::ldsp) {
        int rc = packed_ldsp_dot_launch(P, c, x, y, u, yy, &nsum, s, done, pp);
        if (rc != 1) return rc;
    } else
        return 0;
    if (nofold) { *nofold = nsum; *slots = 0; return 1; }
    int rc = dot_part_fold(P, nsum, yy, part, slots, s, done);
    return rc ? rc : 1;
}

int csr_part_ax_dot(const CsrPart &P, int variant, double mean_row, const double *x, double *y, const double *u, int yy, double *part,
                    int *slots, hipStream_t s, const int *done, const PushPlan *pp, int *nofold)
{
    AxChoice c;
    { int rc = ax_choose<double, false>(P, variant, mean_row, pp != nullptr, AxAsk::part_dot, s, c); if (rc) return rc; }
    return part_dot_launch(P, c, x, y, u, yy, part, slots, s, done, pp, nofold);
}

// A.x with the dot(s) that follow it in the Krylov loops carried in the product (k_spmv_lds1d / k_spmv_ldsp<DOT> / k_spmv_run1d): real
// matrices, the LDS-staged one-window family.  Everything else answers 0 and the caller multiplies and reduces in two launches as before.
int csr_ax_dot(lcg_hip_csr *A, const double *x, double *y, const double *u, int yy, double *part, int *slots, hipStream_t s,
               const int *done)
{
    static const bool off = [] { const char *e = std::getenv("LCG_HIP_AX_DOT"); return e && atoi(e) == 0; }();
    if (off || !A || A->is_complex || A->c64 || A->n_rows <= 0) return 0;
    if (A->distributed) return dist_ax_dot(A, x, y, u, yy, part, slots);
    const CsrPart &P = A->main;
    const int n = P.n_rows;
    AxChoice c;
    { int rc = ax_choose<double, false>(P, A->variant, A->mean_row, false, AxAsk::dot, s, c); if (rc) return rc; }
    switch (c.family) {
    case Ax::tiled:
    case Ax::ldsp: return part_dot_launch(P, c, x, y, u, yy, part, slots, s, done, nullptr, nullptr);
    case Ax::run1: {
        // short-row stencils (k_spmv_run1d): rows of up to 15 entries; longer ones take k_spmv_lds1d below
        const int rc = packed_run1d_launch(P, c, x, y, u, yy, part, slots, s, done);
        if (rc) return rc;
        break;
    }
    case Ax::lds1: break;
    // (long rows -- blocks of 32 / 16 rows with packed columns, Ax::ldsp_long -- keep the dot as a pass of its own: carried in the
    //  product it cost 32 us on the 27-point stencil x 3 unknowns, 187,500 blocks of 16 rows, where the separate pass costs 7)
    default: return 0;      // (ranges, binned, windowed: the product alone)
    }
    // Where it pays (measured, scripts/ax_dot_lab.py + scripts/ab_small.py): systems whose iteration is a chain of kernel
    // latencies -- the product grows by ~0.6 us, a ~3 us pass and its launch go.  At 1M rows (3907 row blocks) the product grew by
    // 3.2 us and every block of the consuming pass re-added 3907 partials: 39.2 vs 38.5 us per PCG iteration, so from
    // 2048 row blocks on the separate pass stays.
    constexpr int maxblk = 2048;
    const int nblk = (n + c.R - 1) / c.R;
    if (nblk > maxblk) return 0;
    DotPlan dp; dp.u = u; dp.part = part; dp.yy = yy;
    const bool ok = pick<256, 128, 64, 32, 16>(c.R, [&](auto R) {
        hipLaunchKernelGGL((k_spmv_lds1d<decltype(R)::value>), dim3(nblk), dim3(VB), 0, s, n, P.rowptr, P.col, P.val, x, y, done, dp);
    });
    if (!ok) return 0;
    HIPCHK(hipGetLastError());
    P.last_kernel = "k_spmv_lds1d (LDS-staged CSR carrying the dot that follows the product)";
    *slots = nblk;
    return 1;
}

void free_part(CsrPart &P)
{
    long_rows_free(P);
    ranges_free(P);
    binned_free(P);
    tiled_free(P);
    if (P.owned) { hipFree(P.rowptr); hipFree(P.col); hipFree(P.val); }
    packed_free(P, true);
    if (P.dot_part) hipFree(P.dot_part);
    P = CsrPart();
}

} // namespace lcgh

using namespace lcgh;

namespace lcgh { void dist_free(lcg_hip_csr *A); }

extern "C" {

int lcg_hip_csr_create(lcg_hip_csr_t *out, int n_rows, int n_cols, int64_t nnz, const int *rowptr, const int *col,
                       const double *val, int is_complex, int mem, int adopt)
{
    if (!out || n_rows <= 0 || nnz < 0 || nnz > 0x7fffffffLL || !rowptr || !col || !val) return LCG_HIP_E_ARG;
    int rc = ensure_init(); if (rc) return rc;
    Ctx &c = ctx();
    lcg_hip_csr *A = new lcg_hip_csr();
    A->n_rows = n_rows; A->n_cols = n_cols; A->is_complex = is_complex != 0;
    A->mean_row = (double)nnz / n_rows;
    A->main.sym_whole = !A->is_complex;
    if (mem == LCG_HIP_MEM_DEVICE && adopt) {
        A->main.n_rows = n_rows; A->main.nnz = nnz; A->main.owned = false; A->main.padded = adopt == 2;
        A->main.n_cols = n_cols;
        A->main.rowptr = const_cast<int *>(rowptr); A->main.col = const_cast<int *>(col); A->main.val = const_cast<double *>(val);
    } else {
        rc = alloc_part(A->main, n_rows, nnz, A->is_complex);
        if (rc) { delete A; return rc; }
        A->main.n_cols = n_cols;
        const hipMemcpyKind kind = mem == LCG_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        hipError_t e = hipMemcpyAsync(A->main.rowptr, rowptr, sizeof(int) * ((size_t)n_rows + 1), kind, c.stream);
        if (e == hipSuccess && nnz) e = hipMemcpyAsync(A->main.col, col, sizeof(int) * (size_t)nnz, kind, c.stream);
        if (e == hipSuccess && nnz) e = hipMemcpyAsync(A->main.val, val, sizeof(double) * (is_complex ? 2 : 1) * (size_t)nnz, kind, c.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        if (e != hipSuccess) { free_part(A->main); delete A; return fail(e, "csr upload", __FILE__, __LINE__); }
    }
    *out = A;
    return 0;
}

int lcg_hip_csr_destroy(lcg_hip_csr_t A)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return 0;
    ctx().place.forget_all();     // (placement.hip remembers timings by the value array's address)
    ctx().place.gave_back((size_t)A->main.nnz * (A->is_complex ? 20 : 12));     // (site 5; the plans beside it not counted: the walk's "fresh allocator" rule needs the order of magnitude)
    dist_free(A);
    free_part(A->main);
    for (int i = 1; i < 4; i++) free_part(A->op[i]);
    normal_free(A);
    if (A->invdiag) hipFree(A->invdiag);
    tri_factor_free(A->ic0);
    tri_factor_free(A->ilu0);
    c64_free(A);
    A->kind = 0;
    delete A;
    return 0;
}

int lcg_hip_csr_rows(lcg_hip_csr_t A) { NOT_DENSE(A, LCG_HIP_E_ARG); return A ? A->n_rows : 0; }
int64_t lcg_hip_csr_nnz(lcg_hip_csr_t A) { NOT_DENSE(A, LCG_HIP_E_ARG); return A ? A->main.nnz : 0; }
int lcg_hip_csr_arrays(lcg_hip_csr_t A, const int **rowptr, const int **col, const double **val)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return LCG_HIP_E_ARG;
    if (rowptr) *rowptr = A->main.rowptr;
    if (col) *col = A->main.col;
    if (val) *val = A->main.val;
    return 0;
}
int lcg_hip_csr_set_kernel(lcg_hip_csr_t A, int variant)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_set_kernel");
    A->variant = variant;
    return 0;
}

} // extern "C"

// set_*(A, 0) is the first half of the rewrite protocol (lcg_hip.h): the transposed / conjugated copies (op_part) are made from the
// arrays too, so they go with the plans and are rebuilt from the new arrays at their next use.  So is the half store of a symmetric
// run stretch (csr_sym.hip), the one copy of VALUES the packed form keeps: it goes with ANY of the setters, and the plan it belongs
// to is built -- and its values compared -- again at the next product.  The normal state (csr_normal.hip) holds K^T and sums of
// squared values: it stays, marked stale, and the next entry that needs it builds it again from the arrays as they are then.
void lcgh::op_copies_free(lcg_hip_csr *A)      // (csr_plan.hpp: the packed family's setters call it too)
{
    normal_stale(A);
    if (sym_runs_bytes(A->main) > 0 || std::strncmp(A->main.sym_why, "refused", 7) == 0) sym_runs_reset(A->main);      // (refused values may mirror each other now)
    if (!A->op[1].rowptr && !A->op[2].rowptr && !A->op[3].rowptr) return;
    if (ctx().inited) (void)hipDeviceSynchronize();
    for (int i = 1; i < 4; i++) free_part(A->op[i]);
}

extern "C" {

int lcg_hip_csr_set_binned(lcg_hip_csr_t A, int mode)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || mode < -1 || mode > 1) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_set_binned");
    if (mode == 0) op_copies_free(A);
    for (CsrPart *P : {&A->main, &A->loc}) {
        P->bn_mode = mode;
        ranges_free(*P);                    // the ranges inherit the modes: cut again at the next product
        if (mode == 0) binned_free(*P);     // gives the plan's memory back
        else P->bn_state = 0;               // decide again at the next product (a plan that exists is kept and reused)
    }
    return 0;
}

int lcg_hip_csr_set_tiled(lcg_hip_csr_t A, int mode)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || mode < -1 || mode > 1) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_set_tiled");
    if (mode == 0) op_copies_free(A);
    for (CsrPart *P : {&A->main, &A->loc}) {
        P->tl_mode = mode;
        ranges_free(*P);                    // the ranges inherit the modes: cut again at the next product
        if (mode == 0) tiled_free(*P);
        else P->tl_state = 0;               // decide again at the next product (a plan that exists is kept and reused)
    }
    return 0;
}

int lcg_hip_csr_set_ranges(lcg_hip_csr_t A, int mode)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || mode < -1 || mode > 1) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_set_ranges");
    if (mode == 0) op_copies_free(A);
    if (ctx().inited) (void)hipDeviceSynchronize();
    for (CsrPart *P : {&A->main, &A->loc}) { ranges_free(*P); P->rg_mode = mode; }
    return 0;
}

int lcg_hip_csr_ranges(lcg_hip_csr_t A, int cap, int *first_row)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return 0;
    const CsrPart &P = A->distributed ? A->loc : A->main;
    const RangePlan *R = static_cast<const RangePlan *>(P.rg_plan);
    if (!R || P.rg_state <= 0) return 0;
    for (int i = 0; i < cap && i < (int)R->r0.size() && first_row; i++) first_row[i] = R->r0[i];
    return (int)R->r0.size();
}

const char *lcg_hip_csr_tiled_status(lcg_hip_csr_t A)
{
    NOT_DENSE(A, "");
    if (!A) return "";
    return A->distributed ? A->loc.tl_why : A->main.tl_why;
}

const char *lcg_hip_csr_last_kernel(lcg_hip_csr_t A)
{
    NOT_DENSE(A, "");
    if (!A) return "";
    return A->distributed ? A->loc.last_kernel : A->main.last_kernel;
}

const char *lcg_hip_csr_binned_status(lcg_hip_csr_t A)
{
    NOT_DENSE(A, "");
    if (!A) return "";
    return A->distributed ? A->loc.bn_why : A->main.bn_why;
}

static int64_t part_traffic_model(const CsrPart &P)
{
    const char *k = P.last_kernel;
    if (!k || !*k) return 0;
    if (P.rg_state > 0 && P.rg_plan) {      // range by range; x is counted once
        const RangePlan *R = static_cast<const RangePlan *>(P.rg_plan);
        int64_t b = 0;
        const int64_t xbytes = 8 * (P.n_cols > 0 ? P.n_cols : (int64_t)P.n_rows);
        for (const CsrPart &Q : R->parts) b += part_traffic_model(Q) - xbytes;
        return b + xbytes;
    }
    const int64_t n = P.n_rows, ncols = P.n_cols > 0 ? P.n_cols : P.n_rows;
    const int64_t vectors = 4 * (n + 1) + 8 * ncols + 8 * n;       // row pointers, x once, y
    if (std::strncmp(k, "k_lr_", 5) == 0) return 12 * P.nnz + vectors;       // CSR as it is, the chunk lists are small
    if (std::strncmp(k, "k_bin_", 6) == 0) return binned_traffic_bytes(P);
    if (std::strncmp(k, "k_tile", 6) == 0) return tiled_traffic_bytes(P);
    if (std::strncmp(k, "k_spmv_ldsp", 11) == 0 || std::strncmp(k, "k_spmv_run1", 11) == 0) return packed_traffic_bytes(P, k) + vectors;
    return 12 * P.nnz + vectors;                       // the CSR arrays as they are
}

int64_t lcg_hip_csr_last_traffic_model(lcg_hip_csr_t A)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || A->is_complex || A->c64) return 0;
    return part_traffic_model(A->distributed ? A->loc : A->main);
}

int lcg_hip_csr_plan_info(lcg_hip_csr_t A, double *build_ms, int64_t *extra_bytes)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return LCG_HIP_E_ARG;
    const CsrPart &P = A->distributed ? A->loc : A->main;
    double ms = P.plan_ms;
    int64_t b = 0;
    auto add = [&](const CsrPart &Q) {
        b += packed_plan_bytes(Q);          // with the stretches' tables and a symmetric stretch's half store
        if (Q.bn_plan) b += (int64_t)binned_plan_bytes(Q);
        if (Q.tl_plan) b += (int64_t)tiled_plan_bytes(Q);
    };
    add(P);
    if (P.rg_state > 0 && P.rg_plan)
        for (const CsrPart &Q : static_cast<const RangePlan *>(P.rg_plan)->parts) { add(Q); ms += Q.plan_ms; }
    if (build_ms) *build_ms = ms;
    if (extra_bytes) *extra_bytes = b;
    return 0;
}

// ---- callbacks -------------------------------------------------------------------------------
// The callback types return void (lcg.h:37-38, clcg.h:40-41): a failure is parked in Ctx::ax_rc, where the solver
// loop picks it up right after the call (driver.hpp: timed_ax / checked_mx) and ends the solve with that code.
static inline void park(int rc) { if (rc && !ctx().ax_rc) ctx().ax_rc = rc; }

void lcg_hip_csr_ax(void *instance, const double *x, double *y, const int n)
{
    NOT_DENSE_CB(instance);
    lcg_hip_csr *A = static_cast<lcg_hip_csr *>(instance);
    (void)n;
    park(lcg_hip_spmv(A, x, y));
}

void clcg_hip_csr_ax(void *instance, const double *x, double *y, const int n, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    (void)n;
    park(lcg_hip_spmv_op(static_cast<lcg_hip_csr *>(instance), x, y, layout, conjugate));
}

void lcg_hip_jacobi_mx(void *instance, const double *x, double *z, const int n)
{
    NOT_DENSE_CB(instance);
    park(jacobi_launch(static_cast<lcg_hip_csr *>(instance), x, z, n, ctx().stream));
}

int lcg_hip_spmv_op(lcg_hip_csr_t A, const double *x, double *y, int layout, int conjugate)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || !x || !y) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_spmv_op");
    if (!layout && (!conjugate || !A->is_complex)) return lcg_hip_spmv(A, x, y);
    Ctx &c = ctx();
    const CsrPart *P = nullptr;
    int rc = op_part(A, layout, conjugate, &P);
    if (rc) return rc;
    if (A->distributed) return dist_spmv_op(A, *P, x, y);
    return spmv_launch(*P, A->is_complex, A->variant, A->mean_row, x, y, false, c.stream,
                       ax_flag(c));
}


int lcg_hip_spmv(lcg_hip_csr_t A, const double *x, double *y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || !x || !y) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_spmv");
    Ctx &c = ctx();
    if (A->distributed) return dist_spmv(A, x, y);
    return spmv_launch(A->main, A->is_complex, A->variant, A->mean_row, x, y, false, c.stream,
                       ax_flag(c));
}

} // extern "C"
