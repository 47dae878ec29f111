// csr_packed.hip -- the packed row-block product of real fp64 CSR parts: its plan (PackedPlan, csr_plan.hpp) built on the device
// at the first product and owned here, its kernels, its launches, its setters and queries of the handle's C ABI.
//
//  k_pk_*           the build: per block of 64 (32 / 16) rows the form it takes -- packed block-relative columns (18 / 21 bits), a RUN
//      block (row 0's columns only), a TEMPLATE block (<= 64 diagonals and a mask per row) -- and the stretches of run blocks.
//  k_spmv_ldsp      k_spmv_lds1's mapping (csr.hip) over that plan: the headline's kernel.  <DOT>: carries the
//      dot that follows the product, folded by k_axp_fold.  The sliced range of a symmetric run stretch: k_spmv_ldsp_sym, csr_sym.hip.
//  k_spmv_run1 / k_spmv_run1d   short rows (stencils) whose blocks are runs: one wavefront per 64-row block, no barrier.
//
// Which part takes which: ax_choose (csr.hip), which asks this file through csr_plan.hpp and reads no field of the plan.  The plan's
// memory is released in ONE place, packed_free; the sites that call it say where their effect differs from it.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "csr_plan.hpp"

namespace lcgh {

// ---- packed columns ----------------------------------------------------------------------------
// The one lever left on the stream itself: a block of 64 rows stores its columns relative to the
// block's smallest column, six 21-bit fields per 16 bytes (2.67 instead of 4 B per entry: 10.67
// instead of 12 B of stream per entry), unpacked on the way into LDS.  Same row mapping and the
// same summation order as k_spmv_lds1 (bit-identical y), eight gathers in flight per lane.
// Measured on the headline system: 0.686 vs 0.719 ms (-4.6 %).  Costs 0.87 GB beside the plain
// `col` (which the other operations keep using), built on the device at the first product.
typedef unsigned long long u64;
typedef int v2i __attribute__((ext_vector_type(2)));
constexpr int PK_SPAN = 1 << 21;

// A RUN block (round 2, third session): every row of the block has the same number of entries L and every entry's column is
// one more than the entry in the same slot of the row above -- the shape of constant diagonals and stencils away from the
// matrix edges.  Such a block needs no columns of its own beyond row 0's: column(row r, slot k) = column(row 0, slot k) + r.
// It stores row 0's L columns as plain int32 (four per 16-byte group) and is marked by base[b] = -1 - L.
// A TEMPLATE block (round 3): what a stencil's blocks look like where the grid's boundaries pass through them.  The rows do not
// all hold the same entries any more, but every entry of the block lies on one of D <= 64 diagonals (column - row in block) -- the
// union of its rows' --, no row holds more than 32 entries, and every row holds them in ascending column order.  Such a block stores the D
// offsets and one 64-bit mask per row (which diagonals the row has) -- 39 groups of 16 bytes for a 27-point stencil instead of ~250 -- and is
// marked by base[b] = -(1 << 30) - D.  (Stencils with several unknowns per grid point need the width: 7 neighbours x 3 unknowns lie on 35.)  Run blocks are the special case "all masks full"; they keep their own, cheaper, form.
constexpr int TPL_MAXD = 64;         // diagonals of a template block (one bit each in a row's 64-bit mask)
constexpr int TPL_MAXROW = 32;       // longest row of a template block (the packed kernel takes a row in ONE predicated batch of UNR * T >= 32 entries)
constexpr int TPL_CODE = 1 << 30;       // base[b] = -TPL_CODE - D; ngroups[b] (before k_pk_groups) = -TPL_GRP - D
constexpr int TPL_GRP = 1 << 20;

// The build kernels below (k_pk_meta, k_pk_pack through tpl_row_mask) call HIP's __shfl_down with the constant width 64, and they
// are its only callers in this file.  The compiler then folds that width into the helper itself before it inlines it and emits
// other (equivalent) instructions than it did while k_spmv_wave's run-time widths shared the translation unit (csr.hip).  One kept
// caller with a run-time width leaves the helper general, so the build kernels stay instruction for instruction the code they were
// when they shared a file with k_spmv_wave.  Never called; no kernel.
__device__ __attribute__((used)) int shfl_down_any_width(int v, unsigned delta, int width) { return __shfl_down(v, delta, width); }

// One wavefront, lane = row of the block: builds tpl[0 .. D) = the ascending offsets (column - row in block) the block's entries
// lie on -- seeded with the longest row's, then completed by the rows that have others (a block that holds the last line of one
// grid plane and the first line of the next has rows that miss DIFFERENT neighbours) -- and returns the lane's mask over them;
// *bad when there are more than TPL_MAXD of them or a row's columns do not ascend.  tpl: TPL_MAXD + 1 ints of LDS, dcount: one.
__device__ __forceinline__ unsigned long long tpl_row_mask(long row0, int r1, const int *__restrict__ rowptr, const int *__restrict__ col, int *tpl,
                                                 int *dcount, int *D_out, bool *bad)
{
    const int lane = threadIdx.x & 63;
    const long row = row0 + lane;
    int s = 0, len = 0;
    if (row < r1) { s = rowptr[row]; len = rowptr[row + 1] - s; }
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    // the longest row (first of them) seeds the template
    int best = len, who = lane;
    for (int off = 32; off > 0; off >>= 1) {
        const int ob = __shfl_down(best, off, 64), ow = __shfl_down(who, off, 64);
        if (ob > best || (ob == best && ow < who)) { best = ob; who = ow; }
    }
    best = __shfl(best, 0, 64); who = __shfl(who, 0, 64);
    *D_out = best;
    *bad = true;
    if (best < 1 || best > TPL_MAXROW) return 0ull;
    bool mine_bad = false;
    {   // columns must ascend strictly: entry e of a row is then the e-th set bit of its mask
        int prev = -0x7fffffff - 1;
        for (int k = 0; k < len; k++) { const int c = col[s + k]; if (c <= prev) mine_bad = true; prev = c; }
    }
    if (__ballot(mine_bad)) return 0ull;
    if (lane == who) { for (int k = 0; k < len; k++) tpl[k] = col[s + k] - lane; *dcount = len; }
    wave_sync();
    auto find = [&](int o, int D) {     // index of o in tpl[0 .. D), or -1
        int lo = 0, hi = D - 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (tpl[mid] < o) lo = mid + 1; else hi = mid; }
        return tpl[lo] == o ? lo : -1;
    };
    for (int round = 0; round < 64; round++) {      // every round takes in one more row's offsets: at most 64
        const int D = *dcount;
        bool missing = false;
        for (int k = 0; k < len && !missing; k++) missing = find(col[s + k] - lane, D) < 0;
        const unsigned long long m = __ballot(missing);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        if (lane == leader) {
            int Dn = D;
            for (int k = 0; k < len; k++) {
                const int o = col[s + k] - lane;
                if (find(o, Dn) >= 0) continue;
                if (Dn >= TPL_MAXD) { Dn = TPL_MAXD + 1; break; }
                int p = Dn;
                while (p > 0 && tpl[p - 1] > o) { tpl[p] = tpl[p - 1]; p--; }
                tpl[p] = o; Dn++;
            }
            *dcount = Dn;
        }
        wave_sync();
        if (*dcount > TPL_MAXD) return 0ull;
    }
    const int D = *dcount;
    *D_out = D;
    unsigned long long mask = 0ull;
    bool b = false;
    for (int k = 0; k < len; k++) { const int p = find(col[s + k] - lane, D); if (p >= 0) mask |= 1ull << p; else b = true; }
    *bad = __ballot(b) != 0ull;
    return mask;
}

__global__ __launch_bounds__(64) void k_pk_meta(int n, const int *rowptr, const int *col, int *base, int *ngroups, int *maxspan, int runs, int R)
{   // ngroups[b] = entries of block b for now, -L for a run block, -TPL_GRP - D for a template block (k_pk_groups turns them into groups);
    // maxspan[0] = widest block, [1] = longest row, [2] = run blocks, [3] = template blocks
    // R: rows per block -- 64, or 32 / 16 for long rows (then runs == 0: run and template blocks are shapes of 64 rows, one per lane)
    __shared__ int tpl[TPL_MAXD + 1], dcount;
    const int b = blockIdx.x;
    const long row0 = (long)b * R;
    const int r1 = (int)min((long)n, row0 + R);
    const int s = rowptr[row0], e = rowptr[r1];
    int lo = 0x7fffffff, hi = 0;
    for (int k = s + threadIdx.x; k < e; k += 64) { const int c = col[k]; lo = min(lo, c); hi = max(hi, c); }
    int len = 0, lmin = 0x7fffffff;
    if (row0 + threadIdx.x < r1) { len = rowptr[row0 + threadIdx.x + 1] - rowptr[row0 + threadIdx.x]; lmin = len; }
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_down(lo, off, 64)); hi = max(hi, __shfl_down(hi, off, 64)); len = max(len, __shfl_down(len, off, 64));
        lmin = min(lmin, __shfl_down(lmin, off, 64));
    }
    const int L = __shfl(len, 0, 64), Lmin = __shfl(lmin, 0, 64);
    int run = runs && L == Lmin && L > 0 && L <= 0x3fffffff;
    if (run) {      // uniform
        int bad = 0;
        for (int k = s + L + threadIdx.x; k < e; k += 64) bad |= col[k] != col[k - L] + 1;
        run = __ballot(bad) == 0;
    }
    int D = 0;
    bool tplb = false;
    if (!run && runs == 1 && e > s) {       // uniform (runs == 2: run blocks only; packed_build never asks for that)
        bool bad;
        (void)tpl_row_mask(row0, r1, rowptr, col, tpl, &dcount, &D, &bad);
        tplb = !bad;        // (uniform)
    }
    if (threadIdx.x == 0) {
        if (e == s) { lo = 0; hi = 0; }
        base[b] = run ? -1 - L : (tplb ? -TPL_CODE - D : lo);
        ngroups[b] = run ? -L : (tplb ? -TPL_GRP - D : e - s);
        if (!tplb && !run) atomicMax(maxspan, hi - lo);     // (only the blocks that keep packed columns store them relative to their smallest)
        atomicMax(maxspan + 1, L);
        if (run) atomicAdd(maxspan + 2, 1);
        if (tplb) atomicAdd(maxspan + 3, 1);
    }
}

__global__ void k_pk_groups(int nb, int per, int *ngroups)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nb) {
        const int g = ngroups[b];
        // (a template block: its D offsets, then a mask per row -- 32 bits wide up to 32 diagonals, 64 beyond)
        // (a run block: row 0's L columns and, behind them, the slot of the block's own diagonal)
        ngroups[b] = g <= -TPL_GRP ? (-g - TPL_GRP + 1 + 3) / 4 + (-g - TPL_GRP <= 32 ? PK_R / 4 : PK_R / 2)
                                   : (g < 0 ? (-g + 1 + 3) / 4 : (per > 0 ? (g + per - 1) / per : 0));
    }
}

// Field j of a 128-bit group (lo, hi): BITS = 21 -> six fields, three per 64-bit half; BITS = 18 -> seven
// fields, the fourth straddling the halves.
template <int BITS> __device__ __forceinline__ int pk_field(u64 lo, u64 hi, int j);
template <> __device__ __forceinline__ int pk_field<21>(u64 lo, u64 hi, int j)
{
    return (int)(((j < 3 ? lo : hi) >> (21 * (j % 3))) & 0x1fffff);
}
template <> __device__ __forceinline__ int pk_field<18>(u64 lo, u64 hi, int j)
{
    const int sh = 18 * j;
    const u64 v = sh + 18 <= 64 ? lo >> sh : (sh >= 64 ? hi >> (sh - 64) : (lo >> sh) | (hi << (64 - sh)));
    return (int)(v & 0x3ffff);
}

// Several unknowns per grid point (a 27-point stencil x 3: 81 entries per row): every row's entries come in groups of g consecutive
// columns -- the g x g coupling block of two points.  ok[g - 2] stays 1 when EVERY row is made of such groups (g = 2, 3, 4): the packed
// form of the long-row blocks then keeps one column field per group (18 bits for three entries: 8.75 instead of 10.3 B per entry).
__global__ __launch_bounds__(VB) void k_pk_dof(int n, const int *__restrict__ rowptr, const int *__restrict__ col, int *ok)
{
    const int i = blockIdx.x * VB + threadIdx.x;
    unsigned bad = 0;       // bit g - 2
    if (i < n) {
        const int s = rowptr[i], len = rowptr[i + 1] - s;
        bad = (len % 2 != 0 ? 1u : 0u) | (len % 3 != 0 ? 2u : 0u) | (len % 4 != 0 ? 4u : 0u);
        int prev = len > 0 ? col[s] : 0;
        for (int k = 1; k < len && bad != 7u; k++) {        // one walk for the three group sizes
            const int c = col[s + k];
            if (c != prev + 1) bad |= (k % 2 != 0 ? 1u : 0u) | (k % 3 != 0 ? 2u : 0u) | (k % 4 != 0 ? 4u : 0u);
            prev = c;
        }
    }
    for (int g = 0; g < 3; g++) if (__ballot((bad >> g) & 1u) != 0ull && (threadIdx.x & 63) == 0) ok[g] = 0;
}

template <int BITS>
__global__ __launch_bounds__(VB) void k_pk_pack(int n, const int *rowptr, const int *col, const int *base, const int *pofs, v4i *packed, int R, int dof)
{
    constexpr int PER = BITS > 0 ? 128 / BITS : 1;
    const int b = blockIdx.x;
    const long row0 = (long)b * R;
    const int r1 = (int)min((long)n, row0 + R);
    const int s = rowptr[row0], e = rowptr[r1];
    const int bs = base[b];
    if (BITS == 0 && bs >= 0) return;       // runs only: the other blocks keep nothing
    if (bs <= -TPL_CODE) {   // template block: the D offsets (padded to whole groups), then the 64 row masks
        __shared__ int tpl[TPL_MAXD + 1], dcount;
        if (threadIdx.x < 64) {
            int D; bool bad;
            const unsigned long long m = tpl_row_mask(row0, r1, rowptr, col, tpl, &dcount, &D, &bad);
            int *dst = reinterpret_cast<int *>(packed + pofs[b]);
            const int Dp = (D + 1 + 3) & ~3;
            // behind the D offsets: which of them is the block's own diagonal (offset = the block's first row) when EVERY row of the block
            // has it, else -1 -- k_spmv_ldsp<DOT> then takes u = x from the gathers (as for run blocks)
            int idg = -1;
            for (int i = 0; i < D; i++) if (tpl[i] == (int)row0) idg = i;
            const bool lacks = idg < 0 || (row0 + (long)threadIdx.x < r1 && !((m >> idg) & 1ull));
            if (__ballot(lacks)) idg = -1;
            if ((int)threadIdx.x < D) dst[threadIdx.x] = tpl[threadIdx.x];
            if (threadIdx.x == 0) { dst[D] = idg; for (int i = D + 1; i < Dp; i++) dst[i] = 0; }      // (D may be 64: one lane writes the tail)
            if (D <= 32) reinterpret_cast<unsigned *>(dst + Dp)[threadIdx.x] = (unsigned)m;
            else reinterpret_cast<unsigned long long *>(dst + Dp)[threadIdx.x] = m;      // (Dp ints = whole 16-byte groups: aligned)
        }
        return;
    }
    if (bs < 0) {       // run block: row 0's columns as they are
        const int L = -1 - bs;
        int *dst = reinterpret_cast<int *>(packed + pofs[b]);
        // behind them: the slot whose column is the block's first row (every row's diagonal, then), or -1: k_spmv_ldsp<DOT> takes u = x from it
        __shared__ int kd;
        if (threadIdx.x == 0) kd = -1;
        __syncthreads();
        for (int k = threadIdx.x; k < L; k += VB) if (col[s + k] == (int)row0) kd = k;       // (columns ascend: one match at most)
        __syncthreads();
        for (int k = threadIdx.x; k < ((L + 1 + 3) & ~3); k += VB) dst[k] = k < L ? col[s + k] : (k == L ? kd : 0);
        return;
    }
    const int ng = (e - s + PER * dof - 1) / (PER * dof);       // (dof > 1: a field is the first column of a group of dof entries)
    for (int g = threadIdx.x; g < ng; g += VB) {
        u64 lo = 0, hi = 0;
        for (int j = 0; j < PER; j++) {
            const int k = s + (PER * g + j) * dof;
            const u64 c = k < e ? (u64)(col[k] - bs) : 0;
            if (BITS == 21) { if (j < 3) lo |= c << (21 * j); else hi |= c << (21 * (j - 3)); }
            else if (BITS > 0) {
                const int sh = BITS * j;
                if (sh < 64) { lo |= c << sh; if (sh + BITS > 64) hi |= c >> (64 - sh); }
                else hi |= c << (sh - 64);
            }
        }
        v4i o; o.x = (int)(unsigned)lo; o.y = (int)(unsigned)(lo >> 32); o.z = (int)(unsigned)hi; o.w = (int)(unsigned)(hi >> 32);
        packed[pofs[b] + g] = o;
    }
}

// Stretches of run blocks (internal.hpp: RunStretches).  flag[b]: 0 = block b can be in no stretch (not a run block, or the partial
// last block), L = a full run block of L entries per row, -L = one that CONTINUES the stretch of block b - 1: the same L, row 0's
// columns those of block b - 1 plus 64 (the same offsets from the block's first row -- and with them the same slot of the diagonal),
// its entries right behind that block's.  One thread per block: 2 L small reads, once per plan.
__global__ __launch_bounds__(VB) void k_pk_stretch_flags(int n, int nb, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                         const int *__restrict__ base, int *__restrict__ flag)
{
    const int b = blockIdx.x * VB + threadIdx.x;
    if (b >= nb) return;
    const int bs = base[b];
    int f = 0;
    if (bs < 0 && bs > -TPL_CODE && (long)b * PK_R + PK_R <= (long)n) {
        const int L = -1 - bs;
        f = L;
        if (b > 0 && base[b - 1] == bs) {
            const int s = rowptr[(long)b * PK_R], sp = rowptr[(long)(b - 1) * PK_R];
            bool same = (long)s == (long)sp + (long)PK_R * L;
            for (int k = 0; k < L && same; k++) same = col[s + k] - PK_R == col[sp + k];
            if (same) f = -L;
        }
    }
    flag[b] = f;
}

// Block i writes the table of stretch i (offset of slot k = column(row 0, k) - first row of its first block, at [(k % 4) * Q + k / 4]:
// the slots of one wavefront of k_spmv_ldsp side by side, zeros behind the L-th; the tables lie behind each other) and leaves
// out[2 i] = the first entry of the stretch, out[2 i + 1] = the slot whose offset is 0 (every row's diagonal; -1: none), which is
// what k_pk_pack keeps behind the columns of each of its blocks.
__global__ __launch_bounds__(64) void k_pk_stretch_fill(RunStretches rs, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                        int *__restrict__ off, int *__restrict__ out)
{
    __shared__ int kd;
    int o = 0, L = 0, Q = 1, b0 = 0;
#pragma unroll
    for (int j = 0; j < RS_MAX; j++) {
        if (j < (int)blockIdx.x) o += 4 * rs.s[j].Q;
        if (j == (int)blockIdx.x) { L = rs.s[j].L; Q = rs.s[j].Q; b0 = rs.s[j].b0; }
    }
    const long row0 = (long)b0 * PK_R;
    const int s = rowptr[row0];
    if (threadIdx.x == 0) kd = -1;
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * Q; i += 64) {
        const int k = i / Q + 4 * (i % Q);
        const int d = k < L ? col[s + k] - (int)row0 : 0;
        off[o + i] = d;
        if (k < L && d == 0) kd = k;
    }
    __syncthreads();
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = s; out[2 * blockIdx.x + 1] = kd; }
}

// NS: gathers a lane keeps in flight.  NS = 8: batches of 8 while they are full, then one by one.
// NS > 8: the FIRST batch is predicated (slots past the row's end read entry 0 with a zero
// coefficient), so rows of up to NS*T entries -- 33 entries on 4 lanes are 9 for one lane, 8 for the
// others -- are done in one round without a serial tail (0.706 vs 0.722 ms on the headline system).
// (end of a block of k_spmv_ldsp<DOT>: ldsp_dot_tail, csr_plan.hpp)
// DOT: the block also leaves its rows' share of y.u (and y.y) in dp.part[block] (dp.part[dp.stride + block]): the dot the
// Krylov loops take right after the product, without a pass of its own over two 80 MB vectors (see k_spmv_lds1d; here one
// partial per block of 64 rows, folded to <= 512 by k_axp_fold before the scalar step adds them up).
// CHE: entries a block holds at most -- the LDS window, about 12 bytes per entry.  With the 2240 entries the shapes are chosen for a
// workgroup asks for 26.9 KB and FIVE fit a CU (the LDS is handed out in granules: six would need <= 26.6 KB each).  Where every
// block of the matrix is smaller the window shrinks: 2208 entries (26.5 KB, six workgroups per CU: the headline's 64 x 33 -- same-box
// A/B 1477 -> 1498 CG iterations/s, 6 of 6 runs), 1872 (22.5 KB, seven: a 27-point stencil's 64 x 27 -- product 401 -> 374 us with
// six already), 1696 (20.4 KB, eight: rows of up to 26 entries).  (PK_CH_SMALL, PK_CH_7, PK_CH_8: csr_plan.hpp)
int pk_window(int max_slice)
{
    static const int env = [] { const char *e = std::getenv("LCG_HIP_PACKED_WINDOW"); return e ? atoi(e) : 0; }();     // A/B runs: least window
    const int need = std::max(max_slice, env);
    return need <= PK_CH_8 ? PK_CH_8 : need <= PK_CH_7 ? PK_CH_7 : need <= PK_CH_SMALL ? PK_CH_SMALL : LdsCfg<double>::CH;
}
// RR: rows per block.  64 (T = 4 lanes per row) for rows of up to ~34 entries; 32 / 16 (T = 8 / 16) for longer rows -- packed columns
// only, the first batch predicated for ANY NS (round 3, late: 27-point stencils with 2 / 3 unknowns per point, 54 / 81 entries per row,
// took the 12-byte k_spmv_lds1 before).
// SKIP: the grid leaves out the blocks [st.skip_from, st.skip_from + st.skip) -- the sliced range of a symmetric stretch, which
// k_spmv_ldsp_sym multiplies (csr_sym.hip) -- so that ONE launch takes the blocks in front of it and behind it.  Instances of their
// own: those without it are the code they were.
struct RunStretchesSkip : RunStretches { int skip_from = 0, skip = 0; };
template <bool PUSH, int NS, int BITS, bool DOT = false, int CHE = LdsCfg<double>::CH, int RR = PK_R, bool SKIP = false>
__global__ __launch_bounds__(VB) void k_spmv_ldsp(int n, const int *__restrict__ rowptr, const v4i *__restrict__ packed,
                                                  const int *__restrict__ pofs, const int *__restrict__ pbase,
                                                  const double *__restrict__ val, const double *__restrict__ x,
                                                  double *__restrict__ y, const int *done, PushPlan pp, DotPlan dp,
                                                  typename std::conditional<SKIP, RunStretchesSkip, RunStretches>::type st)
{
    if (PUSH && (int)blockIdx.x < pp.nblocks) { push_block(pp, blockIdx.x); return; }
    if (PUSH && pp.nrecv > 0 && (int)blockIdx.x >= (int)gridDim.x - pp.nrecv) { recv_block(pp, (int)blockIdx.x - ((int)gridDim.x - pp.nrecv)); return; }
    int bid = PUSH ? blockIdx.x - pp.nblocks : blockIdx.x;
    if constexpr (SKIP) { if (bid >= st.skip_from) bid += st.skip; }
    constexpr int R = RR;
    constexpr int T = VB / R;
    constexpr int UNR = NS;
    constexpr int CH = CHE;                             // entries per block at most (checked by the host)
    constexpr int PER = 128 / BITS;                     // columns per 16-byte group: 6 (21 bits) or 7 (18 bits)
    constexpr int NG = (CH + PER - 1) / PER;            // groups
    constexpr int GR = (NG + VB - 1) / VB;              // rounds of 16-byte group loads
    constexpr int VR = (CH / 2 + 1 + VB - 1) / VB;      // rounds of 16-byte val loads
    __shared__ __attribute__((aligned(16))) double sval[CH + 2];
    __shared__ __attribute__((aligned(16))) int scol[NG * PER];
    double(*sred)[R] = reinterpret_cast<double(*)[R]>(sval);
    const int tid = threadIdx.x;
    const int row0 = bid * R;
    const int rl = tid % R, j0 = tid / R;

    // RUN block (k_pk_meta): every row holds L entries and column(row r, slot k) = column(row 0, slot k) + r.  Nothing but
    // the values streams; the columns are row 0's L integers, read through the scalar cache (a wavefront is one slot j0 of
    // 64 rows: its k is uniform), and -- the point -- the x gathers no longer wait for the staged columns: they go out
    // TOGETHER with the value stream, one memory latency per block instead of two.  Entry order per lane and the order of
    // the additions are those of the general path below: the same bits.
    // [s, e): the block's entries; column(row 0, slot k) = bcol[k], or cadd + the stretch's table (stride Q per wavefront); uv: the
    // lane's u where it does not come from the gathers.
    // STRETCH: the block is one of a stretch (below) and has not looked at the stop flag yet: it asks for it with the columns and
    // consults it once everything is requested, before the first LDS store -- a stopped solve's trailing products stay cheap.
    auto run_block = [&](auto stretch_tag, int s, int e, int nrows, int L, int kd, const int *__restrict__ bcol, int cadd, int Q, double uv) {
        constexpr bool STRETCH = decltype(stretch_tag)::value;
        const int bv = s & ~1, cntv = e - bv;
        const int w = __builtin_amdgcn_readfirstlane(j0);
        const bool live = rl < nrows;
        v2d pv[VR];
#pragma unroll
        for (int r = 0; r < VR; r++) {
            const int u = 2 * (tid + r * VB);
            // (non-temporal value loads, so that the stream would not push x out of the L2: 581 vs 520 us -- measured and removed)
            pv[r] = *reinterpret_cast<const v2d *>(val + (long)bv + (u < cntv ? u : 0));
        }
        // (a stretch: the wavefront's slots lie side by side in the stretch's table, zeros behind the L-th -- read unconditionally, in
        //  one request, the stop flag with them)
        int stop = 0, cs[UNR];
        const int *__restrict__ tw = bcol + (STRETCH ? w * Q : 0);
        if constexpr (STRETCH) {
            if (done) stop = *done;
#pragma unroll
            for (int q = 0; q < UNR; q++) cs[q] = tw[q];
        }
        double xv[UNR];
#pragma unroll
        for (int q = 0; q < UNR; q++) {
            const int k = w + q * T;                     // uniform
            const int c0 = STRETCH ? cs[q] + cadd : bcol[k < L ? k : 0];    // scalar load
            xv[q] = x[(k < L && live) ? c0 + rl : 0];
        }
        __builtin_amdgcn_sched_barrier(0);
        if (STRETCH && stop) return;                    // uniform
#pragma unroll
        for (int r = 0; r < VR; r++) {
            const int u = 2 * (tid + r * VB);
            if (u < cntv) *reinterpret_cast<v2d *>(sval + u) = pv[r];
        }
        __syncthreads();
        double acc = 0.0;
        const int rs0 = s + rl * L - bv;                   // first entry of this lane's row in the staged values
        double *sud = reinterpret_cast<double *>(scol);     // (a run block stages no columns: its u, where the diagonal is among the gathers)
        if (live) {
#pragma unroll
            for (int q = 0; q < UNR; q++) {
                const int k = w + q * T;
                acc = k < L ? fma(sval[rs0 + k], xv[q], acc) : acc;
                if (DOT && k == kd) sud[rl] = xv[q];        // (uniform: one wavefront, one q)
            }
            for (int k = w + UNR * T; k < L; k += T) {
                const double xk = x[(STRETCH ? tw[k / T] + cadd : bcol[k]) + rl];
                acc = fma(sval[rs0 + k], xk, acc);
                if (DOT && k == kd) sud[rl] = xk;
            }
        }
        __syncthreads();
        sred[j0][rl] = acc;
        __syncthreads();
        if (DOT && kd >= 0 && j0 == 0 && live) uv = sud[rl];
        double vfin = 0.0;
        if (j0 == 0 && live) {
            double v = sred[0][rl];
#pragma unroll
            for (int j = 1; j < T; j++) v += sred[j][rl];
            y[row0 + rl] = v;
            vfin = v;
        }
        if (DOT) ldsp_dot_tail(dp, bid, j0, vfin, uv);
    };

    if constexpr (RR == 64) {
        // A block of a STRETCH (k_pk_stretch_flags) loads no row pointer, no pofs / pbase and no columns of its own: its entries, its
        // L and the slot of its diagonal follow from its number and the stretch's few numbers in the kernel arguments (scalar
        // arithmetic), its columns from the stretch's offsets -- one table for all its blocks, hot in the scalar cache.  The value
        // loads wait for no load at all, the gathers for the hot table only; from the first LDS store on it is a run block like any other.
        static_assert(T == 4, "the stretches' tables are laid out for four wavefronts per block");
        RunStretch me = st.s[0];        // (all four read at once, chosen by selects: no dependent loads)
#pragma unroll
        for (int i = 1; i < RS_MAX; i++) {
            const RunStretch c = st.s[i];
            const bool in = bid >= c.b0 && bid < c.b1;
            me.b0 = in ? c.b0 : me.b0; me.b1 = in ? c.b1 : me.b1; me.s0 = in ? c.s0 : me.s0; me.L = in ? c.L : me.L;
            me.kd = in ? c.kd : me.kd; me.Q = in ? c.Q : me.Q; me.off = in ? c.off : me.off;
        }
        if (bid >= me.b0 && bid < me.b1) {       // uniform
            const int s = me.s0 + (bid - me.b0) * (R * me.L);
            const int kd = (DOT && dp.ux) ? me.kd : -1;
            double uv = 0.0;
            if (DOT && kd < 0) uv = dp.u[j0 == 0 ? row0 + rl : 0];
            run_block(std::true_type{}, s, s + R * me.L, R, me.L, kd, me.off, row0, me.Q, uv);
            return;
        }
    }
    if (done && *done) return;

    const int nrows = min(R, n - row0);
    const int s = rowptr[row0], e = rowptr[row0 + nrows];
    const int dof = RR == 64 ? 1 : dp.dof;             // (uniform; groups of consecutive columns are a shape of the long-row blocks)
    const int cnt = e - s, ng = (cnt + PER * dof - 1) / (PER * dof);
    const int po = pofs[bid], bs = pbase[bid];
    const int bv = s & ~1, cntv = e - bv;
    double uv = 0.0;
    // (u == x and a run block that holds its own diagonal: u of row r IS one of the block's gathers, x[column(0, kd) + r] with
    //  column(0, kd) = the block's first row -- 80 MB less to read per product of the headline system.  kd comes with the block's columns:
    //  searching row 0's columns here, 33 dependent scalar loads in front of the stream's requests, made the product 22 % SLOWER.)
    int kd = -1;
    if (DOT && RR == 64 && dp.ux && bs < 0)     // (k_pk_pack left it behind row 0's L columns / the template's D offsets: -1 = not every row of the block holds its diagonal)
        kd = reinterpret_cast<const int *>(packed + po)[bs > -TPL_CODE ? -1 - bs : -bs - TPL_CODE];
    if (DOT && kd < 0) uv = dp.u[(j0 == 0 && rl < nrows) ? row0 + rl : 0];     // requested ahead of the stream: hidden behind it

    if (RR == 64 && bs <= -TPL_CODE) {     // (run and template blocks are shapes of 64 rows: the builder marks none at 32 / 16 rows per block)
        // TEMPLATE block (k_pk_meta): every entry lies on one of D <= 64 diagonals and every row says by a mask which of them it
        // has.  As in a run block nothing but the values streams and the x gathers go out beside the value stream -- their
        // addresses come from the row's mask and the D offsets (held one per lane, fetched by a wavefront shuffle), not from staged
        // columns.  Entry e of a row is the e-th set bit of its mask (columns ascend); lane (row, j0) takes entries j0, j0 + T, ...
        // and the partial sums meet as in the general path: the same bits.
        // (NS < 8 is launched only for matrices whose LONGEST row has NS * T entries at most: its template blocks' rows fit too)
        static_assert(UNR * T >= TPL_MAXROW || NS < 8, "one predicated batch covers the longest row of a template block");
        const int D = -bs - TPL_CODE;
        const int *tplp = reinterpret_cast<const int *>(packed + po);
        const int *mskp = tplp + ((D + 1 + 3) & ~3);       // 64 masks: 32 bits wide up to 32 diagonals, 64 beyond (tplp[D]: the diagonal's index)
        const bool live = rl < nrows;
        double vfin = 0.0;
        // two instances of the same code, chosen by a scalar branch: WIDE (33 .. 64 diagonals) works on 64-bit masks, the other --
        // every plain stencil -- on 32-bit ones (the wide arithmetic costs the narrow case 4-8 %, measured)
        auto block = [&](auto wide_tag) {
            constexpr bool WIDE = decltype(wide_tag)::value;
            typedef typename std::conditional<WIDE, unsigned long long, unsigned>::type M;
            // the small loads FIRST: the gathers wait for the mask, and a wait for a load issued behind the value stream is a wait
            // for the value stream (vmcnt counts in order) -- two memory latencies per block instead of one
            const M mask = live ? reinterpret_cast<const M *>(mskp)[rl] : (M)0;
            const int myoff = tplp[rl < D ? rl : 0];            // lane l < D of every wavefront holds offset l
            const int rs = (live ? rowptr[row0 + rl] : bv) - bv;    // this lane's row in the staged values
            v2d pv[VR];
#pragma unroll
            for (int r = 0; r < VR; r++) {
                const int u = 2 * (tid + r * VB);
                pv[r] = *reinterpret_cast<const v2d *>(val + (long)bv + (u < cntv ? u : 0));
            }
            const int len = WIDE ? __popcll((unsigned long long)mask) : __popc((unsigned)mask);
            const M full = D >= (WIDE ? 64 : 32) ? ~(M)0 : (((M)1 << D) - (M)1);
            const bool dense = __ballot(live && mask != full) == 0ull;      // uniform: every live row has all D diagonals
            // Entry j0 + q T of a row is the (j0 + q T)-th set bit of its mask.  The lane walks its mask instead of searching it: drop
            // the j0 lowest set bits once (j0 is the wavefront's number: a uniform loop), then per entry read the lowest set bit and drop
            // T -- 9 integer instructions per entry where the halving search took about 30 (7-point x 3 unknowns: 300 -> see DESIGN)
            M m = mask;
            if (!dense)
                for (int i = __builtin_amdgcn_readfirstlane(j0); i > 0; i--) m &= m - (M)1;
            double xv[UNR];
#pragma unroll
            for (int q = 0; q < UNR; q++) {
                int slot = j0 + q * T;
                if (!dense) {       // uniform
                    slot = m ? (WIDE ? __builtin_ctzll((unsigned long long)m) : __builtin_ctz((unsigned)m)) : 0;
#pragma unroll
                    for (int t = 0; t < T; t++) m &= m - (M)1;
                }
                const int off = __shfl(myoff, slot & 63, 64);
                const bool ok = live && j0 + q * T < len;
                xv[q] = x[ok ? rl + off : 0];       // (the offsets are row 0's columns, as in a run block: column = offset + row in block)
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < VR; r++) {
                const int u = 2 * (tid + r * VB);
                if (u < cntv) *reinterpret_cast<v2d *>(sval + u) = pv[r];
            }
            __syncthreads();
            double acc = 0.0;
            // (the diagonal is entry e_d of this row -- the set bits of its mask below the diagonal's -- and lives in lane e_d mod T, batch e_d / T)
            double *sud = reinterpret_cast<double *>(scol);
            const int ed = (DOT && kd >= 0) ? (WIDE ? __popcll((unsigned long long)(mask & (((M)1 << kd) - (M)1))) : __popc((unsigned)(mask & (((M)1 << kd) - (M)1)))) : -1;
            const int qd = (ed >= 0 && ed % T == j0) ? ed / T : -1;
#pragma unroll
            for (int q = 0; q < UNR; q++) {
                const int e = j0 + q * T;
                acc = (live && e < len) ? fma(sval[rs + e], xv[q], acc) : acc;
                if (DOT && q == qd && live) sud[rl] = xv[q];
            }
            __syncthreads();
            sred[j0][rl] = acc;
            __syncthreads();
            if (DOT && kd >= 0 && j0 == 0 && live) uv = sud[rl];
            if (j0 == 0 && live) {
                double v = sred[0][rl];
#pragma unroll
                for (int j = 1; j < T; j++) v += sred[j][rl];
                y[row0 + rl] = v;
                vfin = v;
            }
        };
        if (D > 32) block(std::true_type{}); else block(std::false_type{});
        if (DOT) ldsp_dot_tail(dp, bid, j0, vfin, uv);
        return;
    }
    if (RR == 64 && bs < 0) {       // RUN block (above), its plan loaded per block
        run_block(std::false_type{}, s, e, nrows, -1 - bs, kd, reinterpret_cast<const int *>(packed + po), 0, 0, uv);
        return;
    }

    const int rsafe = rl < nrows ? rl : 0;              // (requested before the stream, branch-free: see lds1_block)
    int rs = rowptr[row0 + rsafe], re = rowptr[row0 + rsafe + 1];
    if (rl >= nrows) { rs = 0; re = 0; }
    v4i pg[GR]; v2d pv[VR];
    // (dof > 1: a group's fields are spread over dof lanes -- lane t takes group t / dof and, of each of its fields' dof consecutive
    //  columns, the (t % dof)-th: as many LDS stores per lane as with a field per column.  With the group's lanes taking all dof
    //  columns of a field each, a third of the lanes did three times the stores and the product got SLOWER: 1296 against 1166 us on
    //  the 27-point stencil x 3.)
    const unsigned dmul = dof == 3 ? 0x5556u : 0u;       // t / 3 = (t * 0x5556) >> 16 for t < 2^15
#pragma unroll
    for (int r = 0; r < GR; r++) {
        const int t = tid + r * VB;
        const int gi = dof == 1 ? t : (dof == 2 ? t >> 1 : (dof == 4 ? t >> 2 : (int)(((unsigned)t * dmul) >> 16)));
        pg[r] = packed[po + (gi < ng ? gi : 0)];
    }
#pragma unroll
    for (int r = 0; r < VR; r++) {
        const int u = 2 * (tid + r * VB);
        pv[r] = *reinterpret_cast<const v2d *>(val + (long)bv + (u < cntv ? u : 0));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < GR; r++) {
        const int t = tid + r * VB;
        const int gi = dof == 1 ? t : (dof == 2 ? t >> 1 : (dof == 4 ? t >> 2 : (int)(((unsigned)t * dmul) >> 16)));
        if (gi < ng) {
            const u64 lo = (u64)(unsigned)pg[r].x | ((u64)(unsigned)pg[r].y << 32);
            const u64 hi = (u64)(unsigned)pg[r].z | ((u64)(unsigned)pg[r].w << 32);
            if (dof > 1) {
                // one field per group of dof consecutive columns: the staged columns are what they would be with a field each
                const int d = t - gi * dof;
#pragma unroll
                for (int j = 0; j < PER; j++) {
                    const int i0 = (PER * gi + j) * dof + d;
                    if (i0 < cnt) scol[i0] = bs + pk_field<BITS>(lo, hi, j) + d;      // (fields past the block's end stay out: scol holds CH entries)
                }
            } else if (BITS == 21) {
                v2i a, b, c;
                a.x = bs + (int)(lo & 0x1fffff); a.y = bs + (int)((lo >> 21) & 0x1fffff);
                b.x = bs + (int)((lo >> 42) & 0x1fffff); b.y = bs + (int)(hi & 0x1fffff);
                c.x = bs + (int)((hi >> 21) & 0x1fffff); c.y = bs + (int)((hi >> 42) & 0x1fffff);
                v2i *dst = reinterpret_cast<v2i *>(scol + 6 * gi);
                dst[0] = a; dst[1] = b; dst[2] = c;
            } else {
#pragma unroll
                for (int j = 0; j < PER; j++) scol[PER * gi + j] = bs + pk_field<BITS>(lo, hi, j);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < VR; r++) {
        const int u = 2 * (tid + r * VB);
        if (u < cntv) *reinterpret_cast<v2d *>(sval + u) = pv[r];
    }
    __syncthreads();
    double acc = 0.0;
    int k = rs + j0;
    {   // the first batch is predicated for every NS (it was for NS > 8 only: rows of fewer than 8 T entries then went through the
        // serial loop at the end, one gather at a time -- 29 entries per row were slower than 33: 782 vs 759 us at 10M rows)
        int c[UNR]; double a[UNR], xv[UNR];
#pragma unroll
        for (int q = 0; q < UNR; q++) {
            const int kk = k + q * T;
            const bool ok = kk < re;
            const int cc = scol[ok ? kk - s : 0];
            c[q] = ok ? cc : 0;         // an empty block never wrote scol[0]: column 0 is always a valid address
            a[q] = sval[ok ? kk - bv : 0];
        }
        // (non-temporal gathers: 3.86 instead of 1.44 ms on the row-random band, 0.97 instead of 0.75 on constant diagonals;
        //  L1-bypassing sc1 gathers: no difference -- measured in round 2 and removed)
#pragma unroll
        for (int q = 0; q < UNR; q++) xv[q] = x[c[q]];
#pragma unroll
        for (int q = 0; q < UNR; q++) acc = (k + q * T < re) ? fma(a[q], xv[q], acc) : acc;   // select, not a zero product: same bits as the plain loop
        k += UNR * T;
    }
    for (; k + (UNR - 1) * T < re; k += UNR * T) {
        int c[UNR]; double a[UNR], xv[UNR];
#pragma unroll
        for (int q = 0; q < UNR; q++) { c[q] = scol[k + q * T - s]; a[q] = sval[k + q * T - bv]; }
#pragma unroll
        for (int q = 0; q < UNR; q++) xv[q] = x[c[q]];
#pragma unroll
        for (int q = 0; q < UNR; q++) acc = fma(a[q], xv[q], acc);
    }
    for (; k < re; k += T) acc = fma(sval[k - bv], x[scol[k - s]], acc);
    __syncthreads();
    sred[j0][rl] = acc;
    __syncthreads();
    double vfin = 0.0;
    if (j0 == 0 && rl < nrows) {
        double v = sred[0][rl];
#pragma unroll
        for (int j = 1; j < T; j++) v += sred[j][rl];
        y[row0 + rl] = v;
        vfin = v;
    }
    if (DOT) ldsp_dot_tail(dp, bid, j0, vfin, uv);
}

// The <= 512-way second stage of a product's per-block sums: block i adds the slice [i * per, (i + 1) * per) of `big` in a
// fixed order and leaves it in out[i] (the y.y sums, `stride` further on, in out[AXP_CAP + i]).
__global__ __launch_bounds__(VB) void k_axp_fold(const double *__restrict__ big, int nblk, int stride, int per, int yy, double *__restrict__ out,
                                                 const int *done)
{
    __shared__ double sh[2][VB / 64];
    if (done && *done) return;
    const int lo = blockIdx.x * per, hi = min(nblk, lo + per);
    double a0 = 0.0, a1 = 0.0;
    for (int j0 = lo; j0 < hi; j0 += 4 * VB) {
        double t[4], w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int j = j0 + threadIdx.x + q * VB;
            t[q] = big[j < hi ? j : lo];
            w[q] = yy ? big[stride + (j < hi ? j : lo)] : 0.0;
            if (j >= hi) { t[q] = 0.0; w[q] = 0.0; }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) { a0 += t[q]; a1 += w[q]; }
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == WSUM_LANE) { sh[0][wv] = a0; sh[1][wv] = a1; }
    __syncthreads();
    if (threadIdx.x < 2 && (threadIdx.x == 0 || yy)) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < VB / 64; q++) t += sh[threadIdx.x][q];
        out[threadIdx.x * AXP_CAP + blockIdx.x] = t;
    }
}

// ---- short rows (<= 17 entries on average: 5-point / 7-point stencils, the 1000 x 1000 Laplacian of BASELINE configs[1]) ---------
// The LDS-staged kernels put 256 or 128 rows of such a matrix into a block and spend it on staging ~1300 entries behind two
// barriers.  Where the 64-row blocks are RUNS (k_pk_meta) ONE WAVEFRONT owns a block, lane = row: the L columns of row 0 come
// through the scalar cache, the gathers of x (column + lane: one contiguous run per entry slot) go out at once with the
// block's values, which are read coalesced (the block's 64 L values are contiguous) and handed to their rows through a
// wavefront-private piece of LDS -- no barrier anywhere.  (Reading them straight from the row, 8 bytes at a stride of L
// doubles, was measured first: every 128-byte line is then fetched by L instructions and the L1 does not hold a CU's waves'
// lines in between -- 20.0 us on the 1M-row Laplacian against 15.9 for the staged kernel.)  The few blocks that are not runs
// (grid-row boundaries) are walked from the CSR arrays by the same wavefront.  Entry k of a row is added to partial sum
// k mod T, the partial sums in index order -- the arithmetic of k_spmv_lds1 with VB / T rows per block (T = 1 for up to 8.5
// entries per row, 2 up to 17), which is the kernel the automatic choice would otherwise take: the same bits.
// the work of one wavefront on block b (< number of 64-row blocks); returns the finished y of row 64 b + lane (0 past the end)
template <int T>
__device__ __forceinline__ double run1_block(int b, int wv, int n, int LP, const int *__restrict__ rowptr, const int *__restrict__ col,
                                             const double *__restrict__ val, const int *__restrict__ pofs,
                                             const int *__restrict__ pbase, const int *__restrict__ pcols,
                                             const double *__restrict__ x, double *__restrict__ y, double *wlds)
{
    constexpr int NB = 8;                               // entries in flight per lane and batch (a multiple of T)
    const int lane = threadIdx.x & 63;
    const long row0 = (long)b * 64;
    const int nrows = (int)min(64L, n - row0);
    const bool live = lane < nrows;
    const int bs = pbase[b], po = pofs[b], s = rowptr[row0];
    double acc[T];
#pragma unroll
    for (int j = 0; j < T; j++) acc[j] = 0.0;
    if (bs <= -TPL_CODE) {
        // TEMPLATE block (k_pk_meta): the block's entries lie on D <= 64 diagonals, a mask per row says which.  A uniform loop over
        // the diagonals: the offset is a scalar, the gather x[offset + lane] one run with holes, the row's value the
        // popcount-th of its entries -- no column is read.  Entry e goes to partial sum e mod T like everywhere: the same bits.
        const int D = -bs - TPL_CODE;
        const int *tplp = pcols + 4 * (long)po;
        const bool wide = D > 32;       // uniform: 64-bit masks beyond 32 diagonals
        unsigned long long mask = 0ull;
        if (live) mask = wide ? reinterpret_cast<const unsigned long long *>(tplp + ((D + 1 + 3) & ~3))[lane]
                              : (unsigned long long)reinterpret_cast<const unsigned *>(tplp + ((D + 1 + 3) & ~3))[lane];
        const unsigned mlo = (unsigned)mask, mhi = (unsigned)(mask >> 32);
        const int rs = live ? rowptr[row0 + lane] - s : 0;     // this lane's row in the block's values
        // the block's values, coalesced, into the wavefront's piece of LDS as they lie in memory (64 x LP doubles hold them: LP >= the
        // longest row); read from the rows directly -- a stride of one row per lane -- every batch re-fetched the rows' lines
        double *mine = wlds + (size_t)wv * 64 * LP;
        const int tot = rowptr[row0 + nrows] - s;
        // one batch of NB diagonals: which rows have diagonal k, which of their entries it is (recomputed where it is needed: a few
        // integer instructions are cheaper than the registers that would carry them past the staging loop), x[offset + lane]
        auto has = [&](int k) { return k < D && (((k < 32 ? mlo : mhi) >> (k & 31)) & 1u); };             // (k uniform: a scalar choice)
        auto entry = [&](int k) { return __popc((k < 32 ? mlo : mhi) & ((1u << (k & 31)) - 1u)) + (k < 32 ? 0 : __popc(mlo)); };
        auto gather = [&](int k0, double (&xv)[NB]) {
#pragma unroll
            for (int q = 0; q < NB; q++) {
                const int k = k0 + q;                       // uniform
                const int off = tplp[k < D ? k : 0];        // scalar load
                xv[q] = x[has(k) ? off + lane : 0];
            }
        };
        // the first batch's gathers leave with the values, as in a run block: one memory latency less per block
        double xv[NB];
        gather(0, xv);
        for (int i0 = 0; i0 < tot; i0 += NB * 64) {
            double v[NB];
#pragma unroll
            for (int q = 0; q < NB; q++) { const int i = i0 + q * 64 + lane; v[q] = val[s + (i < tot ? i : 0)]; }
#pragma unroll
            for (int q = 0; q < NB; q++) { const int i = i0 + q * 64 + lane; if (i < tot) mine[i] = v[q]; }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int k0 = 0; k0 < D; k0 += NB) {
            if (k0 > 0) gather(k0, xv);
            double a[NB];
#pragma unroll
            for (int q = 0; q < NB; q++) a[q] = has(k0 + q) ? mine[rs + entry(k0 + q)] : 0.0;
#pragma unroll
            for (int q = 0; q < NB; q++) {
                const bool ok = has(k0 + q);
                if (T == 1) acc[0] = ok ? fma(a[q], xv[q], acc[0]) : acc[0];
                else {
                    const int e = entry(k0 + q);
#pragma unroll
                    for (int j = 0; j < T; j++) acc[j] = (ok && (e % T) == j) ? fma(a[q], xv[q], acc[j]) : acc[j];
                }
            }
        }
    } else if (bs < 0) {
        const int L = -1 - bs;
        const int *bcol = pcols + 4 * (long)po;
        double *mine = wlds + (size_t)wv * 64 * LP;
        const int tot = nrows * L;
        // the batch is as wide as the rows are long (4 / 6 / 8: L is uniform) -- with eight slots for every block a tridiagonal system
        // issued eight value loads and eight gathers per lane for three entries, the 5-point Laplacian for five
        auto run_rows = [&](auto nbt) {
            constexpr int NBX = decltype(nbt)::value;
            static_assert(NBX % T == 0, "entry k goes to partial sum k mod T");
            const float invL = 1.0f / (float)L;
            double xv[NBX];
#pragma unroll
            for (int q = 0; q < NBX; q++) {                  // the gathers of the first batch leave with the values
                const int c0 = bcol[q < L ? q : 0];
                xv[q] = x[(q < L && live) ? c0 + lane : 0];
            }
            for (int j0 = 0; j0 < L; j0 += NBX) {
                double v[NBX];
#pragma unroll
                for (int q = 0; q < NBX; q++) {
                    const int e = (j0 + q) * 64 + lane;
                    v[q] = val[s + ((j0 + q < L && e < tot) ? e : 0)];
                }
#pragma unroll
                for (int q = 0; q < NBX; q++) {
                    const int e = (j0 + q) * 64 + lane;
                    if (j0 + q < L && e < tot) {
                        int r = (int)(((float)e + 0.5f) * invL);        // e / L (e < 2^16: exact after the correction below)
                        r -= r * L > e; r += (r + 1) * L <= e;
                        mine[r * LP + (e - r * L)] = v[q];
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const double *row = mine + lane * LP;
            for (int k0 = 0; k0 < L; k0 += NBX) {
                if (k0 > 0) {
#pragma unroll
                    for (int q = 0; q < NBX; q++) {
                        const int k = k0 + q;
                        const int c0 = bcol[k < L ? k : 0];
                        xv[q] = x[(k < L && live) ? c0 + lane : 0];
                    }
                }
#pragma unroll
                for (int q = 0; q < NBX; q++) {
                    const double a = (k0 + q < L && live) ? row[k0 + q] : 0.0;
                    acc[q % T] = (k0 + q < L) ? fma(a, xv[q], acc[q % T]) : acc[q % T];
                }
            }
        };
        if (L <= 4) run_rows(std::integral_constant<int, 4>{});
        else if (L <= 6) run_rows(std::integral_constant<int, 6>{});
        else run_rows(std::integral_constant<int, NB>{});
    } else {
        // not a run: every lane walks its own row out of the CSR arrays, NB entries at a time -- all columns and values of a
        // batch requested before the first gather, all gathers before the first product (a one-by-one walk is a chain of
        // 2 L dependent loads, and 13 % of the Laplacian's blocks take this path)
        int rs = 0, re = 0;
        if (live) { rs = rowptr[row0 + lane]; re = rowptr[row0 + lane + 1]; }
        // (the batch as wide as the block's longest row needs, like the run blocks above)
        int longest = re - rs;
        for (int off = 32; off > 0; off >>= 1) longest = max(longest, __shfl_xor(longest, off, 64));
        auto walk_rows = [&](auto nbt) {
            constexpr int NBX = decltype(nbt)::value;
            static_assert(NBX % T == 0, "entry k goes to partial sum k mod T");
            for (int k0 = rs; __ballot(k0 < re) != 0; k0 += NBX) {
                int c[NBX]; double a[NBX], xv[NBX];
#pragma unroll
                for (int q = 0; q < NBX; q++) { const bool ok = k0 + q < re; c[q] = col[ok ? k0 + q : 0]; a[q] = val[ok ? k0 + q : 0]; }
#pragma unroll
                for (int q = 0; q < NBX; q++) xv[q] = x[k0 + q < re ? c[q] : 0];
#pragma unroll
                for (int q = 0; q < NBX; q++) acc[q % T] = (k0 + q < re) ? fma(a[q], xv[q], acc[q % T]) : acc[q % T];
            }
        };
        if (longest <= 4) walk_rows(std::integral_constant<int, 4>{});
        else if (longest <= 6) walk_rows(std::integral_constant<int, 6>{});
        else walk_rows(std::integral_constant<int, NB>{});
    }
    double v = acc[0];
#pragma unroll
    for (int j = 1; j < T; j++) v += acc[j];
    if (live) y[row0 + lane] = v;
    return live ? v : 0.0;
}

template <int T>
__global__ __launch_bounds__(VB) void k_spmv_run1(int n, int LP, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                  const double *__restrict__ val, const int *__restrict__ pofs,
                                                  const int *__restrict__ pbase, const int *__restrict__ pcols,
                                                  const double *__restrict__ x, double *__restrict__ y, const int *done)
{
    extern __shared__ double wlds[];                    // [VB / 64][64 * LP]: a wavefront's values, row by row (LP odd: no bank conflicts)
    if (done && *done) return;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * (VB / 64) + wv;
    if ((long)b * 64 >= n) return;
    (void)run1_block<T>(b, wv, n, LP, rowptr, col, val, pofs, pbase, pcols, x, y, wlds);
}

// The same product carrying the dot that follows it (see k_spmv_lds1d): EIGHT wavefronts per workgroup -- there is no
// barrier in the product, so the workgroup's size is free -- each adds its rows' y_i u_i (y_i y_i) with one DPP sum, and the
// workgroup leaves ONE partial per running sum: a quarter of the partials a 256-thread grid would hand the consuming pass
// (1954 instead of 3907 on the 1M-row Laplacian, whose every block re-adds them; sixteen wavefronts were measured too:
// 17.9 us per product against 15.4 -- large workgroups fill the CUs less evenly -- and four: 15.2).
constexpr int RUN1D_WG = 512;
template <int T>
__global__ __launch_bounds__(RUN1D_WG) void k_spmv_run1d(int n, int LP, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                         const double *__restrict__ val, const int *__restrict__ pofs,
                                                         const int *__restrict__ pbase, const int *__restrict__ pcols,
                                                         const double *__restrict__ x, double *__restrict__ y, const int *done, DotPlan dp)
{
    extern __shared__ double wlds[];                    // [16][64 * LP]
    __shared__ double wsum[2][RUN1D_WG / 64];
    __shared__ int arrived;
    if (done && *done) return;
    if (threadIdx.x == 0) arrived = 0;
    __syncthreads();                                    // the only barrier, before anybody has started: costs nothing
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * (RUN1D_WG / 64) + wv;
    double a0 = 0.0, a1 = 0.0;
    if ((long)b * 64 < n) {
        const long row = (long)b * 64 + lane;
        const double uv = dp.u[row < n ? row : 0];      // requested ahead of the block's loads
        const double v = run1_block<T>(b, wv, n, LP, rowptr, col, val, pofs, pbase, pcols, x, y, wlds);
        a0 = wave_sum(v * uv);                          // v = 0 on the lanes past the end
        if (dp.yy) a1 = wave_sum(v * v);
    }
    // No barrier at the end (a workgroup would hold its slots until its slowest wavefront -- the blocks that are not runs --
    // is through): every wavefront leaves its sums in LDS and takes a ticket; whoever draws the last one adds them up in
    // wavefront order (the LDS serves a wavefront's store before its ticket, so the last ticket sees every store).
    if (lane == WSUM_LANE) {
        wsum[0][wv] = a0; wsum[1][wv] = a1;
        const int ticket = __hip_atomic_fetch_add(&arrived, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (ticket == RUN1D_WG / 64 - 1) {
            double t0 = 0.0, t1 = 0.0;
#pragma unroll
            for (int q = 0; q < RUN1D_WG / 64; q++) { t0 += wsum[0][q]; t1 += wsum[1][q]; }
            dp.part[blockIdx.x] = t0;
            if (dp.yy) dp.part[dp.stride + blockIdx.x] = t1;
        }
    }
}

// ---- the plan: build, free, facts ---------------------------------------------------------------

static bool run_stretches_on(const CsrPart &P)
{
    static const int env = [] { const char *e = std::getenv("LCG_HIP_RUN_STRETCHES"); return e ? atoi(e) : -1; }();      // A/B runs: 0 / 1 for the whole process
    return (env >= 0 ? env : P.rs_mode) != 0;
}

// the stretches alone (their build failed half way; packed_free)
static void run_stretches_free(PackedPlan &K)
{
    if (K.rs_off) hipFree(K.rs_off);
    K.rs_off = nullptr; K.rs = RunStretches(); K.rs_blocks = 0; K.rs_groups = 0;
}

// The (up to RS_MAX) longest stretches of at least two blocks, from the flags of k_pk_stretch_flags (read back once: 4 bytes per block);
// their offset tables and the two numbers the host does not know (first entry, slot of the diagonal) come from k_pk_stretch_fill.
// A plan without stretches is still a plan: nothing here fails the build.
static void run_stretches_build(const CsrPart &P, PackedPlan &K, hipStream_t s, const std::vector<int> &flag)
{
    struct St { int b0, b1, L; };
    std::vector<St> all;
    const int nb = (int)flag.size();
    for (int b = 0; b < nb;) {
        if (flag[b] <= 0) { b++; continue; }
        int e = b + 1;
        while (e < nb && flag[e] == -flag[b]) e++;
        if (e - b >= 2) all.push_back({b, e, flag[b]});
        b = e;
    }
    if (all.empty()) return;
    std::stable_sort(all.begin(), all.end(), [](const St &a, const St &c) { return a.b1 - a.b0 > c.b1 - c.b0; });
    if (all.size() > (size_t)RS_MAX) all.resize(RS_MAX);
    std::sort(all.begin(), all.end(), [](const St &a, const St &c) { return a.b0 < c.b0; });
    RunStretches rs;
    rs.n = (int)all.size();
    int ints = 0;
    for (int i = 0; i < rs.n; i++) {
        rs.s[i].b0 = all[i].b0; rs.s[i].b1 = all[i].b1; rs.s[i].L = all[i].L; rs.s[i].Q = std::max(RS_QMIN, (all[i].L + 3) / 4);
        ints += 4 * rs.s[i].Q;
    }
    int h[2 * RS_MAX];
    bool ok = hipMalloc(&K.rs_off, sizeof(int) * ((size_t)ints + 2 * RS_MAX)) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_pk_stretch_fill, dim3(rs.n), dim3(64), 0, s, rs, P.rowptr, P.col, K.rs_off, K.rs_off + ints);
        ok = hipMemcpyAsync(h, K.rs_off + ints, sizeof(int) * 2 * rs.n, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
    }
    if (!ok) { (void)hipGetLastError(); run_stretches_free(K); return; }
    int o = 0;
    for (int i = 0; i < rs.n; i++) {
        RunStretch &r = rs.s[i];
        r.s0 = h[2 * i]; r.kd = h[2 * i + 1]; r.off = K.rs_off + o;
        o += 4 * r.Q;
        K.rs_blocks += r.b1 - r.b0;
        K.rs_groups += (long)(r.b1 - r.b0) * ((r.L + 1 + 3) / 4);
    }
    K.rs = rs;
}

// Everything the plan holds, in the one place that knows what that is.  (No device synchronisation here: the callers whose part may
// still be multiplying wait first, as they always did.)
// The released plan's numbers (R, groups, runs, tpls, ...) stay readable, as they always did: lcg_hip_csr_packed_runs' block count
// and the traffic model of a latest product that used the plan answer from them until the next build overwrites them.
// part_goes: the part itself is being destroyed (free_part, dist_free) -- nothing stays.
void packed_free(const CsrPart &P, bool part_goes)
{
    sym_runs_free(P);       // the half store; sym_why = "not tried"
    if (PackedPlan *K = packed_plan(P)) {
        run_stretches_free(*K);
        if (K->base) hipFree(K->base);
        if (K->ofs) hipFree(K->ofs);
        if (K->data) hipFree(K->data);
        K->base = K->ofs = nullptr; K->data = nullptr;
        if (part_goes) { delete K; P.pk_plan = nullptr; }
    }
    P.pk_state = 0;
}

// Build the packed columns of P once (device; two short synchronisations).  Returns true when ready.
// runs_only (k_spmv_run1, short rows): only the run blocks get anything -- row 0's columns; the other blocks are walked
// from the CSR arrays -- so the copy costs a few integers per block, and small systems take it too (pk_state = 2).
bool packed_build(const CsrPart &P, hipStream_t s, bool runs_only, int R)
{
    if (P.pk_state != 0) return P.pk_state == (runs_only ? 2 : 1) && packed_plan(P)->R == R;
    P.pk_state = -1;
    static const int env = [] { const char *e = std::getenv("LCG_HIP_PACKED"); return e ? atoi(e) : -1; }();
    const int mode = env >= 0 ? env : P.pk_mode;
    if (mode == 0) return false;
    if (!runs_only && mode < 0 && P.nnz < (1 << 22)) return false;       // small systems are launch-bound: not worth the memory
    PlanTimer timer(P, s);
    if (!P.pk_plan) P.pk_plan = new PackedPlan();
    PackedPlan &K = *packed_plan(P);        // (a released plan's object is built into again: its numbers change only when the build succeeds)
    const int n = P.n_rows;
    const int nb = (n + R - 1) / R;
    int *ngr = nullptr, *span = nullptr, *sflag = nullptr;
    std::vector<int> hflag;
    const bool sym = !runs_only && R == PK_R && sym_runs_wanted(P);      // (a symmetric stretch is a stretch: looked for whatever the stretches' switch says)
    const bool stretches = !runs_only && R == PK_R && (run_stretches_on(P) || sym);      // (looked for only where they are switched on)
    long total = 0;
    int hspan[4] = {0, 0, 0, 0};
    int dof = 1;
    if (R != PK_R && !runs_only) {      // long rows: do all rows consist of groups of 2 / 3 / 4 consecutive columns?
        int *d = nullptr, h[3] = {1, 1, 1};
        bool okd = hipMalloc(&d, sizeof h) == hipSuccess && hipMemcpyAsync(d, h, sizeof h, hipMemcpyHostToDevice, s) == hipSuccess;
        if (okd) {
            hipLaunchKernelGGL(k_pk_dof, dim3((n + VB - 1) / VB), dim3(VB), 0, s, n, P.rowptr, P.col, d);
            okd = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        }
        if (d) hipFree(d);
        if (okd) dof = h[2] ? 4 : (h[1] ? 3 : (h[0] ? 2 : 1));
        else (void)hipGetLastError();
    }
    bool ok = hipMalloc(&K.base, sizeof(int) * (size_t)nb) == hipSuccess && hipMalloc(&K.ofs, sizeof(int) * ((size_t)nb + 1)) == hipSuccess &&
              hipMalloc(&ngr, sizeof(int) * (size_t)nb) == hipSuccess && hipMalloc(&span, 4 * sizeof(int)) == hipSuccess &&
              hipMemsetAsync(span, 0, 4 * sizeof(int), s) == hipSuccess;
    if (ok) {
        // (k_pk_meta: 0 no run blocks, 1 run blocks and template blocks, 2 run blocks only)
        hipLaunchKernelGGL(k_pk_meta, dim3(nb), dim3(64), 0, s, n, P.rowptr, P.col, K.base, ngr, span, R == PK_R ? 1 : 0, R);
        if (stretches && hipMalloc(&sflag, sizeof(int) * (size_t)nb) == hipSuccess) {       // (read back with the block statistics: one wait for both)
            hflag.resize(nb);
            hipLaunchKernelGGL(k_pk_stretch_flags, dim3((nb + VB - 1) / VB), dim3(VB), 0, s, n, nb, P.rowptr, P.col, K.base, sflag);
            if (hipMemcpyAsync(hflag.data(), sflag, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, s) != hipSuccess) { (void)hipGetLastError(); hflag.clear(); }
        }
        ok = hipMemcpyAsync(hspan, span, 4 * sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    if (ok) ok = runs_only ? 2L * (hspan[2] + hspan[3]) >= nb : hspan[0] < PK_SPAN;     // runs only: worth it when most blocks are runs or templates
    const int bits = runs_only ? 0 : (hspan[0] < (1 << 18) ? 18 : 21);     // seven 18-bit columns per group where the blocks are narrow enough
    if (ok) {
        hipLaunchKernelGGL(k_pk_groups, dim3((nb + VB - 1) / VB), dim3(VB), 0, s, nb, runs_only ? 0 : (128 / bits) * dof, ngr);
        ok = device_exclusive_scan(nb, ngr, K.ofs, s, &total) == 0;
    }
    if (ok) ok = total > 0 && total < 0x7fffffffL;
    if (ok) ok = hipMalloc(&K.data, 16 * ((size_t)total + 4)) == hipSuccess;
    if (ok) {
        if (runs_only)
            hipLaunchKernelGGL(k_pk_pack<0>, dim3(nb), dim3(VB), 0, s, n, P.rowptr, P.col, K.base, K.ofs, static_cast<v4i *>(K.data), R, 1);
        else if (bits == 18)
            hipLaunchKernelGGL(k_pk_pack<18>, dim3(nb), dim3(VB), 0, s, n, P.rowptr, P.col, K.base, K.ofs, static_cast<v4i *>(K.data), R, dof);
        else
            hipLaunchKernelGGL(k_pk_pack<21>, dim3(nb), dim3(VB), 0, s, n, P.rowptr, P.col, K.base, K.ofs, static_cast<v4i *>(K.data), R, dof);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ngr) hipFree(ngr);
    if (span) hipFree(span);
    if (sflag) hipFree(sflag);
    if (!ok) {
        (void)hipGetLastError();
        const char *why = P.sym_why;
        packed_free(P);
        P.pk_state = -1;        // (this site: a failed build is not tried again until a setter says so ...
        P.sym_why = why;        //  ... and leaves the symmetric stretch's status as it was)
        return false;
    }
    K.maxrow = hspan[1];
    K.runs = hspan[2];
    K.tpls = hspan[3];
    K.groups = total;
    K.bits = bits;
    K.R = R;
    K.dof = dof;
    P.pk_state = runs_only ? 2 : 1;
    if (!hflag.empty() && hspan[2] > 1) run_stretches_build(P, K, s, hflag);
    if (sym) sym_runs_build(P, s);
    return true;
}

int packed_maxrow(const CsrPart &P) { return packed_plan(P)->maxrow; }
int packed_bits(const CsrPart &P) { return packed_plan(P)->bits; }

// what k_spmv_ldsp multiplied with (static strings: lcg_hip_csr_last_kernel hands them out)
static const char *ldsp_name(const CsrPart &P, bool dot)
{
    const PackedPlan &K = *packed_plan(P);
    const int form = (K.runs > 0 ? 1 : 0) + (K.tpls > 0 ? 2 : 0);
    if (dot) {
        static const char *const d[4] = {"k_spmv_ldsp (LDS-staged, packed columns) carrying the dot that follows the product",
                                         "k_spmv_ldsp (LDS-staged, run blocks + packed columns) carrying the dot that follows the product",
                                         "k_spmv_ldsp (LDS-staged, template blocks + packed columns) carrying the dot that follows the product",
                                         "k_spmv_ldsp (LDS-staged, run blocks + template blocks + packed columns) carrying the dot that follows the product"};
        return d[form];
    }
    static const char *const a[2][4] = {{"k_spmv_ldsp (LDS-staged, 18-bit packed columns)", "k_spmv_ldsp (LDS-staged, run blocks + 18-bit packed columns)",
                                         "k_spmv_ldsp (LDS-staged, template blocks + 18-bit packed columns)",
                                         "k_spmv_ldsp (LDS-staged, run blocks + template blocks + 18-bit packed columns)"},
                                        {"k_spmv_ldsp (LDS-staged, 21-bit packed columns)", "k_spmv_ldsp (LDS-staged, run blocks + 21-bit packed columns)",
                                         "k_spmv_ldsp (LDS-staged, template blocks + 21-bit packed columns)",
                                         "k_spmv_ldsp (LDS-staged, run blocks + template blocks + 21-bit packed columns)"}};
    return a[K.bits == 18 ? 0 : 1][form];
}

// the same while the sliced range of a symmetric stretch goes to k_spmv_ldsp_sym (csr_sym.hip): the family's name first, as ever
// (a symmetric stretch is made of run blocks: the forms with them only; static strings like ldsp_name's)
static const char *sym_runs_name(const CsrPart &P, bool dot)
{
#define SYM_AROUND(s) " around k_spmv_ldsp_sym (symmetric run stretch: half store in dispatch order, " s ")"
#define SYM_GROUPED(s) " around k_spmv_ldsp_sym (symmetric run stretch: half store in block order, one slice, " s " consecutive blocks per XCD)"
#define SYM_NAMES(base, tail) {base SYM_AROUND("one slice") tail, base SYM_AROUND("two slices") tail, base SYM_AROUND("four slices") tail, base SYM_AROUND("eight slices") tail, \
                              base SYM_GROUPED("two") tail, base SYM_GROUPED("four") tail, base SYM_GROUPED("eight") tail}
#define SYM_DOT " carrying the dot that follows the product"
    const PackedPlan &K = *packed_plan(P);
    const int G = sym_group_in_use(P);                 // (more than one: one slice only)
    const int nx = G == 8 ? 6 : G == 4 ? 5 : G == 2 ? 4 : K.sym.NX == 8 ? 3 : K.sym.NX == 4 ? 2 : K.sym.NX == 2 ? 1 : 0, tpl = K.tpls > 0 ? 1 : 0;
    if (dot) {
        static const char *const d[2][7] = {SYM_NAMES("k_spmv_ldsp (LDS-staged, run blocks + packed columns)", SYM_DOT),
                                            SYM_NAMES("k_spmv_ldsp (LDS-staged, run blocks + template blocks + packed columns)", SYM_DOT)};
        return d[tpl][nx];
    }
    static const char *const a[2][2][7] = {{SYM_NAMES("k_spmv_ldsp (LDS-staged, run blocks + 18-bit packed columns)", ""),
                                            SYM_NAMES("k_spmv_ldsp (LDS-staged, run blocks + template blocks + 18-bit packed columns)", "")},
                                           {SYM_NAMES("k_spmv_ldsp (LDS-staged, run blocks + 21-bit packed columns)", ""),
                                            SYM_NAMES("k_spmv_ldsp (LDS-staged, run blocks + template blocks + 21-bit packed columns)", "")}};
#undef SYM_DOT
#undef SYM_NAMES
#undef SYM_GROUPED
#undef SYM_AROUND
    return a[K.bits == 18 ? 0 : 1][tpl][nx];
}

// ---- the launches -------------------------------------------------------------------------------
// k_spmv_ldsp's gathers per lane in its first batch (NS): the smallest instantiated one that covers the longest row.
// Blocks of 64 rows: enough for the longest row when that is 9..12 per lane.
// Long rows (a block of 64 does not fit the window): blocks of 32 / 16 rows, 8 / 16 lanes per row, packed columns only.
// ONE predicated batch of NS gathers per lane, NS the smallest of the instantiated ones that covers the longest row
// (nine where the rows are longer still: the loop takes the rest) -- every gather beyond a lane's entries is a wasted
// instruction, and with nine for all the packed form was no faster than the plain one.
int ldsp_ns(const CsrPart &P, int R)
{
    const int per_lane = (packed_plan(P)->maxrow + VB / R - 1) / (VB / R);
    if (R == 32) return per_lane <= 7 ? 7 : 9;
    if (R == 16) return per_lane <= 6 ? 6 : 9;
    return per_lane <= 6 ? 6 : per_lane <= 7 ? 7 : per_lane <= 8 ? 8 : per_lane <= 9 ? 9 : per_lane <= 10 ? 10 : per_lane <= 12 ? 12 : 8;
}

// k_spmv_ldsp as a choice asks for it.  Instances: 64 rows per block with every NS of ldsp_ns, pushing or not, carrying the dot or
// not; long rows (RR = 32 / 16) neither pushing nor carrying the dot.
template <bool PUSH, bool DOT, int RR = PK_R>
static void ldsp_launch(const AxChoice &c, const CsrPart &P, const double *x, double *y, hipStream_t s, const int *done,
                        const PushPlan &pp, const DotPlan &dp)
{
    const PackedPlan &K = *packed_plan(P);
    const unsigned nb = (unsigned)((P.n_rows + RR - 1) / RR);
    // SKIP: the sliced range of a symmetric stretch goes to k_spmv_ldsp_sym (csr_sym.hip), every block in front of it and behind it to
    // ONE launch of this kernel whose grid leaves the range out
    const auto launch = [&](auto skip_tag, unsigned g, const auto &st) {
        constexpr bool SKIP = decltype(skip_tag)::value;
        const auto go = [&](auto ns) {
            pick<18, 21>(c.bits, [&](auto bits) {
                pick<PK_CH_8, PK_CH_7, PK_CH_SMALL, LdsCfg<double>::CH>(c.win, [&](auto win) {
                    hipLaunchKernelGGL((k_spmv_ldsp<PUSH, decltype(ns)::value, decltype(bits)::value, DOT, decltype(win)::value, RR, SKIP>), dim3(g),
                                       dim3(VB), 0, s, P.n_rows, P.rowptr, static_cast<const v4i *>(K.data), K.ofs, K.base, P.val,
                                       x, y, done, pp, dp, st);
                });
            });
        };
        if constexpr (RR == PK_R) pick<6, 7, 8, 9, 10, 12>(c.ns, go);
        else if constexpr (RR == 32) pick<7, 9>(c.ns, go);
        else pick<6, 9>(c.ns, go);
    };
    const RunStretches rs = run_stretches_on(P) ? K.rs : RunStretches();
    if constexpr (!PUSH && RR == PK_R) {
        if (sym_runs_in_use(P)) {
            RunStretchesSkip st;
            static_cast<RunStretches &>(st) = rs;
            st.skip_from = K.sym.inner0; st.skip = K.sym.NX * K.sym.S;
            sym_runs_launch(P, DOT, x, y, s, done, dp);
            launch(std::true_type{}, nb - (unsigned)st.skip, st);
            return;
        }
    }
    launch(std::false_type{}, nb + (PUSH ? (unsigned)(pp.nblocks + pp.nrecv) : 0u), rs);
}

int packed_ldsp_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, hipStream_t s, const int *done, const PushPlan *pp)
{
    if (pp) ldsp_launch<true, false>(c, P, x, y, s, done, *pp, DotPlan());
    else ldsp_launch<false, false>(c, P, x, y, s, done, PushPlan(), DotPlan());
    HIPCHK(hipGetLastError());
    P.last_kernel = sym_runs_in_use(P) ? sym_runs_name(P, false) : ldsp_name(P, false);
    return 0;
}

int packed_ldsp_long_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, hipStream_t s, const int *done)
{
    const PackedPlan &K = *packed_plan(P);
    DotPlan dp; dp.dof = K.dof;
    (c.R == 32 ? ldsp_launch<false, false, 32> : ldsp_launch<false, false, 16>)(c, P, x, y, s, done, PushPlan(), dp);
    HIPCHK(hipGetLastError());
    P.last_kernel = K.dof > 1 ? (K.bits == 18 ? "k_spmv_ldsp (LDS-staged, long rows: one 18-bit packed column per group of consecutive columns)"
                                              : "k_spmv_ldsp (LDS-staged, long rows: one 21-bit packed column per group of consecutive columns)")
                              : (K.bits == 18 ? "k_spmv_ldsp (LDS-staged, long rows: 18-bit packed columns)" : "k_spmv_ldsp (LDS-staged, long rows: 21-bit packed columns)");
    return 0;
}

// The packed kernel carrying y.u (and y.y): one partial per block of 64 rows into a buffer of the part's own (dot_part_fold takes
// them from there).  pp != nullptr: the product of a row shard with its pushing blocks in front (comm.hip).
int packed_ldsp_dot_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, const double *u, int yy, int *nsum, hipStream_t s,
                           const int *done, const PushPlan *pp)
{
    *nsum = (P.n_rows + PK_R - 1) / PK_R;
    if (!ensure_dot_part(P, *nsum)) return 0;
    DotPlan dp; dp.u = u; dp.part = P.dot_part; dp.yy = yy; dp.stride = *nsum; dp.ux = u == x ? 1 : 0;
    if (pp) ldsp_launch<true, true>(c, P, x, y, s, done, *pp, dp);
    else ldsp_launch<false, true>(c, P, x, y, s, done, PushPlan(), dp);
    HIPCHK(hipGetLastError());
    P.last_kernel = (!pp && sym_runs_in_use(P)) ? sym_runs_name(P, true) : ldsp_name(P, true);
    return 1;
}

// Second stage of EVERY product that leaves its sums in P.dot_part: k_spmv_ldsp<DOT> above and the tiled product's dot form
// (csr_tiled.hip, through csr.hip: part_dot_launch) -- it lives here because k_axp_fold does.
int dot_part_fold(const CsrPart &P, int nsum, int yy, double *part, int *slots, hipStream_t s, const int *done)
{
    const int g2 = std::min(512, (nsum + VB - 1) / VB);
    const int per = (nsum + g2 - 1) / g2;
    hipLaunchKernelGGL(k_axp_fold, dim3((nsum + per - 1) / per), dim3(VB), 0, s, P.dot_part, nsum, nsum, per, yy, part, done);
    HIPCHK(hipGetLastError());
    *slots = (nsum + per - 1) / per;
    return 0;
}

int packed_run1_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, hipStream_t s, const int *done)
{
    const PackedPlan &K = *packed_plan(P);
    const int n = P.n_rows;
    const unsigned g = (unsigned)(((n + 63) / 64 + VB / 64 - 1) / (VB / 64));
    const int LP = K.maxrow | 1;
    const size_t lds = sizeof(double) * (VB / 64) * 64 * (size_t)LP;
    pick<1, 2>(c.R == 256 ? 1 : 2, [&](auto t) {
        hipLaunchKernelGGL((k_spmv_run1<decltype(t)::value>), dim3(g), dim3(VB), lds, s, n, LP, P.rowptr, P.col, P.val, K.ofs,
                           K.base, static_cast<const int *>(K.data), x, y, done); });
    HIPCHK(hipGetLastError());
    P.last_kernel = "k_spmv_run1 (one wavefront per 64-row block, run blocks without staging)";
    return 0;
}

// short-row stencils (k_spmv_run1d): eight wavefronts, one partial per workgroup of 512 rows (8 x 64 x LP doubles of
// dynamic LDS: rows of up to 15 entries; longer ones take k_spmv_lds1d, csr.hip)
int packed_run1d_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, const double *u, int yy, double *part, int *slots,
                        hipStream_t s, const int *done)
{
    const PackedPlan &K = *packed_plan(P);
    const int n = P.n_rows;
    const int nwg = (int)((((long)n + 63) / 64 + RUN1D_WG / 64 - 1) / (RUN1D_WG / 64));
    if (K.maxrow > 15 || nwg > AXP_CAP) return 0;
    DotPlan dp; dp.u = u; dp.part = part; dp.yy = yy;
    const int LP = K.maxrow | 1;
    const size_t lds = sizeof(double) * (RUN1D_WG / 64) * 64 * (size_t)LP;
    pick<1, 2>(c.R == 256 ? 1 : 2, [&](auto t) {
        hipLaunchKernelGGL((k_spmv_run1d<decltype(t)::value>), dim3(nwg), dim3(RUN1D_WG), lds, s, n, LP, P.rowptr, P.col, P.val, K.ofs,
                           K.base, static_cast<const int *>(K.data), x, y, done, dp); });
    HIPCHK(hipGetLastError());
    P.last_kernel = "k_spmv_run1d (one wavefront per 64-row block, run blocks without staging) carrying the dot that follows the product";
    *slots = nwg;
    return 1;
}

// ---- what the plan costs ------------------------------------------------------------------------
// (a part that never tried a build has no plan object: it answers as one whose plan holds nothing.  A released plan's object stays
//  with its numbers: packed_free)
static const PackedPlan &plan_or_none(const CsrPart &P)
{
    static const PackedPlan none;
    const PackedPlan *K = packed_plan(P);
    return K ? *K : none;
}

// the stretches a part's k_spmv_ldsp runs from, as things stand
static bool stretches_in_use(const CsrPart &P) { return P.pk_state == 1 && run_stretches_on(P) && packed_plan(P)->rs.n > 0; }

int64_t packed_traffic_bytes(const CsrPart &P, const char *k)
{
    const PackedPlan &K = plan_or_none(P);
    const int64_t n = P.n_rows;
    const int64_t nb = (n + K.R - 1) / K.R;
    if (std::strncmp(k, "k_spmv_ldsp", 11) == 0) {     // values + packed columns (run blocks: row 0's columns only) + two words per block
        int64_t b = 8 * P.nnz + 16 * (int64_t)K.groups + 8 * nb;
        if (stretches_in_use(P)) {          // their blocks read no row pointers, no two words, no columns of their own: one table per stretch instead
            b -= (4 * PK_R + 8) * (int64_t)K.rs_blocks + 16 * (int64_t)K.rs_groups;
            for (int i = 0; i < K.rs.n; i++) b += 16 * K.rs.s[i].Q;
        }
        if (std::strstr(k, "k_spmv_ldsp_sym") && sym_runs_in_use(P) && !stretches_in_use(P)) {     // (stretches in use: the sliced range is part of one, taken off above)
            // the sliced range of a symmetric stretch (csr_sym.hip): as in any stretch, no plan of its own.  Its VALUES stay counted in
            // full: this models what enters the L2s, and a lower entry still does -- as its partner's upper entry, from whichever cache
            // holds it.  What the half store halves is the HBM side, which the counters behind this model cannot tell apart.
            const int64_t sb = (int64_t)K.sym.NX * K.sym.S, p = K.sym.p;
            b -= ((4 * PK_R + 8) + 16 * ((2 * p + 1 + 1 + 3) / 4)) * sb - 16 * K.sym.TQ;
        }
        return b;
    }
    // k_spmv_run1: values + row 0's columns of the run blocks + the CSR columns of the other blocks
    const double other = nb > 0 ? 1.0 - (double)(K.runs + K.tpls) / (double)nb : 1.0;
    return 8 * P.nnz + (int64_t)(4.0 * other * (double)P.nnz) + 16 * (int64_t)K.groups + 8 * nb;
}

int64_t packed_plan_bytes(const CsrPart &P)
{
    const PackedPlan &K = plan_or_none(P);
    int64_t b = 0;
    if (P.pk_state > 0) b += 16 * ((int64_t)K.groups + 4) + 8 * (((int64_t)P.n_rows + K.R - 1) / K.R + 1);
    for (int i = 0; i < K.rs.n; i++) b += 16 * K.rs.s[i].Q;      // the stretches' tables
    return b + sym_runs_bytes(P);                                  // a symmetric stretch's half store
}

// A change of the symmetric stretch's switches: the half store goes, and a plan that would now be built differently is built again
// at the next product (as lcg_hip_csr_set_run_stretches does).  Also where the part becomes eligible again (comm.hip: dist_free) and in the
// rewrite protocol (csr.hip: op_copies_free).
void sym_runs_reset(CsrPart &P)
{
    ranges_free(P);
    const bool want = sym_runs_wanted(P);
    if (sym_runs_bytes(P) == 0 && !(want && P.pk_state == 1)) return;
    if (ctx().inited) (void)hipDeviceSynchronize();
    if (want && P.pk_state == 1) packed_free(P);
    else sym_runs_free(P);      // (the half store alone: the plan stays)
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_csr_set_packed(lcg_hip_csr_t A, int mode)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || mode < -1 || mode > 1) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_set_packed");
    if (mode == 0) op_copies_free(A);
    for (CsrPart *P : {&A->main, &A->loc}) {
        P->pk_mode = mode;
        ranges_free(*P);                    // the ranges inherit the modes: cut again at the next product
        if (P->pk_state > 0 && mode == 0) {         // give the memory back
            if (ctx().inited) (void)hipDeviceSynchronize();
            packed_free(*P);
        }
        if (P->pk_state < 0 || mode == 0) P->pk_state = 0;     // (this site: a part that was not eligible decides again at the next product, whatever the mode)
    }
    return 0;
}

int64_t lcg_hip_csr_packed_runs(lcg_hip_csr_t A, int64_t *blocks_out)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return 0;
    const CsrPart &P = A->distributed ? A->loc : A->main;
    const PackedPlan &K = plan_or_none(P);
    if (blocks_out) *blocks_out = (P.n_rows + K.R - 1) / K.R;
    return P.pk_state > 0 ? K.runs : 0;
}

int64_t lcg_hip_csr_packed_templates(lcg_hip_csr_t A)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return 0;
    const CsrPart &P = A->distributed ? A->loc : A->main;
    return P.pk_state > 0 ? packed_plan(P)->tpls : 0;
}

int lcg_hip_csr_set_run_stretches(lcg_hip_csr_t A, int mode)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || mode < 0 || mode > 1) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_set_run_stretches");
    for (CsrPart *P : {&A->main, &A->loc}) {
        P->rs_mode = mode;
        ranges_free(*P);                    // the ranges inherit the modes: cut again at the next product
        if (mode == 1 && P->pk_state == 1 && packed_plan(*P)->rs.n == 0) {     // a plan built without looking for stretches: build it again at the next product
            if (ctx().inited) (void)hipDeviceSynchronize();
            const char *why = P->sym_why;
            packed_free(*P);
            P->sym_why = why;               // (this site: the symmetric stretch's status stays what the plan's build left -- "no run stretch" -- until the next build)
        }
    }
    return 0;
}

int64_t lcg_hip_csr_run_stretches(lcg_hip_csr_t A, int64_t *blocks_out)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (blocks_out) *blocks_out = 0;
    if (!A) return 0;
    const CsrPart &P = A->distributed ? A->loc : A->main;
    if (!stretches_in_use(P)) return 0;
    if (blocks_out) *blocks_out = packed_plan(P)->rs_blocks;
    return packed_plan(P)->rs.n;
}

int lcg_hip_csr_set_sym_runs(lcg_hip_csr_t A, int mode)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || mode < -1 || mode > 1) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_set_sym_runs");
    A->main.sym_mode = mode;
    sym_runs_reset(A->main);
    return 0;
}

int lcg_hip_csr_set_sym_slices(lcg_hip_csr_t A, int slices)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A || (slices != 0 && slices != 1 && slices != 2 && slices != 4 && slices != 8)) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_set_sym_slices");
    if (A->main.sym_nx == slices) return 0;
    A->main.sym_nx = slices;
    sym_runs_reset(A->main);
    return 0;
}

int64_t lcg_hip_csr_sym_runs(lcg_hip_csr_t A, int64_t *blocks_out, const char **status_out)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (blocks_out) *blocks_out = 0;
    if (status_out) *status_out = "";
    if (!A) return 0;
    const CsrPart &P = A->distributed ? A->loc : A->main;
    if (status_out) *status_out = P.sym_why;
    if (!sym_runs_in_use(P)) return 0;
    const SymRun &sr = packed_plan(P)->sym;
    if (blocks_out) *blocks_out = (int64_t)sr.NX * sr.S;
    return sr.NX;
}

} // extern "C"
