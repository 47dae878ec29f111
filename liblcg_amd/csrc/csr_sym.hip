// csr_sym.hip -- symmetric run stretches: half the value stream, a row slice per XCD.
//
// A run stretch (csr_packed.hip: k_pk_stretch_flags) whose offset table is antisymmetric and whose values mirror each other BIT FOR BIT --
// val(i, k) == val(i + off[k], 2p - k) for the lower slots k < p -- needs only its diagonal and upper diagonals: a lower entry of row
// i is the upper entry of its partner row.  k_sym_pack lays those out tile by tile (csr_sym.hpp: SymRun) in the order the product's
// workgroups are dispatched, k_spmv_ldsp_sym multiplies the blocks of the stretch's sliced range from it -- values straight into
// registers, no LDS staging -- and k_spmv_ldsp keeps every other block.  The same products in the same order as a run block: the
// same bits, which is why the check has no tolerance (+-0, a NaN's payload or one ulp refuse the stretch).
#include <algorithm>
#include <vector>

#include "csr_plan.hpp"

namespace lcgh {

// Slices where neither LCG_HIP_SYM_NX nor lcg_hip_csr_set_sym_slices names a count: one.  Measured on the 10M-row, 33-diagonal system
// (profiles/sym_runs_ab.txt): one slice 1619-1632 CG iterations/s against the parent's 1463-1551 in the job that ran the shipped form;
// in the jobs of the first form one slice 1613-1632, two / four / eight slices 1585-1600 / 1565-1571 / 1576-1617, parent 1498-1581.
constexpr int SYM_NX_DEFAULT = 1;
// Consecutive blocks per XCD of the one slice where LCG_HIP_SYM_GROUP names no count (1 / 2 / 4 / 8, for the whole process): four.
// Measured on the same system (profiles/sym_group_ab.txt): FETCH_SIZE of the kernel 1590.5 -> 1505.4 / 1478.2 / 1502.5 MB with
// two / four / eight, 1653-1658 / 1655-1657 / 1648-1651 CG iterations/s against the parent's 1632-1634 in one job.
// (tests/test_gpu_sym_groups.py holds the kernel string to this count: DEFAULT there changes with it.)
constexpr int SYM_GROUP_DEFAULT = 4;
constexpr int SYM_MAXL = 36;        // entries per row k_spmv_ldsp_sym is instantiated for (nine slots per lane; a block of 64 rows fits the LDS window up to 35)

static int sym_mode_of(const CsrPart &P)
{
    static const int env = [] { const char *e = std::getenv("LCG_HIP_SYM_RUNS"); return e ? atoi(e) : -2; }();     // A/B runs: -1 / 0 / 1 for the whole process
    return env >= -1 && env <= 1 ? env : P.sym_mode;
}

static int sym_nx_of(const CsrPart &P)
{
    static const int env = [] { const char *e = std::getenv("LCG_HIP_SYM_NX"); return e ? atoi(e) : 0; }();        // A/B runs: 1 / 2 / 4 / 8 for the whole process
    const auto ok = [](int v) { return v == 1 || v == 2 || v == 4 || v == 8; };
    return ok(env) ? env : ok(P.sym_nx) ? P.sym_nx : SYM_NX_DEFAULT;      // (the process's word first, as for the mode)
}

bool sym_runs_wanted(const CsrPart &P)
{
    if (!P.sym_whole || P.end_abs >= 0) return false;
    const int mode = sym_mode_of(P);
    if (mode == 0) return false;
    return mode == 1 || P.nnz * 12L >= (512L << 20);        // (automatic: the rule of solvers_real.hip's stream_vectors)
}

void sym_runs_free(const CsrPart &P)
{
    if (PackedPlan *Kp = packed_plan(P)) {
        PackedPlan &K = *Kp;
        if (K.sym_H) (void)hipFree(K.sym_H);
        K.sym_H = nullptr; K.sym = SymRun(); K.sym_tiles = 0;
    }
    P.sym_why = "not tried";
}

int64_t sym_runs_bytes(const CsrPart &P)
{
    const PackedPlan *Kp = packed_plan(P);
    if (!Kp) return 0;
    const PackedPlan &K = *Kp;
    return K.sym.NX > 0 ? 8 * K.sym_tiles * (int64_t)(K.sym.p + 1) * PK_R : 0;
}

// offset of slot k (uniform) from the stretch's table
__device__ __forceinline__ int sym_off(const SymRun &sr, int k) { return sr.off[(k % 4) * sr.TQ + k / 4]; }

// (b) of the plan: one workgroup per block of the sliced range compares its rows' lower entries with their partners' upper ones as
// 64-bit integers; any difference raises the flag.  s0: first entry of the stretch's first block b0.
__global__ __launch_bounds__(VB) void k_sym_check(SymRun sr, int b0, int s0, const double *__restrict__ val, int *flag)
{
    const unsigned long long *v = reinterpret_cast<const unsigned long long *>(val);
    const int b = sr.inner0 + (int)blockIdx.x;
    const int p = sr.p, L = 2 * p + 1;
    bool bad = false;
    for (int idx = threadIdx.x; idx < PK_R * p; idx += VB) {
        const int r = idx % PK_R, k = idx / PK_R;
        const long i = (long)(b - b0) * PK_R + r;        // row within the stretch
        const long ip = i + sym_off(sr, k);               // its partner (inside the stretch: the apron)
        bad |= v[s0 + i * L + k] != v[s0 + ip * L + (2 * p - k)];
    }
    if (bad) *flag = 1;
}

// the half store: workgroup t writes tile t -- its block's diagonal and p upper diagonals, diagonal-major
__global__ __launch_bounds__(VB) void k_sym_pack(SymRun sr, int b0, int s0, const double *__restrict__ val, double *__restrict__ H)
{
    const int t = blockIdx.x;
    const int b = t < sr.Q ? sr.inner0 - sr.Q + t : sym_block_of(t - sr.Q, sr.inner0, sr.S, sr.NX);
    const int p = sr.p, L = 2 * p + 1;
    const long e0 = s0 + (long)(b - b0) * PK_R * L;
    double *dst = H + (long)t * (p + 1) * PK_R;
    for (int idx = threadIdx.x; idx < PK_R * (p + 1); idx += VB) dst[idx] = val[e0 + (long)(idx % PK_R) * L + p + idx / PK_R];
}

// Workgroup w of the sliced range: block sym_block_of(w), own tile Q + w (one slice: block sym_group_block_of(w), own tile
// Q + block - inner0: see below).  Lane (row r, wavefront j0) takes slots k = j0, j0 + 4, ...
// as in a run block (csr_packed.hip: run_block).  A slot k >= p reads H[own tile][k - p][r]; a slot k < p reads the partner row's upper
// entry, H[tile of row i + off[k]][p - k][(i + off[k]) & 63] -- the wavefront's 64 partner rows lie in two consecutive blocks, whose
// tiles are scalar arithmetic; a lane only selects between the two bases.  Values and x gathers go out together; the additions run
// in run_block's order, the carried dot's partial keeps the BLOCK's slot and its u comes from the gather of slot p.
// One slice: which block workgroup w takes is sym_group_block_of's permutation (sr.G consecutive blocks per XCD; the identity at
// G = 1) and the block's tile is Q + its number in the range, wherever it was dispatched.  A lower slot's 512-byte partner run
// starts at row off[k] & 63 of a tile row and ends in the next tile's: unless that is a multiple of 16 rows, the 128-byte line it
// ends in is the line the NEXT block's run starts in, and the x gathers straddle likewise.  Neighbouring blocks dealt to different
// XCDs fetch such a line into two L2s; on one XCD the second reader finds it there.  Per block nothing else changes: the same bits.
template <int NS, bool DOT>
__global__ __launch_bounds__(VB) void k_spmv_ldsp_sym(SymRun sr, const double *__restrict__ x, double *__restrict__ y, const int *done, DotPlan dp)
{
    constexpr int T = VB / PK_R;
    static_assert(T == 4, "the stretches' tables are laid out for four wavefronts per block");
    __shared__ double sred[T][PK_R];
    __shared__ double sud[PK_R];
    const int tid = threadIdx.x;
    const int rl = tid % PK_R, j0 = tid / PK_R;
    const int w = __builtin_amdgcn_readfirstlane(j0);
    const int wg = blockIdx.x;
    const int bid = sr.NX == 1 ? sym_group_block_of(wg, sr.inner0, sr.S, sr.G) : sym_block_of(wg, sr.inner0, sr.S, sr.NX);
    const int wt = sr.NX == 1 ? bid - sr.inner0 : wg;   // own tile = Q + wt.  One slice: the block's number in the range, whichever workgroup takes it; slices: dispatch order
    const int row0 = bid * PK_R;
    const int p = sr.p, L = 2 * p + 1;
    const long TS = (long)(p + 1) * PK_R;
    const double *__restrict__ H = sr.H;
    const double *own = H + (long)(sr.Q + wt) * TS;
    const int *__restrict__ tw = sr.off + w * sr.TQ;    // this wavefront's slots side by side, zeros behind the L-th
    int stop = 0, cs[NS];
    if (done) stop = *done;
#pragma unroll
    for (int q = 0; q < NS; q++) cs[q] = tw[q];
    const int kd = (DOT && dp.ux) ? p : -1;
    double uv = 0.0;
    if (DOT && kd < 0) uv = dp.u[j0 == 0 ? row0 + rl : 0];
    // tile of block b <= bid (uniform): NX tiles per block back while b stays in this block's slice -- all but the first Q blocks of
    // a slice look no further -- else the map's division (across a slice's front, or into the apron)
    const int jown = wt >> (sr.NX == 8 ? 3 : sr.NX == 4 ? 2 : sr.NX == 2 ? 1 : 0);
    const auto tile_of = [&](int b) {
        const int jb = jown - (bid - b);
        return jb >= 0 ? sr.Q + wt - sr.NX * (bid - b) : sym_tile_of(b, sr.inner0, sr.S, sr.NX, sr.Q);
    };
    double xv[NS], av[NS];
#pragma unroll
    for (int q = 0; q < NS; q++) {
        const int k = w + q * T;                        // uniform
        const bool ok = k < L;
        const double *a = H;
        if (ok && k >= p) a = own + (k - p) * PK_R + rl;
        if (ok && k < p) {                              // (uniform)
            const int g = row0 + cs[q];                 // partner row of the block's first row
            const int bA = g >> 6, sh = g & 63;
            const double *ta = H + (long)tile_of(bA) * TS + (p - k) * PK_R;
            const double *tb = H + (long)tile_of(bA + 1) * TS + (p - k) * PK_R;
            const int rr = rl + sh;
            a = rr < PK_R ? ta + rr : tb + (rr - PK_R);
        }
        av[q] = *a;
        xv[q] = x[ok ? row0 + cs[q] + rl : 0];
    }
    __builtin_amdgcn_sched_barrier(0);
    if (stop) return;                                   // uniform
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < NS; q++) {
        const int k = w + q * T;
        acc = k < L ? fma(av[q], xv[q], acc) : acc;
        if (DOT && k == kd) sud[rl] = xv[q];            // (uniform: one wavefront, one q)
    }
    sred[j0][rl] = acc;
    __syncthreads();
    if (DOT && kd >= 0 && j0 == 0) uv = sud[rl];
    double vfin = 0.0;
    if (j0 == 0) {
        double v = sred[0][rl];
#pragma unroll
        for (int j = 1; j < T; j++) v += sred[j][rl];
        y[row0 + rl] = v;
        vfin = v;
    }
    if (DOT) ldsp_dot_tail(dp, bid, j0, vfin, uv);
}

int sym_group_in_use(const CsrPart &P)
{
    static const int env = [] { const char *e = std::getenv("LCG_HIP_SYM_GROUP"); return e ? atoi(e) : 0; }();     // A/B runs: 1 / 2 / 4 / 8 for the whole process
    const auto ok = [](int v) { return v == 1 || v == 2 || v == 4 || v == 8; };
    if (packed_plan(P)->sym.NX != 1) return 1;                    // (slices have their own placement)
    return ok(env) ? env : SYM_GROUP_DEFAULT;
}

void sym_runs_launch(const CsrPart &P, bool dot, const double *x, double *y, hipStream_t s, const int *done, const DotPlan &dp)
{
    SymRun sr = packed_plan(P)->sym;
    sr.G = sym_group_in_use(P);
    const dim3 g((unsigned)(sr.NX * sr.S));
    const bool small = 2 * sr.p + 1 <= 24;
    if (dot) {
        if (small) hipLaunchKernelGGL((k_spmv_ldsp_sym<6, true>), g, dim3(VB), 0, s, sr, x, y, done, dp);
        else hipLaunchKernelGGL((k_spmv_ldsp_sym<9, true>), g, dim3(VB), 0, s, sr, x, y, done, dp);
    } else {
        if (small) hipLaunchKernelGGL((k_spmv_ldsp_sym<6, false>), g, dim3(VB), 0, s, sr, x, y, done, dp);
        else hipLaunchKernelGGL((k_spmv_ldsp_sym<9, false>), g, dim3(VB), 0, s, sr, x, y, done, dp);
    }
}

// The longest stretch that qualifies: (a) its shape, (b) its values, (c) an inner range of at least NX blocks (csr_sym.hpp).
// A plan without one is still a plan: nothing here fails the build.  The status keeps why the LONGEST stretch was refused.
void sym_runs_build(const CsrPart &P, hipStream_t s)
{
    sym_runs_free(P);
    PackedPlan &K = *packed_plan(P);        // (called by packed_build: the plan is there)
    const int NX = sym_nx_of(P);
    const RunStretches &rs = K.rs;
    int order[RS_MAX];
    for (int i = 0; i < RS_MAX; i++) order[i] = i;
    std::stable_sort(order, order + rs.n, [&](int a, int c) { return rs.s[a].b1 - rs.s[a].b0 > rs.s[c].b1 - rs.s[c].b0; });
    P.sym_why = "no run stretch";
    int *flag = nullptr;
    for (int oi = 0; oi < rs.n; oi++) {
        const RunStretch &r = rs.s[order[oi]];
        const int L = r.L, p = L / 2;
        if ((L & 1) == 0 || r.kd != p || L > SYM_MAXL) { if (oi == 0) P.sym_why = "refused: no odd row length with the diagonal in the middle"; continue; }
        std::vector<int> tab(4 * (size_t)r.Q), off(L);
        if (hipMemcpyAsync(tab.data(), r.off, sizeof(int) * tab.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); if (oi == 0) P.sym_why = "refused: the offsets could not be read"; break; }
        for (int k = 0; k < L; k++) off[k] = tab[(size_t)(k % 4) * r.Q + k / 4];
        if (!sym_offsets_ok(off.data(), L)) { if (oi == 0) P.sym_why = "refused: the offsets are not antisymmetric and ascending"; continue; }
        SymRun sr;
        sr.p = p; sr.NX = NX; sr.Q = sym_apron(off[L - 1]); sr.TQ = r.Q; sr.off = r.off;
        if (!sym_range(r.b0, r.b1, sr.Q, NX, &sr.inner0, &sr.S)) { if (oi == 0) P.sym_why = "refused: the inner range is shorter than the slices"; continue; }
        int bad = 1;
        if ((flag || hipMalloc(&flag, sizeof(int)) == hipSuccess) && hipMemsetAsync(flag, 0, sizeof(int), s) == hipSuccess) {
            hipLaunchKernelGGL(k_sym_check, dim3((unsigned)(NX * sr.S)), dim3(VB), 0, s, sr, r.b0, r.s0, P.val, flag);
            if (hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) bad = 1;
        }
        (void)hipGetLastError();
        if (bad) { if (oi == 0) P.sym_why = "refused: the values do not mirror each other bit for bit"; continue; }
        const long tiles = (long)sr.Q + (long)NX * sr.S;
        if (hipMalloc(&K.sym_H, sizeof(double) * (size_t)tiles * (size_t)(p + 1) * PK_R) != hipSuccess) {
            (void)hipGetLastError(); K.sym_H = nullptr; if (oi == 0) P.sym_why = "refused: no memory for the half store"; break;
        }
        hipLaunchKernelGGL(k_sym_pack, dim3((unsigned)tiles), dim3(VB), 0, s, sr, r.b0, r.s0, P.val, K.sym_H);
        if (hipGetLastError() != hipSuccess) { (void)hipFree(K.sym_H); K.sym_H = nullptr; if (oi == 0) P.sym_why = "refused: the half store could not be written"; break; }
        sr.H = K.sym_H;
        K.sym = sr; K.sym_tiles = tiles;
        P.sym_why = "taken";
        break;
    }
    if (flag) (void)hipFree(flag);
}

} // namespace lcgh
