// dense_c64.hip -- complex64 dense operators: K.x, conj(K).x, K^T.x, K^H.x, the solver callbacks, and K.X over k = 2, 4, 8
// right-hand sides on the fp32 matrix instruction, with the sum the batched complex64 loops take after it (solvers_multi_c64.hip:
// clcg_hip_dense_lbicg_sym_multi_c64, clcg_hip_dense_lpcg_multi_c64).  One GPU.  DESIGN.md section 25.
//
// Storage: dense.hip's geometry at half the bytes.  Rows padded to whole 16-byte packs, a pack = the entries of columns 2p and
// 2p + 1 as (re, im, re, im) floats, NP = ceil(N / 2) packs per row, pads zero, 64 bytes of slack.  The plans are dense.hpp's
// (functions of M and NP and the forced variant alone).  Everything is fp32, every multiply-add an explicit fmaf:
//
//   k_cdn_row<CONJ, W>    y_i = sum_j op(K(i,j)) x_j   k_dn_row's mapping; per entry c64_mac's order (multi_c64.hpp's header)
//   (k_cdn_row_split)     the same over gridDim.y strips: fp32 partial sums in slots + k_cdn_fold
//   k_cdn_col<CONJ>       y_j = sum_i op(K(i,j)) x_i   k_dn_col's mapping: a lane owns a pack (two columns) and walks a strip of rows
//   k_cdn_fold            k_dnm_fold's order on floats
//   k_cdnm_mfma<CONJ>     Y = op(K).X for every k: below
//   k_cdnm_dot<K>         column j's unconjugated Y_j . U_j, exact fp64 products summed in fp64 as k_dnm_dot's tree, left in
//                         cspmm_c64_launch's table format
//
// The k-wide product is a real GEMM on K's raw floats.  One v_mfma_f32_16x16x4_f32 computes D[i][n] = C[i][n] + sum_{q < 4} A[i][q]
// B[q][n] as a q-ordered chain of fp32 fused multiply-adds (lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15] and, in register r,
// D[4 (l >> 4) + r][l & 15]).  Here n is one of 16 rows of K, i one of the 16 floats of a row of Y (re and im of 8 block columns:
// i = 2 j + c) and q one of four consecutive packs: lane (n, g) = (l & 15, l >> 4) loads ONE pack, pack base + g of row n, as a
// 16-byte load, and the four floats t of that pack are the B operands of four instructions; the A operand of instruction t in lane
// (i, g) is the float of X that float t of pack base + g meets on its way to output i:
//     t = 0, 2 (K_re of column 2p, 2p + 1):   c = 0: X_re      c = 1: X_im
//     t = 1, 3 (K_im):                        c = 0: -X_im     c = 1: X_re     (conj(K): the two signs flipped; the negation is exact)
// with X the entry (row 2p or 2p + 1, column j).  Lanes of columns j >= k supply 0.0f and their results are not stored: column j's
// chain is the same instructions whatever k is and wherever the column stands, and output i is made from row i of A alone, so
// nothing of another column reaches it.  With the outputs along D's rows a lane's four registers are floats 4g .. 4g + 3 of row n
// of Y: one 16-byte piece.
//
// A wavefront owns one tile of 16 rows and walks its packs eight at a time (a 128-byte line per row and step): packs base + g go
// into one accumulator, packs base + 4 + g into a second (two independent chains: the dependent latency of the instruction is 40
// cycles against a 32-cycle issue), added at the end.  The four wavefronts of a workgroup share a tile: wavefront w takes the steps
// w, w + 4, ... of the strip, and the four sums meet through LDS in wavefront order.  Few long rows: strips over gridDim.y under
// row_plan's split, fp32 slots, k_cdn_fold.  All of it is a function of (M, N) and the forced variant, never of k.
// No atomics.  Every kernel falls through when the solve or the batch has stopped (`done`).
#include <cmath>
#include <vector>

#include "c64common.hpp"
#include "dense.hpp"
#include "multi.hpp"
#include "lcg_hip_staging_dense_c64.h"

namespace lcgh {

static const char *const CDN_NAMES[] = {"k_cdn_row", "k_cdn_row_split", "k_cdn_col", "k_cdnm_mfma", "k_cdnm_mfma_split"};

typedef float cf4 __attribute__((ext_vector_type(4)));      // a pack of K, or a 16-byte piece of a block of vectors

// ---- kernels -------------------------------------------------------------------------------------------------------------------
// acc += op(k) * x in c64_mac's order (csr_c64.hip); conj(k) flips the sign of k's imaginary part and nothing else
template <bool CONJ>
__device__ __forceinline__ void cdn_mac(float2 &acc, float kr, float ki, float2 x)
{
    const float i = CONJ ? -ki : ki;
    acc.x = fmaf(kr, x.x, acc.x); acc.x = fmaf(-i, x.y, acc.x);
    acc.y = fmaf(kr, x.y, acc.y); acc.y = fmaf(i, x.x, acc.y);
}

// one pack of a row times entries 2p and 2p + 1 of x.  Odd N: the last pack's pad entry never reads entry N of x
template <bool CONJ>
__device__ __forceinline__ void cdn_row_term(float2 &acc, cf4 k, const float2 *x, int p, int N)
{
    const int j = 2 * p;
    const float2 x0 = x[j], x1 = j + 1 < N ? x[j + 1] : make_float2(0.f, 0.f);
    cdn_mac<CONJ>(acc, k.x, k.y, x0);
    cdn_mac<CONJ>(acc, k.z, k.w, x1);
}

// Row form: k_dn_row's mapping.  Row i = blockIdx.x * (256 / W) + tid / W; its lanes take the packs [p0, p1) of strip blockIdx.y, W
// apart.  S == 1: out = y.  S > 1: out = the table, slot s at out + s * M entries.
template <bool CONJ, int W>
__global__ __launch_bounds__(256) void k_cdn_row(const cf4 *__restrict__ K, int64_t ldp, int M, int N, int NP, int pps,
                                                 const float2 *__restrict__ x, float2 *__restrict__ out, const int *done)
{
    if (done && *done) return;
    const int sub = threadIdx.x % W;
    const int i = blockIdx.x * (256 / W) + threadIdx.x / W;
    const int p0 = blockIdx.y * pps;
    const int p1 = i < M ? min(NP, p0 + pps) : p0;        // (a row beyond M walks nothing but still joins the butterfly)
    const cf4 *row = K + (int64_t)min(i, M - 1) * ldp;
    float2 acc = make_float2(0.f, 0.f);
    int p = p0 + sub;
    for (; p + 3 * W < p1; p += 4 * W) {
        const cf4 k0 = row[p], k1 = row[p + W], k2 = row[p + 2 * W], k3 = row[p + 3 * W];
        cdn_row_term<CONJ>(acc, k0, x, p, N);
        cdn_row_term<CONJ>(acc, k1, x, p + W, N);
        cdn_row_term<CONJ>(acc, k2, x, p + 2 * W, N);
        cdn_row_term<CONJ>(acc, k3, x, p + 3 * W, N);
    }
    for (; p < p1; p += W) cdn_row_term<CONJ>(acc, row[p], x, p, N);
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        acc.x += __shfl_xor(acc.x, o, W);
        acc.y += __shfl_xor(acc.y, o, W);
    }
    if (sub == 0 && i < M) out[(int64_t)blockIdx.y * M + i] = acc;
}

// Column form: k_dn_col's mapping.  A workgroup owns CW packs of columns (blockIdx.x) and the rows [r0, r0 + rps) (blockIdx.y); thread
// (cp, rg) walks the rows r0 + rg, r0 + rg + RG, ... of pack cp; acc.xy is column 2p, acc.zw column 2p + 1.  The RG sums of a pack are
// added in rg order, then written to slot blockIdx.y of out (N entries per slot; gridDim.y == 1: out = y).
template <bool CONJ>
__global__ __launch_bounds__(256) void k_cdn_col(const cf4 *__restrict__ K, int64_t ldp, int M, int N, int NP, int CW, int rps,
                                                 const float2 *__restrict__ x, float2 *__restrict__ out, const int *done)
{
    __shared__ cf4 sh[256];
    if (done && *done) return;
    const int RG = 256 / CW;
    const int cp = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int p = blockIdx.x * CW + cp;
    const bool live = p < NP;
    const int r0 = blockIdx.y * rps, r1 = min(M, r0 + rps);
    float2 a0 = make_float2(0.f, 0.f), a1 = make_float2(0.f, 0.f);
    if (live) {
        const cf4 *col = K + p;
        int i = r0 + rg;
        for (; i + 7 * RG < r1; i += 8 * RG) {
            cf4 k[8];
            float2 xv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) k[u] = col[(int64_t)(i + u * RG) * ldp];
#pragma unroll
            for (int u = 0; u < 8; u++) xv[u] = x[i + u * RG];
#pragma unroll
            for (int u = 0; u < 8; u++) { cdn_mac<CONJ>(a0, k[u].x, k[u].y, xv[u]); cdn_mac<CONJ>(a1, k[u].z, k[u].w, xv[u]); }
        }
        for (; i < r1; i += RG) {
            const cf4 k = col[(int64_t)i * ldp];
            const float2 xv = x[i];
            cdn_mac<CONJ>(a0, k.x, k.y, xv); cdn_mac<CONJ>(a1, k.z, k.w, xv);
        }
    }
    if (RG > 1) {       // (uniform over the workgroup)
        cf4 v; v.x = a0.x; v.y = a0.y; v.z = a1.x; v.w = a1.y;
        sh[threadIdx.x] = v;
        __syncthreads();
        if (rg == 0)
            for (int g = 1; g < RG; g++) { const cf4 t = sh[g * CW + cp]; a0.x += t.x; a0.y += t.y; a1.x += t.z; a1.y += t.w; }
    }
    if (rg == 0 && live) {
        float2 *o = out + (int64_t)blockIdx.y * N;
        const int64_t j = 2 * (int64_t)p;
        o[j] = a0;
        if (j + 1 < N) o[j + 1] = a1;
    }
}

// y[j] = the sum of the table's S slots of n floats each: k_dnm_fold's order (dense_multi.hip) in fp32
constexpr int CFOLD_Q = 16, CFOLD_J = 16;
__global__ __launch_bounds__(CFOLD_Q * CFOLD_J) void k_cdn_fold(const float *__restrict__ part, int S, int64_t n, float *__restrict__ y,
                                                                const int *done)
{
    __shared__ float sh[CFOLD_Q][CFOLD_J];
    if (done && *done) return;
    const int jj = threadIdx.x % CFOLD_J, q = threadIdx.x / CFOLD_J;
    const int64_t j = (int64_t)blockIdx.x * CFOLD_J + jj;
    const int L = (S + CFOLD_Q - 1) / CFOLD_Q;
    const int k0 = q * L, k1 = min(S, k0 + L);
    float s = 0.f;
    if (j < n) {
        int k = k0;
        for (; k + 7 < k1; k += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = part[(int64_t)(k + u) * n + j];
#pragma unroll
            for (int u = 0; u < 8; u++) s += v[u];
        }
        for (; k < k1; k++) s += part[(int64_t)k * n + j];
    }
    sh[q][jj] = s;
    __syncthreads();
    if (q == 0 && j < n) {
        for (int g = 1; g < CFOLD_Q; g++) s += sh[g][jj];
        y[j] = s;
    }
}

// the A operands of a pack's four instructions in lane (i, g): what floats 0 .. 3 of pack p meet on their way to output float i =
// 2 j + c of the block (the table in the header).  live: the lane's column exists and the pack belongs to this walk
template <bool CONJ>
__device__ __forceinline__ cf4 cdnm_coef(const float2 *Xv, int k, int j, bool im, int p, int N, bool live)
{
    // (every lane loads from an address inside X, then keeps the value or a zero: no branch in the walk)
    const int64_t r = 2 * (int64_t)p;
    const int jc = min(j, k - 1);
    float2 x0 = Xv[min(r, (int64_t)N - 1) * k + jc], x1 = Xv[min(r + 1, (int64_t)N - 1) * k + jc];
    if (!live) x0 = make_float2(0.f, 0.f);
    if (!live || r + 1 >= N) x1 = make_float2(0.f, 0.f);
    cf4 a;
    a.x = im ? x0.y : x0.x;
    a.y = im ? (CONJ ? -x0.x : x0.x) : (CONJ ? x0.y : -x0.y);
    a.z = im ? x1.y : x1.x;
    a.w = im ? (CONJ ? -x1.x : x1.x) : (CONJ ? x1.y : -x1.y);
    return a;
}

// The k-wide product (header).  Workgroup (blockIdx.x, blockIdx.y) owns the 16 rows of tile blockIdx.x and the packs [p0, p1) of strip
// blockIdx.y; slot blockIdx.y of out holds M * k entries (gridDim.y == 1: out = Y).  k is a run-time argument: it selects which lanes
// supply zeros and which pieces are stored, and the stride of a block's rows -- never an instruction of a live column's chain.
template <bool CONJ>
__global__ __launch_bounds__(256) void k_cdnm_mfma(const cf4 *__restrict__ Kv, int64_t ldp, int M, int N, int NP, int pps, int k,
                                                   const float *__restrict__ X, float *__restrict__ out, const int *done)
{
    __shared__ cf4 sh[3][64];
    if (done && *done) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int64_t row = (int64_t)blockIdx.x * 16 + n;
    const bool rlive = row < M;
    const cf4 *krow = Kv + (rlive ? row : (int64_t)M - 1) * ldp;
    const int p0 = blockIdx.y * pps, p1 = min(NP, p0 + pps);
    const int j = n >> 1;               // as an A lane: output float i = n of the block row, column j, part c = n & 1
    const bool im = n & 1, clive = j < k;
    const float2 *Xv = reinterpret_cast<const float2 *>(X);
    const cf4 zero = (cf4)(0.f);
    cf4 acc0 = zero, acc1 = zero;
    for (int base = p0 + 8 * w; base < p1; base += 32) {        // (uniform over the wavefront)
        const int pa = base + g, pb = base + 4 + g;
        const bool la = pa < p1, lb = pb < p1;
        cf4 ka = krow[min(pa, NP - 1)], kb = krow[min(pb, NP - 1)];        // (inside the row; kept, or a zero)
        if (!(rlive && la)) ka = zero;
        if (!(rlive && lb)) kb = zero;
        const cf4 ca = cdnm_coef<CONJ>(Xv, k, j, im, pa, N, clive && la);
        const cf4 cb = cdnm_coef<CONJ>(Xv, k, j, im, pb, N, clive && lb);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca.x, ka.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(cb.x, kb.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca.y, ka.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(cb.y, kb.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca.z, ka.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(cb.z, kb.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca.w, ka.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(cb.w, kb.w, acc1, 0, 0, 0);
    }
    cf4 v = acc0 + acc1;
    if (w) sh[w - 1][lane] = v;
    __syncthreads();
    if (w) return;
    v += sh[0][lane]; v += sh[1][lane]; v += sh[2][lane];       // the wavefronts in order
    // as a D lane: row n of the tile, floats 4g .. 4g + 3 of its block row = piece g (columns 2g, 2g + 1)
    if (rlive && 2 * g < k) reinterpret_cast<cf4 *>(out)[((int64_t)blockIdx.y * M + row) * (k / 2) + g] = v;
}

// Column j's unconjugated Y_j . U_j: k_dnm_dot's frame (dense_multi.hip) on complex64 blocks.  A 16-byte piece holds two columns, so
// G = K / 2 lanes own a row and a lane four running sums (re, im of columns 2c and 2c + 1): exact fp64 products of the fp32 values,
// summed in fp64.  The 64 row lanes r = tid / G add rows r, r + 64, ... in order, then meet as ONE binary tree over r -- the same tree
// for K = 2, 4, 8.  Table row 2 j holds re, 2 j + 1 im (cspmm_c64_launch's format), one partial per workgroup at column blockIdx.x.
template <int K>
__global__ __launch_bounds__(32 * K) void k_cdnm_dot(const float *__restrict__ Y, const float *__restrict__ U, int n, int rpb,
                                                     double *__restrict__ part, const int *done)
{
    constexpr int G = K / 2;
    __shared__ double wsh[G][4 * G];
    if (done && *done) return;
    const int c = threadIdx.x % G, r = threadIdx.x / G;
    const int i0 = blockIdx.x * rpb, i1 = min(n, i0 + rpb);
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = i0 + r; i < i1; i += 64) {
        const cf4 y = reinterpret_cast<const cf4 *>(Y)[(int64_t)i * G + c], u = reinterpret_cast<const cf4 *>(U)[(int64_t)i * G + c];
        a[0] = fma((double)y.x, (double)u.x, fma(-(double)y.y, (double)u.y, a[0]));
        a[1] = fma((double)y.x, (double)u.y, fma((double)y.y, (double)u.x, a[1]));
        a[2] = fma((double)y.z, (double)u.z, fma(-(double)y.w, (double)u.w, a[2]));
        a[3] = fma((double)y.z, (double)u.w, fma((double)y.w, (double)u.z, a[3]));
    }
#pragma unroll
    for (int off = G; off <= 32; off <<= 1) {
#pragma unroll
        for (int q = 0; q < 4; q++) a[q] += __shfl_xor(a[q], off, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane < G) {
#pragma unroll
        for (int q = 0; q < 4; q++) wsh[w][4 * lane + q] = a[q];
    }
    __syncthreads();
    if (threadIdx.x < 4 * G) {
        const int q = threadIdx.x;          // the table row
        double v;
        if constexpr (G == 1) v = wsh[0][q];
        else if constexpr (G == 2) v = wsh[0][q] + wsh[1][q];
        else v = (wsh[0][q] + wsh[1][q]) + (wsh[2][q] + wsh[3][q]);
        part[(size_t)q * MM_MG + blockIdx.x] = v;
    }
}

// d = the diagonal of a square K (diag, if asked for) and inv = 1 / d by the loops' scaled division
__global__ __launch_bounds__(256) void k_cdn_diag(const cf4 *__restrict__ K, int64_t ldp, int n, float2 *__restrict__ diag, float2 *__restrict__ raw,
                                                  float2 *__restrict__ inv)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float2 d = reinterpret_cast<const float2 *>(K + (int64_t)i * ldp)[i];
    if (diag) diag[i] = d;
    raw[i] = d;
    inv[i] = c64_div(make_float2(1.f, 0.f), d);
}

// z = inv .* x
__global__ __launch_bounds__(256) void k_cdn_scale(int n, const float2 *__restrict__ inv, const float2 *__restrict__ x, float2 *__restrict__ z,
                                                   const int *done)
{
    if (done && *done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) z[i] = c64_mul(inv[i], x[i]);
}

// ---- work memory -----------------------------------------------------------------------------------------------------------------
// entries (float pairs) of the single-vector slot table: the split row form under either plan, the column form
static int64_t cdn_table_entries(int M, int N, int NP)
{
    int64_t need = 0;
    for (int forced = 0; forced < 2; forced++) need = std::max(need, (int64_t)row_plan(M, NP, true, forced).S * M);
    return std::max(need, (int64_t)col_plan(M, NP).RS * N) + 2;
}
// entries of the k-wide slot table per column of the block: the split row form under either plan
static int64_t cdnm_table_entries(int M, int NP)
{
    int64_t need = 0;
    for (int forced = 0; forced < 2; forced++) need = std::max(need, (int64_t)row_plan(M, NP, true, forced).S * M);
    return need;
}

int cdnm_reserve(lcg_hip_dense *K, int k)
{
    if (!K->multi) K->multi = new DenseMulti;
    DenseMulti *w = K->multi;
    if (k <= w->kmax) return 0;
    if (w->kmax) HIPCHK(hipStreamSynchronize(ctx().stream));
    if (w->part) (void)hipFree(w->part);
    w->part = nullptr; w->kmax = 0;
    HIPCHK(hipMalloc(&w->part, sizeof(float) * 2 * (size_t)cdnm_table_entries(K->M, K->NP) * k + 16));
    w->kmax = k;
    return 0;
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------
static void cdn_fold_launch(const float *part, int S, int64_t n, float *y, hipStream_t s, const int *done)
{
    hipLaunchKernelGGL(k_cdn_fold, dim3((unsigned)cdiv(n, CFOLD_J)), dim3(CFOLD_Q * CFOLD_J), 0, s, part, S, n, y, done);
}

template <bool CONJ>
static void cdn_row_dispatch(const lcg_hip_dense *K, const RowPlan &r, const float2 *x, float2 *out, hipStream_t s, const int *done)
{
    const dim3 grid((unsigned)cdiv(K->M, 256 / r.W), (unsigned)r.S);
    const cf4 *val = reinterpret_cast<const cf4 *>(K->val);
#define CDN_ROW_CASE(w) case w: hipLaunchKernelGGL((k_cdn_row<CONJ, w>), grid, dim3(256), 0, s, val, K->ldp, K->M, K->N, K->NP, r.pps, x, out, done); break;
    switch (r.W) { CDN_ROW_CASE(4) CDN_ROW_CASE(8) CDN_ROW_CASE(16) CDN_ROW_CASE(32) default: CDN_ROW_CASE(64) }
#undef CDN_ROW_CASE
}

// y[M] = K.x or conj(K).x
static int cdn_row_product(lcg_hip_dense *K, const float *x, float *y, int conjugate, hipStream_t s, const int *done)
{
    const bool forced = K->variant == DN_ROW_SPLIT;
    const bool split = forced || (K->variant != DN_ROW && row_split_auto(K->M, K->NP));
    const RowPlan r = row_plan(K->M, K->NP, split, forced);
    float *part = reinterpret_cast<float *>(K->part);
    float2 *out = reinterpret_cast<float2 *>(r.S > 1 ? part : y);
    if (conjugate) cdn_row_dispatch<true>(K, r, reinterpret_cast<const float2 *>(x), out, s, done);
    else cdn_row_dispatch<false>(K, r, reinterpret_cast<const float2 *>(x), out, s, done);
    if (r.S > 1) cdn_fold_launch(part, r.S, 2 * (int64_t)K->M, y, s, done);
    K->last_kernel = CDN_NAMES[r.S > 1 ? 1 : 0];
    return launched("complex64 dense row product");
}

// y[N] = K^T.x or K^H.x
static int cdn_col_product(lcg_hip_dense *K, const float *x, float *y, int conjugate, hipStream_t s, const int *done)
{
    const ColPlan c = col_plan(K->M, K->NP);
    float *part = reinterpret_cast<float *>(K->part);
    float2 *out = reinterpret_cast<float2 *>(c.RS > 1 ? part : y);
    const dim3 grid((unsigned)c.CT, (unsigned)c.RS);
    const cf4 *val = reinterpret_cast<const cf4 *>(K->val);
    const float2 *xv = reinterpret_cast<const float2 *>(x);
    if (conjugate) hipLaunchKernelGGL((k_cdn_col<true>), grid, dim3(256), 0, s, val, K->ldp, K->M, K->N, K->NP, c.CW, c.rps, xv, out, done);
    else hipLaunchKernelGGL((k_cdn_col<false>), grid, dim3(256), 0, s, val, K->ldp, K->M, K->N, K->NP, c.CW, c.rps, xv, out, done);
    if (c.RS > 1) cdn_fold_launch(part, c.RS, 2 * (int64_t)K->N, y, s, done);
    K->last_kernel = CDN_NAMES[2];
    return launched("complex64 dense column product");
}

// Y[M x k] = K.X or conj(K).X; the handle's forced ROW / ROW_SPLIT reach it as they reach the single-vector row form
static int cdnm_product(lcg_hip_dense *K, int k, const float *X, float *Y, int conjugate, hipStream_t s, const int *done, int *launches)
{
    const bool forced = K->variant == DN_ROW_SPLIT;
    const bool split = forced || (K->variant != DN_ROW && row_split_auto(K->M, K->NP));
    const RowPlan r = row_plan(K->M, K->NP, split, forced);
    float *part = reinterpret_cast<float *>(K->multi->part);
    float *out = r.S > 1 ? part : Y;
    const dim3 grid((unsigned)cdiv(K->M, 16), (unsigned)r.S);
    const cf4 *val = reinterpret_cast<const cf4 *>(K->val);
    if (conjugate) hipLaunchKernelGGL((k_cdnm_mfma<true>), grid, dim3(256), 0, s, val, K->ldp, K->M, K->N, K->NP, r.pps, k, X, out, done);
    else hipLaunchKernelGGL((k_cdnm_mfma<false>), grid, dim3(256), 0, s, val, K->ldp, K->M, K->N, K->NP, r.pps, k, X, out, done);
    if (r.S > 1) cdn_fold_launch(part, r.S, 2 * (int64_t)K->M * k, Y, s, done);
    *launches += r.S > 1 ? 2 : 1;
    K->multi->last_kernel = CDN_NAMES[r.S > 1 ? 4 : 3];
    return launched("complex64 dense k-wide product");
}

int cdnm_op(lcg_hip_dense *K, int k, const float *X, float *Y, hipStream_t s, const int *done, const float *U, double *dots, int *slots,
            int *launches)
{
    int rc = cdnm_product(K, k, X, Y, 0, s, done, launches);
    if (rc || !U) return rc;
    const int n = K->N;
    const int rpb = 64 * (int)cdiv(cdiv(n, 64), MM_MG), nb = (int)cdiv(n, rpb);
    multi_k(k, [&](auto KK) {
        hipLaunchKernelGGL((k_cdnm_dot<decltype(KK)::value>), dim3(nb), dim3(32 * decltype(KK)::value), 0, s, Y, U, n, rpb, dots, done);
        return 0;
    });
    (*launches)++;
    *slots = nb;
    return launched("complex64 dense k-wide dot");
}

lcg_hip_dense *cdn_handle(const char *entry, const void *h)
{
    if (dense_handle(h)) {
        lcg_hip_dense *K = static_cast<lcg_hip_dense *>(const_cast<void *>(h));
        if (K->c64) return K;
    }
    arg_error("%s: the handle is not a complex64 dense matrix (lcg_hip_dense_create_c64)", entry);
    return nullptr;
}

static void cdn_release(lcg_hip_dense *K)
{
    if (K->val) (void)hipFree(K->val);
    if (K->part) (void)hipFree(K->part);
    delete K;
}

static void cdn_park(int rc) { if (rc && !ctx().ax_rc) ctx().ax_rc = rc; }

static int cdn_matvec(const char *entry, lcg_hip_dense_t Kh, const float *x, float *y, int layout, int conjugate)
{
    // (what needs no handle first, the way the k-wide entries look at k and their blocks first)
    if (!x || !y) return arg_error("%s: x or y is NULL", entry);
    if (x == y) return arg_error("%s: x and y are the same vector", entry);
    if (layout < 0 || layout > 1 || conjugate < 0 || conjugate > 1) return arg_error("%s: layout = %d, conjugate = %d", entry, layout, conjugate);
    lcg_hip_dense *K = cdn_handle(entry, Kh);
    if (!K) return LCG_HIP_E_ARG;
    Ctx &c = ctx();
    return layout ? cdn_col_product(K, x, y, conjugate, c.stream, ax_flag(c)) : cdn_row_product(K, x, y, conjugate, c.stream, ax_flag(c));
}

static int cdn_jacobi(void *instance, const float *x, float *z, int n)
{
    const char *entry = "clcg_hip_dense_jacobi_mx_c64";
    lcg_hip_dense *K = cdn_handle(entry, instance);
    if (!K) return LCG_HIP_E_ARG;
    if (!K->invdiag) return arg_error("%s: lcg_hip_dense_build_jacobi_c64() was not called", entry);
    if (n != K->N) return arg_error("%s: n_size = %d, the matrix has %d rows", entry, n, K->N);
    if (!x || !z) return arg_error("%s: x or z is NULL", entry);
    Ctx &c = ctx();
    hipLaunchKernelGGL(k_cdn_scale, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, c.stream, n, reinterpret_cast<const float2 *>(K->invdiag),
                       reinterpret_cast<const float2 *>(x), reinterpret_cast<float2 *>(z), ax_flag(c));
    return launched(entry);
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_dense_create_c64(lcg_hip_dense_t *out, int m_rows, int n_cols, const float *val, int64_t ld, int mem)
{
    const char *entry = "lcg_hip_dense_create_c64";
    if (!out) return arg_error("%s: the handle pointer is NULL", entry);
    *out = nullptr;
    if (!val) return arg_error("%s: val is NULL", entry);
    if (m_rows <= 0 || n_cols <= 0) return arg_error("%s: M = %d, N = %d (both must be positive)", entry, m_rows, n_cols);
    if (ld < n_cols) return arg_error("%s: ld = %lld < N = %d", entry, (long long)ld, n_cols);
    if (mem != LCG_HIP_MEM_HOST && mem != LCG_HIP_MEM_DEVICE) return arg_error("%s: mem = %d", entry, mem);
    TRY(ensure_init());
    Ctx &c = ctx();
    lcg_hip_dense *K = new lcg_hip_dense;
    K->M = m_rows; K->N = n_cols; K->c64 = true;
    K->NP = (n_cols + 1) / 2;
    K->ldp = K->NP;
    const size_t bytes = (size_t)m_rows * (size_t)K->ldp * 16 + 64;
    K->part_doubles = cdn_table_entries(m_rows, n_cols, K->NP);        // (8 bytes each: a float pair)
    hipError_t e = hipMalloc(&K->val, bytes);
    if (e == hipSuccess) e = hipMalloc(&K->part, 8 * (size_t)K->part_doubles);
    if (e == hipSuccess) e = hipMemsetAsync(K->val, 0, bytes, c.stream);
    const hipMemcpyKind kind = mem == LCG_HIP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(K->val, (size_t)K->ldp * 16, val, (size_t)ld * 8, (size_t)n_cols * 8, (size_t)m_rows, kind, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) { cdn_release(K); return fail(e, "complex64 dense matrix allocation or copy", __FILE__, __LINE__); }
    *out = K;
    return 0;
}

int clcg_hip_dense_matvec_c64(lcg_hip_dense_t K, const float *x, float *y, int layout, int conjugate)
{
    return cdn_matvec("clcg_hip_dense_matvec_c64", K, x, y, layout, conjugate);
}

void clcg_hip_dense_ax_c64(void *instance, const float *x, float *prod_Ax, const int n_size, int layout, int conjugate)
{
    const char *entry = "clcg_hip_dense_ax_c64";
    lcg_hip_dense *K = cdn_handle(entry, instance);
    if (!K) return cdn_park(LCG_HIP_E_ARG);
    if (K->M != K->N) return cdn_park(arg_error("%s: the matrix is %d x %d, not square", entry, K->M, K->N));
    if (n_size != K->N) return cdn_park(arg_error("%s: n_size = %d, the matrix has %d rows", entry, n_size, K->N));
    cdn_park(cdn_matvec(entry, K, x, prod_Ax, layout, conjugate));
}

void clcg_hip_dense_jacobi_mx_c64(void *instance, const float *x, float *prod_Mx, const int n_size, int layout, int conjugate)
{
    (void)layout; (void)conjugate;      // as clcg_hip_jacobi_mx_c64: the diagonal is its own transpose, and the loops ask for (0, 0)
    cdn_park(cdn_jacobi(instance, x, prod_Mx, n_size));
}

int lcg_hip_dense_build_jacobi_c64(lcg_hip_dense_t Kh, float *diag_out)
{
    const char *entry = "lcg_hip_dense_build_jacobi_c64";
    lcg_hip_dense *K = cdn_handle(entry, Kh);
    if (!K) return LCG_HIP_E_ARG;
    if (K->M != K->N) return arg_error("%s: the matrix is %d x %d: its diagonal needs a square one", entry, K->M, K->N);
    Ctx &c = ctx();
    const int n = K->N;
    // the reciprocals in the first n float pairs, the diagonal itself (for the check below) in the n behind them
    if (!K->invdiag) HIPCHK(hipMalloc(&K->invdiag, 16 * (size_t)n));
    float2 *inv = reinterpret_cast<float2 *>(K->invdiag);
    hipLaunchKernelGGL(k_cdn_diag, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, c.stream, reinterpret_cast<const cf4 *>(K->val), K->ldp, n,
                       reinterpret_cast<float2 *>(diag_out), inv + n, inv);
    TRY(launched(entry));
    std::vector<float> d(2 * (size_t)n);
    HIPCHK(hipMemcpyAsync(d.data(), inv + n, 8 * (size_t)n, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    for (int i = 0; i < n; i++) {
        const float a = d[2 * (size_t)i], b = d[2 * (size_t)i + 1];
        if ((a == 0.f && b == 0.f) || !std::isfinite(a) || !std::isfinite(b)) {
            (void)hipFree(K->invdiag); K->invdiag = nullptr;
            return arg_error("%s: diagonal entry %d is (%g, %g)", entry, i, a, b);
        }
    }
    return 0;
}

int clcg_hip_dense_matmat_c64(lcg_hip_dense_t Kh, int k, const float *X, float *Y, int conjugate)
{
    const char *entry = "clcg_hip_dense_matmat_c64";
    TRY(multi_args(entry, k, X, Y));
    if (conjugate < 0 || conjugate > 1) return arg_error("%s: conjugate = %d (0: K.X, 1: conj(K).X)", entry, conjugate);
    lcg_hip_dense *K = cdn_handle(entry, Kh);
    if (!K) return LCG_HIP_E_ARG;
    if (overlap(X, 8 * (size_t)K->N * k, Y, 8 * (size_t)K->M * k)) return arg_error("%s: X and Y overlap", entry);
    TRY(ensure_init());
    TRY(cdnm_reserve(K, k));
    int launches = 0;
    return cdnm_product(K, k, X, Y, conjugate, ctx().stream, nullptr, &launches);
}

int clcg_hip_dense_op_multi_dot_c64(lcg_hip_dense_t Kh, int k, const float *X, float *Y, const float *U, double *dots)
{
    const char *entry = "clcg_hip_dense_op_multi_dot_c64";
    TRY(multi_args(entry, k, X, Y, U ? (const void *)U : (const void *)16));
    lcg_hip_dense *K = cdn_handle(entry, Kh);
    if (!K) return LCG_HIP_E_ARG;
    if (K->M != K->N) return arg_error("%s: the matrix is %d x %d: the loops' operator needs a square one", entry, K->M, K->N);
    const size_t nv = 8 * (size_t)K->N * k;
    if (overlap(X, nv, Y, nv) || (U && overlap(U, nv, Y, nv))) return arg_error("%s: Y overlaps X or U", entry);
    if (dots && !U) return arg_error("%s: dots without U", entry);
    TRY(ensure_init());
    TRY(cdnm_reserve(K, k));
    Ctx &c = ctx();
    // (outside a solve the k-wide table of the loops is free: partials_pair[0] holds the partial sums, ax_partials the results)
    int slots = 0, launches = 0;
    TRY(cdnm_op(K, k, X, Y, c.stream, nullptr, U, c.partials_pair[0], &slots, &launches));
    return U && dots ? multi_dots_read(c, 2 * k, slots, dots) : 0;
}

const char *clcg_hip_dense_kernel_name_c64(int index)
{
    return index >= 0 && index < (int)(sizeof CDN_NAMES / sizeof *CDN_NAMES) ? CDN_NAMES[index] : nullptr;
}

} // extern "C"
