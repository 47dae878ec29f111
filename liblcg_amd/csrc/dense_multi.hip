// dense_multi.hip -- dense operators over k = 2, 4, 8 right-hand sides: K.X, K^T.X, K^T.(K.X) with K read ONCE for all k columns,
// and the operator of the batched loops (solvers_multi.hip: lcg_hip_dense_lcg_multi, lcg_hip_dense_lpcg_multi; solvers_multi_cplx.hip:
// the complex ones) with the sum they take after it.  One GPU.  The kernels and the host flow serve real fp64 and complex128 handles;
// the real entries are here, the complex ones in dense_multi_cplx.hip.  A real handle that stores K as fp32 runs the
// *_f32 twins of the real kernels under the same plans and gives the fp64 handle's bits.  DESIGN.md sections 19, 20 and 27.
//
// Blocks of vectors are multi.hpp's: X[i * k + j] is row i of column j, the base 16-byte aligned (complex: multi_cplx.hpp's, column j
// of row i is the 16-byte piece i * k + j).  The kernels are the k-wide twins of dense.hip's, on the same storage (rows of 16-byte
// packs, pads zero) and under the SAME plans (dense.hpp: functions of the shape and the forced variant, never of k).  The column form
// is one template over what a pack is -- two real columns or one complex entry: the element trait E = DnReal<K> or DnCplx<K, CONJ> --
// and the carried sum one over (K, complex); the row forms are two kernels (why: above k_dnm_row).  The real forms:
//
//   k_dnm_row<K, W>   Y(i,:) = sum_j K(i,j) X(j,:)   W lanes per group of k / 2 rows; a lane loads one pack of K per row and access and,
//                     for the pack's two columns, rows 2p and 2p + 1 of X (2k contiguous doubles) once for its rows; K accumulators
//                     per row; butterfly over the W lanes; whole rows of Y.  Columns cut into strips over gridDim.y
//                     (k_dnm_row_split): one slot of M * k values per strip
//   k_dnm_col<E, K>   Y(j,:) = sum_i K(i,j) X(i,:)   thread (cp, rg) owns one pack of columns and walks a strip of rows, reading the
//                     k values X(i,:) per row (one address for all lanes of a row group); 2k accumulators; the row groups meet in
//                     LDS in rg order; one slot of N * k values per strip of rows
//   k_dnm_fold        the slots added in one fixed order; dense.hip's single-vector split forms fold with it too
//   k_dnm_dot<K, CX>  column j's Y_j . U_j left as <= MM_MG partial sums in the table format spmm_launch leaves (multi.hpp), one
//                     launch over the two N x k blocks: no pass over K
//
// (the complex forms: dense_multi_cplx.hip's header.)
// Every multiply-add is an explicit fma and every sum is added in an order fixed by the shape alone, so column j's bits depend on
// K, the handle's forced variant and column j of X (and U) -- not on k, not on what the other columns hold, not on the call.  No
// atomics.  Every kernel falls through when the batch has stopped (`done`).
#include "dense.hpp"
#include "multi.hpp"

namespace lcgh {

static const char *const DNM_NAMES[] = {"k_dnm_row", "k_dnm_row_split", "k_dnm_col", "k_dnm_ata_two_pass"};
static const char *const ZDNM_NAMES[] = {"k_zdnm_row", "k_zdnm_row_split", "k_zdnm_col"};

const char *dnm_kernel_name(bool cplx, int index)
{
    const int n = cplx ? (int)(sizeof ZDNM_NAMES / sizeof *ZDNM_NAMES) : (int)(sizeof DNM_NAMES / sizeof *DNM_NAMES);
    return index >= 0 && index < n ? (cplx ? ZDNM_NAMES : DNM_NAMES)[index] : nullptr;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// acc(:) += a * x(:), one rounding per column and term
template <int K2>
__device__ __forceinline__ void fma_row(m2d *acc, double a, const m2d *x)
{
#pragma unroll
    for (int h = 0; h < K2; h++) { acc[h].x = fma(a, x[h].x, acc[h].x); acc[h].y = fma(a, x[h].y, acc[h].y); }
}

// acc(:) += op(a) * x(:): per column zfma's order (solvers_multi_cplx.hip; cfma in devcommon.hpp), one pair of fmas per component
template <int K, bool CONJ>
__device__ __forceinline__ void zfma_row(m2d *acc, double2 a, const m2d *x)
{
    const double ai = CONJ ? -a.y : a.y;
#pragma unroll
    for (int h = 0; h < K; h++) {
        acc[h].x = fma(a.x, x[h].x, fma(-ai, x[h].y, acc[h].x));
        acc[h].y = fma(a.x, x[h].y, fma(ai, x[h].x, acc[h].y));
    }
}

// Rows a group of the complex row form owns, a function of K alone: four at every K.  A lane loads 16 k bytes of X per pack whatever the
// rows are, W rows of X a wavefront instruction, and the vector cache takes them a 128-byte line at a time: 8 k^2 lines per 64 packs (16,
// 32 and 64 lines per 16-byte load at k = 2, 4, 8), against 16 cycles for a coalesced load of K.  The rows share that cost.  At k = 8
// four rows are 32 complex accumulators = 128 VGPRs and the kernel compiles to 256 VGPRs plus 12 .. 16 AGPR copies, ONE wavefront per
// SIMD; two rows compile to 166 VGPRs and three wavefronts.  Both were measured: 8192^2 and 16384^2 at k = 8 run at 58 %
// and 64 % of the read rate with four rows, 34 % with two -- the lines decide, not the occupancy.
constexpr int zrr(int) { return 4; }

// What a pack of K is to the column form.  A row of a block of vectors is A 16-byte pieces and a pack writes OR rows of Y (OR * A = K
// pieces either way).  real: a pack is two columns of K, rows 2p and 2p + 1 of Y; complex: one entry, op(K) = K or conj(K), row p.
template <int K>
struct DnReal {
    static constexpr int A = K / 2, OR = 2;
    static constexpr int COL_UN = K == 8 ? 4 : 8;       // rows a thread keeps in flight
    static __device__ __forceinline__ void col_term(m2d *acc, double2 kk, const m2d *x) { fma_row<A>(acc, kk.x, x); fma_row<A>(acc + A, kk.y, x); }
};
template <int K, bool CONJ>
struct DnCplx {
    static constexpr int A = K, OR = 1;
    static constexpr int COL_UN = 16 / K;
    static __device__ __forceinline__ void col_term(m2d *acc, double2 kk, const m2d *x) { zfma_row<K, CONJ>(acc, kk, x); }
};

// The row forms stay two kernels.  As one template over the element trait they compiled to the same registers, LDS and occupancy, but
// not to the same code for the real K = 4 and K = 8 instantiations, and the real K = 8 product at 8192^2 measured 0.5 % below the parent in
// three alternating runs out of three (profiles/multi_product_rates.txt).
// The fp32 twins (k_dnm_row_f32, k_dnm_col_f32: a handle made by lcg_hip_dense_create_f32) are copies for the same reason: with one
// body shared between the two pack types, 24 of this file's 61 kernels compiled to other instructions; beside the copies all are
// identical to what they were.

// one pack of row i (columns 2p, 2p + 1) times rows 2p and 2p + 1 of X.  Odd N: the last pack's pad entry never reads row N of X
template <int K2>
__device__ __forceinline__ void row_xload(m2d *xa, m2d *xb, const m2d *Xv, int p, int N)
{
    const int64_t j = 2 * (int64_t)p;
    const bool two = j + 1 < N;
#pragma unroll
    for (int h = 0; h < K2; h++) xa[h] = Xv[j * K2 + h];
#pragma unroll
    for (int h = 0; h < K2; h++) xb[h] = two ? Xv[(j + 1) * K2 + h] : (m2d)(0.0);
}

// Row form.  The W lanes of group g = blockIdx.x * (256 / W) + tid / W own the RR = K / 2 consecutive rows g * RR ...; they take the packs
// [p0, p1) of strip blockIdx.y, W apart (k_dn_row's mapping and, per row, its order of additions).  A lane loads the rows 2p, 2p + 1 of
// X ONCE for its RR rows of K: the 2K doubles of X per 16-byte pack of K would otherwise be K times the matrix's bytes through the
// vector cache; with RR rows they are twice, whatever K is.  Slot blockIdx.y of out holds M * K values (S == 1: out = Y).
template <int K, int W>
__global__ __launch_bounds__(256) void k_dnm_row(const double2 *__restrict__ Kv, int64_t ldp, int M, int N, int NP, int pps,
                                                 const double *__restrict__ X, double *__restrict__ out, const int *done)
{
    constexpr int K2 = K / 2, RR = K / 2;
    constexpr int UN = K == 2 ? 4 : 2;      // packs a lane keeps in flight (each: RR packs of K and 2K doubles of X)
    if (done && *done) return;
    const int sub = threadIdx.x % W;
    const int64_t i0 = ((int64_t)blockIdx.x * (256 / W) + threadIdx.x / W) * RR;
    const int p0 = blockIdx.y * pps;
    const int p1 = i0 < M ? min(NP, p0 + pps) : p0;       // (a group beyond M walks nothing but still joins the butterfly)
    const double2 *row[RR];
#pragma unroll
    for (int r = 0; r < RR; r++) row[r] = Kv + min(i0 + r, (int64_t)M - 1) * ldp;     // (rows beyond M re-read the last one; never written)
    const m2d *Xv = reinterpret_cast<const m2d *>(X);
    m2d acc[RR][K2];
#pragma unroll
    for (int r = 0; r < RR; r++)
#pragma unroll
        for (int h = 0; h < K2; h++) acc[r][h] = (m2d)(0.0);
    int p = p0 + sub;
    for (; p + (UN - 1) * W < p1; p += UN * W) {
        double2 kk[UN][RR];
        m2d xa[UN][K2], xb[UN][K2];
#pragma unroll
        for (int u = 0; u < UN; u++)
#pragma unroll
            for (int r = 0; r < RR; r++) kk[u][r] = row[r][p + u * W];
#pragma unroll
        for (int u = 0; u < UN; u++) row_xload<K2>(xa[u], xb[u], Xv, p + u * W, N);
#pragma unroll
        for (int u = 0; u < UN; u++)
#pragma unroll
            for (int r = 0; r < RR; r++) { fma_row<K2>(acc[r], kk[u][r].x, xa[u]); fma_row<K2>(acc[r], kk[u][r].y, xb[u]); }
    }
    for (; p < p1; p += W) {
        m2d xa[K2], xb[K2];
        row_xload<K2>(xa, xb, Xv, p, N);
#pragma unroll
        for (int r = 0; r < RR; r++) {
            const double2 kk = row[r][p];
            fma_row<K2>(acc[r], kk.x, xa); fma_row<K2>(acc[r], kk.y, xb);
        }
    }
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int r = 0; r < RR; r++)
#pragma unroll
            for (int h = 0; h < K2; h++) { acc[r][h].x += __shfl_xor(acc[r][h].x, o, W); acc[r][h].y += __shfl_xor(acc[r][h].y, o, W); }
    }
    if (sub == 0) {
#pragma unroll
        for (int r = 0; r < RR; r++) {
            if (i0 + r < M) {
                m2d *o = reinterpret_cast<m2d *>(out) + ((int64_t)blockIdx.y * M + i0 + r) * K2;
#pragma unroll
                for (int h = 0; h < K2; h++) o[h] = acc[r][h];
            }
        }
    }
}

// k_dnm_row on fp32 packs (an fp32 handle): the same lanes, packs and order of additions behind ldpack's widening load.
// A copy, not a shared template: see above.  fp32 packs are half the bytes, so a lane keeps twice as many in flight where the registers
// allow it -- at K = 8 the rows of X in flight, not the packs, fill them
template <int K, int W>
__global__ __launch_bounds__(256) void k_dnm_row_f32(const float2 *__restrict__ Kv, int64_t ldp, int M, int N, int NP, int pps,
                                                     const double *__restrict__ X, double *__restrict__ out, const int *done)
{
    constexpr int K2 = K / 2, RR = K / 2;
    constexpr int UN = K == 2 ? 8 : K == 4 ? 4 : 2;
    if (done && *done) return;
    const int sub = threadIdx.x % W;
    const int64_t i0 = ((int64_t)blockIdx.x * (256 / W) + threadIdx.x / W) * RR;
    const int p0 = blockIdx.y * pps;
    const int p1 = i0 < M ? min(NP, p0 + pps) : p0;       // (a group beyond M walks nothing but still joins the butterfly)
    const float2 *row[RR];
#pragma unroll
    for (int r = 0; r < RR; r++) row[r] = Kv + min(i0 + r, (int64_t)M - 1) * ldp;     // (rows beyond M re-read the last one; never written)
    const m2d *Xv = reinterpret_cast<const m2d *>(X);
    m2d acc[RR][K2];
#pragma unroll
    for (int r = 0; r < RR; r++)
#pragma unroll
        for (int h = 0; h < K2; h++) acc[r][h] = (m2d)(0.0);
    int p = p0 + sub;
    for (; p + (UN - 1) * W < p1; p += UN * W) {
        double2 kk[UN][RR];
        m2d xa[UN][K2], xb[UN][K2];
#pragma unroll
        for (int u = 0; u < UN; u++)
#pragma unroll
            for (int r = 0; r < RR; r++) kk[u][r] = ldpack(row[r] + p + u * W);
#pragma unroll
        for (int u = 0; u < UN; u++) row_xload<K2>(xa[u], xb[u], Xv, p + u * W, N);
#pragma unroll
        for (int u = 0; u < UN; u++)
#pragma unroll
            for (int r = 0; r < RR; r++) { fma_row<K2>(acc[r], kk[u][r].x, xa[u]); fma_row<K2>(acc[r], kk[u][r].y, xb[u]); }
    }
    for (; p < p1; p += W) {
        m2d xa[K2], xb[K2];
        row_xload<K2>(xa, xb, Xv, p, N);
#pragma unroll
        for (int r = 0; r < RR; r++) {
            const double2 kk = ldpack(row[r] + p);
            fma_row<K2>(acc[r], kk.x, xa); fma_row<K2>(acc[r], kk.y, xb);
        }
    }
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int r = 0; r < RR; r++)
#pragma unroll
            for (int h = 0; h < K2; h++) { acc[r][h].x += __shfl_xor(acc[r][h].x, o, W); acc[r][h].y += __shfl_xor(acc[r][h].y, o, W); }
    }
    if (sub == 0) {
#pragma unroll
        for (int r = 0; r < RR; r++) {
            if (i0 + r < M) {
                m2d *o = reinterpret_cast<m2d *>(out) + ((int64_t)blockIdx.y * M + i0 + r) * K2;
#pragma unroll
                for (int h = 0; h < K2; h++) o[h] = acc[r][h];
            }
        }
    }
}

template <int K>
__device__ __forceinline__ void zx_load(m2d *x, const m2d *Xv, int64_t row)
{
#pragma unroll
    for (int h = 0; h < K; h++) x[h] = Xv[row * K + h];
}


// Row form.  The W lanes of group g = blockIdx.x * (256 / W) + tid / W own the ZRR = zrr(K) consecutive rows g * ZRR ...; they take the packs
// [p0, p1) of strip blockIdx.y, W apart (k_dn_row's mapping and, per row, its order of additions).  A lane loads row p of X ONCE for
// its ZRR rows of K.  Slot blockIdx.y of out holds M * K complex values (S == 1: out = Y).
template <int K, int W, bool CONJ>
__global__ __launch_bounds__(256) void k_zdnm_row(const double2 *__restrict__ Kv, int64_t ldp, int M, int NP, int pps,
                                                  const double *__restrict__ X, double *__restrict__ out, const int *done)
{
    constexpr int ZRR = zrr(K);
    constexpr int UN = 8 / K;                // packs a lane keeps in flight (each: ZRR entries of K and K of X)
    if (done && *done) return;
    const int sub = threadIdx.x % W;
    const int64_t i0 = ((int64_t)blockIdx.x * (256 / W) + threadIdx.x / W) * ZRR;
    const int p0 = blockIdx.y * pps;
    const int p1 = i0 < M ? min(NP, p0 + pps) : p0;       // (a group beyond M walks nothing but still joins the butterfly)
    const double2 *row[ZRR];
#pragma unroll
    for (int r = 0; r < ZRR; r++) row[r] = Kv + min(i0 + r, (int64_t)M - 1) * ldp;    // (rows beyond M re-read the last one; never written)
    const m2d *Xv = reinterpret_cast<const m2d *>(X);
    m2d acc[ZRR][K];
#pragma unroll
    for (int r = 0; r < ZRR; r++)
#pragma unroll
        for (int h = 0; h < K; h++) acc[r][h] = (m2d)(0.0);
    int p = p0 + sub;
    for (; p + (UN - 1) * W < p1; p += UN * W) {
        double2 kk[UN][ZRR];
        m2d xv[UN][K];
#pragma unroll
        for (int u = 0; u < UN; u++)
#pragma unroll
            for (int r = 0; r < ZRR; r++) kk[u][r] = row[r][p + u * W];
#pragma unroll
        for (int u = 0; u < UN; u++) zx_load<K>(xv[u], Xv, p + u * W);
#pragma unroll
        for (int u = 0; u < UN; u++)
#pragma unroll
            for (int r = 0; r < ZRR; r++) zfma_row<K, CONJ>(acc[r], kk[u][r], xv[u]);
    }
    for (; p < p1; p += W) {
        m2d xv[K];
        zx_load<K>(xv, Xv, p);
#pragma unroll
        for (int r = 0; r < ZRR; r++) zfma_row<K, CONJ>(acc[r], row[r][p], xv);
    }
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int r = 0; r < ZRR; r++)
#pragma unroll
            for (int h = 0; h < K; h++) { acc[r][h].x += __shfl_xor(acc[r][h].x, o, W); acc[r][h].y += __shfl_xor(acc[r][h].y, o, W); }
    }
    if (sub == 0) {
#pragma unroll
        for (int r = 0; r < ZRR; r++) {
            if (i0 + r < M) {
                m2d *o = reinterpret_cast<m2d *>(out) + ((int64_t)blockIdx.y * M + i0 + r) * K;
#pragma unroll
                for (int h = 0; h < K; h++) o[h] = acc[r][h];
            }
        }
    }
}

// y[j] = the sum of the table's S slots of n doubles each, in a fixed order: the slots are cut into MFOLD_Q runs of consecutive slots,
// thread (q, j) adds run q's slots in index order (eight independent loads at a time), and the runs' sums are added in run order.  16
// outputs per workgroup.  The ONE fold of the dense units: it adds doubles and does not care what they are, so the single-vector forms
// (dense.hip, done = nullptr) and the complex ones fold with it too.
constexpr int MFOLD_Q = 16, MFOLD_J = 16;
__global__ __launch_bounds__(MFOLD_Q * MFOLD_J) void k_dnm_fold(const double *__restrict__ part, int S, int64_t n, double *__restrict__ y,
                                                                const int *done)
{
    __shared__ double sh[MFOLD_Q][MFOLD_J];
    if (done && *done) return;
    const int jj = threadIdx.x % MFOLD_J, q = threadIdx.x / MFOLD_J;
    const int64_t j = (int64_t)blockIdx.x * MFOLD_J + jj;
    const int L = (S + MFOLD_Q - 1) / MFOLD_Q;
    const int k0 = q * L, k1 = min(S, k0 + L);
    double s = 0.0;
    if (j < n) {
        int k = k0;
        for (; k + 7 < k1; k += 8) {
            double v[8];
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
        for (int g = 1; g < MFOLD_Q; g++) s += sh[g][jj];
        y[j] = s;
    }
}

// Column form (k_dn_col's mapping).  A workgroup owns CW packs of columns (blockIdx.x) and the rows [r0, r0 + rps) (blockIdx.y); thread
// (cp, rg) walks the rows r0 + rg, r0 + rg + RG, ... of pack cp, reading row i of X (one address for all lanes of a row group).  The RG
// sums of a pack are added in rg order, then written as the pack's OR rows of slot blockIdx.y of out: K pieces from piece p * K on (real:
// rows 2p and 2p + 1, the second only where N has it; n_out doubles per slot; gridDim.y == 1: out = Y).
template <class E, int K>
__global__ __launch_bounds__(256) void k_dnm_col(const double2 *__restrict__ Kv, int64_t ldp, int M, int N, int NP, int CW, int rps,
                                                 const double *__restrict__ X, double *__restrict__ out, int64_t n_out, const int *done)
{
    constexpr int A = E::A, UN = E::COL_UN;
    static_assert(E::OR * A == K, "a pack's sums are K pieces");
    __shared__ m2d sh[K][256];
    if (done && *done) return;
    const int RG = 256 / CW;
    const int cp = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int p = blockIdx.x * CW + cp;
    const bool live = p < NP;
    const int r0 = blockIdx.y * rps, r1 = min(M, r0 + rps);
    const m2d *Xv = reinterpret_cast<const m2d *>(X);
    m2d acc[K];
#pragma unroll
    for (int h = 0; h < K; h++) acc[h] = (m2d)(0.0);
    if (live) {
        const double2 *col = Kv + p;
        int i = r0 + rg;
        for (; i + (UN - 1) * RG < r1; i += UN * RG) {
            double2 kk[UN];
            m2d xv[UN][A];
#pragma unroll
            for (int u = 0; u < UN; u++) kk[u] = col[(int64_t)(i + u * RG) * ldp];
#pragma unroll
            for (int u = 0; u < UN; u++)
#pragma unroll
                for (int h = 0; h < A; h++) xv[u][h] = Xv[(int64_t)(i + u * RG) * A + h];
#pragma unroll
            for (int u = 0; u < UN; u++) E::col_term(acc, kk[u], xv[u]);
        }
        for (; i < r1; i += RG) {
            const double2 kk = col[(int64_t)i * ldp];
            m2d xv[A];
#pragma unroll
            for (int h = 0; h < A; h++) xv[h] = Xv[(int64_t)i * A + h];
            E::col_term(acc, kk, xv);
        }
    }
    if (RG > 1) {       // (uniform over the workgroup)
#pragma unroll
        for (int h = 0; h < A; h++) {
            sh[h][threadIdx.x] = acc[h];
            if (E::OR == 2) sh[A + h][threadIdx.x] = acc[A + h];
        }
        __syncthreads();
        if (rg == 0)
            for (int g = 1; g < RG; g++) {
#pragma unroll
                for (int h = 0; h < A; h++) {
                    acc[h] += sh[h][g * CW + cp];
                    if (E::OR == 2) acc[A + h] += sh[A + h][g * CW + cp];
                }
            }
    }
    if (rg == 0 && live) {
        const int64_t j = E::OR * (int64_t)p;           // the pack's first row of Y
        m2d *o = reinterpret_cast<m2d *>(out + (int64_t)blockIdx.y * n_out) + j * A;
#pragma unroll
        for (int h = 0; h < A; h++) o[h] = acc[h];
        if (E::OR == 2 && j + 1 < N) {
#pragma unroll
            for (int h = 0; h < A; h++) o[A + h] = acc[A + h];
        }
    }
}

// k_dnm_col<DnReal<K>, K> on fp32 packs: the same mapping and order behind the widening load (a copy, as k_dnm_row_f32)
template <int K>
__global__ __launch_bounds__(256) void k_dnm_col_f32(const float2 *__restrict__ Kv, int64_t ldp, int M, int N, int NP, int CW, int rps,
                                                     const double *__restrict__ X, double *__restrict__ out, int64_t n_out, const int *done)
{
    using E = DnReal<K>;
    constexpr int A = E::A, UN = E::COL_UN;
    static_assert(E::OR * A == K, "a pack's sums are K pieces");
    __shared__ m2d sh[K][256];
    if (done && *done) return;
    const int RG = 256 / CW;
    const int cp = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int p = blockIdx.x * CW + cp;
    const bool live = p < NP;
    const int r0 = blockIdx.y * rps, r1 = min(M, r0 + rps);
    const m2d *Xv = reinterpret_cast<const m2d *>(X);
    m2d acc[K];
#pragma unroll
    for (int h = 0; h < K; h++) acc[h] = (m2d)(0.0);
    if (live) {
        const float2 *col = Kv + p;
        int i = r0 + rg;
        for (; i + (UN - 1) * RG < r1; i += UN * RG) {
            double2 kk[UN];
            m2d xv[UN][A];
#pragma unroll
            for (int u = 0; u < UN; u++) kk[u] = ldpack(col + (int64_t)(i + u * RG) * ldp);
#pragma unroll
            for (int u = 0; u < UN; u++)
#pragma unroll
                for (int h = 0; h < A; h++) xv[u][h] = Xv[(int64_t)(i + u * RG) * A + h];
#pragma unroll
            for (int u = 0; u < UN; u++) E::col_term(acc, kk[u], xv[u]);
        }
        for (; i < r1; i += RG) {
            const double2 kk = ldpack(col + (int64_t)i * ldp);
            m2d xv[A];
#pragma unroll
            for (int h = 0; h < A; h++) xv[h] = Xv[(int64_t)i * A + h];
            E::col_term(acc, kk, xv);
        }
    }
    if (RG > 1) {       // (uniform over the workgroup)
#pragma unroll
        for (int h = 0; h < A; h++) {
            sh[h][threadIdx.x] = acc[h];
            if (E::OR == 2) sh[A + h][threadIdx.x] = acc[A + h];
        }
        __syncthreads();
        if (rg == 0)
            for (int g = 1; g < RG; g++) {
#pragma unroll
                for (int h = 0; h < A; h++) {
                    acc[h] += sh[h][g * CW + cp];
                    if (E::OR == 2) acc[A + h] += sh[A + h][g * CW + cp];
                }
            }
    }
    if (rg == 0 && live) {
        const int64_t j = E::OR * (int64_t)p;           // the pack's first row of Y
        m2d *o = reinterpret_cast<m2d *>(out + (int64_t)blockIdx.y * n_out) + j * A;
#pragma unroll
        for (int h = 0; h < A; h++) o[h] = acc[h];
        if (E::OR == 2 && j + 1 < N) {
#pragma unroll
            for (int h = 0; h < A; h++) o[A + h] = acc[A + h];
        }
    }
}

// Column j's Y_j . U_j as one partial sum per workgroup and table row at part[row * MM_MG + blockIdx.x]: real, row j; complex (CX), the
// UNCONJUGATED sum's re in row 2 j and im in row 2 j + 1 -- the table formats spmm_launch and cspmm_launch leave.  A workgroup of 64 * G
// threads (G = the 16-byte pieces of a row: K / 2 real, K complex) owns rpb rows (a multiple of 64); its 64 row lanes r = tid / G add
// rows r, r + 64, ... in order, then meet as ONE binary tree over r (bits 0 .. 5 in turn: inside a wavefront by xor, then the G
// wavefronts pairwise) -- the same tree for K = 2, 4, 8, so a column's partials do not depend on K.  The consumer adds them in index
// order (msum).  One launch over the two N x k blocks: no pass over K.
template <int K, bool CX>
__global__ __launch_bounds__(CX ? 64 * K : 32 * K) void k_dnm_dot(const double *__restrict__ Y, const double *__restrict__ U, int n, int rpb,
                                                                  double *__restrict__ part, const int *done)
{
    constexpr int G = CX ? K : K / 2;
    __shared__ double wsh[G][2 * G];
    if (done && *done) return;
    const int c = threadIdx.x % G, r = threadIdx.x / G;
    const int i0 = blockIdx.x * rpb, i1 = min(n, i0 + rpb);
    m2d acc = (m2d)(0.0);
    for (int i = i0 + r; i < i1; i += 64) {
        const m2d y = reinterpret_cast<const m2d *>(Y)[(int64_t)i * G + c], u = reinterpret_cast<const m2d *>(U)[(int64_t)i * G + c];
        if (CX) {
            m2d t;
            t.x = fma(y.x, u.x, fma(-y.y, u.y, acc.x));
            t.y = fma(y.x, u.y, fma(y.y, u.x, acc.y));
            acc = t;
        } else { acc.x = fma(y.x, u.x, acc.x); acc.y = fma(y.y, u.y, acc.y); }
    }
#pragma unroll
    for (int off = G; off <= 32; off <<= 1) { acc.x += __shfl_xor(acc.x, off, 64); acc.y += __shfl_xor(acc.y, off, 64); }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane < G) { wsh[w][2 * lane] = acc.x; wsh[w][2 * lane + 1] = acc.y; }
    __syncthreads();
    if (threadIdx.x < 2 * G) {
        const int q = threadIdx.x;          // the table row
        double v;
        if constexpr (G == 1) v = wsh[0][q];
        else if constexpr (G == 2) v = wsh[0][q] + wsh[1][q];
        else if constexpr (G == 4) v = (wsh[0][q] + wsh[1][q]) + (wsh[2][q] + wsh[3][q]);
        else v = ((wsh[0][q] + wsh[1][q]) + (wsh[2][q] + wsh[3][q])) + ((wsh[4][q] + wsh[5][q]) + (wsh[6][q] + wsh[7][q]));
        part[(size_t)q * MM_MG + blockIdx.x] = v;
    }
}

// ---- work memory -------------------------------------------------------------------------------------------------------------------
// doubles of the slot table per column of the block: the split row form under either plan, the column form (complex handles: twice
// that, and no M x k block -- there is no complex normal-equations operator)
static int64_t dnm_table_doubles(int M, int N, int NP)
{
    int64_t need = 0;
    for (int forced = 0; forced < 2; forced++) need = std::max(need, (int64_t)row_plan(M, NP, true, forced).S * M);
    return std::max(need, (int64_t)col_plan(M, NP).RS * N);
}

// The first call at a k larger than any before allocates (and waits for the work that may still use the smaller arrays); later calls
// only launch.
int dnm_reserve(lcg_hip_dense *K, int k)
{
    if (!K->multi) K->multi = new DenseMulti;
    DenseMulti *w = K->multi;
    if (k <= w->kmax) return 0;
    if (w->kmax) HIPCHK(hipStreamSynchronize(ctx().stream));
    if (w->t) (void)hipFree(w->t);
    if (w->part) (void)hipFree(w->part);
    w->t = w->part = nullptr; w->kmax = 0;
    if (!K->cplx) HIPCHK(hipMalloc(&w->t, sizeof(double) * (size_t)K->M * k));
    HIPCHK(hipMalloc(&w->part, sizeof(double) * (size_t)dnm_table_doubles(K->M, K->N, K->NP) * k * dn_words(K) + 16));
    w->kmax = k;
    return 0;
}

void dnm_release(lcg_hip_dense *K)
{
    DenseMulti *w = K->multi;
    if (!w) return;
    if (w->t) (void)hipFree(w->t);
    if (w->part) (void)hipFree(w->part);
    delete w;
    K->multi = nullptr;
}

// ---- launches ----------------------------------------------------------------------------------------------------------------------
// Real and complex handles share every function below: they branch on D->cplx the way dense.hip's single-vector ones do, and the complex
// factor 2 of the slot sizes is dn_words(D).
void dnm_fold_launch(const double *part, int S, int64_t n, double *y, hipStream_t s, const int *done)
{
    hipLaunchKernelGGL(k_dnm_fold, dim3((unsigned)cdiv(n, MFOLD_J)), dim3(MFOLD_Q * MFOLD_J), 0, s, part, S, n, y, done);
}

template <int K>
static void row_dispatch(const lcg_hip_dense *D, const RowPlan &r, const double *X, double *out, hipStream_t s, const int *done)
{
    const dim3 grid((unsigned)cdiv(cdiv(D->M, K / 2), 256 / r.W), (unsigned)r.S);        // a group of W lanes owns K / 2 rows
#define DNM_ROW_CASE(w) case w: hipLaunchKernelGGL((k_dnm_row<K, w>), grid, dim3(256), 0, s, D->val, D->ldp, D->M, D->N, D->NP, r.pps, X, out, done); break;
    switch (r.W) { DNM_ROW_CASE(4) DNM_ROW_CASE(8) DNM_ROW_CASE(16) DNM_ROW_CASE(32) default: DNM_ROW_CASE(64) }
#undef DNM_ROW_CASE
}
template <int K>
static void row_dispatch_f32(const lcg_hip_dense *D, const RowPlan &r, const double *X, double *out, hipStream_t s, const int *done)
{
    const dim3 grid((unsigned)cdiv(cdiv(D->M, K / 2), 256 / r.W), (unsigned)r.S);
#define DNM_ROW_CASE(w) case w: hipLaunchKernelGGL((k_dnm_row_f32<K, w>), grid, dim3(256), 0, s, dn_val32(D), D->ldp, D->M, D->N, D->NP, r.pps, X, out, done); break;
    switch (r.W) { DNM_ROW_CASE(4) DNM_ROW_CASE(8) DNM_ROW_CASE(16) DNM_ROW_CASE(32) default: DNM_ROW_CASE(64) }
#undef DNM_ROW_CASE
}
template <int K, bool CONJ>
static void zrow_dispatch(const lcg_hip_dense *D, const RowPlan &r, const double *X, double *out, hipStream_t s, const int *done)
{
    const dim3 grid((unsigned)cdiv(cdiv(D->M, zrr(K)), 256 / r.W), (unsigned)r.S);         // a group of W lanes owns zrr(K) rows
#define ZDNM_ROW_CASE(w) case w: hipLaunchKernelGGL((k_zdnm_row<K, w, CONJ>), grid, dim3(256), 0, s, D->val, D->ldp, D->M, D->NP, r.pps, X, out, done); break;
    switch (r.W) { ZDNM_ROW_CASE(4) ZDNM_ROW_CASE(8) ZDNM_ROW_CASE(16) ZDNM_ROW_CASE(32) default: ZDNM_ROW_CASE(64) }
#undef ZDNM_ROW_CASE
}

// Y[M x k] = K.X (complex: or conj(K).X); variant: DN_ROW / DN_ROW_SPLIT force a form, anything else is the automatic choice.  *launches
// grows by what ran
int dnm_row_product(lcg_hip_dense *D, int k, const double *X, double *Y, int conjugate, int variant, hipStream_t s, const int *done,
                    int *launches)
{
    const bool forced = variant == DN_ROW_SPLIT;
    const bool split = forced || (variant != DN_ROW && row_split_auto(D->M, D->NP));
    const RowPlan r = row_plan(D->M, D->NP, split, forced);
    double *out = r.S > 1 ? D->multi->part : Y;
    multi_k(k, [&](auto K) {
        constexpr int KK = decltype(K)::value;
        if (D->f32) row_dispatch_f32<KK>(D, r, X, out, s, done);
        else if (!D->cplx) row_dispatch<KK>(D, r, X, out, s, done);
        else if (conjugate) zrow_dispatch<KK, true>(D, r, X, out, s, done);
        else zrow_dispatch<KK, false>(D, r, X, out, s, done);
        return 0;
    });
    if (r.S > 1) dnm_fold_launch(D->multi->part, r.S, (int64_t)D->M * k * dn_words(D), Y, s, done);
    *launches += r.S > 1 ? 2 : 1;
    D->multi->last_kernel = (D->cplx ? ZDNM_NAMES : DNM_NAMES)[r.S > 1 ? 1 : 0];
    return launched(D->cplx ? "complex dense k-wide row product" : "dense k-wide row product");
}

// Y[N x k] = K^T.X (complex: or K^H.X)
int dnm_col_product(lcg_hip_dense *D, int k, const double *X, double *Y, int conjugate, hipStream_t s, const int *done, int *launches)
{
    const ColPlan c = col_plan(D->M, D->NP);
    const int64_t n_out = (int64_t)D->N * k * dn_words(D);
    double *out = c.RS > 1 ? D->multi->part : Y;
    const dim3 grid((unsigned)c.CT, (unsigned)c.RS);
#define DNM_COL(...) hipLaunchKernelGGL((k_dnm_col<__VA_ARGS__, KK>), grid, dim3(256), 0, s, D->val, D->ldp, D->M, D->N, D->NP, c.CW, c.rps, X, out, n_out, done)
    multi_k(k, [&](auto K) {
        constexpr int KK = decltype(K)::value;
        if (D->f32) hipLaunchKernelGGL((k_dnm_col_f32<KK>), grid, dim3(256), 0, s, dn_val32(D), D->ldp, D->M, D->N, D->NP, c.CW, c.rps, X, out, n_out, done);
        else if (!D->cplx) DNM_COL(DnReal<KK>);
        else if (conjugate) DNM_COL(DnCplx<KK, true>);
        else DNM_COL(DnCplx<KK, false>);
        return 0;
    });
#undef DNM_COL
    if (c.RS > 1) dnm_fold_launch(D->multi->part, c.RS, n_out, Y, s, done);
    *launches += c.RS > 1 ? 2 : 1;
    D->multi->last_kernel = (D->cplx ? ZDNM_NAMES : DNM_NAMES)[2];
    return launched(D->cplx ? "complex dense k-wide column product" : "dense k-wide column product");
}

// Y[N x k] = K^T.(K.X): the row form into the handle's M x k block, then the column form (the forced row variants reach the first stage)
static int ata_product(lcg_hip_dense *D, int k, const double *X, double *Y, hipStream_t s, const int *done, int *launches)
{
    const int v = D->variant;
    int rc = dnm_row_product(D, k, X, D->multi->t, 0, v == DN_ROW || v == DN_ROW_SPLIT ? v : DN_AUTO, s, done, launches);
    if (!rc) rc = dnm_col_product(D, k, D->multi->t, Y, 0, s, done, launches);
    D->multi->last_kernel = DNM_NAMES[3];
    return rc;
}

// column j's Y_j . U_j over n rows as *slots partial sums per table row; a workgroup of k_dnm_dot owns a multiple of 64 rows that leaves
// at most MM_MG workgroups
static int dot_launch(bool cplx, int k, int n, const double *Y, const double *U, double *dots, int *slots, hipStream_t s, const int *done)
{
    const int rpb = 64 * (int)cdiv(cdiv(n, 64), MM_MG), nb = (int)cdiv(n, rpb);
    multi_k(k, [&](auto K) {
        constexpr int KK = decltype(K)::value;
        if (cplx) hipLaunchKernelGGL((k_dnm_dot<KK, true>), dim3(nb), dim3(64 * KK), 0, s, Y, U, n, rpb, dots, done);
        else hipLaunchKernelGGL((k_dnm_dot<KK, false>), dim3(nb), dim3(32 * KK), 0, s, Y, U, n, rpb, dots, done);
        return 0;
    });
    *slots = nb;
    return launched(cplx ? "complex dense k-wide dot" : "dense k-wide dot");
}

// The operator of the batched loops: Y = (normal ? K^T.K : K).X and, with U, column j's Y_j . U_j (complex: unconjugated) as *slots
// partial sums per table row of dots (k_dnm_dot).  The handle has been checked and its work memory reserved for k; a complex handle
// never comes with normal = 1.
int dnm_op(lcg_hip_dense *D, int k, int normal, const double *X, double *Y, hipStream_t s, const int *done, const double *U, double *dots,
           int *slots, int *launches)
{
    int rc = normal ? ata_product(D, k, X, Y, s, done, launches) : dnm_row_product(D, k, X, Y, 0, D->variant, s, done, launches);
    if (rc || !U) return rc;
    (*launches)++;
    return dot_launch(D->cplx, k, D->N, Y, U, dots, slots, s, done);
}

// a dense handle of the kind the entry serves, or nullptr with the entry's name and the reason in lcg_hip_last_error()
lcg_hip_dense *dnm_handle(const char *entry, const void *h, bool cplx)
{
    if (!dense_handle(h)) { arg_error("%s: the handle is not a dense matrix (lcg_hip_dense_create)", entry); return nullptr; }
    lcg_hip_dense *D = static_cast<lcg_hip_dense *>(const_cast<void *>(h));
    if (D->c64) { refuse_c64_dense(entry); return nullptr; }
    if (D->cplx == cplx) return D;
    if (cplx) arg_error("%s: the matrix is real; the complex k-wide dense path serves complex128 matrices (real: lcg_hip_dense_matmat)", entry);
    else arg_error("%s: the matrix is complex; the k-wide dense path serves real fp64 matrices", entry);
    return nullptr;
}

// what lcg_hip_dense_op_multi_dot and its complex twin do after their checks
int dnm_op_dot_run(lcg_hip_dense *D, int k, int normal, const double *X, double *Y, const double *U, double *dots)
{
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    Ctx &c = ctx();
    // (outside a solve the k-wide table of the loops is free: partials_pair[0] holds the partial sums, ax_partials the results)
    int slots = 0, launches = 0;
    TRY(dnm_op(D, k, normal, X, Y, c.stream, nullptr, U, c.partials_pair[0], &slots, &launches));
    return U && dots ? multi_dots_read(c, k * dn_words(D), slots, dots) : 0;
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_dense_matmat(lcg_hip_dense_t K, int k, const double *X, double *Y, int layout)
{
    const char *entry = "lcg_hip_dense_matmat";
    TRY(multi_args(entry, k, X, Y));
    lcg_hip_dense *D = dnm_handle(entry, K);
    if (!D) return LCG_HIP_E_ARG;
    if (layout < 0 || layout > 1) return arg_error("%s: layout = %d (0: K.X, 1: K^T.X)", entry, layout);
    const size_t nx = (size_t)(layout ? D->M : D->N) * k, ny = (size_t)(layout ? D->N : D->M) * k;
    if (overlap(X, 8 * nx, Y, 8 * ny)) return arg_error("%s: X and Y overlap", entry);
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    int launches = 0;
    return layout ? dnm_col_product(D, k, X, Y, 0, ctx().stream, nullptr, &launches)
                  : dnm_row_product(D, k, X, Y, 0, D->variant, ctx().stream, nullptr, &launches);
}

int lcg_hip_dense_ata_multi(lcg_hip_dense_t K, int k, const double *X, double *Y)
{
    const char *entry = "lcg_hip_dense_ata_multi";
    TRY(multi_args(entry, k, X, Y));
    lcg_hip_dense *D = dnm_handle(entry, K);
    if (!D) return LCG_HIP_E_ARG;
    if (overlap(X, 8 * (size_t)D->N * k, Y, 8 * (size_t)D->N * k)) return arg_error("%s: X and Y overlap", entry);
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    int launches = 0;
    return ata_product(D, k, X, Y, ctx().stream, nullptr, &launches);
}

int lcg_hip_dense_op_multi_dot(lcg_hip_dense_t K, int k, int normal, const double *X, double *Y, const double *U, double *dots)
{
    const char *entry = "lcg_hip_dense_op_multi_dot";
    TRY(multi_args(entry, k, X, Y, U ? (const void *)U : (const void *)16));
    lcg_hip_dense *D = dnm_handle(entry, K);
    if (!D) return LCG_HIP_E_ARG;
    if (normal != 0 && normal != 1) return arg_error("%s: normal = %d (1: K^T.K, 0: K)", entry, normal);
    if (!normal && D->M != D->N) return arg_error("%s: the matrix is %d x %d: normal = 0 needs a square one", entry, D->M, D->N);
    const size_t nv = 8 * (size_t)D->N * k;
    if (overlap(X, nv, Y, nv) || (U && overlap(U, nv, Y, nv))) return arg_error("%s: Y overlaps X or U", entry);
    if (dots && !U) return arg_error("%s: dots without U", entry);
    return dnm_op_dot_run(D, k, normal, X, Y, U, dots);
}

const char *lcg_hip_dense_multi_last_kernel(lcg_hip_dense_t K)
{
    if (!dense_handle(K)) { arg_error("lcg_hip_dense_multi_last_kernel: the handle is not a dense matrix (lcg_hip_dense_create)"); return ""; }
    return K->multi ? K->multi->last_kernel : "";
}

const char *lcg_hip_dense_multi_kernel_name(int index) { return dnm_kernel_name(false, index); }

} // extern "C"
