// dense_multi_cplx.hip -- complex128 dense operators over k = 2, 4, 8 right-hand sides: K.X, conj(K).X, K^T.X, K^H.X with K read ONCE
// for all k columns, and the operator of the batched complex loops (solvers_multi_cplx.hip: clcg_hip_dense_lbicg_sym_multi,
// clcg_hip_dense_lpcg_multi) with the unconjugated sum they take after it.  One GPU.  DESIGN.md section 20.
//
// Blocks of vectors are multi_cplx.hpp's: column j of row i is the 16-byte piece i * k + j, the base 16-byte aligned.  The kernels are
// the k-wide twins of dense.hip's complex forms, on the same storage (one 16-byte pack per entry, NP = N, the single stored copy) and
// under the SAME plans (dense.hpp: functions of the shape and the forced variant, never of k):
//
//   k_zdnm_row<K, W, CONJ>  Y(i,:) = sum_j op(K(i,j)) X(j,:)   W lanes per group of zrr(K) = 4 rows; per pack a lane loads one entry of K per row
//                           and row j of X (16 k contiguous bytes) once for its rows; k complex accumulators per row; butterfly
//                           over the W lanes; whole rows of Y.  Columns cut into strips over gridDim.y (k_zdnm_row_split): one slot
//                           of M * 2k doubles per strip
//   k_zdnm_col<K, CONJ>     Y(j,:) = sum_i op(K(i,j)) X(i,:)   thread (cp, rg) owns one column and walks a strip of rows, reading the k
//                           complex values X(i,:) per row (one address for all lanes of a row group); k accumulators; the row groups
//                           meet in LDS in rg order; one slot of N * 2k doubles per strip of rows
//   k_dnm_fold              (dense_multi.hip) the slots added in its fixed order -- it adds doubles and does not care what they are
//   k_zdnm_dot<K>           column j's unconjugated sum_i Y_ij U_ij left as <= MM_MG partial sums per component in the table format
//                           cspmm_launch leaves (re: row 2 j, im: row 2 j + 1), one launch over the two N x k blocks: no pass over K
//
// Every complex multiply-add is zfma's pair of explicit fmas per component (the conjugated forms flip signs and nothing else) and every
// sum is added in an order fixed by the shape alone, so column j's bits depend on K, the handle's forced variant and column j of X (and
// U) -- not on k, not on what the other columns hold, not on the call.  No atomics.  Every kernel falls through when the batch has
// stopped (`done`).
#include <cstdarg>

#include "dense.hpp"
#include "multi_loop.hpp"
#include "multi_cplx.hpp"

namespace lcgh {

static const char *const ZDNM_NAMES[] = {"k_zdnm_row", "k_zdnm_row_split", "k_zdnm_col"};

static int zdnm_error(const char *fmt, ...)
{
    char buf[400];
    va_list ap; va_start(ap, fmt); std::vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    ctx().err = buf;
    return LCG_HIP_E_ARG;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// Rows a group of the row form owns, a function of K alone: four at every K.  A lane loads 16 k bytes of X per pack whatever the rows
// are, W rows of X a wavefront instruction, and the vector cache takes them a 128-byte line at a time: 8 k^2 lines per 64 packs (16,
// 32 and 64 lines per 16-byte load at k = 2, 4, 8), against 16 cycles for a coalesced load of K.  The rows share that cost.  At k = 8
// four rows are 32 complex accumulators = 128 VGPRs and the kernel compiles to 256 VGPRs plus 12 .. 16 AGPR copies, ONE wavefront per
// SIMD; two rows compile to 166 VGPRs and three wavefronts.  Both were measured: 8192^2 and 16384^2 at k = 8 run at 58 %
// and 64 % of the read rate with four rows, 34 % with two -- the lines decide, not the occupancy.
constexpr int zrr(int) { return 4; }

namespace {

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

template <int K>
__device__ __forceinline__ void zx_load(m2d *x, const m2d *Xv, int64_t row)
{
#pragma unroll
    for (int h = 0; h < K; h++) x[h] = Xv[row * K + h];
}

} // namespace

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

// Column form (k_dn_col's mapping, one column per pack).  A workgroup owns CW columns (blockIdx.x) and the rows [r0, r0 + rps)
// (blockIdx.y); thread (cp, rg) walks the rows r0 + rg, r0 + rg + RG, ... of column cp.  The RG sums of a column are added in rg order,
// then written as row p of slot blockIdx.y of out (n_out = N * 2K doubles per slot; gridDim.y == 1: out = Y).
template <int K, bool CONJ>
__global__ __launch_bounds__(256) void k_zdnm_col(const double2 *__restrict__ Kv, int64_t ldp, int M, int NP, int CW, int rps,
                                                  const double *__restrict__ X, double *__restrict__ out, int64_t n_out, const int *done)
{
    constexpr int UN = 16 / K;
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
            m2d xv[UN][K];
#pragma unroll
            for (int u = 0; u < UN; u++) kk[u] = col[(int64_t)(i + u * RG) * ldp];
#pragma unroll
            for (int u = 0; u < UN; u++) zx_load<K>(xv[u], Xv, i + u * RG);
#pragma unroll
            for (int u = 0; u < UN; u++) zfma_row<K, CONJ>(acc, kk[u], xv[u]);
        }
        for (; i < r1; i += RG) {
            m2d xv[K];
            zx_load<K>(xv, Xv, i);
            zfma_row<K, CONJ>(acc, col[(int64_t)i * ldp], xv);
        }
    }
    if (RG > 1) {       // (uniform over the workgroup)
#pragma unroll
        for (int h = 0; h < K; h++) sh[h][threadIdx.x] = acc[h];
        __syncthreads();
        if (rg == 0)
            for (int g = 1; g < RG; g++) {
#pragma unroll
                for (int h = 0; h < K; h++) acc[h] += sh[h][g * CW + cp];
            }
    }
    if (rg == 0 && live) {
        m2d *o = reinterpret_cast<m2d *>(out + (int64_t)blockIdx.y * n_out) + (int64_t)p * K;
#pragma unroll
        for (int h = 0; h < K; h++) o[h] = acc[h];
    }
}

// Column j's unconjugated sum_i Y_ij U_ij as one partial sum per workgroup and component: re at part[(2 j) * MM_MG + blockIdx.x], im at
// part[(2 j + 1) * MM_MG + blockIdx.x].  A workgroup of 64 * K threads owns rpb rows (a multiple of 64); its 64 row lanes r = tid / K
// add rows r, r + 64, ... in order, then meet as ONE binary tree over r (bits 0 .. 5 in turn: inside a wavefront by xor, then the K
// wavefronts pairwise) -- the same tree for K = 2, 4, 8 (k_dnm_dot's), so a column's partials do not depend on K.  The consumer adds
// them in index order (msum).
template <int K>
__global__ __launch_bounds__(64 * K) void k_zdnm_dot(const double *__restrict__ Y, const double *__restrict__ U, int n, int rpb,
                                                     double *__restrict__ part, const int *done)
{
    __shared__ double wsh[K][2 * K];
    if (done && *done) return;
    const int c = threadIdx.x % K, r = threadIdx.x / K;
    const int i0 = blockIdx.x * rpb, i1 = min(n, i0 + rpb);
    m2d acc = (m2d)(0.0);
    for (int i = i0 + r; i < i1; i += 64) {
        const m2d y = reinterpret_cast<const m2d *>(Y)[(int64_t)i * K + c], u = reinterpret_cast<const m2d *>(U)[(int64_t)i * K + c];
        m2d t;
        t.x = fma(y.x, u.x, fma(-y.y, u.y, acc.x));
        t.y = fma(y.x, u.y, fma(y.y, u.x, acc.y));
        acc = t;
    }
#pragma unroll
    for (int off = K; off <= 32; off <<= 1) { acc.x += __shfl_xor(acc.x, off, 64); acc.y += __shfl_xor(acc.y, off, 64); }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane < K) { wsh[w][2 * lane] = acc.x; wsh[w][2 * lane + 1] = acc.y; }
    __syncthreads();
    if (threadIdx.x < 2 * K) {
        const int q = threadIdx.x;          // 2 j + component
        double v;
        if constexpr (K == 2) v = wsh[0][q] + wsh[1][q];
        else if constexpr (K == 4) v = (wsh[0][q] + wsh[1][q]) + (wsh[2][q] + wsh[3][q]);
        else v = ((wsh[0][q] + wsh[1][q]) + (wsh[2][q] + wsh[3][q])) + ((wsh[4][q] + wsh[5][q]) + (wsh[6][q] + wsh[7][q]));
        part[(size_t)q * MM_MG + blockIdx.x] = v;
    }
}

// the k complex results of clcg_hip_dense_op_multi_dot out of their partial sums (NS = 2k table rows)
template <int NS>
__global__ __launch_bounds__(VB) void k_zdnm_dots(const double *dots, int slots, double *out)
{
    __shared__ double sums[NS];
    msum<NS>(dots, slots, sums);
    if (threadIdx.x < NS) out[threadIdx.x] = sums[threadIdx.x];
}

// ---- launches ----------------------------------------------------------------------------------------------------------------------
static int launched(const char *what)
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(e, what, __FILE__, __LINE__);
}

template <int K, bool CONJ>
static void zrow_dispatch(const lcg_hip_dense *D, const RowPlan &r, const double *X, double *out, hipStream_t s, const int *done)
{
    const dim3 grid((unsigned)cdiv(cdiv(D->M, zrr(K)), 256 / r.W), (unsigned)r.S);         // a group of W lanes owns zrr(K) rows
#define ZDNM_ROW_CASE(w) case w: hipLaunchKernelGGL((k_zdnm_row<K, w, CONJ>), grid, dim3(256), 0, s, D->val, D->ldp, D->M, D->NP, r.pps, X, out, done); break;
    switch (r.W) { ZDNM_ROW_CASE(4) ZDNM_ROW_CASE(8) ZDNM_ROW_CASE(16) ZDNM_ROW_CASE(32) default: ZDNM_ROW_CASE(64) }
#undef ZDNM_ROW_CASE
}

// Y[M x k] = K.X or conj(K).X; variant: DN_ROW / DN_ROW_SPLIT force a form, anything else is the automatic choice.  *launches grows by
// what ran
static int zrow_product(lcg_hip_dense *D, int k, const double *X, double *Y, int conjugate, int variant, hipStream_t s, const int *done,
                        int *launches)
{
    const bool forced = variant == DN_ROW_SPLIT;
    const bool split = forced || (variant != DN_ROW && row_split_auto(D->M, D->NP));
    const RowPlan r = row_plan(D->M, D->NP, split, forced);
    double *out = r.S > 1 ? D->multi->part : Y;
    multi_k(k, [&](auto K) {
        if (conjugate) zrow_dispatch<decltype(K)::value, true>(D, r, X, out, s, done);
        else zrow_dispatch<decltype(K)::value, false>(D, r, X, out, s, done);
        return 0;
    });
    if (r.S > 1) dnm_fold_launch(D->multi->part, r.S, (int64_t)D->M * 2 * k, Y, s, done);
    *launches += r.S > 1 ? 2 : 1;
    D->multi->last_kernel = r.S > 1 ? ZDNM_NAMES[1] : ZDNM_NAMES[0];
    return launched("complex dense k-wide row product");
}

// Y[N x k] = K^T.X or K^H.X
static int zcol_product(lcg_hip_dense *D, int k, const double *X, double *Y, int conjugate, hipStream_t s, const int *done, int *launches)
{
    const ColPlan c = col_plan(D->M, D->NP);
    const int64_t n_out = (int64_t)D->N * 2 * k;
    double *out = c.RS > 1 ? D->multi->part : Y;
    const dim3 grid((unsigned)c.CT, (unsigned)c.RS);
    multi_k(k, [&](auto K) {
        constexpr int KK = decltype(K)::value;
        if (conjugate) hipLaunchKernelGGL((k_zdnm_col<KK, true>), grid, dim3(256), 0, s, D->val, D->ldp, D->M, D->NP, c.CW, c.rps, X, out, n_out, done);
        else hipLaunchKernelGGL((k_zdnm_col<KK, false>), grid, dim3(256), 0, s, D->val, D->ldp, D->M, D->NP, c.CW, c.rps, X, out, n_out, done);
        return 0;
    });
    if (c.RS > 1) dnm_fold_launch(D->multi->part, c.RS, n_out, Y, s, done);
    *launches += c.RS > 1 ? 2 : 1;
    D->multi->last_kernel = ZDNM_NAMES[2];
    return launched("complex dense k-wide column product");
}

// rows a workgroup of k_zdnm_dot owns: a multiple of 64 that leaves at most MM_MG workgroups
static int zdot_rows_per_block(int n) { return 64 * (int)cdiv(cdiv(n, 64), MM_MG); }

static int zdot_launch(int k, int n, const double *Y, const double *U, double *dots, int *slots, hipStream_t s, const int *done)
{
    const int rpb = zdot_rows_per_block(n), nb = (int)cdiv(n, rpb);
    multi_k(k, [&](auto K) {
        constexpr int KK = decltype(K)::value;
        hipLaunchKernelGGL((k_zdnm_dot<KK>), dim3(nb), dim3(64 * KK), 0, s, Y, U, n, rpb, dots, done);
        return 0;
    });
    *slots = nb;
    return launched("complex dense k-wide dot");
}

int zdnm_op(lcg_hip_dense *D, int k, const double *X, double *Y, hipStream_t s, const int *done, const double *U, double *dots, int *slots,
            int *launches)
{
    const int rc = zrow_product(D, k, X, Y, 0, D->variant, s, done, launches);
    if (rc || !U) return rc;
    (*launches)++;
    return zdot_launch(k, D->N, Y, U, dots, slots, s, done);
}

lcg_hip_dense *zdnm_handle(const char *entry, const void *h)
{
    if (!dense_handle(h)) { zdnm_error("%s: the handle is not a dense matrix (lcg_hip_dense_create)", entry); return nullptr; }
    lcg_hip_dense *D = static_cast<lcg_hip_dense *>(const_cast<void *>(h));
    if (!D->cplx) { zdnm_error("%s: the matrix is real; the complex k-wide dense path serves complex128 matrices (real: lcg_hip_dense_matmat)", entry); return nullptr; }
    return D;
}

// n complex values each
static bool zoverlap(const double *a, size_t na, const double *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 16 * na, b0 = (uintptr_t)b, b1 = b0 + 16 * nb;
    return a0 < b1 && b0 < a1;
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int clcg_hip_dense_matmat(lcg_hip_dense_t K, int k, const double *X, double *Y, int layout, int conjugate)
{
    const char *entry = "clcg_hip_dense_matmat";
    TRY(multi_args(entry, k, X, Y));
    lcg_hip_dense *D = zdnm_handle(entry, K);
    if (!D) return LCG_HIP_E_ARG;
    if (layout < 0 || layout > 1 || conjugate < 0 || conjugate > 1)
        return zdnm_error("%s: layout = %d, conjugate = %d (layout 0: K.X, 1: K^T.X; conjugate 0 / 1)", entry, layout, conjugate);
    const size_t nx = (size_t)(layout ? D->M : D->N) * k, ny = (size_t)(layout ? D->N : D->M) * k;
    if (zoverlap(X, nx, Y, ny)) return zdnm_error("%s: X and Y overlap", entry);
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    int launches = 0;
    return layout ? zcol_product(D, k, X, Y, conjugate, ctx().stream, nullptr, &launches)
                  : zrow_product(D, k, X, Y, conjugate, D->variant, ctx().stream, nullptr, &launches);
}

int clcg_hip_dense_op_multi_dot(lcg_hip_dense_t K, int k, const double *X, double *Y, const double *U, double *dots)
{
    const char *entry = "clcg_hip_dense_op_multi_dot";
    TRY(multi_args(entry, k, X, Y, U ? (const void *)U : (const void *)16));
    lcg_hip_dense *D = zdnm_handle(entry, K);
    if (!D) return LCG_HIP_E_ARG;
    if (D->M != D->N) return zdnm_error("%s: the matrix is %d x %d: the loops' operator needs a square one", entry, D->M, D->N);
    const size_t nv = (size_t)D->N * k;
    if (zoverlap(X, nv, Y, nv) || (U && zoverlap(U, nv, Y, nv))) return zdnm_error("%s: Y overlaps X or U", entry);
    if (dots && !U) return zdnm_error("%s: dots without U", entry);
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    Ctx &c = ctx();
    // (outside a solve the k-wide table of the loops is free: partials_pair[0] holds the partial sums, ax_partials the results)
    int slots = 0, launches = 0;
    TRY(zdnm_op(D, k, X, Y, c.stream, nullptr, U, c.partials_pair[0], &slots, &launches));
    if (!U || !dots) return 0;
    const int ns = 2 * k;
    if (ns == 4) hipLaunchKernelGGL((k_zdnm_dots<4>), dim3(1), dim3(VB), 0, c.stream, c.partials_pair[0], slots, c.ax_partials);
    else if (ns == 8) hipLaunchKernelGGL((k_zdnm_dots<8>), dim3(1), dim3(VB), 0, c.stream, c.partials_pair[0], slots, c.ax_partials);
    else hipLaunchKernelGGL((k_zdnm_dots<16>), dim3(1), dim3(VB), 0, c.stream, c.partials_pair[0], slots, c.ax_partials);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c.scratch_host, c.ax_partials, sizeof(double) * ns, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    for (int j = 0; j < ns; j++) dots[j] = c.scratch_host[j];
    return 0;
}

const char *clcg_hip_dense_multi_kernel_name(int index)
{
    return index >= 0 && index < (int)(sizeof ZDNM_NAMES / sizeof *ZDNM_NAMES) ? ZDNM_NAMES[index] : nullptr;
}

} // extern "C"
