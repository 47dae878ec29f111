// dense_multi.hip -- dense operators over k = 2, 4, 8 right-hand sides: K.X, K^T.X, K^T.(K.X) with K read ONCE for all k columns,
// and the operator of the batched loops (solvers_multi.hip: lcg_hip_dense_lcg_multi, lcg_hip_dense_lpcg_multi) with the sum they
// take after it.  Real fp64 handles, one GPU.  DESIGN.md section 19.
//
// Blocks of vectors are multi.hpp's: X[i * k + j] is row i of column j, the base 16-byte aligned.  The kernels are the k-wide twins
// of dense.hip's, on the same storage (rows of 16-byte packs, pads zero) and under the SAME plans (dense.hpp: functions of the
// shape and the forced variant, never of k):
//
//   k_dnm_row<K, W>   Y(i,:) = sum_j K(i,j) X(j,:)   W lanes per group of k / 2 rows; a lane loads one pack of K per row and access and,
//                     for the pack's two columns, rows 2p and 2p + 1 of X (2k contiguous doubles) once for its rows; K accumulators
//                     per row; butterfly over the W lanes; whole rows of Y.  Columns cut into strips over gridDim.y
//                     (k_dnm_row_split): one slot of M * k values per strip
//   k_dnm_col<K>      Y(j,:) = sum_i K(i,j) X(i,:)   thread (cp, rg) owns one pack of columns and walks a strip of rows, reading the
//                     k values X(i,:) per row (one address for all lanes of a row group); 2k accumulators; the row groups meet in
//                     LDS in rg order; one slot of N * k values per strip of rows
//   k_dnm_fold        the slots added in k_dn_fold's fixed order
//   k_dnm_dot<K>      column j's Y_j . U_j left as <= MM_MG partial sums in the table format spmm_launch leaves (multi.hpp), one
//                     launch over the two N x k blocks: no pass over K
//
// Every multiply-add is an explicit fma and every sum is added in an order fixed by the shape alone, so column j's bits depend on
// K, the handle's forced variant and column j of X (and U) -- not on k, not on what the other columns hold, not on the call.  No
// atomics.  Every kernel falls through when the batch has stopped (`done`).
#include <cstdarg>

#include "dense.hpp"
#include "multi.hpp"

namespace lcgh {

static const char *const DNM_NAMES[] = {"k_dnm_row", "k_dnm_row_split", "k_dnm_col", "k_dnm_ata_two_pass"};

static int dnm_error(const char *fmt, ...)
{
    char buf[400];
    va_list ap; va_start(ap, fmt); std::vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    ctx().err = buf;
    return LCG_HIP_E_ARG;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// acc(:) += a * x(:), one rounding per column and term
template <int K2>
__device__ __forceinline__ void fma_row(m2d *acc, double a, const m2d *x)
{
#pragma unroll
    for (int h = 0; h < K2; h++) { acc[h].x = fma(a, x[h].x, acc[h].x); acc[h].y = fma(a, x[h].y, acc[h].y); }
}

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

// y[j] = the sum of the table's S slots of n doubles each, in k_dn_fold's order: FOLD_Q runs of consecutive slots, thread (q, j) adds
// run q's slots in index order, the runs' sums are added in run order.
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
// (cp, rg) walks the rows r0 + rg, r0 + rg + RG, ... of pack cp.  The RG sums of a pack are added in rg order, then written as rows
// 2p and 2p + 1 of slot blockIdx.y of out (n_out = N * K doubles per slot; gridDim.y == 1: out = Y).
template <int K>
__global__ __launch_bounds__(256) void k_dnm_col(const double2 *__restrict__ Kv, int64_t ldp, int M, int N, int NP, int CW, int rps,
                                                 const double *__restrict__ X, double *__restrict__ out, int64_t n_out, const int *done)
{
    constexpr int K2 = K / 2;
    constexpr int UN = K == 8 ? 4 : 8;
    __shared__ m2d sh[K][256];
    if (done && *done) return;
    const int RG = 256 / CW;
    const int cp = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int p = blockIdx.x * CW + cp;
    const bool live = p < NP;
    const int r0 = blockIdx.y * rps, r1 = min(M, r0 + rps);
    const m2d *Xv = reinterpret_cast<const m2d *>(X);
    m2d a0[K2], a1[K2];
#pragma unroll
    for (int h = 0; h < K2; h++) { a0[h] = (m2d)(0.0); a1[h] = (m2d)(0.0); }
    if (live) {
        const double2 *col = Kv + p;
        int i = r0 + rg;
        for (; i + (UN - 1) * RG < r1; i += UN * RG) {
            double2 kk[UN];
            m2d xv[UN][K2];
#pragma unroll
            for (int u = 0; u < UN; u++) kk[u] = col[(int64_t)(i + u * RG) * ldp];
#pragma unroll
            for (int u = 0; u < UN; u++)
#pragma unroll
                for (int h = 0; h < K2; h++) xv[u][h] = Xv[(int64_t)(i + u * RG) * K2 + h];
#pragma unroll
            for (int u = 0; u < UN; u++) { fma_row<K2>(a0, kk[u].x, xv[u]); fma_row<K2>(a1, kk[u].y, xv[u]); }
        }
        for (; i < r1; i += RG) {
            const double2 kk = col[(int64_t)i * ldp];
            m2d xv[K2];
#pragma unroll
            for (int h = 0; h < K2; h++) xv[h] = Xv[(int64_t)i * K2 + h];
            fma_row<K2>(a0, kk.x, xv); fma_row<K2>(a1, kk.y, xv);
        }
    }
    if (RG > 1) {       // (uniform over the workgroup)
#pragma unroll
        for (int h = 0; h < K2; h++) { sh[h][threadIdx.x] = a0[h]; sh[K2 + h][threadIdx.x] = a1[h]; }
        __syncthreads();
        if (rg == 0)
            for (int g = 1; g < RG; g++) {
#pragma unroll
                for (int h = 0; h < K2; h++) { a0[h] += sh[h][g * CW + cp]; a1[h] += sh[K2 + h][g * CW + cp]; }
            }
    }
    if (rg == 0 && live) {
        const int64_t j = 2 * (int64_t)p;
        m2d *o = reinterpret_cast<m2d *>(out + (int64_t)blockIdx.y * n_out) + j * K2;
#pragma unroll
        for (int h = 0; h < K2; h++) o[h] = a0[h];
        if (j + 1 < N) {
#pragma unroll
            for (int h = 0; h < K2; h++) o[K2 + h] = a1[h];
        }
    }
}

// Column j's Y_j . U_j as one partial sum per workgroup at part[j * MM_MG + blockIdx.x].  A workgroup of 64 * K / 2 threads owns rpb rows
// (a multiple of 64); its 64 row lanes r = tid / (K / 2) add rows r, r + 64, ... in order, then meet as ONE binary tree over r (bits
// 0 .. 5 in turn: inside a wavefront by xor, then the wavefronts pairwise) -- the same tree for K = 2, 4, 8, so a column's partials
// do not depend on K.  The consumer adds them in index order (msum).
template <int K>
__global__ __launch_bounds__(32 * K) void k_dnm_dot(const double *__restrict__ Y, const double *__restrict__ U, int n, int rpb,
                                                    double *__restrict__ part, const int *done)
{
    constexpr int K2 = K / 2;
    __shared__ double wsh[K2][K];
    if (done && *done) return;
    const int c = threadIdx.x % K2, r = threadIdx.x / K2;
    const int i0 = blockIdx.x * rpb, i1 = min(n, i0 + rpb);
    m2d acc = (m2d)(0.0);
    for (int i = i0 + r; i < i1; i += 64) {
        const m2d y = reinterpret_cast<const m2d *>(Y)[(int64_t)i * K2 + c], u = reinterpret_cast<const m2d *>(U)[(int64_t)i * K2 + c];
        acc.x = fma(y.x, u.x, acc.x); acc.y = fma(y.y, u.y, acc.y);
    }
#pragma unroll
    for (int off = K2; off <= 32; off <<= 1) { acc.x += __shfl_xor(acc.x, off, 64); acc.y += __shfl_xor(acc.y, off, 64); }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane < K2) { wsh[w][2 * lane] = acc.x; wsh[w][2 * lane + 1] = acc.y; }
    __syncthreads();
    if (threadIdx.x < K) {
        const int j = threadIdx.x;
        double v;
        if (K2 == 1) v = wsh[0][j];
        else if (K2 == 2) v = wsh[0][j] + wsh[1][j];
        else v = (wsh[0][j] + wsh[1][j]) + (wsh[2][j] + wsh[K2 - 1][j]);
        part[(size_t)j * MM_MG + blockIdx.x] = v;
    }
}

// the k results of lcg_hip_dense_op_multi_dot out of their partial sums
template <int K>
__global__ __launch_bounds__(VB) void k_dnm_dots(const double *dots, int slots, double *out)
{
    __shared__ double sums[K];
    msum<K>(dots, slots, sums);
    if (threadIdx.x < K) out[threadIdx.x] = sums[threadIdx.x];
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
    HIPCHK(hipMalloc(&w->part, sizeof(double) * (size_t)dnm_table_doubles(K->M, K->N, K->NP) * k * (K->cplx ? 2 : 1) + 16));
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
static int launched(const char *what)
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(e, what, __FILE__, __LINE__);
}

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

// Y[M x k] = K.X; variant: DN_ROW / DN_ROW_SPLIT force a form, anything else is the automatic choice.  *launches grows by what ran
static int row_product(lcg_hip_dense *D, int k, const double *X, double *Y, int variant, hipStream_t s, const int *done, int *launches)
{
    const bool forced = variant == DN_ROW_SPLIT;
    const bool split = forced || (variant != DN_ROW && row_split_auto(D->M, D->NP));
    const RowPlan r = row_plan(D->M, D->NP, split, forced);
    double *out = r.S > 1 ? D->multi->part : Y;
    if (k == 2) row_dispatch<2>(D, r, X, out, s, done);
    else if (k == 4) row_dispatch<4>(D, r, X, out, s, done);
    else row_dispatch<8>(D, r, X, out, s, done);
    if (r.S > 1) dnm_fold_launch(D->multi->part, r.S, (int64_t)D->M * k, Y, s, done);
    *launches += r.S > 1 ? 2 : 1;
    D->multi->last_kernel = r.S > 1 ? DNM_NAMES[1] : DNM_NAMES[0];
    return launched("dense k-wide row product");
}

// Y[N x k] = K^T.X
static int col_product(lcg_hip_dense *D, int k, const double *X, double *Y, hipStream_t s, const int *done, int *launches)
{
    const ColPlan c = col_plan(D->M, D->NP);
    const int64_t n_out = (int64_t)D->N * k;
    double *out = c.RS > 1 ? D->multi->part : Y;
    const dim3 grid((unsigned)c.CT, (unsigned)c.RS);
#define DNM_COL(kk) hipLaunchKernelGGL((k_dnm_col<kk>), grid, dim3(256), 0, s, D->val, D->ldp, D->M, D->N, D->NP, c.CW, c.rps, X, out, n_out, done)
    if (k == 2) DNM_COL(2); else if (k == 4) DNM_COL(4); else DNM_COL(8);
#undef DNM_COL
    if (c.RS > 1) dnm_fold_launch(D->multi->part, c.RS, n_out, Y, s, done);
    *launches += c.RS > 1 ? 2 : 1;
    D->multi->last_kernel = DNM_NAMES[2];
    return launched("dense k-wide column product");
}

// Y[N x k] = K^T.(K.X): the row form into the handle's M x k block, then the column form (the forced row variants reach the first stage)
static int ata_product(lcg_hip_dense *D, int k, const double *X, double *Y, hipStream_t s, const int *done, int *launches)
{
    const int v = D->variant;
    int rc = row_product(D, k, X, D->multi->t, v == DN_ROW || v == DN_ROW_SPLIT ? v : DN_AUTO, s, done, launches);
    if (!rc) rc = col_product(D, k, D->multi->t, Y, s, done, launches);
    D->multi->last_kernel = DNM_NAMES[3];
    return rc;
}

// rows a workgroup of k_dnm_dot owns: a multiple of 64 that leaves at most MM_MG workgroups
static int dot_rows_per_block(int n) { return 64 * (int)cdiv(cdiv(n, 64), MM_MG); }

static int dot_launch(int k, int n, const double *Y, const double *U, double *dots, int *slots, hipStream_t s, const int *done)
{
    const int rpb = dot_rows_per_block(n), nb = (int)cdiv(n, rpb);
    if (k == 2) hipLaunchKernelGGL((k_dnm_dot<2>), dim3(nb), dim3(64), 0, s, Y, U, n, rpb, dots, done);
    else if (k == 4) hipLaunchKernelGGL((k_dnm_dot<4>), dim3(nb), dim3(128), 0, s, Y, U, n, rpb, dots, done);
    else hipLaunchKernelGGL((k_dnm_dot<8>), dim3(nb), dim3(256), 0, s, Y, U, n, rpb, dots, done);
    *slots = nb;
    return launched("dense k-wide dot");
}

// The operator of the batched loops: Y = (normal ? K^T.K : K).X and, with U, column j's Y_j . U_j as *slots partial sums at
// dots[j * MM_MG ...].  The handle has been checked and its work memory reserved for k.
int dnm_op(lcg_hip_dense *D, int k, int normal, const double *X, double *Y, hipStream_t s, const int *done, const double *U, double *dots,
           int *slots, int *launches)
{
    int rc = normal ? ata_product(D, k, X, Y, s, done, launches) : row_product(D, k, X, Y, D->variant, s, done, launches);
    if (rc || !U) return rc;
    (*launches)++;
    return dot_launch(k, D->N, Y, U, dots, slots, s, done);
}

// a real dense handle, or nullptr with the entry's name and the reason in lcg_hip_last_error()
lcg_hip_dense *dnm_handle(const char *entry, const void *h)
{
    if (!dense_handle(h)) { dnm_error("%s: the handle is not a dense matrix (lcg_hip_dense_create)", entry); return nullptr; }
    lcg_hip_dense *D = static_cast<lcg_hip_dense *>(const_cast<void *>(h));
    if (D->cplx) { dnm_error("%s: the matrix is complex; the k-wide dense path serves real fp64 matrices", entry); return nullptr; }
    return D;
}

static bool overlap(const double *a, size_t na, const double *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 8 * na, b0 = (uintptr_t)b, b1 = b0 + 8 * nb;
    return a0 < b1 && b0 < a1;
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
    if (layout < 0 || layout > 1) return dnm_error("%s: layout = %d (0: K.X, 1: K^T.X)", entry, layout);
    const size_t nx = (size_t)(layout ? D->M : D->N) * k, ny = (size_t)(layout ? D->N : D->M) * k;
    if (overlap(X, nx, Y, ny)) return dnm_error("%s: X and Y overlap", entry);
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    int launches = 0;
    return layout ? col_product(D, k, X, Y, ctx().stream, nullptr, &launches) : row_product(D, k, X, Y, D->variant, ctx().stream, nullptr, &launches);
}

int lcg_hip_dense_ata_multi(lcg_hip_dense_t K, int k, const double *X, double *Y)
{
    const char *entry = "lcg_hip_dense_ata_multi";
    TRY(multi_args(entry, k, X, Y));
    lcg_hip_dense *D = dnm_handle(entry, K);
    if (!D) return LCG_HIP_E_ARG;
    if (overlap(X, (size_t)D->N * k, Y, (size_t)D->N * k)) return dnm_error("%s: X and Y overlap", entry);
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
    if (normal != 0 && normal != 1) return dnm_error("%s: normal = %d (1: K^T.K, 0: K)", entry, normal);
    if (!normal && D->M != D->N) return dnm_error("%s: the matrix is %d x %d: normal = 0 needs a square one", entry, D->M, D->N);
    const size_t nv = (size_t)D->N * k;
    if (overlap(X, nv, Y, nv) || (U && overlap(U, nv, Y, nv))) return dnm_error("%s: Y overlaps X or U", entry);
    if (dots && !U) return dnm_error("%s: dots without U", entry);
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    Ctx &c = ctx();
    // (outside a solve the k-wide table of the loops is free: partials_pair[0] holds the partial sums, ax_partials the results)
    int slots = 0, launches = 0;
    TRY(dnm_op(D, k, normal, X, Y, c.stream, nullptr, U, c.partials_pair[0], &slots, &launches));
    if (!U || !dots) return 0;
    if (k == 2) hipLaunchKernelGGL((k_dnm_dots<2>), dim3(1), dim3(VB), 0, c.stream, c.partials_pair[0], slots, c.ax_partials);
    else if (k == 4) hipLaunchKernelGGL((k_dnm_dots<4>), dim3(1), dim3(VB), 0, c.stream, c.partials_pair[0], slots, c.ax_partials);
    else hipLaunchKernelGGL((k_dnm_dots<8>), dim3(1), dim3(VB), 0, c.stream, c.partials_pair[0], slots, c.ax_partials);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c.scratch_host, c.ax_partials, sizeof(double) * k, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    for (int j = 0; j < k; j++) dots[j] = c.scratch_host[j];
    return 0;
}

const char *lcg_hip_dense_multi_last_kernel(lcg_hip_dense_t K)
{
    if (!dense_handle(K)) { dnm_error("lcg_hip_dense_multi_last_kernel: the handle is not a dense matrix (lcg_hip_dense_create)"); return ""; }
    return K->multi ? K->multi->last_kernel : "";
}

const char *lcg_hip_dense_multi_kernel_name(int index)
{
    return index >= 0 && index < (int)(sizeof DNM_NAMES / sizeof *DNM_NAMES) ? DNM_NAMES[index] : nullptr;
}

} // extern "C"
