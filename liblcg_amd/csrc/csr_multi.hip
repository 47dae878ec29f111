// csr_multi.hip -- Y = A.X for k = 2, 4, 8 vectors at once (real fp64 CSR, one GPU): lcg_hip_spmm, lcg_hip_spmm_dot, lcg_hip_spmm_dot2.
//
// The product is what an iteration costs, and one vector cannot pay less for it than 12 bytes per entry.  k vectors interleaved row
// by row (multi.hpp) share ONE pass over col / val, and every gather of x fetches k * 8 contiguous bytes.
//
//  k_spmm<K, R>   k_spmv_lds1's mapping (csr.hip) with a scalar matrix value and K accumulators.  One 256-thread block owns R
//      consecutive rows (R * T = 256).  Its contiguous slice of col / val streams from HBM into LDS window by window (MM_CH
//      entries), 16 bytes per lane per access, every load of a window issued before the first LDS store: the CSR arrays are read
//      exactly once, at full width, whatever the row lengths.  Lane (row = tid % R, slot j = tid / R) walks entries j, j + T, ... of
//      its row through the windows -- a row of thousands of entries simply spans several of them, its lanes' K sums staying in
//      registers -- and gathers the row of X as K / 2 16-byte loads.  The T partial sums of a row meet in LDS in slot order; Y is
//      written as whole rows.
//      Column j's sum is therefore added in an order fixed by the matrix alone (R comes from the mean row length): the same bits
//      whatever the other columns hold, whatever k is, from call to call.  No atomics.
//      <DOT>: the lanes that write Y multiply it with U on the way out and the block leaves one partial sum per column, as
//      k_spmv_lds1d does for one vector (more than MM_MG blocks: k_mm_fold adds runs of consecutive blocks, in order).
//      <DOT = 2>: the same lanes also square what they write: a second partial sum per column, (A.X)_j . (A.X)_j, in rows K .. 2K - 1
//      of the table -- the two sums BiCGStab takes after its second product (t.s, t.t).  The first has the bits of <DOT = 1>'s.
//
// This unit also defines what multi.hpp declares for all four k-wide product units: the CSR launch frame (multi_launch: R, wide loads,
// folding, slots) that the complex product runs under too, the fold of the partial sums (k_mm_fold), the read-out of every *_dot entry
// (multi_dots_read: k_mm_dots<NS>), multi_dot_run, multi_args and overlap.
//
// The handle's single-vector plans (packed columns, tiles, bins) are neither used nor built.
#include "multi.hpp"

namespace lcgh {

typedef int m4i __attribute__((ext_vector_type(4)));    // (native vector types: arrays of them stay in registers, csr.hip)

constexpr int MM_CH = 2304;     // entries per LDS window: 27,648 B of staging, five blocks per CU; 64 rows of 33 entries fit one

template <int K, int R, int DOT>
__global__ __launch_bounds__(VB) void k_spmm(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                             const double *__restrict__ val, const double *__restrict__ X, double *__restrict__ Y,
                                             const int *done, bool wide, const double *__restrict__ U, double *__restrict__ part,
                                             int pstride)
{
    constexpr int T = VB / R, K2 = K / 2;
    constexpr int NRND = (MM_CH / 4 + VB - 1) / VB;         // 4-entry units per lane and window
    constexpr int UNR = K == 8 ? 2 : 4;                     // entries whose rows of X a lane keeps in flight
    static_assert(T * R * K <= MM_CH, "the row-sum exchange must fit the staging buffer");
    static_assert(R <= 64, "the lanes that finish rows sit in the first wavefront");
    __shared__ __attribute__((aligned(16))) double sval[MM_CH];
    __shared__ __attribute__((aligned(16))) int scol[MM_CH];
    if (done && *done) return;
    const int tid = threadIdx.x;
    const int row0 = (int)blockIdx.x * R;
    const int nrows = min(R, n - row0);
    const int rl = tid % R, j0 = tid / R;
    const int base = rowptr[row0] & ~3, end = rowptr[row0 + nrows];
    const int rsafe = rl < nrows ? rl : 0;
    int rs = rowptr[row0 + rsafe], re = rowptr[row0 + rsafe + 1];
    if (rl >= nrows) { rs = 0; re = 0; }
    const bool mine = j0 == 0 && rl < nrows;
    const m2d *Xv = reinterpret_cast<const m2d *>(X);
    m2d uv[K2];
    if (DOT) {
#pragma unroll
        for (int h = 0; h < K2; h++) uv[h] = reinterpret_cast<const m2d *>(U)[(long)(mine ? row0 + rl : 0) * K2 + h];
    }

    m2d acc[K2];
#pragma unroll
    for (int h = 0; h < K2; h++) acc[h] = (m2d)(0.0);
    int k = rs + j0;
    for (int w0 = base; w0 < end; w0 += MM_CH) {            // (uniform over the block)
        const int cnt = min(MM_CH, end - w0);
        m4i pc[NRND]; m2d pv[NRND * 2];
        if (wide) {
            // col / val 16-byte aligned with >= 64 readable bytes behind their last entry (CsrPart::padded).  Branch-free: lanes past
            // the window re-read its first unit
#pragma unroll
            for (int r = 0; r < NRND; r++) {
                const int u = tid * 4 + r * VB * 4;
                const long g = (long)w0 + (u < cnt ? u : 0);
                pc[r] = *reinterpret_cast<const m4i *>(col + g);
                pv[2 * r] = reinterpret_cast<const m2d *>(val + g)[0];
                pv[2 * r + 1] = reinterpret_cast<const m2d *>(val + g)[1];
            }
        } else {
            // arrays the caller keeps (adopted) without slack or alignment: entry by entry, never past the slice
#pragma unroll
            for (int r = 0; r < NRND; r++) {
                const int u = tid * 4 + r * VB * 4;
                int c4[4]; double v4[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const long g = (long)w0 + (u + q < cnt ? u + q : 0);
                    c4[q] = col[g]; v4[q] = val[g];
                }
                pc[r].x = c4[0]; pc[r].y = c4[1]; pc[r].z = c4[2]; pc[r].w = c4[3];
                pv[2 * r].x = v4[0]; pv[2 * r].y = v4[1]; pv[2 * r + 1].x = v4[2]; pv[2 * r + 1].y = v4[3];
            }
        }
        __builtin_amdgcn_sched_barrier(0);      // every load of the window above every LDS store (csr.hip: lds1_block)
#pragma unroll
        for (int r = 0; r < NRND; r++) {
            const int u = tid * 4 + r * VB * 4;
            if (u < cnt) {
                *reinterpret_cast<m4i *>(scol + u) = pc[r];
                reinterpret_cast<m2d *>(sval + u)[0] = pv[2 * r];
                reinterpret_cast<m2d *>(sval + u)[1] = pv[2 * r + 1];
            }
        }
        __syncthreads();
        // this lane's entries inside the window, in order (k stays where the window ends: the next one goes on from there)
        const int stop = min(re, w0 + cnt);
        for (; k < stop - (UNR - 1) * T; k += UNR * T) {
            int c[UNR]; double a[UNR]; m2d xv[UNR][K2];
#pragma unroll
            for (int q = 0; q < UNR; q++) { c[q] = scol[k + q * T - w0]; a[q] = sval[k + q * T - w0]; }
#pragma unroll
            for (int q = 0; q < UNR; q++)
#pragma unroll
                for (int h = 0; h < K2; h++) xv[q][h] = Xv[(long)c[q] * K2 + h];
#pragma unroll
            for (int q = 0; q < UNR; q++)
#pragma unroll
                for (int h = 0; h < K2; h++) { acc[h].x = fma(a[q], xv[q][h].x, acc[h].x); acc[h].y = fma(a[q], xv[q][h].y, acc[h].y); }
        }
        for (; k < stop; k += T) {
            const int c = scol[k - w0]; const double a = sval[k - w0];
#pragma unroll
            for (int h = 0; h < K2; h++) {
                const m2d xv = Xv[(long)c * K2 + h];
                acc[h].x = fma(a, xv.x, acc[h].x); acc[h].y = fma(a, xv.y, acc[h].y);
            }
        }
        __syncthreads();
    }
    // the T partial sums of a row meet in LDS (the staging buffer reused; [piece][slot][row]: consecutive lanes, consecutive 16 bytes)
    m2d *sred = reinterpret_cast<m2d *>(sval);
#pragma unroll
    for (int h = 0; h < K2; h++) sred[(h * T + j0) * R + rl] = acc[h];
    __syncthreads();
    double dsum[K], dsq[K];
    if (mine) {
#pragma unroll
        for (int h = 0; h < K2; h++) {
            m2d v = sred[(h * T) * R + rl];
            for (int j = 1; j < T; j++) v += sred[(h * T + j) * R + rl];
            reinterpret_cast<m2d *>(Y)[(long)(row0 + rl) * K2 + h] = v;
            if (DOT) { dsum[2 * h] = v.x * uv[h].x; dsum[2 * h + 1] = v.y * uv[h].y; }
            if (DOT == 2) { dsq[2 * h] = v.x * v.x; dsq[2 * h + 1] = v.y * v.y; }
        }
    } else if (DOT) {
#pragma unroll
        for (int j = 0; j < K; j++) { dsum[j] = 0.0; dsq[j] = 0.0; }
    }
    if (DOT && tid < 64) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double t = wave_sum(dsum[j]);
            if (tid == WSUM_LANE) part[(size_t)j * pstride + blockIdx.x] = t;
        }
    }
    if (DOT == 2 && tid < 64) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double t = wave_sum(dsq[j]);
            if (tid == WSUM_LANE) part[(size_t)(K + j) * pstride + blockIdx.x] = t;
        }
    }
}

// more row blocks than a consumer adds up: sum f of a table row = its blocks f * per .. f * per + per - 1, in order (gridDim.y table rows)
__global__ __launch_bounds__(VB) void k_mm_fold(const double *__restrict__ big, int nb, int per, int nf, double *__restrict__ out)
{
    const int f = blockIdx.x * VB + threadIdx.x, j = blockIdx.y;
    if (f >= nf) return;
    const double *src = big + (size_t)j * nb;
    const int b0 = f * per, b1 = min(nb, b0 + per);
    double t = 0.0;
    for (int b = b0; b < b1; b++) t += src[b];
    out[j * MM_MG + f] = t;
}

// the NS results of a *_dot entry out of their partial sums
template <int NS>
__global__ __launch_bounds__(VB) void k_mm_dots(const double *dots, int slots, double *out)
{
    __shared__ double sums[NS];
    msum<NS>(dots, slots, sums);
    if (threadIdx.x < NS) out[threadIdx.x] = sums[threadIdx.x];
}

int multi_fold_launch(const double *big, int nb, int ns, double *out, hipStream_t s)
{
    const int per = (nb + MM_MG - 1) / MM_MG, nf = (nb + per - 1) / per;
    hipLaunchKernelGGL(k_mm_fold, dim3((nf + VB - 1) / VB, ns), dim3(VB), 0, s, big, nb, per, nf, out);
    return nf;
}

int multi_dots_read(Ctx &c, int ns, int slots, double *dots)
{
    // (outside a solve the k-wide table of the loops is free: partials_pair[0] holds the partial sums, ax_partials the results)
    const double *tab = c.partials_pair[0];
    switch (ns) {           // (6, 12, 24: three table rows per column, clcg_hip_spmm_dot2)
    case 2: hipLaunchKernelGGL((k_mm_dots<2>), dim3(1), dim3(VB), 0, c.stream, tab, slots, c.ax_partials); break;
    case 4: hipLaunchKernelGGL((k_mm_dots<4>), dim3(1), dim3(VB), 0, c.stream, tab, slots, c.ax_partials); break;
    case 6: hipLaunchKernelGGL((k_mm_dots<6>), dim3(1), dim3(VB), 0, c.stream, tab, slots, c.ax_partials); break;
    case 8: hipLaunchKernelGGL((k_mm_dots<8>), dim3(1), dim3(VB), 0, c.stream, tab, slots, c.ax_partials); break;
    case 12: hipLaunchKernelGGL((k_mm_dots<12>), dim3(1), dim3(VB), 0, c.stream, tab, slots, c.ax_partials); break;
    case 16: hipLaunchKernelGGL((k_mm_dots<16>), dim3(1), dim3(VB), 0, c.stream, tab, slots, c.ax_partials); break;
    case 24: hipLaunchKernelGGL((k_mm_dots<24>), dim3(1), dim3(VB), 0, c.stream, tab, slots, c.ax_partials); break;
    default: return LCG_HIP_E_ARG;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(c.scratch_host, c.ax_partials, sizeof(double) * ns, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return fail(e, "multi_dots_read", __FILE__, __LINE__);
    for (int j = 0; j < ns; j++) dots[j] = c.scratch_host[j];
    return 0;
}

static int rows_per_block(const CsrPart &P)
{
    const double mean = P.n_rows > 0 ? (double)P.nnz / P.n_rows : 0.0;
    return mean <= 48.0 ? 64 : (mean <= 256.0 ? 16 : 4);      // lanes per row: 4, 16, 64
}
static long multi_blocks(const CsrPart &P) { const int R = rows_per_block(P); return ((long)P.n_rows + R - 1) / R; }

size_t multi_big_doubles(const CsrPart &P, int ns)
{
    const long nb = multi_blocks(P);
    return nb > MM_MG ? (size_t)nb * ns : 0;
}

int multi_launch(const CsrPart &P, int k, int tab, MultiGo go, const double *X, double *Y, hipStream_t s, const int *done, const double *U,
                 double *big, double *dots, int *slots)
{
    const int R = rows_per_block(P);
    const long nb = multi_blocks(P);
    if (nb <= 0) return 0;
    const bool wide = P.padded && (((uintptr_t)P.col | (uintptr_t)P.val) & 15) == 0;
    const bool folded = U != nullptr && nb > MM_MG;
    if (U && (!dots || !slots || (folded && !big))) return LCG_HIP_E_ARG;
    go(P, k, R, X, Y, s, done, wide, U, folded ? big : dots, folded ? (int)nb : MM_MG, tab);
    HIPCHK(hipGetLastError());
    if (U) *slots = (int)nb;
    if (folded) {
        // (the fold runs whatever the stop flag says: after a stop it adds up what the last live product left, and nobody reads it)
        *slots = multi_fold_launch(big, (int)nb, tab * k, dots, s);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int multi_dot_run(const CsrPart &P, int k, int tab, MultiGo go, const double *X, double *Y, const double *U, double *dots)
{
    TRY(ensure_init());
    Ctx &c = ctx();
    double *big = nullptr;
    const size_t nbig = multi_big_doubles(P, tab * k);
    if (nbig) HIPCHK(hipMalloc(&big, sizeof(double) * nbig));
    int slots = 0;
    int rc = multi_launch(P, k, tab, go, X, Y, c.stream, nullptr, U, big, c.partials_pair[0], &slots);
    if (!rc) rc = multi_dots_read(c, tab * k, slots, dots);
    if (big) (void)hipFree(big);
    return rc;
}

// k_spmm<k, R, DOT> with DOT = 0 without U, else the table rows per column
static void spmm_go(const CsrPart &P, int k, int R, const double *X, double *Y, hipStream_t s, const int *done, bool wide, const double *U,
                    double *part, int pstride, int tab)
{
    multi_k(k, [&](auto K) {
        return multi_r(R, [&](auto RR) {
            constexpr int KK = decltype(K)::value, RV = decltype(RR)::value;
            const unsigned nb = (unsigned)(((long)P.n_rows + RV - 1) / RV);
            if (U && tab == 2) hipLaunchKernelGGL((k_spmm<KK, RV, 2>), dim3(nb), dim3(VB), 0, s, P.n_rows, P.rowptr, P.col, P.val, X, Y, done, wide, U, part, pstride);
            else if (U) hipLaunchKernelGGL((k_spmm<KK, RV, 1>), dim3(nb), dim3(VB), 0, s, P.n_rows, P.rowptr, P.col, P.val, X, Y, done, wide, U, part, pstride);
            else hipLaunchKernelGGL((k_spmm<KK, RV, 0>), dim3(nb), dim3(VB), 0, s, P.n_rows, P.rowptr, P.col, P.val, X, Y, done, wide, U, part, pstride);
            return 0;
        });
    });
}

int spmm_launch(const CsrPart &P, int k, const double *X, double *Y, hipStream_t s, const int *done, const double *U, double *big,
                double *dots, int *slots, bool dot2)
{
    if (dot2 && !U) return LCG_HIP_E_ARG;
    return multi_launch(P, k, dot2 ? 2 : 1, spmm_go, X, Y, s, done, U, big, dots, slots);
}

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

int multi_args(const char *entry, int k, const void *a, const void *b, const void *c)
{
    const char *why = nullptr;
    if (k != 2 && k != 4 && k != 8) why = "k must be 2, 4 or 8 (pad other counts with zero columns)";
    else if (!a || !b || !c) why = "a block of vectors is a null pointer";
    else if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) why = "a block of vectors is not 16-byte aligned";
    if (!why) return 0;
    ctx().err = std::string(entry) + ": " + why;
    return LCG_HIP_E_ARG;
}

int multi_handle(const char *entry, const lcg_hip_csr *A)
{
    const char *why = nullptr;
    if (!A) why = "the handle is null";
    else if (dense_handle(A)) { refuse_dense(entry); return LCG_HIP_E_ARG; }
    else if (A->c64) why = "the matrix holds complex64 values; the multi-vector path serves real fp64 matrices";
    else if (A->is_complex) why = "the matrix is complex; the multi-vector path serves real fp64 matrices";
    else if (A->distributed) why = "the matrix's rows are sharded (lcg_hip_csr_distribute); the multi-vector path serves whole matrices on one GPU";
    if (!why) return 0;
    ctx().err = std::string(entry) + ": " + why;
    return LCG_HIP_E_ARG;
}

// lcg_hip_spmm_dot (k sums) and lcg_hip_spmm_dot2 (2k: the Y.U sums, then the Y.Y sums)
static int spmm_dot_entry(const char *entry, lcg_hip_csr *A, int k, const double *X, double *Y, const double *U, double *dots, bool dot2)
{
    TRY(multi_args(entry, k, X, Y, U));
    TRY(multi_handle(entry, A));
    if (!dots) { ctx().err = std::string(entry) + ": the result array is a null pointer"; return LCG_HIP_E_ARG; }
    return multi_dot_run(A->main, k, dot2 ? 2 : 1, spmm_go, X, Y, U, dots);
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_spmm(lcg_hip_csr_t A, int k, const double *X, double *Y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);        // (a handle of the other kind is refused before anything else is looked at, as everywhere)
    TRY(multi_args("lcg_hip_spmm", k, X, Y));
    TRY(multi_handle("lcg_hip_spmm", A));
    TRY(ensure_init());
    Ctx &c = ctx();
    return spmm_launch(A->main, k, X, Y, c.stream, nullptr);
}

int lcg_hip_spmm_dot(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *U, double *dots)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return spmm_dot_entry("lcg_hip_spmm_dot", A, k, X, Y, U, dots, false);
}

int lcg_hip_spmm_dot2(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *U, double *dots2)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return spmm_dot_entry("lcg_hip_spmm_dot2", A, k, X, Y, U, dots2, true);
}

} // extern "C"
