// csr_multi_cplx.hip -- Y = A.X for k = 2, 4, 8 complex vectors at once (complex128 CSR, one GPU): clcg_hip_spmm, clcg_hip_spmm_dot,
// clcg_hip_spmm_inner, clcg_hip_spmm_dot2.
//
// A complex entry costs 20 bytes (4 B column + 16 B value) and the single-vector complex product has nothing cheaper to offer: k
// vectors interleaved row by row (multi_cplx.hpp) share ONE pass over col / val, and every gather of x fetches k * 16 contiguous bytes.
//
//  k_cspmm<K, R>   k_spmm's mapping (csr_multi.hip) with a complex matrix value and K complex accumulators.  One 256-thread block owns
//      R consecutive rows (R * T = 256; T = 4 / 16 / 64 lanes per row by mean row length).  Its contiguous slice of col / val streams
//      from HBM into LDS window by window (CMM_W entries), 16 bytes per lane per access, every load of a window issued before the first
//      LDS store.  Lane (row = tid % R, slot j = tid / R) walks entries j, j + T, ... of its row through the windows and gathers the
//      row of X as K 16-byte loads.  The T partial sums of a row meet in LDS in slot order (the value window reused; K = 8: two rounds of
//      four columns, 256 x 8 x 16 B do not fit it); Y is written as whole rows.
//      Column j's sum is therefore added in an order fixed by the matrix alone: the same bits whatever the other columns hold, whatever
//      k is, from call to call.  No atomics.
//      <MODE>: the lanes that write Y multiply it on the way out and the block leaves one partial sum per column and component (more
//      than MM_MG blocks: k_mm_fold adds runs of consecutive blocks, in order).  Mapping, windows, the order of the row sums and the
//      bits of Y are the same in every mode.
//        CSPMM_DOT    with the block U, unconjugated (clcg_dot, cublasZdotu): what BiCG-sym and PCG take (d.Ad);
//        CSPMM_INNER  conj(u_i) Y_ij with ONE vector u of n elements for all columns, 16 bytes per row: BiCGStab's <rbar0, A.p>;
//        CSPMM_DOT2   conj(Y_ij) U_ij with the block U and, as a third, real sum, |Y_ij|^2: BiCGStab's <A.s, s> and <A.s, A.s>.
//      The conjugated products are formed as acc_inner forms them (solvers_cplx.hip).
//
// The host side is multi.hpp's frame (csr_multi.hip: multi_launch, multi_dot_run) with two table rows per column (CSPMM_DOT2: three);
// this unit adds the kernel, its launcher and the handle's check.  The handle's single-vector plans are neither used nor built.
#include "multi_cplx.hpp"
#include "lcg_hip_staging.h"

namespace lcgh {

typedef int cm4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ m2d cmac(m2d a, m2d x, m2d acc)     // a * x + acc, cfma's order (devcommon.hpp)
{
    m2d r;
    r.x = fma(a.x, x.x, fma(-a.y, x.y, acc.x));
    r.y = fma(a.x, x.y, fma(a.y, x.x, acc.y));
    return r;
}

template <int K, int R, int MODE>     // MODE: 0, or multi_cplx.hpp's CSPMM_DOT, CSPMM_INNER, CSPMM_DOT2
__global__ __launch_bounds__(VB) void k_cspmm(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                              const double *__restrict__ val, const double *__restrict__ X, double *__restrict__ Y,
                                              const int *done, bool wide, const double *__restrict__ U, double *__restrict__ part,
                                              int pstride)
{
    constexpr int T = VB / R;
    constexpr int NRND = (CMM_W / 4 + VB - 1) / VB;         // 4-entry units per lane and window
    constexpr int UNR = K == 8 ? 1 : 2;                     // entries whose rows of X a lane keeps in flight (K = 8 with 2: 124 VGPRs, 3-9 % slower)
    constexpr int XC = K == 8 ? 4 : K;                      // columns per round of the row-sum exchange
    static_assert(VB * XC <= CMM_W, "a round of the row-sum exchange must fit the value window");
    static_assert(R <= 64, "the lanes that finish rows sit in the first wavefront");
    static_assert(CMM_W % 4 == 0, "windows start at 4-entry units");
    __shared__ __attribute__((aligned(16))) m2d sval[CMM_W];
    __shared__ __attribute__((aligned(16))) int scol[CMM_W];
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
    const m2d *Vv = reinterpret_cast<const m2d *>(val);

    m2d acc[K];
#pragma unroll
    for (int h = 0; h < K; h++) acc[h] = (m2d)(0.0);
    int k = rs + j0;
    for (int w0 = base; w0 < end; w0 += CMM_W) {            // (uniform over the block)
        const int cnt = min(CMM_W, end - w0);
        cm4i pc[NRND]; m2d pv[NRND * 4];
        if (wide) {
            // col / val 16-byte aligned with >= 64 readable bytes behind their last entry (CsrPart::padded; a unit reaches at most 3
            // entries = 48 B past the slice).  Branch-free: lanes past the window re-read its first unit
#pragma unroll
            for (int r = 0; r < NRND; r++) {
                const int u = tid * 4 + r * VB * 4;
                const long g = (long)w0 + (u < cnt ? u : 0);
                pc[r] = *reinterpret_cast<const cm4i *>(col + g);
#pragma unroll
                for (int q = 0; q < 4; q++) pv[4 * r + q] = Vv[g + q];
            }
        } else {
            // arrays the caller keeps (adopted) without slack or alignment: entry by entry, never past the slice
#pragma unroll
            for (int r = 0; r < NRND; r++) {
                const int u = tid * 4 + r * VB * 4;
                int c4[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const long g = (long)w0 + (u + q < cnt ? u + q : 0);
                    c4[q] = col[g]; pv[4 * r + q].x = val[2 * g]; pv[4 * r + q].y = val[2 * g + 1];
                }
                pc[r].x = c4[0]; pc[r].y = c4[1]; pc[r].z = c4[2]; pc[r].w = c4[3];
            }
        }
        __builtin_amdgcn_sched_barrier(0);      // every load of the window above every LDS store (csr.hip: lds1_block)
#pragma unroll
        for (int r = 0; r < NRND; r++) {
            const int u = tid * 4 + r * VB * 4;
            if (u < cnt) {                      // (CMM_W is a multiple of 4: the unit lies inside the window's buffers)
                *reinterpret_cast<cm4i *>(scol + u) = pc[r];
#pragma unroll
                for (int q = 0; q < 4; q++) sval[u + q] = pv[4 * r + q];
            }
        }
        __syncthreads();
        // this lane's entries inside the window, in order (k stays where the window ends: the next one goes on from there)
        const int stop = min(re, w0 + cnt);
        for (; k < stop - (UNR - 1) * T; k += UNR * T) {
            int c[UNR]; m2d a[UNR]; m2d xv[UNR][K];
#pragma unroll
            for (int q = 0; q < UNR; q++) { c[q] = scol[k + q * T - w0]; a[q] = sval[k + q * T - w0]; }
#pragma unroll
            for (int q = 0; q < UNR; q++)
#pragma unroll
                for (int h = 0; h < K; h++) xv[q][h] = Xv[(long)c[q] * K + h];
#pragma unroll
            for (int q = 0; q < UNR; q++)
#pragma unroll
                for (int h = 0; h < K; h++) acc[h] = cmac(a[q], xv[q][h], acc[h]);
        }
        for (; k < stop; k += T) {
            const int c = scol[k - w0]; const m2d a = sval[k - w0];
#pragma unroll
            for (int h = 0; h < K; h++) acc[h] = cmac(a, Xv[(long)c * K + h], acc[h]);
        }
        __syncthreads();
    }
    // the T partial sums of a row meet in LDS (the value window reused; [column][slot][row]: consecutive lanes, consecutive 16 bytes)
    double dre[K], dim[K], dsq[K];
    m2d us = (m2d)(0.0);                                    // CSPMM_INNER: the shared vector's element of this row, read once
    if (MODE == CSPMM_INNER && mine) us = reinterpret_cast<const m2d *>(U)[row0 + rl];
#pragma unroll
    for (int h0 = 0; h0 < K; h0 += XC) {
#pragma unroll
        for (int h = 0; h < XC; h++) sval[(h * T + j0) * R + rl] = acc[h0 + h];
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int h = 0; h < XC; h++) {
                m2d v = sval[(h * T) * R + rl];
                for (int j = 1; j < T; j++) v += sval[(h * T + j) * R + rl];
                reinterpret_cast<m2d *>(Y)[(long)(row0 + rl) * K + h0 + h] = v;
                if (MODE == CSPMM_DOT) {
                    const m2d u = reinterpret_cast<const m2d *>(U)[(long)(row0 + rl) * K + h0 + h];
                    dre[h0 + h] = v.x * u.x - v.y * u.y; dim[h0 + h] = v.x * u.y + v.y * u.x;
                }
                if (MODE == CSPMM_INNER) {                  // conj(u) y: acc_inner's products (solvers_cplx.hip)
                    dre[h0 + h] = us.x * v.x + us.y * v.y; dim[h0 + h] = us.x * v.y - us.y * v.x;
                }
                if (MODE == CSPMM_DOT2) {                   // conj(y) u the same way, and |y|^2 (cnorm)
                    const m2d u = reinterpret_cast<const m2d *>(U)[(long)(row0 + rl) * K + h0 + h];
                    dre[h0 + h] = v.x * u.x + v.y * u.y; dim[h0 + h] = v.x * u.y - v.y * u.x;
                    dsq[h0 + h] = v.x * v.x + v.y * v.y;
                }
            }
        } else if (MODE) {
#pragma unroll
            for (int h = 0; h < XC; h++) { dre[h0 + h] = 0.0; dim[h0 + h] = 0.0; dsq[h0 + h] = 0.0; }
        }
        if (h0 + XC < K) __syncthreads();
    }
    if (MODE && tid < 64) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double tr = wave_sum(dre[j]), ti = wave_sum(dim[j]);
            if (tid == WSUM_LANE) { part[(size_t)(2 * j) * pstride + blockIdx.x] = tr; part[(size_t)(2 * j + 1) * pstride + blockIdx.x] = ti; }
        }
    }
    if (MODE == CSPMM_DOT2 && tid < 64) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double tq = wave_sum(dsq[j]);
            if (tid == WSUM_LANE) part[(size_t)(2 * K + j) * pstride + blockIdx.x] = tq;
        }
    }
}

// k_cspmm<k, R, MODE> for multi.hpp's frame (`tab` is not looked at: MODE fixes the table rows per column); without U the plain product
template <int MODE>
static void cspmm_go(const CsrPart &P, int k, int R, const double *X, double *Y, hipStream_t s, const int *done, bool wide, const double *U,
                     double *part, int pstride, int)
{
    multi_k(k, [&](auto K) {
        return multi_r(R, [&](auto RR) {
            constexpr int KK = decltype(K)::value, RV = decltype(RR)::value;
            const unsigned nb = (unsigned)(((long)P.n_rows + RV - 1) / RV);
            if (U) hipLaunchKernelGGL((k_cspmm<KK, RV, MODE>), dim3(nb), dim3(VB), 0, s, P.n_rows, P.rowptr, P.col, P.val, X, Y, done, wide, U, part, pstride);
            else hipLaunchKernelGGL((k_cspmm<KK, RV, 0>), dim3(nb), dim3(VB), 0, s, P.n_rows, P.rowptr, P.col, P.val, X, Y, done, wide, U, part, pstride);
            return 0;
        });
    });
}
static MultiGo cspmm_go_of(int mode) { return mode == CSPMM_INNER ? cspmm_go<CSPMM_INNER> : mode == CSPMM_DOT2 ? cspmm_go<CSPMM_DOT2> : cspmm_go<CSPMM_DOT>; }

int cspmm_launch(const CsrPart &P, int k, const double *X, double *Y, hipStream_t s, const int *done, const double *U, double *big,
                 double *dots, int *slots, int mode)
{
    return multi_launch(P, k, cspmm_tab(mode), cspmm_go_of(mode), X, Y, s, done, U, big, dots, slots);
}

int cmulti_handle(const char *entry, const lcg_hip_csr *A)
{
    const char *why = nullptr;
    if (!A) why = "the handle is null";
    else if (dense_handle(A)) { refuse_dense(entry); return LCG_HIP_E_ARG; }
    else if (A->c64) why = "the matrix holds complex64 values; the complex multi-vector path serves complex128 matrices";
    else if (!A->is_complex) why = "the matrix is real; the complex multi-vector path serves complex128 matrices (real: lcg_hip_spmm)";
    else if (A->distributed) why = "the matrix's rows are sharded (lcg_hip_csr_distribute); the multi-vector path serves whole matrices on one GPU";
    if (!why) return 0;
    ctx().err = std::string(entry) + ": " + why;
    return LCG_HIP_E_ARG;
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int clcg_hip_spmm(lcg_hip_csr_t A, int k, const double *X, double *Y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);        // (a handle of the other kind is refused before anything else is looked at, as everywhere)
    TRY(multi_args("clcg_hip_spmm", k, X, Y));
    TRY(cmulti_handle("clcg_hip_spmm", A));
    TRY(ensure_init());
    Ctx &c = ctx();
    return cspmm_launch(A->main, k, X, Y, c.stream, nullptr);
}

int clcg_hip_spmm_dot(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *U, double *dots)
{
    static const char *entry = "clcg_hip_spmm_dot";
    NOT_DENSE(A, LCG_HIP_E_ARG);
    TRY(multi_args(entry, k, X, Y, U));
    if (!dots) { ctx().err = std::string(entry) + ": the result array is a null pointer"; return LCG_HIP_E_ARG; }
    TRY(cmulti_handle(entry, A));
    return multi_dot_run(A->main, k, 2, cspmm_go<CSPMM_DOT>, X, Y, U, dots);
}

int clcg_hip_spmm_inner(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *u, double *dots)
{
    static const char *entry = "clcg_hip_spmm_inner";
    NOT_DENSE(A, LCG_HIP_E_ARG);
    TRY(multi_args(entry, k, X, Y, u));
    if (!dots) { ctx().err = std::string(entry) + ": the result array is a null pointer"; return LCG_HIP_E_ARG; }
    TRY(cmulti_handle(entry, A));
    return multi_dot_run(A->main, k, 2, cspmm_go<CSPMM_INNER>, X, Y, u, dots);
}

int clcg_hip_spmm_dot2(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *U, double *dots3)
{
    static const char *entry = "clcg_hip_spmm_dot2";
    NOT_DENSE(A, LCG_HIP_E_ARG);
    TRY(multi_args(entry, k, X, Y, U));
    if (!dots3) { ctx().err = std::string(entry) + ": the result array is a null pointer"; return LCG_HIP_E_ARG; }
    TRY(cmulti_handle(entry, A));
    return multi_dot_run(A->main, k, 3, cspmm_go<CSPMM_DOT2>, X, Y, U, dots3);
}

} // extern "C"
