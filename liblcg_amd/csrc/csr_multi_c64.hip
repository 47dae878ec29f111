// csr_multi_c64.hip -- Y = A.X for k = 2, 4, 8 complex64 vectors at once (complex64 CSR, one GPU): clcg_hip_spmm_c64,
// clcg_hip_spmm_dot_c64.  The batched counterpart of lcg_hip_spmv_c64 (clcg_cudaf.cu's cusparseSpMV with CUDA_C_32F).
//
// A complex64 entry costs 12 bytes (4 B column + 8 B value), a real entry's price: k vectors interleaved row by row (multi_c64.hpp)
// share ONE pass over col / val, and a gather of a row of X at k = 8 fetches 64 contiguous bytes -- the real k = 8 shape.
//
//  k_cspmm_c64<K, R>   k_spmm's mapping (csr_multi.hip) with a complex fp32 matrix value and K float-pair accumulators.  One 256-thread
//      block owns R consecutive rows (R * T = 256; T = 4 / 16 / 64 lanes per row by mean row length).  Its contiguous slice of col / val
//      streams from HBM into LDS window by window (C64MM_W entries), 16 bytes per lane per access (one for four columns, two for four
//      values), every load of a window issued before the first LDS store.  Lane (row = tid % R, slot j = tid / R) walks entries j,
//      j + T, ... of its row through the windows and gathers the row of X as K / 2 16-byte loads.  Per entry acc = a * x + acc in fp32
//      in multi_c64.hpp's fma order.  The T partial sums of a row meet in LDS in slot order, in fp32 (the value window reused, as K / 2
//      16-byte pieces per lane); Y is written as whole rows.
//      Column j's sum is therefore added in an order fixed by the matrix alone: the same bits whatever the other columns hold, whatever
//      k is, wherever the column stands, from call to call.  No atomics.
//      <DOT>: the lanes that write Y multiply it with U (unconjugated: cublasCdotu) on the way out -- exact fp64 products of fp32
//      values, summed in fp64 -- and the block leaves one partial sum per column and component (more than MM_MG blocks: k_mm_fold
//      adds runs of consecutive blocks, in order).
//
// The host side is multi.hpp's frame (csr_multi.hip: multi_launch, multi_dot_run) with two table rows per column; the frame's block
// pointers are typed double and only carried through.  The handle's single-vector plans are neither used nor built.
#include "multi_c64.hpp"

namespace lcgh {

typedef int c64m4i __attribute__((ext_vector_type(4)));
typedef float c64m4f __attribute__((ext_vector_type(4)));      // two entries' values, or the two columns of a piece
typedef float c64m2f __attribute__((ext_vector_type(2)));

// (re, im) += a * x, csr_c64.hip's c64_mac order
__device__ __forceinline__ void c64m_mac2(c64m4f &acc, c64m2f a, c64m4f x)     // both columns of a piece
{
    acc.x = fmaf(-a.y, x.y, fmaf(a.x, x.x, acc.x)); acc.y = fmaf(a.y, x.x, fmaf(a.x, x.y, acc.y));
    acc.z = fmaf(-a.y, x.w, fmaf(a.x, x.z, acc.z)); acc.w = fmaf(a.y, x.z, fmaf(a.x, x.w, acc.w));
}

template <int K, int R, bool DOT>
__global__ __launch_bounds__(VB) void k_cspmm_c64(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                  const float *__restrict__ val, const float *__restrict__ X, float *__restrict__ Y,
                                                  const int *done, bool wide, const float *__restrict__ U, double *__restrict__ part,
                                                  int pstride)
{
    constexpr int T = VB / R, K2 = K / 2;
    constexpr int NRND = (C64MM_W / 4 + VB - 1) / VB;       // 4-entry units per lane and window
    constexpr int UNR = K == 8 ? 2 : 4;                     // entries whose rows of X a lane keeps in flight (k_spmm's: the same bytes)
    static_assert(VB * K <= C64MM_W, "the row-sum exchange must fit the value window");
    static_assert(R <= 64, "the lanes that finish rows sit in the first wavefront");
    static_assert(C64MM_W % 4 == 0, "windows start at 4-entry units");
    __shared__ __attribute__((aligned(16))) c64m2f sval[C64MM_W];
    __shared__ __attribute__((aligned(16))) int scol[C64MM_W];
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
    const c64m4f *Xv = reinterpret_cast<const c64m4f *>(X);
    const c64m2f *Vv = reinterpret_cast<const c64m2f *>(val);

    c64m4f acc[K2];
#pragma unroll
    for (int h = 0; h < K2; h++) acc[h] = (c64m4f)(0.0f);
    int k = rs + j0;
    for (int w0 = base; w0 < end; w0 += C64MM_W) {          // (uniform over the block)
        const int cnt = min(C64MM_W, end - w0);
        c64m4i pc[NRND]; c64m4f pv[NRND * 2];
        if (wide) {
            // col / val 16-byte aligned with >= 64 readable bytes behind their last entry (CsrPart::padded; a unit reaches at most 3
            // entries = 24 B of val, 12 B of col past the slice).  Branch-free: lanes past the window re-read its first unit
#pragma unroll
            for (int r = 0; r < NRND; r++) {
                const int u = tid * 4 + r * VB * 4;
                const long g = (long)w0 + (u < cnt ? u : 0);
                pc[r] = *reinterpret_cast<const c64m4i *>(col + g);
                pv[2 * r] = reinterpret_cast<const c64m4f *>(Vv + g)[0];
                pv[2 * r + 1] = reinterpret_cast<const c64m4f *>(Vv + g)[1];
            }
        } else {
            // arrays the caller keeps (adopted) without slack or alignment: entry by entry, never past the slice
#pragma unroll
            for (int r = 0; r < NRND; r++) {
                const int u = tid * 4 + r * VB * 4;
                int c4[4]; float v8[8];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const long g = (long)w0 + (u + q < cnt ? u + q : 0);
                    c4[q] = col[g]; v8[2 * q] = val[2 * g]; v8[2 * q + 1] = val[2 * g + 1];
                }
                pc[r].x = c4[0]; pc[r].y = c4[1]; pc[r].z = c4[2]; pc[r].w = c4[3];
                pv[2 * r].x = v8[0]; pv[2 * r].y = v8[1]; pv[2 * r].z = v8[2]; pv[2 * r].w = v8[3];
                pv[2 * r + 1].x = v8[4]; pv[2 * r + 1].y = v8[5]; pv[2 * r + 1].z = v8[6]; pv[2 * r + 1].w = v8[7];
            }
        }
        __builtin_amdgcn_sched_barrier(0);      // every load of the window above every LDS store (csr.hip: lds1_block)
#pragma unroll
        for (int r = 0; r < NRND; r++) {
            const int u = tid * 4 + r * VB * 4;
            if (u < cnt) {                      // (C64MM_W is a multiple of 4: the unit lies inside the window's buffers)
                *reinterpret_cast<c64m4i *>(scol + u) = pc[r];
                reinterpret_cast<c64m4f *>(sval + u)[0] = pv[2 * r];
                reinterpret_cast<c64m4f *>(sval + u)[1] = pv[2 * r + 1];
            }
        }
        __syncthreads();
        // this lane's entries inside the window, in order (k stays where the window ends: the next one goes on from there)
        const int stop = min(re, w0 + cnt);
        for (; k < stop - (UNR - 1) * T; k += UNR * T) {
            int c[UNR]; c64m2f a[UNR]; c64m4f xv[UNR][K2];
#pragma unroll
            for (int q = 0; q < UNR; q++) { c[q] = scol[k + q * T - w0]; a[q] = sval[k + q * T - w0]; }
#pragma unroll
            for (int q = 0; q < UNR; q++)
#pragma unroll
                for (int h = 0; h < K2; h++) xv[q][h] = Xv[(long)c[q] * K2 + h];
#pragma unroll
            for (int q = 0; q < UNR; q++)
#pragma unroll
                for (int h = 0; h < K2; h++) c64m_mac2(acc[h], a[q], xv[q][h]);
        }
        for (; k < stop; k += T) {
            const int c = scol[k - w0]; const c64m2f a = sval[k - w0];
#pragma unroll
            for (int h = 0; h < K2; h++) c64m_mac2(acc[h], a, Xv[(long)c * K2 + h]);
        }
        __syncthreads();
    }
    // the T partial sums of a row meet in LDS (the value window reused; [piece][slot][row]: consecutive lanes, consecutive 16 bytes)
    c64m4f *sred = reinterpret_cast<c64m4f *>(sval);
#pragma unroll
    for (int h = 0; h < K2; h++) sred[(h * T + j0) * R + rl] = acc[h];
    __syncthreads();
    double dre[K], dim[K];
    if (mine) {
#pragma unroll
        for (int h = 0; h < K2; h++) {
            c64m4f v = sred[(h * T) * R + rl];
            for (int j = 1; j < T; j++) v += sred[(h * T + j) * R + rl];
            reinterpret_cast<c64m4f *>(Y)[(long)(row0 + rl) * K2 + h] = v;
            if (DOT) {
                const c64m4f u = reinterpret_cast<const c64m4f *>(U)[(long)(row0 + rl) * K2 + h];
                dre[2 * h] = (double)v.x * u.x - (double)v.y * u.y; dim[2 * h] = (double)v.x * u.y + (double)v.y * u.x;
                dre[2 * h + 1] = (double)v.z * u.z - (double)v.w * u.w; dim[2 * h + 1] = (double)v.z * u.w + (double)v.w * u.z;
            }
        }
    } else if (DOT) {
#pragma unroll
        for (int j = 0; j < K; j++) { dre[j] = 0.0; dim[j] = 0.0; }
    }
    if (DOT && tid < 64) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double tr = wave_sum(dre[j]), ti = wave_sum(dim[j]);
            if (tid == WSUM_LANE) { part[(size_t)(2 * j) * pstride + blockIdx.x] = tr; part[(size_t)(2 * j + 1) * pstride + blockIdx.x] = ti; }
        }
    }
}

// k_cspmm_c64<k, R, DOT> for multi.hpp's frame (two table rows per column: `tab` is not looked at); X, Y, U are float blocks
static void cspmm_c64_go(const CsrPart &P, int k, int R, const double *X, double *Y, hipStream_t s, const int *done, bool wide,
                         const double *U, double *part, int pstride, int)
{
    const float *val = reinterpret_cast<const float *>(P.val), *Xf = reinterpret_cast<const float *>(X), *Uf = reinterpret_cast<const float *>(U);
    float *Yf = reinterpret_cast<float *>(Y);
    multi_k(k, [&](auto K) {
        return multi_r(R, [&](auto RR) {
            constexpr int KK = decltype(K)::value, RV = decltype(RR)::value;
            const unsigned nb = (unsigned)(((long)P.n_rows + RV - 1) / RV);
            if (U) hipLaunchKernelGGL((k_cspmm_c64<KK, RV, true>), dim3(nb), dim3(VB), 0, s, P.n_rows, P.rowptr, P.col, val, Xf, Yf, done, wide, Uf, part, pstride);
            else hipLaunchKernelGGL((k_cspmm_c64<KK, RV, false>), dim3(nb), dim3(VB), 0, s, P.n_rows, P.rowptr, P.col, val, Xf, Yf, done, wide, Uf, part, pstride);
            return 0;
        });
    });
}

int cspmm_c64_launch(const CsrPart &P, int k, const float *X, float *Y, hipStream_t s, const int *done, const float *U, double *big,
                     double *dots, int *slots)
{
    return multi_launch(P, k, 2, cspmm_c64_go, reinterpret_cast<const double *>(X), reinterpret_cast<double *>(Y), s, done,
                        reinterpret_cast<const double *>(U), big, dots, slots);
}

int c64multi_handle(const char *entry, const lcg_hip_csr *A)
{
    const char *why = nullptr;
    if (!A) why = "the handle is null";
    else if (dense_handle(A)) { refuse_dense(entry); return LCG_HIP_E_ARG; }
    else if (A->is_complex) why = "the matrix holds complex128 values; the complex64 multi-vector path serves complex64 matrices (complex128: clcg_hip_spmm)";
    else if (!A->c64) why = "the matrix is real; the complex64 multi-vector path serves complex64 matrices (real: lcg_hip_spmm)";
    else if (A->distributed) why = "the matrix's rows are sharded (lcg_hip_csr_distribute); the multi-vector path serves whole matrices on one GPU";
    if (!why) return 0;
    ctx().err = std::string(entry) + ": " + why;
    return LCG_HIP_E_ARG;
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int clcg_hip_spmm_c64(lcg_hip_csr_t A, int k, const float *X, float *Y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);        // (a handle of the other kind is refused before anything else is looked at, as everywhere)
    TRY(multi_args("clcg_hip_spmm_c64", k, X, Y));
    TRY(c64multi_handle("clcg_hip_spmm_c64", A));
    TRY(ensure_init());
    Ctx &c = ctx();
    return cspmm_c64_launch(A->main, k, X, Y, c.stream, nullptr);
}

int clcg_hip_spmm_dot_c64(lcg_hip_csr_t A, int k, const float *X, float *Y, const float *U, double *dots)
{
    static const char *entry = "clcg_hip_spmm_dot_c64";
    NOT_DENSE(A, LCG_HIP_E_ARG);
    TRY(multi_args(entry, k, X, Y, U));
    if (!dots) { ctx().err = std::string(entry) + ": the result array is a null pointer"; return LCG_HIP_E_ARG; }
    TRY(c64multi_handle(entry, A));
    return multi_dot_run(A->main, k, 2, cspmm_c64_go, reinterpret_cast<const double *>(X), reinterpret_cast<double *>(Y),
                         reinterpret_cast<const double *>(U), dots);
}

} // extern "C"
