// csr_tri_multi.hip -- an IC(0) / ILU(0) factor applied to a block of k = 2, 4, 8 vectors (multi.hpp's row-major layout): the k-wide
// Jacobi sweep (k_ic_scale_multi, k_ic_sweep_multi), the k-wide row of the exact solve (TriSolveRowMulti on the level walker of
// csr_tri.hpp), the apply that chooses between them, the factor's k-wide work vectors, and the two exported solves.  DESIGN 16.
//
// The point of it: a sweep reads the triangle's col / val ONCE for all k columns, and an exact solve walks the level chain ONCE.
// Column j of every row is summed exactly as the single-vector kernels of csr_tri.hip sum it -- one accumulator from x_i, the
// products subtracted in column order by a fused multiply-add (what `acc - a * y` compiles to there), one division by the stored
// diagonal and none by a unit one -- so a column of a batched apply has the bits of lcg_hip_ic0_solve / lcg_hip_ilu0_solve on
// that column alone, whatever the other columns hold.  No column's value ever meets another's: no shuffle, no shared sum, no atomic.
//
// A complex64 IC(0) factor has the same geometry: a row of k complex64 columns is k / 2 aligned 16-byte pieces of two
// columns, a factor value is 8 bytes.  The kernels are therefore templates on the arithmetic of a piece alone (IcmReal, IcmC64);
// IcmC64 calls csr_tri.hip's own vsub / ic_mul / ic_div on each half, so a column has the bits of lcg_hip_ic0_solve_c64.
#include "csr_tri.hpp"
#include "multi_c64.hpp"
#include "lcg_hip_staging_ic0_c64.h"

namespace lcgh {

typedef int icm_v4i __attribute__((ext_vector_type(4)));
typedef float icm_v4f __attribute__((ext_vector_type(4)));

// The arithmetic of a 16-byte piece (two neighbouring columns of one row) against one factor value.  P: the piece, V: the value.
struct IcmReal {        // fp64: (column c0, column c0 + 1) against a double
    typedef m2d P;
    typedef double V;
    // acc - a * y per column, as the single-vector row: one fused multiply-add
    static __device__ __forceinline__ m2d sub(m2d acc, double a, m2d y)
    {
        m2d r;
        r.x = fma(-a, y.x, acc.x);
        r.y = fma(-a, y.y, acc.y);
        return r;
    }
    static __device__ __forceinline__ m2d div(m2d acc, double d)
    {
        m2d r;
        r.x = acc.x / d;
        r.y = acc.y / d;
        return r;
    }
};
struct IcmC64 {         // complex64: (re, im) of column c0, (re, im) of column c0 + 1 against a float pair; each half as k_ic_sweep<float2>
    typedef icm_v4f P;
    typedef float2 V;
    static __device__ __forceinline__ float2 lo(icm_v4f v) { return make_float2(v.x, v.y); }
    static __device__ __forceinline__ float2 hi(icm_v4f v) { return make_float2(v.z, v.w); }
    static __device__ __forceinline__ icm_v4f join(float2 a, float2 b) { icm_v4f r; r.x = a.x; r.y = a.y; r.z = b.x; r.w = b.y; return r; }
    static __device__ __forceinline__ icm_v4f sub(icm_v4f acc, float2 a, icm_v4f y)
    {
        return join(vsub(lo(acc), ic_mul(a, lo(y))), vsub(hi(acc), ic_mul(a, hi(y))));
    }
    // ic_div of one half, out of line.  Inlined into a piece's code the two halves' products are paired with each other, and the sums
    // inside c64_div are then contracted into other fused multiply-adds than in csr_tri.hip's kernels (re = fma(brs, ars, bis ais)
    // for their fma(ais, bis, ars brs)): one bit apart.  Compiled on its own, the division is the code it is there.
    static __device__ __noinline__ float2 div_half(float2 acc, float2 d) { return ic_div(acc, d); }
    static __device__ __forceinline__ icm_v4f div(icm_v4f acc, float2 d) { return join(div_half(lo(acc), d), div_half(hi(acc), d)); }
};
// vectors travel behind double pointers (TriFactor's); piece e of one
template <class T> __device__ __forceinline__ typename T::P icm_ld(const double *p, long e) { return reinterpret_cast<const typename T::P *>(p)[e]; }
template <class T> __device__ __forceinline__ void icm_st(double *p, long e, typename T::P v) { reinterpret_cast<typename T::P *>(p)[e] = v; }

// ------------------------------------------------------------------------------------------- sweeps
// K / 2 neighbouring lanes own the K / 2 16-byte pieces of one row: piece e = i * K / 2 + sub is lane e of the grid, so X, Y(j) and
// Y(j+1) are read and written coalesced, and one entry's gather of Y(j) is a single K * 8-byte access by those lanes.
template <class T, int K, int DG>
static __global__ __launch_bounds__(IC_MT) void k_ic_scale_multi(int n, const int *__restrict__ rowptr, const typename T::V *__restrict__ val,
                                                                const double *__restrict__ X, double *__restrict__ Y, const int *done)
{   // the first sweep, from Y = 0: Y = X / diag
    constexpr int K2 = K / 2;
    if (done && *done) return;
    const long e = (long)blockIdx.x * IC_MT + threadIdx.x;
    const long i = e / K2;
    if (i >= n) return;
    const typename T::P v = icm_ld<T>(X, e);
    icm_st<T>(Y, e, DG == 2 ? v : T::div(v, val[DG == 1 ? rowptr[i] : rowptr[i + 1] - 1]));
}

// k_ic_sweep's shape (csr_tri.hip), K wide: the workgroup's ic_mrows(K) consecutive rows own one contiguous slice of col / val,
// loaded 16 bytes per lane into the LDS window with every load issued before the first LDS store; then the K / 2 lanes of a row
// walk it out of LDS (the same word for all of them: a broadcast) with up to four gathers of Yin in flight per lane.  A slice
// that does not fit the window is walked out of global memory: the same sums.
template <class T, int K, int DG>
static __global__ __launch_bounds__(IC_MT) void k_ic_sweep_multi(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                                const typename T::V *__restrict__ val, const double *__restrict__ X,
                                                                const double *__restrict__ Yin, double *__restrict__ Yout, const int *done)
{
    constexpr int K2 = K / 2;
    constexpr int MR = ic_mrows(K);
    constexpr int NRND = IC_MCH / (IC_MT * 4);          // 4-entry units per lane
    constexpr int UNR = 4;                              // gathers of Yin in flight per lane
    typedef typename T::P P;
    typedef typename T::V V;
    static_assert(sizeof(V) == 8 && sizeof(P) == 16, "the window holds 8-byte values, a lane moves two of them at a time");
    __shared__ __attribute__((aligned(16))) V sval[IC_MCH];
    __shared__ __attribute__((aligned(16))) int scol[IC_MCH];
    if (done && *done) return;
    const int tid = threadIdx.x;
    const int sub = tid % K2, r = tid / K2;
    const int row0 = blockIdx.x * MR;
    const int nrows = min(MR, n - row0);
    const int base = rowptr[row0] & ~3;
    const int cnt = rowptr[row0 + nrows] - base;
    const int rsafe = r < nrows ? r : 0;
    const int rs = rowptr[row0 + rsafe], re = rowptr[row0 + rsafe + 1];
    const long piece = (long)(row0 + rsafe) * K2 + sub;
    P acc = icm_ld<T>(X, piece);
    const int b = DG == 1 ? rs + 1 : rs, f = DG == 0 ? re - 1 : re, dg = DG == 1 ? rs : re - 1;     // (dg is not read when DG == 2)
    if (cnt > IC_MCH) {                                 // (uniform over the workgroup)
        if (r >= nrows) return;
        for (int p = b; p < f; p++) acc = T::sub(acc, val[p], icm_ld<T>(Yin, (long)col[p] * K2 + sub));
        icm_st<T>(Yout, piece, DG == 2 ? acc : T::div(acc, val[dg]));
        return;
    }
    icm_v4i pc[NRND]; m2d pv[NRND * 2];
#pragma unroll
    for (int q = 0; q < NRND; q++) {
        const int u = tid * 4 + q * IC_MT * 4;
        // branch-free: lanes past the slice re-read its first unit.  col / val carry 64 bytes of slack (alloc_part), so the
        // slice's last unit may reach up to three entries past nnz.
        const long g = (long)base + (u < cnt ? u : 0);
        pc[q] = *reinterpret_cast<const icm_v4i *>(col + g);
        pv[q * 2] = reinterpret_cast<const m2d *>(val + g)[0];
        pv[q * 2 + 1] = reinterpret_cast<const m2d *>(val + g)[1];
    }
    __builtin_amdgcn_sched_barrier(0);                  // every load above every LDS store
#pragma unroll
    for (int q = 0; q < NRND; q++) {
        const int u = tid * 4 + q * IC_MT * 4;
        if (u < cnt) {
            *reinterpret_cast<icm_v4i *>(scol + u) = pc[q];
            reinterpret_cast<m2d *>(sval + u)[0] = pv[q * 2];
            reinterpret_cast<m2d *>(sval + u)[1] = pv[q * 2 + 1];
        }
    }
    __syncthreads();
    if (r >= nrows) return;
    int p = b - base;
    const int fe = f - base;
    for (; p + UNR <= fe; p += UNR) {
        V a[UNR]; P yv[UNR];
#pragma unroll
        for (int q = 0; q < UNR; q++) { a[q] = sval[p + q]; yv[q] = icm_ld<T>(Yin, (long)scol[p + q] * K2 + sub); }
#pragma unroll
        for (int q = 0; q < UNR; q++) acc = T::sub(acc, a[q], yv[q]);
    }
    {   // the row's last 0..3 entries, their gathers in flight together as well
        V a[UNR - 1]; P yv[UNR - 1];
        const int m = fe - p;
#pragma unroll
        for (int q = 0; q < UNR - 1; q++) if (q < m) { a[q] = sval[p + q]; yv[q] = icm_ld<T>(Yin, (long)scol[p + q] * K2 + sub); }
#pragma unroll
        for (int q = 0; q < UNR - 1; q++) if (q < m) acc = T::sub(acc, a[q], yv[q]);
    }
    icm_st<T>(Yout, piece, DG == 2 ? acc : T::div(acc, sval[dg - base]));
}

// ------------------------------------------------------------------------------------------- solves
// Row i of all K columns by one thread: K accumulators, the row's col / val read once.  Y is read (earlier levels) and written.
template <class T, int K, int DG>
struct TriSolveRowMulti {
    const int *rowptr, *col;
    const typename T::V *val;
    const double *x;
    double *y;
    __device__ __forceinline__ void operator()(int i) const
    {
        constexpr int K2 = K / 2;
        const int s = rowptr[i], e = rowptr[i + 1];
        const int b = DG == 1 ? s + 1 : s, f = DG == 0 ? e - 1 : e;
        typename T::P acc[K2];
#pragma unroll
        for (int q = 0; q < K2; q++) acc[q] = icm_ld<T>(x, (long)i * K2 + q);
        for (int p = b; p < f; p++) {
            const typename T::V a = val[p];
            const long c = (long)col[p] * K2;
#pragma unroll
            for (int q = 0; q < K2; q++) acc[q] = T::sub(acc[q], a, icm_ld<T>(y, c + q));
        }
        if (DG != 2) {
            const typename T::V d = val[DG == 1 ? s : e - 1];
#pragma unroll
            for (int q = 0; q < K2; q++) acc[q] = T::div(acc[q], d);
        }
#pragma unroll
        for (int q = 0; q < K2; q++) icm_st<T>(y, (long)i * K2 + q, acc[q]);
    }
};

// ------------------------------------------------------------------------------------------- apply
// s sweeps on one triangle, as tri_sweeps (csr_tri.hip): Y(1) = X / diag, then Y(j+1) from Y(j) between the factor's two k-wide
// sweep vectors; the last one writes Y.  A unit diagonal's first sweep is Y = X, which its second reads in place.
template <class T, int K, int DG>
static int tri_sweeps_multi(const TriFactor *F, const CsrPart &Tr, const double *X, double *Y, hipStream_t s, const int *done)
{
    const int sw = F->sweeps;
    if (F->n == 0) return 0;
    const dim3 grid((unsigned)((F->n + ic_mrows(K) - 1) / ic_mrows(K)));
    const typename T::V *val = reinterpret_cast<const typename T::V *>(Tr.val);
    double *const buf[2] = {F->mw[1], F->mw[2]};
    const double *in = X;
    if (DG != 2 || sw == 1) {
        double *out = sw == 1 ? Y : buf[0];
        hipLaunchKernelGGL((k_ic_scale_multi<T, K, DG>), grid, dim3(IC_MT), 0, s, F->n, Tr.rowptr, val, X, out, done);
        in = out;
    }
    for (int j = 2; j <= sw; j++) {
        double *out = j == sw ? Y : buf[in == buf[0] ? 1 : 0];
        hipLaunchKernelGGL((k_ic_sweep_multi<T, K, DG>), grid, dim3(IC_MT), 0, s, F->n, Tr.rowptr, Tr.col, val, X, in, out, done);
        in = out;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

template <class T, int K, int DG>
static int tri_multi_one(const TriFactor *F, bool up, const double *X, double *Y, hipStream_t s, const int *done)
{
    const CsrPart &Tr = up ? F->up : F->lo;
    if (F->sweeps > 0) return tri_sweeps_multi<T, K, DG>(F, Tr, X, Y, s, done);
    return run_levels(up ? F->bw : F->fw,
                      TriSolveRowMulti<T, K, DG>{Tr.rowptr, Tr.col, reinterpret_cast<const typename T::V *>(Tr.val), X, Y}, done, s);
}

template <class T, int K, int DGLO>
static int tri_multi(const TriFactor *F, int which, const double *X, double *Y, hipStream_t s, const int *done)
{
    if (which == 0) return tri_multi_one<T, K, DGLO>(F, false, X, Y, s, done);
    if (which == 1) return tri_multi_one<T, K, 1>(F, true, X, Y, s, done);
    const int rc = tri_multi_one<T, K, DGLO>(F, false, X, F->mw[0], s, done);
    return rc ? rc : tri_multi_one<T, K, 1>(F, true, F->mw[0], Y, s, done);
}

// X, Y: the block behind double pointers whatever its element type (a complex64 factor's blocks are float pairs)
int tri_apply_multi(const TriFactor *F, int k, int which, const double *X, double *Y, hipStream_t s, const int *done)
{
    if (F->dg[0] == 2)                                  // a unit lower triangle: ILU(0), real only
        return multi_k(k, [&](auto K) { return tri_multi<IcmReal, decltype(K)::value, 2>(F, which, X, Y, s, done); });
    if (F->c64) return multi_k(k, [&](auto K) { return tri_multi<IcmC64, decltype(K)::value, 0>(F, which, X, Y, s, done); });
    return multi_k(k, [&](auto K) { return tri_multi<IcmReal, decltype(K)::value, 0>(F, which, X, Y, s, done); });
}

// The k-wide work vectors an apply of `which` needs at the factor's sweeps setting: lo's result (which = 2) and, from two sweeps
// on, the two sweep vectors.  They are sized for the largest k seen so far; growing frees the smaller ones first (hipFree waits
// for the applies still on the stream).  A call that finds them there does nothing.
int tri_multi_reserve(TriFactor *F, int k, int which)
{
    const bool need[3] = {which == 2, F->sweeps >= 2, F->sweeps >= 2};
    if (k > F->mk) {
        for (double *&p : F->mw) { if (p) (void)hipFree(p); p = nullptr; }
        F->mk = k;
    }
    const size_t bytes = sizeof(double) * (size_t)std::max(F->n, 1) * (size_t)F->mk;
    for (int v = 0; v < 3; v++) {
        if (!need[v] || F->mw[v]) continue;
        if (hipMalloc(&F->mw[v], bytes) != hipSuccess) { F->mw[v] = nullptr; return fail(hipErrorOutOfMemory, "k-wide factor work vectors", __FILE__, __LINE__); }
    }
    return 0;
}

// c64: the complex64 entry (a block's element and column are 8 bytes either way)
static int solve_multi_entry(const char *entry, lcg_hip_csr *A, TriSlot slot, const char *builder, bool c64, int k, int which, const double *X,
                             double *Y)
{
    TRY(multi_args(entry, k, X, Y));
    TRY(c64 ? c64multi_handle(entry, A) : multi_handle(entry, A));
    const TriFactor *F = nullptr;
    TRY(tri_check(A, slot, entry, builder, false, c64, -1, which, X, nullptr, &F));
    const size_t bytes = sizeof(double) * (size_t)F->n * (size_t)k;
    if ((const char *)X < (const char *)Y + bytes && (const char *)Y < (const char *)X + bytes) return arg_error("%s: X and Y overlap", entry);
    TRY(ensure_init());
    TRY(tri_multi_reserve(A->*slot, k, which));
    return tri_apply_multi(F, k, which, X, Y, ctx().stream, nullptr);
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_ic0_solve_multi(lcg_hip_csr_t A, int k, int which, const double *X, double *Y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return solve_multi_entry("lcg_hip_ic0_solve_multi", A, &lcg_hip_csr::ic0, "lcg_hip_csr_build_ic0", false, k, which, X, Y);
}

int lcg_hip_ilu0_solve_multi(lcg_hip_csr_t A, int k, int which, const double *X, double *Y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return solve_multi_entry("lcg_hip_ilu0_solve_multi", A, &lcg_hip_csr::ilu0, "lcg_hip_csr_build_ilu0", false, k, which, X, Y);
}

int clcg_hip_ic0_solve_multi_c64(lcg_hip_csr_t A, int k, int which, const float *X, float *Y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return solve_multi_entry("clcg_hip_ic0_solve_multi_c64", A, &lcg_hip_csr::ic0, "lcg_hip_csr_build_ic0_c64", true, k, which,
                             reinterpret_cast<const double *>(X), reinterpret_cast<double *>(Y));
}

} // extern "C"
