// multi.hpp -- what the k-wide products (csr_multi.hip, csr_multi_cplx.hip, dense_multi.hip, dense_multi_cplx.hip) and the batched loops
// (solvers_multi*.hip) share: the checks of a block of vectors, the dispatch over k, the frame of the CSR products, the fold of their
// partial sums and the read-out of a *_dot entry, each defined once in csr_multi.hip.  Not installed.
//
// A block of k vectors is ONE array of n * k doubles, row-major: X[i * k + j] is row i of column j (k = 2, 4, 8; the base
// 16-byte aligned, so a row is k / 2 aligned 16-byte pieces).  DESIGN.md section 15.
#pragma once

#include "driver.hpp"

namespace lcgh {

constexpr int MM_MG = 512;      // most partial sums per running sum a consumer adds up = stride of the k-wide tables
constexpr int MM_MAXK = 8;

typedef double m2d __attribute__((ext_vector_type(2)));

// k in {2, 4, 8}, no null pointer, every base 16-byte aligned: decided BEFORE the device is touched (0, or LCG_HIP_E_ARG with
// lcg_hip_last_error() naming the entry and the reason)
int multi_args(const char *entry, int k, const void *a, const void *b, const void *c = (const void *)16);
// a CSR handle this path serves: real fp64, whole (not sharded), not dense (0, or LCG_HIP_E_ARG with the text)
int multi_handle(const char *entry, const lcg_hip_csr *A);

// the byte ranges [a, a + na) and [b, b + nb) meet
bool overlap(const void *a, size_t na, const void *b, size_t nb);

// f(std::integral_constant<int, k>) for the k that multi_args has let through; the same for the R = 64, 16, 4 rows of a block
template <class F> int multi_k(int k, F f)
{
    if (k == 2) return f(std::integral_constant<int, 2>{});
    if (k == 4) return f(std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 8>{});
}
template <class F> int multi_r(int R, F f)
{
    if (R == 64) return f(std::integral_constant<int, 64>{});
    if (R == 16) return f(std::integral_constant<int, 16>{});
    return f(std::integral_constant<int, 4>{});
}

// The frame of the k-wide CSR products, real and complex (csr_multi.hip).  `go` launches the product kernel for R rows per block:
// Y = A.X for the k columns in one launch (P's plain CSR arrays: no plan is built or used) and, with U, one partial sum per block
// and table row at part[row * pstride + block].  A column owns `tab` table rows: 1 (real: (A.X)_j . U_j), 2 (real with dot2: besides it
// (A.X)_j . (A.X)_j in rows k ..; complex: re, im of one sum in rows 2 j, 2 j + 1), 3 (complex with a real second sum in rows 2 k ..: multi_cplx.hpp).  multi_launch leaves every row's sum
// as *slots <= MM_MG partial sums at dots[row * MM_MG ...], to be added in index order; `big` holds the per-block sums of a matrix with
// more than MM_MG row blocks on their way there (multi_big_doubles(P, tab * k) doubles; may be null where that is 0).
typedef void (*MultiGo)(const CsrPart &P, int k, int R, const double *X, double *Y, hipStream_t s, const int *done, bool wide,
                        const double *U, double *part, int pstride, int tab);
int multi_launch(const CsrPart &P, int k, int tab, MultiGo go, const double *X, double *Y, hipStream_t s, const int *done, const double *U,
                 double *big, double *dots, int *slots);
size_t multi_big_doubles(const CsrPart &P, int ns);
// what a *_spmm_dot* entry does after its checks: work memory for big, multi_launch, multi_dots_read, free
int multi_dot_run(const CsrPart &P, int k, int tab, MultiGo go, const double *X, double *Y, const double *U, double *dots);
// out[row * MM_MG + f] = the sum of big[row * nb + f * per ...], per consecutive partial sums in order, for ns table rows; the nf <= MM_MG
// sums per row it leaves
int multi_fold_launch(const double *big, int nb, int ns, double *out, hipStream_t s);
// dots[0 .. ns) = the ns running sums of the loops' table c.partials_pair[0], `slots` partial sums each, added by msum (ns = 2, 4, 8,
// 16; 6, 12, 24 with three table rows per column): launch, copy to the host, wait.  0, or the failure's code
int multi_dots_read(Ctx &c, int ns, int slots, double *dots);

// the real product: with U column j's (A.X)_j . U_j, with dot2 besides it (A.X)_j . (A.X)_j, the first sum's bits unchanged
int spmm_launch(const CsrPart &P, int k, const double *X, double *Y, hipStream_t s, const int *done, const double *U = nullptr,
                double *big = nullptr, double *dots = nullptr, int *slots = nullptr, bool dot2 = false);
inline size_t spmm_big_doubles(const CsrPart &P, int k, bool dot2 = false) { return multi_big_doubles(P, dot2 ? 2 * k : k); }

// Sum the g <= MM_MG partials of each of NS running sums (table row r = pin + r * MM_MG) into sums[r] (LDS), the whole block taking
// part: per lane its partials in index order, the lanes by wave_sum, the wavefronts in order -- the same bits wherever and
// however often this runs.  Ends with a barrier.
template <int NS>
__device__ __forceinline__ void msum(const double *pin, int g, double *sums)
{
    constexpr int PER = MM_MG / VB;
    __shared__ double sh[NS][VB / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll 8
    for (int r = 0; r < NS; r++) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int j = threadIdx.x + q * VB;
            const double x = pin[r * MM_MG + (j < g ? j : 0)];      // branch-free: select after the load
            t += j < g ? x : 0.0;
        }
        t = wave_sum(t);
        if (lane == WSUM_LANE) sh[r][w] = t;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < VB / 64; q++) t += sh[threadIdx.x][q];
        sums[threadIdx.x] = t;
    }
    __syncthreads();
}

// The same sums as ONE binary tree over the table's MM_MG slots, adjacent slots first (g <= MM_MG partials, the rest read as +0):
// a lane adds its 8 consecutive slots pairwise, the lanes meet by xor 1, 2, 4, ... 32, one wavefront per running sum.  Partials that
// are themselves such trees over 2^m consecutive leaves (k_mvecf's TREE passes) add up to the tree over all leaves, however many
// leaves a partial holds: what lets a column's sums not depend on k.  Ends with a barrier.
template <int NS>
__device__ __forceinline__ void msum_tree(const double *pin, int g, double *sums)
{
    static_assert(MM_MG == 64 * 8, "eight slots per lane");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int r = w; r < NS; r += VB / 64) {
        double x[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int j = 8 * lane + q;
            const double v = pin[r * MM_MG + (j < g ? j : 0)];      // branch-free: select after the load
            x[q] = j < g ? v : 0.0;
        }
        double t = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) t += __shfl_xor(t, off, 64);
        if (lane == 0) sums[r] = t;
    }
    __syncthreads();
}

// the leaves of a TREE pass: rows i, i + S, i + 2 S, ... share leaf i mod S.  S depends on n alone, so a thread's leaf does not
// depend on k; with g lanes to a row the pass runs S * g / VB workgroups, at most MM_MG with the widest row's gmax lanes (k = 8: 4 for
// real blocks, 8 for complex ones)
inline long tree_leaves(long n, int gmax)
{
    long s = 256;
    while (s < n && s < MM_MG * VB / gmax) s <<= 1;
    return s;
}

} // namespace lcgh
