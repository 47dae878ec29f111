// csr_normal.hip -- sparse least squares on a rectangular real fp64 CSR handle K (M x N, one GPU): K^T.x, K^T.(K.x), their k-wide
// forms and the Jacobi reciprocals of K^T.K (include/lcg_hip_staging_csr_normal.h).  The batched loops on K^T.K are entries of
// solvers_multi.hip and solvers_multi_box.hip, which reach this state through CsrNormalOp (multi_ops.hpp).
//
// An application of K^T.K is two products of the kernels the library has: t = K.x over the handle's arrays, y = K^T.t over a
// materialised K^T (spmv_launch / spmm_launch on each part, so each part chooses its own kernel family and every product is the same
// bits from call to call).  A scatter form of K^T.t would need atomics and is not offered.  What is new here is the build:
//
//   K^T = a stable sort of K's entries by column.  Entry k of K (its offset in col / val) goes to row col[k] of K^T; inside a row the
//   entries stand in ascending k -- by source row, and entries of equal (row, column) in K's own entry order.  The keys of a row are
//   distinct integers, so the order does not depend on the values (NaN, -0.0 included) or on anything but the matrix: the same arrays
//   bit for bit on every build.
//     1. k_nm_count     column counts (integer atomics: the result does not depend on their order); a column index outside
//                       [0, N) raises a flag and nothing else is done with this matrix
//     2. the device scan -> K^T's rowptr
//     3. k_nm_place     entry k into a slot of its row, slots handed out by atomics (arbitrary order inside a row)
//     4. the sort of every row's slots, ascending:
//          rows of <= NM_SHORT entries   k_perm_sort, one thread per row (the COO ingest's kernel)
//          longer rows                   cut into chunks of NM_CH entries (k_nm_items); k_nm_sort_chunk sorts a chunk in LDS, one
//                                        workgroup per chunk (bitonic network over the next power of two, padded with INT_MAX)
//          rows of > NM_CH entries       k_nm_merge: passes of width NM_CH, 2 NM_CH, ... between the slot array and a second one; an
//                                        element finds its place in the merged pair of runs by a binary search in the partner run
//        A column of L entries costs L log2(min(L, NM_CH))^2 / 2 compare-exchanges in LDS plus L log2(L) steps per merge pass,
//        log2(L / NM_CH) passes: for long columns the cost grows like L log L, not like L^2.
//     5. k_nm_gather    K^T's col (the source row of entry k, by binary search in K's rowptr) and val (val[k])
//
//   diag(K^T.K)_c = sum_i K(i,c)^2 = the sum of squares of row c of K^T, one wavefront per row: lane l adds entries l, l + 64, ... in
//   order, the lanes meet by wave_sum -- a fixed order (k_nm_diag).
#include <chrono>

#include "multi.hpp"
#include "csr_normal.hpp"

namespace lcgh {

constexpr int NM_SHORT = 32;        // rows of K^T up to this length: one thread per row
constexpr int NM_CH = 8192;         // entries a workgroup sorts in LDS (32 KB of keys)

// ctr[0]: a column outside [0, ncols); ctr[1]: chunks listed by k_nm_items; ctr[2]: the longest row of K^T
__global__ void k_nm_count(long nnz, int ncols, const int *__restrict__ col, int *cnt, int *ctr)
{
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (long)gridDim.x * blockDim.x) {
        const int c = col[k];
        if (c < 0 || c >= ncols) ctr[0] = 1; else atomicAdd(&cnt[c], 1);
    }
}
__global__ void k_nm_place(long nnz, const int *__restrict__ col, const int *__restrict__ rpT, int *next, int *perm)
{   // (every column has passed k_nm_count's test)
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (long)gridDim.x * blockDim.x) {
        const int c = col[k];
        perm[rpT[c] + atomicAdd(&next[c], 1)] = (int)k;
    }
}
// the chunks of the rows that k_perm_sort leaves alone: items[] = (row, chunk); their order in the list decides nothing
__global__ void k_nm_items(int n, const int *__restrict__ rpT, int2 *items, int *ctr)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int len = rpT[c + 1] - rpT[c];
    atomicMax(&ctr[2], len);
    if (len <= NM_SHORT) return;
    const int nch = (len + NM_CH - 1) / NM_CH;
    const int base = atomicAdd(&ctr[1], nch);
    for (int q = 0; q < nch; q++) items[base + q] = make_int2(c, q);
}
__global__ __launch_bounds__(VB) void k_nm_sort_chunk(const int2 *__restrict__ items, const int *__restrict__ rpT, int *perm)
{
    __shared__ int sh[NM_CH];
    const int2 it = items[blockIdx.x];
    const int s = rpT[it.x] + it.y * NM_CH;
    const int cnt = min(NM_CH, rpT[it.x + 1] - s);
    int P = 2;
    while (P < cnt) P <<= 1;                        // (<= NM_CH, a power of two)
    for (int i = threadIdx.x; i < P; i += VB) sh[i] = i < cnt ? perm[s + i] : 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += VB) {
                const int p = i ^ j;
                if (p > i) {
                    const int a = sh[i], b = sh[p];
                    if ((a > b) == ((i & k) == 0)) { sh[i] = b; sh[p] = a; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < cnt; i += VB) perm[s + i] = sh[i];
}
// one pass over the rows of more than NM_CH entries: sorted runs of w entries merge pairwise from src into dst (a last run without a
// partner is copied).  The keys of a row are distinct: an element's place is its index in its own run plus the partner's elements below it.
__global__ __launch_bounds__(VB) void k_nm_merge(const int2 *__restrict__ items, const int *__restrict__ rpT, const int *__restrict__ src,
                                                 int *__restrict__ dst, long w)
{
    const int2 it = items[blockIdx.x];
    const int base = rpT[it.x], len = rpT[it.x + 1] - base;
    if (len <= NM_CH) return;
    const int i0 = it.y * NM_CH, i1 = min(len, i0 + NM_CH);
    const int *row = src + base;
    for (int i = i0 + threadIdx.x; i < i1; i += VB) {
        const int key = row[i];
        const long r = i / w;
        const long own0 = r * w, pair0 = (r & ~1L) * w;
        long lo = (r ^ 1L) * w, hi = lo + w < len ? lo + w : len;
        long rank = 0;
        if (lo < len) {
            const long p0 = lo;
            while (lo < hi) { const long mid = (lo + hi) >> 1; if (row[mid] < key) lo = mid + 1; else hi = mid; }
            rank = lo - p0;
        }
        dst[base + pair0 + (i - own0) + rank] = key;
    }
}
// largest i in [0, n) with ptr[i] <= v (ptr ascending, ptr[0] <= v < ptr[n]): the row that holds offset v, empty rows skipped
__device__ __forceinline__ int nm_row_of(const int *__restrict__ ptr, int n, int v)
{
    int lo = 0, hi = n;                 // invariant: ptr[lo] <= v < ptr[hi]
    while (hi - lo > 1) { const int mid = (int)(((long)lo + hi) >> 1); if (ptr[mid] <= v) lo = mid; else hi = mid; }
    return lo;
}
__global__ void k_nm_gather(long nnz, int nt, int n, const int *__restrict__ rpT, const int *__restrict__ rowptr, const int *__restrict__ perm,
                            const int *__restrict__ merged, const double *__restrict__ val, int *__restrict__ colT, double *__restrict__ valT)
{   // merged: where the rows of more than NM_CH entries ended up after an odd number of passes (else null)
    for (long pos = (long)blockIdx.x * blockDim.x + threadIdx.x; pos < nnz; pos += (long)gridDim.x * blockDim.x) {
        const int *from = perm;
        if (merged) {
            const int c = nm_row_of(rpT, nt, (int)pos);
            if (rpT[c + 1] - rpT[c] > NM_CH) from = merged;
        }
        const int k = from[pos];
        colT[pos] = nm_row_of(rowptr, n, k);
        valT[pos] = val[k];
    }
}
// d[c] = the sum of squares of row c of K^T, one wavefront per row
__global__ __launch_bounds__(VB) void k_nm_diag(int nt, const int *__restrict__ rpT, const double *__restrict__ valT, double *__restrict__ d)
{
    const int c = blockIdx.x * (VB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= nt) return;                // (uniform over the wavefront)
    double t = 0.0;
    for (int k = rpT[c] + lane; k < rpT[c + 1]; k += 64) t = fma(valT[k], valT[k], t);
    t = wave_sum(t);
    if (lane == WSUM_LANE) d[c] = t;
}
__global__ void k_nm_mul(long n, const double *__restrict__ a, const double *__restrict__ x, double *__restrict__ z)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) z[i] = a[i] * x[i];
}

// K^T of A->main into N->T (which holds nothing).  Drains the stream.
static int build_transpose(lcg_hip_csr *A, CsrNormal *N)
{
    const auto t0 = std::chrono::steady_clock::now();
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int n = A->n_rows, nt = A->n_cols;
    const long nnz = A->main.nnz;
    const CsrPart &P = A->main;
    int *cnt = nullptr, *ctr = nullptr, *perm = nullptr, *tmp = nullptr;
    int2 *items = nullptr;
    CsrPart T;
    auto done = [&](int rc) {
        if (cnt) (void)hipFree(cnt); if (ctr) (void)hipFree(ctr); if (perm) (void)hipFree(perm); if (tmp) (void)hipFree(tmp);
        if (items) (void)hipFree(items);
        if (rc) free_part(T);
        return rc;
    };
#define NM_CHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return done(fail(e_, #call, __FILE__, __LINE__)); } while (0)
    NM_CHK(hipMalloc(&cnt, sizeof(int) * (size_t)nt));
    NM_CHK(hipMalloc(&ctr, sizeof(int) * 4));
    NM_CHK(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)nt, s));
    NM_CHK(hipMemsetAsync(ctr, 0, sizeof(int) * 4, s));
    int h[4] = {0, 0, 0, 0};
    if (nnz > 0) {
        hipLaunchKernelGGL(k_nm_count, dim3(1024), dim3(VB), 0, s, nnz, nt, P.col, cnt, ctr);
        NM_CHK(hipGetLastError());
        NM_CHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, s));
        NM_CHK(hipStreamSynchronize(s));
        if (h[0]) return done(arg_error("lcg_hip_csr_build_normal: a column index lies outside [0, %d)", nt));
    }
    { int rc = alloc_part(T, nt, nnz, false); if (rc) return done(rc); }
    T.n_cols = n;
    long total = 0;
    { int rc = device_exclusive_scan(nt, cnt, T.rowptr, s, &total); if (rc) return done(rc); }
    if (total != nnz) return done(fail(hipErrorUnknown, "normal state: column counts", __FILE__, __LINE__));
    if (nnz > 0) {
        NM_CHK(hipMalloc(&perm, sizeof(int) * (size_t)nnz));
        NM_CHK(hipMalloc(&items, sizeof(int2) * ((size_t)nnz / NM_SHORT + 2)));     // <= nnz / NM_CH + (rows longer than NM_SHORT) chunks
        NM_CHK(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)nt, s));
        hipLaunchKernelGGL(k_nm_place, dim3(1024), dim3(VB), 0, s, nnz, P.col, T.rowptr, cnt, perm);
        hipLaunchKernelGGL(k_nm_items, dim3((unsigned)((nt + VB - 1) / VB)), dim3(VB), 0, s, nt, T.rowptr, items, ctr);
        perm_sort_launch(nt, T.rowptr, perm, NM_SHORT, s);
        NM_CHK(hipGetLastError());
        NM_CHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, s));
        NM_CHK(hipStreamSynchronize(s));
        const int nitems = h[1], longest = h[2];
        const int *merged = nullptr;
        if (nitems > 0) {
            hipLaunchKernelGGL(k_nm_sort_chunk, dim3((unsigned)nitems), dim3(VB), 0, s, items, T.rowptr, perm);
            if (longest > NM_CH) {
                NM_CHK(hipMalloc(&tmp, sizeof(int) * (size_t)nnz));
                int *src = perm, *dst = tmp;
                for (long w = NM_CH; w < longest; w *= 2) {
                    hipLaunchKernelGGL(k_nm_merge, dim3((unsigned)nitems), dim3(VB), 0, s, items, T.rowptr, src, dst, w);
                    std::swap(src, dst);
                }
                if (src == tmp) merged = tmp;
            }
        }
        hipLaunchKernelGGL(k_nm_gather, dim3(1024), dim3(VB), 0, s, nnz, nt, n, T.rowptr, P.rowptr, perm, merged, P.val, T.col, T.val);
        NM_CHK(hipGetLastError());
        NM_CHK(hipStreamSynchronize(s));
        N->longest = longest;
    } else
        N->longest = 0;
#undef NM_CHK
    N->T = T;
    N->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return done(0);
}

// d = the sums of squares of K^T's rows; the reciprocals into N->invdiag when every one is a positive finite number, else LCG_HIP_E_ARG
// naming the first column that is not, with nothing stored
static int build_reciprocals(lcg_hip_csr *A, CsrNormal *N, double *diag_out)
{
    Ctx &c = ctx();
    const int nt = A->n_cols;
    double *d = nullptr;
    HIPCHK(hipMalloc(&d, sizeof(double) * (size_t)nt));
    std::vector<double> h((size_t)nt);
    hipLaunchKernelGGL(k_nm_diag, dim3((unsigned)((nt + VB / 64 - 1) / (VB / 64))), dim3(VB), 0, c.stream, nt, N->T.rowptr, N->T.val, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, sizeof(double) * (size_t)nt, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) { (void)hipFree(d); return fail(e, "normal diagonal", __FILE__, __LINE__); }
    for (int i = 0; i < nt; i++)
        if (!(h[i] > 0.0) || !std::isfinite(h[i])) {
            (void)hipFree(d);
            return arg_error("lcg_hip_csr_build_jacobi_normal: column %d of K has the sum of squares %g: no datum sees this parameter "
                             "and K^T.K is singular", i, h[i]);
        }
    if (diag_out) e = hipMemcpyAsync(diag_out, d, sizeof(double) * (size_t)nt, hipMemcpyDeviceToDevice, c.stream);
    for (int i = 0; i < nt; i++) h[i] = 1.0 / h[i];
    if (e == hipSuccess && !N->invdiag) e = hipMalloc(&N->invdiag, sizeof(double) * (size_t)nt);
    if (e == hipSuccess) e = hipMemcpyAsync(N->invdiag, h.data(), sizeof(double) * (size_t)nt, hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(e, "normal reciprocals", __FILE__, __LINE__);
    return 0;
}

void normal_free(lcg_hip_csr *A)
{
    CsrNormal *N = A->normal;
    if (!N) return;
    free_part(N->T);
    if (N->t) (void)hipFree(N->t);
    if (N->tk) (void)hipFree(N->tk);
    if (N->invdiag) (void)hipFree(N->invdiag);
    delete N;
    A->normal = nullptr;
}

void normal_stale(lcg_hip_csr *A) { if (A->normal) A->normal->stale = true; }

// a stale state: K^T again from the arrays as they are now, and the reciprocals if there were any
static int normal_refresh(lcg_hip_csr *A)
{
    CsrNormal *N = A->normal;
    if (!N->stale) return 0;
    HIPCHK(hipDeviceSynchronize());
    free_part(N->T);
    TRY(build_transpose(A, N));
    N->stale = false;
    if (N->invdiag) {
        const int rc = build_reciprocals(A, N, nullptr);
        if (rc) { (void)hipFree(N->invdiag); N->invdiag = nullptr; return rc; }
    }
    return 0;
}

int normal_kind(const char *entry, const lcg_hip_csr *K)
{
    if (dense_handle(K)) return refuse_dense(entry);
    if (!K) return 0;
    if (K->c64) return arg_error("%s: the matrix holds complex64 values; the normal equations serve real fp64 matrices", entry);
    if (K->is_complex) return arg_error("%s: the matrix is complex; the normal equations serve real fp64 matrices", entry);
    if (K->distributed) return arg_error("%s: the matrix's rows are sharded (lcg_hip_csr_distribute); the normal equations serve whole matrices on one GPU", entry);
    return 0;
}

int normal_ready(const char *entry, lcg_hip_csr *K, bool need_state)
{
    TRY(normal_kind(entry, K));
    TRY(ensure_init());
    if (!K) return arg_error("%s: the handle is null", entry);
    if (!need_state) return 0;
    if (!K->normal) return arg_error("%s: the handle has no normal state: call lcg_hip_csr_build_normal first", entry);
    return normal_refresh(K);
}

int normal_reserve(lcg_hip_csr *K, int k)
{
    CsrNormal *N = K->normal;
    if (k <= N->kmax) return 0;
    if (N->kmax) HIPCHK(hipStreamSynchronize(ctx().stream));
    if (N->tk) (void)hipFree(N->tk);
    N->tk = nullptr; N->kmax = 0;
    HIPCHK(hipMalloc(&N->tk, sizeof(double) * (size_t)K->n_rows * k));
    N->kmax = k;
    return 0;
}

// y[N] = K^T.t, t[M] = K.x: the single-vector launches, both under the flag the built-in products honour
static int normal_kx(lcg_hip_csr *K, const double *x, double *t)
{
    Ctx &c = ctx();
    return spmv_launch(K->main, false, K->variant, K->mean_row, x, t, false, c.stream, ax_flag(c));
}
static int normal_ktx(lcg_hip_csr *K, const double *t, double *y)
{
    Ctx &c = ctx();
    const CsrPart &T = K->normal->T;
    return spmv_launch(T, false, 0, T.n_rows > 0 ? (double)T.nnz / T.n_rows : 0.0, t, y, false, c.stream, ax_flag(c));
}

static void nm_park(int rc) { if (rc && !ctx().ax_rc) ctx().ax_rc = rc; }

// the k-wide entries: Y = K^T.X (two = false) or K^T.(K.X); dot: column j's Y_j . U_j into dots[j]
static int normal_multi(const char *entry, lcg_hip_csr *K, int k, const double *X, double *Y, bool two, bool dot, const double *U, double *dots)
{
    TRY(normal_kind(entry, K));
    TRY(multi_args(entry, k, X, Y, dot ? (const void *)U : (const void *)16));
    if (dot && !dots) return arg_error("%s: the result array is a null pointer", entry);
    TRY(normal_ready(entry, K));
    Ctx &c = ctx();
    CsrNormal *N = K->normal;
    const double *in = X;
    if (two) {
        TRY(normal_reserve(K, k));
        TRY(spmm_launch(K->main, k, X, N->tk, c.stream, nullptr));
        in = N->tk;
    }
    if (!dot) return spmm_launch(N->T, k, in, Y, c.stream, nullptr);
    // (outside a solve the k-wide table of the loops is free: partials_pair[0] holds the partial sums, ax_partials the results)
    double *big = nullptr;
    const size_t nbig = spmm_big_doubles(N->T, k);
    if (nbig) HIPCHK(hipMalloc(&big, sizeof(double) * nbig));
    int slots = 0;
    int rc = spmm_launch(N->T, k, in, Y, c.stream, nullptr, U, big, c.partials_pair[0], &slots);
    if (!rc) rc = multi_dots_read(c, k, slots, dots);
    if (big) { (void)hipStreamSynchronize(c.stream); (void)hipFree(big); }
    return rc;
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_csr_cols(lcg_hip_csr_t A) { NOT_DENSE(A, LCG_HIP_E_ARG); return A ? A->n_cols : 0; }

int lcg_hip_csr_build_normal(lcg_hip_csr_t K)
{
    static const char *entry = "lcg_hip_csr_build_normal";
    TRY(normal_ready(entry, K, false));
    if (K->n_cols <= 0) return arg_error("%s: the matrix has %d columns", entry, K->n_cols);
    if (K->normal) return normal_refresh(K);
    CsrNormal *N = new CsrNormal;
    int rc = build_transpose(K, N);
    if (!rc && hipMalloc(&N->t, sizeof(double) * (size_t)K->n_rows) != hipSuccess) {
        rc = fail(hipErrorOutOfMemory, "normal state: the intermediate vector", __FILE__, __LINE__);
        free_part(N->T);
    }
    if (rc) { delete N; return rc; }
    K->normal = N;
    return 0;
}

int lcg_hip_csr_normal_info(lcg_hip_csr_t K, int *longest_column, int64_t *extra_bytes, double *build_ms)
{
    TRY(normal_ready("lcg_hip_csr_normal_info", K));
    const CsrNormal *N = K->normal;
    if (longest_column) *longest_column = N->longest;
    if (extra_bytes)
        *extra_bytes = 4 * ((int64_t)K->n_cols + 1) + 12 * std::max<int64_t>(N->T.nnz, 1) + 128 + 8 * (int64_t)K->n_rows * (1 + N->kmax)
                       + (N->invdiag ? 8 * (int64_t)K->n_cols : 0);
    if (build_ms) *build_ms = N->build_ms;
    return 0;
}

int lcg_hip_csr_normal_arrays(lcg_hip_csr_t K, const int **rowptr, const int **col, const double **val)
{
    TRY(normal_ready("lcg_hip_csr_normal_arrays", K));
    const CsrPart &T = K->normal->T;
    if (rowptr) *rowptr = T.rowptr;
    if (col) *col = T.col;
    if (val) *val = T.val;
    return 0;
}

int lcg_hip_spmv_t(lcg_hip_csr_t K, const double *x, double *y)
{
    static const char *entry = "lcg_hip_spmv_t";
    TRY(normal_kind(entry, K));
    if (!x || !y) return arg_error("%s: x or y is NULL", entry);
    TRY(normal_ready(entry, K));
    return normal_ktx(K, x, y);
}

// lcg_hip_csr_ata and its callback form, each under its own name
static int ata_entry(const char *entry, lcg_hip_csr *K, const double *x, double *y, const int *n_size = nullptr)
{
    TRY(normal_kind(entry, K));
    if (n_size && K && *n_size != K->n_cols) return arg_error("%s: n_size = %d, the matrix has %d columns", entry, *n_size, K->n_cols);
    if (!x || !y) return arg_error("%s: x or y is NULL", entry);
    TRY(normal_ready(entry, K));
    TRY(normal_kx(K, x, K->normal->t));
    return normal_ktx(K, K->normal->t, y);
}

int lcg_hip_csr_ata(lcg_hip_csr_t K, const double *x, double *y) { return ata_entry("lcg_hip_csr_ata", K, x, y); }

void lcg_hip_csr_ata_ax(void *instance, const double *x, double *prod_Ax, const int n_size)
{
    static const char *entry = "lcg_hip_csr_ata_ax";
    lcg_hip_csr *K = static_cast<lcg_hip_csr *>(instance);
    const int rc = ata_entry(entry, K, x, prod_Ax, &n_size);
    if (!rc && ctx().in_solve) ctx().cnt_ax++;      // (the loop has counted one product for this call: this is the second)
    nm_park(rc);
}

int lcg_hip_csr_build_jacobi_normal(lcg_hip_csr_t K, double *diag_out)
{
    TRY(normal_ready("lcg_hip_csr_build_jacobi_normal", K));
    return build_reciprocals(K, K->normal, diag_out);
}

void lcg_hip_csr_jacobi_normal_mx(void *instance, const double *x, double *prod_Mx, const int n_size)
{
    static const char *entry = "lcg_hip_csr_jacobi_normal_mx";
    lcg_hip_csr *K = static_cast<lcg_hip_csr *>(instance);
    int rc = normal_kind(entry, K);
    if (!rc && K && n_size != K->n_cols) rc = arg_error("%s: n_size = %d, the matrix has %d columns", entry, n_size, K->n_cols);
    if (!rc) rc = normal_ready(entry, K);
    if (!rc && !K->normal->invdiag) rc = arg_error("%s: lcg_hip_csr_build_jacobi_normal was not called", entry);
    if (!rc) {
        hipLaunchKernelGGL(k_nm_mul, dim3(grid_for(n_size)), dim3(VB), 0, ctx().stream, (long)n_size, K->normal->invdiag, x, prod_Mx);
        rc = launched("normal Jacobi");
    }
    nm_park(rc);
}

int lcg_hip_spmm_t(lcg_hip_csr_t K, int k, const double *X, double *Y)
{
    return normal_multi("lcg_hip_spmm_t", K, k, X, Y, false, false, nullptr, nullptr);
}

int lcg_hip_csr_ata_multi(lcg_hip_csr_t K, int k, const double *X, double *Y)
{
    return normal_multi("lcg_hip_csr_ata_multi", K, k, X, Y, true, false, nullptr, nullptr);
}

int lcg_hip_csr_ata_multi_dot(lcg_hip_csr_t K, int k, const double *X, double *Y, const double *U, double *dots)
{
    return normal_multi("lcg_hip_csr_ata_multi_dot", K, k, X, Y, true, true, U, dots);
}

} // extern "C"
