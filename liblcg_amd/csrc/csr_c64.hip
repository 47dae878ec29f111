// csr_c64.hip -- complex64 matrices: the handle, y = op(A).x summed in fp32, and the Jacobi reciprocals.
//
// The values are interleaved (re, im) floats (cuComplex, std::complex<float>): 8 bytes per entry, so a CSR entry costs 12 bytes of
// stream where a c128 entry costs 20.  The handle keeps them in main.val (8 bytes per entry, the size of a real matrix's value
// array) with is_complex = false and c64 = true; every entry that serves fp64 / c128 matrices refuses such a handle
// (internal.hpp: refuse_c64).
//
// Products (clcg_cudaf.cu's cusparseSpMV with CUDA_C_32F, sample14.cu): two kernels, chosen once per matrix at its first product.
//  k_c64_rows<W>  W lanes per row (W = the power of two that covers a mean row's pairs of entries); each lane takes PAIRS of entries
//                 (2p, 2p + 1) on absolute entry indices: one 16-byte load of values and one 8-byte load of columns per two entries,
//                 both gathers of x issued together, the half of a pair outside its row masked by selects (no branch:
//                 global_load_dwordx4 + global_load_dwordx2 + two global_load_dwordx2 per pair on gfx950).  Rows longer than `long_min` entries are left to
//  k_c64_long     one workgroup per long row (256 lanes over its pairs), so that one dense row does not hold up a block of short ones.
// Every lane sums its entries in entry order with fp32 fma; the lanes of a row are added in a fixed butterfly, the waves of a long
// row in wave order: the same bits from call to call.
// op(A) for layout / conjugate (A^T, A^H, conj(A)) is its own CSR, built on the device at its first use: the transpose is
// transpose_launch's 8-byte instantiation moving the float pairs as opaque 8-byte words (its (column, value) sort breaks ties of
// duplicate entries on those words: a fixed order unless an imaginary part is Inf / NaN), conjugation flips the imaginary signs.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "internal.hpp"
#include "c64common.hpp"

namespace lcgh {

struct C64Plan {            // one op(A)'s product
    int state = 0;          // 0 not planned, 1 ready
    int lanes = 1;          // W of k_c64_rows
    int long_min = INT_MAX; // rows with more entries go to k_c64_long
    int n_long = 0;
    int *long_rows = nullptr;
    bool pairs = false;     // pair loads: values 16-byte and columns 8-byte aligned, the entry behind the last one readable
    std::string name;       // what lcg_hip_csr_last_kernel reports
};
struct C64Data {
    C64Plan plan[4];        // [0] A, [1] conj(A), [2] A^T, [3] A^H (parts: A->main, A->op[1..3])
    float2 *invdiag = nullptr;
};
static C64Data *c64_of(lcg_hip_csr *A)
{
    if (!A->c64p) A->c64p = new C64Data();
    return static_cast<C64Data *>(A->c64p);
}

__device__ __forceinline__ void c64_mac(float &ax, float &ay, float2 v, float2 x)      // (ax, ay) += v * x, fixed fma order
{
    ax = fmaf(v.x, x.x, ax); ax = fmaf(-v.y, x.y, ax);
    ay = fmaf(v.x, x.y, ay); ay = fmaf(v.y, x.x, ay);
}

// one lane's share of row [s, e): entries s + lane, s + lane + W, ... (PAIRS: pairs p = s/2 + lane, ... of absolute indices).
// A pair is read whole -- one 16-byte load of values, one 8-byte load of columns -- before anything is decided about its two
// entries; an entry outside the row (the straddling pair's other half) is masked by selects: its gather reads x[0] and both its
// factors become 0, so it adds an exact zero.  Reading a whole pair needs the entry behind the last one to be readable: the
// plan takes this path only for padded arrays or an even entry count (c64_plan).
template <bool PAIRS>
__device__ __forceinline__ void c64_row_part(int s, int e, int lane, int W, const int *__restrict__ col, const float2 *__restrict__ val,
                                             const float2 *__restrict__ x, float &ax, float &ay)
{
    const float2 z = make_float2(0.f, 0.f);
    if (PAIRS) {
        for (long p = (long)(s >> 1) + lane; 2 * p < e; p += W) {
            const long k0 = 2 * p;
            float4 v = *reinterpret_cast<const float4 *>(val + k0);
            int2 c = *reinterpret_cast<const int2 *>(col + k0);
            // (without this the compiler sinks each half of the pair into the branch of its mask: two narrow loads per entry)
            asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w), "+v"(c.x), "+v"(c.y));
            const bool in0 = k0 >= s, in1 = k0 + 1 < e;
            float2 x0 = x[in0 ? c.x : 0], x1 = x[in1 ? c.y : 0];
            asm volatile("" : "+v"(x0.x), "+v"(x0.y), "+v"(x1.x), "+v"(x1.y));      // (both gathers in flight together, no branch)
            c64_mac(ax, ay, in0 ? make_float2(v.x, v.y) : z, in0 ? x0 : z);
            c64_mac(ax, ay, in1 ? make_float2(v.z, v.w) : z, in1 ? x1 : z);
        }
    } else {
        for (long k = (long)s + lane; k < e; k += W) c64_mac(ax, ay, val[k], x[col[k]]);
    }
}

template <int W, bool PAIRS>
__global__ __launch_bounds__(VB) void k_c64_rows(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                 const float2 *__restrict__ val, const float2 *__restrict__ x,
                                                 float2 *__restrict__ y, int long_min, const int *done)
{
    if (done && *done) return;
    const long row = ((long)blockIdx.x * VB + threadIdx.x) / W;
    if (row >= n) return;                   // (the W lanes of a row leave together: W divides the wavefront)
    const int lane = threadIdx.x & (W - 1);
    const int s = rowptr[row], e = rowptr[row + 1];
    if (e - s > long_min) return;           // k_c64_long's row
    float ax = 0.f, ay = 0.f;
    c64_row_part<PAIRS>(s, e, lane, W, col, val, x, ax, ay);
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        ax += __shfl_xor(ax, off, W);
        ay += __shfl_xor(ay, off, W);
    }
    if (lane == 0) y[row] = make_float2(ax, ay);
}

template <bool PAIRS>
__global__ __launch_bounds__(VB) void k_c64_long(const int *__restrict__ rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                 const float2 *__restrict__ val, const float2 *__restrict__ x,
                                                 float2 *__restrict__ y, const int *done)
{
    if (done && *done) return;
    const int row = rows[blockIdx.x];
    const int s = rowptr[row], e = rowptr[row + 1];
    float ax = 0.f, ay = 0.f;
    c64_row_part<PAIRS>(s, e, threadIdx.x, VB, col, val, x, ax, ay);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ax += __shfl_xor(ax, off, 64);
        ay += __shfl_xor(ay, off, 64);
    }
    __shared__ float2 sh[VB / 64];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = make_float2(ax, ay);
    __syncthreads();
    if (threadIdx.x == 0) {
        float2 t = sh[0];
#pragma unroll
        for (int w = 1; w < VB / 64; w++) { t.x += sh[w].x; t.y += sh[w].y; }
        y[row] = t;
    }
}

__global__ void k_c64_conj(long nnz, const float2 *in, float2 *out)
{
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (long)gridDim.x * blockDim.x)
        out[k] = make_float2(in[k].x, -in[k].y);
}

__global__ void k_c64_diag(int n, const int *rowptr, const int *col, const float2 *val, float2 *diag, float2 *inv)
{   // the diagonal (0 where a row has none) and its reciprocal: clcg_smCcsr_get_diagonal's job for sample14.cu's Jacobi
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float2 d = make_float2(0.f, 0.f);
    for (int k = rowptr[i]; k < rowptr[i + 1]; k++)
        if (col[k] == i) { d = val[k]; break; }
    if (diag) diag[i] = d;
    inv[i] = c64_div(make_float2(1.f, 0.f), d);
}

__global__ void k_c64_jacobi(int n, const float2 *__restrict__ inv, const float2 *__restrict__ x, float2 *__restrict__ z, const int *done)
{
    if (done && *done) return;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        z[i] = c64_mul(inv[i], x[i]);
    }
}

static int c64_error(const char *what)
{
    ctx().err = what;
    return LCG_HIP_E_ARG;
}

// the part that realises op(A), built on its first use
static int c64_part(lcg_hip_csr *A, int layout, int conjugate, CsrPart **out)
{
    const int idx = (layout ? 2 : 0) + (conjugate ? 1 : 0);
    if (idx == 0) { *out = &A->main; return 0; }
    CsrPart &T = A->op[idx];
    if (T.rowptr) { *out = &T; return 0; }
    if (A->n_cols != A->n_rows) return c64_error("lcg_hip_spmv_c64: op(A) other than A needs a square matrix");
    Ctx &c = ctx();
    const int n = A->n_rows;
    const long nnz = A->main.nnz;
    int rc = alloc_part(T, n, nnz, false);          // 8 bytes per value: one float pair
    if (rc) { free_part(T); return rc; }
    T.n_cols = n;
    const float2 *src = reinterpret_cast<const float2 *>(A->main.val);
    float2 *dst = reinterpret_cast<float2 *>(T.val);
    if (!layout) {
        HIPCHK(hipMemcpyAsync(T.rowptr, A->main.rowptr, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToDevice, c.stream));
        if (nnz) HIPCHK(hipMemcpyAsync(T.col, A->main.col, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToDevice, c.stream));
        if (nnz) hipLaunchKernelGGL(k_c64_conj, dim3(1024), dim3(VB), 0, c.stream, nnz, src, dst);
    } else {
        int *cnt = nullptr;
        HIPCHK(hipMalloc(&cnt, sizeof(int) * (size_t)n));
        rc = transpose_launch(n, n, nnz, A->main.rowptr, A->main.col, A->main.val, T.rowptr, T.col, T.val, false, 0, cnt, c.stream);
        hipFree(cnt);
        if (rc) { free_part(T); return rc; }
        if (conjugate && nnz) hipLaunchKernelGGL(k_c64_conj, dim3(1024), dim3(VB), 0, c.stream, nnz, dst, dst);
    }
    HIPCHK(hipGetLastError());
    *out = &T;
    return 0;
}

// the kernel of a part, chosen from its row lengths (host pass over the row pointers: once per part, then the launches allocate and
// synchronise nothing)
static int c64_plan(const CsrPart &P, C64Plan &pl, hipStream_t s)
{
    const int n = P.n_rows;
    std::vector<int> rp((size_t)n + 1);
    HIPCHK(hipMemcpyAsync(rp.data(), P.rowptr, sizeof(int) * rp.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double mean = n ? (double)(rp[n] - rp[0]) / n : 0.0;
    int W = 1;
    while (W < 64 && W < (mean + 1.0) / 2.0) W *= 2;       // lanes enough for a mean row's pairs (plus the straddling one)
    pl.lanes = W;
    pl.long_min = std::max(256, 64 * W);                   // more than 32 pairs per lane: the row goes to k_c64_long
    std::vector<int> lr;
    for (int i = 0; i < n; i++) if (rp[i + 1] - rp[i] > pl.long_min) lr.push_back(i);
    if (lr.empty()) pl.long_min = INT_MAX;
    pl.n_long = (int)lr.size();
    if (!lr.empty()) {
        HIPCHK(hipMalloc(&pl.long_rows, sizeof(int) * lr.size()));
        HIPCHK(hipMemcpyAsync(pl.long_rows, lr.data(), sizeof(int) * lr.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    pl.pairs = ((uintptr_t)P.val & 15) == 0 && ((uintptr_t)P.col & 7) == 0 && (P.padded || P.nnz % 2 == 0);
    pl.name = "k_c64_rows<" + std::to_string(W) + ">" + (pl.pairs ? " (entry pairs)" : " (single entries)");
    if (pl.n_long) pl.name += " + k_c64_long (" + std::to_string(pl.n_long) + " long rows)";
    pl.state = 1;
    return 0;
}

template <bool PAIRS>
static void c64_launch_rows(int W, unsigned g, hipStream_t s, int n, const int *rp, const int *col, const float2 *val,
                            const float2 *x, float2 *y, int long_min, const int *done)
{
    switch (W) {
#define C64_W(w) case w: hipLaunchKernelGGL((k_c64_rows<w, PAIRS>), dim3(g), dim3(VB), 0, s, n, rp, col, val, x, y, long_min, done); break;
    C64_W(1) C64_W(2) C64_W(4) C64_W(8) C64_W(16) C64_W(32) C64_W(64)
#undef C64_W
    }
}

static int c64_spmv(lcg_hip_csr *A, const float *x, float *y, int layout, int conjugate, const int *done)
{
    Ctx &c = ctx();
    const int idx = (layout ? 2 : 0) + (conjugate ? 1 : 0);
    CsrPart *P = nullptr;
    int rc = c64_part(A, layout, conjugate, &P);
    if (rc) return rc;
    C64Plan &pl = c64_of(A)->plan[idx];
    if (!pl.state) { rc = c64_plan(*P, pl, c.stream); if (rc) return rc; }
    const int n = P->n_rows;
    const float2 *v = reinterpret_cast<const float2 *>(P->val);
    const float2 *xv = reinterpret_cast<const float2 *>(x);
    float2 *yv = reinterpret_cast<float2 *>(y);
    const unsigned g = (unsigned)(((long)n * pl.lanes + VB - 1) / VB);
    if (pl.pairs) c64_launch_rows<true>(pl.lanes, g, c.stream, n, P->rowptr, P->col, v, xv, yv, pl.long_min, done);
    else c64_launch_rows<false>(pl.lanes, g, c.stream, n, P->rowptr, P->col, v, xv, yv, pl.long_min, done);
    if (pl.n_long) {
        if (pl.pairs) hipLaunchKernelGGL((k_c64_long<true>), dim3(pl.n_long), dim3(VB), 0, c.stream, pl.long_rows, P->rowptr, P->col, v, xv, yv, done);
        else hipLaunchKernelGGL((k_c64_long<false>), dim3(pl.n_long), dim3(VB), 0, c.stream, pl.long_rows, P->rowptr, P->col, v, xv, yv, done);
    }
    HIPCHK(hipGetLastError());
    A->main.last_kernel = pl.name.c_str();
    return 0;
}

void c64_free(lcg_hip_csr *A)
{
    C64Data *D = static_cast<C64Data *>(A->c64p);
    if (!D) return;
    for (C64Plan &pl : D->plan) if (pl.long_rows) hipFree(pl.long_rows);
    if (D->invdiag) hipFree(D->invdiag);
    delete D;
    A->c64p = nullptr;
}

int c64_build_jacobi(lcg_hip_csr *A, void *diag_out)
{
    Ctx &c = ctx();
    C64Data *D = c64_of(A);
    if (!D->invdiag) HIPCHK(hipMalloc(&D->invdiag, sizeof(float2) * (size_t)A->n_rows));
    const unsigned g = (unsigned)((A->n_rows + VB - 1) / VB);
    hipLaunchKernelGGL(k_c64_diag, dim3(g), dim3(VB), 0, c.stream, A->n_rows, A->main.rowptr, A->main.col,
                       reinterpret_cast<const float2 *>(A->main.val), static_cast<float2 *>(diag_out), D->invdiag);
    HIPCHK(hipGetLastError());
    return 0;
}

const float *c64_builtin_invdiag(const void *Mfp, void *inst, int n)
{
    if (Mfp != (const void *)clcg_hip_jacobi_mx_c64 || !inst) return nullptr;
    lcg_hip_csr *A = static_cast<lcg_hip_csr *>(inst);
    const C64Data *D = static_cast<const C64Data *>(A->c64p);
    return A->c64 && A->n_rows == n && D ? reinterpret_cast<const float *>(D->invdiag) : nullptr;
}

static int c64_jacobi(lcg_hip_csr *A, const float *x, float *z, int n)
{
    if (!A || !A->c64) return c64_error("clcg_hip_jacobi_mx_c64: the handle is not a complex64 matrix (lcg_hip_csr_create_c64)");
    const C64Data *D = static_cast<const C64Data *>(A->c64p);
    if (!D || !D->invdiag) return c64_error("clcg_hip_jacobi_mx_c64: lcg_hip_csr_build_jacobi() was not called");
    if (n != A->n_rows) return c64_error("clcg_hip_jacobi_mx_c64: n_size differs from the matrix's rows");
    Ctx &c = ctx();
    const int g = (int)std::min<long>(2048, ((long)n + VB - 1) / VB);
    hipLaunchKernelGGL(k_c64_jacobi, dim3(g), dim3(VB), 0, c.stream, n, D->invdiag, reinterpret_cast<const float2 *>(x),
                       reinterpret_cast<float2 *>(z), ax_flag(c));
    HIPCHK(hipGetLastError());
    return 0;
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_csr_create_c64(lcg_hip_csr_t *out, int n_rows, int n_cols, int64_t nnz, const int *rowptr, const int *col,
                           const float *val, int mem, int adopt)
{
    if (!out || n_rows <= 0 || nnz < 0 || nnz > 0x7fffffffLL || !rowptr || !col || !val) return LCG_HIP_E_ARG;
    int rc = ensure_init(); if (rc) return rc;
    Ctx &c = ctx();
    lcg_hip_csr *A = new lcg_hip_csr();
    A->n_rows = n_rows; A->n_cols = n_cols; A->c64 = true;
    A->mean_row = (double)nnz / n_rows;
    if (mem == LCG_HIP_MEM_DEVICE && adopt) {
        A->main.n_rows = n_rows; A->main.nnz = nnz; A->main.owned = false; A->main.padded = adopt == 2;
        A->main.n_cols = n_cols;
        A->main.rowptr = const_cast<int *>(rowptr); A->main.col = const_cast<int *>(col);
        A->main.val = reinterpret_cast<double *>(const_cast<float *>(val));
    } else {
        rc = alloc_part(A->main, n_rows, nnz, false);      // 8 bytes per value: one float pair
        if (rc) { free_part(A->main); delete A; return rc; }
        A->main.n_cols = n_cols;
        const hipMemcpyKind kind = mem == LCG_HIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        hipError_t e = hipMemcpyAsync(A->main.rowptr, rowptr, sizeof(int) * ((size_t)n_rows + 1), kind, c.stream);
        if (e == hipSuccess && nnz) e = hipMemcpyAsync(A->main.col, col, sizeof(int) * (size_t)nnz, kind, c.stream);
        if (e == hipSuccess && nnz) e = hipMemcpyAsync(A->main.val, val, sizeof(float) * 2 * (size_t)nnz, kind, c.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        if (e != hipSuccess) { free_part(A->main); delete A; return fail(e, "csr upload (c64)", __FILE__, __LINE__); }
    }
    *out = A;
    return 0;
}

int lcg_hip_spmv_c64(lcg_hip_csr_t A, const float *x, float *y, int layout, int conjugate)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    int rc = ensure_init(); if (rc) return rc;
    if (!A || !x || !y) return LCG_HIP_E_ARG;
    if (!A->c64) return c64_error("lcg_hip_spmv_c64: the handle is not a complex64 matrix (lcg_hip_csr_create_c64)");
    if (A->distributed) return c64_error("lcg_hip_spmv_c64: complex64 matrices are not sharded");
    return c64_spmv(A, x, y, layout, conjugate, ax_flag(ctx()));
}

// The callback types return void: a failure is parked in Ctx::ax_rc and ends the solve (driver.hpp: timed_ax / checked_mx).
void clcg_hip_csr_ax_c64(void *instance, const float *x, float *prod_Ax, const int n_size, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    (void)n_size;
    const int rc = lcg_hip_spmv_c64(static_cast<lcg_hip_csr *>(instance), x, prod_Ax, layout, conjugate);
    if (rc && !ctx().ax_rc) ctx().ax_rc = rc;
}

void clcg_hip_jacobi_mx_c64(void *instance, const float *x, float *prod_Mx, const int n_size, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    (void)layout; (void)conjugate;
    const int rc = c64_jacobi(static_cast<lcg_hip_csr *>(instance), x, prod_Mx, n_size);
    if (rc && !ctx().ax_rc) ctx().ax_rc = rc;
}

} // extern "C"
