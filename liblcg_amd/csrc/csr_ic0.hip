// csr_ic0.hip -- incomplete Cholesky IC(0) with zero fill: the preconditioner of sample8.cu's PCG leg (csric02 + two csrsv2
// solves, sample8.cu:105-119,183-238) and of the complex samples' L.L^T (unconjugated, principal square root:
// clcg_incomplete_Cholesky_cuda_full, preconditioner_cuda.cu:207-259).  DESIGN 11.
//
// build: the lower triangle of A (diagonal included, duplicates summed, upper triangle ignored) is extracted on the device
// (extract_rows, csr_tri.hpp), the level sets of L (forward) and L^T (backward) are found by one host pass over the downloaded
// pattern, and the rows are listed level by level.  The factor itself runs on the device over the forward schedule
// (IcFactorRow on the level walker): row i needs exactly the rows its forward solve needs.  L^T is then made by the transpose
// path of op(A) (k_tr_count / k_tr_fill / k_row_sort).  The result is a TriFactor with the diagonal last in L and first in
// L^T; its solves, sweeps and the host surface behind the entries below are csr_tri.hip's, shared with ILU(0).
//
// value types: double (real), double2 (complex128) and float2 (complex64: clcg_incomplete_Cholesky_cuda_half's cuComplex
// overload, preconditioner_cuda.cu, and the two cusparseSpSV solves with CUDA_C_32F of sample14.cu).  The complex64 factor and
// solves are fp32 throughout: products by c64_mul, quotients by c64_div (cuCdivf's scaled formula, c64common.hpp), the
// principal root by csqrt_principal_f, in the same order of operations as the other two types.  Its values are 8 bytes, so
// the build moves them with the real type's helpers as opaque 8-byte words (alloc_part / row_sort_launch / transpose_launch with
// cplx = false).  k_row_sort breaks ties between duplicate (row, column) entries on those words: duplicates are summed in a
// fixed order unless an imaginary part is Inf / NaN.  (L^T has no duplicate columns.)
//
// sweeps (lcg_hip_csr_ic0_set_sweeps, k >= 1): a triangle T = D + N is not solved but approximated by k Jacobi sweeps
// y <- D^-1 (x - N.y) from y = 0: the first is y = x / diag (k_ic_scale), each later one a sparse triangular product over ALL
// rows at once (k_ic_sweep: no level, no dependency between rows, one launch).  2k launches per full apply.
#include <cmath>

#include "csr_tri.hpp"

namespace lcgh {

// ------------------------------------------------------------------------------------------ factor
__device__ __forceinline__ double2 csqrt_principal(double2 z)
{
    if (z.x == 0.0 && z.y == 0.0) return make_double2(0.0, z.y);
    const double r = hypot(z.x, z.y);
    if (z.x >= 0.0) {
        const double t = sqrt(0.5 * (r + z.x));
        return make_double2(t, z.y / (2.0 * t));
    }
    const double t = sqrt(0.5 * (r - z.x));
    return make_double2(fabs(z.y) / (2.0 * t), copysign(t, z.y));
}
__device__ __forceinline__ float2 csqrt_principal_f(float2 z)     // the same branches in fp32 (std::sqrt(std::complex<float>))
{
    if (z.x == 0.0f && z.y == 0.0f) return make_float2(0.0f, z.y);
    const float r = hypotf(z.x, z.y);
    if (z.x >= 0.0f) {
        const float t = sqrtf(0.5f * (r + z.x));
        return make_float2(t, z.y / (2.0f * t));
    }
    const float t = sqrtf(0.5f * (r - z.x));
    return make_float2(fabsf(z.y) / (2.0f * t), copysignf(t, z.y));
}
__device__ __forceinline__ double ic_sqrt(double d) { return sqrt(d); }
__device__ __forceinline__ double2 ic_sqrt(double2 d) { return csqrt_principal(d); }
__device__ __forceinline__ float2 ic_sqrt(float2 d) { return csqrt_principal_f(d); }
__device__ __forceinline__ bool pivot_fails(double d) { return !(d > 0.0) || !isfinite(d); }
__device__ __forceinline__ bool pivot_fails(double2 d) { return (d.x == 0.0 && d.y == 0.0) || !isfinite(d.x) || !isfinite(d.y); }
__device__ __forceinline__ bool pivot_fails(float2 d) { return (d.x == 0.0f && d.y == 0.0f) || !isfinite(d.x) || !isfinite(d.y); }

// Row i of L in place (val holds A's lower triangle on entry).  L(i,j) = (A(i,j) - sum_{k<j} L(i,k) L(j,k)) / L(j,j) by a sorted
// merge of row i's prefix with row j, then L(i,i) = sqrt(A(i,i) - sum_k L(i,k)^2).  Rows j < i are final (earlier levels).
template <class V>
struct IcFactorRow {
    const int *rowptr, *col;
    V *val;
    int *zp;
    __device__ __forceinline__ void operator()(int i) const
    {
        const int s = rowptr[i], e = rowptr[i + 1] - 1;     // e: the diagonal
        for (int p = s; p < e; p++) {
            const int j = col[p];
            V v = val[p];
            int r = s, q = rowptr[j];
            const int qe = rowptr[j + 1] - 1;
            while (r < p && q < qe) {
                const int cr = col[r], cq = col[q];
                if (cr == cq) { v = vsub(v, ic_mul(val[r], val[q])); r++; q++; }
                else if (cr < cq) r++;
                else q++;
            }
            val[p] = ic_div(v, val[qe]);
        }
        V d = val[e];
        for (int p = s; p < e; p++) d = vsub(d, ic_mul(val[p], val[p]));
        if (pivot_fails(d)) atomicMin(zp, i);
        val[e] = ic_sqrt(d);
    }
};

// --------------------------------------------------------------------------------------------- host
constexpr TriSlot IC0 = &lcg_hip_csr::ic0;
constexpr const char *IC0_BUILDERS = "lcg_hip_csr_build_ic0, lcg_hip_csr_build_ic0_c64";

// Everything made here belongs to F (a failed build's caller frees it), but for the transpose's row counts.
template <class V>
static int ic0_build(lcg_hip_csr *A, TriFactor *F, hipStream_t s)
{
    const int n = A->n_rows;
    int rc = extract_rows<V, true>(A, F->lo, F->cplx, s);
    if (rc) return rc;
    // level sets from the pattern: forward level(i) = 1 + max over j < i in row i; backward over L^T, in reverse row order
    const long nnz = F->lo.nnz;
    std::vector<int> rp((size_t)n + 1), col((size_t)nnz);
    HIPCHK(hipMemcpy(rp.data(), F->lo.rowptr, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(col.data(), F->lo.col, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost));
    std::vector<int> lf((size_t)n, 0), lb((size_t)n, 0);
    int nf = 0, nb = 0;
    for (int i = 0; i < n; i++) {
        int l = 0;
        for (int p = rp[(size_t)i]; p < rp[(size_t)i + 1] - 1; p++) l = std::max(l, lf[(size_t)col[(size_t)p]] + 1);
        lf[(size_t)i] = l; nf = std::max(nf, l + 1);
    }
    for (int i = n - 1; i >= 0; i--) {
        const int l = lb[(size_t)i];
        nb = std::max(nb, l + 1);
        for (int p = rp[(size_t)i]; p < rp[(size_t)i + 1] - 1; p++) { int &o = lb[(size_t)col[(size_t)p]]; o = std::max(o, l + 1); }
    }
    rc = tri_schedule(F, lf, nf, lb, nb); if (rc) return rc;
    // factor in place on the forward schedule
    rc = pivot_arm(F, s); if (rc) return rc;
    rc = run_levels(F->fw, IcFactorRow<V>{F->lo.rowptr, F->lo.col, reinterpret_cast<V *>(F->lo.val), F->zp}, nullptr, s); if (rc) return rc;
    rc = pivot_read(F, s); if (rc) return rc;
    // L^T by the transpose path of op(A)
    rc = alloc_part(F->up, n, nnz, F->cplx); if (rc) return rc;
    F->up.n_cols = n;
    int *cnt = nullptr;
    HIPCHK(hipMalloc(&cnt, sizeof(int) * (size_t)n));
    rc = transpose_launch(n, n, nnz, F->lo.rowptr, F->lo.col, F->lo.val, F->up.rowptr, F->up.col, F->up.val, F->cplx, 0, cnt, s);
    hipFree(cnt);
    if (rc) return rc;
    HIPCHK(hipMalloc(&F->tmp, sizeof(V) * (size_t)n));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// the build behind lcg_hip_csr_build_ic0 and lcg_hip_csr_build_ic0_c64 (the handle's type already checked)
static int ic0_build_entry(lcg_hip_csr *A)
{
    return tri_build(A, IC0, "IC(0)", 0, "zero, negative or not finite", [](lcg_hip_csr *A, TriFactor *F, hipStream_t s) {
        return F->c64 ? ic0_build<float2>(A, F, s) : F->cplx ? ic0_build<double2>(A, F, s) : ic0_build<double>(A, F, s);
    });
}

// the apply behind the callbacks and the solve entries.  c64: the complex64 entries (a complex64 handle only); otherwise cplx
// picks the fp64 or the complex128 factor.
static int ic0_call(void *A, bool cplx, bool c64, int which, const void *x, void *y, long n_size)
{
    return tri_call(static_cast<lcg_hip_csr *>(A), IC0, "IC(0)", c64 ? "lcg_hip_csr_build_ic0_c64" : "lcg_hip_csr_build_ic0",
                    cplx, c64, which, static_cast<const double *>(x), static_cast<double *>(y), n_size);
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_csr_build_ic0(lcg_hip_csr_t A)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return LCG_HIP_E_ARG;
    TRY_C64(A, "lcg_hip_csr_build_ic0");
    return ic0_build_entry(A);
}

int lcg_hip_csr_build_ic0_c64(lcg_hip_csr_t A)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    int rc = ensure_init(); if (rc) return rc;
    if (!A) return LCG_HIP_E_ARG;
    if (!A->c64) return arg_error("lcg_hip_csr_build_ic0_c64: the handle is not a complex64 matrix (lcg_hip_csr_create_c64; "
                                  "fp64 / complex128 handles: lcg_hip_csr_build_ic0)");
    return ic0_build_entry(A);
}

int lcg_hip_csr_ic0_info(lcg_hip_csr_t A, int *levels_lower, int *levels_upper, int *launches_per_apply, int *zero_pivot,
                         double *build_ms, int64_t *bytes)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return tri_info(A, IC0, levels_lower, levels_upper, launches_per_apply, zero_pivot, build_ms, bytes);
}

int lcg_hip_csr_ic0_set_sweeps(lcg_hip_csr_t A, int sweeps)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return tri_set_sweeps(A, IC0, __func__, IC0_BUILDERS, sweeps);
}

int lcg_hip_csr_ic0_get_sweeps(lcg_hip_csr_t A, int *sweeps)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return tri_get_sweeps(A, IC0, __func__, IC0_BUILDERS, sweeps);
}

int lcg_hip_csr_ic0_factor(lcg_hip_csr_t A, const int **rowptr, const int **col, const double **val)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return tri_arrays(A, IC0, 0, rowptr, col, val);
}

int lcg_hip_ic0_solve(lcg_hip_csr_t A, int which, const double *x, double *y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    if (!A) return LCG_HIP_E_ARG;
    return ic0_call(A, A->is_complex, false, which, x, y, -1);
}

int lcg_hip_ic0_solve_c64(lcg_hip_csr_t A, int which, const float *x, float *y)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    int rc = ensure_init(); if (rc) return rc;
    return ic0_call(A, false, true, which, x, y, -1);
}

int lcg_hip_csr_ic0_schedule_for_test(lcg_hip_csr_t A, int max_merged_rows)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return tri_schedule_for_test(A, IC0, max_merged_rows);
}

// The callback types return void (lcg.h:37-38, clcg.h:40-41): a failure is parked in Ctx::ax_rc (park, csr_tri.hip).
void lcg_hip_ic0_mx(void *instance, const double *x, double *prod_Mx, const int n_size)
{
    NOT_DENSE_CB(instance);
    park(ic0_call(instance, false, false, 2, x, prod_Mx, n_size));
}

void clcg_hip_ic0_mx(void *instance, const double *x, double *prod_Mx, const int n_size, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    (void)layout;       // M = L.L^T is complex-symmetric: M^T = M
    park(conjugate ? arg_error("IC(0): conjugate = 1 is not offered (M^H != M)") : ic0_call(instance, true, false, 2, x, prod_Mx, n_size));
}

void clcg_hip_ic0_mx_c64(void *instance, const float *x, float *prod_Mx, const int n_size, int layout, int conjugate)
{
    NOT_DENSE_CB(instance);
    (void)layout;       // M = L.L^T is complex-symmetric: M^T = M
    park(conjugate ? arg_error("IC(0): conjugate = 1 is not offered (M^H != M)") : ic0_call(instance, false, true, 2, x, prod_Mx, n_size));
}

} // extern "C"
