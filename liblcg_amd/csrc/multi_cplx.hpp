// multi_cplx.hpp -- what the complex multi-vector product (csr_multi_cplx.hip) and the batched complex loops
// (solvers_multi_cplx.hip, solvers_multi_cbicg.hip) share.  Not installed.
//
// A block of k complex vectors is ONE array of n * k interleaved (re, im) pairs, row-major: column j of row i is the 16-byte piece
// i * k + j (doubles 2 (i k + j) and 2 (i k + j) + 1); k = 2, 4, 8; the base 16-byte aligned.  DESIGN.md section 18.
#pragma once

#include "multi_loop.hpp"

namespace lcgh {

constexpr int CMM_W = 1536;     // entries per LDS window of k_cspmm: 30,720 B of staging (16 B value + 4 B column), five blocks per CU

// a CSR handle this path serves: complex128, whole (not sharded), not dense (0, or LCG_HIP_E_ARG with the text)
int cmulti_handle(const char *entry, const lcg_hip_csr *A);

// what the product's epilogue carries per column j besides Y (the table rows it fills; a sum is re, im in consecutive rows):
//   CSPMM_DOT    U a block:       the UNCONJUGATED sum Y_j . U_j (clcg_dot)                      rows 2 j, 2 j + 1
//   CSPMM_INNER  U ONE vector u:  sum conj(u_i) Y_ij (clcg_inner(u, Y_j)); u is read once per row  rows 2 j, 2 j + 1
//   CSPMM_DOT2   U a block:       sum conj(Y_ij) U_ij (clcg_inner(Y_j, U_j)) and sum |Y_ij|^2    rows 2 j, 2 j + 1 and 2 k + j
enum { CSPMM_DOT = 1, CSPMM_INNER = 2, CSPMM_DOT2 = 3 };
inline int cspmm_tab(int mode) { return mode == CSPMM_DOT2 ? 3 : 2; }

// Y = A.X for the k complex columns in one launch (P's plain CSR arrays, val = interleaved (re, im): no plan is built or used).  With
// U: column j's sums of `mode` are left as *slots <= MM_MG partial sums each, table row q at dots[q * MM_MG ...], to be added in index
// order.  `big` holds the per-workgroup sums of a matrix with more than MM_MG row blocks on their way there (cspmm_big_doubles(P, k,
// mode) doubles; may be null where that is 0).  multi.hpp's frame with cspmm_tab(mode) table rows per column.
int cspmm_launch(const CsrPart &P, int k, const double *X, double *Y, hipStream_t s, const int *done, const double *U = nullptr,
                 double *big = nullptr, double *dots = nullptr, int *slots = nullptr, int mode = CSPMM_DOT);
inline size_t cspmm_big_doubles(const CsrPart &P, int k, int mode = CSPMM_DOT) { return multi_big_doubles(P, cspmm_tab(mode) * k); }

// the shadow residual of the next complex solve on the device (solvers_cplx.hip): lcg_hip_set_shadow_vector's vector, consumed, or the
// draw from lcg_hip_set_shadow_seed; n complex elements, copied on c.stream and waited for
int make_shadow(Ctx &c, int n, double *dev);

// ---- the batched complex loops' state and the steps they share ----------------------------------------------------------------------
struct ZMState : MultiHead {
    double ak[2 * MM_MAXK], bk[2 * MM_MAXK], rho[2 * MM_MAXK];      // complex: re at [2 j], im at [2 j + 1]; rho = r.r (PCG: r.s; BiCGStab: <rb, r>)
    double m2[MM_MAXK], r2[MM_MAXK], residual[MM_MAXK];              // sum |m|^2, sum |r|^2 as they were last added up
};

__device__ __forceinline__ m2d zmul(m2d a, m2d b) { m2d r; r.x = a.x * b.x - a.y * b.y; r.y = a.x * b.y + a.y * b.x; return r; }
__device__ __forceinline__ m2d zfma(m2d a, m2d b, m2d c)     // a * b + c, cfma's order (devcommon.hpp)
{
    m2d r; r.x = fma(a.x, b.x, fma(-a.y, b.y, c.x)); r.y = fma(a.x, b.y, fma(a.y, b.x, c.y)); return r;
}
__device__ __forceinline__ m2d znorms(m2d a, m2d b) { m2d r; r.x = a.x * a.x + a.y * a.y; r.y = b.x * b.x + b.y * b.y; return r; }
__device__ __forceinline__ m2d zinner(m2d a, m2d b)          // conj(a) * b, acc_inner's products (solvers_cplx.hip)
{
    m2d r; r.x = a.x * b.x + a.y * b.y; r.y = a.x * b.y - a.y * b.x; return r;
}
__device__ __forceinline__ void zst(double *p, long e, m2d v) { reinterpret_cast<m2d *>(p)[e] = v; }

// ---- scalar steps: sum[(s * K + j) * 2 + c] ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double2 zld(const double *p, int j) { return make_double2(p[2 * j], p[2 * j + 1]); }
__device__ __forceinline__ void zsts(double *p, int j, double2 v) { p[2 * j] = v.x; p[2 * j + 1] = v.y; }
// the residual of the loop's stop rule out of sum |r|^2 and sum |m|^2
template <bool PCG> __device__ __forceinline__ double zm_residual(const ZMState *st, double r2, double mm)
{
    if (PCG) return st->abs_diff ? sqrt(r2) / st->n_global : r2 / clamp1(mm);               // clcg_cuda.cu:459,472,478
    const double m4 = clamp1(mm * mm), r4 = r2 * r2;                                        // clcg.cpp:262-270
    return st->abs_diff ? sqrt(r4) / st->n_global : r4 / m4;                                // clcg.cpp:295-296
}

// setup.  Sums |m|^2, |r|^2, rho (BiCG-sym: r.r; PCG: r.s; BiCGStab: <rb, r>).  The 4th-power loops try BOTH "already optimised"
// criteria in abs_diff mode, in the reference's order (clcg.cpp:273-290, 574-591); PCG only its mode's own (clcg_cuda.cu:456-466)
template <int K, bool PCG> struct ZMFinInit {
    static constexpr int NS = 4;
    __device__ void operator()(ZMState *st, const double *sum) const
    {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double mm = sum[2 * j], r2 = sum[2 * j + 1];
            st->m2[j] = mm; st->r2[j] = r2;
            zsts(st->rho, j, make_double2(sum[(K + j) * 2], sum[(K + j) * 2 + 1]));
            double r = zm_residual<PCG>(st, r2, mm);
            bool already = r <= st->eps;
            if (!PCG && !already && st->abs_diff) {
                const double rel = (r2 * r2) / clamp1(mm * mm);
                if (rel <= st->eps) { r = rel; already = true; }
            }
            st->residual[j] = r;
            st->stop[j] = already ? ST_ALREADY : ST_RUNNING;
        }
        all_stopped<K>(st);
        mpublish(st);
    }
};
// first step of a body: counts it; ak = rho / sum per running column (clcg.cpp:320-321, 621-622; clcg_cuda.cu:501-502).  Sums: the
// product's (d.Ad; BiCGStab: <rb, A.p>)
template <int K> struct ZMFinAlpha {
    static constexpr int NS = 2;
    __device__ void operator()(ZMState *st, const double *sum) const
    {
        st->it++;
        if (st->all_done) return;
#pragma unroll
        for (int j = 0; j < K; j++)
            if (st->stop[j] == ST_RUNNING) zsts(st->ak, j, cdiv(zld(st->rho, j), make_double2(sum[2 * j], sum[2 * j + 1])));
    }
};

inline int zm_code(int stop)
{
    switch (stop) {
    case ST_ALREADY: return CLCG_ALREADY_OPTIMIZIED;
    case ST_NAN: return CLCG_NAN_VALUE;
    case ST_CONVERGED: return CLCG_CONVERGENCE;
    default: return LCG_REACHED_MAX_ITERATIONS;     // (-1019 from the real enum, as the complex loops return at the cap: SURVEY quirk 5)
    }
}

} // namespace lcgh
