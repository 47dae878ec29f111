// solvers_multi_c64.hip -- batched complex64 loops over k = 2, 4, 8 right-hand sides against one complex-symmetric complex64 matrix:
// clcg_hip_lbicg_sym_multi_c64 (clbicg_symmetric, clcg_cudaf.cu:254-401) and clcg_hip_lpcg_multi_c64 (clpcg with the handle's
// reciprocal Jacobi diagonal, clcg_cudaf.cu:403-558), and the same loops on a dense complex64 handle (clcg_hip_dense_*_multi_c64).
//
// Each column runs solvers_c64.hip's recurrence as if it were alone: its own ak, bk and rho (r.r; PCG: r.s), both inner products
// UNCONJUGATED (cublasCdotu), its own stop test, "already optimised" test, count and code.  What the columns share is the matrix: one
// multi-vector product per iteration (csr_multi_c64.hip) reads col / val once for all of them.
//
// Three launches per iteration, every scalar step in the prologue of the pass that consumes it (k_mvecf, multi_loop.hpp):
//     A.d carrying d.Ad  |  [ak = rho / d.Ad] m += ak d; r -= ak Ad (PCG: s = inv .* r) + |m|^2, |r|^2, r.r (r.s)  |  [close] d = r + bk d (s + bk d)
//
// Arithmetic is solvers_c64.hip's: vectors are fp32 (c64_mul, then one add: cublasCaxpy / Cscal), ak, bk, the norms and the residual are
// fp32 values kept in the state's 8-byte words (exactly representable there), c64_div is cuCdivf's scaled quotient; every dot and norm
// is an fp64 sum of exact products of fp32 values, rounded to fp32 once, in the scalar step.
//
// Stop rule, as the single complex64 loops for BOTH solvers: residual = |r|^2 / max(|m|, 1)^2 in fp32 (|.| the rounded 2-norms), or
// |r| / n with abs_diff, where "already optimised" tests |r| / n only.  A column ends with CLCG_NAN_VALUE at the first iteration whose
// sum |m|^2 or sum |r|^2 is NaN, its count the iteration in which the NaN appeared.
//
// A 16-byte piece holds one row's elements of the columns c0 and c0 + 1 = 2 l, 2 l + 1 of lane l of a row's K / 2 lanes, and the stride
// of a pass is a multiple of K / 2: a thread's columns never change, their coefficients and stop words stay in registers.  Frozen
// columns: r0 / r1 freeze each half on its own -- a SELECT on the stop word, not a multiplication by zero -- so a stopped column's 8
// bytes of m, r, d, s are never stored to again (C64MOp st4) and a NaN column's sums are never read by another.  The product still
// forms such a column's A.d, which nothing reads.
//
// Column j's results are the same bits whatever k is and wherever the column stands: the product's sums are added in an order the
// matrix fixes (msum), the passes' sums as ONE binary tree over leaves that depend on n alone (multi.hpp: tree_leaves, msum_tree).
//
// The pass is k_mvecf with a lane group of G = K / 2: component c of accumulator s belongs to column c0 + c and goes to table row
// s * K + j.  A complex sum takes two accumulators (re, im); a scalar step reads sum[s * K + j].  The product's d.Ad lies in the
// complex frame's order instead: rows 2 j, 2 j + 1.
//
// clcg_hip_lpcg_multi_m_c64 with LCG_HIP_M_IC0: the multiply leaves the update pass, as in solvers_multi.hip:
//     A.d carrying d.Ad  |  [ak] m += ak d; r -= ak Ad  |  s = (L.L^T)^-1 r (the k-wide apply's launches)  |  |m|^2, |r|^2, r.s  |  [close] d = s + bk d
// The apply forms s for every column, stopped ones too (nothing reads theirs: s is scratch); every one of its launches honours all_done.
//
// Kernel functors carry a C64M prefix: k_mvecf is instantiated per translation unit (tests/test_abi.py).
#include "c64common.hpp"
#include "multi_loop.hpp"
#include "multi_c64.hpp"
#include "dense.hpp"
#include "lcg_hip_staging_ic0_c64.h"
#include "lcg_hip_staging_dense_c64.h"

namespace lcgh {
namespace {

typedef float c64v4 __attribute__((ext_vector_type(4)));      // a piece: (re, im) of column c0, (re, im) of column c0 + 1

struct C64MState : MultiHead {
    double ak[2 * MM_MAXK], bk[2 * MM_MAXK], rho[2 * MM_MAXK];      // complex fp32 values: re at [2 j], im at [2 j + 1]; rho = r.r (PCG: r.s)
    double mm[MM_MAXK], rk[MM_MAXK], residual[MM_MAXK];              // fp32 values: max(|m|, 1), |r|, the residual
};

__device__ __forceinline__ float2 c64m_get(const double *p, int j) { return make_float2((float)p[2 * j], (float)p[2 * j + 1]); }
__device__ __forceinline__ void c64m_put(double *p, int j, float2 v) { p[2 * j] = v.x; p[2 * j + 1] = v.y; }
__device__ __forceinline__ float2 c64m_axpy(float2 a, float2 x, float2 y)       // y + a x  (cublasCaxpy; solvers_c64.hip: faxpy)
{
    const float2 p = c64_mul(a, x);
    return make_float2(y.x + p.x, y.y + p.y);
}
__device__ __forceinline__ float2 c64m_lo(c64v4 v) { return make_float2(v.x, v.y); }
__device__ __forceinline__ float2 c64m_hi(c64v4 v) { return make_float2(v.z, v.w); }
__device__ __forceinline__ c64v4 c64m_join(float2 a, float2 b) { c64v4 r; r.x = a.x; r.y = a.y; r.z = b.x; r.w = b.y; return r; }
__device__ __forceinline__ c64v4 c64m_ld(const float *p, long e) { return reinterpret_cast<const c64v4 *>(p)[e]; }
// only the running halves of a piece are written: a stopped column's 8 bytes are never stored to again
__device__ __forceinline__ void c64m_st(float *p, long e, c64v4 v, bool r0, bool r1)
{
    if (r0 && r1) reinterpret_cast<c64v4 *>(p)[e] = v;
    else if (r0) reinterpret_cast<float2 *>(p)[2 * e] = c64m_lo(v);
    else if (r1) reinterpret_cast<float2 *>(p)[2 * e + 1] = c64m_hi(v);
}
// fp64 accumulation of exact products of fp32 values, per half of a piece (solvers_c64.hip: f_acc_norm, f_acc_dotu)
__device__ __forceinline__ double c64m_norm(float2 a) { return (double)a.x * a.x + (double)a.y * a.y; }
__device__ __forceinline__ void c64m_sums(m2d *acc, c64v4 m, c64v4 r, c64v4 z)    // |m|^2, |r|^2, r.z (re, im)
{
    acc[0].x += c64m_norm(c64m_lo(m)); acc[0].y += c64m_norm(c64m_hi(m));
    acc[1].x += c64m_norm(c64m_lo(r)); acc[1].y += c64m_norm(c64m_hi(r));
    acc[2].x += (double)r.x * z.x - (double)r.y * z.y; acc[2].y += (double)r.z * z.z - (double)r.w * z.w;
    acc[3].x += (double)r.x * z.y + (double)r.y * z.x; acc[3].y += (double)r.z * z.w + (double)r.w * z.z;
}

// ---- scalar steps: sum[s * K + j] ---------------------------------------------------------------------------------------------------------
// sums |m|^2, |r|^2 of column j: m_mod (clamped at 1, clcg_cudaf.cu:146) and rk_mod into their slots; the residual they give
template <int K> __device__ __forceinline__ float c64m_norms(C64MState *st, const double *sum, int j)
{
    float mm = (float)sqrt(sum[j]);
    if (mm < 1.0f) mm = 1.0f;
    const float rk = (float)sqrt(sum[K + j]);
    st->mm[j] = mm; st->rk[j] = rk;
    return st->abs_diff ? rk / (float)st->n_global : rk * rk / (mm * mm);
}
// setup.  Sums |m|^2, |r|^2, rho (BiCG-sym: r.r; PCG: r.s): the already-optimised test (clcg_cudaf.cu:314-332, :467-485)
template <int K> struct C64MFinInit {
    static constexpr int NS = 4;
    __device__ void operator()(C64MState *st, const double *sum) const
    {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const float r = c64m_norms<K>(st, sum, j);
            c64m_put(st->rho, j, make_float2((float)sum[2 * K + j], (float)sum[3 * K + j]));
            st->residual[j] = r;
            st->stop[j] = r <= st->eps ? ST_ALREADY : ST_RUNNING;
        }
        all_stopped<K>(st);
        mpublish(st);
    }
};
// first step of a body: counts it; ak = rho / d.Ad per running column (cuCdivf; :363-364, :515-516).  Sums: the product's (rows 2 j, 2 j + 1)
template <int K> struct C64MFinAlpha {
    static constexpr int NS = 2;
    __device__ void operator()(C64MState *st, const double *sum) const
    {
        st->it++;
        if (st->all_done) return;
#pragma unroll
        for (int j = 0; j < K; j++)
            if (st->stop[j] == ST_RUNNING)
                c64m_put(st->ak, j, c64_div(c64m_get(st->rho, j), make_float2((float)sum[2 * j], (float)sum[2 * j + 1])));
    }
};
// closing step of a body, per running column: bk = new / old, rho = new, t++, the stop test of the next loop head (:378-379, :533-534)
template <int K> struct C64MFinClose {
    static constexpr int NS = 4;
    __device__ void operator()(C64MState *st, const double *sum) const
    {
        if (!st->all_done) {
#pragma unroll
            for (int j = 0; j < K; j++) {
                if (st->stop[j] != ST_RUNNING) continue;
                st->t[j]++;
                if (sum[j] != sum[j] || sum[K + j] != sum[K + j]) { st->stop[j] = ST_NAN; continue; }   // a NaN in m or r (a breakdown)
                const float r = c64m_norms<K>(st, sum, j);
                const float2 nw = make_float2((float)sum[2 * K + j], (float)sum[3 * K + j]);
                c64m_put(st->bk, j, c64_div(nw, c64m_get(st->rho, j)));
                c64m_put(st->rho, j, nw);
                st->residual[j] = r;
                if (r <= st->eps) st->stop[j] = ST_CONVERGED;
            }
            all_stopped<K>(st);
        }
        mpublish(st);
    }
};

// ---- vector passes ------------------------------------------------------------------------------------------------------------------------
template <bool PCG> struct C64MOpInit {     // r = B - Ad; d = r (PCG: d = inv .* r); |m|^2, |r|^2, r.r (r.d)    clcg_cudaf.cu:293-311, :445-464
    static constexpr int NS = 4;
    const float *Ad, *B, *m, *inv; float *r, *d;
    __device__ void prep(const C64MState &, int) {}
    __device__ void apply(long e, long row, bool r0, bool r1, m2d *acc)
    {
        const float2 m1 = make_float2(-1.f, 0.f);
        const c64v4 av = c64m_ld(Ad, e), bv = c64m_ld(B, e);
        const c64v4 rv = c64m_join(c64m_axpy(m1, c64m_lo(av), c64m_lo(bv)), c64m_axpy(m1, c64m_hi(av), c64m_hi(bv)));
        c64v4 dv = rv;
        if (PCG) {
            const float2 iv = reinterpret_cast<const float2 *>(inv)[row];
            dv = c64m_join(c64_mul(iv, c64m_lo(rv)), c64_mul(iv, c64m_hi(rv)));
        }
        c64m_st(r, e, rv, r0, r1); c64m_st(d, e, dv, r0, r1);
        c64m_sums(acc, c64m_ld(m, e), rv, dv);
    }
};
template <bool PCG> struct C64MOpUpdate {   // m += ak d; r -= ak Ad (PCG: s = inv .* r); |m|^2, |r|^2, r.r (r.s)   :366-377, :518-532
    static constexpr int NS = 4;
    float *m, *r, *s; const float *d, *Ad, *inv; float2 ak0, ak1;
    __device__ void prep(const C64MState &L, int c) { ak0 = c64m_get(L.ak, c); ak1 = c64m_get(L.ak, c + 1); }
    __device__ void apply(long e, long row, bool r0, bool r1, m2d *acc)
    {
        const c64v4 dv = c64m_ld(d, e), av = c64m_ld(Ad, e), mo = c64m_ld(m, e), ro = c64m_ld(r, e);
        const float2 n0 = make_float2(-ak0.x, -ak0.y), n1 = make_float2(-ak1.x, -ak1.y);
        const c64v4 mv = c64m_join(c64m_axpy(ak0, c64m_lo(dv), c64m_lo(mo)), c64m_axpy(ak1, c64m_hi(dv), c64m_hi(mo)));
        const c64v4 rv = c64m_join(c64m_axpy(n0, c64m_lo(av), c64m_lo(ro)), c64m_axpy(n1, c64m_hi(av), c64m_hi(ro)));
        c64m_st(m, e, mv, r0, r1); c64m_st(r, e, rv, r0, r1);
        c64v4 sv = rv;
        if (PCG) {
            const float2 iv = reinterpret_cast<const float2 *>(inv)[row];
            sv = c64m_join(c64_mul(iv, c64m_lo(rv)), c64_mul(iv, c64m_hi(rv)));
            c64m_st(s, e, sv, r0, r1);
        }
        c64m_sums(acc, mv, rv, sv);
    }
};
struct C64MOpDir {      // d = bk d + z (z: r, PCG: s)   (Cscal + Caxpy: :381-382, :536-537)
    static constexpr int NS = 0;
    float *d; const float *z; float2 bk0, bk1;
    __device__ void prep(const C64MState &L, int c) { bk0 = c64m_get(L.bk, c); bk1 = c64m_get(L.bk, c + 1); }
    __device__ void apply(long e, long, bool r0, bool r1, m2d *)
    {
        const c64v4 dv = c64m_ld(d, e), zv = c64m_ld(z, e);
        const float2 b0 = c64_mul(bk0, c64m_lo(dv)), b1 = c64_mul(bk1, c64m_hi(dv));
        c64v4 o; o.x = b0.x + zv.x; o.y = b0.y + zv.y; o.z = b1.x + zv.z; o.w = b1.y + zv.w;
        c64m_st(d, e, o, r0, r1);
    }
};

// a factor as M (IC(0), applied k wide by csr_tri_multi.hip): the update and the sums are two passes with the apply's launches between them
struct C64MOpFRes {     // r = B - Ad
    static constexpr int NS = 0;
    const float *Ad, *B; float *r;
    __device__ void prep(const C64MState &, int) {}
    __device__ void apply(long e, long, bool r0, bool r1, m2d *)
    {
        const float2 m1 = make_float2(-1.f, 0.f);
        const c64v4 av = c64m_ld(Ad, e), bv = c64m_ld(B, e);
        c64m_st(r, e, c64m_join(c64m_axpy(m1, c64m_lo(av), c64m_lo(bv)), c64m_axpy(m1, c64m_hi(av), c64m_hi(bv))), r0, r1);
    }
};
struct C64MOpFInit {    // d = z; |m|^2, |r|^2, r.z
    static constexpr int NS = 4;
    const float *m, *r, *z; float *d;
    __device__ void prep(const C64MState &, int) {}
    __device__ void apply(long e, long, bool r0, bool r1, m2d *acc)
    {
        const c64v4 zv = c64m_ld(z, e);
        c64m_st(d, e, zv, r0, r1);
        c64m_sums(acc, c64m_ld(m, e), c64m_ld(r, e), zv);
    }
};
struct C64MOpFUpdate {  // m += ak d; r -= ak Ad
    static constexpr int NS = 0;
    float *m, *r; const float *d, *Ad; float2 ak0, ak1;
    __device__ void prep(const C64MState &L, int c) { ak0 = c64m_get(L.ak, c); ak1 = c64m_get(L.ak, c + 1); }
    __device__ void apply(long e, long, bool r0, bool r1, m2d *)
    {
        const c64v4 dv = c64m_ld(d, e), av = c64m_ld(Ad, e), mo = c64m_ld(m, e), ro = c64m_ld(r, e);
        const float2 n0 = make_float2(-ak0.x, -ak0.y), n1 = make_float2(-ak1.x, -ak1.y);
        c64m_st(m, e, c64m_join(c64m_axpy(ak0, c64m_lo(dv), c64m_lo(mo)), c64m_axpy(ak1, c64m_hi(dv), c64m_hi(mo))), r0, r1);
        c64m_st(r, e, c64m_join(c64m_axpy(n0, c64m_lo(av), c64m_lo(ro)), c64m_axpy(n1, c64m_hi(av), c64m_hi(ro))), r0, r1);
    }
};
struct C64MOpFSums {    // |m|^2, |r|^2, r.s
    static constexpr int NS = 4;
    const float *m, *r, *s;
    __device__ void prep(const C64MState &, int) {}
    __device__ void apply(long e, long, bool, bool, m2d *acc) { c64m_sums(acc, c64m_ld(m, e), c64m_ld(r, e), c64m_ld(s, e)); }
};

// ---- host side --------------------------------------------------------------------------------------------------------------------------
inline int c64m_code(int stop)
{
    switch (stop) {
    case ST_ALREADY: return CLCG_ALREADY_OPTIMIZIED;
    case ST_NAN: return CLCG_NAN_VALUE;
    case ST_CONVERGED: return CLCG_CONVERGENCE;
    default: return LCG_REACHED_MAX_ITERATIONS;     // (-1019 from the real enum, as the complex loops return at the cap: SURVEY quirk 5)
    }
}

// The matrix as the loop sees it (multi_ops.hpp's operators in complex64): rows(), inv() (the complex64 Jacobi reciprocals, null without
// Jacobi), factor() (the complex64 IC(0) factor that is M -- PCG only, its k-wide work vectors reserved by the caller -- or null),
// big_doubles(k) and apply(): Y = A.X for the K columns and, with U, column j's unconjugated (A.X)_j . U_j as *slots partial sums in
// `dots` (rows 2 j, 2 j + 1).
struct C64CsrOp {
    lcg_hip_csr *A;
    const float *invdiag;
    const TriFactor *F;
    int rows() const { return A->n_rows; }
    const float *inv() const { return invdiag; }
    const TriFactor *factor() const { return F; }
    size_t big_doubles(int k) const { return cspmm_c64_big_doubles(A->main, k); }
    int apply(Ctx &c, int k, const float *X, float *Y, const int *done, const float *U, double *big, double *dots, int *slots) const
    {
        c.cnt_ax++;
        return cspmm_c64_launch(A->main, k, X, Y, c.stream, done, U, big, dots, slots);
    }
};
// a square complex64 dense handle (dense_c64.hip): the product is one to three launches, all counted as products
struct C64DenseOp {
    lcg_hip_dense *D;
    int rows() const { return D->N; }
    const float *inv() const { return reinterpret_cast<const float *>(D->invdiag); }
    const TriFactor *factor() const { return nullptr; }
    size_t big_doubles(int) const { return 0; }
    int apply(Ctx &c, int k, const float *X, float *Y, const int *done, const float *U, double *, double *dots, int *slots) const
    {
        int launches = 0;
        const int rc = cdnm_op(D, k, X, Y, c.stream, done, U, dots, slots, &launches);
        c.cnt_ax += launches;
        return rc;
    }
};

template <int K, bool PCG, class Op>
static int run_c64m(const Op &A, float *M, const float *B, const clcg_para &p, int *ret, int *iterations, double *residual, int mem)
{
    const float *inv = A.inv();
    const TriFactor *F = A.factor();
    MultiFrame<C64MState, K, K / 2> f(A.rows());
    Ctx &c = f.c;
    {   // (the frame moves blocks as 16-byte pieces behind double pointers)
        double *Md = reinterpret_cast<double *>(M);
        const double *Bd = reinterpret_cast<const double *>(B);
        TRY(f.open(mem, Md, Bd));
        M = reinterpret_cast<float *>(Md); B = reinterpret_cast<const float *>(Bd);
    }
    auto vec = [&](float *&out) -> int { double *v = nullptr; TRY(f.vec(v)); out = reinterpret_cast<float *>(v); return 0; };
    float *r = nullptr, *d = nullptr, *Ad = nullptr, *s = nullptr;
    double *big = nullptr;
    TRY(vec(r));
    TRY(vec(d));
    TRY(vec(Ad));
    if (PCG) TRY(vec(s));
    const size_t nbig = A.big_doubles(K);
    if (nbig) TRY(f.ws.get(big, nullptr, sizeof(double) * nbig));
    TRY(f.start(f.tree_grid(), p.epsilon, p.abs_diff));
    auto product = [&](const float *X, float *Y, const int *done, const float *U, double *dots, int *slots) -> int {
        return A.apply(c, K, X, Y, done, U, big, dots, slots);
    };

    // setup: A.m for the guess, d = r (PCG: inv .* r), the verdict "already optimised"
    TRY(product(M, Ad, nullptr, nullptr, nullptr, nullptr));
    const int m_launches = PCG && F ? tri_apply_launches(F, 2) : 0;         // counted as vector passes (lcg_hip_last_launches)
    auto factor = [&](const int *done) -> int {                              // s = (L.L^T)^-1 r for all K columns
        c.cnt_vec += m_launches;
        return tri_apply_multi(F, K, 2, reinterpret_cast<const double *>(r), reinterpret_cast<double *>(s), c.stream, done);
    };
    if (PCG && F) {
        TRY((f.template pass<0, true>(MFinNone{}, C64MOpFRes{Ad, B, r}, nullptr, 0)));
        TRY(factor(nullptr));
        TRY((f.template pass<1, true>(MFinNone{}, C64MOpFInit{M, r, s, d}, nullptr, 0)));
    } else
        TRY((f.template pass<1, true>(MFinNone{}, C64MOpInit<PCG>{Ad, B, M, inv, r, d}, nullptr, 0)));
    TRY((f.template pass<3, true>(C64MFinInit<K>{}, MOpNone{}, f.tab_sum, f.grid, 1)));

    int g_dot = 0;
    f.run(p.max_iterations, [&]() -> int {
        TRY(product(d, Ad, &f.cur->all_done, d, f.tab_dot, &g_dot));
        if (PCG && F) {
            TRY(f.template pass<0>(C64MFinAlpha<K>{}, C64MOpFUpdate{M, r, d, Ad, float2(), float2()}, f.tab_dot, g_dot));
            TRY(factor(&f.cur->all_done));
            TRY(f.template pass<1>(MFinNone{}, C64MOpFSums{M, r, s}, nullptr, 0));
        } else
            TRY(f.template pass<1>(C64MFinAlpha<K>{}, C64MOpUpdate<PCG>{M, r, s, d, Ad, inv, float2(), float2()}, f.tab_dot, g_dot));
        TRY(f.template pass<3>(C64MFinClose<K>{}, C64MOpDir{d, PCG ? s : r, float2(), float2()}, f.tab_sum, f.grid));
        return 0;
    });
    return f.finish(c64m_code, ret, iterations, residual);
}

template <bool PCG>
static int c64m_entry(const char *entry, lcg_hip_csr *A, int k, float *M, const float *B, const clcg_para *param, int *ret, int *iterations,
                      double *residual, int mem)
{
    clcg_para p;
    TRY(multi_args(entry, k, M, B));
    TRY(c64multi_handle(entry, A));
    TRY(multi_shape(entry, A->n_rows == A->n_cols, mem));
    TRY(multi_para<true>(param, p, A->n_rows));
    const float *inv = PCG ? c64_builtin_invdiag((const void *)clcg_hip_jacobi_mx_c64, A, A->n_rows) : nullptr;
    if (PCG && inv == nullptr) return LCG_NULL_PRECONDITION_MATRIX;     // lcg_hip_csr_build_jacobi has not run
    TRY(ensure_init());
    const C64CsrOp op{A, inv, nullptr};
    return multi_k(k, [&](auto K) { return run_c64m<decltype(K)::value, PCG>(op, M, B, p, ret, iterations, residual, mem); });
}

// the dense entries: A = K, square; PCG with the reciprocals of lcg_hip_dense_build_jacobi_c64
template <bool PCG>
static int c64m_dense_entry(const char *entry, const void *Kh, int k, float *M, const float *B, const clcg_para *param, int *ret,
                            int *iterations, double *residual, int mem)
{
    clcg_para p;
    TRY(multi_args(entry, k, M, B));
    lcg_hip_dense *D = cdn_handle(entry, Kh);
    if (!D) return LCG_HIP_E_ARG;
    TRY(multi_shape(entry, D->M == D->N, mem));
    TRY(multi_para<true>(param, p, D->N));
    if (PCG && D->invdiag == nullptr) return LCG_NULL_PRECONDITION_MATRIX;  // lcg_hip_dense_build_jacobi_c64 has not run
    TRY(ensure_init());
    TRY(cdnm_reserve(D, k));
    const C64DenseOp op{D};
    return multi_k(k, [&](auto K) { return run_c64m<decltype(K)::value, PCG>(op, M, B, p, ret, iterations, residual, mem); });
}

// precond: LCG_HIP_M_JACOBI (clcg_hip_lpcg_multi_c64 itself) or LCG_HIP_M_IC0 (the handle's complex64 factor)
static int c64m_entry_m(const char *entry, lcg_hip_csr *A, int k, int precond, float *M, const float *B, const clcg_para *param, int *ret,
                        int *iterations, double *residual, int mem)
{
    clcg_para p;
    TRY(multi_args(entry, k, M, B));
    TRY(c64multi_handle(entry, A));
    TRY(multi_shape(entry, A->n_rows == A->n_cols, mem));
    if (precond != LCG_HIP_M_JACOBI && precond != LCG_HIP_M_IC0)
        return arg_error("%s: precond = %d is neither LCG_HIP_M_JACOBI nor LCG_HIP_M_IC0 (there is no complex64 ILU(0), and PCG needs an M)", entry, precond);
    if (precond == LCG_HIP_M_JACOBI) return c64m_entry<true>(entry, A, k, M, B, param, ret, iterations, residual, mem);
    TRY(multi_para<true>(param, p, A->n_rows));
    TriFactor *F = A->ic0;
    if (!F || !F->ok || !F->c64) return LCG_NULL_PRECONDITION_MATRIX;   // lcg_hip_csr_build_ic0_c64 has not run (or its pivot failed)
    TRY(ensure_init());
    TRY(tri_multi_reserve(F, k, 2));
    const C64CsrOp op{A, nullptr, F};
    return multi_k(k, [&](auto K) { return run_c64m<decltype(K)::value, true>(op, M, B, p, ret, iterations, residual, mem); });
}

} // namespace
} // namespace lcgh

using namespace lcgh;

extern "C" {

int clcg_hip_lbicg_sym_multi_c64(lcg_hip_csr_t A, int k, float *M, const float *B, const clcg_para *param, int *ret, int *iterations,
                                 double *residual, int mem)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return c64m_entry<false>("clcg_hip_lbicg_sym_multi_c64", A, k, M, B, param, ret, iterations, residual, mem);
}

int clcg_hip_lpcg_multi_c64(lcg_hip_csr_t A, int k, float *M, const float *B, const clcg_para *param, int *ret, int *iterations,
                            double *residual, int mem)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return c64m_entry<true>("clcg_hip_lpcg_multi_c64", A, k, M, B, param, ret, iterations, residual, mem);
}

int clcg_hip_lpcg_multi_m_c64(lcg_hip_csr_t A, int k, int precond, float *M, const float *B, const clcg_para *param, int *ret,
                              int *iterations, double *residual, int mem)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return c64m_entry_m("clcg_hip_lpcg_multi_m_c64", A, k, precond, M, B, param, ret, iterations, residual, mem);
}

int clcg_hip_dense_lbicg_sym_multi_c64(lcg_hip_dense_t K, int k, float *M, const float *B, const clcg_para *param, int *ret, int *iterations,
                                       double *residual, int mem)
{
    return c64m_dense_entry<false>("clcg_hip_dense_lbicg_sym_multi_c64", K, k, M, B, param, ret, iterations, residual, mem);
}

int clcg_hip_dense_lpcg_multi_c64(lcg_hip_dense_t K, int k, float *M, const float *B, const clcg_para *param, int *ret, int *iterations,
                                  double *residual, int mem)
{
    return c64m_dense_entry<true>("clcg_hip_dense_lpcg_multi_c64", K, k, M, B, param, ret, iterations, residual, mem);
}

} // extern "C"
