// solvers_multi_bicg.hip -- batched BiCGStab over k = 2, 4, 8 right-hand sides, plain or right-preconditioned: lcg_hip_lbicgstab_multi.
//
// Each column runs the reference's lbicgstab as if it were alone (lcg.cpp:629-794): its own ak, wk, betak and rkr0_T, the same
// set-up r0_T = p = r = B - A.m, both "already optimised" criteria in the reference's order, the stop test at the loop head, the
// NaN scan of m after the update, its own count and code.  What the columns share is the matrix -- and the preconditioner: both
// products of an iteration (csr_multi.hip) and both applies (csr_tri_multi.hip) read their arrays once for all of them.
//
// Plain (LCG_HIP_M_NONE), two products and three k-wide passes per iteration, the scalar steps in the passes' prologues
// (multi_loop.hpp: k_mvecf):
//     v = A.p carrying v.r0  |  [ak = rho / v.r0] s = r - ak v  |  t = A.s carrying t.s, t.t (k_spmm<DOT = 2>)
//     |  [wk = t.s / t.t] m += ak p + wk s; r = s - wk t + m.m, r.r, r.r0, NaN  |  [close] p = r + betak (p - wk v)
//
// Preconditioned (LCG_HIP_M_JACOBI, _IC0, _ILU0): right preconditioning carried in x-space.  M holds the solution itself, the
// stop rule sees |m|, nothing is applied after the loop:
//     ph = M^-1 p; v = A.ph carrying v.r0; s = r - ak v; sh = M^-1 s; t = A.sh carrying t.s, t.t;
//     m += ak ph + wk sh; r = s - wk t; p = r + betak (p - wk v)
// In exact arithmetic the residuals are those of A.M^-1 u = b - A.m0 from u = 0, and m = m0 + M^-1 u.  With a factor the two
// applies are tri_apply_multi's launches (each honours all_done); with Jacobi ph and sh are formed by the passes that write p and s.
//
// Column j's results are the same bits whatever k is: the products' sums are added in an order the matrix fixes, the passes' sums
// as one binary tree over leaves that depend on n alone (multi_loop.hpp: TREE, multi.hpp: msum_tree, tree_leaves).
//
// Frozen columns as in solvers_multi.hip: a stopped column's columns of m, r, p, s (ph, sh) are never stored to again, by a select
// on its stop word; the products and applies still form such a column's v, t, ph, sh where they write whole rows, and nothing
// reads them.  Breakdowns are the reference's: v.r0 = 0 or t.t = 0 make the coefficient Inf / NaN, the NaN scan of m ends that
// column with LCG_NAN_VALUE at the iteration in which the NaN appeared (t after its t++), and no other column sees it.
#include "multi_loop.hpp"
#include "csr_tri.hpp"

namespace lcgh {
namespace {

struct BState : MultiHead {
    double ak[MM_MAXK], wk[MM_MAXK], bk[MM_MAXK], rho[MM_MAXK], m2[MM_MAXK], r2[MM_MAXK], residual[MM_MAXK];
};

// ---- scalar steps ---------------------------------------------------------------------------------------------------------------------
// setup: |m|^2 (clamped), r.r, rkr0_T (= r.r: r0_T is r, added in the same order); "already optimised" per column, in abs_diff mode
// BOTH criteria in this order (lcg.cpp:658-689).  Sums m.m, r.r
template <int K> struct BFinInit {
    static constexpr int NS = 2;
    __device__ void operator()(BState *st, const double *sum) const
    {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double m2 = clamp1(sum[j]), r2 = sum[K + j];
            st->m2[j] = m2; st->r2[j] = r2; st->rho[j] = r2;
            m_already(st, j, r2, m2);
        }
        all_stopped<K>(st);
        mpublish(st);
    }
};
// first step of a body: counts it; ak = rkr0_T / Apk.r0_T per running column (lcg.cpp:720-725)
template <int K> struct BFinAlpha {
    static constexpr int NS = 1;
    __device__ void operator()(BState *st, const double *sum) const
    {
        st->it++;
        if (st->all_done) return;
#pragma unroll
        for (int j = 0; j < K; j++) if (st->stop[j] == ST_RUNNING) st->ak[j] = st->rho[j] / sum[j];
    }
};
// wk = Ass / AsAs per running column (lcg.cpp:735-741).  Sums t.s, t.t (the second product's)
template <int K> struct BFinOmega {
    static constexpr int NS = 2;
    __device__ void operator()(BState *st, const double *sum) const
    {
        if (st->all_done) return;
#pragma unroll
        for (int j = 0; j < K; j++) if (st->stop[j] == ST_RUNNING) st->wk[j] = sum[j] / sum[K + j];
    }
};
// closing step of a body, per running column (lcg.cpp:749-774, and the next loop head's test :694-708).  Sums m.m, r.r, r.r0, NaN count
template <int K> struct BFinClose {
    static constexpr int NS = 4;
    __device__ void operator()(BState *st, const double *sum) const
    {
        if (!st->all_done) {
#pragma unroll
            for (int j = 0; j < K; j++) {
                if (st->stop[j] != ST_RUNNING) continue;
                const double mm = sum[j], r2 = sum[K + j], rho_new = sum[2 * K + j], nan = sum[3 * K + j];
                st->m2[j] = clamp1(mm);
                st->t[j]++;
                if (nan > 0.0 || mm != mm) { st->stop[j] = ST_NAN; continue; }
                st->bk[j] = (st->ak[j] / st->wk[j]) * rho_new / st->rho[j];
                st->rho[j] = rho_new;
                st->r2[j] = r2;
                const double r = m_residual(st, r2, st->m2[j]);
                st->residual[j] = r;
                if (r <= st->eps) st->stop[j] = ST_CONVERGED;
            }
            all_stopped<K>(st);
        }
        mpublish(st);
    }
};

// ---- vector passes (JAC: ph = p / diag and sh = s / diag are written beside p and s) --------------------------------------------------
template <bool JAC> struct BOpInit {       // r0 = p = r = B - Ad [ph = p / diag]; m.m, r.r        lcg.cpp:650-669
    static constexpr int NS = 2;
    const double *Ad, *B, *m, *invdiag; double *r, *r0, *p, *ph;
    __device__ void prep(const BState &, int) {}
    __device__ void apply(long e, long row, bool r0_, bool r1_, m2d *acc)
    {
        const m2d rv = ld2(B, e) - ld2(Ad, e), mv = ld2(m, e);
        st2(r, e, rv, r0_, r1_); st2(r0, e, rv, r0_, r1_); st2(p, e, rv, r0_, r1_);
        if (JAC) st2(ph, e, invdiag[row] * rv, r0_, r1_);
        acc[0] += mv * mv; acc[1] += rv * rv;
    }
};
template <bool JAC> struct BOpS {          // s = r - ak v [sh = s / diag]                         lcg.cpp:727-731
    static constexpr int NS = 0;
    const double *r, *v, *invdiag; double *s, *sh; m2d ak;
    __device__ void prep(const BState &L, int c0) { ak.x = L.ak[c0]; ak.y = L.ak[c0 + 1]; }
    __device__ void apply(long e, long row, bool r0_, bool r1_, m2d *)
    {
        const m2d sv = ld2(r, e) - ak * ld2(v, e);
        st2(s, e, sv, r0_, r1_);
        if (JAC) st2(sh, e, invdiag[row] * sv, r0_, r1_);
    }
};
struct BOpUpdate {      // m += ak ph + wk sh; r = s - wk t; m.m, r.r, r.r0, NaN                    lcg.cpp:743-772
    static constexpr int NS = 4;
    double *m, *r; const double *ph, *sh, *s, *t, *r0; m2d ak, wk;
    __device__ void prep(const BState &L, int c0) { ak.x = L.ak[c0]; ak.y = L.ak[c0 + 1]; wk.x = L.wk[c0]; wk.y = L.wk[c0 + 1]; }
    __device__ void apply(long e, long, bool r0_, bool r1_, m2d *acc)
    {
        const m2d mv = ld2(m, e) + (ak * ld2(ph, e) + wk * ld2(sh, e));
        const m2d rv = ld2(s, e) - wk * ld2(t, e);
        st2(m, e, mv, r0_, r1_); st2(r, e, rv, r0_, r1_);
        acc[0] += mv * mv; acc[1] += rv * rv; acc[2] += rv * ld2(r0, e); acc[3] += nan2(mv);
    }
};
template <bool JAC> struct BOpDir {        // p = r + betak (p - wk v) [ph = p / diag]             lcg.cpp:776-780
    static constexpr int NS = 0;
    double *p, *ph; const double *r, *v, *invdiag; m2d bk, wk;
    __device__ void prep(const BState &L, int c0) { bk.x = L.bk[c0]; bk.y = L.bk[c0 + 1]; wk.x = L.wk[c0]; wk.y = L.wk[c0 + 1]; }
    __device__ void apply(long e, long row, bool r0_, bool r1_, m2d *)
    {
        const m2d pv = ld2(r, e) + bk * (ld2(p, e) - wk * ld2(v, e));
        st2(p, e, pv, r0_, r1_);
        if (JAC) st2(ph, e, invdiag[row] * pv, r0_, r1_);
    }
};

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// The passes' TREE (multi_loop.hpp) -- 1: the pass leaves sums, 2: it adds up a pass's sums (the products' sums are msum's: their order
// is the matrix's alone)
template <int K, bool JAC>
static int run_bicg(lcg_hip_csr *A, const TriFactor *F, double *M, const double *B, const lcg_para &p, int *ret, int *iterations,
                    double *residual, int mem)
{   // F: the factor that is M (its k-wide work vectors reserved by the caller); JAC: the handle's Jacobi diagonal; neither: plain
    MultiFrame<BState, K, K / 2> f(A->n_rows);
    Ctx &c = f.c;
    TRY(f.open(mem, M, B));
    double *r = nullptr, *r0 = nullptr, *pk = nullptr, *s = nullptr, *v = nullptr, *t = nullptr, *ph = nullptr, *sh = nullptr, *big = nullptr;
    TRY(f.vec(r));
    TRY(f.vec(r0));
    TRY(f.vec(pk));
    TRY(f.vec(s));
    TRY(f.vec(v));
    TRY(f.vec(t));
    if (JAC || F) { TRY(f.vec(ph)); TRY(f.vec(sh)); }
    else { ph = pk; sh = s; }
    const size_t nbig = spmm_big_doubles(A->main, K, true);
    if (nbig) TRY(f.ws.get(big, nullptr, sizeof(double) * nbig));
    TRY(f.start(f.tree_grid(), p.epsilon, p.abs_diff));

    // setup (lcg.cpp:650-689): A.m for the guess, r0 = p = r, the verdict "already optimised"
    const CsrPart &P = A->main;
    c.cnt_ax++;
    TRY(spmm_launch(P, K, M, t, c.stream, nullptr));
    TRY((f.template pass<1, true>(MFinNone{}, BOpInit<JAC>{t, B, M, A->invdiag, r, r0, pk, ph}, nullptr, 0)));
    TRY((f.template pass<2, true>(BFinInit<K>{}, MOpNone{}, f.tab_sum, f.grid, 1)));

    const int m_launches = F ? tri_apply_launches(F, 2) : 0;       // counted as vector passes (lcg_hip_last_launches)
    int g_dot = 0, g_dot2 = 0;
    f.run(p.max_iterations, [&]() -> int {
        if (F) { c.cnt_vec += m_launches; TRY(tri_apply_multi(F, K, 2, pk, ph, c.stream, &f.cur->all_done)); }
        c.cnt_ax++;
        TRY(spmm_launch(P, K, ph, v, c.stream, &f.cur->all_done, r0, big, f.tab_dot, &g_dot));                      // :718-724
        TRY(f.template pass<0>(BFinAlpha<K>{}, BOpS<JAC>{r, v, A->invdiag, s, sh, m2d()}, f.tab_dot, g_dot));                     // :725-731
        if (F) { c.cnt_vec += m_launches; TRY(tri_apply_multi(F, K, 2, s, sh, c.stream, &f.cur->all_done)); }
        c.cnt_ax++;
        TRY(spmm_launch(P, K, sh, t, c.stream, &f.cur->all_done, s, big, f.tab_dot, &g_dot2, true));                // :733-740
        TRY(f.template pass<1>(BFinOmega<K>{}, BOpUpdate{M, r, ph, sh, s, t, r0, m2d(), m2d()}, f.tab_dot, g_dot2));              // :741-772
        TRY(f.template pass<2>(BFinClose<K>{}, BOpDir<JAC>{pk, ph, r, v, A->invdiag, m2d(), m2d()}, f.tab_sum, f.grid));          // :773-780
        return 0;
    });
    return f.finish(lcg_code, ret, iterations, residual);
}

} // namespace
} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_lbicgstab_multi(lcg_hip_csr_t A, int k, int precond, double *M, const double *B, const lcg_para *param, int *ret,
                            int *iterations, double *residual, int mem)
{
    static const char *entry = "lcg_hip_lbicgstab_multi";
    lcg_para p;
    MultiPrecond m;
    NOT_DENSE(A, LCG_HIP_E_ARG);
    TRY(multi_args(entry, k, M, B));
    TRY(multi_handle(entry, A));
    TRY(multi_shape(entry, A->n_rows == A->n_cols, mem));
    TRY(multi_precond(entry, A, precond, true, true, m));
    TRY(multi_para<false>(param, p, A->n_rows));
    if (!m.built) return LCG_NULL_PRECONDITION_MATRIX;
    TRY(ensure_init());
    if (m.F) TRY(tri_multi_reserve(m.F, k, 2));
    return multi_k(k, [&](auto K) {
        return m.jac ? run_bicg<decltype(K)::value, true>(A, m.F, M, B, p, ret, iterations, residual, mem)
                     : run_bicg<decltype(K)::value, false>(A, m.F, M, B, p, ret, iterations, residual, mem);
    });
}

} // extern "C"
