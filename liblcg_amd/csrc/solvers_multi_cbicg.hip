// solvers_multi_cbicg.hip -- batched complex BiCGStab over k = 2, 4, 8 right-hand sides against one square complex128 matrix, symmetric
// or not, plain or right-preconditioned with the Jacobi diagonal: clcg_hip_lbicgstab_multi (clbicgstab, clcg.cpp:524-679).
//
// Each column runs the reference's recurrence as if it were alone: r = p = B - A.m, rho = <rbar0, r>, both "already optimised"
// criteria in the reference's order, the 4th-power stop rule at the loop head (multi_cplx.hpp: zm_residual<false>), ak = rho / <rbar0,
// A.p>, wk = <A.s, s> / <A.s, A.s>, the NaN scan of m through sum |m|^2, betak = rho' ak / (rho wk) in FinZClose<2>'s order
// (solvers_cplx.hip), its own count and code.  The inner products are CONJUGATED in their first argument (clcg_inner).  What the
// columns share is the matrix -- both products of an iteration (csr_multi_cplx.hip) read col / val once for all of them -- and the
// shadow residual: ONE vector of n, make_shadow's (solvers_cplx.hip), so a column sees the rbar0 that clcg_hip_solver(CLCG_BICGSTAB)
// sees at the same seed.
// No redraw of rbar0, as in the single-vector loop: the reference redraws while |rho| < 1e-8 and spins for ever on r = 0
// (clcg.cpp:556-561); here the "already optimised" tests run first and a zero column ends with code 2 at count 0.
//
// Plain (LCG_HIP_M_NONE), two products and three k-wide passes per iteration, the scalar steps in the passes' prologues
// (multi_loop.hpp: k_mvecf):
//     v = A.p carrying <rb,v> (CSPMM_INNER)  |  [ak] s = r - ak v  |  t = A.s carrying <t,s>, |t|^2 (CSPMM_DOT2)
//     |  [wk] m += ak p + wk s; r = s - wk t + |m|^2, |r|^2, <rb,r>  |  [close] p = r + betak (p - wk v)
// LCG_HIP_M_JACOBI: right preconditioning carried in x-space as solvers_multi_bicg.hip carries it: ph = p ./ diag and sh = s ./ diag
// are written by the passes that write p and s (the complex reciprocals of lcg_hip_csr_build_jacobi), v = A.ph, t = A.sh,
// m += ak ph + wk sh.  M holds the solution itself; nothing is applied after the loop.
//
// Frozen columns, breakdowns and the NaN rule are solvers_multi_cplx.hip's: a thread whose column has stopped does nothing -- a select
// on the stop word -- so its elements of m, r, p, s (ph, sh) are never stored to again; the products still form such a column's v and
// t, which nothing reads.  <rb,v> = 0 or t = 0 make the coefficient Inf / NaN, the NaN reaches m in that iteration or the next, and
// the column ends with CLCG_NAN_VALUE at the iteration in which sum |m|^2 turned NaN (t after its t++): one NaN column never keeps
// a batch alive at max_iterations = 0.
//
// Column j's results are the same bits whatever k is and wherever it stands: the products' sums are added in an order the matrix
// fixes (msum), the passes' sums as ONE binary tree over leaves that depend on n alone (multi.hpp: tree_leaves, msum_tree).  Table
// rows as in solvers_multi_cplx.hip; the second product's third sum |t|^2 of column j lies in row 2 K + j.
#include "multi_cplx.hpp"
#include "lcg_hip_staging.h"

namespace lcgh {
namespace {

struct ZBState : ZMState {
    double wk[2 * MM_MAXK];
};

// ---- scalar steps (setup: ZMFinInit<K, false>; first step of a body: ZMFinAlpha<K>) ---------------------------------------------------
// wk = <t,s> / <t,t> per running column (clcg.cpp:631-633; FinZOmega).  Sums: the second product's, <t,s> in rows 2 j, 2 j + 1 and the
// real <t,t> in row 2 K + j
template <int K> struct ZBFinOmega {
    static constexpr int NS = 3;
    __device__ void operator()(ZBState *st, const double *sum) const
    {
        if (st->all_done) return;
#pragma unroll
        for (int j = 0; j < K; j++)
            if (st->stop[j] == ST_RUNNING) zsts(st->wk, j, cdiv(make_double2(sum[2 * j], sum[2 * j + 1]), make_double2(sum[2 * K + j], 0.0)));
    }
};
// closing step of a body, per running column (clcg.cpp:635-659 and the next loop head :594-617).  Sums |m|^2, |r|^2, <rb,r>
template <int K> struct ZBFinClose {
    static constexpr int NS = 4;
    __device__ void operator()(ZBState *st, const double *sum) const
    {
        if (!st->all_done) {
#pragma unroll
            for (int j = 0; j < K; j++) {
                if (st->stop[j] != ST_RUNNING) continue;
                const double mm = sum[2 * j], r2 = sum[2 * j + 1];
                const double2 nw = make_double2(sum[(K + j) * 2], sum[(K + j) * 2 + 1]);
                st->m2[j] = mm; st->r2[j] = r2;
                st->t[j]++;
                if (mm != mm) { st->stop[j] = ST_NAN; continue; }
                zsts(st->bk, j, cdiv(cmul(nw, zld(st->ak, j)), cmul(zld(st->rho, j), zld(st->wk, j))));    // clcg.cpp:658
                zsts(st->rho, j, nw);
                const double r = zm_residual<false>(st, r2, mm);
                st->residual[j] = r;
                if (r <= st->eps) st->stop[j] = ST_CONVERGED;
            }
            all_stopped<K>(st);
        }
        mpublish(st);
    }
};

// ---- vector passes (JAC: ph = p / diag and sh = s / diag are written beside p and s; rb: one element per row) ---------------------------
__device__ __forceinline__ m2d zcoef(const double *a, int c) { m2d v; v.x = a[2 * c]; v.y = a[2 * c + 1]; return v; }

template <bool JAC> struct ZBOpInit {      // p = r = B - Ad [ph = p / diag]; |m|^2, |r|^2, <rb,r>           clcg.cpp:548-572
    static constexpr int NS = 2;
    const double *Ad, *B, *m, *rb, *invdiag; double *r, *p, *ph;
    __device__ void prep(const ZBState &, int) {}
    __device__ void apply(long e, long row, bool, bool, m2d *acc)
    {
        const m2d rv = ld2(B, e) - ld2(Ad, e), mv = ld2(m, e);
        zst(r, e, rv); zst(p, e, rv);
        if (JAC) zst(ph, e, zmul(ld2(invdiag, row), rv));
        acc[0] += znorms(mv, rv); acc[1] += zinner(ld2(rb, row), rv);
    }
};
template <bool JAC> struct ZBOpS {         // s = r - ak v [sh = s / diag]                                   clcg.cpp:624-628
    static constexpr int NS = 0;
    const double *r, *v, *invdiag; double *s, *sh; m2d ak;
    __device__ void prep(const ZBState &L, int c) { ak = zcoef(L.ak, c); }
    __device__ void apply(long e, long row, bool, bool, m2d *)
    {
        const m2d sv = zfma(-ak, ld2(v, e), ld2(r, e));
        zst(s, e, sv);
        if (JAC) zst(sh, e, zmul(ld2(invdiag, row), sv));
    }
};
struct ZBOpUpdate {     // m += ak ph + wk sh; r = s - wk t; |m|^2, |r|^2, <rb,r>                           clcg.cpp:635-657
    static constexpr int NS = 2;
    double *m, *r; const double *ph, *sh, *s, *t, *rb; m2d ak, wk;
    __device__ void prep(const ZBState &L, int c) { ak = zcoef(L.ak, c); wk = zcoef(L.wk, c); }
    __device__ void apply(long e, long row, bool, bool, m2d *acc)
    {
        const m2d mv = zfma(wk, ld2(sh, e), zfma(ak, ld2(ph, e), ld2(m, e)));
        const m2d rv = zfma(-wk, ld2(t, e), ld2(s, e));
        zst(m, e, mv); zst(r, e, rv);
        acc[0] += znorms(mv, rv); acc[1] += zinner(ld2(rb, row), rv);
    }
};
template <bool JAC> struct ZBOpDir {       // p = r + betak (p - wk v) [ph = p / diag]                       clcg.cpp:661-665
    static constexpr int NS = 0;
    double *p, *ph; const double *r, *v, *invdiag; m2d bk, wk;
    __device__ void prep(const ZBState &L, int c) { bk = zcoef(L.bk, c); wk = zcoef(L.wk, c); }
    __device__ void apply(long e, long row, bool, bool, m2d *)
    {
        const m2d pv = zfma(bk, zfma(-wk, ld2(v, e), ld2(p, e)), ld2(r, e));
        zst(p, e, pv);
        if (JAC) zst(ph, e, zmul(ld2(invdiag, row), pv));
    }
};

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// The passes' TREE (multi_loop.hpp) -- 1: the pass leaves sums, 2: it adds up a pass's sums (the products' sums are msum's: their order
// is the matrix's alone)
template <int K, bool JAC>
static int run_zbicg(lcg_hip_csr *A, double *M, const double *B, const clcg_para &p, int *ret, int *iterations, double *residual, int mem)
{
    MultiFrame<ZBState, K, K> f(A->n_rows);
    Ctx &c = f.c;
    TRY(f.open(mem, M, B));
    double *r = nullptr, *pk = nullptr, *s = nullptr, *v = nullptr, *t = nullptr, *ph = nullptr, *sh = nullptr, *rb = nullptr, *big = nullptr;
    TRY(f.vec(r));
    TRY(f.vec(pk));
    TRY(f.vec(s));
    TRY(f.vec(v));
    TRY(f.vec(t));
    if (JAC) { TRY(f.vec(ph)); TRY(f.vec(sh)); }
    else { ph = pk; sh = s; }
    TRY(f.ws.get(rb, nullptr, 16 * (size_t)A->n_rows));
    const CsrPart &P = A->main;
    const size_t nbig = cspmm_big_doubles(P, K, CSPMM_DOT2);       // (the larger of the two products' needs)
    if (nbig) TRY(f.ws.get(big, nullptr, sizeof(double) * nbig));
    TRY(f.start(f.tree_grid(), p.epsilon, p.abs_diff));
    TRY(make_shadow(c, A->n_rows, rb));                                                                             // clcg.cpp:556-561

    // setup (clcg.cpp:548-591): A.m for the guess, p = r, rho = <rb,r>, the verdict "already optimised"
    c.cnt_ax++;
    TRY(cspmm_launch(P, K, M, t, c.stream, nullptr));
    TRY((f.template pass<1, true>(MFinNone{}, ZBOpInit<JAC>{t, B, M, rb, A->invdiag, r, pk, ph}, nullptr, 0)));
    TRY((f.template pass<3, true>(ZMFinInit<K, false>{}, MOpNone{}, f.tab_sum, f.grid, 1)));

    int g_in = 0, g_d2 = 0;
    f.run(p.max_iterations, [&]() -> int {
        c.cnt_ax++;
        TRY(cspmm_launch(P, K, ph, v, c.stream, &f.cur->all_done, rb, big, f.tab_dot, &g_in, CSPMM_INNER));                 // :620-621
        TRY(f.template pass<0>(ZMFinAlpha<K>{}, ZBOpS<JAC>{r, v, A->invdiag, s, sh, m2d()}, f.tab_dot, g_in));             // :622-628
        c.cnt_ax++;
        TRY(cspmm_launch(P, K, sh, t, c.stream, &f.cur->all_done, s, big, f.tab_dot, &g_d2, CSPMM_DOT2));                   // :630-632
        TRY(f.template pass<1>(ZBFinOmega<K>{}, ZBOpUpdate{M, r, ph, sh, s, t, rb, m2d(), m2d()}, f.tab_dot, g_d2));        // :633-657
        TRY(f.template pass<3>(ZBFinClose<K>{}, ZBOpDir<JAC>{pk, ph, r, v, A->invdiag, m2d(), m2d()}, f.tab_sum, f.grid));  // :658-665
        return 0;
    });
    return f.finish(zm_code, ret, iterations, residual);
}

} // namespace
} // namespace lcgh

using namespace lcgh;

extern "C" {

int clcg_hip_lbicgstab_multi(lcg_hip_csr_t A, int k, int precond, double *M, const double *B, const clcg_para *param, int *ret,
                             int *iterations, double *residual, int mem)
{
    static const char *entry = "clcg_hip_lbicgstab_multi";
    clcg_para p;
    NOT_DENSE(A, LCG_HIP_E_ARG);
    TRY(multi_args(entry, k, M, B));
    TRY(cmulti_handle(entry, A));
    TRY(multi_shape(entry, A->n_rows == A->n_cols, mem));
    if (precond != LCG_HIP_M_NONE && precond != LCG_HIP_M_JACOBI) {
        ctx().err = std::string(entry) + ": precond is neither LCG_HIP_M_NONE nor LCG_HIP_M_JACOBI (there are no k-wide complex IC(0) / ILU(0) applies)";
        return LCG_HIP_E_ARG;
    }
    TRY(multi_para<true>(param, p, A->n_rows));
    if (precond == LCG_HIP_M_JACOBI && A->invdiag == nullptr) return LCG_NULL_PRECONDITION_MATRIX;     // lcg_hip_csr_build_jacobi has not run
    TRY(ensure_init());
    return multi_k(k, [&](auto K) {
        return precond == LCG_HIP_M_JACOBI ? run_zbicg<decltype(K)::value, true>(A, M, B, p, ret, iterations, residual, mem)
                                           : run_zbicg<decltype(K)::value, false>(A, M, B, p, ret, iterations, residual, mem);
    });
}

} // extern "C"
