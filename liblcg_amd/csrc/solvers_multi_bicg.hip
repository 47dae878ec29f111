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

struct BState {
    double ak[MM_MAXK], wk[MM_MAXK], bk[MM_MAXK], rho[MM_MAXK], m2[MM_MAXK], r2[MM_MAXK], residual[MM_MAXK];
    double eps, n_global;
    int t[MM_MAXK];         // completed iterations (the reference's t), per column
    int stop[MM_MAXK];      // ST_RUNNING, or why the column stopped (ST_CONVERGED, ST_NAN, ST_ALREADY)
    int abs_diff;
    int it;                 // iteration bodies started
    int all_done;           // every column has stopped: every later kernel is a no-op
    int pub_mask;           // HostStatus is refreshed when (it & pub_mask) == 0, and when all columns have stopped
    HostStatus *host;
};
static_assert(sizeof(BState) % 8 == 0, "BState is copied in 8-byte words");
constexpr size_t BSLOT = 1024;
static_assert(sizeof(BState) <= BSLOT, "two states share one small pool vector");

__global__ void k_binit(BState *st, double eps, double n_global, int abs_diff, int pub_mask, HostStatus *host)
{
    double *w = reinterpret_cast<double *>(st);
    for (int i = threadIdx.x; i < (int)(sizeof(BState) / 8); i += blockDim.x) w[i] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) { st->eps = eps; st->n_global = n_global; st->abs_diff = abs_diff; st->pub_mask = pub_mask; st->host = host; }
}

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
            double r;
            bool already = false;
            if (st->abs_diff && sqrt(r2) / st->n_global <= st->eps) { r = sqrt(r2) / st->n_global; already = true; }
            else if (r2 / m2 <= st->eps) { r = r2 / m2; already = true; }
            else r = st->abs_diff ? sqrt(r2) / st->n_global : r2 / m2;
            st->residual[j] = r;
            st->stop[j] = already ? ST_ALREADY : ST_RUNNING;
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
                const double r = st->abs_diff ? sqrt(r2) / st->n_global : r2 / st->m2[j];
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
template <int K>
struct BicgSolve {
    Ctx &c;
    long n2;
    int grid;
    BState *cur, *next;
    double *tab_dot, *tab_sum;      // the k-wide tables: the products' partial sums (v.r0; t.s and t.t), the update pass's

    // TREE: multi_loop.hpp -- 1: this pass leaves sums, 2: it adds up a pass's sums (the products' sums are msum's: their order is
    // the matrix's alone)
    template <int TREE, class Fin, class Op, bool ALL = false> int pass(Fin fin, Op op, const double *pin, int gin, int g = 0)
    {
        c.cnt_vec++;
        hipLaunchKernelGGL((k_mvecf<BState, K, Fin, Op, ALL, TREE>), dim3(g ? g : grid), dim3(VB), 0, c.stream, fin, op, n2, pin, gin, tab_sum, cur, next);
        HIPCHK(hipGetLastError());
        std::swap(cur, next);
        return 0;
    }
};

template <int K, bool JAC>
static int run_bicg(lcg_hip_csr *A, const TriFactor *F, double *M, const double *B, const lcg_para &p, int *ret, int *iterations,
                    double *residual, int mem)
{   // F: the factor that is M (its k-wide work vectors reserved by the caller); JAC: the handle's Jacobi diagonal; neither: plain
    Ctx &c = ctx();
    const int n = A->n_rows;
    const size_t nb = sizeof(double) * (size_t)n * K;
    HostBridge hb;
    Workspace ws;
    SolveGuard guard(c);
    TRY(hb.open(mem, M, B, nb, c.stream));
    double *r = nullptr, *r0 = nullptr, *pk = nullptr, *s = nullptr, *v = nullptr, *t = nullptr, *ph = nullptr, *sh = nullptr;
    double *big = nullptr, *stmem = nullptr;
    TRY(ws.get(r, nullptr, nb));
    TRY(ws.get(r0, nullptr, nb));
    TRY(ws.get(pk, nullptr, nb));
    TRY(ws.get(s, nullptr, nb));
    TRY(ws.get(v, nullptr, nb));
    TRY(ws.get(t, nullptr, nb));
    if (JAC || F) { TRY(ws.get(ph, nullptr, nb)); TRY(ws.get(sh, nullptr, nb)); }
    else { ph = pk; sh = s; }
    const size_t nbig = spmm_big_doubles(A->main, K, true);
    if (nbig) TRY(ws.get(big, nullptr, sizeof(double) * nbig));
    TRY(ws.get(stmem, nullptr, 2 * BSLOT));

    const CsrPart &P = A->main;
    BicgSolve<K> k{c, (long)n * (K / 2), 0, reinterpret_cast<BState *>(stmem),
                   reinterpret_cast<BState *>(reinterpret_cast<char *>(stmem) + BSLOT), c.partials_pair[0], c.partials_pair[1]};
    k.grid = (int)(tree_leaves(n) * (K / 2) / VB);      // a thread's rows do not depend on K (multi_loop.hpp: TREE)
    const long work = (long)n * K;
    c.hstat->it = 0; c.hstat->done = 0; c.hstat->status = 0; c.hstat->t = 0; c.hstat->residual = 0.0;
    hipLaunchKernelGGL(k_binit, dim3(1), dim3(64), 0, c.stream, k.cur, p.epsilon, (double)n, p.abs_diff, work >= (1 << 20) ? 0 : 3, c.hstat_dev);
    HIPCHK(hipGetLastError());

    // setup (lcg.cpp:650-689): A.m for the guess, r0 = p = r, the verdict "already optimised"
    c.cnt_ax++;
    TRY(spmm_launch(P, K, M, t, c.stream, nullptr));
    TRY((k.template pass<1, MFinNone, BOpInit<JAC>, true>(MFinNone{}, BOpInit<JAC>{t, B, M, A->invdiag, r, r0, pk, ph}, nullptr, 0)));
    TRY((k.template pass<2, BFinInit<K>, MOpNone, true>(BFinInit<K>{}, MOpNone{}, k.tab_sum, k.grid, 1)));

    const int m_launches = F ? tri_apply_launches(F, 2) : 0;       // counted as vector passes (lcg_hip_last_launches)
    int g_dot = 0, g_dot2 = 0;
    auto body = [&]() -> int {
        if (F) { c.cnt_vec += m_launches; TRY(tri_apply_multi(F, K, 2, pk, ph, c.stream, &k.cur->all_done)); }
        c.cnt_ax++;
        TRY(spmm_launch(P, K, ph, v, c.stream, &k.cur->all_done, r0, big, k.tab_dot, &g_dot));                      // :718-724
        TRY(k.template pass<0>(BFinAlpha<K>{}, BOpS<JAC>{r, v, A->invdiag, s, sh, m2d()}, k.tab_dot, g_dot));                     // :725-731
        if (F) { c.cnt_vec += m_launches; TRY(tri_apply_multi(F, K, 2, s, sh, c.stream, &k.cur->all_done)); }
        c.cnt_ax++;
        TRY(spmm_launch(P, K, sh, t, c.stream, &k.cur->all_done, s, big, k.tab_dot, &g_dot2, true));                // :733-740
        TRY(k.template pass<1>(BFinOmega<K>{}, BOpUpdate{M, r, ph, sh, s, t, r0, m2d(), m2d()}, k.tab_dot, g_dot2));              // :741-772
        TRY(k.template pass<2>(BFinClose<K>{}, BOpDir<JAC>{pk, ph, r, v, A->invdiag, m2d(), m2d()}, k.tab_sum, k.grid));          // :773-780
        return 0;
    };

    BState h;
    auto read_state = [&]() -> int {
        HIPCHK(hipMemcpyAsync(&h, k.cur, sizeof h, hipMemcpyDeviceToHost, c.stream));
        HIPCHK(hipStreamSynchronize(c.stream));
        return 0;
    };
    const int rc = enqueue_ahead(c, p.max_iterations, work >= (1 << 20) ? 6 : 24, body, read_state, h);
    if (!rc) {
        int longest = 0;
        for (int j = 0; j < K; j++) {
            if (ret) ret[j] = lcg_code(h.stop[j]);
            if (iterations) iterations[j] = h.t[j];
            if (residual) residual[j] = h.residual[j];
            if (h.t[j] > h.t[longest]) longest = j;
        }
        c.last_iters = h.t[longest];
        c.last_residual = h.residual[longest];
        c.last_ax_calls = 0; c.last_ax_mean_us = 0.0; c.prof_pending = 0;
    } else {
        (void)hipStreamSynchronize(c.stream);       // nothing of this solve may still run on vectors that go back to the pool
        (void)hipGetLastError();
    }
    const int rc2 = hb.close(c.stream);
    return rc ? rc : rc2;
}

template <int K>
static int run_bicg_k(lcg_hip_csr *A, bool jac, const TriFactor *F, double *M, const double *B, const lcg_para &p, int *ret, int *iterations,
                      double *residual, int mem)
{
    return jac ? run_bicg<K, true>(A, F, M, B, p, ret, iterations, residual, mem) : run_bicg<K, false>(A, F, M, B, p, ret, iterations, residual, mem);
}

} // namespace
} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_lbicgstab_multi(lcg_hip_csr_t A, int k, int precond, double *M, const double *B, const lcg_para *param, int *ret,
                            int *iterations, double *residual, int mem)
{
    static const char *entry = "lcg_hip_lbicgstab_multi";
    NOT_DENSE(A, LCG_HIP_E_ARG);
    TRY(multi_args(entry, k, M, B));
    TRY(multi_handle(entry, A));
    if (A->n_rows != A->n_cols) { ctx().err = std::string(entry) + ": the matrix is not square"; return LCG_HIP_E_ARG; }
    if (mem != LCG_HIP_MEM_HOST && mem != LCG_HIP_MEM_DEVICE) { ctx().err = std::string(entry) + ": mem is neither LCG_HIP_MEM_HOST nor LCG_HIP_MEM_DEVICE"; return LCG_HIP_E_ARG; }
    if (precond != LCG_HIP_M_NONE && precond != LCG_HIP_M_JACOBI && precond != LCG_HIP_M_IC0 && precond != LCG_HIP_M_ILU0) {
        ctx().err = std::string(entry) + ": precond is none of LCG_HIP_M_NONE, LCG_HIP_M_JACOBI, LCG_HIP_M_IC0, LCG_HIP_M_ILU0";
        return LCG_HIP_E_ARG;
    }
    const lcg_para p = param ? *param : lcg_hip_default_parameters();
    if (p.max_iterations < 0) return LCG_INVILAD_MAX_ITERATIONS;            // lcg.cpp:637-638
    if (p.epsilon <= 0.0 || p.epsilon >= 1.0) return LCG_INVILAD_EPSILON;
    TriFactor *F = nullptr;
    const bool jac = precond == LCG_HIP_M_JACOBI;
    if (jac) {
        if (A->invdiag == nullptr) return LCG_NULL_PRECONDITION_MATRIX;     // lcg_hip_csr_build_jacobi has not run
    } else if (precond != LCG_HIP_M_NONE) {
        F = precond == LCG_HIP_M_IC0 ? A->ic0 : A->ilu0;
        if (!F || !F->ok) return LCG_NULL_PRECONDITION_MATRIX;              // lcg_hip_csr_build_ic0 / _ilu0 has not run (or its pivot failed)
    }
    TRY(ensure_init());
    if (F) TRY(tri_multi_reserve(F, k, 2));
    if (k == 2) return run_bicg_k<2>(A, jac, F, M, B, p, ret, iterations, residual, mem);
    if (k == 4) return run_bicg_k<4>(A, jac, F, M, B, p, ret, iterations, residual, mem);
    return run_bicg_k<8>(A, jac, F, M, B, p, ret, iterations, residual, mem);
}

} // extern "C"
