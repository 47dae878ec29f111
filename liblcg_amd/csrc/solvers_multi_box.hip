// solvers_multi_box.hip -- batched box-constrained solvers over k = 2, 4, 8 right-hand sides: lcg_hip_solver_constrained_multi (a CSR
// handle), lcg_hip_dense_solver_constrained_multi (a dense handle's K^T.K or K) and lcg_hip_csr_normal_solver_constrained_multi (a
// rectangular CSR handle's K^T.K: csr_normal.hip).  DESIGN.md sections 24, 26.
//
// Each column runs the reference's lpg (lcg.cpp:1054-1204) or lspg (lcg.cpp:1224-1446) as if it were alone: the guess projected
// into the box, g = A.m - b, both "already optimised" criteria in the reference's order, the stop rule and the cap at the loop
// head, Barzilai-Borwein steps s.s / s.y from param->step, and for SPG the non-monotone line search over its own ring of the last
// maxi_m accepted q = sum(0.5 m_i (A.m)_i - b_i m_i).  What the columns share is the matrix (one k-wide product per body, through
// multi_ops.hpp's operator argument) and the bounds (one low / hig per row).
//
// The line search is device resident.  Every running column has exactly ONE trial point pending in `mn`; a body is
//     Ad = A.mn  |  [head] sums over the trial point: q, s.s, s.y, m.m, g.g  |  [decide] commit / next direction / shrink
// and the decision is taken per column in the prologue of the last pass (k_mvecf's scalar step):
//     accepted  (PG: always; SPG: not q > max(ring) + sigma a g.d): t++, ring[(t + 1) mod maxi_m] = q, lambda = s.s / s.y, the
//               residual, then convergence, the cap, the breakdown test; the pass commits m = mn, g = Ad - b and, if the column
//               goes on, writes d = P(m - lambda g) - m, the trial point m + d and the sums of g.d (PG: the trial point
//               P(m - lambda g));
//     rejected  a *= beta and the pass rewrites the trial point m + a d.
// So columns drift apart in trial count and none is ever idle; a body is one iteration for PG and one trial for SPG.  The cap is
// the column's own and is enforced here: the host's enqueue-ahead loop only paces.
//
// State: XState in MultiFrame's pair.  The q rings do not fit its slot: they live in a pair of their own under the same
// discipline -- the decide step of every workgroup reads one copy, workgroup 0 writes the other in full, the host swaps them.
// The decide pass reads the head pass's table and leaves its own sums (g.d) in a second table, which the next head step adds up: no
// pass reads a table that the same launch writes.  Both tables are this loop's own (five sums per column at k = 8 are 40 rows).
//
// Sums: every pass is a TREE pass (multi_loop.hpp) for CSR and dense alike, so column j's iterate, count, products, residual and
// code are the same bits whatever k is, wherever the column stands, whatever the other columns hold.
//
// Frozen columns: the decide pass runs for ALL columns under its own per-column action word, because the launch in which a column
// stops is also the one that commits its last iterate.  A column without an action is not stored to: m, g, d, mn of a stopped
// column are final (st2's select), a stopped NaN column leaks into nothing.
//
// Deviations from the reference (the header states them): a column whose next step s.s / s.y is not finite ends with
// LCG_NAN_VALUE at that iteration, its last accepted iterate kept; a column whose |m|^2 or |g|^2 is NaN after an accepted step
// ends with LCG_NAN_VALUE; there is no callback.
#include <cmath>

#include "multi_ops.hpp"
#include "lcg_hip_staging_box_multi.h"

namespace lcgh {
namespace {

constexpr int XB_MAXIM = 64;            // the largest maxi_m (documented in the header)
constexpr int ST_XCAP = 16;             // a stop word of this loop: the column's own cap (lcg_code's default: LCG_REACHED_MAX_ITERATIONS)
enum { XA_COMMIT = 1, XA_DIR = 2, XA_SHRINK = 4 };

struct XState : MultiHead {
    double lam[MM_MAXK], a[MM_MAXK], gd[MM_MAXK], qmax[MM_MAXK], m2[MM_MAXK], g2[MM_MAXK], residual[MM_MAXK];
    int act[MM_MAXK];       // what the decide pass does to the column: XA_* bits
    int prod[MM_MAXK];      // A.x calls of the reference on this column: 1 + its trial points
};

struct XPara { double step, sigma, beta; int maxi_m, max_iterations; };

__device__ __forceinline__ double xbox(double lo, double hi, double a) { return a >= hi ? hi : (a <= lo ? lo : a); }   // algebra.cpp:50-58

// ---- scalar steps ---------------------------------------------------------------------------------------------------------------------
// setup: |m|^2 (clamped), |g|^2, both "already optimised" criteria (lcg.cpp:1100-1125, 1277-1302); the first step length; q of the
// projected guess in slot 0 of the ring, the other slots -1e30 (:1304-1314).  Sums m.m, g.g, q
template <int K, bool SPG> struct XFinInit {
    static constexpr int NS = 3;
    XPara p; double *ring;
    __device__ void operator()(XState *st, const double *sum) const
    {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double m2 = clamp1(sum[j]), g2 = sum[K + j], q = sum[2 * K + j];
            st->m2[j] = m2; st->g2[j] = g2; st->lam[j] = p.step; st->a[j] = 1.0; st->qmax[j] = q; st->gd[j] = 0.0; st->prod[j] = 1;
            m_already(st, j, g2, m2);
            st->act[j] = st->stop[j] == ST_RUNNING ? XA_DIR : 0;
            if (SPG && blockIdx.x == 0)
                for (int i = 0; i < p.maxi_m; i++) ring[j * p.maxi_m + i] = i == 0 ? q : -1e+30;
        }
        all_stopped<K>(st);
        mpublish(st);
    }
};
// first step of a body: counts it; SPG: g.d of the columns whose direction the last decide pass wrote (lcg.cpp:1365-1369)
template <int K, bool SPG> struct XFinHead {
    static constexpr int NS = SPG ? 1 : 0;
    __device__ void operator()(XState *st, const double *sum) const
    {
        st->it++;
        if (!SPG || st->all_done) return;
#pragma unroll
        for (int j = 0; j < K; j++) if (st->stop[j] == ST_RUNNING && (st->act[j] & XA_DIR)) st->gd[j] = sum[j];
    }
};
// the decision on every running column's trial point.  Sums SPG: q, s.s, s.y, m.m, g.g; PG: s.s, s.y, m.m, g.g
template <int K, bool SPG> struct XFinDecide {
    static constexpr int NS = SPG ? 5 : 4;
    XPara p; const double *rcur; double *rnext;
    __device__ void operator()(XState *st, const double *sum) const
    {
#pragma unroll
        for (int j = 0; j < K; j++) st->act[j] = 0;
        if (!st->all_done) {
            constexpr int O = SPG ? 1 : 0;
#pragma unroll
            for (int j = 0; j < K; j++) {
                if (st->stop[j] != ST_RUNNING) continue;
                st->prod[j]++;
                const double q = sum[j], ss = sum[O * K + j], sy = sum[(O + 1) * K + j], mm = sum[(O + 2) * K + j], gg = sum[(O + 3) * K + j];
                if (SPG) {
                    const double *rc = rcur + j * p.maxi_m;
                    double *rn = rnext + j * p.maxi_m;
                    if (q > st->qmax[j] + p.sigma * st->a[j] * st->gd[j]) {         // lcg.cpp:1377-1399
                        st->a[j] *= p.beta;
                        st->act[j] = XA_SHRINK;
                        if (blockIdx.x == 0) for (int i = 0; i < p.maxi_m; i++) rn[i] = rc[i];
                        continue;
                    }
                    const int w = (st->t[j] + 2) % p.maxi_m;                        // (t + 1) mod maxi_m after t++ (:1402)
                    double mx = 0.0;
                    for (int i = 0; i < p.maxi_m; i++) {                            // the next iteration's maxi_qk (:1371-1375)
                        const double v = i == w ? q : rc[i];
                        mx = i == 0 ? v : (mx >= v ? mx : v);
                        if (blockIdx.x == 0) rn[i] = v;
                    }
                    st->qmax[j] = mx;
                    st->a[j] = 1.0;
                }
                st->t[j]++;
                st->act[j] = XA_COMMIT;
                const double lam = ss / sy;                                         // :1178, :1419
                st->lam[j] = lam;
                st->m2[j] = clamp1(mm);
                st->g2[j] = gg;
                if (mm != mm || gg != gg) { st->stop[j] = ST_NAN; continue; }
                const double r = m_residual(st, gg, st->m2[j]);                     // the next loop head (:1130-1150, :1320-1340)
                st->residual[j] = r;
                if (r <= st->eps) st->stop[j] = ST_CONVERGED;
                else if (p.max_iterations > 0 && st->t[j] + 1 > p.max_iterations) st->stop[j] = ST_XCAP;
                else if (!isfinite(lam)) st->stop[j] = ST_NAN;                      // the reference would fill m with NaN from here
                else st->act[j] |= XA_DIR;
            }
            all_stopped<K>(st);
        }
        mpublish(st);
    }
};

// ---- vector passes --------------------------------------------------------------------------------------------------------------------
struct XOpProject {     // m = P(m)                                           lcg.cpp:1086-1090, 1263-1267
    static constexpr int NS = 0;
    double *m; const double *low, *hig;
    __device__ void prep(const XState &, int) {}
    __device__ void apply(long e, long row, bool r0, bool r1, m2d *)
    {
        const double lo = low[row], hi = hig[row];
        m2d v = ld2(m, e);
        v.x = xbox(lo, hi, v.x); v.y = xbox(lo, hi, v.y);
        st2(m, e, v, r0, r1);
    }
};
struct XOpInit {        // g = Ad - B; m.m, g.g, q                            lcg.cpp:1092-1105, 1269-1282, 1305-1308
    static constexpr int NS = 3;
    const double *Ad, *B, *m; double *g;
    __device__ void prep(const XState &, int) {}
    __device__ void apply(long e, long, bool r0, bool r1, m2d *acc)
    {
        const m2d av = ld2(Ad, e), bv = ld2(B, e), mv = ld2(m, e), gv = av - bv;
        st2(g, e, gv, r0, r1);
        acc[0] += mv * mv; acc[1] += gv * gv; acc[2] += (0.5 * mv) * av - bv * mv;
    }
};
template <bool SPG> struct XOpSums {    // over the trial point: [q,] s.s, s.y, m.m, g.g   lcg.cpp:1159-1190, 1359-1363, 1404-1431
    static constexpr int NS = SPG ? 5 : 4;
    const double *mn, *Ad, *B, *m, *g;
    __device__ void prep(const XState &, int) {}
    __device__ void apply(long e, long, bool, bool, m2d *acc)
    {
        constexpr int O = SPG ? 1 : 0;
        const m2d tv = ld2(mn, e), av = ld2(Ad, e), bv = ld2(B, e), gn = av - bv;
        const m2d s = tv - ld2(m, e), y = gn - ld2(g, e);
        if (SPG) acc[0] += (0.5 * tv) * av - bv * tv;
        acc[O] += s * s; acc[O + 1] += s * y; acc[O + 2] += tv * tv; acc[O + 3] += gn * gn;
    }
};
// what the decision asks for, per column of the piece: commit m = mn, g = Ad - B (:1180-1185, :1421-1426); the next direction and
// trial point (:1154-1159; :1344-1355 with g.d); a shorter trial (:1379-1384)
template <bool SPG> struct XOpStep {
    static constexpr int NS = SPG ? 1 : 0;
    double *m, *g, *d, *mn; const double *Ad, *B, *low, *hig;
    int a0, a1; m2d lam, ak;
    __device__ void prep(const XState &L, int c0)
    {
        a0 = L.act[c0]; a1 = L.act[c0 + 1];
        lam.x = L.lam[c0]; lam.y = L.lam[c0 + 1]; ak.x = L.a[c0]; ak.y = L.a[c0 + 1];
    }
    __device__ __forceinline__ void half(int act, double lo, double hi, double lm, double a, double &mv, double &gv, double tn, double av,
                                         double bv, double &dv, double &out, double &gd) const
    {
        if (act & XA_COMMIT) { mv = tn; gv = av - bv; }
        if (act & XA_DIR) {
            if (SPG) { dv = xbox(lo, hi, mv - lm * gv) - mv; out = mv + dv; gd += gv * dv; }
            else out = xbox(lo, hi, mv - lm * gv);
        } else if (act & XA_SHRINK) out = mv + a * dv;
    }
    __device__ void apply(long e, long row, bool, bool, m2d *acc)
    {
        const int any = a0 | a1;
        if (!any) return;
        const double lo = low[row], hi = hig[row];
        m2d mv = ld2(m, e), gv = ld2(g, e), tn = (m2d)(0.0), av = (m2d)(0.0), bv = (m2d)(0.0), dv = (m2d)(0.0), out = (m2d)(0.0), gd = (m2d)(0.0);
        if (any & XA_COMMIT) { tn = ld2(mn, e); av = ld2(Ad, e); bv = ld2(B, e); }
        if (SPG && (any & XA_SHRINK)) dv = ld2(d, e);
        double mx = mv.x, my = mv.y, gx = gv.x, gy = gv.y, dx = dv.x, dy = dv.y, ox = 0.0, oy = 0.0, sx = 0.0, sy = 0.0;
        half(a0, lo, hi, lam.x, ak.x, mx, gx, tn.x, av.x, bv.x, dx, ox, sx);
        half(a1, lo, hi, lam.y, ak.y, my, gy, tn.y, av.y, bv.y, dy, oy, sy);
        mv.x = mx; mv.y = my; gv.x = gx; gv.y = gy; dv.x = dx; dv.y = dy; out.x = ox; out.y = oy; gd.x = sx; gd.y = sy;
        st2(m, e, mv, a0 & XA_COMMIT, a1 & XA_COMMIT);
        st2(g, e, gv, a0 & XA_COMMIT, a1 & XA_COMMIT);
        if (SPG) { st2(d, e, dv, a0 & XA_DIR, a1 & XA_DIR); acc[0] += gd; }
        st2(mn, e, out, a0 & (XA_DIR | XA_SHRINK), a1 & (XA_DIR | XA_SHRINK));
    }
};

// ---- host side ------------------------------------------------------------------------------------------------------------------------
template <int K, bool SPG, class OpA>
static int run_box(const OpA &A, double *M, const double *B, const double *low, const double *hig, const XPara &xp, const lcg_para &p,
                   int *ret, int *iterations, int *products, double *residual, int mem)
{
    using F = MultiFrame<XState, K, K / 2>;
    F f(A.rows());
    Ctx &c = f.c;
    const size_t nb = sizeof(double) * (size_t)A.rows();
    TRY(f.open(mem, M, B));
    double *g = nullptr, *d = nullptr, *mn = nullptr, *Ad = nullptr, *big = nullptr, *ring = nullptr;
    TRY(f.vec(g));
    if (SPG) TRY(f.vec(d));
    TRY(f.vec(mn));
    TRY(f.vec(Ad));
    const size_t nbig = A.big_doubles(K);
    if (nbig) TRY(f.ws.get(big, nullptr, sizeof(double) * nbig));
    if (mem == LCG_HIP_MEM_HOST) {      // the bounds onto the device, like M and B
        double *dl = nullptr, *dh = nullptr;
        TRY(f.ws.get(dl, nullptr, nb)); TRY(f.ws.get(dh, nullptr, nb));
        HIPCHK(hipMemcpyAsync(dl, low, nb, hipMemcpyHostToDevice, c.stream));
        HIPCHK(hipMemcpyAsync(dh, hig, nb, hipMemcpyHostToDevice, c.stream));
        low = dl; hig = dh;
    }
    const size_t ring_doubles = (size_t)K * xp.maxi_m;
    if (SPG) TRY(f.ws.get(ring, nullptr, 2 * sizeof(double) * ring_doubles));
    double *rcur = ring, *rnext = SPG ? ring + ring_doubles : nullptr;
    // the passes' tables: five sums per column at K = 8 are more rows than the context's tables hold (MAXR * MAXG doubles), so this
    // loop brings its own -- tab_head for the head pass's (and the setup's) sums, tab_gd for the decide pass's
    constexpr int HEAD_ROWS = (SPG ? 5 : 4) * K;
    double *tab_head = nullptr;
    TRY(f.ws.get(tab_head, nullptr, sizeof(double) * (size_t)(HEAD_ROWS + K) * MM_MG));
    double *tab_gd = tab_head + (size_t)HEAD_ROWS * MM_MG;
    TRY(f.start(f.tree_grid(), p.epsilon, p.abs_diff));

    // MultiFrame::pass with the table the pass writes named: TREE as there, `pout` is never the table `pin`
    auto pass = [&](auto tree, auto all, auto fin, auto op, const double *pin, double *pout) -> int {
        using Fin = decltype(fin); using Op = decltype(op);
        c.cnt_vec++;
        hipLaunchKernelGGL((k_mvecf<XState, K, K / 2, Fin, Op, decltype(all)::value, decltype(tree)::value>), dim3(f.grid), dim3(VB), 0, c.stream,
                           fin, op, f.n2, pin, f.grid, pout, f.cur, f.next);
        HIPCHK(hipGetLastError());
        std::swap(f.cur, f.next);
        return 0;
    };
    using T0 = std::integral_constant<int, 0>; using T1 = std::integral_constant<int, 1>;
    using TD = std::integral_constant<int, SPG ? 3 : 2>; using TH = std::integral_constant<int, SPG ? 3 : 1>;
    const XOpStep<SPG> step{M, g, d, mn, Ad, B, low, hig, 0, 0, m2d(), m2d()};

    // setup: the guess into the box, A.m, g, the verdict "already optimised", the first trial point
    TRY(pass(T0{}, std::true_type{}, MFinNone{}, XOpProject{M, low, hig}, nullptr, tab_head));
    TRY(A.apply(c, K, M, Ad, nullptr));
    TRY(pass(T1{}, std::true_type{}, MFinNone{}, XOpInit{Ad, B, M, g}, nullptr, tab_head));
    TRY(pass(TD{}, std::true_type{}, XFinInit<K, SPG>{xp, rcur}, step, tab_head, tab_gd));

    // the cap is the columns' own, on the device (XFinDecide): the host only paces.  PG: a body is an iteration of every running
    // column, so no column needs more bodies than the cap
    f.run(SPG ? 0 : p.max_iterations, [&]() -> int {
        TRY(A.apply(c, K, mn, Ad, &f.cur->all_done));
        TRY(pass(TH{}, std::false_type{}, XFinHead<K, SPG>{}, XOpSums<SPG>{mn, Ad, B, M, g}, tab_gd, tab_head));
        TRY(pass(TD{}, std::true_type{}, XFinDecide<K, SPG>{xp, rcur, rnext}, step, tab_head, tab_gd));
        std::swap(rcur, rnext);
        return 0;
    });
    if (!f.rc && products) for (int j = 0; j < K; j++) products[j] = f.h.prod[j];
    return f.finish(lcg_code, ret, iterations, residual);
}

// the reference's parameter codes in its order, per solver (lcg.cpp:1062-1065, 1232-1238); then this loop's own bound on maxi_m
static int box_para(const char *entry, bool spg, const lcg_para *param, lcg_para &p, XPara &xp)
{
    p = param ? *param : lcg_hip_default_parameters();
    if (p.max_iterations < 0) return LCG_INVILAD_MAX_ITERATIONS;
    if (spg) {
        if (p.epsilon <= 0.0 || p.epsilon >= 1.0) return LCG_INVILAD_EPSILON;
        if (p.step <= 0.0) return LCG_INVALID_LAMBDA;
        if (p.sigma <= 0.0 || p.sigma >= 1.0) return LCG_INVALID_SIGMA;
        if (p.beta <= 0.0 || p.beta >= 1.0) return LCG_INVALID_BETA;
        if (p.maxi_m <= 0) return LCG_INVALID_MAXIM;
        if (p.maxi_m > XB_MAXIM) { ctx().err = std::string(entry) + ": maxi_m is larger than 64"; return LCG_HIP_E_ARG; }
    } else {
        if (p.epsilon <= 0.0) return LCG_INVILAD_EPSILON;
        if (p.step <= 0.0 || p.epsilon >= 1.0) return LCG_INVALID_LAMBDA;
    }
    xp = XPara{p.step, p.sigma, p.beta, spg ? p.maxi_m : 1, p.max_iterations};
    return 0;
}

static int box_bounds(const char *entry, const double *low, const double *hig)
{
    if (!low || !hig) { ctx().err = std::string(entry) + ": low or hig is null"; return LCG_HIP_E_ARG; }
    return 0;
}

template <class OpA>
static int box_dispatch(const OpA &op, int k, bool spg, double *M, const double *B, const double *low, const double *hig, const XPara &xp,
                        const lcg_para &p, int *ret, int *iterations, int *products, double *residual, int mem)
{
    return multi_k(k, [&](auto K) {
        return spg ? run_box<decltype(K)::value, true>(op, M, B, low, hig, xp, p, ret, iterations, products, residual, mem)
                   : run_box<decltype(K)::value, false>(op, M, B, low, hig, xp, p, ret, iterations, products, residual, mem);
    });
}

} // namespace
} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_solver_constrained_multi(lcg_hip_csr_t A, int k, int solver_id, double *M, const double *B, const double *low,
                                     const double *hig, const lcg_para *param, int *ret, int *iterations, int *products,
                                     double *residual, int mem)
{
    static const char *entry = "lcg_hip_solver_constrained_multi";
    const bool spg = solver_id == LCG_SPG;
    lcg_para p;
    XPara xp;
    TRY(multi_args(entry, k, M, B));
    TRY(box_bounds(entry, low, hig));
    NOT_DENSE(A, LCG_HIP_E_ARG);
    TRY(multi_handle(entry, A));
    TRY(multi_shape(entry, A->n_rows == A->n_cols, mem));
    TRY(box_para(entry, spg, param, p, xp));
    TRY(ensure_init());
    return box_dispatch(CsrOp{A, nullptr}, k, spg, M, B, low, hig, xp, p, ret, iterations, products, residual, mem);
}

int lcg_hip_dense_solver_constrained_multi(lcg_hip_dense_t K, int k, int normal, int solver_id, double *M, const double *B,
                                           const double *low, const double *hig, const lcg_para *param, int *ret, int *iterations,
                                           int *products, double *residual, int mem)
{
    static const char *entry = "lcg_hip_dense_solver_constrained_multi";
    const bool spg = solver_id == LCG_SPG;
    lcg_para p;
    XPara xp;
    TRY(multi_args(entry, k, M, B));
    TRY(box_bounds(entry, low, hig));
    lcg_hip_dense *D = dnm_handle(entry, K);
    if (!D) return LCG_HIP_E_ARG;
    TRY(multi_shape(entry, normal != 0 || D->M == D->N, mem, ": normal = 0 needs a square one"));
    if (normal != 0 && normal != 1) { ctx().err = std::string(entry) + ": normal is neither 1 (K^T.K) nor 0 (K)"; return LCG_HIP_E_ARG; }
    TRY(box_para(entry, spg, param, p, xp));
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    return box_dispatch(DenseOp{D, normal}, k, spg, M, B, low, hig, xp, p, ret, iterations, products, residual, mem);
}

int lcg_hip_csr_normal_solver_constrained_multi(lcg_hip_csr_t K, int k, int solver_id, double *M, const double *B, const double *low,
                                                const double *hig, const lcg_para *param, int *ret, int *iterations, int *products,
                                                double *residual, int mem)
{
    static const char *entry = "lcg_hip_csr_normal_solver_constrained_multi";
    const bool spg = solver_id == LCG_SPG;
    lcg_para p;
    XPara xp;
    TRY(normal_kind(entry, K));
    TRY(multi_args(entry, k, M, B));
    TRY(box_bounds(entry, low, hig));
    TRY(multi_shape(entry, true, mem));
    TRY(normal_ready(entry, K));
    TRY(box_para(entry, spg, param, p, xp));
    TRY(normal_reserve(K, k));
    return box_dispatch(CsrNormalOp{K}, k, spg, M, B, low, hig, xp, p, ret, iterations, products, residual, mem);
}

} // extern "C"
