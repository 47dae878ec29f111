// solvers_multi.hip -- batched CG and PCG over k = 2, 4, 8 right-hand sides: lcg_hip_lcg_multi, lcg_hip_lpcg_multi (the built-in
// Jacobi), lcg_hip_lpcg_multi_m (Jacobi, or the handle's IC(0) / ILU(0) factor applied k wide: csr_tri_multi.hip), and the same loop
// on a dense handle's K^T.K or K: lcg_hip_dense_lcg_multi, lcg_hip_dense_lpcg_multi (dense_multi.hip), and on a rectangular CSR
// handle's K^T.K: lcg_hip_csr_normal_lcg_multi, lcg_hip_csr_normal_lpcg_multi (csr_normal.hip).  The loop reaches the matrix
// through a small operator argument (CsrOp, CsrNormalOp, DenseOp: multi_ops.hpp).
//
// Each column runs the reference's own recurrence as if it were alone (lcg.cpp:143-274, 293-434): its own alpha, beta, rho, its own
// residual under the same stop rule, its own "already optimised" test, NaN scan, count and return code.  What the columns share is
// the matrix: one multi-vector product (csr_multi.hip) per iteration reads col / val once for all of them.
//
// The classic three-pass schedule of solvers_real.hip, k wide (vectors: multi.hpp's row-major blocks):
//     A.d carrying d.Ad  |  [alpha] m += a d, g += a Ad (PCG: r -= a Ad, z = r / diag) + m.m, g.g (r.r, z.r), NaN  |  [close] d = b d - g (z + b d)
// All scalars live on the device in MState, k wide.  A scalar step rides in the prologue of the pass that consumes it (k_mvecf,
// multi_loop.hpp: shared with the batched BiCGStab of solvers_multi_bicg.hip), as in k_vecf (devcommon.hpp): every block adds the
// previous pass's partial sums in msum's fixed order, runs the step for all columns on
// a copy of MState in LDS, and block 0 commits the copy to the other buffer of a pair.
//
// With a factor as M the multiply leaves the update pass:
//     A.d carrying d.Ad  |  [alpha] m += a d, r -= a Ad  |  z = M^-1 r (the apply's launches)  |  m.m, r.r, z.r, NaN  |  [close] d = z + b d
// The apply forms z for every column, stopped ones too (nothing reads theirs); every one of its launches honours all_done.
//
// Frozen columns: once a column has stopped (converged, NaN, already optimised) its column of the iterate and of g / r, z, d is never
// written again -- a SELECT on the column's stop word, not a multiplication by zero, so a stopped NaN column leaks into nothing
// (its sums are computed apart and never read).  The product still forms such a column's A.d, which nothing reads.  When every column
// has stopped, MState::all_done makes every later kernel fall through, like DevState::done, so the host enqueues ahead.
//
// A thread of a vector pass handles 16-byte pieces e, e + stride, ...; the stride is a multiple of k / 2, so its two columns never
// change: their coefficients and stop words sit in registers, their sums are two accumulators per running sum.  A column's partial
// sums are added in a fixed order (lane's own in index order, lanes of a wavefront by xor-butterfly, wavefronts in order, blocks in
// order): the same bits whatever the other columns hold, from call to call.
#include "multi_ops.hpp"

namespace lcgh {
namespace {

struct MState : MultiHead {
    double ak[MM_MAXK], bk[MM_MAXK], rho[MM_MAXK], m2[MM_MAXK], g2[MM_MAXK], residual[MM_MAXK];
};

// ---- scalar steps: sums[s * K + j] = running sum s of column j ------------------------------------------------------------------
// setup: |m|^2 (clamped), the residual's numerator, rho; "already optimised" per column (lcg.cpp:178-203, 341-359: in abs_diff mode
// BOTH criteria are tried, in this order).  PCG: sums m.m, r.r, z.r; CG: m.m, g.g (rho = g.g)
template <int K, bool PCG> struct MFinInit {
    static constexpr int NS = PCG ? 3 : 2;
    __device__ void operator()(MState *st, const double *sum) const
    {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double m2 = clamp1(sum[j]), g2 = sum[K + j];
            st->m2[j] = m2; st->g2[j] = g2; st->rho[j] = PCG ? sum[2 * K + j] : g2;
            m_already(st, j, g2, m2);
        }
        all_stopped<K>(st);
        mpublish(st);
    }
};
// first step of a body: counts it; alpha = rho / d.Ad per running column (lcg.cpp:235, 390)
template <int K> struct MFinAlpha {
    static constexpr int NS = 1;
    __device__ void operator()(MState *st, const double *sum) const
    {
        st->it++;
        if (st->all_done) return;
#pragma unroll
        for (int j = 0; j < K; j++) if (st->stop[j] == ST_RUNNING) st->ak[j] = st->rho[j] / sum[j];
    }
};
// closing step of a body, per running column (lcg.cpp:244-257, 401-416).  CG sums: m.m, g.g, NaN count; PCG: m.m, r.r, z.r, NaN count
template <int K, bool PCG> struct MFinClose {
    static constexpr int NS = PCG ? 4 : 3;
    __device__ void operator()(MState *st, const double *sum) const
    {
        if (!st->all_done) {
#pragma unroll
            for (int j = 0; j < K; j++) {
                if (st->stop[j] != ST_RUNNING) continue;
                const double mm = sum[j], g2 = sum[K + j], nan = sum[(NS - 1) * K + j];
                const double rho_new = PCG ? sum[2 * K + j] : g2;
                st->m2[j] = clamp1(mm);
                st->t[j]++;
                if (nan > 0.0 || mm != mm) { st->stop[j] = ST_NAN; continue; }
                st->bk[j] = rho_new / st->rho[j];
                st->rho[j] = rho_new;
                st->g2[j] = g2;
                const double r = m_residual(st, g2, st->m2[j]);      // the next loop head's test (lcg.cpp:208-222)
                st->residual[j] = r;
                if (r <= st->eps) st->stop[j] = ST_CONVERGED;
            }
            all_stopped<K>(st);
        }
        mpublish(st);
    }
};

// ---- vector passes ----------------------------------------------------------------------------------------------------------------
struct MOpCgInit {      // g = Ad - B; d = -g; m.m, g.g                   lcg.cpp:171-183
    static constexpr int NS = 2;
    const double *Ad, *B, *m; double *g, *d;
    __device__ void prep(const MState &, int) {}
    __device__ void apply(long e, long, bool r0, bool r1, m2d *acc)
    {
        const m2d gv = ld2(Ad, e) - ld2(B, e), mv = ld2(m, e);
        st2(g, e, gv, r0, r1); st2(d, e, -gv, r0, r1);
        acc[0] += mv * mv; acc[1] += gv * gv;
    }
};
struct MOpPcgInit {     // r = B - Ad; z = r / diag; d = z; m.m, r.r, z.r  lcg.cpp:317-339
    static constexpr int NS = 3;
    const double *Ad, *B, *m, *invdiag; double *r, *z, *d;
    __device__ void prep(const MState &, int) {}
    __device__ void apply(long e, long row, bool r0, bool r1, m2d *acc)
    {
        const m2d rv = ld2(B, e) - ld2(Ad, e), mv = ld2(m, e);
        const m2d zv = invdiag[row] * rv;
        st2(r, e, rv, r0, r1); st2(z, e, zv, r0, r1); st2(d, e, zv, r0, r1);
        acc[0] += mv * mv; acc[1] += rv * rv; acc[2] += zv * rv;
    }
};
struct MOpCgUpdate {    // m += a d; g += a Ad; m.m, g.g, NaN              lcg.cpp:237-255
    static constexpr int NS = 3;
    double *m, *g; const double *d, *Ad; m2d ak;
    __device__ void prep(const MState &L, int c0) { ak.x = L.ak[c0]; ak.y = L.ak[c0 + 1]; }
    __device__ void apply(long e, long, bool r0, bool r1, m2d *acc)
    {
        const m2d mv = ld2(m, e) + ak * ld2(d, e);
        const m2d gv = ld2(g, e) + ak * ld2(Ad, e);
        st2(m, e, mv, r0, r1); st2(g, e, gv, r0, r1);
        acc[0] += mv * mv; acc[1] += gv * gv; acc[2] += nan2(mv);
    }
};
struct MOpPcgUpdate {   // m += a d; r -= a Ad; z = r / diag; m.m, r.r, z.r, NaN   lcg.cpp:392-414
    static constexpr int NS = 4;
    double *m, *r, *z; const double *d, *Ad, *invdiag; m2d ak;
    __device__ void prep(const MState &L, int c0) { ak.x = L.ak[c0]; ak.y = L.ak[c0 + 1]; }
    __device__ void apply(long e, long row, bool r0, bool r1, m2d *acc)
    {
        const m2d mv = ld2(m, e) + ak * ld2(d, e);
        const m2d rv = ld2(r, e) - ak * ld2(Ad, e);
        const m2d zv = invdiag[row] * rv;
        st2(m, e, mv, r0, r1); st2(r, e, rv, r0, r1); st2(z, e, zv, r0, r1);
        acc[0] += mv * mv; acc[1] += rv * rv; acc[2] += zv * rv; acc[3] += nan2(mv);
    }
};
// a factor as M: the update and the sums are two passes with the apply's launches between them
struct MOpFRes {        // r = B - Ad                                      lcg.cpp:317-321
    static constexpr int NS = 0;
    const double *Ad, *B; double *r;
    __device__ void prep(const MState &, int) {}
    __device__ void apply(long e, long, bool r0, bool r1, m2d *) { st2(r, e, ld2(B, e) - ld2(Ad, e), r0, r1); }
};
struct MOpFInit {       // d = z; m.m, r.r, z.r                            lcg.cpp:322-339
    static constexpr int NS = 3;
    const double *m, *r, *z; double *d;
    __device__ void prep(const MState &, int) {}
    __device__ void apply(long e, long, bool r0, bool r1, m2d *acc)
    {
        const m2d mv = ld2(m, e), rv = ld2(r, e), zv = ld2(z, e);
        st2(d, e, zv, r0, r1);
        acc[0] += mv * mv; acc[1] += rv * rv; acc[2] += zv * rv;
    }
};
struct MOpFUpdate {     // m += a d; r -= a Ad                             lcg.cpp:392-399
    static constexpr int NS = 0;
    double *m, *r; const double *d, *Ad; m2d ak;
    __device__ void prep(const MState &L, int c0) { ak.x = L.ak[c0]; ak.y = L.ak[c0 + 1]; }
    __device__ void apply(long e, long, bool r0, bool r1, m2d *)
    {
        st2(m, e, ld2(m, e) + ak * ld2(d, e), r0, r1);
        st2(r, e, ld2(r, e) - ak * ld2(Ad, e), r0, r1);
    }
};
struct MOpFSums {       // m.m, r.r, z.r, NaN                              lcg.cpp:401-414
    static constexpr int NS = 4;
    const double *m, *r, *z;
    __device__ void prep(const MState &, int) {}
    __device__ void apply(long e, long, bool, bool, m2d *acc)
    {
        const m2d mv = ld2(m, e), rv = ld2(r, e), zv = ld2(z, e);
        acc[0] += mv * mv; acc[1] += rv * rv; acc[2] += zv * rv; acc[3] += nan2(mv);
    }
};
struct MOpCgDir {       // d = b d - g                                     lcg.cpp:259-263
    static constexpr int NS = 0;
    double *d; const double *g; m2d bk;
    __device__ void prep(const MState &L, int c0) { bk.x = L.bk[c0]; bk.y = L.bk[c0 + 1]; }
    __device__ void apply(long e, long, bool r0, bool r1, m2d *) { st2(d, e, bk * ld2(d, e) - ld2(g, e), r0, r1); }
};
struct MOpPcgDir {      // d = z + b d                                     lcg.cpp:418-422
    static constexpr int NS = 0;
    double *d; const double *z; m2d bk;
    __device__ void prep(const MState &L, int c0) { bk.x = L.bk[c0]; bk.y = L.bk[c0 + 1]; }
    __device__ void apply(long e, long, bool r0, bool r1, m2d *) { st2(d, e, ld2(z, e) + bk * ld2(d, e), r0, r1); }
};

// ---- the matrix, as the loop sees it: CsrOp, DenseOp (multi_ops.hpp) ------------------------------------------------------------------
template <int K, bool PCG, class OpA>
static int run_multi(const OpA &A, double *M, const double *B, const lcg_para &p, int *ret, int *iterations, double *residual, int mem)
{   // A.factor(): the factor that is M (PCG only; its k-wide work vectors reserved by the caller), nullptr: the built-in Jacobi
    const TriFactor *F = A.factor();
    constexpr int T1 = OpA::TREE ? 1 : 0, T2 = OpA::TREE ? 2 : 0;      // (a factor comes with a CsrOp only: the plain order of the sums)
    MultiFrame<MState, K, K / 2> f(A.rows());
    Ctx &c = f.c;
    TRY(f.open(mem, M, B));
    double *g = nullptr, *z = nullptr, *d = nullptr, *Ad = nullptr, *big = nullptr;
    TRY(f.vec(g));          // (PCG: r)
    if (PCG) TRY(f.vec(z));
    TRY(f.vec(d));
    TRY(f.vec(Ad));
    const size_t nbig = A.big_doubles(K);
    if (nbig) TRY(f.ws.get(big, nullptr, sizeof(double) * nbig));
    TRY(f.start(OpA::TREE ? f.tree_grid() : grid_for(f.n2), p.epsilon, p.abs_diff));

    // setup (lcg.cpp:168-203, 314-359): A.m for the guess, the first residual and direction, the verdict "already optimised"
    TRY(A.apply(c, K, M, Ad, nullptr));
    const int m_launches = PCG && F ? tri_apply_launches(F, 2) : 0;        // counted as vector passes (lcg_hip_last_launches)
    if (PCG && F) {
        TRY((f.template pass<0, true>(MFinNone{}, MOpFRes{Ad, B, g}, nullptr, 0)));
        c.cnt_vec += m_launches;
        TRY(tri_apply_multi(F, K, 2, g, z, c.stream, nullptr));
        TRY((f.template pass<0, true>(MFinNone{}, MOpFInit{M, g, z, d}, nullptr, 0)));
    } else if (PCG) TRY((f.template pass<T1, true>(MFinNone{}, MOpPcgInit{Ad, B, M, A.invdiag(), g, z, d}, nullptr, 0)));
    else TRY((f.template pass<T1, true>(MFinNone{}, MOpCgInit{Ad, B, M, g, d}, nullptr, 0)));
    TRY((f.template pass<T2, true>(MFinInit<K, PCG>{}, MOpNone{}, f.tab_sum, f.grid, 1)));

    int g_dot = 0;
    f.run(p.max_iterations, [&]() -> int {
        TRY(A.apply(c, K, d, Ad, &f.cur->all_done, d, big, f.tab_dot, &g_dot));                                 // :232-234, :387-389
        if (PCG && F) {
            TRY(f.template pass<0>(MFinAlpha<K>{}, MOpFUpdate{M, g, d, Ad, m2d()}, f.tab_dot, g_dot));          // :390-399
            c.cnt_vec += m_launches;
            TRY(tri_apply_multi(F, K, 2, g, z, c.stream, &f.cur->all_done));                                    // :400
            TRY(f.template pass<0>(MFinNone{}, MOpFSums{M, g, z}, nullptr, 0));                                 // :401-414
            TRY(f.template pass<0>(MFinClose<K, true>{}, MOpPcgDir{d, z, m2d()}, f.tab_sum, f.grid));           // :415-422
        } else if (PCG) {
            TRY(f.template pass<T1>(MFinAlpha<K>{}, MOpPcgUpdate{M, g, z, d, Ad, A.invdiag(), m2d()}, f.tab_dot, g_dot));  // :390-414
            TRY(f.template pass<T2>(MFinClose<K, true>{}, MOpPcgDir{d, z, m2d()}, f.tab_sum, f.grid));          // :415-422
        } else {
            TRY(f.template pass<T1>(MFinAlpha<K>{}, MOpCgUpdate{M, g, d, Ad, m2d()}, f.tab_dot, g_dot));        // :235-255
            TRY(f.template pass<T2>(MFinClose<K, false>{}, MOpCgDir{d, g, m2d()}, f.tab_sum, f.grid));          // :256-263
        }
        return 0;
    });
    return f.finish(lcg_code, ret, iterations, residual);
}

// precond: LCG_HIP_M_JACOBI (CG: not looked at), LCG_HIP_M_IC0, LCG_HIP_M_ILU0
template <bool PCG>
static int solve_multi(const char *entry, lcg_hip_csr *A, int k, int precond, double *M, const double *B, const lcg_para *param, int *ret, int *iterations,
                       double *residual, int mem)
{
    lcg_para p;
    MultiPrecond m;
    TRY(multi_args(entry, k, M, B));
    TRY(multi_handle(entry, A));
    TRY(multi_shape(entry, A->n_rows == A->n_cols, mem));
    TRY(multi_precond(entry, A, precond, false, PCG, m));
    TRY(multi_para<false>(param, p, A->n_rows));
    if (!m.built) return LCG_NULL_PRECONDITION_MATRIX;
    TRY(ensure_init());
    if (m.F) TRY(tri_multi_reserve(m.F, k, 2));
    const CsrOp op{A, m.F};
    return multi_k(k, [&](auto K) { return run_multi<decltype(K)::value, PCG>(op, M, B, p, ret, iterations, residual, mem); });
}

// the dense entries: A = K^T.K (normal = 1) or K (normal = 0, square), PCG with the reciprocals of lcg_hip_dense_build_jacobi
template <bool PCG>
static int solve_dense_multi(const char *entry, const void *Kh, int k, int normal, double *M, const double *B, const lcg_para *param, int *ret,
                             int *iterations, double *residual, int mem)
{
    lcg_para p;
    TRY(multi_args(entry, k, M, B));
    lcg_hip_dense *D = dnm_handle(entry, Kh);
    if (!D) return LCG_HIP_E_ARG;
    if (normal != 0 && normal != 1) { ctx().err = std::string(entry) + ": normal is neither 1 (K^T.K) nor 0 (K)"; return LCG_HIP_E_ARG; }
    TRY(multi_shape(entry, normal || D->M == D->N, mem, ": normal = 0 needs a square one"));
    TRY(multi_para<false>(param, p, D->N));
    // no diagonal, or the other operator's (lcg_hip_dense_build_jacobi records which it built)
    if (PCG && (D->invdiag == nullptr || D->invdiag_normal != normal)) return LCG_NULL_PRECONDITION_MATRIX;
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    const DenseOp op{D, normal};
    return multi_k(k, [&](auto K) { return run_multi<decltype(K)::value, PCG>(op, M, B, p, ret, iterations, residual, mem); });
}

// the normal equations of a rectangular CSR handle: A = K^T.K through the handle's normal state (csr_normal.hip), PCG with the
// reciprocals of lcg_hip_csr_build_jacobi_normal
template <bool PCG>
static int solve_normal_multi(const char *entry, lcg_hip_csr *K, int k, double *M, const double *B, const lcg_para *param, int *ret,
                              int *iterations, double *residual, int mem)
{
    lcg_para p;
    TRY(normal_kind(entry, K));
    TRY(multi_args(entry, k, M, B));
    TRY(multi_shape(entry, true, mem));
    TRY(normal_ready(entry, K));
    TRY(multi_para<false>(param, p, K->n_cols));
    if (PCG && !K->normal->invdiag) return LCG_NULL_PRECONDITION_MATRIX;
    TRY(normal_reserve(K, k));
    const CsrNormalOp op{K};
    return multi_k(k, [&](auto KK) { return run_multi<decltype(KK)::value, PCG>(op, M, B, p, ret, iterations, residual, mem); });
}

} // namespace
} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_lcg_multi(lcg_hip_csr_t A, int k, double *M, const double *B, const lcg_para *param, int *ret, int *iterations,
                      double *residual, int mem)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return solve_multi<false>("lcg_hip_lcg_multi", A, k, LCG_HIP_M_JACOBI, M, B, param, ret, iterations, residual, mem);
}

int lcg_hip_lpcg_multi(lcg_hip_csr_t A, int k, double *M, const double *B, const lcg_para *param, int *ret, int *iterations,
                       double *residual, int mem)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return solve_multi<true>("lcg_hip_lpcg_multi", A, k, LCG_HIP_M_JACOBI, M, B, param, ret, iterations, residual, mem);
}

int lcg_hip_lpcg_multi_m(lcg_hip_csr_t A, int k, int precond, double *M, const double *B, const lcg_para *param, int *ret,
                         int *iterations, double *residual, int mem)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return solve_multi<true>("lcg_hip_lpcg_multi_m", A, k, precond, M, B, param, ret, iterations, residual, mem);
}

int lcg_hip_dense_lcg_multi(lcg_hip_dense_t K, int k, int normal, double *M, const double *B, const lcg_para *param, int *ret,
                            int *iterations, double *residual, int mem)
{
    return solve_dense_multi<false>("lcg_hip_dense_lcg_multi", K, k, normal, M, B, param, ret, iterations, residual, mem);
}

int lcg_hip_dense_lpcg_multi(lcg_hip_dense_t K, int k, int normal, double *M, const double *B, const lcg_para *param, int *ret,
                             int *iterations, double *residual, int mem)
{
    return solve_dense_multi<true>("lcg_hip_dense_lpcg_multi", K, k, normal, M, B, param, ret, iterations, residual, mem);
}

int lcg_hip_csr_normal_lcg_multi(lcg_hip_csr_t K, int k, double *M, const double *B, const lcg_para *param, int *ret, int *iterations,
                                 double *residual, int mem)
{
    return solve_normal_multi<false>("lcg_hip_csr_normal_lcg_multi", K, k, M, B, param, ret, iterations, residual, mem);
}

int lcg_hip_csr_normal_lpcg_multi(lcg_hip_csr_t K, int k, double *M, const double *B, const lcg_para *param, int *ret, int *iterations,
                                  double *residual, int mem)
{
    return solve_normal_multi<true>("lcg_hip_csr_normal_lpcg_multi", K, k, M, B, param, ret, iterations, residual, mem);
}

} // extern "C"

