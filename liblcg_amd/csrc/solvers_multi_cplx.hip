// solvers_multi_cplx.hip -- batched complex loops over k = 2, 4, 8 right-hand sides against one complex-symmetric complex128 matrix:
// clcg_hip_lbicg_sym_multi (clbicg_symmetric, clcg.cpp:228-364) and clcg_hip_lpcg_multi (clpcg with the handle's reciprocal Jacobi
// diagonal, clcg_cuda.cu:403-558).
//
// Each column runs the reference's recurrence as if it were alone: its own ak, bk and rr (PCG: r.s), both inner products
// UNCONJUGATED (clcg_dot, cublasZdotu), its own stop test, "already optimised" test, count and code.  What the columns share is the
// matrix: one multi-vector product per iteration (csr_multi_cplx.hip) reads col / val once for all of them.
//
// Three launches per iteration, every scalar step in the prologue of the pass that consumes it (k_mvecf, multi_loop.hpp):
//     A.d carrying d.Ad  |  [ak = rr / d.Ad] m += ak d; r -= ak Ad (PCG: s = r / diag) + |m|^2, |r|^2, r.r (r.s)  |  [close] d = r + bk d (s + bk d)
// All scalars live on the device in ZMState, k wide, in a pair of buffers; the host only enqueues (multi_loop.hpp: enqueue_ahead).
//
// BiCG-sym's stop rule is the CPU complex loops' 4th-power one, (sum |r|^2)^2 / max((sum |m|^2)^2, 1), or sum |r|^2 / n with
// abs_diff (solvers_cplx.hip: FinZInit, FinZClose<1>), both "already optimised" criteria in the reference's order; the NaN scan of m
// after the update ends that column with CLCG_NAN_VALUE (a NaN element of m makes sum |m|^2 NaN and nothing else does: squares never
// cancel -- the sum IS the scan), the count t after its t++.  PCG's rule is the real loops', sum |r|^2 / max(sum |m|^2, 1), or
// sqrt(sum |r|^2) / n with abs_diff, where |m|^2 takes no part, the "already optimised" test included (FinZPcg).
// One deliberate deviation: the reference's clpcg and this library's single-vector c128 loop have no NaN scan and a broken column
// runs to the cap; here a column whose sum |m|^2, sum |r|^2 or r.s is NaN stops with CLCG_NAN_VALUE at that iteration, as the c64
// loops do -- otherwise one NaN column keeps the whole batch alive for ever at max_iterations = 0.
//
// A 16-byte piece is one complex element of one column, and the stride of a pass is a multiple of k: a thread's column never changes,
// its coefficients and stop word stay in registers.  Frozen columns: a thread whose column has stopped does nothing -- a SELECT on
// the stop word, not a multiplication by zero -- so its elements of m, r, d, s are never stored to again and a NaN column's sums are
// never read by another.  The product still forms such a column's A.d, which nothing reads.
//
// Column j's results are the same bits whatever k is: the product's sums are added in an order the matrix fixes (msum), the passes'
// sums as ONE binary tree over leaves that depend on n alone (multi.hpp: tree_leaves, msum_tree).
//
// The pass is k_mvecf with a lane group of K (multi_loop.hpp): an Op keeps Op::NS 16-byte accumulators = 2 Op::NS running sums per
// column; running sum q = 2 s + c (accumulator s, component c) of column j is table row (s * K + j) * 2 + c, and a scalar step reads
// Fin::NS sums per column in that numbering (the product's d.Ad lies the same way: rows 2 j, 2 j + 1).  Every pass leaves its sums
// for a tree (TREE bit 0); bit 1 says that `pin` holds a pass's sums, not the product's.
#include "multi_loop.hpp"
#include "multi_cplx.hpp"
#include "dense.hpp"

namespace lcgh {
namespace {

// ZMState, the z-helpers, zm_residual, the setup step ZMFinInit and the first step ZMFinAlpha: multi_cplx.hpp (solvers_multi_cbicg.hip
// runs them too)

// closing step of a body, per running column (clcg.cpp:330-347 and the next loop head :295-318; clcg_cuda.cu:507-517, :478-480)
template <int K, bool PCG> struct ZMFinClose {
    static constexpr int NS = 4;
    __device__ void operator()(ZMState *st, const double *sum) const
    {
        if (!st->all_done) {
#pragma unroll
            for (int j = 0; j < K; j++) {
                if (st->stop[j] != ST_RUNNING) continue;
                const double mm = sum[2 * j], r2 = sum[2 * j + 1];
                const double2 nw = make_double2(sum[(K + j) * 2], sum[(K + j) * 2 + 1]);
                st->m2[j] = mm; st->r2[j] = r2;
                st->t[j]++;
                const bool bad = PCG ? (mm != mm || r2 != r2 || nw.x != nw.x || nw.y != nw.y) : mm != mm;
                if (bad) { st->stop[j] = ST_NAN; continue; }
                zsts(st->bk, j, cdiv(nw, zld(st->rho, j)));
                zsts(st->rho, j, nw);
                const double r = zm_residual<PCG>(st, r2, mm);
                st->residual[j] = r;
                if (r <= st->eps) st->stop[j] = ST_CONVERGED;
            }
            all_stopped<K>(st);
        }
        mpublish(st);
    }
};

// ---- vector passes ----------------------------------------------------------------------------------------------------------------------
template <bool PCG> struct ZMOpInit {      // r = B - Ad; d = r (PCG: d = r / diag); |m|^2, |r|^2, r.r (r.d)    clcg.cpp:250-270, clcg_cuda.cu:441-457
    static constexpr int NS = 2;
    const double *Ad, *B, *m, *invdiag; double *r, *d;
    __device__ void prep(const ZMState &, int) {}
    __device__ void apply(long e, long row, bool, bool, m2d *acc)
    {
        const m2d rv = ld2(B, e) - ld2(Ad, e), mv = ld2(m, e);
        const m2d dv = PCG ? zmul(ld2(invdiag, row), rv) : rv;
        zst(r, e, rv); zst(d, e, dv);
        acc[0] += znorms(mv, rv); acc[1] += zmul(rv, dv);
    }
};
template <bool PCG> struct ZMOpUpdate {    // m += ak d; r -= ak Ad (PCG: s = r / diag); |m|^2, |r|^2, r.r (r.s)   clcg.cpp:323-345, clcg_cuda.cu:504-516
    static constexpr int NS = 2;
    double *m, *r, *s; const double *d, *Ad, *invdiag; m2d ak;
    __device__ void prep(const ZMState &L, int c) { ak.x = L.ak[2 * c]; ak.y = L.ak[2 * c + 1]; }
    __device__ void apply(long e, long row, bool, bool, m2d *acc)
    {
        const m2d mv = zfma(ak, ld2(d, e), ld2(m, e));
        const m2d rv = zfma(-ak, ld2(Ad, e), ld2(r, e));
        zst(m, e, mv); zst(r, e, rv);
        m2d sv = rv;
        if (PCG) { sv = zmul(ld2(invdiag, row), rv); zst(s, e, sv); }
        acc[0] += znorms(mv, rv); acc[1] += zmul(rv, sv);
    }
};
struct ZMOpDir {        // d = z + bk d (z: r, PCG: s)                           clcg.cpp:349-353, clcg_cuda.cu:519-520
    static constexpr int NS = 0;
    double *d; const double *z; m2d bk;
    __device__ void prep(const ZMState &L, int c) { bk.x = L.bk[2 * c]; bk.y = L.bk[2 * c + 1]; }
    __device__ void apply(long e, long, bool, bool, m2d *) { zst(d, e, zfma(bk, ld2(d, e), ld2(z, e))); }
};

// ---- host side (a column's stop word -> its code: zm_code, multi_cplx.hpp) ------------------------------------------------------------
// ---- the matrix, as the loop sees it (solvers_multi.hip's seam) ------------------------------------------------------------------------
// rows(), invdiag() (the complex Jacobi reciprocals), big_doubles(k) (what the product's carried sum needs on its way to the table)
// and apply(): Y = A.X for the K columns and, with U, column j's unconjugated (A.X)_j . U_j as *slots partial sums in `dots`, re in row
// 2 j and im in row 2 j + 1 (multi_cplx.hpp's table format)
struct ZCsrOp {
    lcg_hip_csr *A;
    int rows() const { return A->n_rows; }
    const double *invdiag() const { return A->invdiag; }
    size_t big_doubles(int k) const { return cspmm_big_doubles(A->main, k); }
    int apply(Ctx &c, int k, const double *X, double *Y, const int *done, const double *U = nullptr, double *big = nullptr,
              double *dots = nullptr, int *slots = nullptr) const
    {
        c.cnt_ax++;
        return cspmm_launch(A->main, k, X, Y, c.stream, done, U, big, dots, slots);
    }
};
// K of a square complex128 dense handle (dense_multi.hip: dnm_op): the product is two or three launches, all counted as products
struct ZDenseOp {
    lcg_hip_dense *D;
    int rows() const { return D->N; }
    const double *invdiag() const { return D->invdiag; }
    size_t big_doubles(int) const { return 0; }
    int apply(Ctx &c, int k, const double *X, double *Y, const int *done, const double *U = nullptr, double * = nullptr,
              double *dots = nullptr, int *slots = nullptr) const
    {
        int launches = 0;
        const int rc = dnm_op(D, k, 0, X, Y, c.stream, done, U, dots, slots, &launches);
        c.cnt_ax += launches;
        return rc;
    }
};

template <int K, bool PCG, class OpA>
static int run_zm(const OpA &A, double *M, const double *B, const clcg_para &p, int *ret, int *iterations, double *residual, int mem)
{
    MultiFrame<ZMState, K, K> f(A.rows());
    Ctx &c = f.c;
    TRY(f.open(mem, M, B));
    double *r = nullptr, *d = nullptr, *Ad = nullptr, *s = nullptr, *big = nullptr;
    TRY(f.vec(r));
    TRY(f.vec(d));
    TRY(f.vec(Ad));
    if (PCG) TRY(f.vec(s));
    const size_t nbig = A.big_doubles(K);
    if (nbig) TRY(f.ws.get(big, nullptr, sizeof(double) * nbig));
    TRY(f.start(f.tree_grid(), p.epsilon, p.abs_diff));

    // setup: A.m for the guess, d = r (PCG: r / diag), the verdict "already optimised"
    TRY(A.apply(c, K, M, Ad, nullptr));
    TRY((f.template pass<1, true>(MFinNone{}, ZMOpInit<PCG>{Ad, B, M, A.invdiag(), r, d}, nullptr, 0)));
    TRY((f.template pass<3, true>(ZMFinInit<K, PCG>{}, MOpNone{}, f.tab_sum, f.grid, 1)));

    int g_dot = 0;
    f.run(p.max_iterations, [&]() -> int {
        TRY(A.apply(c, K, d, Ad, &f.cur->all_done, d, big, f.tab_dot, &g_dot));
        TRY(f.template pass<1>(ZMFinAlpha<K>{}, ZMOpUpdate<PCG>{M, r, s, d, Ad, A.invdiag(), m2d()}, f.tab_dot, g_dot));
        TRY(f.template pass<3>(ZMFinClose<K, PCG>{}, ZMOpDir{d, PCG ? s : r, m2d()}, f.tab_sum, f.grid));
        return 0;
    });
    return f.finish(zm_code, ret, iterations, residual);
}

template <bool PCG>
static int zm_entry(const char *entry, lcg_hip_csr *A, int k, double *M, const double *B, const clcg_para *param, int *ret, int *iterations,
                    double *residual, int mem)
{
    clcg_para p;
    TRY(multi_args(entry, k, M, B));
    TRY(cmulti_handle(entry, A));
    TRY(multi_shape(entry, A->n_rows == A->n_cols, mem));
    TRY(multi_para<true>(param, p, A->n_rows));
    if (PCG && A->invdiag == nullptr) return LCG_NULL_PRECONDITION_MATRIX;  // lcg_hip_csr_build_jacobi has not run
    TRY(ensure_init());
    const ZCsrOp op{A};
    return multi_k(k, [&](auto K) { return run_zm<decltype(K)::value, PCG>(op, M, B, p, ret, iterations, residual, mem); });
}

// the dense entries: A = K, square; PCG with the reciprocals of lcg_hip_dense_build_jacobi(K, 0, ...)
template <bool PCG>
static int zm_dense_entry(const char *entry, const void *Kh, int k, double *M, const double *B, const clcg_para *param, int *ret,
                          int *iterations, double *residual, int mem)
{
    clcg_para p;
    TRY(multi_args(entry, k, M, B));
    lcg_hip_dense *D = dnm_handle(entry, Kh, true);
    if (!D) return LCG_HIP_E_ARG;
    TRY(multi_shape(entry, D->M == D->N, mem));
    TRY(multi_para<true>(param, p, D->N));
    if (PCG && D->invdiag == nullptr) return LCG_NULL_PRECONDITION_MATRIX;  // lcg_hip_dense_build_jacobi has not run
    TRY(ensure_init());
    TRY(dnm_reserve(D, k));
    const ZDenseOp op{D};
    return multi_k(k, [&](auto K) { return run_zm<decltype(K)::value, PCG>(op, M, B, p, ret, iterations, residual, mem); });
}

} // namespace
} // namespace lcgh

using namespace lcgh;

extern "C" {

int clcg_hip_lbicg_sym_multi(lcg_hip_csr_t A, int k, double *M, const double *B, const clcg_para *param, int *ret, int *iterations,
                             double *residual, int mem)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return zm_entry<false>("clcg_hip_lbicg_sym_multi", A, k, M, B, param, ret, iterations, residual, mem);
}

int clcg_hip_lpcg_multi(lcg_hip_csr_t A, int k, double *M, const double *B, const clcg_para *param, int *ret, int *iterations,
                        double *residual, int mem)
{
    NOT_DENSE(A, LCG_HIP_E_ARG);
    return zm_entry<true>("clcg_hip_lpcg_multi", A, k, M, B, param, ret, iterations, residual, mem);
}

int clcg_hip_dense_lbicg_sym_multi(lcg_hip_dense_t K, int k, double *M, const double *B, const clcg_para *param, int *ret, int *iterations,
                                   double *residual, int mem)
{
    return zm_dense_entry<false>("clcg_hip_dense_lbicg_sym_multi", K, k, M, B, param, ret, iterations, residual, mem);
}

int clcg_hip_dense_lpcg_multi(lcg_hip_dense_t K, int k, double *M, const double *B, const clcg_para *param, int *ret, int *iterations,
                              double *residual, int mem)
{
    return zm_dense_entry<true>("clcg_hip_dense_lpcg_multi", K, k, M, B, param, ret, iterations, residual, mem);
}

} // extern "C"

