// solvers_multi_cplx.hip -- batched complex loops over k = 2, 4, 8 right-hand sides against one complex-symmetric complex128 matrix:
// clcg_hip_lbicg_sym_multi (clbicg_symmetric, clcg.cpp:228-364) and clcg_hip_lpcg_multi (clpcg with the handle's reciprocal Jacobi
// diagonal, clcg_cuda.cu:403-558).
//
// Each column runs the reference's recurrence as if it were alone: its own ak, bk and rr (PCG: r.s), both inner products
// UNCONJUGATED (clcg_dot, cublasZdotu), its own stop test, "already optimised" test, count and code.  What the columns share is the
// matrix: one multi-vector product per iteration (csr_multi_cplx.hip) reads col / val once for all of them.
//
// Three launches per iteration, every scalar step in the prologue of the pass that consumes it (k_cvecf below, k_mvecf's complex twin):
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
// sums as ONE binary tree over leaves that depend on n alone (multi_cplx.hpp: ctree_leaves; multi.hpp: msum_tree).
#include "multi_loop.hpp"
#include "multi_cplx.hpp"

namespace lcgh {
namespace {

struct ZMState {
    double ak[2 * MM_MAXK], bk[2 * MM_MAXK], rho[2 * MM_MAXK];      // complex: re at [2 j], im at [2 j + 1]; rho = r.r (PCG: r.s)
    double m2[MM_MAXK], r2[MM_MAXK], residual[MM_MAXK];              // sum |m|^2, sum |r|^2 as they were last added up
    double eps, n_global;
    int t[MM_MAXK];         // completed iterations (the reference's t), per column
    int stop[MM_MAXK];      // ST_RUNNING, or why the column stopped (ST_CONVERGED, ST_NAN, ST_ALREADY)
    int abs_diff;
    int it;                 // iteration bodies started
    int all_done;           // every column has stopped: every later kernel is a no-op
    int pub_mask;           // HostStatus is refreshed when (it & pub_mask) == 0, and when all columns have stopped
    HostStatus *host;
};
static_assert(sizeof(ZMState) % 8 == 0, "ZMState is copied in 8-byte words");
constexpr size_t ZMSLOT = 1024;
static_assert(sizeof(ZMState) <= ZMSLOT, "two states share one small pool vector");

__global__ void k_zminit(ZMState *st, double eps, double n_global, int abs_diff, int pub_mask, HostStatus *host)
{
    double *w = reinterpret_cast<double *>(st);
    for (int i = threadIdx.x; i < (int)(sizeof(ZMState) / 8); i += blockDim.x) w[i] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) { st->eps = eps; st->n_global = n_global; st->abs_diff = abs_diff; st->pub_mask = pub_mask; st->host = host; }
}

__device__ __forceinline__ m2d zmul(m2d a, m2d b) { m2d r; r.x = a.x * b.x - a.y * b.y; r.y = a.x * b.y + a.y * b.x; return r; }
__device__ __forceinline__ m2d zfma(m2d a, m2d b, m2d c)     // a * b + c, cfma's order (devcommon.hpp)
{
    m2d r; r.x = fma(a.x, b.x, fma(-a.y, b.y, c.x)); r.y = fma(a.x, b.y, fma(a.y, b.x, c.y)); return r;
}
__device__ __forceinline__ m2d znorms(m2d a, m2d b) { m2d r; r.x = a.x * a.x + a.y * a.y; r.y = b.x * b.x + b.y * b.y; return r; }
__device__ __forceinline__ void zst(double *p, long e, m2d v) { reinterpret_cast<m2d *>(p)[e] = v; }

// ---- the k-wide complex vector pass ---------------------------------------------------------------------------------------------------
// k_mvecf (multi_loop.hpp) for blocks of complex columns: one fused pass over n2 = n * K pieces, piece e = row e / K of column e % K,
// with the scalar step `fin` in its prologue.  The grid is ctree_leaves(n) * K / VB workgroups, so the thread of piece e adds rows
// (e / K) + m ctree_leaves(n), m = 0, 1, ... in order, whatever K is; the workgroup adds its threads' sums as a binary tree over
// consecutive leaves (lanes by xor K, 2 K, ... 32, then wavefronts 0 + 1, 2 + 3) and msum_tree adds the workgroups' sums: one tree
// over the leaves, the same for K = 2, 4, 8.  An Op keeps Op::NS 16-byte accumulators = 2 Op::NS running sums per column; running sum
// q = 2 s + c (accumulator s, component c) of column j is table row (s * K + j) * 2 + c, and fin reads Fin::NS sums per column in that
// numbering (the product's d.Ad lies the same way: rows 2 j, 2 j + 1).  PIN_TREE: `pin` holds a pass's sums (msum_tree), else a
// product's (msum).  ALL: every column is worked on whatever its stop word says (the setup passes).
// Op provides: static constexpr int NS;  void prep(const S &, int column);  void apply(long e, long row, m2d *acc)
template <class S, int K, class Fin, class Op, bool ALL, bool PIN_TREE>
__global__ __launch_bounds__(VB) void k_cvecf(Fin fin, Op op, long n2, const double *pin, int gin, double *pout, const S *cur, S *next)
{
    constexpr int NSF = Fin::NS > 0 ? Fin::NS * K : 1, NSO = Op::NS > 0 ? Op::NS : 1;
    static_assert(VB % K == 0 && 64 % K == 0, "a thread's column never changes");
    __shared__ S L;
    __shared__ double sums[NSF];
    __shared__ double wsh[VB / 64][NSO][K][2];
    {
        const double *src = reinterpret_cast<const double *>(cur);
        double *dst = reinterpret_cast<double *>(&L);
        for (int i = threadIdx.x; i < (int)(sizeof(S) / 8); i += VB) dst[i] = src[i];
    }
    if (Fin::NS > 0) {                              // (both end with a barrier: L and sums are complete)
        if (PIN_TREE) msum_tree<NSF>(pin, gin, sums);
        else msum<NSF>(pin, gin, sums);
    }
    else __syncthreads();
    if (threadIdx.x == 0) {
        if (blockIdx.x != 0) L.host = nullptr;
        fin(&L, sums);
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        const double *src = reinterpret_cast<const double *>(&L);
        double *dst = reinterpret_cast<double *>(next);
        for (int i = threadIdx.x; i < (int)(sizeof(S) / 8); i += VB) dst[i] = src[i];
    }
    if (L.all_done && !ALL) return;
    // (gridDim.x * VB and VB are multiples of K: this thread's pieces all belong to column col)
    const int col = (int)threadIdx.x % K;
    const bool run = ALL || L.stop[col] == ST_RUNNING;
    op.prep(L, col);
    m2d acc[NSO];
#pragma unroll
    for (int s = 0; s < NSO; s++) acc[s] = (m2d)(0.0);
    if (run) {
        const long stride = (long)gridDim.x * VB;
        for (long e = (long)blockIdx.x * VB + threadIdx.x; e < n2; e += stride) op.apply(e, e / K, acc);
    }
    if (Op::NS > 0) {
        // lanes l, l + K, l + 2 K, ... of a wavefront hold the same column: xor-butterfly over them, adjacent leaves first
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
        for (int s = 0; s < NSO; s++) {
            double x = acc[s].x, y = acc[s].y;
#pragma unroll
            for (int off = K; off <= 32; off <<= 1) { x += __shfl_xor(x, off, 64); y += __shfl_xor(y, off, 64); }
            if (lane < K) { wsh[w][s][lane][0] = x; wsh[w][s][lane][1] = y; }
        }
        __syncthreads();
        if (threadIdx.x < NSO * K * 2) {
            const int s = threadIdx.x / (2 * K), j = (threadIdx.x / 2) % K, c = threadIdx.x & 1;
            static_assert(VB / 64 == 4, "the tree over the wavefronts");
            const double v = (wsh[0][s][j][c] + wsh[1][s][j][c]) + (wsh[2][s][j][c] + wsh[3][s][j][c]);
            pout[((s * K + j) * 2 + c) * MM_MG + blockIdx.x] = v;
        }
    }
}

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

// setup.  Sums |m|^2, |r|^2, rho (BiCG-sym: r.r; PCG: r.s).  BiCG-sym tries BOTH "already optimised" criteria in abs_diff mode, in the
// reference's order (clcg.cpp:273-290); PCG only its mode's own (clcg_cuda.cu:456-466)
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
// first step of a body: counts it; ak = rho / d.Ad per running column (clcg.cpp:320-321, clcg_cuda.cu:501-502).  Sums: the product's
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
    __device__ void apply(long e, long row, m2d *acc)
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
    __device__ void apply(long e, long row, m2d *acc)
    {
        const m2d mv = zfma(ak, ld2(d, e), ld2(m, e));
        const m2d rv = zfma(-ak, ld2(Ad, e), ld2(r, e));
        zst(m, e, mv); zst(r, e, rv);
        m2d sv = rv;
        if (PCG) { sv = zmul(ld2(invdiag, row), rv); zst(s, e, sv); }
        acc[0] += znorms(mv, rv); acc[1] += zmul(rv, sv);
    }
};
struct ZMOpNone {
    static constexpr int NS = 0;
    __device__ void prep(const ZMState &, int) {}
    __device__ void apply(long, long, m2d *) {}
};
struct ZMOpDir {        // d = z + bk d (z: r, PCG: s)                           clcg.cpp:349-353, clcg_cuda.cu:519-520
    static constexpr int NS = 0;
    double *d; const double *z; m2d bk;
    __device__ void prep(const ZMState &L, int c) { bk.x = L.bk[2 * c]; bk.y = L.bk[2 * c + 1]; }
    __device__ void apply(long e, long, m2d *) { zst(d, e, zfma(bk, ld2(d, e), ld2(z, e))); }
};

// ---- host side ------------------------------------------------------------------------------------------------------------------------
template <int K>
struct ZMSolve {
    Ctx &c;
    long n2;
    int grid;
    ZMState *cur, *next;
    double *tab_dot, *tab_sum;      // the k-wide tables: the product's partial sums (d.Ad), the update pass's

    template <bool PIN_TREE, class Fin, class Op, bool ALL = false> int pass(Fin fin, Op op, const double *pin, int gin, int g = 0)
    {
        c.cnt_vec++;
        hipLaunchKernelGGL((k_cvecf<ZMState, K, Fin, Op, ALL, PIN_TREE>), dim3(g ? g : grid), dim3(VB), 0, c.stream, fin, op, n2, pin, gin, tab_sum, cur, next);
        HIPCHK(hipGetLastError());
        std::swap(cur, next);
        return 0;
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

template <int K, bool PCG>
static int run_zm(lcg_hip_csr *A, double *M, const double *B, const clcg_para &p, int *ret, int *iterations, double *residual, int mem)
{
    Ctx &c = ctx();
    const int n = A->n_rows;
    const size_t nb = sizeof(double) * 2 * (size_t)n * K;
    HostBridge hb;
    Workspace ws;
    SolveGuard guard(c);
    TRY(hb.open(mem, M, B, nb, c.stream));
    double *r = nullptr, *d = nullptr, *Ad = nullptr, *s = nullptr, *big = nullptr, *stmem = nullptr;
    TRY(ws.get(r, nullptr, nb));
    TRY(ws.get(d, nullptr, nb));
    TRY(ws.get(Ad, nullptr, nb));
    if (PCG) TRY(ws.get(s, nullptr, nb));
    const size_t nbig = cspmm_big_doubles(A->main, K);
    if (nbig) TRY(ws.get(big, nullptr, sizeof(double) * nbig));
    TRY(ws.get(stmem, nullptr, 2 * ZMSLOT));

    const CsrPart &P = A->main;
    ZMSolve<K> k{c, (long)n * K, 0, reinterpret_cast<ZMState *>(stmem),
                 reinterpret_cast<ZMState *>(reinterpret_cast<char *>(stmem) + ZMSLOT), c.partials_pair[0], c.partials_pair[1]};
    k.grid = (int)(ctree_leaves(n) * K / VB);       // a thread's rows do not depend on K
    const long work = (long)n * K * 2;
    c.hstat->it = 0; c.hstat->done = 0; c.hstat->status = 0; c.hstat->t = 0; c.hstat->residual = 0.0;
    hipLaunchKernelGGL(k_zminit, dim3(1), dim3(64), 0, c.stream, k.cur, p.epsilon, (double)n, p.abs_diff, work >= (1 << 20) ? 0 : 3, c.hstat_dev);
    HIPCHK(hipGetLastError());

    // setup: A.m for the guess, d = r (PCG: r / diag), the verdict "already optimised"
    c.cnt_ax++;
    TRY(cspmm_launch(P, K, M, Ad, c.stream, nullptr));
    TRY((k.template pass<false, MFinNone, ZMOpInit<PCG>, true>(MFinNone{}, ZMOpInit<PCG>{Ad, B, M, A->invdiag, r, d}, nullptr, 0)));
    TRY((k.template pass<true, ZMFinInit<K, PCG>, ZMOpNone, true>(ZMFinInit<K, PCG>{}, ZMOpNone{}, k.tab_sum, k.grid, 1)));

    int g_dot = 0;
    auto body = [&]() -> int {
        c.cnt_ax++;
        TRY(cspmm_launch(P, K, d, Ad, c.stream, &k.cur->all_done, d, big, k.tab_dot, &g_dot));
        TRY((k.template pass<false>(ZMFinAlpha<K>{}, ZMOpUpdate<PCG>{M, r, s, d, Ad, A->invdiag, m2d()}, k.tab_dot, g_dot)));
        TRY((k.template pass<true>(ZMFinClose<K, PCG>{}, ZMOpDir{d, PCG ? s : r, m2d()}, k.tab_sum, k.grid)));
        return 0;
    };

    ZMState h;
    auto read_state = [&]() -> int {
        HIPCHK(hipMemcpyAsync(&h, k.cur, sizeof h, hipMemcpyDeviceToHost, c.stream));
        HIPCHK(hipStreamSynchronize(c.stream));
        return 0;
    };
    const int rc = enqueue_ahead(c, p.max_iterations, work >= (1 << 20) ? 6 : 24, body, read_state, h);
    if (!rc) {
        int longest = 0;
        for (int j = 0; j < K; j++) {
            if (ret) ret[j] = zm_code(h.stop[j]);
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

template <bool PCG>
static int zm_entry(const char *entry, lcg_hip_csr *A, int k, double *M, const double *B, const clcg_para *param, int *ret, int *iterations,
                    double *residual, int mem)
{
    TRY(multi_args(entry, k, M, B));
    TRY(cmulti_handle(entry, A));
    if (A->n_rows != A->n_cols) { ctx().err = std::string(entry) + ": the matrix is not square"; return LCG_HIP_E_ARG; }
    if (mem != LCG_HIP_MEM_HOST && mem != LCG_HIP_MEM_DEVICE) { ctx().err = std::string(entry) + ": mem is neither LCG_HIP_MEM_HOST nor LCG_HIP_MEM_DEVICE"; return LCG_HIP_E_ARG; }
    const clcg_para p = param ? *param : clcg_hip_default_parameters();
    if (A->n_rows <= 0) return CLCG_INVILAD_VARIABLE_SIZE;
    if (p.max_iterations < 0) return CLCG_INVILAD_MAX_ITERATIONS;           // clcg.cpp:235-240
    if (p.epsilon <= 0.0 || p.epsilon >= 1.0) return CLCG_INVILAD_EPSILON;
    if (PCG && A->invdiag == nullptr) return LCG_NULL_PRECONDITION_MATRIX;  // lcg_hip_csr_build_jacobi has not run
    TRY(ensure_init());
    if (k == 2) return run_zm<2, PCG>(A, M, B, p, ret, iterations, residual, mem);
    if (k == 4) return run_zm<4, PCG>(A, M, B, p, ret, iterations, residual, mem);
    return run_zm<8, PCG>(A, M, B, p, ret, iterations, residual, mem);
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

} // extern "C"
