// multi_loop.hpp -- what the batched loops (solvers_multi.hip: CG, PCG; solvers_multi_bicg.hip: BiCGStab; solvers_multi_cplx.hip: complex
// BiCG-sym, PCG) share: the head of their device state, the fused k-wide vector pass with a scalar step in its prologue, its loads and
// frozen-column stores, the frame of one solve (setup, launcher, the host's enqueue-ahead loop, teardown) and the entries' refusals.
// Not installed.
//
// A loop brings its own state S: MultiHead plus its coefficient arrays (double residual[MM_MAXK] among them), a plain struct of 8-byte
// words that lives in a pair of device buffers (a pass reads one and commits the other) and is copied word-wise into LDS and to the host.
#pragma once

#include "multi.hpp"
#include "csr_tri.hpp"

namespace lcgh {

struct MultiHead {
    double eps, n_global;
    int t[MM_MAXK];         // completed iterations (the reference's t), per column
    int stop[MM_MAXK];      // ST_RUNNING, or why the column stopped (ST_CONVERGED, ST_NAN, ST_ALREADY)
    int abs_diff;
    int it;                 // iteration bodies started
    int all_done;           // every column has stopped: every later kernel is a no-op
    int pub_mask;           // HostStatus is refreshed when (it & pub_mask) == 0, and when all columns have stopped
    HostStatus *host;
};
constexpr size_t MM_SLOT = 1024;    // two states share one small pool vector

template <class S> __global__ void k_state_init(S *st, double eps, double n_global, int abs_diff, int pub_mask, HostStatus *host)
{
    double *w = reinterpret_cast<double *>(st);
    for (int i = threadIdx.x; i < (int)(sizeof(S) / 8); i += blockDim.x) w[i] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) { st->eps = eps; st->n_global = n_global; st->abs_diff = abs_diff; st->pub_mask = pub_mask; st->host = host; }
}

template <class S> __device__ __forceinline__ void mpublish(S *st)
{
    HostStatus *h = st->host;
    if (!h) return;         // a block's private copy: only block 0 mirrors to the host
    if (!st->all_done && (st->it & st->pub_mask)) return;
    h->done = st->all_done;
    h->it = st->it;         // (posted writes: the host paces itself on them and reads the state with a real copy before it returns)
}
template <int K, class S> __device__ __forceinline__ void all_stopped(S *st)
{
    int all = 1;
#pragma unroll
    for (int j = 0; j < K; j++) all &= st->stop[j] != ST_RUNNING;
    st->all_done = all;
}

// ---- scalar steps: sums[s * K + j] = running sum s of column j ------------------------------------------------------------------
struct MFinNone {
    static constexpr int NS = 0;
    template <class S> __device__ void operator()(S *, const double *) const {}
};
// the real loops' stop rule out of the residual's numerator g2 and the clamped |m|^2 (lcg.cpp:208-222, 694-708)
template <class S> __device__ __forceinline__ double m_residual(const S *st, double g2, double m2)
{
    return st->abs_diff ? sqrt(g2) / st->n_global : g2 / m2;
}
// their setup verdict for column j: "already optimised" -- in abs_diff mode BOTH criteria are tried, the mode's own first
// (lcg.cpp:178-203, 341-359, 658-689)
template <class S> __device__ __forceinline__ void m_already(S *st, int j, double g2, double m2)
{
    double r;
    bool already = false;
    if (st->abs_diff && sqrt(g2) / st->n_global <= st->eps) { r = sqrt(g2) / st->n_global; already = true; }
    else if (g2 / m2 <= st->eps) { r = g2 / m2; already = true; }
    else r = m_residual(st, g2, m2);
    st->residual[j] = r;
    st->stop[j] = already ? ST_ALREADY : ST_RUNNING;
}

// ---- vector passes ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ m2d ld2(const double *p, long e) { return reinterpret_cast<const m2d *>(p)[e]; }
// only the running halves of a piece are written: a stopped column's bytes are never stored to again
__device__ __forceinline__ void st2(double *p, long e, m2d v, bool r0, bool r1)
{
    if (r0 && r1) reinterpret_cast<m2d *>(p)[e] = v;
    else if (r0) p[2 * e] = v.x;
    else if (r1) p[2 * e + 1] = v.y;
}
__device__ __forceinline__ m2d nan2(m2d v) { m2d f; f.x = v.x != v.x ? 1.0 : 0.0; f.y = v.y != v.y ? 1.0 : 0.0; return f; }

// Op provides: static constexpr int NS;  void prep(const S &, int c0) (the coefficients of the thread's first column c0);
//              void apply(long e, long row, bool r0, bool r1, m2d *acc)
struct MOpNone {
    static constexpr int NS = 0;
    template <class S> __device__ void prep(const S &, int) {}
    __device__ void apply(long, long, bool, bool, m2d *) {}
};
// One fused pass over n2 = n * G 16-byte pieces with the scalar step `fin` in its prologue.  G: the pieces of a row, = the lanes that
// share it.  Real blocks: G = K / 2, a piece holds columns c0, c0 + 1, r0 and r1 say which of them runs.  Complex blocks: G = K, a
// piece is one complex element of column c0, r0 and r1 are the same flag and a thread whose column has stopped does nothing, so its
// Ops store whole pieces.  An Op keeps Op::NS 16-byte accumulators; component c of accumulator s of lane l goes to table row
// s * 2 G + 2 l + c, which is (s * K + j) for the real column j = 2 l + c and (s * K + j) * 2 + c for the complex column j = l, and fin
// reads Fin::NS * K sums in that numbering.  ALL: every column is worked on whatever its stop word says (the setup passes, before the
// words mean anything).
// TREE: a column's sums must not depend on K either.  The grid is tree_leaves(n, ...) * G / VB workgroups, so the thread of piece e adds
// rows (e / G) + m tree_leaves, m = 0, 1, ... in order, whatever K is.  Bit 0: the workgroup adds its threads' sums as a binary tree
// over consecutive leaves (lanes by xor G, 2 G, ... 32, then wavefronts 0 + 1, 2 + 3); bit 1: `pin` holds such partials and
// msum_tree adds them (else a product's, msum).  Together: one tree over the leaves, the same for K = 2, 4, 8.
template <class S, int K, int G, class Fin, class Op, bool ALL, int TREE = 0>
__global__ __launch_bounds__(VB) void k_mvecf(Fin fin, Op op, long n2, const double *pin, int gin, double *pout, const S *cur, S *next)
{
    constexpr int NSF = Fin::NS > 0 ? Fin::NS * K : 1, NSO = Op::NS > 0 ? Op::NS : 1;
    static_assert((G == K || 2 * G == K) && VB % G == 0 && 64 % G == 0, "a thread's columns never change");
    __shared__ S L;
    __shared__ double sums[NSF];
    __shared__ double wsh[VB / 64][NSO][2 * G];
    {
        const double *src = reinterpret_cast<const double *>(cur);
        double *dst = reinterpret_cast<double *>(&L);
        for (int i = threadIdx.x; i < (int)(sizeof(S) / 8); i += VB) dst[i] = src[i];
    }
    if (Fin::NS > 0) {                              // (both end with a barrier: L and sums are complete)
        if (TREE & 2) msum_tree<NSF>(pin, gin, sums);
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
    // (gridDim.x * VB and VB are multiples of G: this thread's pieces all belong to columns c0 .. c1)
    const int c0 = (K / G) * ((int)threadIdx.x % G), c1 = c0 + K / G - 1;
    const bool r0 = ALL || L.stop[c0] == ST_RUNNING, r1 = ALL || L.stop[c1] == ST_RUNNING;
    op.prep(L, c0);
    m2d acc[NSO];
#pragma unroll
    for (int s = 0; s < NSO; s++) acc[s] = (m2d)(0.0);
    if (r0 || r1) {
        const long stride = (long)gridDim.x * VB;
        for (long e = (long)blockIdx.x * VB + threadIdx.x; e < n2; e += stride) op.apply(e, e / G, r0, r1, acc);
    }
    if (Op::NS > 0) {
        // lanes l, l + G, l + 2 G, ... of a wavefront hold the same columns: xor-butterfly over them, then the wavefronts in order
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
        for (int s = 0; s < NSO; s++) {
            double x = acc[s].x, y = acc[s].y;
            if (TREE & 1) {
#pragma unroll
                for (int off = G; off <= 32; off <<= 1) { x += __shfl_xor(x, off, 64); y += __shfl_xor(y, off, 64); }
            } else {
#pragma unroll
                for (int off = 32; off >= G; off >>= 1) { x += __shfl_xor(x, off, 64); y += __shfl_xor(y, off, 64); }
            }
            if (lane < G) { wsh[w][s][2 * lane] = x; wsh[w][s][2 * lane + 1] = y; }
        }
        __syncthreads();
        if (threadIdx.x < NSO * 2 * G) {
            const int s = threadIdx.x / (2 * G), q = threadIdx.x % (2 * G);
            double v = 0.0;
            static_assert(VB / 64 == 4, "the tree over the wavefronts");
            if (TREE & 1) v = (wsh[0][s][q] + wsh[1][s][q]) + (wsh[2][s][q] + wsh[3][s][q]);
            else {
#pragma unroll
                for (int p = 0; p < VB / 64; p++) v += wsh[p][s][q];
            }
            pout[(s * 2 * G + q) * MM_MG + blockIdx.x] = v;
        }
    }
}

struct SolveGuard {     // what ~Driver does for the single-vector loops
    Ctx &c;
    explicit SolveGuard(Ctx &c_) : c(c_) { c.in_solve = true; c.ax_rc = 0; c.cnt_vec = c.cnt_scal = c.cnt_allreduce = c.cnt_ax = 0; }
    ~SolveGuard() { c.in_solve = false; }
};

// ---- host side ------------------------------------------------------------------------------------------------------------------------
inline int lcg_code(int stop)
{
    switch (stop) {
    case ST_ALREADY: return LCG_ALREADY_OPTIMIZIED;
    case ST_NAN: return LCG_NAN_VALUE;
    case ST_CONVERGED: return LCG_CONVERGENCE;
    default: return LCG_REACHED_MAX_ITERATIONS;
    }
}

// The asynchronous loop of driver.hpp: the host only enqueues, at most `inflight` bodies ahead of the device.  body() enqueues one
// iteration, read_state() copies the device's latest state into h and waits for it.  Ends with h read (0), or a failure's code.
template <class S, class Body, class Read>
int enqueue_ahead(Ctx &c, int max_iterations, int inflight, Body body, Read read_state, S &h)
{
    int enq = 0, rc = 0;
    for (;;) {
        if (max_iterations > 0 && enq >= max_iterations) break;
        rc = body(); if (rc) break;
        enq++;
        if (c.hstat->done) break;
        int spins = 0;
        while (c.hstat->it < enq - inflight && !c.hstat->done) {
            if (++spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(20));
            if (spins > 200000) {   // backstop: the mapped mirror is not advancing
                rc = read_state(); if (rc) break;
                if (h.all_done || h.it >= enq - inflight) break;
                spins = 0;
            }
        }
        if (rc) break;
        if ((enq & 255) == 0) {     // authoritative check now and then
            rc = read_state(); if (rc) break;
            if (h.all_done) break;
        }
    }
    if (!rc) rc = read_state();
    return rc;
}

// One batched solve, the counterpart of driver.hpp's Solve: after the entry's checks and ensure_init(), in this order: open() (M and B
// onto the device when they live in host memory), vec() (the work vectors -- the ORDER of the calls decides which pool vector a role
// receives), start() (the state pair, the init launch), the setup passes, run(), finish().  Destruction runs in reverse: the guard,
// the Workspace (its vectors back to the pool), the HostBridge.
template <class S, int K, int G>
struct MultiFrame {
    static_assert(sizeof(S) % 8 == 0 && sizeof(S) <= MM_SLOT, "a state is copied in 8-byte words, and two share one small pool vector");
    Ctx &c;
    HostBridge hb;
    Workspace ws;
    SolveGuard guard;
    const long n2;                  // 16-byte pieces of a k-wide vector
    int grid = 0;                   // workgroups of a vector pass
    S *cur = nullptr, *next = nullptr;
    double *tab_dot, *tab_sum;      // the k-wide tables: the products' partial sums, the passes'
    S h;                            // the state as run() last read it
    int rc = 0;

    explicit MultiFrame(int n) : c(ctx()), guard(c), n2((long)n * G), tab_dot(c.partials_pair[0]), tab_sum(c.partials_pair[1]) {}

    int open(int mem, double *&M, const double *&B) { return hb.open(mem, M, B, 16 * (size_t)n2, c.stream); }
    int vec(double *&out) { return ws.get(out, nullptr, 16 * (size_t)n2); }
    // a TREE pass's grid: a thread's rows do not depend on K
    int tree_grid() const { return (int)(tree_leaves(n2 / G, G * MM_MAXK / K) * G / VB); }
    int start(int grid_, double eps, int abs_diff)
    {
        double *stmem = nullptr;
        TRY(ws.get(stmem, nullptr, 2 * MM_SLOT));
        cur = reinterpret_cast<S *>(stmem);
        next = reinterpret_cast<S *>(reinterpret_cast<char *>(stmem) + MM_SLOT);
        grid = grid_;
        c.hstat->it = 0; c.hstat->done = 0; c.hstat->status = 0; c.hstat->t = 0; c.hstat->residual = 0.0;
        hipLaunchKernelGGL(k_state_init<S>, dim3(1), dim3(64), 0, c.stream, cur, eps, (double)(n2 / G), abs_diff, big_work() ? 0 : 3, c.hstat_dev);
        HIPCHK(hipGetLastError());
        return 0;
    }
    bool big_work() const { return 2 * n2 >= (1 << 20); }      // doubles of a vector: publish every iteration, fewer bodies in flight

    // TREE: k_mvecf -- 1: this pass leaves sums for a tree, 2: it adds up such a pass's sums (else a product's, or a plain pass's)
    template <int TREE, bool ALL = false, class Fin, class Op> int pass(Fin fin, Op op, const double *pin, int gin, int g = 0)
    {
        c.cnt_vec++;
        hipLaunchKernelGGL((k_mvecf<S, K, G, Fin, Op, ALL, TREE>), dim3(g ? g : grid), dim3(VB), 0, c.stream, fin, op, n2, pin, gin, tab_sum, cur, next);
        HIPCHK(hipGetLastError());
        std::swap(cur, next);
        return 0;
    }
    template <class Body> void run(int max_iterations, Body body)
    {
        auto read_state = [&]() -> int {
            HIPCHK(hipMemcpyAsync(&h, cur, sizeof h, hipMemcpyDeviceToHost, c.stream));
            HIPCHK(hipStreamSynchronize(c.stream));
            return 0;
        };
        rc = enqueue_ahead(c, max_iterations, big_work() ? 6 : 24, body, read_state, h);
    }
    // code: a column's stop word -> its return code
    int finish(int (*code)(int), int *ret, int *iterations, double *residual)
    {
        if (!rc) {
            int longest = 0;
            for (int j = 0; j < K; j++) {
                if (ret) ret[j] = code(h.stop[j]);
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
};

// ---- the entries' refusals, after multi_args and the handle's own check -----------------------------------------------------------------
inline int multi_shape(const char *entry, bool square, int mem, const char *why = "")
{
    if (!square) { ctx().err = std::string(entry) + ": the matrix is not square" + why; return LCG_HIP_E_ARG; }
    if (mem != LCG_HIP_MEM_HOST && mem != LCG_HIP_MEM_DEVICE) { ctx().err = std::string(entry) + ": mem is neither LCG_HIP_MEM_HOST nor LCG_HIP_MEM_DEVICE"; return LCG_HIP_E_ARG; }
    return 0;
}
// the caller's parameters or the defaults, and the reference's range checks (lcg.cpp:150-155, 637-638; clcg.cpp:235-240)
template <bool CPLX> int multi_para(const typename SolveTypes<CPLX>::Para *param, typename SolveTypes<CPLX>::Para &p, int n)
{
    if constexpr (CPLX) p = param ? *param : clcg_hip_default_parameters();
    else p = param ? *param : lcg_hip_default_parameters();
    if (CPLX && n <= 0) return CLCG_INVILAD_VARIABLE_SIZE;
    if (p.max_iterations < 0) return CPLX ? (int)CLCG_INVILAD_MAX_ITERATIONS : (int)LCG_INVILAD_MAX_ITERATIONS;
    if (p.epsilon <= 0.0 || p.epsilon >= 1.0) return CPLX ? (int)CLCG_INVILAD_EPSILON : (int)LCG_INVILAD_EPSILON;
    return 0;
}
// precond -> the built-in Jacobi, or a triangular factor of the handle, or neither (LCG_HIP_M_NONE, where none_ok).  A value that is
// not allowed is refused here; `built` says whether what it names exists (need_diag: the loop reads the Jacobi reciprocals) -- the
// caller returns LCG_NULL_PRECONDITION_MATRIX for that AFTER the parameters' checks, as the entries always have
struct MultiPrecond { bool jac = false; TriFactor *F = nullptr; bool built = false; };
inline int multi_precond(const char *entry, const lcg_hip_csr *A, int precond, bool none_ok, bool need_diag, MultiPrecond &m)
{
    if (!(none_ok && precond == LCG_HIP_M_NONE) && precond != LCG_HIP_M_JACOBI && precond != LCG_HIP_M_IC0 && precond != LCG_HIP_M_ILU0) {
        ctx().err = std::string(entry) + ": precond is none of " + (none_ok ? "LCG_HIP_M_NONE, " : "") + "LCG_HIP_M_JACOBI, LCG_HIP_M_IC0, LCG_HIP_M_ILU0";
        return LCG_HIP_E_ARG;
    }
    m.jac = precond == LCG_HIP_M_JACOBI;
    m.F = precond == LCG_HIP_M_IC0 ? A->ic0 : precond == LCG_HIP_M_ILU0 ? A->ilu0 : nullptr;
    // lcg_hip_csr_build_jacobi / _ic0 / _ilu0 has not run (or the factor's pivot failed)
    m.built = m.jac ? !need_diag || A->invdiag != nullptr : precond == LCG_HIP_M_NONE || (m.F && m.F->ok);
    return 0;
}
} // namespace lcgh
