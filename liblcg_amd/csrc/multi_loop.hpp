// multi_loop.hpp -- what the batched loops (solvers_multi.hip: CG, PCG; solvers_multi_bicg.hip: BiCGStab) share: the fused k-wide
// vector pass with a scalar step in its prologue, its loads and frozen-column stores, the host's enqueue-ahead loop.  Not installed.
//
// A loop brings its own state S, a struct of 8-byte words that lives in a pair of device buffers (a pass reads one and commits the
// other).  What this file needs of it:  int stop[MM_MAXK] (ST_RUNNING, or why the column stopped), it (iteration bodies started),
// all_done, pub_mask;  HostStatus *host.
#pragma once

#include "multi.hpp"

namespace lcgh {

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

// Op provides: static constexpr int NS;  void prep(const S &, int c0) (the coefficients of columns c0, c0 + 1);
//              void apply(long e, long row, bool r0, bool r1, m2d *acc)
struct MOpNone {
    static constexpr int NS = 0;
    template <class S> __device__ void prep(const S &, int) {}
    __device__ void apply(long, long, bool, bool, m2d *) {}
};
// One fused pass over n2 = n * K / 2 pieces with the scalar step `fin` in its prologue.  ALL: every column is worked on whatever its
// stop word says (the setup passes, before the words mean anything).
// TREE (BiCGStab): a column's sums must not depend on K either.  The grid is tree_leaves(n) * K2 / VB workgroups, so the thread of
// piece e adds rows (e / K2) + m tree_leaves(n), m = 0, 1, ... in order, whatever K is.  Bit 0: the workgroup adds its threads' sums as
// a binary tree over consecutive leaves (lanes by xor K2, 2 K2, ... 32, then wavefronts 0 + 1, 2 + 3); bit 1: `pin` holds such
// partials and msum_tree adds them.  Together: one tree over the leaves, the same for K = 2, 4, 8.
template <class S, int K, class Fin, class Op, bool ALL, int TREE = 0>
__global__ __launch_bounds__(VB) void k_mvecf(Fin fin, Op op, long n2, const double *pin, int gin, double *pout, const S *cur, S *next)
{
    constexpr int K2 = K / 2;
    constexpr int NSF = Fin::NS > 0 ? Fin::NS * K : 1, NSO = Op::NS > 0 ? Op::NS : 1;
    __shared__ S L;
    __shared__ double sums[NSF];
    __shared__ double wsh[VB / 64][NSO][K];
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
    // (gridDim.x * VB and VB are multiples of K2: this thread's pieces all belong to columns c0, c0 + 1)
    const int c0 = 2 * ((int)threadIdx.x % K2);
    const bool r0 = ALL || L.stop[c0] == ST_RUNNING, r1 = ALL || L.stop[c0 + 1] == ST_RUNNING;
    op.prep(L, c0);
    m2d acc[NSO];
#pragma unroll
    for (int s = 0; s < NSO; s++) acc[s] = (m2d)(0.0);
    if (r0 || r1) {
        const long stride = (long)gridDim.x * VB;
        for (long e = (long)blockIdx.x * VB + threadIdx.x; e < n2; e += stride) op.apply(e, e / K2, r0, r1, acc);
    }
    if (Op::NS > 0) {
        // lanes l, l + K2, l + 2 K2, ... of a wavefront hold the same two columns: xor-butterfly over them, then the wavefronts in order
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
        for (int s = 0; s < NSO; s++) {
            double x = acc[s].x, y = acc[s].y;
            if (TREE & 1) {
#pragma unroll
                for (int off = K2; off <= 32; off <<= 1) { x += __shfl_xor(x, off, 64); y += __shfl_xor(y, off, 64); }
            } else {
#pragma unroll
                for (int off = 32; off >= K2; off >>= 1) { x += __shfl_xor(x, off, 64); y += __shfl_xor(y, off, 64); }
            }
            if (lane < K2) { wsh[w][s][2 * lane] = x; wsh[w][s][2 * lane + 1] = y; }
        }
        __syncthreads();
        if (threadIdx.x < NSO * K) {
            const int s = threadIdx.x / K, j = threadIdx.x % K;
            double v = 0.0;
            static_assert(VB / 64 == 4, "the tree over the wavefronts");
            if (TREE & 1) v = (wsh[0][s][j] + wsh[1][s][j]) + (wsh[2][s][j] + wsh[3][s][j]);
            else {
#pragma unroll
                for (int q = 0; q < VB / 64; q++) v += wsh[q][s][j];
            }
            pout[(s * K + j) * MM_MG + blockIdx.x] = v;
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

} // namespace lcgh
