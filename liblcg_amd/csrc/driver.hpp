// driver.hpp -- host side of a device-resident Krylov loop.
//
// The host only enqueues: every coefficient lives in DevState, the stop test runs in the
// scalar kernels, and once it fires the remaining enqueued kernels fall through.  Without a
// progress callback the host therefore never blocks on the stream; it watches the
// host-mapped HostStatus to (a) stop enqueuing soon after convergence and (b) stay at most
// `inflight` iterations ahead.  With a progress callback the reference's contract (residual
// and live m handed over before every iteration, lcg.cpp:211-217) forces one stream
// synchronisation per iteration.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <cstring>
#include <thread>
#include <typeinfo>
#include <vector>

#include "devcommon.hpp"

namespace lcgh {

#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
inline uintptr_t al(const void *p) { return (uintptr_t)p; }
double global_rows_of(Ctx &c, int n, const void *afp, const void *inst);   // comm.hip: n summed over ranks (n itself when single)

// One k_vec pass over n elements; returns its grid.  Complex vectors are naturally 16-byte elements; reals use the 2-wide path
// when every pointer is 16-byte aligned (align_or: the pointers OR-ed together).
template <class Op> int launch_vec(const Op &op, long n, bool cplx, uintptr_t align_or, double *partials, hipStream_t s)
{
    const bool v2 = !cplx && (align_or & 15) == 0;
    const int g = grid_for(v2 ? (n + 1) / 2 : n);
    if (v2) hipLaunchKernelGGL((k_vec<Op, true>), dim3(g), dim3(VB), 0, s, op, n, partials);
    else hipLaunchKernelGGL((k_vec<Op, false>), dim3(g), dim3(VB), 0, s, op, n, partials);
    return g;
}

struct Driver {
    Ctx &c;
    long n;            // local vector length (reals: elements, complex: complex elements)
    bool cplx;
    int max_it, abs_diff;
    double eps;
    int enq = 0;       // iteration bodies enqueued
    // a callback of the caller's own (not the built-in product / Jacobi) is in the loop: such a callback cannot honour the stop
    // flag, so nothing is enqueued ahead of a verdict the reference would have returned on first (lcg.cpp:186-203)
    bool user_cb = false;

    Driver(Ctx &c_, long n_, bool cplx_, int max_it_, double eps_, int abs_diff_)
        : c(c_), n(n_), cplx(cplx_), max_it(max_it_), abs_diff(abs_diff_), eps(eps_) {}
    ~Driver() { c.in_solve = false; }
    Driver(const Driver &) = delete;

    // ---- launches ------------------------------------------------------------------------
    template <class Op> int vec(Op op, uintptr_t align_or = 0) { return vec_n(op, n, align_or); }
    // a reducing pass whose sums land in table rows row0, row0 + 1, ... beside the rows an earlier pass of the same body left
    // there (same grid: the per-row counts stay as they are)
    template <class Op> int vec_rows(Op op, int row0, uintptr_t align_or)
    {
        const PartCount keep = pcnt;
        double *table = c.partials;
        c.partials = table + (size_t)row0 * MAXG;
        int rc = vec_n(op, n, align_or);
        c.partials = table;
        const int g = pcnt.g[0];
        pcnt = keep;
        for (int r = 0; r < Op::NR; r++) pcnt.g[row0 + r] = g;
        return rc;
    }
    // same pass over a vector of another length (e.g. the per-block partials of a fused A.x)
    template <class Op> int vec_n(Op op, long n, uintptr_t align_or)
    {
        c.cnt_vec++;
        op.st = c.state;        // the state of THIS launch (vecf below moves it between the buffers of a pair)
        const int g = launch_vec(op, n, cplx, align_or, c.partials, c.stream);
        if (Op::NR > 0) pcnt.all(g);
        HIPCHK(hipGetLastError());
        return dbg(typeid(Op).name());
    }
    // Scalar step `fin` (on the sums of the latest reducing pass) fused into the pass `op` that consumes its result:
    // one launch instead of k_scal + k_vec (devcommon.hpp: k_vecf).  One GPU; when the rows are sharded the
    // sums have to meet the other ranks' first, so the step stays its own kernel(s) around the all-reduce.
    template <class Fin, class Op> int vecf(Fin fin, Op op, uintptr_t align_or = 0)
    {
        if (comm_active()) {
            int rc = scal(fin);
            return rc ? rc : vec(op, align_or);
        }
        c.cnt_vec++;        // (the scalar step rides in this pass: no launch of its own)
        const bool v2 = !cplx && (align_or & 15) == 0;      // complex passes take one 16-byte element per lane (vec_n)
        const int g = grid_for(v2 ? (n + 1) / 2 : n);
        DevState *cur = c.state, *next = c.state == c.state_pair[0] ? c.state_pair[1] : c.state_pair[0];
        double *pin = c.partials, *pout = c.partials == c.partials_pair[0] ? c.partials_pair[1] : c.partials_pair[0];
        if (v2) hipLaunchKernelGGL((k_vecf<Fin, Op, true>), dim3(g), dim3(VB), 0, c.stream, fin, op, n, pin, pcnt, pout, cur, next);
        else hipLaunchKernelGGL((k_vecf<Fin, Op, false>), dim3(g), dim3(VB), 0, c.stream, fin, op, n, pin, pcnt, pout, cur, next);
        HIPCHK(hipGetLastError());
        c.state = next;
        if (Op::NR > 0) { c.partials = pout; pcnt.all(g); }
        return dbg(typeid(Op).name());
    }
    // partial sums waiting in c.partials, per running sum: the latest reducing pass sets all rows to its grid; an A.x that
    // carried a dot in its epilogue (csr_ax_dot) sets the rows it wrote
    PartCount pcnt = [] { PartCount p; p.all(1); return p; }();
    // A body whose closing scalar step rides in the NEXT body's first pass (vecf) leaves the last one open: `tail`
    // closes it, once, after the last body and before the state is read.
    std::function<int()> tail;
    int run_tail() { if (!tail) return 0; auto t = std::move(tail); tail = nullptr; return t(); }
    // LCG_HIP_DEBUG=2: synchronise after every launch and name it on stderr (fault isolation)
    bool debug_sync = debug_level() >= 2;
    int dbg(const char *what)
    {
        if (!debug_sync) return 0;
        std::fprintf(stderr, "[lcg_hip] %s ...", what); std::fflush(stderr);
        HIPCHK(hipStreamSynchronize(c.stream));
        std::fprintf(stderr, " ok\n");
        return 0;
    }

    // scalar step after the most recent reducing vec()
    // The sharded loop's host decides from the state as of the LAST body of a batch (run_lockstep).  With sharded rows only the
    // scalar steps change DevState, so every step of that body leaves the state it produced in `snap_to` (host-mapped; the body's
    // last step wins, in stream order): no device-to-host copy and none of its two boundaries on the stream.
    DevState *snap_to = nullptr;
    int snap_taken = 0;
    template <class Fin> int scal(Fin fin)
    {
        const PartCount g = pcnt;
        XgBox xb;
        c.cnt_scal++;
        if (comm_active() && Fin::NR > 0) c.cnt_allreduce++;       // (RCCL all-reduce between two launches, or the mailboxes inside one)
        if (snap_to) snap_taken++;
        if (comm_active() && Fin::NR > 0 && xg_box(&xb)) {
            // reduce + exchange over the peer mailboxes + scalar step in one launch
            hipLaunchKernelGGL((k_scal<Fin>), dim3(1), dim3(VB), 0, c.stream, fin, c.partials, g, c.state, SC_XGMI, xb, snap_to);
        } else if (comm_active() && Fin::NR > 0) {
            hipLaunchKernelGGL((k_scal<Fin>), dim3(1), dim3(VB), 0, c.stream, fin, c.partials, g, c.state, SC_REDUCE, xb, (DevState *)nullptr);
            int rc = comm_allreduce(c.state->red, Fin::NR, c.stream);
            if (rc) return rc;
            hipLaunchKernelGGL((k_scal<Fin>), dim3(1), dim3(VB), 0, c.stream, fin, c.partials, g, c.state, SC_FIN, xb, snap_to);
        } else {
            hipLaunchKernelGGL((k_scal<Fin>), dim3(1), dim3(VB), 0, c.stream, fin, c.partials, g, c.state, SC_FUSED, xb, snap_to);
        }
        HIPCHK(hipGetLastError());
        return dbg(typeid(Fin).name());
    }

    // ---- state -------------------------------------------------------------------------------
    // the solve begins here (not in the constructor: placement's trial products come first, and must neither be counted nor
    // honour a stop flag): launch counters zeroed, the built-in callbacks told that a solve runs, DevState initialised
    int init_state(double n_global)
    {
        c.in_solve = true; c.ax_rc = 0; c.cnt_vec = c.cnt_scal = c.cnt_allreduce = c.cnt_ax = 0;
        DevState h;
        std::memset(&h, 0, sizeof h);
        h.eps = eps; h.abs_diff = abs_diff; h.n_global = n_global; h.host = c.hstat_dev;
        // the lock-step loop of a sharded run never looks at the mirror; the asynchronous loop paces
        // itself on it: every 4th body on small systems (3-5 us of a 20-35 us iteration at 1e4 rows),
        // every body where a body is long and only 6 are kept in flight
        h.pub_mask = comm_active() ? 0x3fffffff : ((cplx ? 2 * n : n) >= (1 << 20) ? 0 : 3);
        c.hstat->it = 0; c.hstat->done = 0; c.hstat->status = 0; c.hstat->t = 0; c.hstat->residual = 0.0;
        (void)lcg_hip_last_ax_mean_us();        // a previous solve's events, if nobody asked yet: they are about to be reused
        // from a pinned staging slot, in stream order in front of the solve's first kernel: no synchronisation here (the
        // previous solve ended with one, so the slot is free)
        *c.state_stage = h;
        HIPCHK(hipMemcpyAsync(c.state, c.state_stage, sizeof h, hipMemcpyHostToDevice, c.stream));
        // kernels that a sharded A.x puts on the second stream read the stop flag too, and the direct exchange starts them
        // without a fork event: they must not see the previous solve's flag
        HIPCHK(hipEventRecord(c.ev_a, c.stream));
        HIPCHK(hipStreamWaitEvent(c.comm_stream, c.ev_a, 0));
        return 0;
    }
    int read_state(DevState &h)
    {
        HIPCHK(hipMemcpyAsync(&h, c.state, sizeof h, hipMemcpyDeviceToHost, c.stream));
        HIPCHK(hipStreamSynchronize(c.stream));
        return 0;
    }

    // A.x callback with optional event timing.  liblcg's callback types return void (lcg.h:37-38), so the built-in
    // callbacks park their failure (a refused exchange, an RCCL error, a HIP error) in Ctx::ax_rc; it ends the
    // solve here with that LCG_HIP_E_* code instead of letting the loop run on over a stale product.
    template <class F> int timed_ax(F &&call)
    {
        c.cnt_ax++;
        if (c.profile && (c.ax_seq++ % c.profile_every) == 0 && c.prof_used + 2 <= (int)c.prof_ev.size()) {
            HIPCHK(hipEventRecord(c.prof_ev[c.prof_used], c.stream));
            call();
            HIPCHK(hipEventRecord(c.prof_ev[c.prof_used + 1], c.stream));
            c.prof_used += 2;
        } else {
            call();
        }
        return c.ax_rc;
    }
    // same for the preconditioner callback
    template <class F> int checked_mx(F &&call) { call(); return c.ax_rc; }

    // ---- the loop --------------------------------------------------------------------------
    // body(): enqueue one counted iteration.  pfp(residual, t): progress callback or nullptr
    // semantics via `has_pfp`.  Returns the liblcg status code.
    template <class Body, class Pfp>
    int run(Body &&body, bool has_pfp, Pfp &&pfp, int code_max_it, int code_nan)
    {
        DevState h;
        int rc = 0;
        if (has_pfp || user_cb) {
            rc = read_state(h);
            if (rc) return rc;
            if (h.status == ST_ALREADY) {                   // lcg.cpp:186-203
                if (has_pfp) pfp(h.residual, 0);
                finish(h);
                return LCG_ALREADY_OPTIMIZIED;
            }
        }
        // (without a progress callback and with the built-in callbacks nobody needs the setup's verdict yet: "already optimised" has
        //  set the stop flag, the bodies enqueued below fall through -- the built-in products honour the flag --, and the verdict is
        //  read with the final state: one stream drain less per solve.  A user's A.x / M callback would be CALLED for every body
        //  enqueued ahead, which the reference never does after this verdict: there the verdict is read first.)
        if (has_pfp) {
            for (;;) {                                      // lcg.cpp:206-230, one sync per iteration
                if (pfp(h.residual, h.t)) { finish(h); return LCG_STOP; }
                if (h.residual <= eps) { finish(h); return LCG_CONVERGENCE; }
                if (max_it > 0 && h.t + 1 > max_it) { finish(h); return code_max_it; }
                rc = body(); if (rc) return rc;
                enq++;
                rc = read_state(h); if (rc) return rc;
                if (h.status == ST_COMM) return comm_lost(h);
                if (h.status == ST_NAN) { finish(h); return code_nan; }
            }
        }
        if (comm_active()) return run_lockstep(body, code_max_it, code_nan);
        // asynchronous path
        const long work = cplx ? 2 * n : n;
        const int inflight = work >= (1 << 20) ? 6 : 24;
        // (Replaying the body from a hipGraph was measured and dropped: on the launch-bound 1e4-row
        // system an iteration is six DEPENDENT ~2 us kernels, 23 us eager vs 24.6 us replayed in
        // batches of four -- the chain on the device is the limit, not the host's launch rate.)
        for (;;) {
            if (max_it > 0 && enq >= max_it) break;
            rc = body(); if (rc) return rc;
            enq++;
            if (c.hstat->done) break;
            // stay at most `inflight` bodies ahead of the device
            int spins = 0;
            while (c.hstat->it < enq - inflight && !c.hstat->done) {
                if (++spins > 2000) { std::this_thread::sleep_for(std::chrono::microseconds(20)); }
                if (spins > 200000) {   // backstop: the mapped mirror is not advancing
                    rc = read_state(h); if (rc) return rc;
                    if (h.done || h.it >= enq - inflight) break;
                    spins = 0;
                }
            }
            if ((enq & 255) == 0) {     // authoritative check now and then
                rc = read_state(h); if (rc) return rc;
                if (h.done) break;
            }
        }
        rc = run_tail(); if (rc) return rc;
        rc = read_state(h); if (rc) return rc;
        if (h.status == ST_COMM) return comm_lost(h);
        finish(h);
        if (h.status == ST_ALREADY) return LCG_ALREADY_OPTIMIZIED;
        if (h.status == ST_NAN) return code_nan;
        if (h.done && h.status == ST_CONVERGED) return LCG_CONVERGENCE;
        return code_max_it;
    }

    // Sharded rows: every body holds collectives, so every rank must enqueue the SAME number of
    // bodies -- a rank that stopped on its own view of the mapped stop flag would leave its peers
    // waiting in an all-reduce.  Bodies therefore go out in batches; behind each batch the stream
    // copies DevState into a pinned slot, and the decision to go on after batch k+1 is taken from
    // the slot of batch k.  That slot holds the state as of one fixed body, computed from
    // all-reduced sums only, so it is bit-identical on all ranks and so is the decision; and the
    // stream always holds one whole batch while the host waits (no drain).
    template <class Body>
    int run_lockstep(Body &&body, int code_max_it, int code_nan)
    {
        constexpr int batch = 8;
        int nb = 0, rc = 0;
        DevState h;
        for (;;) {
            int todo = batch;
            if (max_it > 0) todo = std::min(batch, max_it - enq);
            if (todo <= 0) break;
            const int slot = nb & 1;
            for (int i = 0; i < todo; i++) {
                if (i == todo - 1) { snap_to = c.snap_dev[slot]; snap_taken = 0; }
                rc = body();
                if (rc) { snap_to = nullptr; return rc; }
                enq++;
            }
            snap_to = nullptr;
            // (a body without a scalar step of its own -- none of the built-in loops -- is copied the old way)
            if (!snap_taken) HIPCHK(hipMemcpyAsync(c.snap[slot], c.state, sizeof(DevState), hipMemcpyDeviceToHost, c.stream));
            HIPCHK(hipEventRecord(c.snap_ev[slot], c.stream));
            nb++;
            if (nb >= 2) {
                const int prev = (nb - 2) & 1;
                HIPCHK(hipEventSynchronize(c.snap_ev[prev]));
                if (c.snap[prev]->done) break;
            }
        }
        // the verdict: the snapshot behind the last batch (bodies enqueued after a stop fall through: counts, residual and status
        // are those of the stop) -- the stream is drained by waiting for that batch's event, nothing is copied
        if (nb > 0) {
            HIPCHK(hipEventSynchronize(c.snap_ev[(nb - 1) & 1]));
            HIPCHK(hipStreamSynchronize(c.stream));
            std::memcpy(&h, c.snap[(nb - 1) & 1], sizeof h);
        } else {
            rc = read_state(h); if (rc) return rc;
        }
        if (h.status == ST_COMM) return comm_lost(h);
        finish(h);
        if (h.status == ST_ALREADY) return LCG_ALREADY_OPTIMIZIED;
        if (h.status == ST_NAN) return code_nan;
        if (h.done && h.status == ST_CONVERGED) return LCG_CONVERGENCE;
        return code_max_it;
    }

    // a peer's sums did not arrive in the direct all-reduce (devcommon.hpp: xg_allreduce)
    int comm_lost(const DevState &h)
    {
        finish(h);
        c.err = "direct all-reduce: a peer's contribution did not arrive in time";
        return LCG_HIP_E_COMM;
    }

    void finish(const DevState &h)
    {
        c.last_iters = h.t;
        c.last_residual = h.residual;
        c.last_ax_calls = c.prof_used / 2;
        c.last_ax_mean_us = 0.0;
        c.prof_pending = c.profile ? c.prof_used : 0;   // turned into a mean when somebody asks (lcg_hip_last_ax_mean_us)
        c.prof_used = 0;
    }
};

// copy-in / copy-out of caller vectors when mem == HOST
struct HostBridge {
    double *dm = nullptr, *dB = nullptr;
    double *hm = nullptr;
    size_t bytes = 0;
    bool active = false;
    int open(int mem, double *&m, const double *&B, size_t nbytes, hipStream_t s)
    {
        if (mem == LCG_HIP_MEM_DEVICE) return 0;
        active = true; bytes = nbytes; hm = m;
        HIPCHK(hipMalloc(&dm, nbytes));
        HIPCHK(hipMalloc(&dB, nbytes));
        HIPCHK(hipMemcpyAsync(dm, m, nbytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dB, B, nbytes, hipMemcpyHostToDevice, s));
        m = dm; B = dB;
        return 0;
    }
    int close(hipStream_t s)
    {
        if (!active) return 0;
        hipError_t e = hipMemcpyAsync(hm, dm, bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        hipFree(dm); hipFree(dB);
        active = false;
        if (e != hipSuccess) return fail(e, "copy back m", __FILE__, __LINE__);
        return 0;
    }
    ~HostBridge() { if (active) { hipFree(dm); hipFree(dB); } }
};

// device scratch vectors of one solve: what it holds of the pool (pool.hpp), idle again on scope exit; caller-provided pointers win
struct Workspace {
    std::vector<double *> held;
    int get(double *&out, double *given, size_t bytes)
    {
        if (given) { out = given; return 0; }
        TRY(ctx().pool.take(bytes, out));
        held.push_back(out);
        return 0;
    }
    bool owns(const double *p) const { for (double *h : held) if (h == p) return true; return false; }
    // an idle vector of the pool joins this solve (placement.hip: it becomes a product's output)
    void adopt(double *p) { ctx().pool.set_busy(p, true); held.push_back(p); }
    ~Workspace() { for (double *p : held) ctx().pool.set_busy(p, false); }
};

// placement.hip, where the work vectors lie: the solve's own vectors are classed by the time of y = A.x into each and dealt
// to `roles` by weight -- the products' outputs (n_out of them) first, then the vector the most frequent product reads, then the rest.
// x: any n-vector that holds finite numbers (the right-hand side).  Always 0: a timing that fails means "not tried".
int place_roles(Ctx &c, int n, const void *afp, void *inst, const double *x, Workspace &ws, std::initializer_list<double **> roles, int n_out);

// ---- one solve: the plumbing around a solver's loop (real and complex differ in callback types and NaN code) --------------------
template <bool CPLX> struct SolveTypes;
template <> struct SolveTypes<false> {
    using Para = lcg_para; using Ax = lcg_axfunc_ptr; using Progress = lcg_progress_ptr;
    static constexpr Ax csr_ax = lcg_hip_csr_ax;
    static constexpr int NAN_CODE = LCG_NAN_VALUE;
};
template <> struct SolveTypes<true> {
    using Para = clcg_para; using Ax = clcg_hip_axfunc_ptr; using Progress = clcg_hip_progress_ptr;
    static constexpr Ax csr_ax = clcg_hip_csr_ax;
    static constexpr int NAN_CODE = CLCG_NAN_VALUE;
};

// A solver's setup, after its own argument checks and ensure_init(), in this order: open() (m and B onto the device when they live
// in host memory), get() (the work vectors -- the ORDER of the calls decides which pool vector a role receives), place() (real,
// optional: before start(), whose counters its trial products must not bump), start(); the loop's return code goes through
// finish(rc).  Destruction runs in reverse: the Driver, the Workspace (its vectors back to the pool), the HostBridge.
template <bool CPLX>
struct Solve {
    using T = SolveTypes<CPLX>;
    Ctx &c;
    HostBridge hb;
    Workspace ws;
    Driver drv;
    typename T::Para para; void *inst; typename T::Ax Afp; typename T::Progress Pfp;
    int n;
    size_t nb;              // bytes of one vector
    double *m = nullptr;    // the solution vector on the device (set by open)
    Solve(const typename T::Para &p, int n_, void *inst_, typename T::Ax A, typename T::Progress P)
        : c(ctx()), drv(c, n_, CPLX, p.max_iterations, p.epsilon, p.abs_diff), para(p), inst(inst_), Afp(A), Pfp(P), n(n_),
          nb(sizeof(double) * (CPLX ? 2 : 1) * (size_t)n_)
    { drv.user_cb = A != T::csr_ax; }

    int open(int mem, double *&m_, const double *&B) { TRY(hb.open(mem, m_, B, nb, c.stream)); m = m_; return 0; }
    int get(double *&out, double *given = nullptr) { return ws.get(out, given, nb); }
    int place(const double *x, std::initializer_list<double **> roles, int n_out) { return place_roles(c, n, (const void *)Afp, inst, x, ws, roles, n_out); }
    int start() { return drv.init_state(global_rows_of(c, n, (const void *)Afp, inst)); }
    // a runtime failure of the loop (LCG_HIP_E_*) wins over one of the copy-back; that one over the loop's verdict
    int finish(int rc) { const int rc2 = hb.close(c.stream); return rc <= -2000 ? rc : (rc2 ? rc2 : rc); }

    int axop(const double *x, double *y, int layout, int conj) { return drv.timed_ax([&] { Afp(inst, x, y, n, layout, conj); }); }
    int ax(const double *x, double *y)
    {
        if constexpr (CPLX) return axop(x, y, 0, 0);
        else return drv.timed_ax([&] { Afp(inst, x, y, n); });
    }
    int run_loop(const std::function<int()> &body)
    {
        auto pfp = [&](double resid, int t) -> int { return Pfp(inst, m, resid, &para, n, t); };
        // (the complex loops hand back the REAL enum's iteration-cap code, clcg.cpp:126,164 ...)
        return drv.run(body, Pfp != nullptr, pfp, LCG_REACHED_MAX_ITERATIONS, T::NAN_CODE);
    }
};

// the built-in Jacobi on a handle that owns its reciprocal diagonal: M^-1 folds into the update pass (its diagonal; else nullptr)
inline const double *builtin_invdiag(const void *Mfp, void *inst, int n, bool cplx)
{
    if (Mfp != (cplx ? (const void *)clcg_hip_jacobi_mx : (const void *)lcg_hip_jacobi_mx) || !inst) return nullptr;
    const lcg_hip_csr *A = static_cast<const lcg_hip_csr *>(inst);
    return A->is_complex == cplx && A->n_rows == n ? A->invdiag : nullptr;
}

} // namespace lcgh
