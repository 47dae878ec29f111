"""Helpers of tests/test_gpu_streams.py and tests/test_gpu_streams_kwide.py: the late-input pattern that shows on WHICH stream the library's work runs.

lcg_hip_set_stream() puts the library on a caller's stream.  The library's own stream is a blocking one, so everything the rest
of the suite does is ordered against torch's default stream by the runtime; a torch side stream is non-blocking and has no such
protection.  The pattern: on the side stream S a long chain of filler kernels (the delay) runs, behind it torch copies write the
real inputs into buffers that hold NaN until then, and the library is entered while the delay is still running.  Work that the
library puts on S waits for the inputs and computes the bits of a run on the own stream with the inputs ready; work that lands
anywhere else (the own stream, the null stream, a forked stream that was not joined) reads NaN or an unfinished intermediate,
and the clones taken on S differ from the reference run.  Every comparison is an identity.

Two streams that share a hardware queue are serialised in submission order, and work mis-streamed onto such a stream would see
finished inputs: `pick_stream` therefore accepts a side stream only after both controls (the product deliberately left on the own
stream, and a kernel on the null stream) came out NaN under the same pattern.  The controls only READ a buffer that is written
later.
"""
import ctypes as C
import math

import numpy as np

NAN = float("nan")
TARGET_MS = 100.0           # the delay lasts at least this long: four to five orders of magnitude above a launch (a choice)
MARGIN = 1.5                # the chain is made this much longer than the timed op asks for (clock ramps, a faster second pass)
SCRATCH_BYTES = 256 << 20   # the filler's tensor, at most
COUNT_CAP = 8192            # hard cap of the chain's length
CANDIDATES = 8
PREMISE = ("the delay had already finished when the library was entered: the premise of the late-input pattern did not hold "
           "(this is a failure of the test's set-up, not a pass)")


def nan_fill(t):
    """NaN into a floating or complex tensor; an integer one (row pointers, columns) gets zeros -- an empty pattern: read too
    early it gives a wrong result, never an index out of range."""
    if t.dtype.is_complex:
        t.fill_(complex(NAN, NAN))
    elif t.dtype.is_floating_point:
        t.fill_(NAN)
    else:
        t.zero_()


class Delay:
    """A chain of in-place torch ops on one large tensor, calibrated once: the time of one op by events, the count from it."""
    def __init__(self, torch):
        self.torch = torch
        self.buf = torch.ones(SCRATCH_BYTES // 8, dtype=torch.float64, device="cuda")
        for _ in range(5):
            self.buf.mul_(1.0)
        torch.cuda.synchronize()
        reps = 20
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            self.buf.mul_(1.0)
        t1.record(); t1.synchronize()
        self.op_ms = t0.elapsed_time(t1) / reps
        self.count = min(COUNT_CAP, int(math.ceil(MARGIN * TARGET_MS / self.op_ms)))
        assert self.count * self.op_ms >= TARGET_MS, (self.op_ms, self.count, "the capped chain is shorter than the target")
        print(f"stream tests: one filler op over {SCRATCH_BYTES >> 20} MB takes {self.op_ms:.4f} ms; chain of {self.count} ops "
              f"= {self.count * self.op_ms:.0f} ms (target {TARGET_MS:.0f} ms)")

    def enqueue(self):
        """The chain on torch's current stream, and an event behind it."""
        for _ in range(self.count):
            self.buf.mul_(1.0)
        e = self.torch.cuda.Event()
        e.record()
        return e


class Env:
    """torch, api, lib, the calibrated delay and the accepted side stream (None until pick_stream)."""
    def __init__(self, torch, api, lib):
        self.torch, self.api, self.lib = torch, api, lib
        self.delay = Delay(torch)
        self.S = None
        self.kept = []          # candidates, kept alive so that the queues keep rotating
        self.accepted = None    # index of the accepted candidate
        self.why_not = []
        self.rows = None        # the control matrix's non-empty rows (an empty row's y is 0 whatever x holds)

    def set_stream_handle(self, handle):
        rc = self.lib.lcg_hip_set_stream(C.c_void_p(handle))
        assert rc == 0, (rc, self.lib.lcg_hip_last_error())

    # ------------------------------------------------------------------------------------------------------------ control
    def control(self, S, where, A, x_real, x, y):
        """While S runs the delay and writes x late: lcg_hip_spmv left on the library's own stream (`where` = "own"), or a kernel on
        the null stream ("null": a torch op on torch's default stream, which is the null stream -- lcg_hip_set_stream cannot put
        the library there, NULL is its name for the own stream).  Returns True when y came out NaN in every row: work on that
        stream is NOT ordered behind S, so the pattern sees it."""
        torch, api = self.torch, self.api
        nan_fill(x); y.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            E = self.delay.enqueue()
            x.copy_(x_real, non_blocking=True)
        assert not E.query(), PREMISE
        if where == "own":
            assert self.lib.lcg_hip_get_stream() != S.cuda_stream
            A.spmv(x, y)
        else:
            assert torch.cuda.current_stream().cuda_stream == 0
            torch.mul(x, 1.0, out=y)
        S.synchronize()
        api.synchronize()
        torch.cuda.synchronize()
        return self.all_nan(y) if where == "own" else bool(torch.isnan(y).all().item())

    def all_nan(self, y):
        """Every non-empty row of the control product read NaN."""
        return bool(self.torch.isnan(y[self.rows]).all().item())

    def pick_stream(self, A, x_real):
        """Up to CANDIDATES fresh streams; the first for which both controls show NaN."""
        torch = self.torch
        x, y = torch.empty_like(x_real), torch.empty_like(x_real)
        for i in range(CANDIDATES):
            S = torch.cuda.Stream()
            self.kept.append(S)
            own = self.control(S, "own", A, x_real, x, y)
            null = own and self.control(S, "null", A, x_real, x, y)
            print(f"stream tests: candidate {i}: product on the own stream saw {'NaN' if own else 'finished inputs'}"
                  + (f", a kernel on the null stream {'NaN' if null else 'finished inputs'}" if own else ""))
            if own and null:
                self.S, self.accepted = S, i
                return
            self.why_not.append((i, own, null))

    def need_stream(self):
        assert self.S is not None, ("no side stream qualified: for each of the candidates a product left on the own or the null stream "
                                    f"saw finished inputs (shared hardware queue), so the ordering tests would be blind: {self.why_not}")
        return self.S

    # ------------------------------------------------------------------------------------------------------------ pattern
    def reference(self, inputs, call, outputs):
        """Run (a): inputs ready, the library on its own stream.  Returns (what call returned, the outputs' bytes, numpy copies)."""
        torch, api = self.torch, self.api
        ins = {d.data_ptr() for d, _ in inputs}
        for o in outputs:
            if o.data_ptr() not in ins:
                nan_fill(o)
        for d, s in inputs:
            d.copy_(s)
        torch.cuda.synchronize()
        r = call()
        api.synchronize()
        torch.cuda.synchronize()
        outs = [o.cpu().numpy().copy() for o in outputs]
        return r, outs

    def late(self, inputs, call, outputs, enqueue_only, S=None, on_default=False):
        """Run (b): the delay, then the late writes, then the library, then clones -- all on S (on_default: on torch's default
        stream with the library on its own; no synchronisation in between).  Returns (what call returned, numpy copies of the clones)."""
        torch, api = self.torch, self.api
        S = S or (torch.cuda.default_stream() if on_default else self.need_stream())
        ins = {d.data_ptr() for d, _ in inputs}
        for d, _ in inputs:
            nan_fill(d)
        for o in outputs:
            if o.data_ptr() not in ins:
                nan_fill(o)
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(S):
                if not on_default:
                    api.use_torch_stream()
                E = self.delay.enqueue()
                for d, s in inputs:
                    d.copy_(s, non_blocking=True)
                assert not E.query(), PREMISE
                r = call()
                if enqueue_only:
                    assert not E.query(), "the call drained the stream (the delay had finished when it returned): it is documented to only enqueue"
                clones = [o.clone() for o in outputs]
                S.synchronize()
            outs = [c.cpu().numpy().copy() for c in clones]
        finally:
            api.use_own_stream()
        torch.cuda.synchronize()
        return r, outs

    def pair(self, inputs, call, outputs, enqueue_only, tag=(), anchor=None, on_default=False, between=None):
        """(a) then (b); anchor(r, outs) holds run (a) to the exact reference first, so that the identity never compares two wrong
        answers.  between() runs on the own stream after the anchor: where run (a) leaves the right intermediate in scratch that the
        handle owns, it overwrites that scratch, so that a launch of run (b) that reads it too early cannot find run (a)'s.
        Returns run (a)."""
        ra, oa = self.reference(inputs, call, outputs)
        if anchor is not None:
            anchor(ra, oa)
        if between is not None:
            between()
            self.api.synchronize()
            self.torch.cuda.synchronize()
        rb, ob = self.late(inputs, call, outputs, enqueue_only, on_default=on_default)
        assert same_scalars(ra, rb), (tag, "returned values", ra, rb)
        for i, (a, b) in enumerate(zip(oa, ob)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (tag, "output", i, "differs from the run on the own stream",
                                                                       int(np.isnan(b.view(np.float32 if b.dtype == np.complex64 else np.float64)).sum()), "NaN words")
        return ra, oa


def make_env(torch, api, lib):
    """The calibrated delay, the control system and the side stream the controls accepted (Env.pick_stream): what the `env` fixture
    of either stream module wraps.  close_env() when the module is done."""
    from test_gpu_exact_products import data
    from test_gpu_kernels import _ragged
    e = Env(torch, api, lib)
    rng = np.random.default_rng(1)
    rp, col = _ragged(rng, 3001, 3001, 30)
    val, x = data(rng, rp, 3001, False, True)
    A = api.CsrMatrix.from_csr(rp, col, val)
    xs = torch.from_numpy(np.ascontiguousarray(x)).cuda(); y = torch.empty_like(xs)
    A.spmv(xs, y); api.synchronize()            # (the first product builds the handle's plan: not inside the control)
    e.control_system = (A, xs, rp, col, val, x)
    e.rows = torch.from_numpy(np.flatnonzero(np.diff(rp) > 0)).cuda()
    e.pick_stream(A, xs)
    print(f"stream tests: accepted candidate {e.accepted}")
    return e


def close_env(e):
    e.api.use_own_stream()
    e.control_system[0].destroy()


def pick_second(env):
    """A second side stream that does not queue behind the first: a product on it (the library switched to it) while the FIRST runs
    the delay and writes x late sees NaN -- otherwise the switch tests would be blind to a missing wait."""
    torch, api = env.torch, env.api
    S1 = env.need_stream()
    A, xs, *_ = env.control_system
    x, y = torch.empty_like(xs), torch.empty_like(xs)
    for i in range(CANDIDATES):
        S2 = torch.cuda.Stream()
        env.kept.append(S2)
        nan_fill(x); y.zero_()
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(S1):
                E = env.delay.enqueue()
                x.copy_(xs, non_blocking=True)
                assert not E.query(), PREMISE
            with torch.cuda.stream(S2):
                api.use_torch_stream()          # (from the idle own stream: nothing to wait for)
                A.spmv(x, y)
                S2.synchronize()
            S1.synchronize()
        finally:
            api.use_own_stream()
        torch.cuda.synchronize()
        seen = env.all_nan(y)
        print(f"stream tests: second stream, candidate {i}: {'independent of the first' if seen else 'queued behind the first'}")
        if seen:
            return S2
    raise AssertionError("no second stream runs beside the first: the switch tests would be blind")


def same_scalars(a, b):
    """Returned scalars bit for bit (floats by their bytes: NaN equals the same NaN)."""
    def flat(v):
        if v is None:
            return ()
        if isinstance(v, (list, tuple)):
            return tuple(x for e in v for x in flat(e))
        if isinstance(v, (float, complex, np.floating, np.complexfloating)):
            return (np.asarray(v).tobytes(),)
        if isinstance(v, np.ndarray):
            return (v.dtype.str, v.tobytes())
        return (v,)
    return flat(a) == flat(b)


def no_nan(outs, tag=()):
    for i, o in enumerate(outs):
        w = o.view(np.float32 if o.dtype == np.complex64 else np.float64) if o.dtype.kind in "fc" else o
        assert not np.isnan(w).any(), (tag, "output", i, "holds NaN")


# -------------------------------------------------------------------------------------------------------- the solver loops
class LateBuffers:
    """Stands in for test_gpu_stop_contract.guarded while Bench.solve runs: hands out buffers made BEFORE the delay (m first, then
    b, the order Bench.solve asks in), so that Bench.solve itself allocates and uploads nothing on the side stream."""
    def __init__(self, pairs):
        self.pairs = list(pairs)

    def __call__(self, values):
        buf, view = self.pairs.pop(0)
        assert view.numel() == len(values)
        return buf, view


def bench_solve(env, T, B, late, on_default=False, **kw):
    """One Bench.solve (tests/test_gpu_stop_contract.py, unchanged) -- late: under the late-input pattern, with m, b and a box
    loop's bounds written behind the delay.  kw: cap, on_progress, afp."""
    torch, api = env.torch, env.api
    n = B.n
    b_in = np.ascontiguousarray(B.rhs)
    mbuf, m = T.guarded(np.zeros(n, B.dtype))
    bbuf, b = T.guarded(b_in)
    stage = [(m, m.clone()), (b, b.clone())]
    if B.L.entry == "box":
        stage += [(B.low, B.low.clone()), (B.hig, B.hig.clone())]
    ws = B.workspaces()
    torch.cuda.synchronize()
    real = T.guarded
    T.guarded = LateBuffers([(mbuf, m), (bbuf, b)])
    try:
        if not late:
            r = B.solve(ws=ws, **kw)
            api.synchronize()
            return r
        S = torch.cuda.default_stream() if on_default else env.need_stream()
        for d, _ in stage:
            nan_fill(d)
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(S):
                if not on_default:
                    api.use_torch_stream()
                E = env.delay.enqueue()
                for d, s in stage:
                    d.copy_(s, non_blocking=True)
                assert not E.query(), PREMISE
                r = B.solve(ws=ws, **kw)
                S.synchronize()
        finally:
            api.use_own_stream()
        return r
    finally:
        T.guarded = real
        torch.cuda.synchronize()


def same_solve(a, b, tag=()):
    assert (a["ret"], a["iters"]) == (b["ret"], b["iters"]) and np.float64(a["residual"]).tobytes() == np.float64(b["residual"]).tobytes(), \
        (tag, "verdict", (a["ret"], a["iters"], a["residual"]), (b["ret"], b["iters"], b["residual"]))
    assert a["ks"] == b["ks"], (tag, "callback's ks", a["ks"], b["ks"])
    assert a["x"].dtype == b["x"].dtype and a["x"].tobytes() == b["x"].tobytes(), (tag, "iterate differs", int(np.isnan(b["x"].view(np.float32 if b["x"].dtype == np.complex64 else np.float64)).sum()), "NaN words")
    for i, (u, v) in enumerate(zip(a["ws"], b["ws"])):
        assert u.tobytes() == v.tobytes(), (tag, "workspace", i)


class DevPtr:
    """A device address as a tensor source (torch.as_tensor reads __cuda_array_interface__): what a caller's own Afp does with the
    pointers it is handed."""
    def __init__(self, ptr, n, typestr="<f8"):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 2}


# ------------------------------------------------------------------------------------------ which test runs which entry
# Every entry include/lcg_hip.h exports, and the stream test that runs it under the late-input pattern -- or why none does.
# tests/test_streams_cpu.py holds the table to the header (no entry missing, none left over) and each covered entry to its test:
#   "file::test"                  the test exists in tests/file, and the file's text names the entry;
#   ("file::test", text)          ... the file's text holds `text`, a call of the liblcg_amd.api method that wraps the entry;
#   ("file::test", text, helper)  ... the call is spelled in tests/helper, a module the test file uses: `text` is found there;
#   ("exempt", reason)            no stream test: getters, host-side switches, comm / p2p (they need peers), test hooks, lcg_hip_init.
OLD, NEW = "test_gpu_streams.py", "test_gpu_streams_kwide.py"
_CONTRACT, _LOOPS = "test_gpu_stop_contract.py", "stop_cases.py"
_GETTER = ("exempt", "a query answered on the host: enqueues nothing")
_SWITCH = ("exempt", "sets a host-side switch: enqueues nothing")
_HOOK = ("exempt", "a test or probe hook")
_PEERS = ("exempt", "comm / p2p: needs peers (multi-GPU paths on a caller's stream are not covered)")
_FREES = ("exempt", "frees device memory (after a device synchronise where something may be in flight): enqueues nothing")
_GENERATED = ("exempt", "builds a matrix or a vector from a seed: no input of the caller's that could be written late")
_SOLVERS = OLD + "::test_solver_loops"
_FACTOR = OLD + "::test_factor_built_and_applied_on_a_side_stream"
_CALLBACKS = NEW + "::test_ready_made_callbacks_called_directly"
_NEW_LOOPS = NEW + "::test_batched_loops_of_the_new_families"
_CREATED = NEW + "::test_csr_handles_made_from_device_memory_written_late"

STREAM_COVERAGE = {
    # runtime / stream
    "lcg_hip_init": ("exempt", "selects the device"),
    "lcg_hip_set_stream": OLD + "::test_get_stream_and_setting_the_current_stream_again",
    "lcg_hip_get_stream": OLD + "::test_get_stream_and_setting_the_current_stream_again",
    "lcg_hip_synchronize": OLD + "::test_back_to_the_own_stream_and_synchronize",
    "lcg_hip_memcpy": (_FACTOR, "A.ic0_factor_to_host"),
    "lcg_hip_last_error": _GETTER,
    "lcg_hip_default_parameters": _GETTER,
    "clcg_hip_default_parameters": _GETTER,
    "lcg_hip_last_iterations": _GETTER,
    "lcg_hip_last_residual": _GETTER,
    "lcg_hip_set_profiling": _SWITCH,
    "lcg_hip_last_ax_mean_us": _GETTER,
    "lcg_hip_last_ax_calls": _GETTER,
    "lcg_hip_last_launches": _GETTER,
    "lcg_hip_last_finisher_steps": _GETTER,
    "lcg_hip_trim": _FREES,
    "lcg_hip_set_cg_schedule": _SWITCH,
    "lcg_hip_set_placement": _SWITCH,
    "lcg_hip_last_placement": _GETTER,
    "lcg_hip_pool_info": _GETTER,
    "lcg_hip_pool_add_arena_for_test": _HOOK,
    "lcg_hip_placement_tune_for_test": _HOOK,
    "lcg_hip_last_placement_walk": _GETTER,
    # solver entries: every loop of stop_cases.LOOPS through Bench.solve
    "lcg_hip_solver": (_SOLVERS, "api.lcg_solver(", _CONTRACT),
    "lcg_hip_solver_preconditioned": (_SOLVERS, "api.lcg_solver_preconditioned(", _CONTRACT),
    "lcg_hip_solver_constrained": (_SOLVERS, "api.lcg_solver_constrained(", _CONTRACT),
    "lcg_hip_lcg": (_SOLVERS, "api.lcg(", _CONTRACT),
    "lcg_hip_lcgs": (_SOLVERS, "api.lcgs(", _CONTRACT),
    "clcg_hip_solver": (_SOLVERS, "api.clcg_solver(", _CONTRACT),
    "clcg_hip_solver_preconditioned": (_SOLVERS, "api.clcg_solver_preconditioned(", _CONTRACT),
    "clcg_hip_solver_c64": (_SOLVERS, "api.clcg_solver_c64(", _CONTRACT),
    "clcg_hip_solver_preconditioned_c64": (_SOLVERS, "api.clcg_solver_preconditioned_c64(", _CONTRACT),
    "lcg_hip_set_shadow_seed": ("exempt", "host-side state of the next complex solve"),
    "lcg_hip_set_shadow_vector": ("exempt", "host-side state of the next complex solve (the solve uploads it on its stream)"),
    # CSR matrices
    "lcg_hip_csr_create": _CREATED,
    "lcg_hip_csr_create_c64": _CREATED,
    "lcg_hip_csr_from_coo": _CREATED,
    "lcg_hip_csr_destroy": _FREES,
    "lcg_hip_csr_rows": _GETTER,
    "lcg_hip_csr_nnz": _GETTER,
    "lcg_hip_csr_arrays": _GETTER,
    "lcg_hip_csr_set_kernel": _SWITCH,
    "lcg_hip_csr_set_packed": NEW + "::test_symmetric_run_stretch_adopted_values_written_late",
    "lcg_hip_csr_packed_runs": _GETTER,
    "lcg_hip_csr_set_run_stretches": _SWITCH,
    "lcg_hip_csr_run_stretches": _GETTER,
    "lcg_hip_csr_set_sym_runs": _SWITCH,
    "lcg_hip_csr_set_sym_slices": _SWITCH,
    "lcg_hip_csr_sym_runs": _GETTER,
    "lcg_hip_csr_packed_templates": _GETTER,
    "lcg_hip_csr_set_binned": _SWITCH,
    "lcg_hip_csr_set_tiled": _SWITCH,
    "lcg_hip_csr_tiled_status": _GETTER,
    "lcg_hip_csr_set_ranges": _SWITCH,
    "lcg_hip_csr_ranges": _GETTER,
    "lcg_hip_csr_binned_status": _GETTER,
    "lcg_hip_csr_last_kernel": _GETTER,
    "lcg_hip_csr_last_traffic_model": _GETTER,
    "lcg_hip_csr_plan_info": _GETTER,
    "lcg_hip_csr_build_jacobi": OLD + "::test_jacobi",
    # ready-made callbacks
    "lcg_hip_csr_ax": OLD + "::test_host_vectors",
    "lcg_hip_jacobi_mx": OLD + "::test_jacobi",
    "clcg_hip_csr_ax": OLD + "::test_host_vectors",
    "clcg_hip_jacobi_mx": (_SOLVERS, "clcg_hip_jacobi_mx", _LOOPS),
    "clcg_hip_csr_ax_c64": OLD + "::test_host_vectors",
    "clcg_hip_jacobi_mx_c64": (_SOLVERS, "clcg_hip_jacobi_mx_c64", _LOOPS),
    # IC(0)
    "lcg_hip_csr_build_ic0": (_FACTOR, "A.build_ic0"),
    "lcg_hip_csr_build_ic0_c64": (_FACTOR, "A.build_ic0"),
    "lcg_hip_csr_ic0_info": _GETTER,
    "lcg_hip_csr_ic0_set_sweeps": ("exempt", "allocates or frees the two sweep vectors: enqueues nothing"),
    "lcg_hip_csr_ic0_get_sweeps": _GETTER,
    "lcg_hip_csr_ic0_factor": _GETTER,
    "lcg_hip_ic0_solve": (_FACTOR, "A.ic0_solve"),
    "lcg_hip_ic0_solve_c64": (_FACTOR, "A.ic0_solve"),
    "lcg_hip_ic0_mx": (_SOLVERS, "lcg_hip_ic0_mx", _LOOPS),
    "clcg_hip_ic0_mx": _CALLBACKS,
    "clcg_hip_ic0_mx_c64": _CALLBACKS,
    "lcg_hip_csr_ic0_schedule_for_test": _HOOK,
    # ILU(0)
    "lcg_hip_csr_build_ilu0": (_FACTOR, "A.build_ilu0"),
    "lcg_hip_csr_ilu0_info": _GETTER,
    "lcg_hip_csr_ilu0_set_sweeps": ("exempt", "allocates or frees the two sweep vectors: enqueues nothing"),
    "lcg_hip_csr_ilu0_get_sweeps": _GETTER,
    "lcg_hip_csr_ilu0_factor": _GETTER,
    "lcg_hip_ilu0_solve": (_FACTOR, "A.ilu0_solve"),
    "lcg_hip_ilu0_mx": (_SOLVERS, "lcg_hip_ilu0_mx", _LOOPS),
    "clcg_hip_ilu0_mx": _CALLBACKS,
    "lcg_hip_csr_ax_ilu0": (_SOLVERS, "lcg_hip_csr_ax_ilu0", _LOOPS),
    "clcg_hip_csr_ax_ilu0": _CALLBACKS,
    "lcg_hip_csr_ilu0_schedule_for_test": _HOOK,
    # dense operators
    "lcg_hip_dense_create": NEW + "::test_dense_handle_made_from_device_memory_written_late",
    "lcg_hip_dense_create_rows": ("exempt", "host rows only, staged and uploaded before it returns: no input that could be written late"),
    "lcg_hip_dense_destroy": _FREES,
    "lcg_hip_dense_rows": _GETTER,
    "lcg_hip_dense_cols": _GETTER,
    "lcg_hip_dense_matvec": OLD + "::test_dense_products",
    "clcg_hip_dense_matvec": NEW + "::test_complex_dense_block_products",
    "lcg_hip_dense_ata": OLD + "::test_dense_products",
    "lcg_hip_dense_ata_ax": (_SOLVERS, "lcg_hip_dense_ata_ax", _CONTRACT),
    "lcg_hip_dense_ax": _CALLBACKS,
    "clcg_hip_dense_ax": _CALLBACKS,
    "lcg_hip_dense_build_jacobi": NEW + "::test_dense_jacobi_built_on_a_side_stream",
    "lcg_hip_dense_jacobi_mx": NEW + "::test_dense_jacobi_built_on_a_side_stream",
    "clcg_hip_dense_jacobi_mx": _CALLBACKS,
    "lcg_hip_dense_last_kernel": _GETTER,
    "lcg_hip_dense_kernel_name": _GETTER,
    "lcg_hip_dense_set_kernel": _SWITCH,
    "lcg_hip_dense_matmat": NEW + "::test_real_dense_block_products",
    "lcg_hip_dense_ata_multi": NEW + "::test_real_dense_block_products",
    "lcg_hip_dense_op_multi_dot": NEW + "::test_real_dense_block_products",
    "lcg_hip_dense_multi_last_kernel": _GETTER,
    "lcg_hip_dense_multi_kernel_name": _GETTER,
    "lcg_hip_dense_lcg_multi": _NEW_LOOPS,
    "lcg_hip_dense_lpcg_multi": _NEW_LOOPS,
    "clcg_hip_dense_matmat": NEW + "::test_complex_dense_block_products",
    "clcg_hip_dense_op_multi_dot": NEW + "::test_complex_dense_block_products",
    "clcg_hip_dense_multi_kernel_name": _GETTER,
    "clcg_hip_dense_lbicg_sym_multi": _NEW_LOOPS,
    "clcg_hip_dense_lpcg_multi": _NEW_LOOPS,
    # kernels
    "lcg_hip_spmv": OLD + "::test_real_product_families",
    "lcg_hip_spmv_op": OLD + "::test_spmv_op_all_forms",
    "lcg_hip_spmv_dot": OLD + "::test_spmv_dot",
    "lcg_hip_spmm": OLD + "::test_real_block_products",
    "lcg_hip_spmm_dot": OLD + "::test_real_block_products",
    "lcg_hip_spmm_dot2": OLD + "::test_real_block_products",
    "lcg_hip_lcg_multi": OLD + "::test_batched_loops",
    "lcg_hip_lpcg_multi": OLD + "::test_batched_loops",
    "lcg_hip_ic0_solve_multi": OLD + "::test_batched_triangular_solves",
    "lcg_hip_ilu0_solve_multi": OLD + "::test_batched_triangular_solves",
    "lcg_hip_lpcg_multi_m": OLD + "::test_batched_loops",
    "lcg_hip_lbicgstab_multi": OLD + "::test_batched_loops",
    "clcg_hip_spmm": OLD + "::test_complex_block_products",
    "clcg_hip_spmm_dot": OLD + "::test_complex_block_products",
    "clcg_hip_lbicg_sym_multi": OLD + "::test_batched_loops",
    "clcg_hip_lpcg_multi": OLD + "::test_batched_loops",
    "lcg_hip_spmv_c64": OLD + "::test_c128_and_c64_products",
    "clcg_hip_spmm_c64": NEW + "::test_complex64_block_products",
    "clcg_hip_spmm_dot_c64": NEW + "::test_complex64_block_products",
    "clcg_hip_lbicg_sym_multi_c64": _NEW_LOOPS,
    "clcg_hip_lpcg_multi_c64": _NEW_LOOPS,
    "lcg_hip_dot": (OLD + "::test_level_one", "api.dot("),
    "lcg_hip_nrm2": (OLD + "::test_level_one", "api.nrm2("),
    "lcg_hip_axpy": OLD + "::test_level_one",
    "lcg_hip_scal": OLD + "::test_level_one",
    "lcg_hip_set2box": OLD + "::test_level_one",
    "lcg_hip_vecmul": OLD + "::test_level_one",
    "lcg_hip_vecdiv": OLD + "::test_level_one",
    "clcg_hip_dot": (OLD + "::test_level_one", "api.cdot("),
    "clcg_hip_inner": (OLD + "::test_level_one", "api.cdot("),
    "clcg_hip_axpy": NEW + "::test_complex_level_one",
    "clcg_hip_vecdiv": NEW + "::test_complex_level_one",
    # generators
    "lcg_hip_csr_generate": _GENERATED,
    "lcg_hip_csr_generate_ex": _GENERATED,
    "lcg_hip_gen_xtrue": _GENERATED,
    "lcg_hip_csr_laplace2d": _GENERATED,
    # several GPUs
    "lcg_hip_comm_unique_id": _PEERS,
    "lcg_hip_comm_init": _PEERS,
    "lcg_hip_comm_destroy": _PEERS,
    "lcg_hip_comm_rank": _PEERS,
    "lcg_hip_comm_size": _PEERS,
    "lcg_hip_comm_library": _PEERS,
    "lcg_hip_csr_distribute": _PEERS,
    "lcg_hip_csr_exchange_volume": _PEERS,
    "lcg_hip_allreduce_sum": _PEERS,
    "lcg_hip_barrier": _PEERS,
    "lcg_hip_p2p_export": _PEERS,
    "lcg_hip_p2p_connect": _PEERS,
    "lcg_hip_p2p_selftest": _PEERS,
    "lcg_hip_p2p_enable": _PEERS,
    "lcg_hip_p2p_status": _PEERS,
    "lcg_hip_p2p_set_timeout_ms": _PEERS,
    "lcg_hip_p2p_disconnect": _PEERS,
    "lcg_hip_csr_split_for_test": OLD + "::test_sharded_product_on_one_gpu",
    "lcg_hip_csr_xfull": _GETTER,
    "lcg_hip_csr_ax_part_for_probe": _HOOK,
    "lcg_hip_csr_direct_selfloop_for_test": _HOOK,
    "lcg_hip_csr_local_nnz": _GETTER,
    "lcg_hip_csr_need_ranges_for_test": _HOOK,
}
