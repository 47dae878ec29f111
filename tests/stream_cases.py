"""Helpers of tests/test_gpu_streams.py: the late-input pattern that shows on WHICH stream the library's work runs.

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

    def pair(self, inputs, call, outputs, enqueue_only, tag=(), anchor=None, on_default=False):
        """(a) then (b); anchor(r, outs) holds run (a) to the exact reference first, so that the identity never compares two wrong
        answers.  Returns run (a)."""
        ra, oa = self.reference(inputs, call, outputs)
        if anchor is not None:
            anchor(ra, oa)
        rb, ob = self.late(inputs, call, outputs, enqueue_only, on_default=on_default)
        assert same_scalars(ra, rb), (tag, "returned values", ra, rb)
        for i, (a, b) in enumerate(zip(oa, ob)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (tag, "output", i, "differs from the run on the own stream",
                                                                       int(np.isnan(b.view(np.float32 if b.dtype == np.complex64 else np.float64)).sum()), "NaN words")
        return ra, oa


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
