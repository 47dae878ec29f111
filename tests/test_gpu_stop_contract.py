"""-m gpu: every solver loop's stop, held to the reference's contract bit for bit (tests/stop_cases.py; the CPU twin
tests/test_stop_contract_cpu.py shows the contract on the oracle).  The loops are device-resident: the host enqueues ahead of the
stop test and the passes enqueued behind it must fall through (driver.hpp; devcommon.hpp: should_skip).  So for every loop and size:

  1. a converged solve is the same (ret, iterations, residual, x) with a progress callback (one synchronisation per iteration) as
     without (run-ahead), and the callback is called with k = 0 ... iterations;
  2. the live iterate the callback is handed at k = K is what a fresh solve capped at K returns (-1019, or the converged code where
     the loop converges at K);
  3. a callback that returns non-zero at K ends the solve with code 1, K iterations and that iterate;
  4. nothing is written ahead of the stop: a larger cap changes nothing, caller-owned workspaces come back as the synchronised run
     leaves them, b is untouched and so are 64 guard elements on either side of m and b;
  5. a solve does not remember the previous one (state and partial-sum pairs left on the other parity by another family);
  6. a NaN in b -- first element, last element (the odd tail), mid-stride -- gives the oracle's return code and count;
  7. a caller's own product (a Python Afp that forwards to the library's product) gives the built-in product's bits.
All of these are identities: no tolerance.  The anchor to the oracle: the converged run under conftest.check_converged_run, and the
callback's iterate at K = 3 against the oracle's third iterate under the rule of the existing capped tests."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import stop_cases as sc
from conftest import ROOT, check_converged_run

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PATTERN64 = 0x7FF8DEAD0000BEEF      # a quiet NaN with a payload nobody computes
PATTERN32 = 0x7FC0BEEF
GUARD = 64
STOP, CAP = 1, -1019


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


def guarded(values):
    """values (numpy) on the device between two runs of GUARD elements of a NaN pattern: (whole buffer, the view that is used)."""
    values = np.ascontiguousarray(values)
    host = np.empty(len(values) + 2 * GUARD, values.dtype)
    if values.dtype == np.complex64:
        host.view(np.uint32)[:] = PATTERN32
    else:
        host.view(np.uint64)[:] = PATTERN64
    host[GUARD:GUARD + len(values)] = values
    buf = torch.from_numpy(host).cuda()
    view = buf[GUARD:GUARD + len(values)]
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return buf, view


def guards_intact(buf):
    h = buf.cpu().numpy()
    words = h.view(np.uint32 if h.dtype == np.complex64 else np.uint64)
    per = words.size // h.size
    pat = PATTERN32 if h.dtype == np.complex64 else PATTERN64
    return bool(np.all(words[:GUARD * per] == pat) and np.all(words[-GUARD * per:] == pat))


class Bench:
    """One loop on one system: the device matrix, the right-hand side, and the runs several tests share."""
    def __init__(self, api, lib, port, L, n, S):
        self.api, self.lib, self.port, self.L, self.n, self.S = api, lib, port, L, n, S
        self.dtype = {"real": np.float64, "c128": np.complex128, "c64": np.complex64}[L.family]
        if L.family == "c64":
            self.A = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"])
        elif L.entry == "dense":
            self.A = api.DenseMatrix.from_array(sc.dense_of(S))
        else:
            self.A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
        if L.factor == "ic0":
            self.A.build_ic0(); self.A.ic0_set_sweeps(L.sweeps)
        elif L.factor == "ilu0":
            self.A.build_ilu0(); self.A.ilu0_set_sweeps(L.sweeps)
        elif L.mfp is not None:
            self.A.build_jacobi()
        self.rhs = sc.rhs_of(L, S)
        self.shadow = port.vecrnd(n, sc.SHADOW_SEED) if L.shadow else None
        if L.entry == "box":
            low, hig = sc.box(S)
            self.low, self.hig = torch.from_numpy(low).cuda(), torch.from_numpy(hig).cuda()
        self.base = None

    def workspaces(self):
        k = {"lcg": 3, "lcgs": 7}.get(self.L.entry, 0)
        return [torch.full((self.n,), 7.25, dtype=torch.float64, device="cuda") for _ in range(k)]

    def solve(self, b=None, cap=0, on_progress=None, afp=None, ws=None):
        """One solve from m = 0.  on_progress(k, m_ptr, residual) -> int.  Returns dict(ret, iters, residual, x (numpy), ks, mbuf,
        bbuf, b_in, ws)."""
        api, L, n, A = self.api, self.L, self.n, self.A
        b_in = np.ascontiguousarray(self.rhs if b is None else b)
        mbuf, m = guarded(np.zeros(n, self.dtype))
        bbuf, bd = guarded(b_in)
        ks = []
        pfp = None
        if on_progress is not None:
            def pfp(inst, mp, res, para, nn, k):
                ks.append(k)
                return int(on_progress(k, mp, res))
        cplx = L.family != "real"
        para = (api.clcg_default_parameters if cplx else api.lcg_default_parameters)(epsilon=L.eps, abs_diff=L.abs_diff, max_iterations=cap)
        ws = self.workspaces() if ws is None else ws
        if L.schedule is not None:
            api.set_cg_schedule(L.schedule)
        try:
            if L.entry == "solver":
                info = api.lcg_solver(afp or L.afp or "lcg_hip_csr_ax", pfp, m, bd, n, para, None if afp else A, L.sid)
            elif L.entry == "dense":
                info = api.lcg_solver("lcg_hip_dense_ata_ax", pfp, m, bd, n, para, A, L.sid)
            elif L.entry == "pre":
                info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", L.mfp, pfp, m, bd, n, para, A)
            elif L.entry == "box":
                info = api.lcg_solver_constrained("lcg_hip_csr_ax", pfp, m, bd, self.low, self.hig, n, para, A, L.sid)
            elif L.entry == "lcg":
                info = api.lcg("lcg_hip_csr_ax", pfp, m, bd, n, para, A, *ws)
            elif L.entry == "lcgs":
                info = api.lcgs("lcg_hip_csr_ax", pfp, m, bd, n, para, A, *ws)
            elif L.entry == "csolver":
                info = api.clcg_solver(afp or "clcg_hip_csr_ax", pfp, m, bd, n, para, None if afp else A, L.sid, shadow=self.shadow)
            elif L.entry == "cpre":
                info = api.clcg_solver_preconditioned("clcg_hip_csr_ax", L.mfp, pfp, m, bd, n, para, A, L.sid)
            elif L.entry == "c64solver":
                info = api.clcg_solver_c64("clcg_hip_csr_ax_c64", pfp, m, bd, n, para, A, L.sid)
            else:
                info = api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", L.mfp, pfp, m, bd, n, para, A, L.sid)
        finally:
            if L.schedule is not None:
                api.set_cg_schedule(api.CG_AUTO)
        return {"ret": info.ret, "iters": info.iterations, "residual": info.residual, "x": m.cpu().numpy(), "ks": ks, "mbuf": mbuf,
                "bbuf": bbuf, "b_in": b_in, "ws": [w.cpu().numpy() for w in ws]}

    def snapshot(self, mp):
        """The live device iterate the callback was handed, copied out with lcg_hip_memcpy."""
        out = np.empty(self.n, self.dtype)
        assert self.lib.lcg_hip_memcpy(out.ctypes.data, mp, out.nbytes, 2) == 0
        return out

    def base_runs(self):
        """The run-ahead solve and the synchronised one (callback returns 0, keeps the iterate at K = 1, 3, last - 1, last)."""
        if self.base is None:
            free = self.solve()
            want = set(sc.pick_ks(free["iters"]))
            seen = {}

            def keep(k, mp, res):
                if k in want:
                    seen[k] = self.snapshot(mp)
                return 0
            synced = self.solve(on_progress=keep)
            self.base = (free, synced, seen)
        return self.base


_systems = {}


@pytest.fixture(scope="module")
def benches(api, lib, port):
    """(loop name, n) -> Bench, made on first use and kept for the module's tests; the device matrices are destroyed at its end."""
    made = {}

    def get(L, n):
        if (L.name, n) not in made:
            if (L.kind, n) not in _systems:
                _systems[(L.kind, n)] = sc.system(L.kind, n)
            made[(L.name, n)] = Bench(api, lib, port, L, n, _systems[(L.kind, n)])
        return made[(L.name, n)]
    yield get
    for B in made.values():
        B.A.destroy()
    made.clear(); _systems.clear(); _oracle_cache.clear()


@pytest.fixture
def bench(benches, request):
    return benches(*request.param)


def same(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def verdict(r):
    return r["ret"], r["iters"], r["residual"]


ALL = pytest.mark.parametrize("bench", sc.CASES, ids=sc.CASE_IDS, indirect=True)


@ALL
def test_synced_is_run_ahead(bench):
    """1: the same bits with a callback as without; k = 0 ... iterations; the count inside the window the oracle's run was held to."""
    free, synced, _ = bench.base_runs()
    print(f"{bench.L.name} n={bench.n}: device iterations {free['iters']} (ret {free['ret']}, residual {free['residual']:.3e})")
    assert free["ret"] == 0 and sc.ITER_WINDOW[0] <= free["iters"] <= sc.ITER_WINDOW[1], verdict(free)
    assert verdict(synced) == verdict(free), (verdict(synced), verdict(free))
    assert synced["ks"] == list(range(free["iters"] + 1)), synced["ks"]
    assert same(synced["x"], free["x"]), float(np.max(np.abs(synced["x"] - free["x"])))


@ALL
def test_callbacks_iterate_is_the_capped_iterate_and_stop_returns_it(bench):
    """2 and 3, at K = 1, 3, the last iteration but one and the last (BiCGStab2 under abs_diff counts two per pass: the counts are
    the ones its callback reports)."""
    free, synced, seen = bench.base_runs()
    last = synced["iters"]
    assert sorted(seen) == sc.pick_ks(last)
    for K in sorted(seen):
        capped = bench.solve(cap=K)
        assert (capped["ret"], capped["iters"]) == ((0 if K == last else CAP), K), (K, verdict(capped))
        assert same(capped["x"], seen[K]), (K, "capped run against the callback's iterate", float(np.max(np.abs(capped["x"] - seen[K]))))
        stopped = bench.solve(on_progress=lambda k, mp, res: int(k == K))
        assert (stopped["ret"], stopped["iters"]) == (STOP, K) and stopped["ks"] == list(range(K + 1)), (K, verdict(stopped))
        assert same(stopped["x"], capped["x"]), (K, "LCG_STOP against the cap", float(np.max(np.abs(stopped["x"] - capped["x"]))))
        if K == last:
            assert same(capped["x"], free["x"])


@ALL
def test_nothing_is_written_ahead_of_the_stop(bench):
    """4: cap = iterations + 50 is the default cap's run; workspaces as the synchronised run leaves them; b and the guards intact."""
    free, synced, _ = bench.base_runs()
    roomy = bench.solve(cap=free["iters"] + 50)
    assert verdict(roomy) == verdict(free) and same(roomy["x"], free["x"])
    for r in (free, synced, roomy):
        assert guards_intact(r["mbuf"]) and guards_intact(r["bbuf"])
        assert same(r["bbuf"].cpu().numpy()[GUARD:-GUARD], r["b_in"])
    assert len(free["ws"]) == {"lcg": 3, "lcgs": 7}.get(bench.L.entry, 0)
    for i, (a, b) in enumerate(zip(free["ws"], synced["ws"])):
        assert same(a, b), ("workspace", i, float(np.max(np.abs(a - b))))
        assert not np.all(a == 7.25), ("workspace never used", i)


@ALL
def test_no_memory_of_the_previous_solve(bench, benches):
    """5: X, a real Y of another family, X, a complex Y, X -- the three X results are the same bits."""
    free, _, _ = bench.base_runs()
    others = []
    for name in ("bicgstab" if bench.L.oracle in ("cg", "pcg", "pg", "spg", "pcg_factor", "cg_dense") else "cg_classic", "c_cgs" if bench.L.name != "c_cgs" else "c_bicg_sym"):
        others.append(benches(sc.BY_NAME[name], 513))
    for Y in others:
        y = Y.solve(cap=7)
        assert (y["ret"], y["iters"]) == (CAP, 7)
        again = bench.solve()
        assert verdict(again) == verdict(free) and same(again["x"], free["x"]), (Y.L.name, verdict(again), verdict(free))


NAN_CAP = 6         # (tests/test_stop_contract_cpu.py: the loops whose reference has no NaN scan would spin without a cap)


@ALL
def test_nan_stop(bench):
    """6: return code and count as the oracle's, with and without a callback (lpg, lspg and clpcg have no NaN scan, in the
    reference and here: both sides run to the cap).  clpbicg has none in the reference either (clcg_eigen.cpp:685-802 spins to the
    cap); the library closes its body with the step of the other complex BiCG loops (solvers_cplx.hip: FinZClose), which stops at
    the first iteration whose sums are NaN with CLCG_NAN_VALUE -- that verdict is asserted there instead of the oracle's spin."""
    L, S = bench.L, bench.S
    for where in ("first", "last", "mid"):
        b = sc.rhs_with_nan(S, where, L)
        if L.oracle == "c_pbicg":
            want = (-1019, 1)
        else:
            o = sc.oracle_run(bench.port, L, S, b=b, cap=NAN_CAP)
            want = (o["ret"], o["iters"])
        r1 = bench.solve(b=b, cap=NAN_CAP)
        r2 = bench.solve(b=b, cap=NAN_CAP, on_progress=lambda k, mp, res: 0)
        assert (r1["ret"], r1["iters"]) == want, (where, "run-ahead", verdict(r1), want)
        assert (r2["ret"], r2["iters"]) == want, (where, "synchronised", verdict(r2), want)
        assert guards_intact(r1["mbuf"]) and guards_intact(r2["mbuf"])


# ---------------------------------------------------------------------------------------------- anchors to the oracle
_oracle_cache = {}


def _cap3_rule(bench, x3, o3):
    L = bench.L
    if L.family == "real":
        from test_gpu_fuzz_solvers import CAPPED_ITERATES_RTOL as tol       # test_short_row_systems_against_the_oracle's capped iterations
    elif L.family == "c128":
        # test_complex_solvers_beyond_one_grid_stride's capped iterations (PCG / PBiCG + Jacobi: the same figure in tests/test_gpu_more_solvers.py)
        from test_gpu_solvers import CAPPED_C128_BICGSTAB_RTOL, CAPPED_C128_RTOL
        tol = CAPPED_C128_BICGSTAB_RTOL if L.name == "c_bicgstab" else CAPPED_C128_RTOL
    else:
        from test_gpu_c64 import _tol       # the rule of tests/test_gpu_c64.py::test_capped_runs_against_the_checker
        import c64_checker as K
        S = bench.S
        ops = K.csr_ops(S["rp"], S["ci"], S["v"], np.complex64)
        m0 = np.zeros(S["n"], np.complex64)
        cap = {"epsilon": L.eps, "abs_diff": L.abs_diff, "max_iterations": 3}
        run = {"c64_bicg": lambda dt, k: K.bicg(ops["A"], ops["AH"], S["b"], m0, cap, dt),
               "c64_bicg_sym": lambda dt, k: K.bicg_sym(ops["A"], S["b"], m0, cap, dt),
               "c64_pcg": lambda dt, k: K.pcg(ops["A"], sc._c64_jacobi(S, dt), S["b"], m0, cap, dt)}[L.oracle]
        _, tol = _tol(run, 3)
    rel = np.linalg.norm(x3.astype(np.complex128) - o3["x"]) / np.linalg.norm(o3["x"])
    print(f"{L.name} n={bench.n}: |x_3 - oracle's| / |oracle's| = {rel:.3e} (rule {tol:.1e})")
    assert rel <= tol, (L.name, bench.n, rel, tol)


@ALL
def test_anchor_to_the_oracle(bench):
    """The converged run under conftest.check_converged_run (every loop's oracle behind the interface that function asks of
    `port`: stop_cases.AsPort), and the callback's iterate at K = 3 against the oracle's third iterate."""
    L, S = bench.L, bench.S
    free, synced, seen = bench.base_runs()

    def solve_gpu(cap):
        r = free if cap == 0 else bench.solve(cap=cap)
        return r["ret"], r["iters"], r["residual"], r["x"]
    # (the right-preconditioned loop iterates on u = M.x, not on x: S["xt"] is no solution of its system, and the distance clause
    #  would compare both sides with a vector neither approaches)
    xt = None if L.oracle == "bicgstab_right" else S["xt"]
    cache = _oracle_cache.setdefault((L.oracle, L.kind, L.factor, L.sweeps, L.eps, bench.n), {})       # loops that share an oracle run share it
    check_converged_run(sc.AsPort(bench.port, L, S), solve_gpu, None, S["rp"], S["ci"], S["v"], bench.rhs, L.eps, L.abs_diff, tag=(L.name, bench.n),
                        samples=1, wide=L.wide, cache=cache, xt=xt, late=L.late)
    if "cap3" not in cache:
        cache["cap3"] = sc.oracle_run(bench.port, L, S, cap=3)
    o3 = cache["cap3"]
    assert (o3["ret"], o3["iters"]) == (CAP, 3)
    _cap3_rule(bench, seen[3], o3)


# ---------------------------------------------------------------------------------------------- 7. a caller's own product
def test_python_afp_complex_bicg(api, lib, port):
    """Complex BiCG at n = 513 through a Python Afp that forwards to the library's product (both forms the loop asks for)."""
    L = sc.BY_NAME["c_bicg"]
    B = Bench(api, lib, port, L, 513, sc.system(L.kind, 513))
    asked = []

    def my_ax(inst, x, y, nn, layout, conj):
        asked.append((layout, conj))
        assert lib.lcg_hip_spmv_op(B.A.h, x, y, layout, conj) == 0
    own = B.solve(afp=my_ax)
    builtin = B.solve()
    assert verdict(own) == verdict(builtin) and builtin["ret"] == 0, (verdict(own), verdict(builtin))
    assert same(own["x"], builtin["x"])
    assert (1, 1) in asked and (0, 0) in asked
    assert guards_intact(own["mbuf"]) and guards_intact(own["bbuf"])
    B.A.destroy()


def test_python_afp_real_loops():
    """CG and BiCGStab at n = 513 through a Python Afp that forwards to lcg_hip_spmv, against the built-in product: the same bits.
    Two things are held equal that have nothing to do with the product: a caller's Afp takes CG's classic schedule (solvers_real.hip:
    solve_cg), so the built-in run is made under CG_CLASSIC; and the built-in product may carry the dot that follows it in its
    epilogue (csr.hip: csr_ax_dot), summed in another order than the loop's own reducing pass -- LCG_HIP_AX_DOT=0 asks for the
    product alone.  That switch is read once per process: the comparison runs in a worker (tests/_afp_worker.py)."""
    env = dict(os.environ); env["LCG_HIP_AX_DOT"] = "0"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_afp_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("afp ")]
    assert [l[1] for l in lines] == ["cg_classic", "bicgstab"], r.stdout
    for _, name, ret_a, it_a, res_a, hash_a, ret_b, it_b, res_b, hash_b, calls, diff in lines:
        assert (ret_a, it_a, res_a, hash_a) == (ret_b, it_b, res_b, hash_b) and ret_a == "0", (name, "max |x_own - x_builtin|", diff, lines)
        assert int(calls) >= int(it_a) + 1, (name, calls, it_a)
