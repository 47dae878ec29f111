"""-m gpu: the HIP solvers, called through the C ABI, against the oracle on the reference's own
bundled systems and against the goldens produced by the real liblcg.

Tolerances (fp64).  The GPU sums in tree order and contracts to FMA; the reference sums serially.
How far that may move a result is a property of each ALGORITHM on each system, measured on the
oracle itself by perturbing b in its last bit (tests/test_oracle_sensitivity.py, which pins the
bands used here):
  * CG / PCG / CGS (real): insensitive (1e-15).  Tight run (abs_diff=1, eps=1e-12):
    ||x_gpu - x_oracle|| / ||x_oracle|| <= 1e-9, iteration count within +-3, and no farther from
    case_10K_B than the real liblcg itself.  Loose run (sample8.cu:241-243, eps=1e-6): +-2, 1e-6.
  * BiCGStab (real): the oracle moves by 4e-10 (tight) / 1e-4 (loose) under a 1-ulp change of b,
    and its iteration count by several percent: bands 1e-7 / 5e-3 and +-15 %.
  * complex BiCG-sym / CGS / TFQMR to convergence: the oracle moves by 1e-6..2e-6 and +-3 % in
    iterations: bands 5e-5 relative and +-12 %; ||x - x*|| <= 2e-3 (the reference reaches
    2e-5 .. 1.3e-3).  Their first 12 iterates track the oracle to 1e-9.
  * complex BiCGStab diverges on the bundled systems and is chaotic from the
    first iterations (oracle: 2e-7 on 1K, 6e-3 on 10K after 12 its): return code, count and
    finiteness only, plus 1e-4 on the 1K system after 12 iterations.
"""
# (rel x vs oracle tight, rel x loose, iteration band as a fraction)
REAL_BANDS = {0: (1e-9, 1e-6, 0.0), 1: (1e-9, 1e-6, 0.0), 2: (1e-9, 1e-6, 0.0), 3: (1e-7, 5e-3, 0.15)}
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def A10k(api, case10k):
    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    A.build_jacobi()
    return A


def _solve_real(api, A, sid, b, n, para, m0=None, pfp=None):
    m = torch.zeros(n, dtype=torch.float64, device="cuda") if m0 is None else torch.from_numpy(m0).cuda()
    bd = torch.from_numpy(b).cuda()
    if sid == api.LCG_PCG:
        info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_jacobi_mx", pfp, m, bd, n, para, A)
    else:
        info = api.lcg_solver("lcg_hip_csr_ax", pfp, m, bd, n, para, A, sid)
    return info, m.cpu().numpy()


@pytest.mark.parametrize("sid,name", [(0, "cg"), (1, "pcg"), (2, "cgs"), (3, "bicgstab")])
def test_real_tight_vs_oracle_and_golden(api, port, goldens, case10k, A10k, sid, name):
    from oracle import pyoracle as po
    n, rp, ci, v, b, xs = case10k
    info, x = _solve_real(api, A10k, sid, b, n, api.lcg_default_parameters(epsilon=1e-12, abs_diff=1))
    ref = port.solve(sid, rp, ci, v, b, para=po.default_para(epsilon=1e-12, abs_diff=1), jacobi=(sid == 1))
    gold = goldens[f"real/{name}_e12/x"]
    tol, _, band = REAL_BANDS[sid]
    assert info.ret == ref["ret"] == 0
    assert abs(info.iterations - ref["iters"]) <= max(3, band * ref["iters"])
    assert info.residual <= 1e-12
    assert np.linalg.norm(x - ref["x"]) / np.linalg.norm(ref["x"]) <= tol
    assert np.linalg.norm(x - gold) / np.linalg.norm(gold) <= tol          # the real liblcg's output
    # distance to the known answer: no worse than the real liblcg's own (5e-8 .. 3.5e-7 here)
    assert np.linalg.norm(x - xs) <= 1.1 * np.linalg.norm(gold - xs) + 1e-9 <= 5e-7


@pytest.mark.parametrize("sid,name", [(0, "cg"), (1, "pcg"), (2, "cgs"), (3, "bicgstab")])
def test_real_loose_sample8_setting(api, goldens, case10k, A10k, sid, name):
    n, rp, ci, v, b, xs = case10k
    info, x = _solve_real(api, A10k, sid, b, n, api.lcg_default_parameters(epsilon=1e-6, abs_diff=0))
    ret, iters = goldens[f"real/{name}_e6/meta"][:2]
    gold = goldens[f"real/{name}_e6/x"]
    _, tol, band = REAL_BANDS[sid]
    assert info.ret == ret == 0
    assert abs(info.iterations - iters) <= max(2, band * iters)
    assert np.linalg.norm(x - gold) / np.linalg.norm(gold) <= tol


def test_max_iterations_and_counts(api, goldens, case10k, A10k):
    n, rp, ci, v, b, _ = case10k
    info, x = _solve_real(api, A10k, 0, b, n, api.lcg_default_parameters(epsilon=1e-12, abs_diff=1, max_iterations=25))
    gold = goldens["real/cg_max25/x"]
    assert info.ret == -1019 and info.iterations == 25                     # LCG_REACHED_MAX_ITERATIONS
    assert np.linalg.norm(x - gold) / np.linalg.norm(gold) <= 1e-10
    assert abs(info.residual - goldens["real/cg_max25/fl"][1]) <= 1e-9 * info.residual


def test_argument_errors(api, case10k, A10k):
    n, rp, ci, v, b, _ = case10k
    assert _solve_real(api, A10k, 0, b, n, api.lcg_default_parameters(max_iterations=-1))[0].ret == -1022
    assert _solve_real(api, A10k, 0, b, n, api.lcg_default_parameters(epsilon=0.0))[0].ret == -1021
    assert _solve_real(api, A10k, 0, b, n, api.lcg_default_parameters(epsilon=1.0))[0].ret == -1021
    from liblcg_amd import _lib
    lib = _lib.load()
    p = api.lcg_default_parameters()
    assert lib.lcg_hip_solver(_lib.fnptr(lib, "lcg_hip_csr_ax"), None, None, None, 0, C.byref(p), A10k.h, 0, 1) == -1023
    assert lib.lcg_hip_solver(_lib.fnptr(lib, "lcg_hip_csr_ax"), None, None, None, 5, C.byref(p), A10k.h, 0, 1) == -1016
    assert lib.lcg_hip_solver_preconditioned(_lib.fnptr(lib, "lcg_hip_csr_ax"), None, None, 8, 8, 5, C.byref(p),
                                             A10k.h, 1, 1) == -1018


def test_already_optimized_and_unknown_solver(api, case10k, A10k):
    n, rp, ci, v, b, xs = case10k
    for sid in (0, 1, 2, 3):
        info, x = _solve_real(api, A10k, sid, b, n, api.lcg_default_parameters(epsilon=1e-6), m0=xs.copy())
        assert info.ret == 2 and info.iterations == 0
        assert np.array_equal(x, xs)
    a, xa = _solve_real(api, A10k, api.LCG_CGS, b, n, api.lcg_default_parameters())
    for sid in (5, 6):                  # lcg.cpp:76-78: PG/SPG handed to lcg_solver run CGS
        c, xc = _solve_real(api, A10k, sid, b, n, api.lcg_default_parameters())
        assert c.iterations == a.iterations and np.array_equal(xa, xc)


def test_progress_callback_trace_and_stop(api, port, case10k, A10k):
    """Pfp sees (device m, residual, k) before every iteration (lcg.cpp:211-217); non-zero stops."""
    n, rp, ci, v, b, _ = case10k
    seen = []

    def pfp(inst, m_ptr, conv, para, nn, k):
        seen.append((k, conv, para.contents.epsilon, nn))
        return 1 if k == 7 else 0
    info, x = _solve_real(api, A10k, 0, b, n, api.lcg_default_parameters(epsilon=1e-10, abs_diff=1), pfp=pfp)
    assert info.ret == 1 and info.iterations == 7                          # LCG_STOP
    assert [s[0] for s in seen] == list(range(8))
    assert all(s[2] == 1e-10 and s[3] == n for s in seen)
    res = [s[1] for s in seen]
    assert all(res[i + 1] < res[0] * 10 for i in range(7))
    # the callback path and the asynchronous path walk the same iterates
    seen2 = []
    info2, x2 = _solve_real(api, A10k, 0, b, n, api.lcg_default_parameters(epsilon=1e-10, abs_diff=1),
                            pfp=lambda i, m, c, p, nn, k: seen2.append(c) or 0)
    info3, x3 = _solve_real(api, A10k, 0, b, n, api.lcg_default_parameters(epsilon=1e-10, abs_diff=1))
    assert info2.ret == info3.ret == 0 and info2.iterations == info3.iterations == len(seen2) - 1
    assert np.array_equal(x2, x3)
    assert seen2[:8] == res


def test_nan_is_reported(api, case10k, A10k):
    n, rp, ci, v, b, _ = case10k
    bad = b.copy(); bad[123] = np.nan
    info, x = _solve_real(api, A10k, 0, bad, n, api.lcg_default_parameters())
    assert info.ret == -1017 and info.iterations == 1                      # LCG_NAN_VALUE, first iteration
    info, x = _solve_real(api, A10k, 3, bad, n, api.lcg_default_parameters())
    assert info.ret == -1017


def test_host_memory_in_out(api, port, case10k, A10k):
    """mem == HOST: numpy in, numpy out (lcg_solver_cuda behaviour, lcg_cuda.cu:103-111,210)."""
    n, rp, ci, v, b, xs = case10k
    m = np.zeros(n)
    info = api.lcg_solver("lcg_hip_csr_ax", None, m, b, n, api.lcg_default_parameters(epsilon=1e-12, abs_diff=1), A10k, api.LCG_CG)
    assert info.ret == 0 and np.linalg.norm(m - xs) <= 1e-7


def test_caller_workspaces(api, case10k, A10k):
    """lcg()/lcgs() with external vectors (lcg.h:129-131,151-158) give the same iterates."""
    n, rp, ci, v, b, xs = case10k
    bd = torch.from_numpy(b).cuda()
    p = api.lcg_default_parameters(epsilon=1e-12, abs_diff=1)
    ws = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(7)]
    m1 = torch.zeros(n, dtype=torch.float64, device="cuda"); m2 = torch.zeros_like(m1)
    i1 = api.lcg("lcg_hip_csr_ax", None, m1, bd, n, p, A10k, *ws[:3])
    i2 = api.lcg("lcg_hip_csr_ax", None, m2, bd, n, p, A10k)
    assert i1.ret == i2.ret == 0 and i1.iterations == i2.iterations and torch.equal(m1, m2)
    m1.zero_(); m2.zero_()
    i1 = api.lcgs("lcg_hip_csr_ax", None, m1, bd, n, p, A10k, *ws)
    i2 = api.lcg_solver("lcg_hip_csr_ax", None, m2, bd, n, p, A10k, api.LCG_CGS)
    assert i1.ret == i2.ret == 0 and i1.iterations == i2.iterations and torch.equal(m1, m2)


def test_python_callback_as_afp(api, case10k, A10k):
    """A user-written A.x callback (here: Python launching the library's kernel on the solver
    stream) plugs into the unchanged lcg_axfunc_ptr signature."""
    n, rp, ci, v, b, xs = case10k
    from liblcg_amd import _lib
    lib = _lib.load()
    calls = [0]

    def my_ax(inst, x, y, nn):
        calls[0] += 1
        lib.lcg_hip_spmv(A10k.h, x, y)
    m = torch.zeros(n, dtype=torch.float64, device="cuda")
    info = api.lcg_solver(my_ax, None, m, torch.from_numpy(b).cuda(), n,
                          api.lcg_default_parameters(epsilon=1e-12, abs_diff=1), None, api.LCG_CG)
    assert info.ret == 0 and calls[0] >= info.iterations + 1
    assert np.linalg.norm(m.cpu().numpy() - xs) <= 1e-7


def test_already_optimised_with_a_user_callback_calls_it_as_the_reference_does(api, case10k, A10k):
    """lcg.cpp:168-203: with a start that already meets the tolerance the reference calls Afp ONCE (the set-up product) and
    returns LCG_ALREADY_OPTIMIZIED.  A user's callback cannot honour the device's stop flag, so nothing may be enqueued ahead of
    that verdict (up to 24 bodies used to be)."""
    n, rp, ci, v, b, xs = case10k
    from liblcg_amd import _lib
    lib = _lib.load()
    for sid, per_setup in ((api.LCG_CG, 1), (api.LCG_CGS, 1), (api.LCG_BICGSTAB, 1)):
        calls = [0]

        def my_ax(inst, x, y, nn):
            calls[0] += 1
            lib.lcg_hip_spmv(A10k.h, x, y)
        m = torch.from_numpy(xs.copy()).cuda()
        info = api.lcg_solver(my_ax, None, m, torch.from_numpy(b).cuda(), n, api.lcg_default_parameters(epsilon=1e-6), None, sid)
        assert info.ret == 2 and info.iterations == 0 and calls[0] == per_setup, (sid, info.ret, calls[0])
        assert np.array_equal(m.cpu().numpy(), xs)


def test_cg_schedules_on_an_ill_conditioned_system(api, port):
    """Below 2^17 rows one GPU runs CG in the one-reduction (Chronopoulos-Gear) arrangement (two launches per iteration); the
    reference's loop (lcg.cpp:206-264) is the classic two-reduction recurrence.  Same iterates in exact arithmetic -- here on
    a system where rounding has room to show: the 1D Laplacian of 3000 rows (condition number 3.6e6; 2981 iterations to 1e-16).
    Both schedules against the oracle's classic loop: iteration counts in the band the oracle's own 1-ulp sensitivity gives,
    the TRUE residual of the answer within the stop rule, and the monitored residual equal to the true one."""
    from oracle import pyoracle as po
    n = 3000
    rp = np.zeros(n + 1, np.int32); ci = []; v = []
    for i in range(n):
        for j, a in ((i - 1, -1.0), (i, 2.0), (i + 1, -1.0)):
            if 0 <= j < n:
                ci.append(j); v.append(a)
        rp[i + 1] = len(ci)
    ci = np.array(ci, np.int32); v = np.array(v)
    rng = np.random.default_rng(5)
    xt = rng.standard_normal(n)
    b = port.csr_matvec(rp, ci, v, xt)
    eps = 1e-16
    opara = po.default_para(epsilon=eps, abs_diff=0, max_iterations=20000)
    ref = port.solve(po.LCG_CG, rp, ci, v, b, para=opara)
    assert ref["ret"] == 0 and ref["iters"] > 1000
    dit = 0
    for k in range(3):
        alt = port.solve(po.LCG_CG, rp, ci, v, b * (1.0 + 1e-16 * np.random.default_rng(k).standard_normal(n)), para=opara)
        dit = max(dit, abs(alt["iters"] - ref["iters"]))
    A = api.CsrMatrix.from_csr(rp, ci, v)
    bd = torch.from_numpy(b).cuda()
    try:
        for sched in (api.CG_AUTO, api.CG_CLASSIC, api.CG_ONE_REDUCTION):
            api.set_cg_schedule(sched)
            m = torch.zeros(n, dtype=torch.float64, device="cuda")
            info = api.lcg_solver("lcg_hip_csr_ax", None, m, bd, n, api.lcg_default_parameters(epsilon=eps, abs_diff=0, max_iterations=20000), A, api.LCG_CG)
            x = m.cpu().numpy()
            tag = (sched, info.ret, info.iterations, ref["iters"], dit)
            assert info.ret == 0, tag
            assert abs(info.iterations - ref["iters"]) <= max(5, 3 * dit, 0.03 * ref["iters"]), tag
            r = port.csr_matvec(rp, ci, v, x) - b
            true_res = float(r @ r) / max(float(x @ x), 1.0)               # lcg.cpp:208-222 (relative form)
            # the recurred g.g is what the stop rule sees; it may not flatter the answer
            assert true_res <= 4.0 * eps and abs(true_res - info.residual) <= 0.5 * info.residual + 1e-14, tag + (true_res, info.residual)
            assert np.linalg.norm(x - xt) <= 3.0 * np.linalg.norm(ref["x"] - xt), tag
        # PCG with the built-in Jacobi has the same two arrangements (lpcg, lcg.cpp:361-423, and its one-reduction form); on a
        # diagonal that is not constant, so that the preconditioner is not a mere scaling: D A D with D = diag(1 .. 3)
        dg = 1.0 + 2.0 * rng.random(n)
        v2 = v * dg[np.repeat(np.arange(n), np.diff(rp))] * dg[ci]
        b2 = port.csr_matvec(rp, ci, v2, xt)
        ref2 = port.solve(po.LCG_PCG, rp, ci, v2, b2, para=opara, jacobi=True)
        dit2 = 0
        for k in range(3):
            alt = port.solve(po.LCG_PCG, rp, ci, v2, b2 * (1.0 + 1e-16 * np.random.default_rng(k).standard_normal(n)), para=opara, jacobi=True)
            dit2 = max(dit2, abs(alt["iters"] - ref2["iters"]))
        assert ref2["ret"] == 0 and ref2["iters"] > 1000
        A2 = api.CsrMatrix.from_csr(rp, ci, v2); A2.build_jacobi()
        bd2 = torch.from_numpy(b2).cuda()
        for sched in (api.CG_AUTO, api.CG_CLASSIC, api.CG_ONE_REDUCTION):
            api.set_cg_schedule(sched)
            m = torch.zeros(n, dtype=torch.float64, device="cuda")
            info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_jacobi_mx", None, m, bd2, n,
                                                 api.lcg_default_parameters(epsilon=eps, abs_diff=0, max_iterations=20000), A2)
            x = m.cpu().numpy()
            tag = ("pcg", sched, info.ret, info.iterations, ref2["iters"], dit2)
            assert info.ret == 0, tag
            assert abs(info.iterations - ref2["iters"]) <= max(5, 3 * dit2, 0.03 * ref2["iters"]), tag
            r = port.csr_matvec(rp, ci, v2, x) - b2
            true_res = float(r @ r) / max(float(x @ x), 1.0)
            assert true_res <= 4.0 * eps and abs(true_res - info.residual) <= 0.5 * info.residual + 1e-14, tag + (true_res, info.residual)
            assert np.linalg.norm(x - xt) <= 3.0 * np.linalg.norm(ref2["x"] - xt), tag
        A2.destroy()
    finally:
        api.set_cg_schedule(api.CG_AUTO)
    A.destroy()


# ------------------------------------------------------------------------------- complex
def _solve_cplx(api, A, sid, b, n, para, shadow=None):
    m = torch.zeros(n, dtype=torch.complex128, device="cuda")
    info = api.clcg_solver("clcg_hip_csr_ax", None, m, torch.from_numpy(b).cuda(), n, para, A, sid, shadow=shadow)
    return info, m.cpu().numpy()


@pytest.mark.parametrize("case", ["1K", "10K"])
def test_complex_bicg_symmetric(api, port, goldens, case1kc, case10kc, case):
    from oracle import pyoracle as po
    n, rp, ci, v, b, xs = case1kc if case == "1K" else case10kc
    A = api.CsrMatrix.from_csr(rp, ci, v)
    info, x = _solve_cplx(api, A, api.CLCG_BICG_SYM, b, n, api.clcg_default_parameters(epsilon=1e-10, abs_diff=1))
    ref = port.csolve(po.CLCG_BICG_SYM, rp, ci, v, b, para=po.default_cpara(epsilon=1e-10, abs_diff=1))
    assert info.ret == ref["ret"] == 0
    assert abs(info.iterations - ref["iters"]) <= 0.12 * ref["iters"]
    assert np.linalg.norm(x - ref["x"]) / np.linalg.norm(ref["x"]) <= 5e-5
    assert np.linalg.norm(x - xs) <= 2e-3
    gold = goldens[f"cplx/bicgsym_{case}/x"]
    assert np.linalg.norm(x - gold) / np.linalg.norm(gold) <= 5e-5


@pytest.mark.parametrize("case", ["1K", "10K"])
def test_complex_bicg_with_adjoint_product(api, port, goldens, case1kc, case10kc, case):
    """clbicg (clcg.cpp:77-226): the second product of every iteration is A^H.d2 (:187)."""
    from oracle import pyoracle as po
    n, rp, ci, v, b, xs = case1kc if case == "1K" else case10kc
    A = api.CsrMatrix.from_csr(rp, ci, v)
    info, x = _solve_cplx(api, A, api.CLCG_BICG, b, n, api.clcg_default_parameters(epsilon=1e-10, abs_diff=1))
    ret, iters = goldens[f"cplx/bicg_{case}/meta"][:2]
    gold = goldens[f"cplx/bicg_{case}/x"]
    assert info.ret == ret == 0
    assert abs(info.iterations - iters) <= 0.12 * iters
    assert np.linalg.norm(x - gold) / np.linalg.norm(gold) <= 5e-5
    assert np.linalg.norm(x - xs) <= 2e-3
    # first iterates track the oracle tightly
    i12, x12 = _solve_cplx(api, A, api.CLCG_BICG, b, n, api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=12))
    ref = port.csolve(po.CLCG_BICG, rp, ci, v, b, para=po.default_cpara(epsilon=1e-10, abs_diff=1, max_iterations=12))
    assert i12.ret == ref["ret"] == -1019 and i12.iterations == 12
    assert np.linalg.norm(x12 - ref["x"]) <= 1e-9 * np.linalg.norm(ref["x"])


XS_BAND = 1e-2     # |x - x_known| of a converged complex CGS / TFQMR run on the bundled systems (see the sensitivity test)


@pytest.mark.parametrize("sid,name", [(2, "cgs"), (4, "tfqmr")])
@pytest.mark.parametrize("case", ["1K", "10K"])
def test_complex_shadow_solvers(api, port, goldens, case1kc, case10kc, sid, name, case):
    """CGS / TFQMR with the reference's own shadow residual replayed (seed from the golden)."""
    n, rp, ci, v, b, xs = case1kc if case == "1K" else case10kc
    A = api.CsrMatrix.from_csr(rp, ci, v)
    ret, iters, _, _, _, seed = goldens[f"cplx/{name}_{case}/meta"]
    rbar0 = port.vecrnd(n, int(seed))
    info, x = _solve_cplx(api, A, sid, b, n, api.clcg_default_parameters(epsilon=1e-10, abs_diff=1), shadow=rbar0)
    assert info.ret == ret == 0
    assert info.residual <= 1e-10
    assert abs(info.iterations - iters) <= 0.12 * iters                 # rounding-order sensitive recurrences
    # distance to the bundled answer at the stop (sqrt(r.r)/N <= 1e-10): the reference's own runs end 0.6e-3 .. 4.1e-3 away on
    # the 10K system depending on 1-ulp changes of b (tests/test_oracle_sensitivity.py::test_complex_10k_distance_to_the_known_answer)
    assert np.linalg.norm(x - xs) <= XS_BAND
    gold = goldens[f"cplx/{name}_{case}/x"]
    assert np.linalg.norm(x - gold) / np.linalg.norm(gold) <= 5e-5
    # default (seeded) shadow vector: still converges to the known answer
    info2, x2 = _solve_cplx(api, A, sid, b, n, api.clcg_default_parameters(epsilon=1e-10, abs_diff=1))
    assert info2.ret == 0 and np.linalg.norm(x2 - xs) <= XS_BAND


def test_complex_bicgstab_and_cap(api, port, goldens, case1kc):
    """clbicgstab does not converge on the bundled systems: the cap returns the
    REAL enum's -1019 as clcg.cpp:164 does; TFQMR returns cleanly at the cap (documented deviation)."""
    n, rp, ci, v, b, xs = case1kc
    A = api.CsrMatrix.from_csr(rp, ci, v)
    info, x = _solve_cplx(api, A, api.CLCG_BICGSTAB, b, n, api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=300))
    assert info.ret == -1019 and info.iterations == 300 and np.all(np.isfinite(x))
    for cap in (10, 11):
        info, x = _solve_cplx(api, A, api.CLCG_TFQMR, b, n, api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=cap))
        assert info.ret == -1019 and info.iterations == cap
    # early iterates follow the oracle closely when the same shadow vector is used
    from oracle import pyoracle as po
    rbar0 = port.vecrnd(n, 42)
    for sid in (po.CLCG_CGS, po.CLCG_BICGSTAB, po.CLCG_TFQMR):
        info, x = _solve_cplx(api, A, sid, b, n, api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=12), shadow=rbar0)
        ref = port.csolve(sid, rp, ci, v, b, para=po.default_cpara(epsilon=1e-10, abs_diff=1, max_iterations=12), rbar0=rbar0)
        tol = 1e-4 if sid == po.CLCG_BICGSTAB else 1e-9
        assert info.ret == ref["ret"] == -1019 and info.iterations == ref["iters"] == 12
        assert np.linalg.norm(x - ref["x"]) <= tol * np.linalg.norm(ref["x"])
        assert abs(info.residual - ref["residual"]) <= 100 * tol * abs(ref["residual"])


def test_temporaries_are_kept_between_solves_and_can_be_given_back(api, case10k, A10k):
    """The reference allocates and frees its temporaries per call (lcg.cpp:158-166,266-271); here they stay for the next solve
    (no hipMalloc / hipFree inside the timed region of a repeated solve) until lcg_hip_trim(): same answers either way, and the
    device memory comes back."""
    from liblcg_amd import _lib
    lib = _lib.load()
    n, rp, ci, v, b, xs = case10k
    p = api.lcg_default_parameters(epsilon=1e-12, abs_diff=1)
    assert lib.lcg_hip_trim() == 0
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    i1, x1 = _solve_real(api, A10k, api.LCG_CGS, b, n, p)            # seven work vectors
    i2, x2 = _solve_real(api, A10k, api.LCG_CGS, b, n, p)            # ... reused
    i3, x3 = _solve_real(api, A10k, api.LCG_CG, b, n, p)             # a smaller set from the same pool
    assert i1.ret == i2.ret == i3.ret == 0 and np.array_equal(x1, x2) and i1.iterations == i2.iterations
    assert np.linalg.norm(x3 - xs) <= 1e-7
    assert lib.lcg_hip_trim() == 0
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (1 << 21)        # nothing of the solves' scratch is still held
    i4, x4 = _solve_real(api, A10k, api.LCG_CGS, b, n, p)
    assert np.array_equal(x1, x4)


def test_cache_policy_of_the_vector_passes_changes_no_bit():
    """Large systems read and write what the next kernels do not need with non-temporal accesses (solvers_real.hip: stream_vectors).
    That is a cache hint: with the policy forced off and forced on, in two processes, every solver's iterate after 25 iterations must be
    the same to the last bit (CG and PCG + Jacobi in both schedules, CGS, BiCGStab)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for nt in ("0", "1"):
        env = dict(os.environ); env["LCG_HIP_NT_VECTORS"] = nt
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "_nt_worker.py")], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("iterate ")]
        assert len(lines) == 7, r.stdout
        outs.append(lines)
    assert outs[0] == outs[1], outs


@pytest.mark.parametrize("guess", ["zeros", "one_component", "random", "negative_zeros"])
def test_initial_guess_and_the_product_that_is_not_made(api, port, case10k, guess):
    """The reference multiplies the initial guess before anything else (lcg.cpp:168, 314, 476, 648).  The library probes the guess on the
    device and does not make that product when it is all zeros (solvers_real.hip: ax_setup): capped iterates of all four solvers against
    the oracle's loop from the same guess -- all zeros (the product is skipped), a single non-zero component and a random guess (it is
    made), and negative zeros (skipped: -0 == 0, and A.(-0) adds up to zeros)."""
    from oracle import pyoracle as po
    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    A.build_jacobi()
    rng = np.random.default_rng(11)
    m0 = {"zeros": np.zeros(n), "one_component": np.zeros(n), "random": rng.standard_normal(n), "negative_zeros": -np.zeros(n)}[guess]
    if guess == "one_component":
        m0[n // 3] = 1e-3
    bd = torch.from_numpy(b).cuda()
    for sid, jac in ((api.LCG_CG, False), (api.LCG_PCG, True), (api.LCG_CGS, False), (api.LCG_BICGSTAB, False)):
        para = api.lcg_default_parameters(epsilon=1e-20, abs_diff=1, max_iterations=9)
        m = torch.from_numpy(m0.copy()).cuda()
        if jac:
            info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_jacobi_mx", None, m, bd, n, para, A)
        else:
            info = api.lcg_solver("lcg_hip_csr_ax", None, m, bd, n, para, A, sid)
        ref = port.solve(sid, rp, ci, v, b, m0=m0, para=po.default_para(epsilon=1e-20, abs_diff=1, max_iterations=9), jacobi=jac)
        x = m.cpu().numpy()
        assert info.ret == ref["ret"] and info.iterations == ref["iters"] == 9
        assert np.linalg.norm(x - ref["x"]) <= 1e-12 * np.linalg.norm(ref["x"]), (guess, sid)
        assert abs(info.residual - ref["residual"]) <= 1e-9 * ref["residual"]
    A.destroy()


CAPPED_C128_RTOL, CAPPED_C128_BICGSTAB_RTOL = 1e-9, 1e-6     # capped complex128 iterates against the oracle's (BiCGStab: chaotic from the start)


def test_complex_solvers_beyond_one_grid_stride(api, port):
    """The bundled complex systems have 10^3 / 10^4 rows: every vector pass is one grid stride of <= 40 workgroups and every
    product a few dozen blocks.  Here 360,000 rows -- a damped 2-D Helmholtz operator, 5-point Laplacian + (0.3 + 0.8i) I: complex
    symmetric, every eigenvalue off the real axis -- so that the passes walk several strides of the 512-workgroup grid, the partial
    sums fill their table and the product runs on thousands of blocks.  A.x and A^H.x row-wise against the oracle's products at
    1e-13 |A||x|; twelve capped iterations of BiCG-sym, BiCG (adjoint product), CGS, BiCGStab and TFQMR against the oracle's loops
    (clcg.cpp:228-881 restated) with the same shadow residual; BiCG-sym to convergence against the oracle's converged run."""
    from oracle import pyoracle as po
    nx = 600
    n = nx * nx
    idx = np.arange(n, dtype=np.int64)
    ix, iy = idx % nx, idx // nx
    rows, cols, vals = [idx], [idx], [np.full(n, 4.0 + 0.3 + 0.8j, dtype=np.complex128)]
    for ok, off in ((ix > 0, -1), (ix < nx - 1, 1), (iy > 0, -nx), (iy < nx - 1, nx)):
        rows.append(idx[ok]); cols.append(idx[ok] + off); vals.append(np.full(int(ok.sum()), -1.0 + 0.0j, dtype=np.complex128))
    row = np.concatenate(rows).astype(np.int32); col = np.concatenate(cols).astype(np.int32); val = np.concatenate(vals)
    order = np.lexsort((col, row))
    row, col, val = row[order], col[order], val[order]
    rp = np.zeros(n + 1, dtype=np.int32); np.add.at(rp, row + 1, 1); rp = np.cumsum(rp).astype(np.int32)
    A = api.CsrMatrix.from_csr(rp, col, val)
    rng = np.random.default_rng(11)
    xt = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    # products
    xd = torch.from_numpy(xt).cuda(); yd = torch.empty_like(xd)
    A.spmv(xd, yd); api.synchronize()
    ref = port.csr_matvec(rp, col, val, xt)
    bound = port.csr_matvec(rp, col, np.abs(val).astype(np.complex128), np.abs(xt).astype(np.complex128)).real
    assert np.max(np.abs(yd.cpu().numpy() - ref) / bound) <= 1e-13
    b = ref
    rbar0 = port.vecrnd(n, 7)
    cap = api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=12)
    ocap = po.default_cpara(epsilon=1e-10, abs_diff=1, max_iterations=12)
    for sid, tol in ((po.CLCG_BICG_SYM, CAPPED_C128_RTOL), (po.CLCG_BICG, CAPPED_C128_RTOL), (po.CLCG_CGS, CAPPED_C128_RTOL),
                     (po.CLCG_BICGSTAB, CAPPED_C128_BICGSTAB_RTOL), (po.CLCG_TFQMR, CAPPED_C128_RTOL)):
        shadow = None if sid in (po.CLCG_BICG_SYM, po.CLCG_BICG) else rbar0
        info, x = _solve_cplx(api, A, sid, b, n, cap, shadow=shadow)
        o = port.csolve(sid, rp, col, val, b, para=ocap, rbar0=shadow) if shadow is not None else port.csolve(sid, rp, col, val, b, para=ocap)
        assert info.ret == o["ret"] == -1019 and info.iterations == o["iters"] == 12, (sid, info.ret, o["ret"], info.iterations, o["iters"])
        assert np.linalg.norm(x - o["x"]) <= tol * np.linalg.norm(o["x"]), (sid, np.linalg.norm(x - o["x"]) / np.linalg.norm(o["x"]))
        assert abs(info.residual - o["residual"]) <= 1e3 * tol * abs(o["residual"]), (sid, info.residual, o["residual"])
    # to convergence
    tight = api.clcg_default_parameters(epsilon=1e-12, abs_diff=1)
    info, x = _solve_cplx(api, A, po.CLCG_BICG_SYM, b, n, tight)
    o = port.csolve(po.CLCG_BICG_SYM, rp, col, val, b, para=po.default_cpara(epsilon=1e-12, abs_diff=1))
    assert info.ret == o["ret"] == 0 and abs(info.iterations - o["iters"]) <= max(3, 0.05 * o["iters"])
    assert np.linalg.norm(x - o["x"]) <= 1e-7 * np.linalg.norm(o["x"]) and np.linalg.norm(x - xt) <= 1e-6 * np.linalg.norm(xt)
    A.destroy()


def test_tiny_and_ragged_systems(api, port):
    """n = 1, 2, 3, 5, 63, 64, 65, 129, 257 -- below, at and just above a wavefront and a row block -- SPD, ragged (rows that hold
    nothing but their diagonal), with a right-hand side and with b = 0 (lcg.cpp:186-203: LCG_ALREADY_OPTIMIZIED before the first
    iteration), both stop rules, CG / PCG + Jacobi / CGS / BiCGStab: return code, iteration count (+-1) and solution as the oracle's."""
    from oracle import pyoracle as po
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 5, 63, 64, 65, 129, 257):
        off = rng.standard_normal(n - 1) * (rng.random(n - 1) < 0.7) if n > 1 else np.zeros(0)
        d = np.full(n, 0.5)
        rows, cols, vals = list(range(n)), list(range(n)), None
        ov = []
        for i in range(n - 1):
            if off[i] != 0.0:
                rows += [i, i + 1]; cols += [i + 1, i]; ov += [off[i], off[i]]
                d[i] += abs(off[i]); d[i + 1] += abs(off[i])
        row = np.array(rows, np.int32); col = np.array(cols, np.int32); val = np.concatenate([d, np.array(ov, dtype=np.float64)])
        o = np.lexsort((col, row)); row, col, val = row[o], col[o], val[o]
        rp = np.zeros(n + 1, np.int32); np.add.at(rp, row + 1, 1); rp = np.cumsum(rp).astype(np.int32)
        A = api.CsrMatrix.from_csr(rp, col, val); A.build_jacobi()
        b = port.csr_matvec(rp, col, val, rng.standard_normal(n))
        for sid, name in ((api.LCG_CG, "cg"), (api.LCG_PCG, "pcg"), (api.LCG_CGS, "cgs"), (api.LCG_BICGSTAB, "bicgstab")):
            for eps, ad in ((1e-12, 1), (1e-10, 0)):
                for bh in (b, np.zeros(n)):
                    bd = torch.from_numpy(bh).cuda()
                    m = torch.zeros(n, dtype=torch.float64, device="cuda")
                    para = api.lcg_default_parameters(epsilon=eps, abs_diff=ad)
                    if sid == api.LCG_PCG:
                        info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_jacobi_mx", None, m, bd, n, para, A)
                    else:
                        info = api.lcg_solver("lcg_hip_csr_ax", None, m, bd, n, para, A, sid)
                    ref = port.solve(sid, rp, col, val, bh, para=po.default_para(epsilon=eps, abs_diff=ad), jacobi=(sid == api.LCG_PCG))
                    tag = (n, name, eps, ad, "b = 0" if not bh.any() else "b", info.ret, info.iterations, ref["ret"], ref["iters"])
                    assert info.ret == ref["ret"] and abs(info.iterations - ref["iters"]) <= 1, tag
                    if not np.all(np.isfinite(ref["x"])):       # (n = 1: BiCGStab breaks down exactly on both sides -- LCG_NAN_VALUE, the same code)
                        assert info.ret == -1017, tag
                        continue
                    assert np.linalg.norm(m.cpu().numpy() - ref["x"]) <= 1e-9 * max(1.0, np.linalg.norm(ref["x"])), tag
        A.destroy()


def test_tiny_complex_systems(api, port):
    """The complex solvers on n = 1 ... 129 (complex symmetric, ragged), with a right-hand side and with b = 0: return code, iteration
    count (+-2) and solution (5e-5: the band of the converged complex runs on the bundled systems) as the oracle's, the same shadow
    residual on both sides.  One known difference, kept here on purpose: at n = 1 TFQMR reaches the exact solution in its first half
    step, and the next half step divides 0 by 0 in the reference (theta = omega / tao, clcg.cpp:832: CLCG_NAN_VALUE after one
    iteration) -- here alpha = rho / sigma rounds differently (Smith's division against libgcc's), the residual is 1e-32 instead of 0,
    and the solve returns the converged solution."""
    from oracle import pyoracle as po
    rng = np.random.default_rng(4)
    for n in (1, 2, 3, 5, 63, 64, 65, 129):
        off = (rng.standard_normal(n - 1) + 1j * rng.standard_normal(n - 1)) * (rng.random(n - 1) < 0.7) if n > 1 else np.zeros(0, complex)
        d = np.full(n, 0.5 + 0.3j)
        rows, cols, ov = list(range(n)), list(range(n)), []
        for i in range(n - 1):
            if off[i] != 0:
                rows += [i, i + 1]; cols += [i + 1, i]; ov += [off[i], off[i]]
                d[i] += abs(off[i]); d[i + 1] += abs(off[i])
        row = np.array(rows, np.int32); col = np.array(cols, np.int32); val = np.concatenate([d, np.array(ov, dtype=np.complex128)])
        o = np.lexsort((col, row)); row, col, val = row[o], col[o], val[o]
        rp = np.zeros(n + 1, np.int32); np.add.at(rp, row + 1, 1); rp = np.cumsum(rp).astype(np.int32)
        A = api.CsrMatrix.from_csr(rp, col, val)
        xt = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        b = port.csr_matvec(rp, col, val, xt)
        rbar0 = port.vecrnd(n, 9)
        for sid in (po.CLCG_BICG, po.CLCG_BICG_SYM, po.CLCG_CGS, po.CLCG_BICGSTAB, po.CLCG_TFQMR):
            for bh in (b, np.zeros(n, complex)):
                sh = None if sid in (po.CLCG_BICG, po.CLCG_BICG_SYM) else rbar0
                info, x = _solve_cplx(api, A, sid, bh, n, api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=200), shadow=sh)
                opara = po.default_cpara(epsilon=1e-10, abs_diff=1, max_iterations=200)
                ref = port.csolve(sid, rp, col, val, bh, para=opara, rbar0=sh) if sh is not None else port.csolve(sid, rp, col, val, bh, para=opara)
                tag = (n, sid, "b = 0" if not bh.any() else "b", info.ret, info.iterations, ref["ret"], ref["iters"])
                if n == 1 and sid == po.CLCG_TFQMR and bh.any():
                    assert ref["ret"] == -1019 and not np.all(np.isfinite(ref["x"])), tag       # the reference's 0 / 0
                    assert info.ret == 0 and abs(x[0] - xt[0]) <= 1e-14 * abs(xt[0]), tag
                    continue
                assert info.ret == ref["ret"] and abs(info.iterations - ref["iters"]) <= 2, tag
                assert np.linalg.norm(x - ref["x"]) <= 5e-5 * max(1.0, np.linalg.norm(ref["x"])), tag
        A.destroy()
