"""-m gpu: the batched BiCGStab (lcg_hip_lbicgstab_multi) and the product carrying two sums (lcg_hip_spmm_dot2) on the systems of
tests/multi_bicg_cases.py, every column against the oracle's lbicgstab on that column alone (plain) or against the helper's numpy
restatement of the x-space loop with the checkers' applies (preconditioned).

Bands.  Capped at 8 iterations: test_gpu_multi_solvers.py's band -- code and count equal; |m_j - x| <= max(1e-9, 50 x the reference
run's own response to 1-ulp changes of b at that count) |x|; the reported residual within 1e-9 relative.  (The bands' 1e-6 b column
stops at 3 iterations under the absolute rule: it is compared in a run capped at 2.)  Converged: conftest.check_converged_run's
statement for the rounding-sensitive loops (wide=True) per column, and the host's own residual of the returned column
(multi_cases.host_residual, extended precision) meets epsilon within multi_cases.rounding_floor.

Tiny systems (n = 1, 2, 3): only kernel edges are asserted.  BiCGStab finishes such systems by an exact half step, and whether the
0 / 0 that follows ends as LCG_NAN_VALUE (the oracle does at n = 1) or as a converged step is decided by one rounding of
s = r - ak v, fused or not."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import multi_bicg_cases as bc
import multi_cases as mc
import tri_multi_cases as tm
from conftest import check_converged_run
from multi_bicg_cases import ALREADY, BADEPS, BADIT, CONV, E_ARG, MAXIT, M_IC0, M_ILU0, M_JACOBI, M_NONE, NANV, NOPRE, bicg, bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KS = bc.KS
CAP = bc.CAP


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


_HANDLES = {}


@pytest.fixture(scope="module")
def handle(api):
    """(kind, n) -> the system's handle (kept for the module)."""
    def get(key):
        if key not in _HANDLES:
            S = bc.system(*key)
            _HANDLES[key] = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
        return _HANDLES[key]
    yield get
    for A in _HANDLES.values():
        A.destroy()
    _HANDLES.clear()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------ 1. lcg_hip_spmm_dot2
def _dot2(lib, A, k, Xd, Ud, n):
    Y = torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")
    out = (C.c_double * (2 * k))()
    assert lib.lcg_hip_spmm_dot2(A.h, k, Xd.data_ptr(), Y.data_ptr(), Ud.data_ptr(), out) == 0, lib.lcg_hip_last_error()
    return Y.cpu().numpy(), list(out)


@pytest.mark.parametrize("key", [("nonsym", 513), ("nonsym", 32771), ("band30", 1029), ("band140", 2051)], ids=bc.sys_id)
def test_product_carrying_two_sums(api, lib, handle, key):
    S = bc.system(*key)
    A, n = handle(key), S["n"]
    rng = np.random.default_rng(11)
    col0 = {}
    for k in KS:
        Xh = rng.standard_normal((n, k)); Uh = rng.standard_normal((n, k)) * 2.0 ** rng.uniform(-10, 10, (n, 1))
        if col0:
            Xh[:, 0], Uh[:, 0] = col0["x"], col0["u"]
        Xd, Ud = dev(Xh), dev(Uh)
        Yh, d2 = _dot2(lib, A, k, Xd, Ud, n)
        Yp = torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")
        assert lib.lcg_hip_spmm(A.h, k, Xd.data_ptr(), Yp.data_ptr()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(bits(Yh), bits(Yp.cpu().numpy()))                 # Y: the plain product's bits
        d1 = (C.c_double * k)()
        assert lib.lcg_hip_spmm_dot(A.h, k, Xd.data_ptr(), Yp.data_ptr(), Ud.data_ptr(), d1) == 0
        assert np.array_equal(bits(np.array(d2[:k])), bits(np.array(list(d1))))  # Y.U: lcg_hip_spmm_dot's bits
        for j in range(k):
            yj = np.ascontiguousarray(Yh[:, j])
            X.assert_dot(d2[k + j], yj, yj, (key, k, j, "Y.Y"))
        # column 0's two sums: the same whatever the others hold (NaN and Inf included), from call to call, whatever k is
        X2, U2 = Xh.copy(), Uh.copy()
        X2[:, 1:] = rng.standard_normal((n, k - 1)) * 1e3; U2[:, 1:] = 0.0
        X2[n // 2, 1] = np.nan; U2[0, k - 1] = np.inf; X2[n - 1, k - 1] = -np.inf
        _, e2 = _dot2(lib, A, k, dev(X2), dev(U2), n)
        _, f2 = _dot2(lib, A, k, Xd, Ud, n)
        assert (e2[0], e2[k]) == (d2[0], d2[k]) and np.array_equal(bits(np.array(f2)), bits(np.array(d2)))
        if not col0:
            col0 = {"x": Xh[:, 0].copy(), "u": Uh[:, 0].copy(), "sums": (d2[0], d2[k])}
        assert (d2[0], d2[k]) == col0["sums"], (k, d2[0], d2[k], col0["sums"])


def test_product_error_returns_leave_y_alone(api, lib, handle):
    key = ("nonsym", 513)
    A, n = handle(key), 513
    rng = np.random.default_rng(9)
    Xd = dev(rng.standard_normal((n, 4))); Y = torch.full((n, 4), 7.0, dtype=torch.float64, device="cuda")
    out = (C.c_double * 8)()
    S = bc.system(*key)
    Ac = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"] + 1j * S["v"])
    D = api.DenseMatrix.from_array(rng.standard_normal((8, 8)))
    calls = [("k", lambda: lib.lcg_hip_spmm_dot2(A.h, 3, Xd.data_ptr(), Y.data_ptr(), Xd.data_ptr(), out)),
             ("null pointer", lambda: lib.lcg_hip_spmm_dot2(A.h, 4, Xd.data_ptr(), Y.data_ptr(), None, out)),
             ("aligned", lambda: lib.lcg_hip_spmm_dot2(A.h, 4, Xd.data_ptr() + 8, Y.data_ptr(), Xd.data_ptr(), out)),
             ("aligned", lambda: lib.lcg_hip_spmm_dot2(A.h, 4, Xd.data_ptr(), Y.data_ptr(), Xd.data_ptr() + 8, out)),
             ("null pointer", lambda: lib.lcg_hip_spmm_dot2(A.h, 4, Xd.data_ptr(), Y.data_ptr(), Xd.data_ptr(), None)),
             ("complex", lambda: lib.lcg_hip_spmm_dot2(Ac.h, 4, Xd.data_ptr(), Y.data_ptr(), Xd.data_ptr(), out)),
             ("dense", lambda: lib.lcg_hip_spmm_dot2(D.h, 4, Xd.data_ptr(), Y.data_ptr(), Xd.data_ptr(), out))]
    for what, call in calls:
        assert call() == E_ARG, what
        assert what in lib.lcg_hip_last_error().decode(), (what, lib.lcg_hip_last_error())
        torch.cuda.synchronize()
        assert bool((Y == 7.0).all()), what
    Ac.destroy(); D.destroy()


# ------------------------------------------------------------------------------------------------------------ 2. capped, plain
def _compare_capped(S, ref, sens, ret, its, res, mj, j, tag):
    print("  ", tag, j, "ret", ret, ref["ret"], "its", its, ref["iters"], "residual", res, ref["residual"])
    assert ret == ref["ret"] and its == ref["iters"], (tag, j, ret, ref["ret"], its, ref["iters"])
    nx = np.linalg.norm(ref["x"])
    d = np.linalg.norm(mj - ref["x"]) / nx
    print("      distance", d, "reference run's response", sens)
    assert d <= max(1e-9, 50.0 * sens), (tag, j, d, sens)
    assert abs(res - ref["residual"]) <= 1e-9 * ref["residual"], (tag, j, res, ref["residual"])


@pytest.mark.parametrize("rule", sorted(bc.RULES))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("key", bc.NON_TINY, ids=bc.sys_id)
def test_capped_at_8_iterations(lib, api, port, handle, key, k, rule):
    S = bc.system(*key)
    A, n = handle(key), S["n"]
    B = bc.columns(n, S["b"], k)
    M0 = np.zeros((n, k))
    zero = [j for j in range(k) if not B[:, j].any()]
    for j in zero:
        M0[:, j] = -0.0
    short = 1 if key[0].startswith("band") and rule == "abs" else None     # (module docstring)
    for cap, cols in ((CAP, [j for j in range(k) if j != short]), (2, [short] if short is not None else [])):
        if not cols:
            continue
        para = dict(max_iterations=cap, **bc.RULES[rule])
        rc, ret, its, res, M = bicg(lib, api, M_NONE, A, M0, B, **para)
        assert rc == 0, lib.lcg_hip_last_error()
        for j in cols:
            if j in zero:
                assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))      # the sign bit too
                continue
            run = lambda b, tag: bc.oracle_column(port, S, b, tag, **para)
            ref = run(B[:, j], ("col", j))
            _compare_capped(S, ref, bc.response(run, B[:, j], (j,)), ret[j], its[j], res[j], M[:, j], j, (key, k, rule, cap))
        if cap == CAP:
            assert lib.lcg_hip_last_iterations() == max(its)


# ------------------------------------------------------------------------------------------------------------ 3. converged, plain
_CACHES = {}


@pytest.mark.parametrize("rule", sorted(bc.RULES))
@pytest.mark.parametrize("k", (4, 8))
@pytest.mark.parametrize("key", [("nonsym", 513), ("nonsym", 32771), bc.CONVDIFF], ids=bc.sys_id)
def test_converged_columns(lib, api, port, handle, key, k, rule):
    S = bc.system(*key)
    A, n = handle(key), S["n"]
    B = bc.columns(n, S["b"], k)
    sols = mc.solutions(S["xt"], k)
    para = bc.RULES[rule]
    eps, abs_diff = para["epsilon"], para["abs_diff"]
    rc, ret, its, res, M = bicg(lib, api, M_NONE, A, np.zeros((n, k)), B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    print(key, k, rule, "ret", ret, "its", its)
    for j in range(k):
        if not B[:, j].any():
            assert ret[j] == ALREADY and its[j] == 0 and not M[:, j].any()
            continue
        check_converged_run(port, lambda cap: (ret[j], its[j], res[j], M[:, j]), bc.BICGSTAB, S["rp"], S["ci"], S["v"], B[:, j], eps, abs_diff,
                            tag=(key, k, rule, j), wide=True, xt=sols[j], cache=_CACHES.setdefault((key, rule, j), {}))
        host, g2, m2 = bc.host_residual(S, M[:, j], B[:, j], abs_diff)
        floor = bc.rounding_floor(S, M[:, j], B[:, j], abs_diff)
        print("   column", j, "its", its[j], "reported", res[j], "host residual", host, "rounding floor", floor)
        assert host <= eps + floor, (j, host, eps, floor)
    longest = int(np.argmax(its))
    assert lib.lcg_hip_last_iterations() == its[longest] and lib.lcg_hip_last_residual() == res[longest]


# ------------------------------------------------------------------------------------------------------------ 4. preconditioned
PRE = {"ilu0": (M_ILU0, 0), "ilu0_s2": (M_ILU0, 2), "ilu0_s4": (M_ILU0, 4), "jacobi": (M_JACOBI, 0)}


def _restated_apply(S, name):
    if name == "jacobi":
        return bc.jacobi_apply(S)
    return tm.checker_apply("ilu0", S["key"], S["n"], S["rp"], S["ci"], S["v"], PRE[name][1])


@pytest.fixture(scope="module")
def convdiff_pre(api):
    S = bc.system(*bc.CONVDIFF)
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    A.build_ilu0(); A.build_jacobi()
    yield S, A
    A.destroy()


def _set(A, name):
    A.ilu0_set_sweeps(PRE[name][1])
    return PRE[name][0]


@pytest.mark.parametrize("name", sorted(PRE))
def test_preconditioned_capped_at_8(lib, api, convdiff_pre, name):
    S, A = convdiff_pre
    n, k = S["n"], 4
    B = bc.columns(n, S["b"], k)
    apply = _restated_apply(S, name)
    para = dict(max_iterations=CAP, **bc.RULES["abs"])
    rc, ret, its, res, M = bicg(lib, api, _set(A, name), A, np.zeros((n, k)), B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        if not B[:, j].any():
            assert ret[j] == ALREADY and its[j] == 0 and not M[:, j].any()
            continue
        run = lambda b, tag: bc.restated_column(S, name, apply, b, tag, **para)
        ref = run(B[:, j], ("col", j))
        _compare_capped(S, ref, bc.response(run, B[:, j], (j,)), ret[j], its[j], res[j], M[:, j], j, (name, "cap", CAP))


def test_preconditioned_converged(lib, api, convdiff_pre):
    S, A = convdiff_pre
    n, k = S["n"], 4
    B = bc.columns(n, S["b"], k)
    para = dict(abs_diff=1, epsilon=1e-10)
    counts = {}
    for name in [None] + sorted(PRE):
        if name is None:
            precond, apply = M_NONE, None
        else:
            precond, apply = _set(A, name), _restated_apply(S, name)
        rc, ret, its, res, M = bicg(lib, api, precond, A, np.zeros((n, k)), B, **para)
        assert rc == 0, lib.lcg_hip_last_error()
        print(name, "ret", ret, "its", its)
        counts[name] = its
        for j in (0, 1, 2):
            ref = bc.restated_column(S, name or "plain", apply, B[:, j], ("col", j), **para)
            dit = max(abs(bc.restated_column(S, name or "plain", apply, bc.perturbed(B[:, j], s), ("pert", s, j), **para)["iters"] - ref["iters"])
                      for s in range(2))
            assert ret[j] == ref["ret"] == CONV and res[j] <= para["epsilon"]
            band = max(3, 4 * dit, 0.3 * ref["iters"])                  # conftest.check_converged_run, wide
            assert abs(its[j] - ref["iters"]) <= band, (name, j, its[j], ref["iters"], dit)
            host, _, _ = bc.host_residual(S, M[:, j], B[:, j], 1)
            floor = bc.rounding_floor(S, M[:, j], B[:, j], 1)
            print("   column", j, "its", its[j], "restated", ref["iters"], "host residual", host, "floor", floor)
            assert host <= para["epsilon"] + floor, (name, j, host)
        assert ret[3] == ALREADY and its[3] == 0
    for j in (0, 1, 2):         # test_gpu_ilu0.py::test_right_bicgstab's statements
        assert 2 * counts["ilu0"][j] <= counts[None][j], (j, counts)
        assert counts["ilu0_s4"][j] < counts[None][j], (j, counts)


def test_preconditioned_from_a_block_of_guesses(lib, api):
    """The x-space form needs no final apply: from non-zero guesses the converged m itself solves the system."""
    S = bc.system("nonsym", 513)
    n, k = S["n"], 4
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    A.build_ilu0(); A.build_jacobi()
    B = bc.columns(n, S["b"], k)
    M0 = bc.guesses(S, k)
    para = dict(abs_diff=1, epsilon=1e-10)
    for precond, sweeps in ((M_ILU0, 0), (M_ILU0, 2), (M_JACOBI, 0)):
        A.ilu0_set_sweeps(sweeps)
        rc, ret, its, res, M = bicg(lib, api, precond, A, M0, B, **para)
        assert rc == 0, lib.lcg_hip_last_error()
        print(precond, sweeps, "ret", ret, "its", its)
        for j in range(k):
            assert ret[j] == CONV and its[j] > 0 and res[j] <= para["epsilon"], (precond, sweeps, j, ret[j], its[j])
            host, _, _ = bc.host_residual(S, M[:, j], B[:, j], 1)
            assert host <= para["epsilon"] + bc.rounding_floor(S, M[:, j], B[:, j], 1), (precond, sweeps, j, host)
    A.destroy()


def test_ic0_on_an_spd_system_and_missing_preconditioners(lib, api):
    S = mc.system("spd", 513)
    n, k = S["n"], 4
    B = bc.columns(n, S["b"], k)
    para = dict(abs_diff=1, epsilon=1e-10)
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    for precond in (M_JACOBI, M_IC0, M_ILU0):
        r = bicg(lib, api, precond, A, np.zeros((n, k)), B, **para)
        assert r[0] == NOPRE and r[1] == [99] * k and r[2] == [-1] * k and not r[4].any()       # nothing ran, nothing was reported
    plain = bicg(lib, api, M_NONE, A, np.zeros((n, k)), B, **para)
    assert plain[0] == 0 and plain[1] == [CONV, CONV, CONV, ALREADY]
    A.build_ic0()
    rc, ret, its, res, M = bicg(lib, api, M_IC0, A, np.zeros((n, k)), B, **para)
    assert rc == 0 and ret == [CONV, CONV, CONV, ALREADY], (rc, ret)
    print("IC(0)", its, "plain", plain[2])
    for j in (0, 1, 2):
        assert its[j] < plain[2][j]
        host, _, _ = bc.host_residual(S, M[:, j], B[:, j], 1)
        assert host <= para["epsilon"] + bc.rounding_floor(S, M[:, j], B[:, j], 1), (j, host)
    assert bicg(lib, api, M_ILU0, A, np.zeros((n, k)), B, **para)[0] == NOPRE                   # IC(0) is not ILU(0)
    A.destroy()


# ------------------------------------------------------------------------------------------------------------ 5. a batch is a batch
BATCH = {"plain-513": (("nonsym", 513), M_NONE, 0), "ilu0_s2-513": (("nonsym", 513), M_ILU0, 2), "plain-32771": (("nonsym", 32771), M_NONE, 0)}


@pytest.fixture(scope="module")
def batch_handle(api):
    made = {}

    def get(name):
        if name not in made:
            key, precond, sweeps = BATCH[name]
            S = bc.system(*key)
            A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
            if precond == M_ILU0:
                A.build_ilu0(); A.ilu0_set_sweeps(sweeps)
            made[name] = (S, A, precond)
        return made[name]
    yield get
    for _, A, _ in made.values():
        A.destroy()


@pytest.mark.parametrize("name", sorted(BATCH))
def test_verdicts_differ_and_stopped_columns_are_final(lib, api, batch_handle, name):
    S, A, precond = batch_handle(name)
    n, k = S["n"], 4
    B = bc.columns(n, S["b"], k)
    para = dict(epsilon=1e-10, abs_diff=1)
    Z = np.zeros((n, k))
    rc, ret, its, res, M = bicg(lib, api, precond, A, Z, B, **para)
    assert rc == 0 and ret[0] == ret[1] == CONV, (rc, ret)
    t_fast, t_slow = its[1], its[0]
    print(name, "counts", its)
    assert 0 < t_fast and t_fast + 2 <= t_slow, its
    cap = (t_fast + t_slow) // 2
    rc, ret_c, its_c, res_c, M_c = bicg(lib, api, precond, A, Z, B, max_iterations=cap, **para)
    assert rc == 0
    assert ret_c[1] == CONV and its_c[1] == t_fast and ret_c[0] == MAXIT and its_c[0] == cap and ret_c[3] == ALREADY and its_c[3] == 0
    assert np.array_equal(bits(M_c[:, 1]), bits(M[:, 1])) and res_c[1] == res[1]
    # frozen means final: the column that stopped at t_fast while the others went on = the same batch capped at t_fast
    rc, ret_f, its_f, res_f, M_f = bicg(lib, api, precond, A, Z, B, max_iterations=t_fast, **para)
    assert rc == 0 and ret_f[1] == CONV and its_f[1] == t_fast and ret_f[0] == MAXIT and its_f[0] == t_fast
    assert np.array_equal(bits(M_f[:, 1]), bits(M[:, 1])) and res_f[1] == res[1]


@pytest.mark.parametrize("name", sorted(BATCH))
def test_a_nan_stays_in_its_column(lib, api, batch_handle, name):
    S, A, precond = batch_handle(name)
    n = S["n"]
    for k in (4, 8):
        B = bc.columns(n, S["b"], k)
        para = dict(epsilon=1e-10, abs_diff=1, max_iterations=60)
        rc, ret, its, res, M = bicg(lib, api, precond, A, np.zeros((n, k)), B, **para)
        Bn = B.copy(); Bn[n // 2, 1] = np.nan
        rc_n, ret_n, its_n, res_n, M_n = bicg(lib, api, precond, A, np.zeros((n, k)), Bn, **para)
        assert rc == 0 and rc_n == 0
        assert ret_n[1] == NANV and its_n[1] == 1, (ret_n, its_n)
        for j in range(k):
            if j == 1:
                continue
            assert ret_n[j] == ret[j] and its_n[j] == its[j] and res_n[j] == res[j], j
            assert np.array_equal(bits(M_n[:, j]), bits(M[:, j])), j
            assert np.isfinite(M_n[:, j]).all()


@pytest.mark.parametrize("name", sorted(BATCH))
def test_independence_and_repeatability(lib, api, batch_handle, name):
    S, A, precond = batch_handle(name)
    n, k = S["n"], 4
    B = bc.columns(n, S["b"], k)
    para = dict(epsilon=1e-10, abs_diff=1, max_iterations=12)
    Z = np.zeros((n, k))
    r1 = bicg(lib, api, precond, A, Z, B, **para)
    r2 = bicg(lib, api, precond, A, Z, B, **para)
    r3 = bicg(lib, api, precond, A, Z, B, mem="host", **para)
    for r in (r2, r3):
        assert r[0] == r1[0] == 0 and r[1:4] == r1[1:4]
        assert np.array_equal(bits(r[4]), bits(r1[4]))
    B2 = B.copy()
    rng = np.random.default_rng(8)
    B2[:, 1] = rng.standard_normal(n) * 1e3; B2[:, 2] = 0.0; B2[:, 3] = 1e-6 * S["b"]
    M2 = np.zeros((n, k)); M2[:, 1] = rng.standard_normal(n); M2[:, 3] = 0.5 * S["xt"]
    r4 = bicg(lib, api, precond, A, M2, B2, **para)
    assert r4[0] == 0 and (r4[1][0], r4[2][0], r4[3][0]) == (r1[1][0], r1[2][0], r1[3][0])
    assert np.array_equal(bits(r4[4][:, 0]), bits(r1[4][:, 0]))
    # column j among 8 = column j among 4 where both hold the same data
    r8 = bicg(lib, api, precond, A, np.zeros((n, 8)), bc.columns(n, S["b"], 8), **para)
    assert r8[0] == 0
    for j in range(k):
        assert (r8[1][j], r8[2][j], r8[3][j]) == (r1[1][j], r1[2][j], r1[3][j]), j
        assert np.array_equal(bits(r8[4][:, j]), bits(r1[4][:, j])), j


# ------------------------------------------------------------------------------------------------------------ 6. tiny systems
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", (1, 2, 3))
def test_tiny_systems(lib, api, port, n, k):
    S = bc.system("tiny", n)
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    B = bc.columns(n, S["b"], k)
    for rule, para in bc.RULES.items():
        M0 = np.zeros((n, k))
        for j in range(k):
            if not B[:, j].any():
                M0[:, j] = -0.0
        rc, ret, its, res, M = bicg(lib, api, M_NONE, A, M0, B, **para)
        assert rc == 0, lib.lcg_hip_last_error()
        print(n, k, rule, "ret", ret, "its", its)
        for j in range(k):
            assert ret[j] in (CONV, ALREADY, NANV, MAXIT), (j, ret[j])
            ref = bc.oracle_column(port, S, B[:, j], ("col", j), **para)
            if ref["ret"] == ALREADY:       # zero columns and columns "already optimised": as the oracle's, untouched
                assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j])), (j, ret[j], its[j])
            else:
                assert ret[j] != ALREADY and its[j] >= 1, (j, ret[j], its[j])
            if ret[j] == CONV:
                host, _, _ = bc.host_residual(S, M[:, j], B[:, j], para["abs_diff"])
                assert host <= para["epsilon"] + bc.rounding_floor(S, M[:, j], B[:, j], para["abs_diff"]), (j, host)
            if ret[j] != NANV:
                assert np.isfinite(M[:, j]).all() and np.isfinite(res[j]), j
        again = bicg(lib, api, M_NONE, A, M0, B, **para)
        assert again[0] == 0 and list(again[1:3]) == [ret, its]
        assert np.array_equal(bits(np.array(again[3])), bits(np.array(res))) and np.array_equal(bits(again[4]), bits(M))
    A.destroy()


# ------------------------------------------------------------------------------------------------------------ 7. error returns
def test_error_returns_release_the_solver(lib, api, handle):
    key = ("nonsym", 513)
    S = bc.system(*key)
    A, n, k = handle(key), S["n"], 4
    B = bc.columns(n, S["b"], k)
    good = dict(epsilon=1e-10, abs_diff=1, max_iterations=10)
    Z = np.zeros((n, k))
    ref = bicg(lib, api, M_NONE, A, Z, B, **good)
    assert ref[0] == 0
    bd = dev(S["b"])

    def single():
        m = torch.zeros(n, dtype=torch.float64, device="cuda")
        info = api.lcg_solver("lcg_hip_csr_ax", None, m, bd, n, api.lcg_default_parameters(**good), A, api.LCG_BICGSTAB)
        torch.cuda.synchronize()
        return info.ret, info.iterations, info.residual, m.cpu().numpy()

    ref1 = single()
    assert ref1[0] == MAXIT and ref1[1] == 10

    def still_works():
        r = bicg(lib, api, M_NONE, A, Z, B, **good)
        assert r[0] == 0 and r[1:4] == ref[1:4] and np.array_equal(bits(r[4]), bits(ref[4]))
        s = single()
        assert s[:3] == ref1[:3] and np.array_equal(bits(s[3]), bits(ref1[3]))

    p = api.lcg_default_parameters(**good)
    Md, Bd = dev(Z), dev(B)
    M8 = torch.zeros(n * 8 + 2, dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(2)
    Ac = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"] + 1j * S["v"])
    D = api.DenseMatrix.from_array(rng.standard_normal((n, n)))
    R = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"], n_cols=2 * n)

    def raw(h, kk, precond, mptr):
        return lib.lcg_hip_lbicgstab_multi(h, kk, precond, mptr, Bd.data_ptr(), C.byref(p), None, None, None, 1)

    for what, call in (("bad k", lambda: raw(A.h, 3, M_NONE, Md.data_ptr())),
                       ("misaligned M", lambda: raw(A.h, k, M_NONE, M8.data_ptr() + 8)),
                       ("complex handle", lambda: raw(Ac.h, k, M_NONE, Md.data_ptr())),
                       ("dense handle", lambda: raw(D.h, k, M_NONE, Md.data_ptr())),
                       ("non-square", lambda: raw(R.h, k, M_NONE, Md.data_ptr())),
                       ("precond = 7", lambda: raw(A.h, k, 7, Md.data_ptr()))):
        assert call() == E_ARG, what
        assert lib.lcg_hip_last_error(), what
        still_works()
    torch.cuda.synchronize()
    assert not Md.cpu().numpy().any()
    for para, code in ((dict(epsilon=0.0), BADEPS), (dict(epsilon=1.0), BADEPS), (dict(max_iterations=-1), BADIT)):
        for precond in (M_NONE, M_JACOBI):
            r = bicg(lib, api, precond, A, Z, B, **para)
            assert r[0] == code and r[1] == [99] * k, (para, precond, r[0])
        still_works()
    for M in (Ac, D, R):
        M.destroy()


# ------------------------------------------------------------------------------------------------------------ 8. front and sample
def test_python_front(api, convdiff_pre):
    S, A = convdiff_pre
    n = S["n"]
    Bh = bc.columns(n, S["b"], 4)
    B = dev(Bh)
    para = api.lcg_default_parameters(epsilon=1e-10, abs_diff=1)
    M = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    infos = api.lbicgstab_multi(A, M, B, para)
    assert [i.ret for i in infos] == [CONV, CONV, CONV, ALREADY] and infos[3].iterations == 0
    A.ilu0_set_sweeps(0)
    Mi = torch.zeros_like(M)
    infos_i = api.lbicgstab_multi(A, Mi, B, para, precond="ilu0")
    assert [i.ret for i in infos_i] == [CONV, CONV, CONV, ALREADY]
    assert all(2 * infos_i[j].iterations <= infos[j].iterations for j in range(3))
    Y = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda")
    sums = A.spmm_dot2(Mi, Y, B)
    r = (Y - B).cpu().numpy()
    assert np.linalg.norm(r[:, 0]) / n <= 2e-10
    Yh = Y.cpu().numpy()
    assert np.allclose(sums[:4], np.einsum("ij,ij->j", Yh, Bh), rtol=1e-12) and np.allclose(sums[4:], np.einsum("ij,ij->j", Yh, Yh), rtol=1e-12)
    Mh = np.zeros((n, 4))
    infos_h = api.lbicgstab_multi(A, Mh, Bh, para, precond="jacobi")
    assert [i.ret for i in infos_h] == [CONV, CONV, CONV, ALREADY]
    assert np.linalg.norm(Mh[:, 0] - Mi[:, 0].cpu().numpy()) <= 1e-7 * np.linalg.norm(Mh[:, 0])
    with pytest.raises(ValueError):
        api.lbicgstab_multi(A, Mh, Bh, para, precond="ssor")


def test_sample_program_solves_four_right_hand_sides_plain_and_with_ilu0():
    import re
    import subprocess
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_bicgstab")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = re.findall(r"^(plain|ilu0) column (\d): ret=(-?\d+) iterations=(\d+)", p.stdout, flags=re.M)
    assert [(w, int(j), int(r)) for w, j, r, _ in got] == [(w, j, ALREADY if j == 3 else CONV) for w in ("plain", "ilu0") for j in range(4)]
    its = {(w, int(j)): int(t) for w, j, _, t in got}
    for j in range(3):
        assert its[("ilu0", j)] < its[("plain", j)], its
    assert its[("plain", 3)] == its[("ilu0", 3)] == 0
