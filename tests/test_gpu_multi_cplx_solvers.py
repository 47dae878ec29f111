"""-m gpu: the batched complex loops (clcg_hip_lbicg_sym_multi, clcg_hip_lpcg_multi) for k = 2, 4, 8, every column against the
oracle's run of that column alone (orc_clbicg_symmetric, orc_clpcg); then what makes a batch a batch: different verdicts in one
call, a NaN that stays in its column, stopped columns that are final, columns that do not depend on their neighbours or on k, and
the error returns.  Systems, columns and the driver: tests/multi_cplx_cases.py (tests/test_multi_cplx_cases_cpu.py shows with the
oracle alone that each case reaches the branch its id names).

Bands.  Capped at 6 and 25 iterations (epsilon = 1e-20): codes and counts equal the oracle's; the iterate within max(1e-13, 50 x the
oracle's own response to 1-ulp changes of b at that count) of the oracle's, relative to |x| -- the recurrence IS the oracle's, 50 is
the project's factor, the response is measured here (a zero column that starts from a non-zero guess: 1-ulp changes of the guess); the reported residual within 1e-9 relative.  Converged (abs_diff = 1,
epsilon = 1e-10, helm40): conftest.check_converged_run's rules 1 and 2 -- code 0, the count within max(3, 3 x the oracle's own
spread under 1-ulp changes of b, 5 %), the reported residual <= epsilon, the distance to x_true within 10 x the oracle's."""
import numpy as np
import pytest

import multi_cplx_cases as cc
from multi_cplx_cases import ALREADY, BADEPS, BADMAXIT, BICG_SYM, CONV, E_ARG, KS, MAXIT, NANV, NOPRE, PCG, SIDS, bits, cmulti

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


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
    """handle(kind, n) -> (S, CsrMatrix with its Jacobi diagonal), kept for the module."""
    def get(kind, n=0):
        if (kind, n) not in _HANDLES:
            S = cc.system(kind, n)
            A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
            A.build_jacobi()
            _HANDLES[(kind, n)] = (S, A)
        return _HANDLES[(kind, n)]
    yield get
    for _, A in _HANDLES.values():
        A.destroy()
    _HANDLES.clear()


def check_capped(lib, api, port, S, A, sid, k, cap, M0=None, tag="zero"):
    n = S["n"]
    B = cc.columns(n, S["b"], k)
    para = dict(epsilon=1e-20, max_iterations=cap)
    M0 = np.zeros((n, k), np.complex128) if M0 is None else M0
    rc, ret, its, res, M = cmulti(lib, api, sid, A, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        m0 = M0[:, j].copy()
        ref = cc.oracle_column(port, S, sid, B[:, j], ("col", tag, j), m0=m0, **para)
        print(S["key"], sid, k, j, "ret", ret[j], ref["ret"], "its", its[j], ref["iters"])
        assert ret[j] == ref["ret"] and its[j] == ref["iters"], (j, ret[j], ref["ret"], its[j], ref["iters"])
        if ret[j] == ALREADY:
            assert its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            continue
        nx = np.linalg.norm(ref["x"])
        # (a zero column that starts from a non-zero guess has no b to move by an ulp: its only input, the guess, is moved instead)
        moved = [(cc.ulp_changes(B[:, j], s), m0) if B[:, j].any() else (B[:, j], cc.ulp_changes(m0, s)) for s in range(2)]
        sens = max(np.linalg.norm(cc.oracle_column(port, S, sid, bp, ("pert", tag, j, s), m0=mp, **para)["x"] - ref["x"]) / nx
                   for s, (bp, mp) in enumerate(moved))
        d = np.linalg.norm(M[:, j] - ref["x"]) / nx
        print("   distance", d, "oracle's response", sens, "residual", res[j], ref["residual"])
        assert d <= max(1e-13, 50.0 * sens), (j, d, sens)
        if ref["residual"] > 1e-25:          # (n <= 3: converged to rounding, the residual is rounding itself)
            assert abs(res[j] - ref["residual"]) <= 1e-9 * ref["residual"], (j, res[j], ref["residual"])
    return ret, its


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", SIDS)
@pytest.mark.parametrize("cap", [6, 25])
def test_capped_runs_on_helm40(lib, api, port, handle, cap, sid, k):
    S, A = handle(*cc.HELM40)
    ret, its = check_capped(lib, api, port, S, A, sid, k, cap)
    assert ret[0] == MAXIT and its[0] == cap
    if k >= 4:
        assert ret[3] == ALREADY
    assert lib.lcg_hip_last_iterations() == cap


@pytest.mark.parametrize("sid", SIDS)
@pytest.mark.parametrize("case", sorted(cc.EDGE_CASES), ids=lambda c: cc.EDGE_IDS[c])
def test_edges_capped_at_6(lib, api, port, handle, case, sid):
    """Size edges n = 1, 2, 3, 65, 513; R = 64, 16, 4 with a partial last block; more than 512 row blocks at each class (the folded
    d.Ad inside the loop); a second and third stride of a vector pass; n k >= 2^20; the golden case_1K_cA."""
    kind, n, k = case
    S, A = handle(kind, n)
    check_capped(lib, api, port, S, A, sid, k, 6)


@pytest.mark.parametrize("sid", SIDS)
def test_non_zero_guesses(lib, api, port, handle, sid):
    S, A = handle(*cc.HELM40)
    for k in KS:
        check_capped(lib, api, port, S, A, sid, k, 6, M0=cc.guesses(S, k), tag="guess")
    S, A = handle("band30", 1029)
    check_capped(lib, api, port, S, A, sid, 4, 6, M0=cc.guesses(S, 4), tag="guess")


_SPREAD = {}


def converged_column(port, S, sid, b, tag, got, xt, eps, abs_diff):
    """check_converged_run's rules 1 and 2 for one column: got = (ret, iterations, residual, x)."""
    para = dict(epsilon=eps, abs_diff=abs_diff)
    ref = cc.oracle_column(port, S, sid, b, ("conv", tag), **para)
    key = (S["key"], sid, tag, eps, abs_diff)
    if key not in _SPREAD:
        _SPREAD[key] = max(abs(cc.oracle_column(port, S, sid, cc.ulp_changes(b, s), ("convpert", tag, s), **para)["iters"] - ref["iters"])
                           for s in range(2))
    dit = _SPREAD[key]
    ret, its, res, x = got
    print(S["key"], sid, tag, "ret", ret, ref["ret"], "its", its, ref["iters"], "spread", dit, "residual", res)
    assert ret == ref["ret"] == CONV, (tag, ret, ref["ret"])
    assert abs(its - ref["iters"]) <= max(3, 3 * dit, 0.05 * ref["iters"]), (tag, its, ref["iters"], dit)
    assert res <= eps, (tag, res)
    if xt is not None:
        e_gpu, e_ref = np.linalg.norm(x - xt), np.linalg.norm(ref["x"] - xt)
        print("   distance to x_true", e_gpu, "oracle's", e_ref)
        assert e_gpu <= 10.0 * max(e_ref, 1e-14 * np.linalg.norm(xt)), (tag, e_gpu, e_ref)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", SIDS)
@pytest.mark.parametrize("rule", ["abs", "rel"])
def test_converged_columns_match_the_oracle(lib, api, port, handle, rule, sid, k):
    """abs: abs_diff = 1, epsilon = 1e-10.  rel: the relative rule, one column with |m|^2 far above 1 and one (1e-2 b) below it, where
    the clamp decides."""
    S, A = handle(*cc.HELM40)
    n, xt = S["n"], S["xt"]
    B = cc.columns(n, S["b"], k)
    eps, ad = 1e-10, int(rule == "abs")
    M0 = np.zeros((n, k), np.complex128)
    zero = [j for j in range(k) if not B[:, j].any()]
    for j in zero:
        M0[:, j] = -0.0 - 0.0j      # a guess of zeros that shows a write
    rc, ret, its, res, M = cmulti(lib, api, sid, A, M0, B, epsilon=eps, abs_diff=ad)
    assert rc == 0, lib.lcg_hip_last_error()
    sols = [xt, cc.SMALL * xt, None, None, -xt, None, 0.5 * xt, 2.0 * xt]
    for j in range(k):
        if j in zero:
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            continue
        converged_column(port, S, sid, B[:, j], ("col", j), (ret[j], its[j], res[j], M[:, j]), sols[j], eps, ad)
    if rule == "rel":
        assert np.linalg.norm(M[:, 0]) ** 2 > 100.0 and np.linalg.norm(M[:, 1]) ** 2 < 1.0
    longest = int(np.argmax(its))
    assert lib.lcg_hip_last_iterations() == its[longest] and lib.lcg_hip_last_residual() == res[longest]


def rounding_floor(S, m, b, sid):
    """The abs_diff residual that rounding alone can leave where b - A.m is exactly zero: every row of r within exact_ref's c128 row
    bound sqrt(2) gamma(2 L + 4) (|A||m| + |b|), through the loop's own formula (BiCG-sym: sum |r|^2 / n; PCG: sqrt(sum |r|^2) / n)."""
    import exact_ref as X
    absax = np.abs(S["A"]) @ np.abs(m)
    g = np.sqrt(2.0) * X.gamma(2 * X.lengths(S["rp"]) + 4) * (absax + np.abs(b))
    r2 = float(g @ g)
    return r2 / S["n"] if sid == BICG_SYM else np.sqrt(r2) / S["n"]


@pytest.mark.parametrize("sid", SIDS)
def test_both_already_optimised_criteria(lib, api, port, handle, sid):
    S, A = handle(*cc.HELM40)
    M0, B = cc.already_batch(S)
    para = dict(epsilon=cc.ALREADY_EPS, abs_diff=1)
    rc, ret, its, res, M = cmulti(lib, api, sid, A, M0, B, **para)
    assert rc == 0
    want = [ALREADY, ALREADY, CONV, ALREADY] if sid == BICG_SYM else [CONV, ALREADY, CONV, ALREADY]
    assert ret == want, ret
    for j in range(4):
        ref = cc.oracle_column(port, S, sid, B[:, j], ("already", j), m0=M0[:, j], **para)
        assert ret[j] == ref["ret"], (j, ret[j], ref["ret"])
        if ret[j] == ALREADY:
            assert its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            floor = rounding_floor(S, M0[:, j], B[:, j], sid)
            print(sid, j, "residual", res[j], ref["residual"], "rounding alone", floor)
            if ref["residual"] > 1e3 * floor:
                assert abs(res[j] - ref["residual"]) <= 1e-6 * ref["residual"], (j, res[j], ref["residual"])
            else:                           # a guess that is the solution to rounding: the residual is rounding itself, on either side
                assert res[j] <= floor and ref["residual"] <= floor, (j, res[j], ref["residual"], floor)
        else:
            assert abs(its[j] - ref["iters"]) <= 3 and res[j] <= cc.ALREADY_EPS


def verdict_batch(S):
    """Four columns under abs_diff = 1: 0 late (b), 1 early (1e-2 b), 2 a NaN in B, 3 zero."""
    n = S["n"]
    B = cc.columns(n, S["b"], 4)
    B[n // 2, 2] = complex(np.nan, 1.0)
    return B


@pytest.mark.parametrize("sid", SIDS)
def test_one_batch_different_verdicts(lib, api, handle, sid):
    S, A = handle(*cc.HELM40)
    n, k = S["n"], 4
    B = verdict_batch(S)
    M0 = np.zeros((n, k), np.complex128); M0[:, 3] = -0.0 - 0.0j
    para = dict(epsilon=1e-10, abs_diff=1)
    rc, ret, its, res, M = cmulti(lib, api, sid, A, M0, B, **para)
    assert rc == 0
    print(sid, ret, its, res)
    assert ret == [CONV, CONV, NANV, ALREADY], ret
    assert its[2] == 1 and its[3] == 0 and np.array_equal(bits(M[:, 3]), bits(M0[:, 3]))
    t_fast, t_slow = its[1], its[0]
    assert 0 < t_fast and t_fast + 2 <= t_slow, its
    assert np.isfinite(M[:, :2].view(np.float64)).all()
    # a cap between the two counts: all four verdicts in one call
    cap = (t_fast + t_slow) // 2
    rc, ret_c, its_c, res_c, M_c = cmulti(lib, api, sid, A, M0, B, max_iterations=cap, **para)
    assert rc == 0 and ret_c[1] == CONV and its_c[1] == t_fast and ret_c[0] == MAXIT and its_c[0] == cap
    assert np.array_equal(bits(M_c[:, 1]), bits(M[:, 1])) and res_c[1] == res[1]
    # frozen means final: the column that converged at t_fast while the others went on = the same B capped at t_fast
    rc, ret_f, its_f, res_f, M_f = cmulti(lib, api, sid, A, M0, B, max_iterations=t_fast, **para)
    assert rc == 0 and ret_f[1] == CONV and its_f[1] == t_fast and ret_f[0] == MAXIT and its_f[0] == t_fast
    assert np.array_equal(bits(M_f[:, 1]), bits(M[:, 1])) and res_f[1] == res[1]
    # max_iterations = 0 (no cap): the NaN column must not keep the batch alive -- the call above returned
    assert lib.lcg_hip_last_iterations() == t_fast


@pytest.mark.parametrize("key", [cc.HELM40, ("helm", 182), ("band30", 1029), ("band140", 2051)], ids=lambda k: f"{k[0]}-{k[1]}")
@pytest.mark.parametrize("sid", SIDS)
def test_independence_of_neighbours_k_and_calls(lib, api, handle, sid, key):
    """Column 0's iterate, count, residual and code: the same bits with its neighbours replaced by NaN, zero or other data, at k = 2,
    4 and 8, from call to call, from host memory -- on one stride and on three (helm 182), with and without the folded d.Ad."""
    S, A = handle(*key)
    n = S["n"]
    para = dict(epsilon=1e-10, abs_diff=1, max_iterations=12 if n > 2000 else 40)
    rng = np.random.default_rng(8)
    b0 = S["b"]
    m0 = 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))

    def run(k, pos, others, mem="device"):
        B = np.zeros((n, k), np.complex128); M0 = np.zeros((n, k), np.complex128)
        for j in range(k):
            if j == pos:
                B[:, j], M0[:, j] = b0, m0
            else:
                B[:, j], M0[:, j] = others(j)
        rc, ret, its, res, M = cmulti(lib, api, sid, A, M0, B, mem=mem, **para)
        assert rc == 0
        return ret[pos], its[pos], res[pos], bits(M[:, pos]).copy()

    def same(a, b, what):
        assert a[:3] == b[:3] and np.array_equal(a[3], b[3]), (what, a[:3], b[:3])

    other = lambda j: (3.0 * np.roll(b0, j + 1), np.zeros(n, np.complex128))
    base = run(4, 0, other)
    assert base[0] in (CONV, MAXIT) and base[1] > 5
    same(run(4, 0, other), base, "again")
    same(run(4, 0, other, mem="host"), base, "host")
    same(run(4, 0, lambda j: (np.full(n, complex(np.nan, np.nan)), np.zeros(n, np.complex128))), base, "NaN neighbours")
    same(run(4, 0, lambda j: (np.zeros(n, np.complex128), np.zeros(n, np.complex128))), base, "zero neighbours")
    same(run(4, 2, lambda j: (1e3 * np.roll(b0, 7 * j + 1), np.roll(m0, j + 1))), base, "another slot, other data")
    same(run(2, 1, other), base, "k = 2")
    same(run(8, 5, other), base, "k = 8")


def test_error_returns_release_the_solver(lib, api, handle):
    S, A = handle(*cc.HELM40)
    n, k = S["n"], 4
    B = cc.columns(n, S["b"], k)
    Z = np.zeros((n, k), np.complex128)
    good = dict(epsilon=1e-10, abs_diff=1, max_iterations=10)
    ref = cmulti(lib, api, BICG_SYM, A, Z, B, **good)
    assert ref[0] == 0

    def still_works():
        r = cmulti(lib, api, BICG_SYM, A, Z, B, **good)
        assert r[0] == 0 and r[1:4] == ref[1:4] and np.array_equal(bits(r[4]), bits(ref[4]))
        m = torch.zeros(n, dtype=torch.complex128, device="cuda")
        info = api.clcg_solver("clcg_hip_csr_ax", None, m, torch.from_numpy(S["b"]).cuda(), n,
                               api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=10), A, api.CLCG_BICG_SYM)
        assert info.ret == MAXIT and info.iterations == 10

    bare = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])            # no Jacobi diagonal
    r = cmulti(lib, api, PCG, bare, Z, B, **good)
    assert r[0] == NOPRE and r[1] == [99] * k                           # nothing ran, nothing was reported
    still_works()
    assert cmulti(lib, api, BICG_SYM, bare, Z, B, **good)[0] == 0       # BiCG-sym needs no diagonal
    bare.destroy()
    for sid in SIDS:
        assert cmulti(lib, api, sid, A, Z, B, epsilon=0.0)[0] == BADEPS
        still_works()
        assert cmulti(lib, api, sid, A, Z, B, epsilon=1.0)[0] == BADEPS
        assert cmulti(lib, api, sid, A, Z, B, max_iterations=-1)[0] == BADMAXIT
        still_works()
        # a non-square handle, a bad mem
        rect = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"], n_cols=n + 5)
        assert cmulti(lib, api, sid, rect, Z, B, **good)[0] == E_ARG and "square" in lib.lcg_hip_last_error().decode()
        rect.destroy()
        fn = lib.clcg_hip_lpcg_multi if sid == PCG else lib.clcg_hip_lbicg_sym_multi
        Zd = torch.zeros((n, k), dtype=torch.complex128, device="cuda")
        assert fn(A.h, k, Zd.data_ptr(), Zd.data_ptr(), None, None, None, None, 7) == E_ARG and "mem" in lib.lcg_hip_last_error().decode()
        still_works()


def test_python_front(api, handle):
    S, A = handle(*cc.HELM40)
    n = S["n"]
    B = torch.from_numpy(cc.columns(n, S["b"], 4)).cuda()
    p = api.clcg_default_parameters(epsilon=1e-10, abs_diff=1)
    for f in (api.clbicg_sym_multi, api.clpcg_multi):
        M = torch.zeros((n, 4), dtype=torch.complex128, device="cuda")
        infos = f(A, M, B, p)
        assert [i.ret for i in infos] == [CONV, CONV, CONV, ALREADY] and infos[3].iterations == 0
        Y = torch.full((n, 4), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
        A.cspmm(M, Y)
        api.synchronize()
        r = (Y - B).cpu().numpy()
        assert np.linalg.norm(r[:, 0]) / n <= 2e-5                      # (BiCG-sym's abs rule is sum |r|^2 / n <= 1e-10)
        Mh = np.zeros((n, 4), np.complex128)
        infos_h = f(A, Mh, B.cpu().numpy(), p)
        assert [i.ret for i in infos_h] == [CONV, CONV, CONV, ALREADY]
        assert np.array_equal(bits(Mh), bits(M.cpu().numpy()))


def test_sample_program_solves_four_sources_with_both_loops():
    import re
    import subprocess
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_c128")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = re.findall(r"^column (\d): ret=(-?\d+) iterations=(\d+)", p.stdout, flags=re.M)
    assert [(int(j), int(r)) for j, r, _ in got] == [(0, CONV), (1, CONV), (2, CONV), (3, ALREADY)] * 2
    assert "clcg_hip_lbicg_sym_multi" in p.stdout and "clcg_hip_lpcg_multi" in p.stdout
