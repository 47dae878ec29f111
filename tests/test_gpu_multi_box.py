"""-m gpu: the batched box-constrained solvers (lcg_hip_solver_constrained_multi, lcg_hip_dense_solver_constrained_multi; DESIGN.md
section 24) -- every column against the oracle's run of that column alone (tests/multi_box_cases.py: the table, its bounds and caps),
against the real liblcg's goldens, converged, with different verdicts in one call, at the reference's breakdown, with a NaN in one
column, independent of k, position and call, under every refusal, on a dense handle, on a caller's stream and through the Python
front and the example program.

Bands: the relative distance to the oracle's iterate is at most max(1e-9, 50 x the oracle's own response to 1-ulp changes of b at
that cap) (tests/test_gpu_multi_solvers.py's band); residuals within 1e-8 relative (test_box_constrained_vs_golden's figure).
products[j] equals the oracle's n_ax; device sums round differently from the oracle's, so over everything this module compares at
most 1 running column in 20 may differ in products (it still meets the distance band), counted in test_products_budget.
No test runs with max_iterations = 0: 500 stands for "unbounded"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dense_multi_cases as dm
import multi_box_cases as X
import multi_cases as mc
import stream_cases as st
from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PG, SPG, KS, RULE = X.PG, X.SPG, X.KS, X.RULE
CONV, ALREADY, MAXIT, NANV, E_ARG = X.CONV, X.ALREADY, X.MAXIT, X.NANV, X.E_ARG
UNBOUNDED = 500


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


_HANDLES = {}


@pytest.fixture(scope="module")
def handle(api):
    def get(S):
        if S["key"] not in _HANDLES:
            _HANDLES[S["key"]] = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
        return _HANDLES[S["key"]]
    yield get
    for A in _HANDLES.values():
        A.destroy()
    _HANDLES.clear()


def col(Y, j):
    return np.ascontiguousarray(Y[:, j])


_PRODUCTS = {}      # (what, column) -> whether products[j] differed from the oracle's n_ax, for every running column compared


def against_oracle(port, S, sid, r, B, low, hig, tag, m0=None, **para):
    """Every column of the batched result r against the oracle's run of that column alone."""
    rc, ret, its, prods, res, out = r
    assert rc == 0, (tag, rc)
    for j in range(B.shape[1]):
        g0 = None if m0 is None else col(m0, j)
        pj = dict(para)
        ref = X.oracle_column(port, S, sid, col(B, j), low, hig, m0=g0, **pj)
        want = (ref["ret"], ref["iters"])
        if not np.isfinite(ref["x"]).all():
            # the reference broke down before the cap and ran on with NaN (deviation 1): the batch column ends with LCG_NAN_VALUE one
            # iteration before the reference's first NaN iterate, and is held to the oracle's run capped there
            rest = {a: b for a, b in pj.items() if a != "max_iterations"}
            c = X.first_nan_cap(port, S, sid, col(B, j), low, hig, limit=pj["max_iterations"], m0=g0, **rest)
            assert c is not None and c >= 2, (tag, j, c)
            pj = dict(rest, max_iterations=c - 1)
            ref = X.oracle_column(port, S, sid, col(B, j), low, hig, m0=g0, **pj)
            want = (NANV, c - 1)
        assert (ret[j], its[j]) == want, (tag, j, ret[j], its[j], want)
        x = col(out, j)
        assert np.isfinite(x).all() and (x >= low).all() and (x <= hig).all(), (tag, j, "outside the box")
        dist, lim = X.rel(x, ref["x"]), X.band(port, S, sid, col(B, j), low, hig, m0=g0, **pj)
        print(f"{tag} column {j}: ret {ret[j]} iterations {its[j]} products {prods[j]} (oracle {ref['n_ax']}) distance {dist:.3e} band {lim:.3e}")
        assert dist <= lim, (tag, j, dist, lim)
        # 1e-8 relative, on top of what rounding alone can put into the residual of this iterate (multi_cases.rounding_floor: every row
        # of g within the product's rounding bound) -- near the stop rule g is a difference of numbers 1e9 times larger, and a
        # residual that is rounding of an exact zero has no relative accuracy at all
        floor = mc.rounding_floor(S, ref["x"], col(B, j), pj["abs_diff"])
        assert abs(res[j] - ref["residual"]) <= 1e-8 * abs(ref["residual"]) + floor, (tag, j, res[j], ref["residual"], floor)
        if ref["ret"] != ALREADY:
            _PRODUCTS[(tag, j)] = prods[j] != ref["n_ax"]
        else:
            assert prods[j] == ref["n_ax"] == 1, (tag, j, prods[j])


_RUNS = {}


def table_run(lib, api, handle, key, sid, k):
    if (key, sid, k) not in _RUNS:
        S = X.system(*key)
        low, hig = X.bounds(S)
        _RUNS[(key, sid, k)] = X.solve(lib, api, sid, handle(S), np.zeros((S["n"], k)), X.columns(S, k), low, hig, max_iterations=X.TABLE[key][2], **RULE)
    return _RUNS[(key, sid, k)]


# ================================================================================================ 1. capped, the whole table
@pytest.mark.parametrize("sid", X.SOLVERS)
@pytest.mark.parametrize("key", list(X.TABLE), ids=lambda c: X.IDS[c])
def test_capped_every_column_against_the_oracle(lib, api, port, handle, key, sid):
    S = X.system(*key)
    low, hig = X.bounds(S)
    for k in KS:
        against_oracle(port, S, sid, table_run(lib, api, handle, key, sid, k), X.columns(S, k), low, hig, (key, sid, k),
                       max_iterations=X.TABLE[key][2], **RULE)


# ================================================================================================ 2. the real liblcg
@pytest.mark.parametrize("tag", ["pg_40", "spg_40"])
def test_column_b_against_the_real_liblcg(lib, api, goldens, handle, tag):
    """test_box_constrained_vs_golden's assertions on column b of the batch, at k = 2, 4, 8."""
    ret, iters, sid, ad, maxit, n_ax = goldens[f"box/{tag}/meta"]
    eps, resid = goldens[f"box/{tag}/fl"]
    gold = goldens[f"box/{tag}/x"]
    assert (float(eps), int(ad), int(maxit)) == (RULE["epsilon"], RULE["abs_diff"], 40)
    for k in KS:
        rc, rets, its, prods, res, out = table_run(lib, api, handle, ("case10k", 10000), int(sid), k)
        x = col(out, 0)
        assert rc == 0 and rets[0] == ret and its[0] == iters
        assert prods[0] == n_ax                                         # same number of A.x calls: same line-search path
        assert x.min() >= -5.0 and x.max() <= 8.0
        assert np.array_equal(x <= -5.0, gold <= -5.0) and np.array_equal(x >= 8.0, gold >= 8.0)    # same active set
        assert np.linalg.norm(x - gold) / np.linalg.norm(gold) <= 1e-9
        assert abs(res[0] - resid) <= 1e-8 * resid


# ================================================================================================ 3. converged
_CONVERGED = {}


def converged_run(lib, api, handle, sid):
    if sid not in _CONVERGED:
        S = X.system("case10k")
        low, hig = X.bounds(S)
        _CONVERGED[sid] = X.solve(lib, api, sid, handle(S), np.zeros((S["n"], 2)), X.columns(S, 2), low, hig, max_iterations=UNBOUNDED, **RULE)
    return _CONVERGED[sid]


@pytest.mark.parametrize("sid", X.SOLVERS)
def test_converged_column(lib, api, port, handle, sid):
    """Column 1e-6 b of case_10K_A between -5 and 8 meets the stop rule (the oracle: 71 iterations for PG, 83 for SPG)."""
    S = X.system("case10k")
    low, hig = X.bounds(S)
    bcol = col(X.columns(S, 2), 1)
    ref = X.oracle_column(port, S, sid, bcol, low, hig, max_iterations=UNBOUNDED, **RULE)
    assert ref["ret"] == CONV and ref["iters"] == {PG: 71, SPG: 83}[sid]
    rc, ret, its, prods, res, out = converged_run(lib, api, handle, sid)
    print(f"converged {sid}: iterations {its[1]} (oracle {ref['iters']}) products {prods[1]} (oracle {ref['n_ax']}) residual {res[1]:.3e}")
    assert rc == 0 and ret[1] == CONV and abs(its[1] - ref["iters"]) <= 3 and res[1] <= RULE["epsilon"]
    same = its[1] == ref["iters"]
    lim = X.band(port, S, sid, bcol, low, hig, max_iterations=UNBOUNDED, **RULE) if same else 1e-7
    assert X.rel(col(out, 1), ref["x"]) <= lim, (X.rel(col(out, 1), ref["x"]), lim, same)


# ================================================================================================ 4. different verdicts in one call
@pytest.mark.parametrize("sid", X.SOLVERS)
def test_different_verdicts_in_one_call_and_stopped_columns_are_final(lib, api, handle, sid):
    S = X.system("case10k")
    low, hig = X.bounds(S)
    A = handle(S)
    count = converged_run(lib, api, handle, sid)[2][1]
    cap = count + 5                                     # column b and the random column are far from their stop rule there
    B = X.columns(S, 4)
    M0 = np.zeros((S["n"], 4)); M0[:, 3] = -0.0
    rc, ret, its, prods, res, out = X.solve(lib, api, sid, A, M0, B, low, hig, max_iterations=cap, **RULE)
    assert rc == 0 and ret == [MAXIT, CONV, MAXIT, ALREADY] and its == [cap, count, cap, 0], (ret, its, cap)
    assert prods[3] == 1 and res[1] <= RULE["epsilon"]
    # the zero column with its -0.0 guess: not a bit has changed
    assert np.array_equal(X.bits(col(out, 3)), X.bits(np.full(S["n"], -0.0)))
    # the converged column went on for nothing after its stop: the run capped at its own count has its bits
    rc2, ret2, its2, prods2, res2, out2 = X.solve(lib, api, sid, A, M0, B, low, hig, max_iterations=count, **RULE)
    assert rc2 == 0 and (ret2[1], its2[1]) == (CONV, count)
    assert np.array_equal(X.bits(col(out, 1)), X.bits(col(out2, 1))) and X.bits(np.array([res[1]]))[0] == X.bits(np.array([res2[1]]))[0]
    assert prods[1] == prods2[1]


# ================================================================================================ 5. breakdown
@pytest.mark.parametrize("sid", X.SOLVERS)
@pytest.mark.parametrize("case", X.BREAKDOWN, ids=X.BREAKDOWN_IDS)
def test_breakdown_ends_the_column_one_iteration_before_the_references_nan(lib, api, port, handle, case, sid):
    key, lo, hi = case
    S = X.system(*key)
    low, hig = X.bounds(S, lo, hi)
    A = handle(S)
    nan_cap = X.first_nan_cap(port, S, sid, S["b"], low, hig, **RULE)
    assert nan_cap is not None and nan_cap >= 2
    B = X.columns(S, 4)
    rc, ret, its, prods, res, out = X.solve(lib, api, sid, A, np.zeros((S["n"], 4)), B, low, hig, max_iterations=UNBOUNDED, **RULE)
    print(f"breakdown {key} {sid}: ret {ret} iterations {its} products {prods} (the oracle's first NaN iterate: cap {nan_cap})")
    assert rc == 0 and ret[0] == NANV and its[0] == nan_cap - 1, (ret, its, nan_cap)
    x = col(out, 0)
    assert np.isfinite(x).all() and x.min() >= lo and x.max() <= hi
    ref = X.oracle_column(port, S, sid, S["b"], low, hig, max_iterations=nan_cap - 1, **RULE)
    lim = X.band(port, S, sid, S["b"], low, hig, max_iterations=nan_cap - 1, **RULE)
    assert X.rel(x, ref["x"]) <= lim, (X.rel(x, ref["x"]), lim)
    # nobody else noticed
    B0 = B.copy(); B0[:, 0] = 0.0
    rc0, ret0, its0, prods0, res0, out0 = X.solve(lib, api, sid, A, np.zeros((S["n"], 4)), B0, low, hig, max_iterations=UNBOUNDED, **RULE)
    assert rc0 == 0
    for j in (1, 2, 3):
        assert (ret[j], its[j], prods[j]) == (ret0[j], its0[j], prods0[j]) and np.array_equal(X.bits(col(out, j)), X.bits(col(out0, j))), (key, sid, j)
        assert X.bits(np.array([res[j]]))[0] == X.bits(np.array([res0[j]]))[0]


@pytest.mark.parametrize("sid", X.SOLVERS)
def test_breakdown_whose_iteration_rounding_moves(lib, api, port, handle, sid):
    """spd 65 between -0.5 and 0.8: the iteration at which the iterate stops moving to the last bit depends on rounding (the CPU test:
    44 .. 57 in the oracle over 1-ulp changes of b), so the count is held to that window only; the verdict, the box and the iterate
    -- the constrained solution, where every such run ends -- are held as in the pinned cases."""
    key, lo, hi = X.UNPINNED_BREAKDOWN
    S = X.system(*key)
    low, hig = X.bounds(S, lo, hi)
    nan_cap = X.first_nan_cap(port, S, sid, S["b"], low, hig, **RULE)
    rc, ret, its, prods, res, out = X.solve(lib, api, sid, handle(S), np.zeros((S["n"], 2)), X.columns(S, 2), low, hig, max_iterations=UNBOUNDED, **RULE)
    print(f"unpinned breakdown {sid}: ret {ret} iterations {its} products {prods} (the oracle's first NaN iterate: cap {nan_cap})")
    assert rc == 0 and ret[0] == NANV and 40 <= its[0] <= 60, (ret, its)
    x = col(out, 0)
    assert np.isfinite(x).all() and x.min() >= lo and x.max() <= hi
    ref = X.oracle_column(port, S, sid, S["b"], low, hig, max_iterations=nan_cap - 1, **RULE)
    assert X.rel(x, ref["x"]) <= 1e-9, X.rel(x, ref["x"])


# ================================================================================================ 6. a NaN stays in its column
@pytest.mark.parametrize("sid", X.SOLVERS)
def test_a_nan_stays_in_its_column(lib, api, handle, sid):
    key = ("spd", 513)
    S = X.system(*key)
    low, hig = X.bounds(S)
    clean = table_run(lib, api, handle, key, sid, 4)
    B = X.columns(S, 4).copy()
    B[300, 1] = np.nan
    rc, ret, its, prods, res, out = X.solve(lib, api, sid, handle(S), np.zeros((S["n"], 4)), B, low, hig, max_iterations=X.TABLE[key][2], **RULE)
    assert rc == 0 and ret[1] == NANV, ret
    for j in (0, 2, 3):
        assert (ret[j], its[j], prods[j]) == (clean[1][j], clean[2][j], clean[3][j]), (sid, j)
        assert np.array_equal(X.bits(col(out, j)), X.bits(col(clean[5], j))) and X.bits(np.array([res[j]]))[0] == X.bits(np.array([clean[4][j]]))[0]


# ================================================================================================ 7. independence, repeatability
@pytest.mark.parametrize("sid", X.SOLVERS)
@pytest.mark.parametrize("key", [("spd", 513), ("case10k", 10000)], ids=lambda c: X.IDS[c])
def test_a_column_has_the_same_bits_whatever_k_is_and_wherever_it_stands(lib, api, handle, key, sid):
    S = X.system(*key)
    low, hig = X.bounds(S)
    cap = X.TABLE[key][2]
    runs = {k: table_run(lib, api, handle, key, sid, k) for k in KS}

    def same(a, ja, b, jb, why):
        assert (a[1][ja], a[2][ja], a[3][ja]) == (b[1][jb], b[2][jb], b[3][jb]), (why, key, sid)
        assert X.bits(np.array([a[4][ja]]))[0] == X.bits(np.array([b[4][jb]]))[0], (why, key, sid)
        assert np.array_equal(X.bits(col(a[5], ja)), X.bits(col(b[5], jb))), (why, key, sid)
    for j in (0, 1):
        same(runs[2], j, runs[4], j, "k = 2 / 4"); same(runs[2], j, runs[8], j, "k = 2 / 8")
    for j in (2, 3):
        same(runs[4], j, runs[8], j, "k = 4 / 8")
    B = X.columns(S, 4)
    perm = [3, 2, 0, 1]
    moved = X.solve(lib, api, sid, handle(S), np.zeros((S["n"], 4)), np.ascontiguousarray(B[:, perm]), low, hig, max_iterations=cap, **RULE)
    for pos, j in enumerate(perm):
        same(moved, pos, runs[4], j, "position")
    again = X.solve(lib, api, sid, handle(S), np.zeros((S["n"], 4)), B, low, hig, max_iterations=cap, **RULE)
    host = X.solve(lib, api, sid, handle(S), np.zeros((S["n"], 4)), B, low, hig, mem="host", max_iterations=cap, **RULE)
    for j in range(4):
        same(again, j, runs[4], j, "second call"); same(host, j, runs[4], j, "host memory")


@pytest.mark.parametrize("sid", X.SOLVERS)
def test_a_guess_outside_the_box_is_projected_first(lib, api, port, handle, sid):
    S = X.system("case10k")
    low, hig = X.bounds(S)
    B = X.columns(S, 2)
    M0 = np.full((S["n"], 2), 20.0)
    r = X.solve(lib, api, sid, handle(S), M0, B, low, hig, max_iterations=15, **RULE)
    against_oracle(port, S, sid, r, B, low, hig, ("guess 20", sid), m0=M0, max_iterations=15, **RULE)


# ================================================================================================ 8. SPG parameters
SETTINGS = [dict(maxi_m=1), dict(maxi_m=3), dict(maxi_m=X.MAXIM_BOUND), dict(sigma=0.5, beta=0.5)]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "-".join(f"{a}{b}" for a, b in s.items()))
def test_spg_parameters(lib, api, port, handle, setting):
    """(Each setting passes tests/test_multi_box_cases_cpu.py's zero-flip check.)"""
    S = X.system("spd", 65)
    low, hig = X.bounds(S)
    B = X.columns(S, 4)
    r = X.solve(lib, api, SPG, handle(S), np.zeros((S["n"], 4)), B, low, hig, max_iterations=12, **RULE, **setting)
    against_oracle(port, S, SPG, r, B, low, hig, ("setting", tuple(setting.items())), max_iterations=12, **RULE, **setting)


def test_products_budget(lib, api, port, handle):
    """Over every running column this module compared with the oracle -- the whole table, if this test runs alone -- at most one
    in twenty differs from the oracle's n_ax."""
    for key in X.TABLE:
        for sid in X.SOLVERS:
            if not any(t[0] == (key, sid, 8) for t in _PRODUCTS):
                test_capped_every_column_against_the_oracle(lib, api, port, handle, key, sid)
    differ = sorted(t for t, d in _PRODUCTS.items() if d)
    print(f"products: {len(differ)} of {len(_PRODUCTS)} running columns differ from the oracle's n_ax: {differ}")
    assert 20 * len(differ) <= len(_PRODUCTS), differ


# ================================================================================================ 9. error returns
def test_error_returns(lib, api, port, handle):
    S = X.system("spd", 65)
    low, hig = X.bounds(S)
    A = handle(S)
    B = X.columns(S, 2)
    M0 = np.zeros((S["n"], 2))
    good = lambda: X.solve(lib, api, SPG, A, M0, B, low, hig, max_iterations=12, **RULE)       # noqa: E731
    first = good()
    assert first[0] == 0

    def still_fine():
        r = good()
        assert r[:5] == first[:5] and np.array_equal(X.bits(r[5]), X.bits(first[5]))
        m = torch.zeros(S["n"], dtype=torch.float64, device="cuda")
        info = api.lcg_solver("lcg_hip_csr_ax", None, m, torch.from_numpy(S["b"]).cuda(), S["n"], api.lcg_default_parameters(epsilon=1e-10), A, 0)
        assert info.ret == CONV

    def refused(code, sid, A_=A, M=M0, normal=None, **para):
        rc, ret, its, prods, res, out = X.solve(lib, api, sid, A_, M, np.ascontiguousarray(B[:M.shape[0]]), low[:M.shape[0]], hig[:M.shape[0]],
                                                normal=normal, **para)
        assert rc == code and ret == [99, 99] and its == [-1, -1] and prods == [-1, -1], (rc, code, sid, para, ret)
        assert np.array_equal(out, M)
        if code == E_ARG:
            assert "lcg_hip_" in lib.lcg_hip_last_error().decode(), lib.lcg_hip_last_error()
        still_fine()
    # the reference's parameter codes, in its order (lcg.cpp:1062-1065, 1232-1238)
    refused(-1022, PG, max_iterations=-1); refused(-1021, PG, epsilon=0.0); refused(-1015, PG, step=0.0); refused(-1015, PG, epsilon=1.0)
    refused(-1022, PG, max_iterations=-1, epsilon=0.0, step=0.0); refused(-1021, PG, epsilon=0.0, step=0.0)
    refused(-1022, SPG, max_iterations=-1); refused(-1021, SPG, epsilon=0.0); refused(-1021, SPG, epsilon=1.0); refused(-1015, SPG, step=-1.0)
    refused(-1014, SPG, sigma=1.0); refused(-1014, SPG, sigma=0.0); refused(-1013, SPG, beta=0.0); refused(-1013, SPG, beta=1.0)
    refused(-1012, SPG, maxi_m=0)
    refused(-1021, SPG, epsilon=2.0, step=0.0, sigma=0.0, beta=0.0, maxi_m=0); refused(-1015, SPG, step=0.0, sigma=0.0, beta=0.0, maxi_m=0)
    refused(-1014, SPG, sigma=0.0, beta=0.0, maxi_m=0); refused(-1013, SPG, beta=0.0, maxi_m=0)
    refused(E_ARG, SPG, maxi_m=X.MAXIM_BOUND + 1)
    assert "maxi_m" in lib.lcg_hip_last_error().decode()
    assert X.solve(lib, api, PG, A, M0, B, low, hig, max_iterations=3, maxi_m=1000, **RULE)[0] == 0       # lpg does not look at maxi_m
    # LCG_HIP_E_ARG: handles and mem (k, null and misaligned vectors: tests/test_multi_box_cases_cpu.py, without a device; a sharded
    # handle needs a second rank and is refused by the check all batched entries share, multi_handle)
    Z = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"].astype(np.complex128))
    Z64 = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"].astype(np.complex64))
    wide = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"], n_cols=S["n"] + 3)
    D = api.DenseMatrix.from_array(dm.system(96, 80)["K"])
    try:
        for sid in X.SOLVERS:
            for H in (Z, Z64, wide, D):
                refused(E_ARG, sid, A_=H, max_iterations=12)
        rc = lib.lcg_hip_solver_constrained_multi(A.h, 2, SPG, None, None, None, None, None, None, None, None, None, 1)
        assert rc == E_ARG
        p = api.lcg_default_parameters(max_iterations=12)
        Md, Bd, ld, hd = (torch.from_numpy(a).cuda() for a in (M0, B, low, hig))
        ret = (C.c_int * 2)(99, 99)
        for mem in (2, -1, 7):
            assert lib.lcg_hip_solver_constrained_multi(A.h, 2, SPG, Md.data_ptr(), Bd.data_ptr(), ld.data_ptr(), hd.data_ptr(), C.byref(p), ret, None, None, None, mem) == E_ARG
            assert "mem" in lib.lcg_hip_last_error().decode() and list(ret) == [99, 99]
        still_fine()
        # the dense entry: a CSR handle, normal = 0 on a K that is not square, mem, normal
        M80 = np.zeros((80, 2))
        refused(E_ARG, SPG, A_=A, M=M80, normal=1, max_iterations=12)
        refused(E_ARG, SPG, A_=D, M=M80, normal=0, max_iterations=12)
        assert "square" in lib.lcg_hip_last_error().decode()
        refused(E_ARG, PG, A_=D, M=M80, normal=2, max_iterations=12)
        assert "normal" in lib.lcg_hip_last_error().decode()
        refused(-1015, PG, A_=D, M=M80, normal=1, epsilon=1.0)
        refused(E_ARG, SPG, A_=D, M=M80, normal=1, maxi_m=65)
    finally:
        for H in (Z, Z64, wide, D):
            H.destroy()


# ================================================================================================ 10. dense
def dense_as_csr(S):
    """The operator of a dense system, formed on the host in float64, as a full CSR matrix for the oracle."""
    K = S["K"]
    A = K.T @ K if S["normal"] else K
    n = A.shape[0]
    return {"key": ("dense",) + S["key"], "n": n, "rp": (np.arange(n + 1) * n).astype(np.int32), "ci": np.tile(np.arange(n), n).astype(np.int32),
            "v": np.ascontiguousarray(A).ravel().copy(), "b": S["b"]}


@pytest.mark.parametrize("sid", X.SOLVERS)
@pytest.mark.parametrize("shape", [(96, 80, True), (80, 80, False)], ids=["KtK-96x80", "K-80x80"])
def test_dense_operators(lib, api, port, shape, sid):
    """K^T.K of a 96 x 80 K and a square SPD 80 x 80 K, bounds that cut the solution (xt lies in [1, 2]), cap 12."""
    DS = dm.system(*shape)
    S = dense_as_csr(DS)
    normal = int(shape[2])
    low, hig = np.full(80, 0.5), np.full(80, 1.6)
    D = api.DenseMatrix.from_array(DS["K"])
    try:
        # what one product costs in launches: lcg_hip_dense_lcg_multi's own count, a setup product and one per iteration with its sum
        runs = {}
        for k in KS:
            B = dm.columns(DS, k)
            dm.multi(lib, api, dm.CG, D, bool(normal), np.zeros((80, k)), B, epsilon=1e-10, max_iterations=1)
            prod = C.c_int(); lib.lcg_hip_last_launches(None, None, None, C.byref(prod))
            per = (prod.value - 1) // 2
            assert prod.value == 2 * per + 1 and per >= 1
            runs[k] = X.solve(lib, api, sid, D, np.zeros((80, k)), B, low, hig, normal=normal, max_iterations=12, **RULE)
            vec = C.c_int(); lib.lcg_hip_last_launches(C.byref(vec), None, None, C.byref(prod))
            against_oracle(port, S, sid, runs[k], B, low, hig, ("dense", shape, sid, k), max_iterations=12, **RULE)
            bodies = max(runs[k][3]) - 1
            assert prod.value % per == 0 and vec.value == 3 + 2 * (prod.value // per - 1), (prod.value, per, vec.value)
            assert prod.value // per - 1 >= bodies and (sid == SPG or prod.value // per - 1 == 12), (prod.value, per, bodies)
            active = [int(((col(runs[k][5], j) <= 0.5) | (col(runs[k][5], j) >= 1.6)).sum()) for j in range(k)]
            assert active[0] > 0, active
        for a, b, cols in ((runs[2], runs[4], (0, 1)), (runs[2], runs[8], (0, 1)), (runs[4], runs[8], (2, 3))):      # column bits independent of k
            for j in cols:
                assert (a[1][j], a[2][j], a[3][j]) == (b[1][j], b[2][j], b[3][j]) and np.array_equal(X.bits(col(a[5], j)), X.bits(col(b[5], j))), (shape, sid, j)
    finally:
        D.destroy()


# ================================================================================================ 11. a caller's stream
@pytest.fixture(scope="module")
def env(api, lib):
    e = st.make_env(torch, api, lib)
    yield e
    st.close_env(e)


@pytest.mark.parametrize("sid", X.SOLVERS)
def test_callers_stream(env, api, lib, handle, sid):
    """tests/test_gpu_streams_kwide.py's pattern: run (b) on the side stream, entered while the delay runs on it with M, B, low and hig
    written behind the delay, has run (a)'s codes, counts, products, residuals and iterate, for both entries."""
    S = X.system("spd", 513)
    DS = dm.system(96, 80)
    D = api.DenseMatrix.from_array(DS["K"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    para = api.lcg_default_parameters(max_iterations=12, **RULE)
    try:
        for which, k in (("csr", 2), ("csr", 8), ("dense", 4)):
            if which == "csr":
                Bh, (lo, hi) = X.columns(S, k), X.bounds(S)
                fn, lead = lib.lcg_hip_solver_constrained_multi, (handle(S).h, k, sid)
            else:
                Bh, lo, hi = dm.columns(DS, k), np.full(80, 0.5), np.full(80, 1.6)
                fn, lead = lib.lcg_hip_dense_solver_constrained_multi, (D.h, k, 1, sid)
            srcs = [dev(np.zeros_like(Bh)), dev(Bh), dev(lo), dev(hi)]
            Md, Bd, ld, hd = (torch.empty_like(t) for t in srcs)

            def call():
                ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); prods = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
                rc = fn(*lead, Md.data_ptr(), Bd.data_ptr(), ld.data_ptr(), hd.data_ptr(), C.byref(para), ret, its, prods, res, 1)
                return rc, list(ret), list(its), list(prods), list(res)

            def anchor(r, outs):
                rc, ret, its, prods, res = r
                assert rc == 0 and 99 not in ret and -1 not in its and max(its) == 12 and max(prods) >= 13, (which, k, r, lib.lcg_hip_last_error())
                st.no_nan(outs, (which, k, sid))
            env.pair(list(zip((Md, Bd, ld, hd), srcs)), call, [Md], False, tag=(which, k, sid), anchor=anchor)
    finally:
        D.destroy()


# ================================================================================================ 12. the Python front, the example
def test_python_front(lib, api, handle):
    S = X.system("spd", 513)
    low, hig = X.bounds(S)
    B = X.columns(S, 4)
    para = api.lcg_default_parameters(max_iterations=12, **RULE)
    for sid in X.SOLVERS:
        want = table_run(lib, api, handle, ("spd", 513), sid, 4)
        M = torch.zeros((S["n"], 4), dtype=torch.float64, device="cuda")
        infos = api.lcg_solver_constrained_multi(handle(S), M, torch.from_numpy(B).cuda(), torch.from_numpy(low).cuda(), torch.from_numpy(hig).cuda(), para, sid)
        api.synchronize()
        assert [(i.ret, i.iterations, i.products, i.residual) for i in infos] == list(zip(want[1], want[2], want[3], want[4]))
        assert np.array_equal(X.bits(M.cpu().numpy()), X.bits(want[5]))
        Mh = X.aligned(np.zeros((S["n"], 4)))
        infos = api.lcg_solver_constrained_multi(handle(S), Mh, X.aligned(B), low, hig, para, sid)
        assert [i.products for i in infos] == want[3] and np.array_equal(X.bits(Mh), X.bits(want[5]))
    DS = dm.system(96, 80)
    D = api.DenseMatrix.from_array(DS["K"])
    try:
        M = X.aligned(np.zeros((80, 2)))
        infos = api.dense_solver_constrained_multi(D, M, X.aligned(dm.columns(DS, 2)), np.full(80, 0.5), np.full(80, 1.6), para, SPG, normal=True)
        assert [i.ret for i in infos] == [MAXIT, MAXIT] and all(i.products >= 13 for i in infos) and M.min() >= 0.5 and M.max() <= 1.6
    finally:
        D.destroy()


def test_sample_program_solves_four_columns_with_both_solvers():
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_box")
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout, p.stderr)
    import re
    lines = re.findall(r"^column (\d): ret=(-?\d+) iterations=(\d+) products=(\d+)", p.stdout, flags=re.M)
    assert len(lines) == 8, p.stdout
    got = [(int(a), int(b), int(c), int(d)) for a, b, c, d in lines]
    assert [g[:3] for g in got[:4]] == [(0, MAXIT, 40), (1, MAXIT, 40), (2, MAXIT, 40), (3, ALREADY, 0)], p.stdout      # PG
    assert [g[3] for g in got[:4]] == [41, 41, 41, 1]
    assert [g[:3] for g in got[4:]] == [(0, MAXIT, 40), (1, MAXIT, 40), (2, MAXIT, 40), (3, ALREADY, 0)], p.stdout      # SPG
    assert [got[4][3], got[5][3], got[7][3]] == [125, 198, 1] and got[6][3] > 41, p.stdout     # b and 1e-6 b: the oracle's counts
