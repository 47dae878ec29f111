"""With the checker alone (tests/c64_checker.py in complex64, no GPU): the solver cases of tests/multi_c64_cases.py are what
tests/test_gpu_multi_c64_solvers.py takes them for.  The properties are conditions on the inputs, asserted here so that a change of
a seed or a system that loses them is caught where it is made."""
import numpy as np
import pytest

import multi_c64_cases as cc
from multi_c64_cases import ALREADY, BICG_SYM, CONV, KS, PCG, SIDS

NAMES = ["b", "small", "rand", "zero", "minus", "rand3", "half", "twice"]


def _runs(S, sid, k, eps):
    B = cc.columns(S, k)
    return B, [cc.checker_column(S, sid, B[:, j], ("col", NAMES[j]), epsilon=eps, max_iterations=3000) for j in range(k)]


def test_blocks_are_complex64_row_major():
    S = cc.system("helmholtz", 40)
    for k in KS:
        B = cc.columns(S, k)
        assert B.shape == (1600, k) and B.dtype == np.complex64 and B.flags["C_CONTIGUOUS"]
    B8 = cc.columns(S, 8)
    for k in (2, 4):
        assert np.array_equal(cc.columns(S, k), B8[:, :k])      # a column is the same data at every k
    assert not B8[:, 3].any() and all(B8[:, j].any() for j in (0, 1, 2, 4, 5, 6, 7))
    P = cc.pair_small_zero(S)
    assert np.array_equal(P[:, 0], B8[:, 1]) and not P[:, 1].any()
    a = cc.aligned_block(B8)
    assert a.ctypes.data % 16 == 0 and np.array_equal(a, B8)


@pytest.mark.parametrize("sid", SIDS)
@pytest.mark.parametrize("nx", [40, 100])
def test_converged_cases_converge_in_complex64(sid, nx):
    """epsilon = 1e-10 on helmholtz(nx): every non-zero column converges (code 0) well inside the cap, the zero column is "already
    optimised" at iteration 0."""
    S = cc.system("helmholtz", nx)
    B, runs = _runs(S, sid, 8, 1e-10)
    for j, r in enumerate(runs):
        if not B[:, j].any():
            assert r["ret"] == ALREADY and r["iters"] == 0
        else:
            assert r["ret"] == CONV and 10 <= r["iters"] <= 60, (j, r["ret"], r["iters"])


@pytest.mark.parametrize("sid", SIDS)
def test_freezing_case_stops_its_columns_at_different_iterations(sid):
    """epsilon = 1e-8 on helmholtz(40): the columns of a k = 4 batch do not all stop together, and 1e-2 b stops at least two
    iterations before b and the random column -- what makes the batch freeze a column while its neighbours run."""
    S = cc.system("helmholtz", 40)
    B, runs = _runs(S, sid, 4, 1e-8)
    assert [r["ret"] for r in runs] == [CONV, CONV, CONV, ALREADY]
    its = [r["iters"] for r in runs]
    assert len(set(its[:3])) >= 2 and its[3] == 0, its
    assert its[1] + 2 <= its[0] and its[1] + 2 <= its[2], its
    # a NaN in B: the checker ends that column with CLCG_NAN_VALUE at count 1
    bad = B[:, 2].copy(); bad[S["n"] // 2] = complex(np.nan, 1.0)
    r = cc.checker_column(S, sid, bad, ("col", "nan"), epsilon=1e-8, max_iterations=3000)
    assert r["ret"] == cc.NANV and r["iters"] == 1


@pytest.mark.parametrize("sid", SIDS)
def test_capped_cases_run_to_their_caps(sid):
    """helmholtz(100), caps 1 .. 6, epsilon = 1e-30: every non-zero column is still running at the cap."""
    S = cc.system("helmholtz", 100)
    B = cc.columns(S, 8)
    for cap in range(1, 7):
        for j in (0, 1, 2, 4, 5, 6, 7):
            r, tol = cc.tol_column(S, sid, B[:, j], ("col", NAMES[j]), epsilon=1e-30, max_iterations=cap)
            assert r["ret"] == cc.MAXIT and r["iters"] == cap and tol < 1e-3, (cap, j, r["ret"], r["iters"], tol)
