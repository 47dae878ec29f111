"""The stop contract the device loops are held to (tests/test_gpu_stop_contract.py) is the reference's own: on the same systems
the oracle's capped run returns, bit for bit, the iterate its progress callback was handed at that count; a non-zero return from
the callback ends the run with that iterate; a NaN in b ends it where the device tests expect.  And the systems are fit for the
purpose: every loop's oracle run converges in 8 ... 200 iterations at all sizes, and the PG / SPG box is active for some
components and not for others."""
import numpy as np
import pytest

import stop_cases as sc


@pytest.fixture(scope="module")
def systems():
    cache = {}

    def get(kind, n):
        if (kind, n) not in cache:
            cache[(kind, n)] = sc.system(kind, n)
        return cache[(kind, n)]
    return get


@pytest.mark.parametrize("L,n", sc.CASES, ids=sc.CASE_IDS)
def test_oracle_converges_in_the_window(port, systems, L, n):
    S = systems(L.kind, n)
    r = sc.oracle_run(port, L, S)
    print(f"{L.name} n={n}: oracle ret {r['ret']} after {r['iters']} iterations, residual {r['residual']:.3e}")
    assert r["ret"] == 0, (L.name, n, r["ret"], r["iters"])
    assert sc.ITER_WINDOW[0] <= r["iters"] <= sc.ITER_WINDOW[1], (L.name, n, r["iters"])
    assert r["ks"] == list(range(r["iters"] + 1))
    if L.oracle in ("pg", "spg"):
        low, hig = sc.box(S)
        at_bound = (r["x"] == hig) | (r["x"] == low)
        assert at_bound.any() and not at_bound.all(), (L.name, n, int(at_bound.sum()))
        assert np.all(r["x"] <= hig) and np.all(r["x"] >= low)


SMALL = [(L, n) for L, n in sc.CASES if n <= 513]


@pytest.mark.parametrize("L,n", SMALL, ids=[f"{L.name}-{n}" for L, n in SMALL])
def test_oracle_capped_run_is_the_callbacks_iterate_and_stop_returns_it(port, systems, L, n):
    S = systems(L.kind, n)
    seen = {}
    full = sc.oracle_run(port, L, S, on_progress=lambda k, m, res: seen.__setitem__(k, m) or 0)
    assert full["ret"] == 0
    last = full["iters"]
    assert full["x"].tobytes() == seen[last].tobytes()
    for K in sc.pick_ks(last):
        capped = sc.oracle_run(port, L, S, cap=K)
        assert capped["ret"] == (0 if K == last else -1019) and capped["iters"] == K, (L.name, n, K, capped["ret"], capped["iters"])
        assert capped["x"].tobytes() == seen[K].tobytes(), (L.name, n, K)
        stopped = sc.oracle_run(port, L, S, on_progress=lambda k, m, res: int(k == K))
        assert stopped["ret"] == 1 and stopped["iters"] == K and stopped["ks"] == list(range(K + 1)), (L.name, n, K, stopped["ret"])
        assert stopped["x"].tobytes() == capped["x"].tobytes(), (L.name, n, K)


NAN_CAP = 6     # the loops without a NaN scan of their own (lpg, lspg; clpcg and clpbicg) would spin without a cap


@pytest.mark.parametrize("L,n", SMALL, ids=[f"{L.name}-{n}" for L, n in SMALL])
def test_oracle_nan_stop(port, systems, L, n):
    """A NaN in b reaches the iterate with the first step: the loops that scan for it (lcg.cpp:247-253 and twins) leave in
    iteration 1; the others run to the cap."""
    S = systems(L.kind, n)
    for where in ("first", "last", "mid"):
        r = sc.oracle_run(port, L, S, b=sc.rhs_with_nan(S, where, L), cap=NAN_CAP)
        if L.oracle in ("pg", "spg", "c_pcg", "c_pbicg"):
            assert (r["ret"], r["iters"]) == (-1019, NAN_CAP), (L.name, n, where, r["ret"], r["iters"])
        else:
            # (lbicgstab2 under abs_diff has advanced t a second time, at its mid-iteration test, when the scan runs: lcg.cpp:910-939)
            t = 2 if L.oracle == "bicgstab2" else 1
            assert (r["ret"], r["iters"]) == (-1019 if L.family != "real" else -1017, t), (L.name, n, where, r["ret"], r["iters"])
