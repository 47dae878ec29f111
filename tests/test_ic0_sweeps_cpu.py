"""IC(0) applied by Jacobi sweeps, on the CPU: the C ABI names the two new entries; the sweep checker (tests/ic0_sweeps_checker.py)
reaches the exact row-ordered solve's bits after `levels` sweeps; its rounding stays inside sweep_bound against the same
recurrence in np.longdouble; the k-sweep operator is symmetric; PCG with it reproduces the measured iteration counts."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import ic0_checker as IC
import ic0_sweeps_checker as S

KS = (1, 2, 3, 4, 7)


def test_abi_names_the_sweep_entries():
    from liblcg_amd import _lib
    header = open(os.path.join(ROOT, "include", "lcg_hip.h")).read()
    for name in ("lcg_hip_csr_ic0_set_sweeps", "lcg_hip_csr_ic0_get_sweeps"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name


# ------------------------------------------------------------------------------------------ systems
def _system(name, case10k, case1kc, case10kc):
    if name == "case10k":
        return case10k[1:4]
    if name in ("case1kc", "case10kc", "case1kc64", "case10kc64"):
        rp, ci, v = (case1kc if "1k" in name else case10kc)[1:4]
        return rp, ci, v.astype(np.complex64) if name.endswith("64") else v
    if name == "lap40":
        return S.laplace2d(40)
    if name == "chain":
        return S.chain(300)
    rp, ci, v = S.uneven(name[:-2] if name.endswith("64") else name)
    return rp, ci, v.astype(np.complex64) if name.endswith("64") else v


_factors = {}


def _factor(name, case10k, case1kc, case10kc):
    if name not in _factors:
        _factors[name] = S.factor(*_system(name, case10k, case1kc, case10kc))
    return _factors[name]


# ------------------------------------------------------------------------------------------ 1. levels sweeps = the exact solve
@pytest.mark.parametrize("name", ["case10k", "case1kc", "case10kc", "case1kc64", "lap40", "spd", "chain"])
def test_levels_sweeps_give_the_exact_solves_bits(case10k, case1kc, case10kc, name):
    n, rp, cc, vv = _factor(name, case10k, case1kc, case10kc)
    kind = S.kind_of(vv)
    x = S.random_vector(n, kind, 3)
    for T in S.triangles(n, rp, cc, vv):
        want = S.exact(T, x)
        got = S.sweeps(T, x, T.levels)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (name, T.up, T.levels)
    if name == "case10k":
        assert S.triangles(n, rp, cc, vv)[0].levels == 201


# ------------------------------------------------------------------------------------------ 2. the bound holds for the checker
BOUND_CASES = ["case10k", "spd", "arrow700", "arrow4096", "case1kc", "case10kc", "layered", "carrow700", "carrow4096",
               "case1kc64", "case10kc64", "layered64", "carrow70064", "carrow409664"]


@pytest.mark.parametrize("name", BOUND_CASES)
def test_checker_stays_inside_the_bound(case10k, case1kc, case10kc, name):
    """|checker - the same recurrence in np.longdouble| <= E(k) componentwise, for every which: the bound that the GPU's sweeps are
    held to (2 E(k): both sides round) holds for the reference alone.  which = 2 compares the whole apply in both precisions."""
    n, rp, cc, vv = _factor(name, case10k, case1kc, case10kc)
    kind = S.kind_of(vv)
    wide = "c80" if S.KINDS[kind][1] else "f80"
    x = S.random_vector(n, kind, 4)
    L, LT = S.triangles(n, rp, cc, vv)
    worst = 0.0
    for k in KS:
        lo = {0: S.sweeps(L, x, k), 1: S.sweeps(LT, x, k)}
        hi = {0: S.sweeps(L, x, k, wide), 1: S.sweeps(LT, x, k, wide)}
        lo[2], hi[2] = S.sweeps(LT, lo[0], k), S.sweeps(LT, hi[0], k, wide)
        for which in (0, 1, 2):
            E = S.apply_bound(L, LT, x, k, which)
            err = np.abs(hi[which] - lo[which]).astype(np.float64)
            assert np.all(np.isfinite(E)) and np.all(err <= E), (name, k, which, float(np.max(err / E)))
            worst = max(worst, float(np.max(err / np.maximum(E, 1e-300))))
    print(f"{name}: max |checker - longdouble| / E(k) = {worst:.3f}")


# ------------------------------------------------------------------------------------------ 3. symmetry
@pytest.mark.parametrize("name", ["case10k", "spd", "case1kc"])
def test_the_sweep_operator_is_symmetric(case10k, case1kc, case10kc, name):
    """u.(M^-1 v) = v.(M^-1 u), unconjugated (M^-1 = S^T S: symmetric, complex symmetric for a complex factor).  The two sides
    differ by the applies' rounding, sum_i |u_i| E_i(v) + |v_i| E_i(u), and the two dots' own, (n + 2) u sum_i |u_i| |(M^-1 v)_i|
    + the same with u and v exchanged (complex: x 4, as in the bound)."""
    n, rp, cc, vv = _factor(name, case10k, case1kc, case10kc)
    kind = S.kind_of(vv)
    _, cplx, u = S.KINDS[kind]
    L, LT = S.triangles(n, rp, cc, vv)
    uu, v = S.random_vector(n, kind, 5), S.random_vector(n, kind, 6)
    for k in (1, 2, 3, 5):
        M = S.SweepApply(n, rp, cc, vv, k)
        Mv, Mu = M.mx(v), M.mx(uu)
        lhs, rhs = np.sum(uu * Mv), np.sum(v * Mu)
        tol = np.abs(uu) @ S.apply_bound(L, LT, v, k, 2) + np.abs(v) @ S.apply_bound(L, LT, uu, k, 2)
        tol += (n + 2) * u * (4.0 if cplx else 1.0) * (np.abs(uu) @ np.abs(Mv) + np.abs(v) @ np.abs(Mu))
        assert abs(lhs - rhs) <= tol, (name, k, abs(lhs - rhs), tol)
        assert tol <= 1e-9 * (np.abs(uu) @ np.abs(Mv)), (name, k)      # the statement is not empty


# ------------------------------------------------------------------------------------------ 4. PCG iteration counts
def test_pcg_iteration_counts_on_case10k(case10k):
    """lpcg to eps = 1e-8 on r.r / max(m.m, 1) from m = 0 with the k-sweep operator: the measured row of DESIGN 11's table,
    Jacobi 80, k = 1, 2, 3, 4, 6, 8, 12: 82, 42, 32, 27, 25, 25, 24, exact IC(0) 24."""
    n, rp, ci, v, b, xs = case10k
    A = IC.to_sparse(n, rp, ci, v)
    _, lrp, lc, lv = _factor("case10k", case10k, None, None)
    d = A.diagonal()
    _, jac = IC.lpcg(A, lambda r: r / d, b, 1e-8, 0)
    assert jac == 80
    want = {1: 82, 2: 42, 3: 32, 4: 27, 6: 25, 8: 25, 12: 24, 0: 24}
    got = {}
    for k in want:
        m, got[k] = IC.lpcg(A, S.SweepApply(n, lrp, lc, lv, k).mx, b, 1e-8, 0)
        assert np.abs(m - xs).mean() < 2e-2, k                 # (eps = 1e-8 on r.r / m.m stops early: a sanity check only)
    assert got == want, got
    seq = [got[k] for k in (1, 2, 3, 4, 6, 8, 12, 0)]
    assert all(a >= c for a, c in zip(seq, seq[1:])) and seq[0] > seq[-1]
    # the exact row-ordered solves precondition like SciPy's
    _, ref = IC.lpcg(A, IC.IcApply(IC.to_sparse(n, lrp, lc, lv)).solve, b, 1e-8, 0)
    assert ref == got[0]
