"""The ILU(0) checker against the math it restates (tests/ilu0_checker.py), without a GPU: the defining property within its
rounding bound, agreement with IC(0) on an SPD matrix, the pivot rule, sweeps against the exact solves, and the iteration counts
of right-preconditioned BiCGStab that the GPU tests' conditions rest on."""
import numpy as np
import pytest

from conftest import GOLDEN  # noqa: F401
import ic0_checker as IC
import ic0_sweeps_checker as S
import ilu0_checker as K


def _factor(rp, ci, v):
    n = len(rp) - 1
    L, U, zp = K.ilu0(n, rp, ci, v)
    return n, L, U, zp


@pytest.mark.parametrize("name", ["convdiff24_0", "convdiff24_4", "shifted40", "shuffled_dups", "nonsym_pattern", "case1kc"])
def test_defining_property(case1kc, name):
    if name.startswith("convdiff"):
        k, pe = map(int, name[8:].split("_"))
        rp, ci, v = K.convdiff(k, pe)
    elif name == "shifted40":
        rp, ci, v = K.shifted(40, 3.5)
    elif name == "shuffled_dups":
        rp, ci, v = IC.shuffle_split(*K.convdiff(20, 2), seed=11)
    elif name == "nonsym_pattern":
        rp, ci, v = K.drop_upper(*K.convdiff(24, 1))
    else:
        rp, ci, v = case1kc[1:4]
    n, L, U, zp = _factor(rp, ci, v)
    assert zp == -1
    worst, where, tmax = K.residual_check(n, rp, ci, v, L, U)
    assert worst <= 1.0, (worst, where, tmax)
    # L has no diagonal, U begins with it, both sorted
    for i in range(0, n, max(1, n // 50)):
        lc, uc = L[1][L[0][i]:L[0][i + 1]], U[1][U[0][i]:U[0][i + 1]]
        assert np.all(lc < i) and np.all(np.diff(lc) > 0) and uc[0] == i and np.all(np.diff(uc) > 0)


def test_residual_check_sees_a_wrong_entry():
    rp, ci, v = K.convdiff(12, 1)
    n, L, U, _ = _factor(rp, ci, v)
    U[2][U[0][37] + 1] *= 1.0 + 1e-12
    assert K.residual_check(n, rp, ci, v, L, U)[0] > 1.0


def test_spd_factor_is_ic0s():
    """On an SPD matrix U = D L^T and L.U = (L D^1/2)(L D^1/2)^T, IC(0)'s product, in exact arithmetic."""
    rp, ci, v = S.laplace2d(40)
    n, L, U, zp = _factor(rp, ci, v)
    Kr, Kc, Kv, zpc = IC.ic0(n, rp, ci, v)
    assert zp == zpc == -1
    Lc = IC.to_sparse(n, Kr, Kc, Kv)
    M = K.IluApply(n, L, U)
    d = abs(M.L @ M.U - Lc @ Lc.T).max()
    # an entry of either product is a sum of at most 3 products and at most 4 in magnitude; the factors' own entries come from
    # recurrences as short (relative error of a few u each, both sides, through products and sums): 16 u on a magnitude of 4
    assert d <= 64 * 2.0 ** -53, d


def test_pivot_rule():
    rp, ci, v = K.shifted(40, 3.5)
    n = len(rp) - 1
    assert IC.ic0(n, rp, ci, v)[3] == 1                      # IC(0) refuses: the second pivot is negative
    _, L, U, zp = _factor(rp, ci, v)
    assert zp == -1 and U[2][U[0][:-1]].min() < 0.0 and np.isfinite(U[2]).all()
    assert _factor(np.array([0, 1, 2]), np.array([1, 0]), np.array([1.0, 1.0]))[3] == 0
    assert _factor(np.array([0, 2, 4]), np.array([0, 1, 0, 1]), np.array([1.0, 2.0, 3.0, 6.0]))[3] == 1      # U(1,1) = 6 - 3.2 = 0
    assert _factor(np.array([0, 2, 4]), np.array([0, 1, 0, 1]), np.array([1.0, 2.0, 3.0, 6.0 + 0j]))[3] == 1


@pytest.mark.parametrize("cplx", [False, True])
def test_levels_sweeps_are_the_exact_solves(cplx):
    rp, ci, v = K.drop_upper(*K.convdiff(10, 2))
    if cplx:
        v = v * (1.0 + 0.3j)
    n, L, U, _ = _factor(rp, ci, v)
    TL, TU = K.triangles(n, L, U)
    assert TL.levels > 3 and TU.levels > 3
    x = S.random_vector(n, "c128" if cplx else "f64", 3)
    np.testing.assert_array_equal(S.sweeps(TL, x, 1), x)             # L's first sweep is y = x: dividing by the unit diagonal is exact
    ref = K.IluApply(n, L, U)
    for T, which in ((TL, 0), (TU, 1)):
        ex = S.exact(T, x)
        np.testing.assert_array_equal(S.sweeps(T, x, T.levels), ex)
        np.testing.assert_array_equal(S.sweeps(T, x, T.levels + 2), ex)
        assert np.any(S.sweeps(T, x, T.levels - 1) != ex)
        want = ref.solve(x, which)
        assert np.linalg.norm(ex - want) <= 1e-13 * np.linalg.norm(want)
    for k in (1, 2, 3, 5):
        for which in (0, 1, 2):
            E = K.apply_bound(TL, TU, x, k, which)
            assert np.all(np.isfinite(E)) and np.all(E >= 0)
    assert [K.sweep_launches(k) for k in (1, 2, 3, 4, 8)] == [2, 3, 5, 7, 15]


# iterations of liblcg's BiCGStab restated (eps = 1e-10 on r.r / max(m.m, 1), m = 0, b = A x*, x* uniform in [1, 2], seed 3):
# plain, right ILU(0) exact, k = 2, 3, 4, 6 sweeps.  These are THIS checker's counts; the issue's table came from a prototype
# with another draw of x* and differs from them by at most 6 (71/23/38/29/23/23, 91/21/47/34/28/25, 95/12/48/33/27/19,
# 148/24/74/54/44/31).
COUNTS = {(64, 0): [70, 22, 38, 28, 23, 23], (64, 1): [90, 20, 47, 35, 29, 24], (64, 4): [99, 13, 50, 34, 24, 19],
          (100, 2): [142, 23, 74, 53, 42, 32]}


@pytest.mark.parametrize("k,pe", sorted(COUNTS))
def test_bicgstab_counts(k, pe):
    rp, ci, v = K.convdiff(k, pe)
    n = k * k
    As = IC.to_sparse(n, rp, ci, v)
    b, xs = K.rhs(As)
    _, L, U, zp = _factor(rp, ci, v)
    assert zp == -1 and U[2][U[0][:-1]].min() > 0.0          # an M-matrix: every pivot positive
    got = [K.lbicgstab(lambda x: As @ x, b, 1e-10)[1]]
    x, t, res = K.right_bicgstab(As, K.IluApply(n, L, U).solve, b, 1e-10)
    got.append(t)
    assert res <= 1e-4 and np.linalg.norm(x - xs) <= 1e-3 * np.linalg.norm(xs)
    for s in (2, 3, 4, 6):
        got.append(K.right_bicgstab(As, K.SweepApply(n, L, U, s).solve, b, 1e-10)[1])
    assert got == COUNTS[(k, pe)]
    assert 2 * got[1] <= got[0] and got[4] <= got[0]         # what the GPU test asks of the device runs
