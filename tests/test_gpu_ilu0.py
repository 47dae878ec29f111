"""ILU(0) on the MI355X (csr_ilu0.hip): the device factor against the checker (tests/ilu0_checker.py) and against its own
defining property, the triangular solves against SciPy, the sweep apply against the sweep checker's bound, PCG / PBiCG with
Mfp = ILU(0), right-preconditioned BiCGStab through the A.M^-1 callback, the error paths and the C++ sample.

Right-preconditioned BiCGStab, measured on the MI355X (plain / exact ILU(0) / 4 sweeps iterations, |b - A x| / |b| of the exact
run against the checker's): printed by test_right_bicgstab on every run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import ic0_checker as IC
import ic0_sweeps_checker as S
import ilu0_checker as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
E_ARG = -2003


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------ fixtures
def _host(api, name, case10k, case1kc, case10kc):
    """(rowptr, col, val) of a named test matrix."""
    if name == "case10k":
        return case10k[1:4]
    if name == "case1kc":
        return case1kc[1:4]
    if name == "case10kc":
        return case10kc[1:4]
    if name.startswith("lap2d"):
        nx, ny = map(int, name[5:].split("x"))
        A = api.CsrMatrix.laplace2d(nx, ny)
        out = A.arrays_to_host()
        A.destroy()
        return out
    if name.startswith("convdiff"):
        k, pe = map(int, name[8:].split("_"))
        return K.convdiff(k, pe)
    if name == "generated":
        A = api.CsrMatrix.generate(3000, 4, 30, True, 7, 0.5, pattern=api.GEN_DIAGONALS)
        out = A.arrays_to_host()
        A.destroy()
        return out
    if name == "arrow4096":
        return S.arrow(4096)
    if name == "diagonal":
        n = 5000
        return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), 1.0 + np.arange(n) % 13
    if name == "shuffled_dups":
        return IC.shuffle_split(*K.convdiff(40, 2), seed=11)
    if name == "nonsym_pattern":
        return K.drop_upper(*K.convdiff(48, 1))
    if name == "shifted40":
        return K.shifted(40, 3.5)
    if name == "chain1500":
        return K.chain(1500)
    if name == "cchain1200":
        rp, ci, v = K.chain(1200, seed=8)
        return rp, ci, v * (1.0 + 0.25j) + 0.5j * (ci == np.repeat(np.arange(1200), np.diff(rp)))
    raise KeyError(name)


FACTOR_CASES = ["case10k", "case1kc", "case10kc", "lap2d64x64", "lap2d300x200", "convdiff64_1", "convdiff64_4", "generated",
                "arrow4096", "diagonal", "shuffled_dups", "nonsym_pattern"]


def _device_factor(A):
    return A.ilu0_factor_to_host(0), A.ilu0_factor_to_host(1)


# ------------------------------------------------------------------------------------------ 1, 2. factor
@pytest.mark.parametrize("name", FACTOR_CASES)
def test_factor_matches_checker(api, case10k, case1kc, case10kc, name):
    rp, ci, v = _host(api, name, case10k, case1kc, case10kc)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        info = A.ilu0_info()
        assert info["zero_pivot"] == -1 and info["bytes"] > 0 and info["build_ms"] > 0 and info["sweeps"] == 0
        L, U = _device_factor(A)
        KL, KU, zp = K.ilu0(n, rp, ci, v)
        assert zp == -1
        for got, want in ((L, KL), (U, KU)):
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
        top = max(np.abs(KL[2]).max(initial=0.0), np.abs(KU[2]).max())
        diff = max(np.abs(L[2] - KL[2]).max(initial=0.0), np.abs(U[2] - KU[2]).max())
        print(f"{name}: max |factor - checker| / max |factor| = {diff / top:.2e}")
        assert diff <= 1e-12 * top
        fw, bw = K.levels(n, KL, KU)
        assert (info["levels_L"], info["levels_U"]) == (int(fw.max()) + 1, int(bw.max()) + 1)
    finally:
        A.destroy()


@pytest.mark.parametrize("name", FACTOR_CASES + ["shifted40"])
def test_defining_property(api, case10k, case1kc, case10kc, name):
    """|(L.U - A)(i,j)| <= gamma(t + 1) (|L| |U|)(i,j) on the pattern for the DEVICE's factor (ilu0_checker.residual_check: L.U in
    exact rational arithmetic, nothing in the bound measured)."""
    rp, ci, v = _host(api, name, case10k, case1kc, case10kc)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        L, U = _device_factor(A)
        worst, where, tmax = K.residual_check(n, rp, ci, v, L, U)
        print(f"{name}: worst |L.U - A| / bound = {worst:.3f} at {where}, most products in one sum {tmax}")
        assert worst <= 1.0
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 3. solves
def _random(n, cplx, seed=2):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n) + (1j * rng.uniform(-1, 1, n) if cplx else 0)


@pytest.mark.parametrize("name", ["case10k", "convdiff64_4", "lap2d300x200", "nonsym_pattern", "chain1500", "case10kc"])
def test_solves_match_scipy_and_repeat_bitwise(api, lib, case10k, case1kc, case10kc, name):
    rp, ci, v = _host(api, name, case10k, case1kc, case10kc)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        L, U = _device_factor(A)
        M = K.IluApply(n, L, U)
        x = _random(n, A.is_complex)
        xd = torch.from_numpy(x).cuda()
        info = A.ilu0_info()
        assert info["launches_per_apply"] == K.launches(n, L, U)
        for which in (0, 1, 2):
            ys = [torch.zeros_like(xd) for _ in range(3)]
            for y in ys:
                A.ilu0_solve(xd, y, which)
            torch.cuda.synchronize()
            ref = M.solve(x, which)
            assert np.linalg.norm(ys[0].cpu().numpy() - ref) <= 1e-12 * np.linalg.norm(ref), (name, which)
            assert all(torch.equal(ys[0], y) for y in ys[1:])                  # the same bits on every call
            assert lib.lcg_hip_csr_ilu0_schedule_for_test(A.h, 0) == 0         # one launch per level: the same bits again
            per_level = A.ilu0_info()["launches_per_apply"]
            y0 = torch.zeros_like(xd)
            A.ilu0_solve(xd, y0, which)
            assert lib.lcg_hip_csr_ilu0_schedule_for_test(A.h, -1) == 0
            torch.cuda.synchronize()
            assert torch.equal(y0, ys[0])
            assert per_level == info["levels_L"] + info["levels_U"]
        assert A.ilu0_info()["launches_per_apply"] == info["launches_per_apply"]
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 4. sweeps
@pytest.mark.parametrize("name", ["convdiff64_1", "chain1500", "nonsym_pattern", "arrow4096", "case1kc", "cchain1200"])
def test_sweeps(api, case10k, case1kc, case10kc, name):
    rp, ci, v = _host(api, name, case10k, case1kc, case10kc)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        L, U = _device_factor(A)
        TL, TU = K.triangles(n, L, U)
        info = A.ilu0_info()
        assert (info["levels_L"], info["levels_U"]) == (TL.levels, TU.levels)
        if "chain" in name:
            assert TL.levels == TU.levels == n >= 1000
        x = _random(n, A.is_complex, seed=4)
        xd = torch.from_numpy(x).cuda()
        exact = []
        for which in (0, 1, 2):
            y = torch.zeros_like(xd)
            A.ilu0_solve(xd, y, which)
            exact.append(y)
        # `levels` sweeps: the exact solves' bytes
        for which, k in ((0, TL.levels), (1, TU.levels), (2, max(TL.levels, TU.levels))):
            A.ilu0_set_sweeps(k)
            assert A.ilu0_info()["sweeps"] == k and A.ilu0_info()["launches_per_apply"] == K.sweep_launches(k)
            y = torch.zeros_like(xd)
            A.ilu0_solve(xd, y, which)
            torch.cuda.synchronize()
            assert torch.equal(y, exact[which]), (name, which, k)
        # a few sweeps: within the componentwise rounding bound of the sweep checker on the device's own factor
        for k in (1, 2, 3, 5):
            A.ilu0_set_sweeps(k)
            assert A.ilu0_info()["launches_per_apply"] == K.sweep_launches(k)
            SA = K.SweepApply(n, L, U, k)
            for which in (0, 1, 2):
                y = torch.zeros_like(xd)
                A.ilu0_solve(xd, y, which)
                torch.cuda.synchronize()
                want = SA.solve(x, which)
                E = K.apply_bound(TL, TU, x, k, which)
                excess = np.abs(y.cpu().numpy() - want) - 2.0 * E
                assert excess.max() <= 0.0, (name, k, which, float(excess.max()))
        bytes_sw = A.ilu0_info()["bytes"]
        A.ilu0_set_sweeps(0)
        assert A.ilu0_info()["sweeps"] == 0 and A.ilu0_info()["bytes"] < bytes_sw
        y = torch.zeros_like(xd)
        A.ilu0_solve(xd, y, 2)
        torch.cuda.synchronize()
        assert torch.equal(y, exact[2])
        A.ilu0_set_sweeps(3)
        A.build_ilu0()                                       # every build resets the setting
        assert A.ilu0_info()["sweeps"] == 0
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 5. PCG / PBiCG with Mfp = ILU(0)
def test_pcg_case10k(api, case10k):
    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        bd = torch.from_numpy(b).cuda()
        para = api.lcg_default_parameters(epsilon=1e-10, abs_diff=1)
        m = torch.zeros(n, dtype=torch.float64, device="cuda")
        info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ilu0_mx", None, m, bd, n, para, A)
        KL, KU, _ = K.ilu0(n, rp, ci, v)
        As = IC.to_sparse(n, rp, ci, v)
        M = K.IluApply(n, KL, KU)
        _, iref = K.lpcg(As, M.solve, b, 1e-10, 1)
        print(f"PCG-ILU0 case_10K_A: {info.iterations} iterations, checker {iref}, IC(0) 54")
        assert info.ret == 0 and abs(info.iterations - iref) <= 2 and abs(info.iterations - 54) <= 2
        assert np.abs(m.cpu().numpy() - xs).mean() < 1e-6
        for k in (1, 2, 3, 4):
            mk = torch.zeros_like(m)
            ik = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ilu0_mx", None, mk, bd, n,
                                               api.lcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=k), A)
            want, _ = K.lpcg(As, M.solve, b, 1e-10, 1, max_iterations=k)
            assert ik.iterations == k
            assert np.linalg.norm(mk.cpu().numpy() - want) <= 1e-12 * np.linalg.norm(want)
    finally:
        A.destroy()


@pytest.mark.parametrize("case", ["1K", "10K"])
@pytest.mark.parametrize("solver", ["PCG", "PBICG"])
def test_complex_mfp(api, case1kc, case10kc, case, solver):
    n, rp, ci, v, b, xs = case1kc if case == "1K" else case10kc
    sid = api.CLCG_PCG if solver == "PCG" else api.CLCG_PBICG
    loop = K.clpcg if solver == "PCG" else K.clpbicg
    KL, KU, _ = K.ilu0(n, rp, ci, v)
    As = IC.to_sparse(n, rp, ci, v)
    M = K.IluApply(n, KL, KU)
    _, conv = loop(As, M.solve, b, 1e-10, 1)
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        bd = torch.from_numpy(b).cuda()
        m = torch.zeros(n, dtype=torch.complex128, device="cuda")
        info = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ilu0_mx", None, m, bd, n,
                                              api.clcg_default_parameters(epsilon=1e-10, abs_diff=1), A, sid)
        assert info.ret == 0 and abs(info.iterations - conv) <= 2, (info, conv)
        assert np.linalg.norm(m.cpu().numpy() - xs) <= 1e-5
        for k in range(1, min(4, conv) + 1):
            mk = torch.zeros_like(m)
            ik = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ilu0_mx", None, mk, bd, n,
                                                api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=k), A, sid)
            want, t = loop(As, M.solve, b, 1e-10, 1, max_iterations=k)
            assert ik.iterations == t == k
            assert np.linalg.norm(mk.cpu().numpy() - want) <= 1e-12 * np.linalg.norm(want), (case, solver, k)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 6. the indefinite case
def test_indefinite_ic0_refuses_ilu0_factors(api, lib):
    rp, ci, v = K.shifted(40, 3.5)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        assert lib.lcg_hip_csr_build_ic0(A.h) == E_ARG
        assert "row 1 " in lib.lcg_hip_last_error().decode() and A.ic0_info()["zero_pivot"] == 1
        assert lib.lcg_hip_csr_build_ilu0(A.h) == 0
        assert A.ilu0_info()["zero_pivot"] == -1
        L, U = _device_factor(A)
        worst, where, _ = K.residual_check(n, rp, ci, v, L, U)
        assert worst <= 1.0, (worst, where)
        assert U[2][U[0][:-1]].min() < 0.0                   # negative pivots are fine
    finally:
        A.destroy()


def test_both_factors_on_one_handle(api, case10k):
    """IC(0) and ILU(0) have a slot each: building, setting and rebuilding one leaves the other's results as they were."""
    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        x = torch.from_numpy(b).cuda()
        y = [torch.zeros_like(x) for _ in range(4)]
        A.build_ilu0()
        A.ilu0_solve(x, y[0])
        A.build_ic0()
        A.ic0_solve(x, y[1])
        A.ic0_set_sweeps(2)
        assert A.ilu0_info()["sweeps"] == 0 and A.ic0_info()["sweeps"] == 2
        A.ilu0_solve(x, y[2])
        A.build_ilu0()
        A.ic0_set_sweeps(0)
        A.ic0_solve(x, y[3])
        torch.cuda.synchronize()
        assert torch.equal(y[0], y[2]) and torch.equal(y[1], y[3])
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 7. right-preconditioned BiCGStab
@pytest.mark.parametrize("k,pe", [(64, 1), (64, 4), (100, 2)])
def test_right_bicgstab(api, k, pe):
    rp, ci, v = K.convdiff(k, pe)
    n = k * k
    As = IC.to_sparse(n, rp, ci, v)
    b, xstar = K.rhs(As)
    KL, KU, _ = K.ilu0(n, rp, ci, v)
    _, it_ref, res_ref = K.right_bicgstab(As, K.IluApply(n, KL, KU).solve, b, 1e-10)
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        bd = torch.from_numpy(b).cuda()
        para = api.lcg_default_parameters(epsilon=1e-10)
        m = torch.zeros(n, dtype=torch.float64, device="cuda")
        plain = api.lcg_solver("lcg_hip_csr_ax", None, m, bd, n, para, A, api.LCG_BICGSTAB)
        assert plain.ret == 0

        def run():
            u = torch.zeros(n, dtype=torch.float64, device="cuda")
            x = torch.zeros_like(u)
            info = api.lcg_solver("lcg_hip_csr_ax_ilu0", None, u, bd, n, para, A, api.LCG_BICGSTAB)
            A.ilu0_solve(u, x, 2)
            torch.cuda.synchronize()
            xh = x.cpu().numpy()
            return info, xh, float(np.linalg.norm(b - As @ xh) / np.linalg.norm(b))

        info, xh, res = run()
        print(f"convdiff({k}, {pe}): plain {plain.iterations}, right ILU(0) {info.iterations} (checker {it_ref}), "
              f"|b - A x| / |b| = {res:.3e} (checker {res_ref:.3e}), |x - x*| / |x*| = {np.linalg.norm(xh - xstar) / np.linalg.norm(xstar):.2e}")
        assert info.ret == 0
        assert res <= 10.0 * res_ref
        assert 2 * info.iterations <= plain.iterations
        A.ilu0_set_sweeps(4)
        info4, _, res4 = run()
        print(f"convdiff({k}, {pe}): 4 sweeps {info4.iterations} iterations, |b - A x| / |b| = {res4:.3e}")
        assert info4.ret == 0 and info4.iterations <= plain.iterations
    finally:
        A.destroy()


def test_complex_right_product(api, lib, case1kc):
    n, rp, ci, v, b, xs = case1kc
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        L, U = _device_factor(A)
        x = _random(n, True, seed=9)
        xd = torch.from_numpy(x).cuda()
        y = torch.zeros_like(xd)
        lib.clcg_hip_csr_ax_ilu0(A.h, xd.data_ptr(), y.data_ptr(), n, 0, 0)
        torch.cuda.synchronize()
        want = IC.to_sparse(n, rp, ci, v) @ K.IluApply(n, L, U).solve(x, 2)
        assert np.linalg.norm(y.cpu().numpy() - want) <= 1e-12 * np.linalg.norm(want)
        # and through a loop that asks for (0, 0) only: right-preconditioned complex BiCGStab converges to the _cB solution
        u = torch.zeros_like(xd)
        bd = torch.from_numpy(b).cuda()
        info = api.clcg_solver("clcg_hip_csr_ax_ilu0", None, u, bd, n, api.clcg_default_parameters(epsilon=1e-10, abs_diff=1), A,
                               api.CLCG_BICGSTAB)
        xo = torch.zeros_like(u)
        A.ilu0_solve(u, xo, 2)
        torch.cuda.synchronize()
        assert info.ret == 0 and np.linalg.norm(xo.cpu().numpy() - xs) <= 1e-5
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 8. errors
def test_errors(api, lib, case10k, case1kc):
    from liblcg_amd import _lib
    err = lambda: lib.lcg_hip_last_error().decode()
    assert lib.lcg_hip_csr_build_ilu0(None) == E_ARG
    assert lib.lcg_hip_ilu0_solve(None, 2, None, None) == E_ARG
    assert lib.lcg_hip_csr_ilu0_set_sweeps(None, 1) == E_ARG
    # non-square
    R = api.CsrMatrix.from_csr(np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.array([1.0, 2.0]), n_cols=3)
    assert lib.lcg_hip_csr_build_ilu0(R.h) == E_ARG and "square" in err()
    R.destroy()
    # complex64 handle
    Q = api.CsrMatrix.from_csr_c64(np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([1.0, 2.0], np.complex64))
    assert lib.lcg_hip_csr_build_ilu0(Q.h) == E_ARG and "complex64" in err()
    Q.destroy()
    # sharded
    n, rp, ci, v, b, xs = case10k
    Sh = api.CsrMatrix.generate(8192, 4, 30, True, 7, 0.5, 0, 4096, pattern=api.GEN_DIAGONALS)     # rank 0's rows of two ranks
    assert lib.lcg_hip_csr_split_for_test(Sh.h, 8192, 2, 0) == 0, err()
    assert lib.lcg_hip_csr_build_ilu0(Sh.h) == E_ARG and "sharded" in err()
    Sh.destroy()
    # a zero pivot
    Z = api.CsrMatrix.from_csr(np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, 1.0]))
    assert lib.lcg_hip_csr_build_ilu0(Z.h) == E_ARG and "row 0 " in err()
    assert Z.ilu0_info()["zero_pivot"] == 0
    x2 = torch.ones(2, dtype=torch.float64, device="cuda"); y2 = torch.zeros_like(x2)
    assert lib.lcg_hip_ilu0_solve(Z.h, 2, x2.data_ptr(), y2.data_ptr()) == E_ARG
    assert lib.lcg_hip_csr_ilu0_set_sweeps(Z.h, 1) == E_ARG
    Z.destroy()

    A = api.CsrMatrix.from_csr(rp, ci, v)
    bd = torch.from_numpy(b).cuda()
    m = torch.zeros(n, dtype=torch.float64, device="cuda")
    para = api.lcg_default_parameters(epsilon=1e-10, abs_diff=1)
    ax, ax_ilu, mx_ilu = (_lib.fnptr(lib, s) for s in ("lcg_hip_csr_ax", "lcg_hip_csr_ax_ilu0", "lcg_hip_ilu0_mx"))
    # before a build: the solve entry, the setting and both callbacks
    assert lib.lcg_hip_ilu0_solve(A.h, 2, bd.data_ptr(), m.data_ptr()) == E_ARG and "no factor" in err()
    assert lib.lcg_hip_csr_ilu0_set_sweeps(A.h, 2) == E_ARG
    assert lib.lcg_hip_csr_ilu0_info(A.h, None, None, None, None, None, None) == E_ARG
    assert lib.lcg_hip_solver_preconditioned(ax, mx_ilu, None, m.data_ptr(), bd.data_ptr(), n, para, A.h, api.LCG_PCG, api.MEM_DEVICE) == E_ARG
    assert lib.lcg_hip_solver(ax_ilu, None, m.data_ptr(), bd.data_ptr(), n, para, A.h, api.LCG_BICGSTAB, api.MEM_DEVICE) == E_ARG
    A.build_ilu0()
    assert lib.lcg_hip_ilu0_solve(A.h, 2, bd.data_ptr(), bd.data_ptr()) == E_ARG and "overlap" in err()
    assert lib.lcg_hip_ilu0_solve(A.h, 3, bd.data_ptr(), m.data_ptr()) == E_ARG
    assert lib.lcg_hip_ilu0_solve(A.h, -1, bd.data_ptr(), m.data_ptr()) == E_ARG
    assert lib.lcg_hip_csr_ilu0_set_sweeps(A.h, -1) == E_ARG
    assert lib.lcg_hip_csr_ilu0_factor(A.h, 2, None, None, None) == E_ARG
    # a callback given another n_size ends its solve
    assert lib.lcg_hip_solver(ax_ilu, None, m.data_ptr(), bd.data_ptr(), n - 1, para, A.h, api.LCG_BICGSTAB, api.MEM_DEVICE) == E_ARG
    assert "n_size" in err()
    assert lib.lcg_hip_solver_preconditioned(ax, mx_ilu, None, m.data_ptr(), bd.data_ptr(), n - 1, para, A.h, api.LCG_PCG, api.MEM_DEVICE) == E_ARG
    # the complex callbacks on a real factor
    mc = torch.zeros(n, dtype=torch.complex128, device="cuda"); bc = bd.to(torch.complex128)
    cpara = api.clcg_default_parameters(epsilon=1e-10, abs_diff=1)
    cax, cax_ilu, cmx_ilu = (_lib.fnptr(lib, s) for s in ("clcg_hip_csr_ax", "clcg_hip_csr_ax_ilu0", "clcg_hip_ilu0_mx"))
    assert lib.clcg_hip_solver_preconditioned(cax, cmx_ilu, None, mc.data_ptr(), bc.data_ptr(), n, cpara, A.h, api.CLCG_PCG, api.MEM_DEVICE) == E_ARG
    assert lib.clcg_hip_solver(cax_ilu, None, mc.data_ptr(), bc.data_ptr(), n, cpara, A.h, api.CLCG_BICGSTAB, api.MEM_DEVICE) == E_ARG
    # the parked code does not outlive its solve
    m.zero_()
    assert api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ilu0_mx", None, m, bd, n, para, A).ret == 0
    A.destroy()

    # the real callbacks on a complex factor; conjugate = 1 and layout = 1
    nc, rpc, cic, vc, bcx, _ = case1kc
    Cx = api.CsrMatrix.from_csr(rpc, cic, vc)
    Cx.build_ilu0()
    xr = torch.zeros(nc, dtype=torch.float64, device="cuda"); br = torch.ones(nc, dtype=torch.float64, device="cuda")
    assert lib.lcg_hip_solver(ax_ilu, None, xr.data_ptr(), br.data_ptr(), nc, para, Cx.h, api.LCG_BICGSTAB, api.MEM_DEVICE) == E_ARG
    xd = torch.from_numpy(bcx).cuda(); y = torch.zeros_like(xd)
    for layout, conj in ((0, 1), (1, 0)):
        lib.clcg_hip_ilu0_mx(Cx.h, xd.data_ptr(), y.data_ptr(), nc, layout, conj)
        torch.cuda.synchronize()
        assert "not offered" in err() and not y.any().item()
        lib.clcg_hip_csr_ax_ilu0(Cx.h, xd.data_ptr(), y.data_ptr(), nc, layout, conj)
        torch.cuda.synchronize()
        assert "(0, 0) only" in err() and not y.any().item()
    # BiCG asks its product for A^H: the right-preconditioned product refuses, and the solve ends with the code
    mz = torch.zeros_like(xd)
    assert lib.clcg_hip_solver(cax_ilu, None, mz.data_ptr(), xd.data_ptr(), nc, cpara, Cx.h, api.CLCG_BICG, api.MEM_DEVICE) == E_ARG
    Cx.destroy()
    torch.cuda.synchronize()

    # create -> build_ilu0 -> destroy gives its memory back
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        A = api.CsrMatrix.from_csr(rp, ci, v)
        A.build_ilu0()
        A.ilu0_set_sweeps(2)
        A.build_ilu0()                                       # rebuild on repeat
        A.destroy()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)


# ------------------------------------------------------------------------------------------ 9. C++
def test_cpp_sample(api, case10kc):
    from liblcg_amd import _lib
    _lib.build()
    bindir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "sample_csr_ilu0")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sample_csr_ilu0.cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", exe])
    p = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    it_c = int(re.search(r"PCG-ILU0 \(complex\):.*iterations:\s*(\d+)", p.stdout).group(1))
    err_c = float(re.search(r"PCG-ILU0 \(complex\):.*error:\s*(\S+)", p.stdout).group(1))
    it_p = int(re.search(r"BiCGStab plain:.*iterations:\s*(\d+)", p.stdout).group(1))
    it_r = int(re.search(r"BiCGStab right ILU0:.*iterations:\s*(\d+)", p.stdout).group(1))
    res_r = float(re.search(r"BiCGStab right ILU0:.*residual:\s*(\S+)", p.stdout).group(1))
    # the same runs from Python
    n, rp, ci, v, b, xs = case10kc
    A = api.CsrMatrix.from_csr(rp, ci, v)
    A.build_ilu0()
    m = torch.zeros(n, dtype=torch.complex128, device="cuda")
    info = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ilu0_mx", None, m, torch.from_numpy(b).cuda(), n,
                                          api.clcg_default_parameters(epsilon=1e-10, abs_diff=1), A, api.CLCG_PCG)
    A.destroy()
    assert it_c == info.iterations and err_c <= 1e-5, p.stdout
    rp, ci, v = K.convdiff(64, 1)
    A = api.CsrMatrix.from_csr(rp, ci, v)
    A.build_ilu0()
    nn = 64 * 64
    bd = torch.from_numpy(IC.to_sparse(nn, rp, ci, v) @ (1.0 + (np.arange(nn) % 10) / 10.0)).cuda()
    para = api.lcg_default_parameters(epsilon=1e-10)
    plain = api.lcg_solver("lcg_hip_csr_ax", None, torch.zeros_like(bd), bd, nn, para, A, api.LCG_BICGSTAB)
    right = api.lcg_solver("lcg_hip_csr_ax_ilu0", None, torch.zeros_like(bd), bd, nn, para, A, api.LCG_BICGSTAB)
    A.destroy()
    assert (it_p, it_r) == (plain.iterations, right.iterations) and res_r < 1e-4, p.stdout
