"""ILU(0) (csr_ilu0.hip) where its execution shape depends on the matrix: level schedules that mix wide launches
(one level over many workgroups) and narrow ones (a run of levels inside one workgroup) in both triangles, with U's backward
levels its own and not those of L's transpose, real and complex; the same bits under every grouping of the levels, factor and
solves; the same bits however the rows are stored; pivot failures across workgroups and launches; the sweep kernel on both sides
of its staging window; and PCG / right-preconditioned BiCGStab over whole runs.  Every reference is the checker
(tests/ilu0_checker.py) or SciPy.

Schedules tested (rows per level of L / of U; launches per apply in production, max_merged = 1024):
  convdiff3d40           64,000 rows, 118 / 118 levels, 26 wide in each, 28 + 28 launches
  convdiff3d40_dropped   the same without every third upper entry: L as above, U 118 levels of which 3 wide (widest 1041), 7 launches
  layered_nonsym, _c      9,150 rows, L: 1024 1025 1 1023 3000 1024 5 2048 (6 launches), U: 2048 7 1024 1500 1 1025 1023 2522 in
                         backward order (7 launches); independent patterns; stored unsorted with split duplicates; real, complex
  fuzz20k_nonsym         20,000 rows on two independent random patterns, 71 / 62 levels: 3 / 2 wide at the top, then narrow runs
  window_edges            1,380 rows, 6 / 6 levels, all narrow: made for the sweep kernel (ilu0_checker.window_edges)
"""
import re
import time

import numpy as np
import pytest

from conftest import FUZZ_SEED_OFFSET
import ic0_checker as IC
import ilu0_checker as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
E_ARG = -2003
WG = 1024                                                   # production max_merged
GROUPINGS = (0, 1, 2, 63, 64, 1023, 1024)


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    return _lib.load()


_SYSTEMS = {}


def system(name):
    """(rp, ci, v, checker's L, checker's U, forward levels, backward levels) of a named test matrix, built once."""
    if name not in _SYSTEMS:
        off = FUZZ_SEED_OFFSET
        if name == "convdiff3d40":
            rp, ci, v = K.convdiff3d(40, 2)
        elif name == "convdiff3d40_dropped":
            rp, ci, v = K.drop_upper(*K.convdiff3d(40, 2))
        elif name in ("layered_nonsym", "layered_nonsym_c"):
            rp, ci, v = K.layered_nonsym(K.LAYERS_L, K.LAYERS_U, 41 + off, name.endswith("_c"))
            rp, ci, v = IC.shuffle_split(rp, ci, v, 42 + off)
        elif name == "fuzz20k_nonsym":
            rp, ci, v = K.random_nonsym(20000, 902 + off)
        elif name == "laplace3d40":
            rp, ci, v = IC.laplace3d(40)
        else:
            raise KeyError(name)
        n = len(rp) - 1
        KL, KU, zp = K.ilu0(n, rp, ci, v)
        assert zp == -1
        fw, bw = K.levels(n, KL, KU)
        if name.startswith("layered"):                          # the generator made the schedules asked for
            assert list(IC.widths(fw)) == K.LAYERS_L and list(IC.widths(bw)) == K.LAYERS_U
        _SYSTEMS[name] = (rp, ci, v, KL, KU, fw, bw)
    return _SYSTEMS[name]


SCHEDULED = ["convdiff3d40", "convdiff3d40_dropped", "layered_nonsym", "layered_nonsym_c", "fuzz20k_nonsym"]


def launches(fw, bw, max_merged):
    return IC.segments(IC.widths(fw), max_merged) + IC.segments(IC.widths(bw), max_merged)


def rhs(n, cplx, seed):
    rng = np.random.default_rng(seed + FUZZ_SEED_OFFSET)
    return rng.uniform(-1, 1, n) + (1j * rng.uniform(-1, 1, n) if cplx else 0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind == "i" else a.view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def device_factor(A):
    return A.ilu0_factor_to_host(0), A.ilu0_factor_to_host(1)


def device_solves(A, x):
    xd = torch.from_numpy(x).cuda()
    out = []
    for which in (0, 1, 2):
        y = torch.zeros_like(xd)
        A.ilu0_solve(xd, y, which)
        out.append(y)
    torch.cuda.synchronize()
    return [y.cpu().numpy() for y in out]


# ------------------------------------------------------------------------------------------ 1. mixed schedules
@pytest.mark.parametrize("name", SCHEDULED)
def test_mixed_schedule_factor_and_solves(api, name):
    """The factor on a schedule of wide and narrow launches that read each other's rows, against the checker (pattern, levels,
    launches, values) and against its own defining property |(L.U - A)(i,j)| <= gamma(t + 1) (|L| |U|)(i,j) (a theorem bound,
    L.U exact); the three solves against SciPy on the device's factor."""
    rp, ci, v, KL, KU, fw, bw = system(name)
    n = len(rp) - 1
    wf, wb = IC.widths(fw), IC.widths(bw)
    # the point of these matrices: wide levels and narrow runs in both triangles
    for w in (wf, wb):
        assert (w > WG).any() and (w <= WG).any() and IC.segments(w, WG) >= 2, (name, list(w))
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        info = A.ilu0_info()
        assert (info["levels_L"], info["levels_U"]) == (len(wf), len(wb))
        assert info["launches_per_apply"] == launches(fw, bw, WG) == K.launches(n, KL, KU)
        assert info["zero_pivot"] == -1
        L, U = device_factor(A)
        for got, want in ((L, KL), (U, KU)):
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
        top = max(np.abs(KL[2]).max(), np.abs(KU[2]).max())
        diff = max(np.abs(L[2] - KL[2]).max(), np.abs(U[2] - KU[2]).max())
        assert diff <= 1e-12 * top, (name, diff, top)              # test_gpu_ilu0.test_factor_matches_checker's tolerance
        worst, where, tmax = K.residual_check(n, rp, ci, v, L, U)
        print(f"{name}: max |factor - checker| / max |factor| = {diff / top:.2e}; worst |L.U - A| / bound = {worst:.3f} at {where}, "
              f"most products in one sum {tmax}")
        assert worst <= 1.0, (name, worst, where)
        M = K.IluApply(n, L, U)
        x = rhs(n, A.is_complex, 3)
        for which, got in enumerate(device_solves(A, x)):
            ref = M.solve(x, which)
            # test_gpu_ilu0.test_solves_match_scipy_and_repeat_bitwise's tolerance
            assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref), (name, which)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 2. every grouping
@pytest.mark.parametrize("name", SCHEDULED)
def test_every_grouping_same_bits(api, lib, name):
    """A rebuild keeps the grouping set on the handle, so the factor kernels run under it too: the factor and the three solves
    have the default grouping's bits under every one."""
    rp, ci, v, KL, KU, fw, bw = system(name)
    n = len(rp) - 1
    x = rhs(n, np.iscomplexobj(v), 4)
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        assert A.ilu0_info()["launches_per_apply"] == launches(fw, bw, WG)         # a fresh handle starts at 1024
        f0 = device_factor(A)
        y0 = device_solves(A, x)
        try:
            for mm in GROUPINGS:
                assert lib.lcg_hip_csr_ilu0_schedule_for_test(A.h, mm) == 0
                A.build_ilu0()
                assert A.ilu0_info()["launches_per_apply"] == launches(fw, bw, mm) == K.launches(n, KL, KU, mm), (name, mm)
                f = device_factor(A)
                for t, t0 in zip(f, f0):
                    for a, b in zip(t, t0):
                        assert same_bits(a, b), (name, mm)
                for which, (y, ref) in enumerate(zip(device_solves(A, x), y0)):
                    assert same_bits(y, ref), (name, mm, which)
        finally:
            assert lib.lcg_hip_csr_ilu0_schedule_for_test(A.h, -1) == 0
        assert A.ilu0_info()["launches_per_apply"] == launches(fw, bw, WG)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 3. storage order
@pytest.mark.parametrize("cplx", [False, True])
def test_storage_order_does_not_matter(api, cplx):
    """Rows sorted and rows in random order (no duplicates) give the same factor and solves to the bit; entries split in two give
    the same pattern and a factor within residual_check, whose `dup` term covers the build's sum of the halves."""
    rp, ci, v = K.layered_nonsym(K.LAYERS_L, K.LAYERS_U, 41 + FUZZ_SEED_OFFSET, cplx)
    n = len(rp) - 1
    x = rhs(n, cplx, 5)
    stored = {"sorted": (rp, ci, v), "permuted": IC.shuffle_split(rp, ci, v, 46 + FUZZ_SEED_OFFSET, split=0.0),
              "split": system("layered_nonsym_c" if cplx else "layered_nonsym")[:3]}
    assert len(stored["permuted"][1]) == len(ci) and np.any(stored["permuted"][1] != ci) and len(stored["split"][1]) > len(ci)
    got = {}
    for tag, (r, c, w) in stored.items():
        A = api.CsrMatrix.from_csr(r, c, w)
        try:
            A.build_ilu0()
            got[tag] = (device_factor(A), device_solves(A, x))
        finally:
            A.destroy()
    (L0, U0), y0 = got["sorted"]
    (L1, U1), y1 = got["permuted"]
    for t, t0 in ((L1, L0), (U1, U0)):
        for a, b in zip(t, t0):
            assert same_bits(a, b)
    for which in (0, 1, 2):
        assert same_bits(y1[which], y0[which]), which
    (L2, U2), _ = got["split"]
    for t, t0 in ((L2, L0), (U2, U0)):
        np.testing.assert_array_equal(t[0], t0[0])
        np.testing.assert_array_equal(t[1], t0[1])
    worst, where, _ = K.residual_check(n, *stored["split"], L2, U2)
    assert worst <= 1.0, (worst, where)


# ------------------------------------------------------------------------------------------ 4. pivot failures
@pytest.mark.parametrize("case", K.PIVOT_CASES)
def test_pivot_failure(api, lib, case):
    """atomicMin over workgroups and launches reports the smallest failing row; the factor loop finishes although later rows
    divide by the bad pivot; every apply refuses; a new handle with the value repaired builds."""
    from liblcg_amd import _lib
    (rp, ci, v), want, good = K.pivot_case(case, 45 + FUZZ_SEED_OFFSET)
    n = len(rp) - 1
    cplx = np.iscomplexobj(v)
    assert K.ilu0(n, rp, ci, v)[2] == want                       # before any GPU call: the checker names the row
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        assert lib.lcg_hip_csr_build_ilu0(A.h) == E_ARG
        msg = lib.lcg_hip_last_error().decode()
        assert [int(s) for s in re.findall(r"row (\d+)", msg)] == [want], msg
        assert A.ilu0_info()["zero_pivot"] == want
        dt = torch.complex128 if cplx else torch.float64
        x = torch.ones(n, dtype=dt, device="cuda")
        y = torch.zeros_like(x)
        assert lib.lcg_hip_ilu0_solve(A.h, 2, x.data_ptr(), y.data_ptr()) == E_ARG
        assert lib.lcg_hip_csr_ilu0_set_sweeps(A.h, 2) == E_ARG
        m = torch.zeros_like(x)
        if cplx:
            para = api.clcg_default_parameters(epsilon=1e-10, abs_diff=1)
            rc = lib.clcg_hip_solver_preconditioned(_lib.fnptr(lib, "clcg_hip_csr_ax"), _lib.fnptr(lib, "clcg_hip_ilu0_mx"), None,
                                                    m.data_ptr(), x.data_ptr(), n, para, A.h, api.CLCG_PCG, api.MEM_DEVICE)
            rb = lib.clcg_hip_solver(_lib.fnptr(lib, "clcg_hip_csr_ax_ilu0"), None, m.data_ptr(), x.data_ptr(), n, para, A.h,
                                     api.CLCG_BICGSTAB, api.MEM_DEVICE)
        else:
            para = api.lcg_default_parameters(epsilon=1e-10, abs_diff=1)
            rc = lib.lcg_hip_solver_preconditioned(_lib.fnptr(lib, "lcg_hip_csr_ax"), _lib.fnptr(lib, "lcg_hip_ilu0_mx"), None,
                                                   m.data_ptr(), x.data_ptr(), n, para, A.h, api.LCG_PCG, api.MEM_DEVICE)
            rb = lib.lcg_hip_solver(_lib.fnptr(lib, "lcg_hip_csr_ax_ilu0"), None, m.data_ptr(), x.data_ptr(), n, para, A.h,
                                    api.LCG_BICGSTAB, api.MEM_DEVICE)
        assert (rc, rb) == (E_ARG, E_ARG)
        torch.cuda.synchronize()
        assert not y.any().item()                                # no answer was written
    finally:
        A.destroy()
    # repaired, through a new handle: nothing of the failure is left behind
    rp, ci, v = good
    KL, KU, zp = K.ilu0(n, rp, ci, v)
    assert zp == -1
    B = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        assert lib.lcg_hip_csr_build_ilu0(B.h) == 0, lib.lcg_hip_last_error().decode()
        assert B.ilu0_info()["zero_pivot"] == -1
        L, U = device_factor(B)
        for got, ref in ((L, KL), (U, KU)):
            np.testing.assert_array_equal(got[1], ref[1])
        top = max(np.abs(KL[2]).max(), np.abs(KU[2]).max())
        assert max(np.abs(L[2] - KL[2]).max(), np.abs(U[2] - KU[2]).max()) <= 1e-12 * top      # test 1's tolerance
        xh = rhs(n, cplx, 7)
        ref = K.IluApply(n, L, U).solve(xh, 2)
        assert np.linalg.norm(device_solves(B, xh)[2] - ref) <= 1e-12 * np.linalg.norm(ref)   # test 1's tolerance
    finally:
        B.destroy()


# ------------------------------------------------------------------------------------------ 5. the sweep kernel's window
@pytest.mark.parametrize("cplx", [False, True])
def test_sweep_window_edges(api, cplx):
    """k_ic_sweep stages a workgroup's slice when cnt = rowptr[row0 + nrows] - (rowptr[row0] & ~3) <= 2048 and walks global memory
    otherwise: workgroups on both sides of that edge, in L (no diagonal, empty rows) and in U (diagonal first), read off the
    DEVICE's row pointers.  `levels` sweeps are the exact solves to the bit; k sweeps are within twice the sweep checker's
    componentwise bound (test_gpu_ilu0.test_sweeps' bound)."""
    rp, ci, v = K.window_edges(5 + FUZZ_SEED_OFFSET, cplx)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        L, U = device_factor(A)
        for name, T, more in (("L", L, {"all_rows_empty"}), ("U", U, set())):
            found = K.window_cases(n, T[0])
            print(f"window_edges {'c128' if cplx else 'f64'} {name}: (own, cnt, rowptr[row0] & 3) = {K.sweep_windows(n, T[0])}")
            assert found >= K.WINDOW_SET | more, (name, found)       # this test's own coverage
        TL, TU = K.triangles(n, L, U)
        assert A.ilu0_info()["levels_L"] == TL.levels <= 8 and A.ilu0_info()["levels_U"] == TU.levels <= 8
        x = rhs(n, cplx, 8)
        xd = torch.from_numpy(x).cuda()
        exact = []
        for which in (0, 1, 2):
            y = torch.zeros_like(xd)
            A.ilu0_solve(xd, y, which)
            exact.append(y)
        for which, k in ((0, TL.levels), (1, TU.levels), (2, max(TL.levels, TU.levels))):
            A.ilu0_set_sweeps(k)
            ys = [torch.zeros_like(xd) for _ in range(2)]
            for y in ys:
                A.ilu0_solve(xd, y, which)
            torch.cuda.synchronize()
            assert torch.equal(ys[0], exact[which]), (which, k)
            assert torch.equal(ys[0], ys[1])
        for k in (1, 2, 3, 5):
            A.ilu0_set_sweeps(k)
            assert A.ilu0_info()["launches_per_apply"] == K.sweep_launches(k)
            SA = K.SweepApply(n, L, U, k)
            for which in (0, 1, 2):
                ys = [torch.zeros_like(xd) for _ in range(2)]
                for y in ys:
                    A.ilu0_solve(xd, y, which)
                torch.cuda.synchronize()
                want = SA.solve(x, which)
                E = K.apply_bound(TL, TU, x, k, which)
                excess = np.abs(ys[0].cpu().numpy() - want) - 2.0 * E
                assert excess.max() <= 0.0, (k, which, float(excess.max()))
                assert torch.equal(ys[0], ys[1]), (k, which)                  # a second call returns the same bits
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 6. whole runs
def test_pcg_whole_run(api):
    """PCG with Mfp = ILU(0) on the 40^3 Laplacian (symmetric: ILU(0) is IC(0)'s operator there, so lpcg with IluApply is the
    reference), by test_gpu_ic0_schedules.test_pcg_whole_run's rule: the count within 2 of the checker's, the distance to x* within
    10 x the checker's, the capped iterates at k = 8, 16, 32 and two short of the stop within max(1e-12, 50 x the checker's own
    response to 1e-16 relative changes of b)."""
    rp, ci, v, KL, KU, _, _ = system("laplace3d40")
    n = len(rp) - 1
    eps = 1e-10
    As = IC.to_sparse(n, rp, ci, v)
    xt = rhs(n, False, 6)
    b = As @ xt
    M = K.IluApply(n, KL, KU)
    mconv, conv = K.lpcg(As, M.solve, b, eps, 1)
    ks = [k for k in (8, 16, 32) if k < conv - 2] + [conv - 2]
    ref = dict.fromkeys(ks)
    K.lpcg(As, M.solve, b, eps, 1, snap=ref)
    sens = dict.fromkeys(ks, 0.0)
    for s in range(2):                                          # the checker's own response to 1e-16 relative changes of b
        bp = b * (1.0 + 1e-16 * np.random.default_rng(1000 + s).standard_normal(n))
        got = dict.fromkeys(ks)
        K.lpcg(As, M.solve, bp, eps, 1, snap=got)
        for k in ks:
            sens[k] = max(sens[k], np.linalg.norm(got[k] - ref[k]) / np.linalg.norm(ref[k]))
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        bd = torch.from_numpy(b).cuda()
        m = torch.zeros(n, dtype=torch.float64, device="cuda")
        info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ilu0_mx", None, m, bd, n,
                                             api.lcg_default_parameters(epsilon=eps, abs_diff=1), A)
        assert info.ret == 0 and abs(info.iterations - conv) <= 2, (info, conv)
        assert np.linalg.norm(m.cpu().numpy() - xt) <= 10 * max(np.linalg.norm(mconv - xt), 1e-14 * np.linalg.norm(xt))
        for k in ks:
            mk = torch.zeros_like(m)
            ik = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ilu0_mx", None, mk, bd, n,
                                               api.lcg_default_parameters(epsilon=eps, abs_diff=1, max_iterations=k), A)
            assert ik.iterations == k
            d = np.linalg.norm(mk.cpu().numpy() - ref[k]) / np.linalg.norm(ref[k])
            print(f"PCG-ILU0 laplace3d40 k = {k} of {conv}: |m - checker| / |checker| = {d:.2e}, band {max(1e-12, 50.0 * sens[k]):.2e}")
            assert d <= max(1e-12, 50.0 * sens[k]), (k, d, sens[k])
    finally:
        A.destroy()


@pytest.mark.parametrize("name,eps", [("convdiff3d40", 1e-10), ("layered_nonsym", 1e-20)])
def test_right_bicgstab_whole_run(api, name, eps):
    """Right-preconditioned BiCGStab (Afp = lcg_hip_csr_ax_ilu0, u from 0, x = U^-1 L^-1 u) against the checker's lbicgstab on
    A.M^-1, by test_pcg_whole_run's rule and constants.  BiCGStab's count wanders more than PCG's: the band is 2 while the checker's
    own counts for its two perturbed right-hand sides stay within 2 of its unperturbed one, else what conftest.check_converged_run
    gives its `wide` loops, max(3, 4 x that spread, 0.3 x the count).  layered_nonsym is strictly dominant and its ILU(0) nearly
    exact: to eps = 1e-10 it takes two iterations and leaves no iterate to compare, so it runs to 1e-20."""
    rp, ci, v, KL, KU, _, _ = system(name)
    n = len(rp) - 1
    As = IC.to_sparse(n, rp, ci, v)
    xt = rhs(n, False, 6)
    b = As @ xt
    M = K.IluApply(n, KL, KU)
    op = lambda u: As @ M.solve(u)
    uconv, conv = K.lbicgstab(op, b, eps)
    xconv = M.solve(uconv)
    ks = [k for k in (8, 16, 32) if k < conv - 2] + ([conv - 2] if conv > 2 else [])
    assert ks, conv
    ref = {k: K.lbicgstab(op, b, eps, k)[0] for k in ks}
    sens, dit = dict.fromkeys(ks, 0.0), 0
    for s in range(2):                                          # the checker's own response to 1e-16 relative changes of b
        bp = b * (1.0 + 1e-16 * np.random.default_rng(1000 + s).standard_normal(n))
        dit = max(dit, abs(K.lbicgstab(op, bp, eps)[1] - conv))
        for k in ks:
            sens[k] = max(sens[k], np.linalg.norm(K.lbicgstab(op, bp, eps, k)[0] - ref[k]) / np.linalg.norm(ref[k]))
    band = 2 if dit <= 2 else max(3, 4 * dit, 0.3 * conv)
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        bd = torch.from_numpy(b).cuda()

        def run(cap):
            u = torch.zeros(n, dtype=torch.float64, device="cuda")
            info = api.lcg_solver("lcg_hip_csr_ax_ilu0", None, u, bd, n, api.lcg_default_parameters(epsilon=eps, max_iterations=cap), A,
                                  api.LCG_BICGSTAB)
            return info, u

        info, u = run(0)
        x = torch.zeros_like(u)
        A.ilu0_solve(u, x, 2)
        torch.cuda.synchronize()
        print(f"right BiCGStab {name}: {info.iterations} iterations (checker {conv}, its spread {dit}, band {band})")
        assert info.ret == 0 and abs(info.iterations - conv) <= band, (info, conv, band)
        assert np.linalg.norm(x.cpu().numpy() - xt) <= 10 * max(np.linalg.norm(xconv - xt), 1e-14 * np.linalg.norm(xt))
        for k in ks:
            ik, uk = run(k)
            assert ik.iterations == k
            d = np.linalg.norm(uk.cpu().numpy() - ref[k]) / np.linalg.norm(ref[k])
            print(f"right BiCGStab {name} k = {k} of {conv}: |u - checker| / |checker| = {d:.2e}, band {max(1e-12, 50.0 * sens[k]):.2e}")
            assert d <= max(1e-12, 50.0 * sens[k]), (name, k, d, sens[k])
    finally:
        A.destroy()


@pytest.mark.parametrize("sweeps", [0, 4])
def test_early_convergence_with_and_without_progress_callback(api, case10k, sweeps):
    """A solve that converges leaves the same iterate and count whether or not a progress callback forces a synchronisation in
    every iteration: the solves (k_lvl_wide / _narrow over TriSolveRow) and sweeps launched after the stop see the done flag and write
    nothing."""
    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ilu0()
        A.ilu0_set_sweeps(sweeps)
        bd = torch.from_numpy(b).cuda()
        para = api.lcg_default_parameters(epsilon=1e-10, abs_diff=1)
        m = torch.zeros(n, dtype=torch.float64, device="cuda")
        info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ilu0_mx", None, m, bd, n, para, A)
        seen = []

        def progress(inst, mp, res, para_p, nn, k):
            seen.append(k)
            return 0
        mp = torch.zeros_like(m)
        ip = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ilu0_mx", progress, mp, bd, n, para, A)
        assert info.ret == ip.ret == 0 and ip.iterations == info.iterations == max(seen), (info, ip)
        assert torch.equal(m, mp)
    finally:
        A.destroy()
