"""IC(0) (csr_ic0.hip) where its execution shape depends on the matrix: level schedules that mix wide launches
(one level over many workgroups) and narrow ones (a run of levels inside one workgroup) in both triangles, real and complex;
the same bits under every grouping of the levels; the pattern rules (upper triangle ignored) on the device; pivot failures;
and PCG / PBiCG preconditioned by it over whole runs.  Every reference is the checker (tests/ic0_checker.py) or SciPy.

Schedules tested (rows per level of L / L^T; launches per apply in production, max_merged = 1024):
  laplace3d(40)   64,000 rows, 118 / 118 levels, 26 wide in each, 56 launches
  layered          9,150 rows, L: 1024 1025 1 1023 3000 1024 5 2048 (6 launches), L^T: 3 wide levels then a narrow run
                  (4 launches); stored unsorted with split duplicates; real and complex
  fuzz20k         20,000 rows on a random pattern, about 70 levels per triangle: 2-3 wide at the top, then narrow runs
"""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import FUZZ_SEED_OFFSET
import ic0_checker as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
E_ARG = -2003
WG = 1024                                                   # production max_merged
GROUPINGS = (0, 1, 2, 63, 64, 1023, 1024)
LAYERS = [1024, 1025, 1, 1023, 3000, 1024, 5, 2048]


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
    """(rp, ci, v, levels forward, levels backward, checker factor (rp, ci, v)) of a named test matrix, built once."""
    if name not in _SYSTEMS:
        if name == "laplace3d40":
            rp, ci, v = K.laplace3d(40)
        elif name in ("layered", "layered_c"):
            rp, ci, v = K.layered(LAYERS, 41 + FUZZ_SEED_OFFSET, name == "layered_c")
            rp, ci, v = K.shuffle_split(rp, ci, v, 42 + FUZZ_SEED_OFFSET)
        elif name == "fuzz20k":
            rp, ci, v = K.random_spd(20000, 902 + FUZZ_SEED_OFFSET)
        n = len(rp) - 1
        fw, bw = K.levels(n, rp, ci)
        Lr, Lc, Lv, zp = K.ic0(n, rp, ci, v)
        assert zp == -1
        if name.startswith("layered"):
            assert list(K.widths(fw)) == LAYERS                 # the generator made the schedule asked for
        _SYSTEMS[name] = (rp, ci, v, fw, bw, (Lr, Lc, Lv))
    return _SYSTEMS[name]


SCHEDULED = ["laplace3d40", "layered", "layered_c", "fuzz20k"]


def launches(fw, bw, max_merged):
    return K.segments(K.widths(fw), max_merged) + K.segments(K.widths(bw), max_merged)


def rhs(n, cplx, seed):
    rng = np.random.default_rng(seed + FUZZ_SEED_OFFSET)
    return rng.uniform(-1, 1, n) + (1j * rng.uniform(-1, 1, n) if cplx else 0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64)


def device_solves(A, x):
    xd = torch.from_numpy(x).cuda()
    out = []
    for which in (0, 1, 2):
        y = torch.zeros_like(xd)
        A.ic0_solve(xd, y, which)
        out.append(y)
    torch.cuda.synchronize()
    return [y.cpu().numpy() for y in out]


# ------------------------------------------------------------------------------------------ 3. mixed schedules
@pytest.mark.parametrize("name", SCHEDULED)
def test_mixed_schedule_factor_and_solves(api, name):
    rp, ci, v, fw, bw, (Kr, Kc, Kv) = system(name)
    n = len(rp) - 1
    wf, wb = K.widths(fw), K.widths(bw)
    # the point of these matrices: wide levels and narrow runs in both triangles
    for w in (wf, wb):
        assert (w > WG).any() and (w <= WG).any() and K.segments(w, WG) >= 2, (name, list(w))
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ic0()
        info = A.ic0_info()
        assert (info["levels_lower"], info["levels_upper"]) == (len(wf), len(wb))
        assert info["launches_per_apply"] == launches(fw, bw, WG)
        assert info["zero_pivot"] == -1
        Lr, Lc, Lv = A.ic0_factor_to_host()
        np.testing.assert_array_equal(Lr, Kr)
        np.testing.assert_array_equal(Lc, Kc)
        assert np.abs(Lv - Kv).max() <= 1e-12 * np.abs(Kv).max()
        M = K.IcApply(K.to_sparse(n, Lr, Lc, Lv))
        x = rhs(n, A.is_complex, 3)
        for which, got in enumerate(device_solves(A, x)):
            ref = M.solve(x, which)
            assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref), (name, which)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 4. every grouping
@pytest.mark.parametrize("name", SCHEDULED)
def test_every_grouping_same_bits(api, lib, name):
    rp, ci, v, fw, bw, _ = system(name)
    n = len(rp) - 1
    x = rhs(n, np.iscomplexobj(v), 4)
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ic0()
        f0 = A.ic0_factor_to_host()
        y0 = device_solves(A, x)
        try:
            for mm in GROUPINGS:
                assert lib.lcg_hip_csr_ic0_schedule_for_test(A.h, mm) == 0
                A.build_ic0()                               # a rebuild keeps the grouping: the factor runs under it too
                assert A.ic0_info()["launches_per_apply"] == launches(fw, bw, mm), (name, mm)
                f = A.ic0_factor_to_host()
                for a, b in zip(f, f0):
                    assert np.array_equal(a, b) if a.dtype.kind == "i" else np.array_equal(bits(a), bits(b)), (name, mm)
                for which, (y, ref) in enumerate(zip(device_solves(A, x), y0)):
                    assert np.array_equal(bits(y), bits(ref)), (name, mm, which)
        finally:
            assert lib.lcg_hip_csr_ic0_schedule_for_test(A.h, -1) == 0
        assert A.ic0_info()["launches_per_apply"] == launches(fw, bw, WG)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 5. pattern rules
def _with_upper_garbage(n, lower, diag, seed):
    """The lower triangle of (lower, diag) plus an upper triangle that mirrors nothing: other values on the mirrored places,
    extra columns and duplicates; every row stored in random order."""
    rng = np.random.default_rng(seed)
    cplx = np.iscomplexobj(diag)
    rows = [[(j, x) for j, x in lower[i].items()] + [(i, diag[i])] for i in range(n)]
    for i in range(n):
        for j in lower[i]:
            if rng.uniform() < 0.5:
                rows[j].append((i, 3.0 * rng.uniform(-1, 1) + (1j if cplx else 0) * rng.uniform(-1, 1)))
        for j in rng.integers(i + 1, n + 1, size=int(rng.integers(0, 3))):
            if j < n:
                rows[i].append((int(j), -50.0 + (7j if cplx else 0)))
                if rng.uniform() < 0.5:
                    rows[i].append((int(j), 1e3))            # a duplicate up there too
    rp, ci, v = [0], [], []
    for r in rows:
        for q in rng.permutation(len(r)):
            ci.append(r[q][0]); v.append(r[q][1])
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(v, np.complex128 if cplx else np.float64)


def _factor_of(api, rp, ci, v):
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ic0()
        return A.ic0_factor_to_host()
    finally:
        A.destroy()


@pytest.mark.parametrize("cplx", [False, True])
def test_upper_triangle_is_ignored_on_device(api, cplx):
    lower, diag, _ = K.layered_parts(LAYERS, 43 + FUZZ_SEED_OFFSET, cplx)
    n = len(diag)
    lo = K.assemble(n, lower, diag, upper=False)
    want = _factor_of(api, *lo)
    Kr, Kc, Kv, zp = K.ic0(n, *lo)
    assert zp == -1 and np.array_equal(want[1], Kc)
    assert np.abs(want[2] - Kv).max() <= 1e-12 * np.abs(Kv).max()
    got = _factor_of(api, *_with_upper_garbage(n, lower, diag, 44 + FUZZ_SEED_OFFSET))
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert np.array_equal(bits(got[2]), bits(want[2]))
    # stored as its upper triangle only: nothing below the diagonal, so L is the diagonal's square roots
    up = [dict() for _ in range(n)]
    for i in range(n):
        for j, x in lower[i].items():
            up[j][i] = x
    rows = [sorted(list(up[i].items()) + [(i, diag[i])]) for i in range(n)]
    rp = np.array([0] + list(np.cumsum([len(r) for r in rows])), np.int32)
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    v = np.array([x for r in rows for _, x in r], diag.dtype)
    Lr, Lc, Lv = _factor_of(api, rp, ci, v)
    np.testing.assert_array_equal(Lr, np.arange(n + 1))
    np.testing.assert_array_equal(Lc, np.arange(n))
    np.testing.assert_allclose(Lv, np.sqrt(diag), rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------ 6. pivot failures
def _pivot_case(case):
    """(rp, ci, v, the row whose pivot fails first by row number)."""
    off = FUZZ_SEED_OFFSET
    if case == "larger_row_first_in_time":
        # laplace3d(40): row 1600 = (1, 0, 0) is on level 1, row 39 = (0, 0, 39) on level 39: the larger row fails launches earlier
        rp, ci, v = K.laplace3d(40)
        v = v.copy()
        for r in (1600, 39):
            v[rp[r] + np.nonzero(ci[rp[r]:rp[r + 1]] == r)[0][0]] = -2.0
        return rp, ci, v, 39
    lower, diag, st = K.layered_parts(LAYERS, 45 + off, case == "complex_zero")
    n = len(diag)
    drop = None
    if case == "two_in_wide_level":             # level 4: 3000 rows, 12 workgroups; the failing rows in the first and the last
        diag[st[4] + 2950] = -1.0
        diag[st[4] + 100] = -4.0
        want = st[4] + 100
    elif case == "narrow_run":                  # level 3 (1023 rows) in the narrow run of levels 2-3
        want = st[3] + 500
        diag[want] = -1.0
    elif case == "empty_row":                   # nothing stored: its diagonal is the explicit zero the extraction puts there
        want = drop = st[5] + 10
    elif case == "nan_value":                   # a NaN below the diagonal in a wide level
        want = st[4] + 7
        lower[want][next(iter(lower[want]))] = np.nan
    elif case == "complex_zero":                # L(j,j) = sqrt(4) = 2, L(i,j) = 2 / 2 = 1, pivot 1 - 1*1 = 0 exactly
        want, j = st[1] + 3, st[0] + 5
        lower[want] = {j: 2.0 + 0j}
        diag[j], diag[want] = 4.0 + 0j, 1.0 + 0j
    rp, ci, v = K.assemble(n, lower, diag)
    if drop is not None:
        keep = np.ones(len(ci), bool)
        keep[rp[drop]:rp[drop + 1]] = False
        rp = np.concatenate([rp[:drop + 1], rp[drop + 1:] - (rp[drop + 1] - rp[drop])]).astype(np.int32)
        ci, v = ci[keep], v[keep]
    return rp, ci, v, int(want)


@pytest.mark.parametrize("case", ["two_in_wide_level", "larger_row_first_in_time", "narrow_run", "empty_row", "nan_value",
                                  "complex_zero"])
def test_pivot_failure(api, lib, case):
    from liblcg_amd import _lib
    rp, ci, v, want = _pivot_case(case)
    n = len(rp) - 1
    cplx = np.iscomplexobj(v)
    with np.errstate(all="ignore"):
        assert K.ic0(n, rp, ci, v)[3] == want
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        assert lib.lcg_hip_csr_build_ic0(A.h) == E_ARG
        msg = lib.lcg_hip_last_error().decode()
        assert [int(s) for s in re.findall(r"row (\d+)", msg)] == [want], msg
        assert A.ic0_info()["zero_pivot"] == want
        dt = torch.complex128 if cplx else torch.float64
        x = torch.ones(n, dtype=dt, device="cuda")
        y = torch.zeros_like(x)
        assert lib.lcg_hip_ic0_solve(A.h, 2, x.data_ptr(), y.data_ptr()) == E_ARG
        m = torch.zeros_like(x)
        if cplx:
            para = api.clcg_default_parameters(epsilon=1e-10, abs_diff=1)
            rc = lib.clcg_hip_solver_preconditioned(_lib.fnptr(lib, "clcg_hip_csr_ax"), _lib.fnptr(lib, "clcg_hip_ic0_mx"), None,
                                                    m.data_ptr(), x.data_ptr(), n, para, A.h, api.CLCG_PCG, api.MEM_DEVICE)
        else:
            para = api.lcg_default_parameters(epsilon=1e-10, abs_diff=1)
            rc = lib.lcg_hip_solver_preconditioned(_lib.fnptr(lib, "lcg_hip_csr_ax"), _lib.fnptr(lib, "lcg_hip_ic0_mx"), None,
                                                   m.data_ptr(), x.data_ptr(), n, para, A.h, api.LCG_PCG, api.MEM_DEVICE)
        assert rc == E_ARG
        torch.cuda.synchronize()
        assert not y.any().item()                                # no answer was written
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 7. PCG / PBiCG whole runs
def _pcg_system(name, case10k):
    if name == "case10k":
        n, rp, ci, v, b, xs = case10k
        return rp, ci, v, b, xs
    rp, ci, v = system(name)[:3]
    As = K.to_sparse(len(rp) - 1, rp, ci, v)
    xt = rhs(len(rp) - 1, False, 6)
    return rp, ci, v, As @ xt, xt


@pytest.mark.parametrize("name,want_its", [("case10k", 54), ("laplace3d40", None)])
def test_pcg_whole_run(api, case10k, name, want_its):
    rp, ci, v, b, xt = _pcg_system(name, case10k)
    n = len(b)
    eps = 1e-10
    Kr, Kc, Kv, zp = K.ic0(n, rp, ci, v)
    As = K.to_sparse(n, rp, ci, v)
    M = K.IcApply(K.to_sparse(n, Kr, Kc, Kv))
    mconv, conv = K.lpcg(As, M.solve, b, eps, 1)
    if want_its is not None:
        assert conv == want_its
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
        A.build_ic0()
        bd = torch.from_numpy(b).cuda()
        m = torch.zeros(n, dtype=torch.float64, device="cuda")
        info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", None, m, bd, n,
                                             api.lcg_default_parameters(epsilon=eps, abs_diff=1), A)
        assert info.ret == 0 and abs(info.iterations - conv) <= 2, (info, conv)
        assert np.linalg.norm(m.cpu().numpy() - xt) <= 10 * max(np.linalg.norm(mconv - xt), 1e-14 * np.linalg.norm(xt))
        for k in ks:
            mk = torch.zeros_like(m)
            ik = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", None, mk, bd, n,
                                               api.lcg_default_parameters(epsilon=eps, abs_diff=1, max_iterations=k), A)
            assert ik.iterations == k
            d = np.linalg.norm(mk.cpu().numpy() - ref[k]) / np.linalg.norm(ref[k])
            assert d <= max(1e-12, 50.0 * sens[k]), (name, k, d, sens[k])
    finally:
        A.destroy()


@pytest.mark.parametrize("case", ["1K", "10K"])
def test_complex_pbicg(api, case1kc, case10kc, case):
    n, rp, ci, v, b, xs = case1kc if case == "1K" else case10kc
    Kr, Kc, Kv, zp = K.ic0(n, rp, ci, v)
    As = K.to_sparse(n, rp, ci, v)
    M = K.IcApply(K.to_sparse(n, Kr, Kc, Kv))
    _, conv = K.clpbicg(As, M.solve, b, 1e-10, 1)
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ic0()
        bd = torch.from_numpy(b).cuda()
        m = torch.zeros(n, dtype=torch.complex128, device="cuda")
        info = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ic0_mx", None, m, bd, n,
                                              api.clcg_default_parameters(epsilon=1e-10, abs_diff=1), A, api.CLCG_PBICG)
        assert info.ret == 0 and abs(info.iterations - conv) <= 2, (info, conv)
        assert np.linalg.norm(m.cpu().numpy() - xs) <= 1e-5
        for k in range(1, min(4, conv) + 1):
            mk = torch.zeros_like(m)
            ik = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ic0_mx", None, mk, bd, n,
                                                api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=k), A,
                                                api.CLCG_PBICG)
            want, t = K.clpbicg(As, M.solve, b, 1e-10, 1, max_iterations=k)
            assert ik.iterations == t == k
            assert np.linalg.norm(mk.cpu().numpy() - want) <= 1e-12 * np.linalg.norm(want), (case, k)
    finally:
        A.destroy()


def test_apply_errors(api, lib, case10k, case1kc):
    from liblcg_amd import _lib
    n, rp, ci, v, b, xs = case1kc
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ic0()
        x = torch.from_numpy(b).cuda()
        y = torch.zeros_like(x)
        # conjugate = 1 asks for M^H, which is not M: refused, directly ...
        lib.clcg_hip_ic0_mx(A.h, x.data_ptr(), y.data_ptr(), n, 0, 1)
        torch.cuda.synchronize()
        assert "conjugate" in lib.lcg_hip_last_error().decode() and not y.any().item()
        # ... and from inside a solve, where the parked code ends it
        seen = []

        def mx_conj(inst, xp, yp, nn, layout, conj):
            seen.append(nn)
            lib.clcg_hip_ic0_mx(inst, xp, yp, nn, layout, 1)
        cb = api.CAXFUNC(mx_conj)
        m = torch.zeros_like(x)
        para = api.clcg_default_parameters(epsilon=1e-10, abs_diff=1)
        for sid in (api.CLCG_PBICG, api.CLCG_PCG):
            rc = lib.clcg_hip_solver_preconditioned(_lib.fnptr(lib, "clcg_hip_csr_ax"), C.cast(cb, C.c_void_p), None, m.data_ptr(),
                                                    x.data_ptr(), n, para, A.h, sid, api.MEM_DEVICE)
            assert rc == E_ARG, sid
        assert seen
        # an n_size other than the factor's
        lib.clcg_hip_ic0_mx(A.h, x.data_ptr(), y.data_ptr(), n - 1, 0, 0)
        torch.cuda.synchronize()
        assert "n_size" in lib.lcg_hip_last_error().decode() and not y.any().item()
        # the parked codes do not outlive their solve: a good run afterwards converges
        info = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ic0_mx", None, m, x, n, para, A, api.CLCG_PBICG)
        assert info.ret == 0
    finally:
        A.destroy()

    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ic0()
        x = torch.from_numpy(b).cuda()
        y = torch.zeros_like(x)
        lib.lcg_hip_ic0_mx(A.h, x.data_ptr(), y.data_ptr(), n + 1)
        torch.cuda.synchronize()
        assert "n_size" in lib.lcg_hip_last_error().decode() and not y.any().item()

        def mx_short(inst, xp, yp, nn):
            lib.lcg_hip_ic0_mx(inst, xp, yp, nn - 1)
        cb = api.AXFUNC(mx_short)
        m = torch.zeros_like(x)
        rc = lib.lcg_hip_solver_preconditioned(_lib.fnptr(lib, "lcg_hip_csr_ax"), C.cast(cb, C.c_void_p), None, m.data_ptr(),
                                               x.data_ptr(), n, api.lcg_default_parameters(epsilon=1e-10, abs_diff=1), A.h,
                                               api.LCG_PCG, api.MEM_DEVICE)
        assert rc == E_ARG
    finally:
        A.destroy()

    # a matrix that is not square has no IC(0)
    rp, ci, v = K.laplace3d(8)
    A = api.CsrMatrix.from_csr(rp, ci, v, n_cols=len(rp))
    try:
        assert lib.lcg_hip_csr_build_ic0(A.h) == E_ARG
        assert "square" in lib.lcg_hip_last_error().decode()
        assert lib.lcg_hip_csr_ic0_info(A.h, None, None, None, None, None, None) == E_ARG     # and no factor was kept
    finally:
        A.destroy()
