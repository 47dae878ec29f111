"""Complex64 IC(0) on the MI355X (csr_ic0.hip's float2 instantiation): the device factor against the fp32 checker
(tests/ic0_c64_checker.py), its schedule against the complex128 build of the same pattern, the three solves against SciPy in
complex128 on the device's own L, every grouping of levels giving the same bits, capped and converged PCG runs against
c64_checker.pcg with the checker's IC(0), the type checks between c64 and fp64 / c128 handles, device memory over rebuilds, and
the C++ sample (sample14.cu's own run)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.sparse.linalg import spsolve_triangular

from conftest import GOLDEN, ROOT
import c64_checker as K
import ic0_c64_checker as Q
import ic0_checker as IC
from test_gpu_c64 import _tol, case, dev, helmholtz

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
E_ARG = -2003
U = 2.0 ** -24          # fp32 unit roundoff
SAMPLE14 = {"epsilon": 1e-6, "abs_diff": 0, "max_iterations": 5000}     # sample14.cu (uncapped there; Jacobi needs ~1600)


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------ systems
LAYER_WIDTHS = [3, 40, 1, 1, 700, 5, 2, 1500, 30, 1, 1, 200, 9]     # narrow runs, and one level wider than a workgroup (1500)


def system(name):
    """(rowptr, col, complex64 values) of a named test matrix."""
    if name in ("1K", "10K"):
        rp, ci, v, _, _ = case(name)
        return rp, ci, v
    if name == "helmholtz":
        return helmholtz(100)
    rp, ci, v = IC.layered(LAYER_WIDTHS, seed=6, cplx=True)
    v = v.astype(np.complex64)
    if name == "layered":
        return rp, ci, v
    return IC.shuffle_split(rp, ci, v, seed=12)                 # "shuffled": rows in random order, duplicate entries


NAMES = ["1K", "10K", "helmholtz", "layered", "shuffled"]


def _row_rel(a, b, rp):
    """max over rows of |a_row - b_row| / |b_row|."""
    a, b = a.astype(np.complex128), b.astype(np.complex128)
    return max(np.linalg.norm(a[rp[i]:rp[i + 1]] - b[rp[i]:rp[i + 1]]) / np.linalg.norm(b[rp[i]:rp[i + 1]])
               for i in range(len(rp) - 1))


# ------------------------------------------------------------------------------------------ 1. factor
@pytest.mark.parametrize("name", NAMES)
def test_factor_matches_checker(api, lib, name):
    """The device's L has the checker's pattern, and its values lie within 4 g (and at least 64 u) of the checker's per row, where
    g is the checker's own per-row gap between its fp32 factor and the complex128 factor of the same complex64 matrix: the device
    and the checker are two fp32 evaluations of one factor, each about g from the exact one, so at most 2 g apart -- 4 g with
    margin.  Two builds give the same bits; levels and launches are the complex128 build's of the same pattern."""
    rp, ci, v = system(name)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    A128 = api.CsrMatrix.from_csr(rp, ci, v.astype(np.complex128))
    try:
        A.build_ic0()
        info = A.ic0_info()
        assert info["zero_pivot"] == -1
        drp, dcol, dval = A.ic0_factor_to_host()
        assert dval.dtype == np.complex64
        crp, ccol, cval, zp = Q.ic0(n, rp, ci, v)
        assert zp == -1
        assert np.array_equal(drp, crp) and np.array_equal(dcol, ccol)
        _, _, c128, _ = IC.ic0(n, rp, ci, v.astype(np.complex128))
        g = _row_rel(cval, c128, crp)
        tol = max(4 * g, 64 * U)
        assert tol <= 1e-4, (name, g)                           # well-conditioned systems: the bound stays meaningful
        err = _row_rel(dval, cval, crp)
        assert err <= tol, (name, err, tol)
        A.build_ic0()                                           # rebuild: the same bits
        assert A.ic0_factor_to_host()[2].tobytes() == dval.tobytes()
        A128.build_ic0()
        i128 = A128.ic0_info()
        for key in ("levels_lower", "levels_upper", "launches_per_apply"):
            assert info[key] == i128[key], (name, key, info[key], i128[key])
        assert i128["bytes"] - info["bytes"] == 8 * (2 * len(dcol) + n)     # 8-byte values in L, L^T and the work vector
        if name in ("layered", "shuffled"):
            assert info["levels_lower"] == len(LAYER_WIDTHS)
    finally:
        A.destroy()
        A128.destroy()


# ------------------------------------------------------------------------------------------ 2. solves
def _solve(lib, A, which, x):
    y = torch.zeros_like(x)
    assert lib.lcg_hip_ic0_solve_c64(A.h, which, x.data_ptr(), y.data_ptr()) == 0
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_solves_match_scipy_and_repeat_bitwise(api, lib, name):
    """L^-1 x, L^-T x and (L L^T)^-1 x against SciPy's complex128 triangular solves on the device's own L: within 4 g (at least
    64 u), g the checker's fp32 solves' gap to the same SciPy solves (two fp32 evaluations of one solve).  Repeated calls, one
    launch per level (grouping 0) and narrow groups of at most 64 rows give the production bits."""
    rp, ci, v = system(name)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    try:
        A.build_ic0()
        drp, dcol, dval = A.ic0_factor_to_host()
        L = IC.to_sparse(n, drp, dcol, dval.astype(np.complex128))
        LT = L.T.tocsr()
        ap = Q.Ic64Apply(n, drp, dcol, dval)
        rng = np.random.default_rng(7)
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        xd = dev(x)
        x128 = x.astype(np.complex128)
        refs = {0: spsolve_triangular(L, x128, lower=True), 1: spsolve_triangular(LT, x128, lower=False)}
        refs[2] = spsolve_triangular(LT, refs[0], lower=False)
        prod = {}
        for which in (0, 1, 2):
            ref = refs[which]
            g = np.linalg.norm(ap.solve(x, which) - ref) / np.linalg.norm(ref)
            tol = max(4 * g, 64 * U)
            y = _solve(lib, A, which, xd)
            rel = np.linalg.norm(y - ref) / np.linalg.norm(ref)
            assert rel <= tol, (name, which, rel, tol)
            assert _solve(lib, A, which, xd).tobytes() == y.tobytes()
            prod[which] = y.tobytes()
        for grouping in (0, 64):
            assert lib.lcg_hip_csr_ic0_schedule_for_test(A.h, grouping) == 0
            for which in (0, 1, 2):
                assert _solve(lib, A, which, xd).tobytes() == prod[which], (name, grouping, which)
        assert lib.lcg_hip_csr_ic0_schedule_for_test(A.h, -1) == 0
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 3. PCG
def _pcg(api, A, b, para, Mfp="clcg_hip_ic0_mx_c64"):
    n = len(b)
    m = torch.zeros(n, dtype=torch.complex64, device="cuda")
    info = api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", Mfp, None, m, dev(b), n, para, A)
    return info, m.cpu().numpy()


@pytest.mark.parametrize("name,caps", [("10K", range(1, 5)), ("helmholtz", range(1, 9))])
def test_capped_pcg_against_the_checker(api, lib, name, caps):
    """clpcg with the device's IC(0) against c64_checker.pcg with the checker's IC(0): the same return code and iteration count,
    the iterate within test_gpu_c64's tolerance for capped c64 runs (4x the checker's own fp32-vs-complex128 gap)."""
    rp, ci, v = system(name)
    n = len(rp) - 1
    ops = K.csr_ops(rp, ci, v, np.complex64)
    if name == "helmholtz":
        rng = np.random.default_rng(9)
        b = ops["A"]((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)).astype(np.complex64)
    else:
        b = case(name)[3]
    lrp, lc, lv, _ = Q.ic0(n, rp, ci, v)
    mx = {np.complex64: Q.Ic64Apply(n, lrp, lc, lv).mx, np.complex128: Q.c128_apply(n, rp, ci, v)}
    m0 = np.zeros(n, np.complex64)
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    try:
        A.build_ic0()
        for k in caps:
            cap = {"epsilon": 1e-30, "max_iterations": k}
            ref, tol = _tol(lambda dt, k: K.pcg(ops["A"], mx[dt], b, m0, cap, dt), k)
            info, x = _pcg(api, A, b, api.clcg_default_parameters(epsilon=1e-30, max_iterations=k))
            assert info.ret == ref["ret"] and info.iterations == ref["iters"], (name, k, info, ref["ret"], ref["iters"])
            rel = np.linalg.norm(x.astype(np.complex128) - ref["x"]) / np.linalg.norm(ref["x"])
            assert rel <= tol, (name, k, rel, tol)
    finally:
        A.destroy()


def test_converged_pcg_at_sample14_settings(api, lib):
    """case_1K_cA to eps = 1e-6 (sample14.cu): CLCG_CONVERGENCE in no more iterations than the c64 Jacobi run, and the averaged
    error (sample14's avg_error) within 3x (+ 1e-7) of the checker's run."""
    rp, ci, v, b, xs = case("1K")
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    try:
        A.build_ic0()
        assert api.L.load().lcg_hip_csr_build_jacobi(A.h, None) == 0
        para = api.clcg_default_parameters(**SAMPLE14)
        info, x = _pcg(api, A, b, para)
        jac, _ = _pcg(api, A, b, para, Mfp="clcg_hip_jacobi_mx_c64")
        assert info.ret == K.CLCG_CONVERGENCE, info
        assert info.iterations <= jac.iterations, (info.iterations, jac.iterations)
        lrp, lc, lv, _ = Q.ic0(n, rp, ci, v)
        ref = K.pcg(K.csr_ops(rp, ci, v, np.complex64)["A"], Q.Ic64Apply(n, lrp, lc, lv).mx, b, np.zeros(n, np.complex64), SAMPLE14)
        xs64 = xs.astype(np.complex64)
        e_ref = float(np.linalg.norm((ref["x"] - xs64).astype(np.complex128)) / n)
        e = float(np.linalg.norm((x - xs64).astype(np.complex128)) / n)
        assert e <= 3 * e_ref + 1e-7, (e, e_ref)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 4. errors and type mixing
def test_errors_and_type_mixing(api, lib):
    from liblcg_amd import _lib
    rp, ci, v = helmholtz(30)
    n = len(rp) - 1
    A64 = api.CsrMatrix.from_csr_c64(rp, ci, v)
    A128 = api.CsrMatrix.from_csr(rp, ci, v.astype(np.complex128))
    Areal = api.CsrMatrix.from_csr(rp, ci, v.real.astype(np.float64))
    x = torch.ones(n, dtype=torch.complex64, device="cuda"); y = torch.zeros_like(x)
    b = dev(K.csr_ops(rp, ci, v)["A"](np.ones(n)).astype(np.complex64))
    para = api.clcg_default_parameters(epsilon=1e-30, max_iterations=3)
    try:
        # the c64 build refuses other handles; without a factor the c64 entries refuse
        for H in (A128, Areal):
            assert lib.lcg_hip_csr_build_ic0_c64(H.h) == E_ARG
            assert "complex64" in lib.lcg_hip_last_error().decode()
        assert lib.lcg_hip_ic0_solve_c64(A64.h, 2, x.data_ptr(), y.data_ptr()) == E_ARG
        assert "no factor" in lib.lcg_hip_last_error().decode()
        with pytest.raises(api.LcgHipError, match="-2003"):
            api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_ic0_mx_c64", None, torch.zeros_like(x), b, n, para, A64)
        # a complex128 factor is not served by the c64 callback or solve
        A128.build_ic0()
        assert lib.lcg_hip_ic0_solve_c64(A128.h, 2, x.data_ptr(), y.data_ptr()) == E_ARG
        with pytest.raises(api.LcgHipError, match="-2003"):
            api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_ic0_mx_c64", None, torch.zeros_like(x), b, n, para, A128)
        # with a c64 factor: the fp64 / c128 entries still refuse the handle, naming the c64 ones
        A64.build_ic0()
        x128 = torch.ones(n, dtype=torch.complex128, device="cuda"); y128 = torch.zeros_like(x128)
        assert lib.lcg_hip_ic0_solve(A64.h, 2, x128.data_ptr(), y128.data_ptr()) == E_ARG
        msg = lib.lcg_hip_last_error().decode()
        assert "complex64" in msg and "lcg_hip_ic0_solve_c64" in msg, msg
        assert lib.lcg_hip_csr_build_ic0(A64.h) == E_ARG and "lcg_hip_csr_build_ic0_c64" in lib.lcg_hip_last_error().decode()
        with pytest.raises(api.LcgHipError, match="-2003"):
            api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ic0_mx", None, torch.zeros_like(x128), x128, n,
                                           api.clcg_default_parameters(), A64)
        # conjugate = 1, directly and from inside a solve; a wrong n_size
        lib.clcg_hip_ic0_mx_c64(A64.h, x.data_ptr(), y.data_ptr(), n, 0, 1)
        torch.cuda.synchronize()
        assert "conjugate" in lib.lcg_hip_last_error().decode() and not y.any().item()
        for conj, nn in ((1, None), (0, n - 1)):
            def mx(inst, xp, yp, k, layout, c, conj=conj, nn=nn):
                lib.clcg_hip_ic0_mx_c64(inst, xp, yp, k if nn is None else nn, layout, conj)
            cb = api.CAXFUNC(mx)
            rc = lib.clcg_hip_solver_preconditioned_c64(_lib.fnptr(lib, "clcg_hip_csr_ax_c64"), C.cast(cb, C.c_void_p), None,
                                                        torch.zeros_like(x).data_ptr(), b.data_ptr(), n, C.byref(para), A64.h,
                                                        api.CLCG_PCG, api.MEM_DEVICE)
            assert rc == E_ARG, (conj, nn)
        # overlap, which
        assert lib.lcg_hip_ic0_solve_c64(A64.h, 2, x.data_ptr(), x.data_ptr()) == E_ARG
        assert lib.lcg_hip_ic0_solve_c64(A64.h, 0, x.data_ptr(), x.data_ptr() + 8 * (n - 1)) == E_ARG
        assert "overlap" in lib.lcg_hip_last_error().decode()
        assert lib.lcg_hip_ic0_solve_c64(A64.h, 3, x.data_ptr(), y.data_ptr()) == E_ARG
        # and a working solve afterwards
        assert lib.lcg_hip_ic0_solve_c64(A64.h, 2, x.data_ptr(), y.data_ptr()) == 0
    finally:
        for H in (A64, A128, Areal):
            H.destroy()

    # a failed pivot: first-layer rows read no other row, so a zero diagonal there is a zero pivot; the smallest is named
    rp, ci, v = system("layered")
    v = v.copy()
    for i in (2, 1):
        v[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] == i] = 0
    assert Q.ic0(len(rp) - 1, rp, ci, v)[3] == 1
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    try:
        assert lib.lcg_hip_csr_build_ic0_c64(A.h) == E_ARG
        assert "row 1 " in lib.lcg_hip_last_error().decode()
        assert A.ic0_info()["zero_pivot"] == 1
        assert lib.lcg_hip_ic0_solve_c64(A.h, 2, x.data_ptr(), y.data_ptr()) == E_ARG
    finally:
        A.destroy()


def test_memory_over_rebuilds(api, lib):
    """create -> build -> rebuild -> destroy, three times, gives the device memory back."""
    rp, ci, v = helmholtz(200)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        A = api.CsrMatrix.from_csr_c64(rp, ci, v)
        A.build_ic0()
        A.build_ic0()
        A.destroy()
    assert lib.lcg_hip_trim() == 0
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)


# ------------------------------------------------------------------------------------------ 5. C++ sample
def test_cpp_sample(api):
    """sample14.cu's run: exit 0 (converged), the iteration count within 10 % (+ 2) of the checker's, the averaged error within
    3x (+ 1e-7) of the checker's."""
    from liblcg_amd import _lib
    _lib.build()
    bindir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "sample_csr_c64_ic0")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sample_csr_c64_ic0.cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", exe])
    p = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    it = int(re.search(r"iterations:\s*(\d+)", p.stdout).group(1))
    err = float(re.search(r"Averaged error \(compared with ans_x\):\s*(\S+)", p.stdout).group(1))
    rp, ci, v, b, xs = case("1K")
    n = len(b)
    lrp, lc, lv, _ = Q.ic0(n, rp, ci, v)
    ref = K.pcg(K.csr_ops(rp, ci, v, np.complex64)["A"], Q.Ic64Apply(n, lrp, lc, lv).mx, b, np.zeros(n, np.complex64),
                {"epsilon": 1e-6, "abs_diff": 0, "max_iterations": 1000})
    assert ref["ret"] == K.CLCG_CONVERGENCE
    assert abs(it - ref["iters"]) <= 0.1 * ref["iters"] + 2, (p.stdout, ref["iters"])
    e_ref = float(np.linalg.norm((ref["x"] - xs.astype(np.complex64)).astype(np.complex128)) / n)
    assert err <= 3 * e_ref + 1e-7, (p.stdout, e_ref)
