"""Complex64 IC(0) without a GPU: the fp32 checker (tests/ic0_c64_checker.py) against a complex128 dense Cholesky where IC(0) is
exact, its handling of the input (upper triangle ignored, duplicates summed, the smallest failed pivot), its PCG run at sample14's
settings against its Jacobi run, the new entries exported, declared and failing loudly without a device, and the sample
compiling with -Werror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import c64_checker as K
import ic0_c64_checker as Q
import ic0_checker as IC
from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system, read_solution

E_NO_DEVICE = -2001
U = 2.0 ** -24
NEW = ("lcg_hip_csr_build_ic0_c64", "lcg_hip_ic0_solve_c64", "clcg_hip_ic0_mx_c64")


def _band(n, width, seed):
    """A complex symmetric, diagonally dominant matrix whose lower triangle is full within `width` diagonals (width 1:
    tridiagonal): IC(0) has no fill to drop there, so it is the exact unconjugated Cholesky factor."""
    rng = np.random.default_rng(seed)
    lower = [{j: complex(rng.uniform(-1, 1), rng.uniform(-1, 1)) for j in range(max(0, i - width), i)} for i in range(n)]
    return IC.assemble(n, lower, IC.dominant_diagonal(rng, n, lower, True))


def _dense(n, rp, ci, v):
    return IC.to_sparse(n, rp, ci, v).toarray()


@pytest.mark.parametrize("width", [1, 4])
def test_factor_matches_complex128_dense_cholesky(width):
    """Per row, |L32 - L128| <= 64 n u |L128| (u = 2^-24): each entry is a chain of at most n fp32 operations on well-conditioned
    data (diagonally dominant: every pivot of modulus above 1), so its error grows at most linearly in the chain's length."""
    n = 60
    rp, ci, v = _band(n, width, seed=width)
    v64 = v.astype(np.complex64)
    lrp, lc, lv, zp = Q.ic0(n, rp, ci, v64)
    assert zp == -1 and lv.dtype == np.complex64
    L = _dense(n, lrp, lc, lv).astype(np.complex128)
    ref = Q.dense_cholesky_unconjugated(_dense(n, rp, ci, v64.astype(np.complex128)))
    assert np.array_equal(L != 0, np.tril(ref) != 0)                 # the band's pattern, nothing outside it
    for i in range(n):
        err = np.linalg.norm(L[i] - ref[i])
        assert err <= 64 * n * U * np.linalg.norm(ref[i]), (width, i, err / np.linalg.norm(ref[i]))
    # and the product reproduces A to fp32 accuracy
    A = _dense(n, rp, ci, v64.astype(np.complex128))
    assert np.linalg.norm(L @ L.T - A) <= 64 * n * U * np.linalg.norm(A)


def test_upper_triangle_ignored_duplicates_summed_smallest_pivot():
    rp, ci, v = IC.layered([7, 30, 12, 60, 1, 90], seed=4, cplx=True)
    n = len(rp) - 1
    v64 = v.astype(np.complex64)
    ref = Q.ic0(n, rp, ci, v64)
    # the lower triangle alone gives the same bits
    keep = np.concatenate([np.nonzero(ci[rp[i]:rp[i + 1]] <= i)[0] + rp[i] for i in range(n)])
    lrp = np.zeros(n + 1, np.int64); lrp[1:] = np.cumsum([np.sum(ci[rp[i]:rp[i + 1]] <= i) for i in range(n)])
    low = Q.ic0(n, lrp, ci[keep], v64[keep])
    assert np.array_equal(low[1], ref[1]) and low[2].tobytes() == ref[2].tobytes()
    # rows shuffled, entries split into 0.75 x + 0.25 x: the same pattern, values within fp32 rounding of the sums
    srp, sci, sv = IC.shuffle_split(rp, ci, v64, seed=8)
    dup = Q.ic0(n, srp, sci, sv)
    assert np.array_equal(dup[0], ref[0]) and np.array_equal(dup[1], ref[1]) and dup[3] == -1
    assert np.max(np.abs(dup[2] - ref[2]) / np.abs(ref[2])) <= 1e-5
    # zero pivots at rows 6 and 3 (first-layer rows, which read no other row: a zero diagonal is a zero pivot), a NaN one at
    # row 5: the smallest is reported
    bad = v64.copy()
    for i, x in ((6, 0), (3, 0), (5, np.nan)):
        bad[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] == i] = x
    assert Q.ic0(n, rp, ci, bad)[3] == 3
    bad = v64.copy()
    bad[rp[5]:rp[6]][ci[rp[5]:rp[6]] == 5] = np.nan
    assert Q.ic0(n, rp, ci, bad)[3] == 5


def test_fp32_helpers_follow_the_complex_formulas():
    rng = np.random.default_rng(1)
    for _ in range(200):
        a = tuple(float(np.float32(x)) for x in rng.standard_normal(2))
        b = tuple(float(np.float32(x)) for x in rng.standard_normal(2))
        ca, cb = complex(*a), complex(*b)
        assert abs(complex(*Q.mul(a, b)) - ca * cb) <= 4 * U * abs(ca) * abs(cb)
        assert abs(complex(*Q.div(a, b)) - ca / cb) <= 8 * U * abs(ca / cb)
        r = complex(*Q.csqrt(a))
        ref = np.sqrt(np.complex64(ca))
        assert abs(r - complex(ref)) <= 4 * U * abs(ref)
        assert r.real >= 0.0
    assert Q.csqrt((-4.0, 0.0)) == (0.0, 2.0) and Q.csqrt((-4.0, -0.0)) == (0.0, -2.0) and Q.csqrt((0.0, -0.0)) == (0.0, -0.0)


def _case(tag):
    n, row, col, val, b = read_coo_system(os.path.join(GOLDEN, f"case_{tag}_cA"), True)
    rp, ci, v = coo_to_csr_host(n, row, col, val)
    return n, rp, ci, v.astype(np.complex64), b.astype(np.complex64), read_solution(os.path.join(GOLDEN, f"case_{tag}_cB"), True)


def test_checker_pcg_with_ic0_converges_at_sample14_settings():
    n, rp, ci, v, b, xs = _case("1K")
    ops = K.csr_ops(rp, ci, v, np.complex64)
    lrp, lc, lv, zp = Q.ic0(n, rp, ci, v)
    assert zp == -1
    ap = Q.Ic64Apply(n, lrp, lc, lv)
    cfg = {"epsilon": 1e-6, "abs_diff": 0, "max_iterations": 5000}        # (sample14 runs uncapped: Jacobi needs ~1600)
    m0 = np.zeros(n, np.complex64)
    ic = K.pcg(ops["A"], ap.mx, b, m0, cfg)
    jac = K.pcg(ops["A"], K.jacobi(rp, ci, v), b, m0, cfg)
    assert ic["ret"] == jac["ret"] == K.CLCG_CONVERGENCE
    assert ic["iters"] < jac["iters"], (ic["iters"], jac["iters"])
    err = np.linalg.norm((ic["x"] - xs.astype(np.complex64)).astype(np.complex128)) / n
    assert err < 1e-4, err
    # the fp32 apply against SciPy's complex128 solves on the same fp32 L
    sp_ap = IC.IcApply(IC.to_sparse(n, lrp, lc, lv.astype(np.complex128)))
    x = (np.random.default_rng(3).standard_normal(n) + 1j * np.random.default_rng(4).standard_normal(n)).astype(np.complex64)
    for which in (0, 1, 2):
        y, ref = ap.solve(x, which), sp_ap.solve(x.astype(np.complex128), which)
        assert y.dtype == np.complex64
        assert np.linalg.norm(y - ref) <= 1e-5 * np.linalg.norm(ref), which


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def test_new_entries_exported_and_declared(lib):
    from liblcg_amd import _lib
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.build()], text=True)
    header = open(os.path.join(ROOT, "include", "lcg_hip.h")).read()
    for name in NEW:
        assert f" T {name}\n" in syms, name
        assert f"{name}(" in header and name in _lib.SIGNATURES, name


def test_new_entries_fail_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path cannot be exercised")
    from liblcg_amd import _lib
    ax = _lib.fnptr(lib, "clcg_hip_csr_ax_c64")
    im = _lib.fnptr(lib, "clcg_hip_ic0_mx_c64")
    buf = (C.c_float * 8)()
    p = lib.clcg_hip_default_parameters()
    assert lib.lcg_hip_csr_build_ic0_c64(None) == E_NO_DEVICE
    assert lib.lcg_hip_ic0_solve_c64(None, 2, buf, buf) == E_NO_DEVICE
    assert lib.clcg_hip_solver_preconditioned_c64(ax, im, None, buf, buf, 4, C.byref(p), None, 5, 0) == E_NO_DEVICE
    assert "no HIP device" in lib.lcg_hip_last_error().decode()


def test_sample_compiles_with_werror_and_exits_3_without_gpu(lib):
    bindir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "sample_csr_c64_ic0")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sample_csr_c64_ic0.cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", exe])
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_ic0_c64.py runs the sample")
    p = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 3, p.stdout + p.stderr
