"""Complex64 solvers without a GPU: the checker's loops (tests/c64_checker.py) against a direct solver, the dispatch and the
argument-check order of clcg_cudaf.cu in the checker and in the library, every new entry failing loudly without a device, and
the sample compiling with -Werror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import c64_checker as K
from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system, read_solution

E_NO_DEVICE = -2001


def _case(tag):
    n, row, col, val, b = read_coo_system(os.path.join(GOLDEN, f"case_{tag}_cA"), True)
    rp, ci, v = coo_to_csr_host(n, row, col, val)
    return n, rp, ci, v, b, read_solution(os.path.join(GOLDEN, f"case_{tag}_cB"), True)


def test_checker_loops_in_complex128_match_spsolve():
    import scipy.sparse.linalg as spla
    n, rp, ci, v, b, _ = _case("1K")
    ops = K.csr_ops(rp, ci, v, np.complex128)
    x_ref = spla.spsolve(ops["matrix"].tocsc(), b)
    m0 = np.zeros(n, np.complex128)
    para = {"epsilon": 1e-24, "max_iterations": 20000}
    jac = K.jacobi(rp, ci, v, np.complex128)
    runs = {"BiCG": K.bicg(ops["A"], ops["AH"], b, m0, para, np.complex128),
            "BiCG-sym": K.bicg_sym(ops["A"], b, m0, para, np.complex128),
            "PCG": K.pcg(ops["A"], jac, b, m0, para, np.complex128)}
    for name, r in runs.items():
        assert r["ret"] == K.CLCG_CONVERGENCE, (name, r["ret"], r["iters"], r["residual"])
        rel = np.linalg.norm(r["x"] - x_ref) / np.linalg.norm(x_ref)
        assert rel < 1e-8, (name, rel)


def test_checker_complex64_loops_follow_their_complex128_twins():
    """The same loops in complex64 stay within fp32 reach of the double run over the first iterations."""
    n, rp, ci, v, b, _ = _case("1K")
    ops = K.csr_ops(rp, ci, v, np.complex64)
    m0 = np.zeros(n, np.complex64)
    cap = {"epsilon": 1e-20, "max_iterations": 5}
    for f in (lambda dt: K.bicg_sym(ops["A"], b, m0, cap, dt), lambda dt: K.bicg(ops["A"], ops["AH"], b, m0, cap, dt)):
        a, d = f(np.complex64), f(np.complex128)
        assert a["x"].dtype == np.complex64 and a["iters"] == d["iters"] == 5
        assert np.linalg.norm(a["x"] - d["x"]) <= 1e-4 * np.linalg.norm(d["x"])


def test_checker_dispatch_and_argument_order():
    b = np.ones(4, np.complex64)
    assert K.solver(K.CLCG_PCG, None, None, None, None, {})["ret"] == K.CLCG_UNKNOWN_SOLVER
    assert K.check_args(0, {"max_iterations": -1, "epsilon": 2.0}, None, None) == K.CLCG_INVILAD_VARIABLE_SIZE
    assert K.check_args(4, {"max_iterations": -1, "epsilon": 2.0}, None, None) == K.CLCG_INVILAD_MAX_ITERATIONS
    assert K.check_args(4, {"epsilon": 1.0}, None, None) == K.CLCG_INVILAD_EPSILON
    assert K.check_args(4, {"epsilon": 0.5}, None, b) == K.CLCG_INVALID_POINTER
    assert K.check_args(4, {"epsilon": 0.5}, b, b) == 0


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def test_library_dispatch_and_argument_order(lib):
    """clcg_cudaf.cu:42-84 and :94-101: the id is looked at before the arguments, the arguments in the reference's order --
    all decided before the device is touched, so this runs anywhere."""
    from liblcg_amd import _lib
    ax = _lib.fnptr(lib, "clcg_hip_csr_ax_c64")
    buf = (C.c_float * 8)()
    def para(**kw):
        p = lib.clcg_hip_default_parameters()
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)
    for sid in (2, 3, 4, 5, 6, 99):
        assert lib.clcg_hip_solver_c64(ax, None, None, None, 0, para(epsilon=5.0), None, sid, 0) == K.CLCG_UNKNOWN_SOLVER
    for sid in (0, 1, 2, 6):
        assert lib.clcg_hip_solver_preconditioned_c64(ax, ax, None, None, None, 0, para(), None, sid, 0) == K.CLCG_UNKNOWN_SOLVER
    for call in (lambda p, n, m, b: lib.clcg_hip_solver_c64(ax, None, m, b, n, p, None, 0, 0),
                 lambda p, n, m, b: lib.clcg_hip_solver_c64(ax, None, m, b, n, p, None, 1, 0),
                 lambda p, n, m, b: lib.clcg_hip_solver_preconditioned_c64(ax, ax, None, m, b, n, p, None, 5, 0)):
        assert call(para(max_iterations=-1, epsilon=2.0), 0, None, None) == K.CLCG_INVILAD_VARIABLE_SIZE
        assert call(para(max_iterations=-1, epsilon=2.0), 4, None, None) == K.CLCG_INVILAD_MAX_ITERATIONS
        assert call(para(epsilon=0.0), 4, None, None) == K.CLCG_INVILAD_EPSILON
        assert call(para(epsilon=1.0), 4, None, None) == K.CLCG_INVILAD_EPSILON
        assert call(para(), 4, None, buf) == K.CLCG_INVALID_POINTER
        assert call(para(), 4, buf, None) == K.CLCG_INVALID_POINTER
    # then a missing preconditioner (LCG_NULL_PRECONDITION_MATRIX, as the c128 entry) or product (CLCG_INVALID_POINTER): both -1018
    assert lib.clcg_hip_solver_preconditioned_c64(ax, None, None, buf, buf, 4, para(), None, 5, 0) == -1018
    assert lib.clcg_hip_solver_c64(None, None, buf, buf, 4, para(), None, 1, 0) == K.CLCG_INVALID_POINTER


def test_new_entries_fail_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path cannot be exercised")
    from liblcg_amd import _lib
    ax = _lib.fnptr(lib, "clcg_hip_csr_ax_c64")
    jm = _lib.fnptr(lib, "clcg_hip_jacobi_mx_c64")
    buf = (C.c_float * 8)()
    rp = (C.c_int * 5)(0, 1, 2, 3, 4)
    ci = (C.c_int * 4)(0, 1, 2, 3)
    p = lib.clcg_hip_default_parameters()
    h = C.c_void_p()
    assert lib.lcg_hip_csr_create_c64(C.byref(h), 4, 4, 4, rp, ci, buf, 0, 0) == E_NO_DEVICE
    assert lib.lcg_hip_spmv_c64(None, buf, buf, 0, 0) == E_NO_DEVICE
    for sid in (0, 1):
        assert lib.clcg_hip_solver_c64(ax, None, buf, buf, 4, C.byref(p), None, sid, 0) == E_NO_DEVICE
    assert lib.clcg_hip_solver_preconditioned_c64(ax, jm, None, buf, buf, 4, C.byref(p), None, 5, 0) == E_NO_DEVICE
    assert "no HIP device" in lib.lcg_hip_last_error().decode()


def test_sample_compiles_with_werror_and_exits_3_without_gpu(lib):
    bindir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "sample_csr_c64")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sample_csr_c64.cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", exe])
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_c64.py runs the sample")
    p = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 3, p.stdout + p.stderr
