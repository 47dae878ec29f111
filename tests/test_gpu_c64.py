"""Complex64 on the MI355X (csr_c64.hip, solvers_c64.hip): the products in all four forms row by row against NumPy, capped and
converged BiCG / BiCG-sym / PCG runs against the checker's restatements of clcg_cudaf.cu (tests/c64_checker.py), return codes,
type confusion between c64 and c128 handles, device memory over repeated solves, and the C++ sample."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import c64_checker as K
from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system, read_solution

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
E_ARG = -2003
U = 2.0 ** -24          # fp32 unit roundoff


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
def case(tag):
    n, row, col, val, b = read_coo_system(os.path.join(GOLDEN, f"case_{tag}_cA"), True)
    rp, ci, v = coo_to_csr_host(n, row, col, val)
    return rp, ci, v.astype(np.complex64), b.astype(np.complex64), read_solution(os.path.join(GOLDEN, f"case_{tag}_cB"), True)


def helmholtz(nx):
    """The damped 2-D Helmholtz operator of tests/test_gpu_solvers.py (5-point Laplacian + (0.3 + 0.8i) I): complex symmetric."""
    n = nx * nx
    idx = np.arange(n, dtype=np.int64)
    ix, iy = idx % nx, idx // nx
    rows, cols, vals = [idx], [idx], [np.full(n, 4.0 + 0.3 + 0.8j, dtype=np.complex64)]
    for ok, off in ((ix > 0, -1), (ix < nx - 1, 1), (iy > 0, -nx), (iy < nx - 1, nx)):
        rows.append(idx[ok]); cols.append(idx[ok] + off); vals.append(np.full(int(ok.sum()), -1.0, dtype=np.complex64))
    row = np.concatenate(rows); col = np.concatenate(cols).astype(np.int32); val = np.concatenate(vals)
    order = np.lexsort((col, row))
    rp = np.zeros(n + 1, np.int64); np.add.at(rp, row + 1, 1)
    return np.cumsum(rp).astype(np.int32), col[order], val[order]


def ragged(n=20000, long_len=5000, seed=3):
    """Empty rows, short rows of 1..9 entries at random columns, one row of `long_len` entries (not square-symmetric)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 10, n)
    lens[rng.choice(n, n // 10, replace=False)] = 0
    lens[n // 3] = long_len
    rp = np.zeros(n + 1, np.int64); rp[1:] = np.cumsum(lens)
    ci = np.concatenate([np.sort(rng.choice(n, int(k), replace=False)) for k in lens]).astype(np.int32)
    v = (rng.standard_normal(len(ci)) + 1j * rng.standard_normal(len(ci))).astype(np.complex64)
    return rp.astype(np.int32), ci, v


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------ 1. products
FORMS = ((0, 0, "A"), (1, 1, "AH"), (1, 0, "AT"), (0, 1, "conj"))


@pytest.mark.parametrize("name", ["1K", "10K", "helmholtz600", "ragged"])
def test_products_all_forms(api, lib, name):
    """Row by row against NumPy complex128 on the c64-rounded inputs: |y_i - y_ref,i| <= c_i 2^-24 (|A||x|)_i with
    c_i = 3 (len_i + 5).  Each real component of a row's sum is one chain of fp32 roundings: two fma per entry (2 len_i), then at
    most 9 adds combining lanes (a 64-lane butterfly, the four waves of a long row).  With m = 2 len_i + 10 roundings, recursive
    summation gives |error| <= gamma_m sum|terms| ~ m u sum|terms| (Higham, Accuracy and Stability, 3.1 / 4.2), and a component's
    terms |a.x x.x| + |a.y x.y| <= |a||x| (Cauchy-Schwarz).  The complex modulus of the two components' errors adds sqrt(2):
    sqrt(2) (2 len_i + 10) = 2.83 (len_i + 5) <= 3 (len_i + 5).  Repeated calls give the same bits."""
    if name == "helmholtz600":
        rp, ci, v = helmholtz(600)
    elif name == "ragged":
        rp, ci, v = ragged()
    else:
        rp, ci, v, _, _ = case(name)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    ops = K.csr_ops(rp, ci, v, np.complex64)
    absops = K.csr_ops(rp, ci, np.abs(v).astype(np.complex64), np.complex64)
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    xd = dev(x)
    lens_rows = np.diff(rp)
    for layout, conj, key in FORMS:
        y = torch.empty_like(xd)
        assert lib.lcg_hip_spmv_c64(A.h, xd.data_ptr(), y.data_ptr(), layout, conj) == 0
        torch.cuda.synchronize()
        y1 = y.cpu().numpy()
        ref = ops[key](x)
        bound_mag = absops["AT" if layout else "A"](np.abs(x)).real
        lens = np.diff(ops["matrix"].T.tocsr().indptr) if layout else lens_rows
        c = 3.0 * (lens + 5)
        err = np.abs(y1.astype(np.complex128) - ref)
        assert np.all(err <= c * U * bound_mag + 1e-30), (name, key, float(np.max(err / (c * U * bound_mag + 1e-30))))
        y2 = torch.empty_like(xd)
        assert lib.lcg_hip_spmv_c64(A.h, xd.data_ptr(), y2.data_ptr(), layout, conj) == 0
        torch.cuda.synchronize()
        assert y1.tobytes() == y2.cpu().numpy().tobytes(), (name, key)
        kern = lib.lcg_hip_csr_last_kernel(A.h).decode()
        assert kern.startswith("k_c64_rows"), kern
        if name == "ragged" and key == "A":
            assert "k_c64_long (1 long rows)" in kern, kern
        if name == "helmholtz600":
            assert "entry pairs" in kern, kern
    A.destroy()


# ------------------------------------------------------------------------------------------ 2. capped runs
def _tol(run, k):
    """What separates two fp32 evaluations of the same recurrence after k iterations: each lies about as far from the exact
    iterate as the checker's complex64 run lies from its complex128 twin (d); two of them at most 2 d apart -- 4 d with margin,
    and never below 64 u."""
    a, e = run(np.complex64, k), run(np.complex128, k)
    d = np.linalg.norm(a["x"].astype(np.complex128) - e["x"]) / max(np.linalg.norm(e["x"]), 1e-30)
    return a, max(4.0 * d, 64 * U)


def _solve(api, kind, A, b, para, Mfp="clcg_hip_jacobi_mx_c64", mem_host=False, Afp="clcg_hip_csr_ax_c64", Pfp=None):
    n = len(b)
    if mem_host:
        m = np.zeros(n, np.complex64); bb = np.ascontiguousarray(b, np.complex64)
    else:
        m = torch.zeros(n, dtype=torch.complex64, device="cuda"); bb = dev(b)
    if kind == "pcg":
        info = api.clcg_solver_preconditioned_c64(Afp, Mfp, Pfp, m, bb, n, para, A)
    else:
        info = api.clcg_solver_c64(Afp, Pfp, m, bb, n, para, A, api.CLCG_BICG if kind == "bicg" else api.CLCG_BICG_SYM)
    x = m if mem_host else m.cpu().numpy()
    return info, x


@pytest.mark.parametrize("kind", ["bicg", "bicg_sym", "pcg", "pcg_user"])
def test_capped_runs_against_the_checker(api, lib, kind):
    rp, ci, v = helmholtz(100)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    assert lib.lcg_hip_csr_build_jacobi(A.h, None) == 0
    ops = K.csr_ops(rp, ci, v, np.complex64)
    rng = np.random.default_rng(9)
    xt = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    b = ops["A"](xt).astype(np.complex64)
    jac = {np.complex64: K.jacobi(rp, ci, v, np.complex64), np.complex128: K.jacobi(rp, ci, v, np.complex128)}
    m0 = np.zeros(n, np.complex64)
    asked = []
    lib_ax = lib.clcg_hip_csr_ax_c64

    def user_ax(inst, x, y, nn, layout, conj):      # records the forms BiCG asks for, multiplies with the built-in product
        asked.append((layout, conj))
        lib_ax(inst, x, y, nn, layout, conj)

    def user_mx(inst, x, y, nn, layout, conj):       # a caller's own Mfp (the loop's unfused branch), applying the same Jacobi
        lib.clcg_hip_jacobi_mx_c64(inst, x, y, nn, layout, conj)

    for k in range(1, 7):
        para = api.clcg_default_parameters(epsilon=1e-30, max_iterations=k)
        cap = {"epsilon": 1e-30, "max_iterations": k}
        if kind == "bicg":
            run = lambda dt, k: K.bicg(ops["A"], ops["AH"], b, m0, cap, dt)
            asked.clear()
            info, x = _solve(api, kind, A, b, para, Afp=user_ax)
            assert (1, 1) in asked and asked.count((1, 1)) == k, asked
        elif kind == "bicg_sym":
            run = lambda dt, k: K.bicg_sym(ops["A"], b, m0, cap, dt)
            info, x = _solve(api, kind, A, b, para)
        else:
            run = lambda dt, k: K.pcg(ops["A"], jac[dt], b, m0, cap, dt)
            info, x = _solve(api, "pcg", A, b, para, Mfp=user_mx if kind == "pcg_user" else "clcg_hip_jacobi_mx_c64")
        ref, tol = _tol(run, k)
        assert info.ret == ref["ret"] == K.LCG_REACHED_MAX_ITERATIONS and info.iterations == ref["iters"] == k
        rel = np.linalg.norm(x.astype(np.complex128) - ref["x"]) / np.linalg.norm(ref["x"])
        assert rel <= tol, (kind, k, rel, tol)
        assert abs(info.residual - ref["residual"]) <= max(8 * tol, 1e-5) * ref["residual"], (kind, k, info.residual, ref["residual"])
    A.destroy()


def test_bicg_needs_the_adjoint_product(api, lib):
    """BiCG on a non-Hermitian, non-symmetric matrix: a product that answers A^T where A^H is asked for leaves the loop's
    iterates (checked against the checker, which asks for A^H)."""
    rp, ci, v = helmholtz(60)
    n = len(rp) - 1
    rng = np.random.default_rng(2)
    v = (v + (0.2 + 0.1j) * rng.standard_normal(len(v))).astype(np.complex64)      # not symmetric any more
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    ops = K.csr_ops(rp, ci, v, np.complex64)
    b = ops["A"](np.ones(n)).astype(np.complex64)
    m0 = np.zeros(n, np.complex64)
    for k in (3, 6):
        ref, tol = _tol(lambda dt, k: K.bicg(ops["A"], ops["AH"], b, m0, {"epsilon": 1e-30, "max_iterations": k}, dt), k)
        info, x = _solve(api, "bicg", A, b, api.clcg_default_parameters(epsilon=1e-30, max_iterations=k))
        rel = np.linalg.norm(x.astype(np.complex128) - ref["x"]) / np.linalg.norm(ref["x"])
        assert rel <= tol, (k, rel, tol)
    A.destroy()


# ------------------------------------------------------------------------------------------ 3. converged runs
@pytest.mark.parametrize("kind", ["bicg", "bicg_sym", "pcg"])
def test_converged_runs(api, lib, kind):
    """To eps = 1e-10 on |r|^2 / max(|m|, 1)^2 (reachable in fp32 on this well-conditioned system): the iterate's distance to
    the generating x within 10x the checker's own converged error, and the iteration count within 10 % (+2) of the checker's."""
    rp, ci, v = helmholtz(300)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    assert lib.lcg_hip_csr_build_jacobi(A.h, None) == 0
    ops = K.csr_ops(rp, ci, v, np.complex64)
    rng = np.random.default_rng(4)
    xt = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    b = ops["A"](xt).astype(np.complex64)
    m0 = np.zeros(n, np.complex64)
    cfg = {"epsilon": 1e-10, "max_iterations": 3000}
    ref = {"bicg": lambda: K.bicg(ops["A"], ops["AH"], b, m0, cfg),
           "bicg_sym": lambda: K.bicg_sym(ops["A"], b, m0, cfg),
           "pcg": lambda: K.pcg(ops["A"], K.jacobi(rp, ci, v), b, m0, cfg)}[kind]()
    assert ref["ret"] == 0
    info, x = _solve(api, kind, A, b, api.clcg_default_parameters(epsilon=1e-10, max_iterations=3000))
    assert info.ret == 0
    err_ref = np.linalg.norm(ref["x"] - xt) / np.linalg.norm(xt)
    err = np.linalg.norm(x - xt) / np.linalg.norm(xt)
    assert err <= 10 * err_ref, (kind, err, err_ref)
    assert abs(info.iterations - ref["iters"]) <= 0.1 * ref["iters"] + 2, (kind, info.iterations, ref["iters"])
    A.destroy()


# ------------------------------------------------------------------------------------------ 4. return codes
def test_return_codes(api, lib):
    rp, ci, v = helmholtz(40)
    n = len(rp) - 1
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    assert lib.lcg_hip_csr_build_jacobi(A.h, None) == 0
    ops = K.csr_ops(rp, ci, v, np.complex64)
    b = ops["A"](np.ones(n)).astype(np.complex64)
    # already optimised: m = the solution of a system whose B is its own product
    for kind in ("bicg", "bicg_sym", "pcg"):
        m = torch.ones(n, dtype=torch.complex64, device="cuda")
        bd = torch.empty_like(m)
        assert lib.lcg_hip_spmv_c64(A.h, m.data_ptr(), bd.data_ptr(), 0, 0) == 0
        seen = []
        def prog(inst, mp, conv, para, nn, k):
            seen.append((conv, k)); return 0
        p = api.clcg_default_parameters(epsilon=1e-6)
        if kind == "pcg":
            info = api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_jacobi_mx_c64", prog, m, bd, n, p, A)
        else:
            info = api.clcg_solver_c64("clcg_hip_csr_ax_c64", prog, m, bd, n, p, A, api.CLCG_BICG if kind == "bicg" else api.CLCG_BICG_SYM)
        assert info.ret == K.CLCG_ALREADY and len(seen) == 1 and seen[0][1] == 0, (kind, info.ret, seen)
    # max iterations, and the same bits from host and device memory
    for kind in ("bicg", "bicg_sym", "pcg"):
        para = api.clcg_default_parameters(epsilon=1e-30, max_iterations=7)
        i1, x1 = _solve(api, kind, A, b, para)
        i2, x2 = _solve(api, kind, A, b, para, mem_host=True)
        i3, x3 = _solve(api, kind, A, b, para)
        assert i1.ret == i2.ret == K.LCG_REACHED_MAX_ITERATIONS and i1.iterations == 7
        assert x1.tobytes() == x2.tobytes() == x3.tobytes(), kind
    # progress stop at k = 3, m handed over on the device
    for kind in ("bicg", "bicg_sym", "pcg"):
        ks = []
        def stop(inst, mp, conv, para, nn, k):
            ks.append(k); return 1 if k == 3 else 0
        m = torch.zeros(n, dtype=torch.complex64, device="cuda")
        p = api.clcg_default_parameters(epsilon=1e-30)
        if kind == "pcg":
            info = api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_jacobi_mx_c64", stop, m, dev(b), n, p, A)
        else:
            info = api.clcg_solver_c64("clcg_hip_csr_ax_c64", stop, m, dev(b), n, p, A, api.CLCG_BICG if kind == "bicg" else api.CLCG_BICG_SYM)
        assert info.ret == K.CLCG_STOP and ks == [0, 1, 2, 3] and info.iterations == 3, (kind, ks)
    # invalid epsilon / size / pointer, unknown solver (the id first)
    buf = torch.zeros(n, dtype=torch.complex64, device="cuda")
    ax = api.L.fnptr(lib, "clcg_hip_csr_ax_c64")
    for eps, nn, mp, code in ((0.0, n, buf.data_ptr(), K.CLCG_INVILAD_EPSILON), (1e-6, 0, buf.data_ptr(), K.CLCG_INVILAD_VARIABLE_SIZE),
                              (1e-6, n, None, K.CLCG_INVALID_POINTER)):
        p = api.clcg_default_parameters(epsilon=eps)
        for sid in (0, 1):
            assert lib.clcg_hip_solver_c64(ax, None, mp, buf.data_ptr(), nn, C.byref(p), A.h, sid, 1) == code
        assert lib.clcg_hip_solver_preconditioned_c64(ax, ax, None, mp, buf.data_ptr(), nn, C.byref(p), A.h, 5, 1) == code
    p = api.clcg_default_parameters()
    assert lib.clcg_hip_solver_c64(ax, None, buf.data_ptr(), buf.data_ptr(), n, C.byref(p), A.h, api.CLCG_CGS, 1) == K.CLCG_UNKNOWN_SOLVER
    assert lib.clcg_hip_solver_preconditioned_c64(ax, ax, None, buf.data_ptr(), buf.data_ptr(), n, C.byref(p), A.h, api.CLCG_PBICG, 1) \
        == K.CLCG_UNKNOWN_SOLVER
    A.destroy()


def test_breakdown_stops_with_nan_value(api, lib):
    """A = 0: the first step length is 1 / 0 (cuCdivf's scaled quotient: NaN), m turns NaN.  The reference would spin to the cap --
    for ever with max_iterations = 0; the library stops after that iteration with CLCG_NAN_VALUE, as the checker does."""
    n = 4
    rp = np.arange(n + 1, dtype=np.int32); ci = np.arange(n, dtype=np.int32); v = np.zeros(n, np.complex64)
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    assert lib.lcg_hip_csr_build_jacobi(A.h, None) == 0
    ops = K.csr_ops(rp, ci, v, np.complex64)
    b = np.ones(n, np.complex64)
    m0 = np.zeros(n, np.complex64)
    cfg = {"epsilon": 1e-6, "max_iterations": 0}
    refs = {"bicg": K.bicg(ops["A"], ops["AH"], b, m0, cfg), "bicg_sym": K.bicg_sym(ops["A"], b, m0, cfg),
            "pcg": K.pcg(ops["A"], K.jacobi(rp, ci, v), b, m0, cfg)}
    for kind, ref in refs.items():
        for mem_host in (False, True):
            info, _ = _solve(api, kind, A, b, api.clcg_default_parameters(epsilon=1e-6, max_iterations=0), mem_host=mem_host)
            assert info.ret == ref["ret"] == K.CLCG_NAN_VALUE and info.iterations == ref["iters"] == 1, (kind, info.ret, info.iterations, ref)
    A.destroy()


# ------------------------------------------------------------------------------------------ 5. type confusion
def test_c64_and_c128_handles_do_not_mix(api, lib):
    rp, ci, v = helmholtz(30)
    n = len(rp) - 1
    A64 = api.CsrMatrix.from_csr_c64(rp, ci, v)
    A128 = api.CsrMatrix.from_csr(rp, ci, v.astype(np.complex128))
    Areal = api.CsrMatrix.from_csr(rp, ci, v.real.astype(np.float64))
    x = torch.ones(n, dtype=torch.complex128, device="cuda"); y = torch.empty_like(x)
    h = A64.h
    for rc in (lib.lcg_hip_spmv(h, x.data_ptr(), y.data_ptr()), lib.lcg_hip_spmv_op(h, x.data_ptr(), y.data_ptr(), 1, 1),
               lib.lcg_hip_spmv_dot(h, x.data_ptr(), y.data_ptr(), x.data_ptr(), None),
               lib.lcg_hip_csr_set_kernel(h, 4), lib.lcg_hip_csr_set_packed(h, 1), lib.lcg_hip_csr_set_binned(h, 1),
               lib.lcg_hip_csr_set_tiled(h, 1), lib.lcg_hip_csr_set_ranges(h, 1), lib.lcg_hip_csr_distribute(h, n, 0),
               lib.lcg_hip_csr_build_ic0(h)):
        assert rc == E_ARG
    assert "complex64" in lib.lcg_hip_last_error().decode()
    # the fp64 / c128 ready-made callbacks end a solve with LCG_HIP_E_ARG
    assert lib.lcg_hip_csr_build_jacobi(h, None) == 0
    b = torch.ones(n, dtype=torch.complex128, device="cuda")
    for Afp, Mfp in (("clcg_hip_csr_ax", None), ("clcg_hip_csr_ax", "clcg_hip_jacobi_mx"), ("clcg_hip_csr_ax", "clcg_hip_ic0_mx")):
        m = torch.zeros_like(b)
        with pytest.raises(api.LcgHipError, match="-2003"):
            if Mfp:
                api.clcg_solver_preconditioned(Afp, Mfp, None, m, b, n, api.clcg_default_parameters(), A64)
            else:
                api.clcg_solver(Afp, None, m, b, n, api.clcg_default_parameters(), A64, api.CLCG_BICG_SYM)
    br = torch.ones(n, dtype=torch.float64, device="cuda")
    for Mfp in (None, "lcg_hip_jacobi_mx"):
        m = torch.zeros_like(br)
        with pytest.raises(api.LcgHipError, match="-2003"):
            if Mfp:
                api.lcg_solver_preconditioned("lcg_hip_csr_ax", Mfp, None, m, br, n, api.lcg_default_parameters(), A64)
            else:
                api.lcg_solver("lcg_hip_csr_ax", None, m, br, n, api.lcg_default_parameters(), A64, api.LCG_CG)
    # and the reverse: c128 / real handles in the c64 entries and callbacks
    x64 = torch.ones(n, dtype=torch.complex64, device="cuda"); y64 = torch.empty_like(x64)
    for H in (A128, Areal):
        assert lib.lcg_hip_spmv_c64(H.h, x64.data_ptr(), y64.data_ptr(), 0, 0) == E_ARG
        m = torch.zeros_like(x64)
        with pytest.raises(api.LcgHipError, match="-2003"):
            api.clcg_solver_c64("clcg_hip_csr_ax_c64", None, m, x64, n, api.clcg_default_parameters(), H, api.CLCG_BICG_SYM)
    assert lib.lcg_hip_csr_build_jacobi(A128.h, None) == 0
    m = torch.zeros_like(x64)
    with pytest.raises(api.LcgHipError, match="-2003"):
        api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_jacobi_mx_c64", None, m, x64, n,
                                           api.clcg_default_parameters(), A128)
    for H in (A64, A128, Areal):
        H.destroy()


# ------------------------------------------------------------------------------------------ 6. memory
def test_repeated_solves_do_not_grow_device_memory(api, lib):
    rp, ci, v = helmholtz(200)
    n = len(rp) - 1
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    b = np.ones(n, np.complex64)
    for rnd in range(3):
        A = api.CsrMatrix.from_csr_c64(rp, ci, v)
        assert lib.lcg_hip_csr_build_jacobi(A.h, None) == 0
        para = api.clcg_default_parameters(epsilon=1e-30, max_iterations=5)
        for kind in ("bicg", "bicg_sym", "pcg"):          # (BiCG builds A^H: freed by destroy)
            for _ in range(3):
                _solve(api, kind, A, b, para)
        if rnd == 0:
            torch.cuda.synchronize()
            free1 = torch.cuda.mem_get_info()[0]
        A.destroy()
        assert lib.lcg_hip_trim() == 0
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)
    assert free1 < free0


# ------------------------------------------------------------------------------------------ 7. C++ sample
def test_cpp_sample(api):
    """sample14's flow on case_10K_cA in fp32: the averaged error of each leg within 3x (+ 1e-7) of the checker's run of the
    same loop with the same cap (in fp32 the system may stop at the cap of 1000 before eps = 1e-6; the error is then the
    stagnation level, which two fp32 evaluations reach alike)."""
    from liblcg_amd import _lib
    _lib.build()
    bindir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "sample_csr_c64")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sample_csr_c64.cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", exe])
    p = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    errs = [float(e) for e in re.findall(r"Averaged error \(compared with ans_x\):\s*(\S+)", p.stdout)]
    assert len(errs) == 2, p.stdout
    rp, ci, v, b, xs = case("10K")
    ops = K.csr_ops(rp, ci, v, np.complex64)
    n = len(b)
    cfg = {"epsilon": 1e-6, "max_iterations": 1000}
    xs64 = xs.astype(np.complex64)
    refs = [K.bicg_sym(ops["A"], b, np.zeros(n, np.complex64), cfg), K.pcg(ops["A"], K.jacobi(rp, ci, v), b, np.zeros(n, np.complex64), cfg)]
    for e, r in zip(errs, refs):
        e_ref = float(np.linalg.norm((r["x"] - xs64).astype(np.complex128)) / n)
        assert e <= 3 * e_ref + 1e-7, (p.stdout, e_ref)
