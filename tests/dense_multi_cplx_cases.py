"""Systems, right-hand sides and drivers of the complex dense k-wide tests (tests/test_dense_multi_cplx_cpu.py,
tests/test_gpu_dense_multi_cplx_product.py, tests/test_gpu_dense_multi_cplx_solvers.py): a helper of the tests, not a conftest.
Modelled on tests/dense_multi_cases.py and tests/multi_cplx_cases.py.

Systems: K = G^T.G / n + 0.02 I + 0.1i (H^T.H / n + 0.2 I), then symmetrised; G, H uniform(-1, 1) from default_rng(5000 + n); xt with
real and imaginary parts in [1, 2]; b = K.xt in the reference's serial order (dense_checker.cmatvec).  Complex-symmetric with full
complex off-diagonals, not Hermitian, condition number about 31 - 33.  Columns of a batch: multi_cplx_cases.columns' (b, 1e-2 b whose
|m|^2 stays below 1, from k = 4 on a seeded random column and a zero column, ...)."""
import ctypes as C

import numpy as np

import dense_checker as dc
import multi_cplx_cases as cc
from multi_cplx_cases import ALREADY, BADEPS, BADMAXIT, BICG_SYM, CONV, E_ARG, KS, MAXIT, NANV, NOPRE, PCG, SIDS, SMALL, bits  # noqa: F401
from oracle import pyoracle as po

SIZES = (1, 2, 3, 65, 200, 513)
FACTOR, FLOOR = 50.0, 1e-9          # tests/dense_multi_cases.py: late_band's factor and floor
NAMES = ["k_zdnm_row", "k_zdnm_row_split", "k_zdnm_col"]
# the ranges of the iteration counts the numpy restatement needs at n = 65, 200, 513 over the non-zero columns (epsilon = 1e-10, abs_diff = 1)
COUNTS = {BICG_SYM: (21, 53), PCG: (45, 80)}

_SYSTEMS = {}


def system(n):
    """dict(K, A (= K, what multi_cplx_cases.restate reads), xt, b, n, key)."""
    if n not in _SYSTEMS:
        rng = np.random.default_rng(5000 + n)
        G = rng.uniform(-1.0, 1.0, (n, n)); H = rng.uniform(-1.0, 1.0, (n, n))
        K = G.T @ G / n + 0.02 * np.eye(n) + 0.1j * (H.T @ H / n + 0.2 * np.eye(n))
        K = np.ascontiguousarray((K + K.T) / 2.0)
        xt = rng.uniform(1.0, 2.0, n) + 1j * rng.uniform(1.0, 2.0, n)
        _SYSTEMS[n] = dict(K=K, A=K, xt=xt, b=dc.cmatvec(K, xt), n=n, key=("zdense", n))
    return _SYSTEMS[n]


def columns(S, k):
    return cc.columns(S["n"], S["b"], k)


def solution(S, bcol):
    return np.linalg.solve(S["K"], bcol)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def late_band(x_ref, x_alt, xt):
    """dense_multi_cases.late_band's rule: max(1e-9, 50 x the oracle's own response to swapping the product's summation order,
    0.25 x its distance to the column's solution)."""
    return max(FLOOR, FACTOR * rel(x_alt, x_ref), 0.25 * rel(xt, x_ref))


# ---------------------------------------------------------------------------------------------------------------- the oracle
_AX = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int)
_PF = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_int)
_RUNS = {}
_LIB = []


def oracle(S, sid, bcol, serial=True, m0=None, **para):
    """The oracle's own loop (orc_clbicg_symmetric, orc_clpcg: oracle/lcg_oracle.h) on ONE column, its product in Python: the
    checker's serial order (dense_checker.cmatvec), or numpy's K @ x.  Cached.  dict(x, ret, iters, residual)."""
    key = (S["key"], sid, np.ascontiguousarray(bcol).tobytes(), serial, None if m0 is None else np.ascontiguousarray(m0).tobytes(),
           tuple(sorted(para.items())))
    if key in _RUNS:
        return _RUNS[key]
    if not _LIB:
        po.build(ref=False)
        _LIB.append(po.Oracle("port").lib)
    lib, K, n = _LIB[0], S["K"], S["n"]
    inv = 1.0 / np.diag(K).copy()

    def cview(p, nn):
        return np.ctypeslib.as_array(p, (2 * nn,)).view(np.complex128)

    def ax(_, xp, yp, nn, layout, conj):
        assert layout == 0 and conj == 0
        x = cview(xp, nn)
        cview(yp, nn)[:] = dc.cmatvec(K, x) if serial else K @ x

    def mx(_, xp, yp, nn, layout, conj):
        cview(yp, nn)[:] = cview(xp, nn) * inv

    last = [0, 0.0]

    def pf(_, mp, conv, par, nn, kk):
        last[0], last[1] = kk, conv
        return 0

    a, mf, p = _AX(ax), _AX(mx), _PF(pf)
    cp = po.default_cpara(**para)
    m = np.zeros(n, np.complex128) if m0 is None else np.array(m0, dtype=np.complex128)
    b = np.ascontiguousarray(bcol, np.complex128)
    vp = lambda v: v.ctypes.data_as(C.c_void_p)
    if sid == PCG:
        f = lib.orc_clpcg; f.restype = C.c_int
        ret = f(a, mf, p, vp(m), vp(b), n, C.byref(cp), None)
    else:
        f = lib.orc_clbicg_symmetric; f.restype = C.c_int
        ret = f(a, p, vp(m), vp(b), n, C.byref(cp), None)
    _RUNS[key] = dict(x=m, ret=ret, iters=last[0], residual=last[1])
    return _RUNS[key]


# ---------------------------------------------------------------------------------------------------------------- the device
def zmulti(lib, api, sid, D, M, B, mem="device", **para):
    """One batched solve on the complex dense handle D: (rc, ret[k], iterations[k], residual[k], M afterwards).  M, B: (n, k)
    complex128 numpy arrays."""
    import torch
    k = B.shape[1]
    p = api.clcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    fn = lib.clcg_hip_dense_lpcg_multi if sid == PCG else lib.clcg_hip_dense_lbicg_sym_multi
    if mem == "device":
        Md, Bd = torch.from_numpy(np.ascontiguousarray(M).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(B)).cuda()
        rc = fn(D.h, k, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        out, Bh = cc.aligned_block(M), cc.aligned_block(B)
        rc = fn(D.h, k, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    return rc, list(ret), list(its), list(res), out
