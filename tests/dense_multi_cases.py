"""Systems, right-hand sides and drivers of tests/test_gpu_dense_multi_solvers.py (the batched CG / PCG on a dense handle): a helper
of the tests, not a conftest.  Modelled on tests/multi_cases.py; the Python-product oracle driver of tests/test_gpu_dense.py is
restated here (a helper does not import from a test module).

Systems: K = uniform(-1, 1), seeded, xt in [1, 2], b = K^T.(K.xt) in the reference's serial order (dense_checker.ata); the operator
is K^T.K (normal = 1).  One square SPD system for normal = 0: K = G^T.G / 200 + I, 200 x 200, b = K.xt.
Columns of a batch: {b, a seeded random vector, 2 b, 0, -b, 3 x another random vector, 0.5 b, 1e-3 b}; k = 2 and 4 take the first
columns, so every k holds b and a column whose solution is not a multiple of xt, and k >= 4 a zero column.
"""
import ctypes as C

import numpy as np

import dense_checker as dc
from oracle import pyoracle as po

CONV, ALREADY, MAXIT, NANV, NOPRE, BADEPS, BADCAP, E_ARG = 0, 2, -1019, -1017, -1018, -1021, -1022, -2003
CG, PCG = 0, 1
KS = (2, 4, 8)
FACTOR, FLOOR = 50.0, 1e-9          # tests/conftest.py: check_converged_run's factor and floor (tests/test_gpu_dense.py)
MAIN = (300, 240)
EDGES = [(3, 1), (5, 2), (7, 3), (80, 65), (600, 513)]      # vector passes over n k / 2 pieces at 1, 2, 3, 65 and 513 rows

_SYSTEMS = {}


def system(m, n, normal=True):
    """dict(K, xt, b, normal, n, key)."""
    key = (m, n, normal)
    if key not in _SYSTEMS:
        rng = np.random.default_rng(1000 * m + n)
        if normal:
            K = rng.uniform(-1.0, 1.0, (m, n))
            xt = rng.uniform(1.0, 2.0, n)
            b = dc.ata(K, xt)
        else:
            assert m == n
            G = rng.uniform(-1.0, 1.0, (n, n))
            K = G.T @ G / 200.0 + np.eye(n)
            K = (K + K.T) / 2.0
            xt = rng.uniform(1.0, 2.0, n)
            b = dc.matvec(K, xt)
        _SYSTEMS[key] = dict(K=K, xt=xt, b=b, normal=normal, n=n, key=key)
    return _SYSTEMS[key]


def columns(S, k):
    """The k right-hand sides of a batch (module docstring), (n, k) row-major."""
    n, b = S["n"], S["b"]
    r = np.random.default_rng(77)
    cols = [b, r.standard_normal(n), 2.0 * b, np.zeros(n), -b, 3.0 * r.standard_normal(n), 0.5 * b, 1e-3 * b]
    return np.ascontiguousarray(np.stack(cols[:k], axis=1))


def solution(S, bcol):
    """The solution of the column's system, from numpy (the operators here have condition numbers of a few hundred)."""
    K = S["K"]
    A = K.T @ K if S["normal"] else K
    return np.linalg.solve(A, bcol)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def late_band(x_ref, x_alt, xt):
    """check_converged_run's rule 3 (tests/test_gpu_dense.py: _late_band)."""
    return max(FLOOR, FACTOR * rel(x_alt, x_ref), 0.25 * rel(xt, x_ref))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the oracle
_AX = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int)
_PF = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_int)
_RUNS = {}
_LIB = []


def oracle(S, sid, bcol, cap, eps, serial=True, m0=None):
    """The oracle's own loop (orc_lcg, orc_lpcg: oracle/lcg_oracle.h) on ONE column, its product in Python: the checker's serial
    order (dense_checker), or numpy's.  Cached.  dict(x, ret, iters)."""
    key = (S["key"], sid, bcol.tobytes(), cap, eps, serial, None if m0 is None else m0.tobytes())
    if key in _RUNS:
        return _RUNS[key]
    if not _LIB:
        po.build(ref=False)
        _LIB.append(po.Oracle("port").lib)
    lib, K, n, normal = _LIB[0], S["K"], S["n"], S["normal"]
    inv = 1.0 / (dc.normal_diagonal(K) if normal else np.diag(K).copy())

    def ax(_, xp, yp, nn):
        x = np.ctypeslib.as_array(xp, (nn,)); y = np.ctypeslib.as_array(yp, (nn,))
        if normal:
            y[:] = dc.ata(K, x) if serial else K.T @ (K @ x)
        else:
            y[:] = dc.matvec(K, x) if serial else K @ x

    def mx(_, xp, yp, nn):
        np.ctypeslib.as_array(yp, (nn,))[:] = np.ctypeslib.as_array(xp, (nn,)) * inv

    last = [0]

    def pf(_, mp, conv, par, nn, kk):
        last[0] = kk
        return 0

    a, mf, p = _AX(ax), _AX(mx), _PF(pf)
    para = po.default_para(epsilon=eps, abs_diff=0, max_iterations=cap)
    m = np.zeros(n) if m0 is None else np.array(m0, dtype=np.float64)
    b = np.ascontiguousarray(bcol)
    vp = lambda v: v.ctypes.data_as(C.c_void_p)
    if sid == PCG:
        f = lib.orc_lpcg; f.restype = C.c_int
        ret = f(a, mf, p, vp(m), vp(b), n, C.byref(para), None)
    else:
        f = lib.orc_lcg; f.restype = C.c_int
        ret = f(a, p, vp(m), vp(b), n, C.byref(para), None)
    _RUNS[key] = dict(x=m, ret=ret, iters=last[0])
    return _RUNS[key]


# ---------------------------------------------------------------------------------------------------------------- the device
def multi(lib, api, sid, D, normal, M, B, mem="device", **para):
    """One batched solve on the dense handle D: (rc, ret[k], iterations[k], residual[k], M afterwards).  M, B: (n, k) numpy arrays."""
    import torch
    k = B.shape[1]
    para.setdefault("abs_diff", 0)
    p = api.lcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    fn = lib.lcg_hip_dense_lpcg_multi if sid == PCG else lib.lcg_hip_dense_lcg_multi
    if mem == "device":
        Md, Bd = torch.from_numpy(M.copy()).cuda(), torch.from_numpy(np.ascontiguousarray(B)).cuda()
        rc = fn(D.h, k, int(normal), Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        raw = np.zeros(M.size + 2); off = 0 if raw.ctypes.data % 16 == 0 else 1
        out = raw[off:off + M.size].reshape(M.shape); out[:] = M
        rawb = np.zeros(B.size + 2); offb = 0 if rawb.ctypes.data % 16 == 0 else 1
        Bh = rawb[offb:offb + B.size].reshape(B.shape); Bh[:] = B
        rc = fn(D.h, k, int(normal), out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    return rc, list(ret), list(its), list(res), out
