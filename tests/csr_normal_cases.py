"""Systems, right-hand sides, the Python-product oracle driver and the drivers of the entries of include/lcg_hip_staging_csr_normal.h
(K^T.x, K^T.K.x and the batched loops on K^T.K of a rectangular CSR matrix): shared by tests/test_csr_normal_cases_cpu.py,
tests/test_gpu_csr_normal_product.py and tests/test_gpu_csr_normal_solvers.py.  A helper of the tests, not a conftest.  Systems and
oracle driver follow tests/dense_multi_cases.py, ENTRIES and STAGING_COVERAGE follow tests/multi_box_cases.py.

Systems: every row of K draws t distinct columns with default_rng(seed).choice (stored ascending) and values uniform(-1, 1); xt in
[1, 2]; b = K^T.(K.xt) in the reference's serial order (the oracle's row-by-row product over K, then over the stable transposition of
K).  The table (CG's count to 1e-10 from zeros by the oracle, tests/test_csr_normal_cases_cpu.py):
  edge65     600 x 65, t = 6                          the wavefront edge of the vector passes
  wide513    65 x 513, t = 12, stacked on 0.5 I       578 x 513: a wide K, many one-entry rows, the 513 edge
  dense3000  3000 x 513, t = 8, column 0 and row 7 dense    a row of K^T of 3000 entries (longer than the k-wide product's 2304-entry
                                                      window), a row of K of 513
  tall9000   9000 x 33, t = 4, column 0 dense         a row of K^T longer than the 8192 entries a workgroup sorts in LDS: the merge passes
  main       600 x 513, t = 8                         the slow one
  small      80 x 65, t = 8
  tiny7x3, tiny5x2, tiny3x1                           one block, n k / 2 pieces
PRODUCT_ONLY: 200 x 300 with empty rows, empty columns and duplicate (row, column) entries, unsorted rows (no Jacobi, no solve).
Columns of a batch: dense_multi_cases.columns' recipe {b, random, 2 b, 0, -b, 3 x random, 0.5 b, 1e-3 b}.
"""
import ctypes as C
import os

import numpy as np

from oracle import pyoracle as po

CONV, ALREADY, MAXIT, NANV, NOPRE, BADEPS, BADCAP, E_ARG, E_NO_DEVICE = 0, 2, -1019, -1017, -1018, -1021, -1022, -2003, -2001
CG, PCG, CGS, BICGSTAB, BICGSTAB2, PG, SPG = range(7)
KS = (2, 4, 8)
FACTOR, FLOOR = 50.0, 1e-9          # tests/conftest.py: check_converged_run's factor and floor
EPS = 1e-10

# name -> (M of the drawn part, N, t, dense column 0, a dense row (or None), sqrt(lambda) of stacked rows (or None))
TABLE = {
    "edge65": (600, 65, 6, False, None, None),
    "wide513": (65, 513, 12, False, None, 0.5),
    "dense3000": (3000, 513, 8, True, 7, None),
    "tall9000": (9000, 33, 4, True, None, None),
    "main": (600, 513, 8, False, None, None),
    "small": (80, 65, 8, False, None, None),
    "tiny7x3": (7, 3, 2, False, None, None),
    "tiny5x2": (5, 2, 2, False, None, None),
    "tiny3x1": (3, 1, 1, False, None, None),
}
# CG's count to EPS from zeros by the oracle's lcg (the reference's stop rule |g|^2 / max(|m|^2, 1) <= 1e-10, serial-order product):
# the run must stay within these.  The issue that asked for these systems quotes 10 / 15 / 16 / 5 / 90 / 52 and cond 4 / 35 / 200 / 700
# for its own draws; it fixes shapes, t, the dense column / row and the value ranges, not the seed or the stop rule of its count.  The
# seed rule here is default_rng(1000 * M + N) (dense_multi_cases.system's), drawn in the order columns of row 0, values of row 0,
# columns of row 1, ..., then xt: the same shapes give cond 4 / 34 / 230 / 750 and the counts below, 20-40 % above the quoted ones.
CG_COUNTS = {"edge65": 13, "wide513": 17, "dense3000": 22, "tall9000": 8, "main": 114, "small": 68, "tiny7x3": 3, "tiny5x2": 2, "tiny3x1": 1}
# cond(K^T.K) by numpy, to two digits (what makes the counts what they are)
CONDS = {"edge65": 4.0, "wide513": 34.0, "dense3000": 230.0, "tall9000": 12.0, "main": 750.0, "small": 470.0}
TINY = ("tiny7x3", "tiny5x2", "tiny3x1")
# Systems on which the oracle's serial-against-pairwise spread does not measure how far two roundings of one run drift apart: on
# dense3000 (one eigenvalue of K^T.K near 1000, the others below 30) the oracle's run on 1e-3 b and 1e-3 x its run on b are 7e-6 apart
# at 15 iterations where the spread says 7e-8, and CGS moves by 7e-5 under a 1-ulp change of b at 5 iterations where the spread says
# 7e-7 (tests/test_csr_normal_cases_cpu.py pins both).  On such a system response() below takes, besides the spread, the oracle's
# response to SEEDS seeded 1-ulp changes of b -- the band of the box loops and of conftest.check_converged_run -- and every check runs.
TOUCHY = ("dense3000",)

_SYSTEMS = {}
_PORT = []


def port():
    if not _PORT:
        po.build(ref=False)
        _PORT.append(po.Oracle("port"))
    return _PORT[0]


def transpose_host(rp, ci, v, n_cols):
    """The stable transposition of a CSR matrix -- the rule of lcg_hip_csr_build_normal: a row of K^T holds a column of K by source
    row, duplicates in K's own entry order.  (rowptr, col, val) with int32 indices."""
    rp = np.asarray(rp, np.int64); ci = np.asarray(ci, np.int64)
    order = np.argsort(ci, kind="stable")
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    rpT = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n_cols))])
    return rpT.astype(np.int32), rows[order].astype(np.int32), np.asarray(v)[order]


def _finish(name, rp, ci, v, m, n, rng):
    rpT, ciT, vT = transpose_host(rp, ci, v, n)
    S = dict(key=name, m=m, n=n, rp=rp, ci=ci, v=v, rpT=rpT, ciT=ciT, vT=vT)
    S["xt"] = rng.uniform(1.0, 2.0, n)
    S["b"] = ata(S, S["xt"])
    for a in (rp, ci, v, rpT, ciT, vT, S["xt"], S["b"]):
        a.setflags(write=False)
    return S


def system(name):
    """dict(key, m, n, rp, ci, v (K), rpT, ciT, vT (K^T), xt, b).  Nobody writes into it."""
    if name in _SYSTEMS:
        return _SYSTEMS[name]
    m, n, t, dense_col, dense_row, lam = TABLE[name]
    rng = np.random.default_rng(1000 * m + n)
    rows = []
    for i in range(m):
        cols = rng.choice(n, t, replace=False)
        if dense_row is not None and i == dense_row:
            cols = np.arange(n)
        elif dense_col and 0 not in cols:
            cols[0] = 0                 # (the first one drawn: any column gives way)
        cols = np.sort(cols)
        rows.append((cols, rng.uniform(-1.0, 1.0, len(cols))))
    if lam is not None:
        rows += [(np.array([j]), np.array([lam])) for j in range(n)]
    rp = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
    ci = np.concatenate([c for c, _ in rows]).astype(np.int32)
    v = np.concatenate([w for _, w in rows])
    _SYSTEMS[name] = _finish(name, rp, ci, v, len(rows), n, rng)
    return _SYSTEMS[name]


def product_only():
    """200 x 300: rows 3, 50 and 199 empty, columns 0, 17 and 299 empty, unsorted rows, and every fifth row repeats two of its
    (row, column) pairs with other values."""
    if "product_only" in _SYSTEMS:
        return _SYSTEMS["product_only"]
    m, n = 200, 300
    rng = np.random.default_rng(200300)
    live = np.setdiff1d(np.arange(n), [0, 17, 299])
    rows = []
    for i in range(m):
        if i in (3, 50, 199):
            rows.append((np.zeros(0, np.int64), np.zeros(0)))
            continue
        cols = rng.choice(live, 7, replace=False)
        if i % 5 == 0:
            cols = np.concatenate([cols, cols[[1, 4]], cols[[1]]])
        rows.append((cols, rng.uniform(-1.0, 1.0, len(cols))))
    rp = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
    ci = np.concatenate([c for c, _ in rows]).astype(np.int32)
    v = np.concatenate([w for _, w in rows])
    _SYSTEMS["product_only"] = _finish("product_only", rp, ci, v, m, n, rng)
    return _SYSTEMS["product_only"]


# ---------------------------------------------------------------------------------------------------------------- products
def _pairwise(rp, ci, v, x):
    """A.x with every row's products added as a binary tree over adjacent pairs (rows grouped by length, vectorised)."""
    rp = np.asarray(rp, np.int64)
    lens = np.diff(rp)
    y = np.zeros(len(lens))
    prod = v * x[ci]
    for L in np.unique(lens):
        if L == 0:
            continue
        r = np.flatnonzero(lens == L)
        a = prod[rp[r][:, None] + np.arange(L)[None, :]]
        while a.shape[1] > 1:
            w = a.shape[1]
            h = a[:, 0:w - (w & 1):2] + a[:, 1:w:2]
            a = np.concatenate([h, a[:, w - 1:w]], axis=1) if w & 1 else h
        y[r] = a[:, 0]
    return y


def kx(S, x, serial=True):
    return port().csr_matvec(S["rp"], S["ci"], S["v"], x) if serial else _pairwise(S["rp"], S["ci"], S["v"], x)


def ktx(S, t, serial=True):
    return port().csr_matvec(S["rpT"], S["ciT"], S["vT"], t) if serial else _pairwise(S["rpT"], S["ciT"], S["vT"], t)


def ata(S, x, serial=True):
    """K^T.(K.x): the reference's serial order (entry by entry along a row of K, by source row along a column), or pairwise."""
    return ktx(S, kx(S, x, serial), serial)


def normal_diagonal(S):
    """sum_i K(i,c)^2 per column, serially by source row."""
    return port().csr_matvec(S["rpT"], np.zeros(len(S["ciT"]), np.int32), S["vT"] * S["vT"], np.ones(1))


def columns(S, k):
    """The k right-hand sides of a batch (dense_multi_cases.columns' recipe), (n, k) row-major."""
    n, b = S["n"], S["b"]
    r = np.random.default_rng(77)
    cols = [b, r.standard_normal(n), 2.0 * b, np.zeros(n), -b, 3.0 * r.standard_normal(n), 0.5 * b, 1e-3 * b]
    return np.ascontiguousarray(np.stack(cols[:k], axis=1))


def dense(S):
    K = np.zeros((S["m"], S["n"]))
    np.add.at(K, (np.repeat(np.arange(S["m"]), np.diff(S["rp"])), S["ci"]), S["v"])
    return K


def solution(S, bcol):
    K = dense(S)
    return np.linalg.solve(K.T @ K, bcol)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def late_band(x_ref, response_, xt):
    """check_converged_run's rule 3 (tests/test_gpu_dense.py: _late_band) with the oracle's response() as its second term."""
    return max(FLOOR, FACTOR * response_, 0.25 * rel(xt, x_ref))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def perturbed(b, seed):
    """b with seeded changes of at most an ulp (conftest.check_converged_run's perturbation)."""
    return b * (1.0 + 1e-16 * np.random.default_rng(1000 + seed).standard_normal(len(b)))


# ---------------------------------------------------------------------------------------------------------------- the oracle
_AX = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int)
_PF = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_int)
_NAMES = ["orc_lcg", "orc_lpcg", "orc_lcgs", "orc_lbicgstab", "orc_lbicgstab2", "orc_lpg", "orc_lspg"]
_RUNS = {}


def oracle(S, sid, bcol, cap, eps=EPS, serial=True, m0=None, low=None, hig=None, abs_diff=0, **more):
    """The oracle's own loop (oracle/lcg_oracle.h) on ONE column with K^T.K as a Python product: the serial order, or pairwise.
    PCG: the normal Jacobi.  PG / SPG: between low and hig, from the guess as it is (the loop projects it).  Cached on the column's
    bytes; nobody writes into a cached result.  dict(x, ret, iters, n_ax)."""
    key = (S["key"], sid, bcol.tobytes(), cap, eps, serial, None if m0 is None else m0.tobytes(),
           None if low is None else (low.tobytes(), hig.tobytes()), abs_diff, tuple(sorted(more.items())))
    if key in _RUNS:
        return _RUNS[key]
    lib, n = port().lib, S["n"]
    inv = 1.0 / normal_diagonal(S) if sid == PCG else None
    calls = [0]

    def ax(_, xp, yp, nn):
        calls[0] += 1
        np.ctypeslib.as_array(yp, (nn,))[:] = ata(S, np.ctypeslib.as_array(xp, (nn,)).copy(), serial)

    def mx(_, xp, yp, nn):
        np.ctypeslib.as_array(yp, (nn,))[:] = np.ctypeslib.as_array(xp, (nn,)) * inv

    last = [0]

    def pf(_, mp, conv, par, nn, kk):
        last[0] = kk
        return 0

    a, mf, p = _AX(ax), _AX(mx), _PF(pf)
    para = po.default_para(epsilon=eps, abs_diff=abs_diff, max_iterations=cap, **more)
    m = np.zeros(n) if m0 is None else np.array(m0, dtype=np.float64)
    b = np.ascontiguousarray(bcol)
    vp = lambda w: w.ctypes.data_as(C.c_void_p)
    f = getattr(lib, _NAMES[sid]); f.restype = C.c_int
    if sid == PCG:
        ret = f(a, mf, p, vp(m), vp(b), n, C.byref(para), None)
    elif sid >= PG:
        lo, hi = np.ascontiguousarray(low), np.ascontiguousarray(hig)
        ret = f(a, p, vp(m), vp(b), vp(lo), vp(hi), n, C.byref(para), None)
    else:
        ret = f(a, p, vp(m), vp(b), n, C.byref(para), None)
    m.setflags(write=False)
    _RUNS[key] = dict(x=m, ret=ret, iters=last[0], n_ax=calls[0])
    return _RUNS[key]


SEEDS = 4


def response(S, sid, bcol, cap, **kw):
    """The oracle's own response at that count, what FACTOR multiplies in every band: the relative distance between its serial-order
    and its pairwise-order run; on a TOUCHY system the larger of that and its distance to its runs on SEEDS seeded 1-ulp changes of b."""
    ref = oracle(S, sid, bcol, cap, **kw)
    out = rel(oracle(S, sid, bcol, cap, serial=False, **kw)["x"], ref["x"])
    if S["key"] in TOUCHY:
        out = max([out] + [rel(oracle(S, sid, perturbed(bcol, seed), cap, **kw)["x"], ref["x"]) for seed in range(SEEDS)])
    return out


# ---------------------------------------------------------------------------------------------------------------- the device
def aligned(a):
    """A 16-byte aligned copy of a float64 array."""
    raw = np.zeros(a.size + 2)
    off = 0 if raw.ctypes.data % 16 == 0 else 1
    out = raw[off:off + a.size].reshape(a.shape)
    out[:] = a
    return out


def handle(api, S, normal=True, jacobi=True):
    """The CSR handle of K with its normal state (and the normal Jacobi)."""
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"], n_cols=S["n"])
    if normal:
        A.build_normal()
        if jacobi:
            A.build_jacobi_normal()
    return A


def multi(lib, api, sid, A, M, B, mem="device", **para):
    """One batched CG / PCG solve on K^T.K: (rc, ret[k], iterations[k], residual[k], M afterwards).  M, B: (n, k) numpy arrays."""
    import torch
    k = B.shape[1]
    para.setdefault("abs_diff", 0)
    p = api.lcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    fn = lib.lcg_hip_csr_normal_lpcg_multi if sid == PCG else lib.lcg_hip_csr_normal_lcg_multi
    if mem == "device":
        Md, Bd = torch.from_numpy(np.ascontiguousarray(M).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(B)).cuda()
        rc = fn(A.h, k, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        out, Bh = aligned(M), aligned(B)
        rc = fn(A.h, k, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    return rc, list(ret), list(its), list(res), out


def box(lib, api, sid, A, M, B, low, hig, mem="device", **para):
    """One batched PG / SPG solve on K^T.K: (rc, ret[k], iterations[k], products[k], residual[k], M afterwards)."""
    import torch
    k = B.shape[1]
    p = api.lcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); prods = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    fn = lib.lcg_hip_csr_normal_solver_constrained_multi
    if mem == "device":
        Md, Bd = torch.from_numpy(np.ascontiguousarray(M).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(B)).cuda()
        ld, hd = torch.from_numpy(np.ascontiguousarray(low)).cuda(), torch.from_numpy(np.ascontiguousarray(hig)).cuda()
        rc = fn(A.h, k, sid, Md.data_ptr(), Bd.data_ptr(), ld.data_ptr(), hd.data_ptr(), C.byref(p), ret, its, prods, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        out, Bh = aligned(M), aligned(B)
        lo, hi = np.ascontiguousarray(low), np.ascontiguousarray(hig)
        rc = fn(A.h, k, sid, out.ctypes.data, Bh.ctypes.data, lo.ctypes.data, hi.ctypes.data, C.byref(p), ret, its, prods, res, 0)
    return rc, list(ret), list(its), list(prods), list(res), out


# ------------------------------------------------------------------------------------------ the staging header and its table
ENTRIES = sorted([
    "lcg_hip_csr_cols", "lcg_hip_csr_build_normal", "lcg_hip_csr_normal_info", "lcg_hip_csr_normal_arrays",
    "lcg_hip_spmv_t", "lcg_hip_csr_ata", "lcg_hip_csr_ata_ax", "lcg_hip_csr_build_jacobi_normal", "lcg_hip_csr_jacobi_normal_mx",
    "lcg_hip_spmm_t", "lcg_hip_csr_ata_multi", "lcg_hip_csr_ata_multi_dot",
    "lcg_hip_csr_normal_lcg_multi", "lcg_hip_csr_normal_lpcg_multi", "lcg_hip_csr_normal_solver_constrained_multi"])
# the entries that launch work: LCG_HIP_E_NO_DEVICE without a device
COMPUTE = [e for e in ENTRIES if e not in ("lcg_hip_csr_cols",)]


def staging_header():
    from conftest import ROOT
    return os.path.join(ROOT, "include", "lcg_hip_staging_csr_normal.h")


# The lines the staged entries will bring to stream_cases.STREAM_COVERAGE when they move to lcg_hip.h, in that table's format
_STREAMS = "test_gpu_csr_normal_solvers.py::test_callers_stream"
STAGING_COVERAGE = {name: _STREAMS for name in ENTRIES}
STAGING_COVERAGE["lcg_hip_csr_cols"] = ("exempt", "a query answered on the host: enqueues nothing")
