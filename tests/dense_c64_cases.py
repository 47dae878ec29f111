"""Shapes, systems, drivers and tolerances of the complex64 dense tests (tests/test_dense_c64_cpu.py,
tests/test_gpu_dense_c64_product.py, tests/test_gpu_dense_c64_solvers.py): a helper of the tests, not a conftest.

Systems: tests/dense_multi_cplx_cases.py's system(n) -- complex-symmetric, full complex off-diagonals, condition number about 32 --
with K and xt rounded to complex64 and b = K.xt the exact product of the rounded inputs, rounded once.  Columns of a batch:
tests/multi_c64_cases.py's (b, 1e-2 b, a seeded random column, a zero column, ...).

The checker is tests/c64_checker.py with the dense product given three ways: the exact sum of the rounded inputs rounded once ("exact":
what the CSR tests hand it), and a sequential fp32 chain over the columns j ascending ("asc") or descending ("desc").  The capped-run
tolerance is tests/test_gpu_c64.py's _tol argument -- two correct fp32 evaluations of the recurrence lie about d from the exact iterate,
so at most 2 d apart, 4 d with margin, never below 64 u -- with d the LARGER of two distances measured on the checker alone: its
complex64 run against its complex128 twin, and its complex64 run with the product summed ascending against descending (the one thing
a dense row of n terms adds to a 5-entry CSR row: the summation order moves the product by about sqrt(n) u).  Nothing in it comes from
the device."""
import ctypes as C
import os

import numpy as np

import c64_checker as K
import dense_multi_cplx_cases as zc
import multi_c64_cases as mc
from multi_c64_cases import ALREADY, BADEPS, BADMAXIT, BICG_SYM, CONV, E_ARG, KS, MAXIT, NANV, NOPRE, PCG, SIDS, SMALL, U32, aligned_block, bits  # noqa: F401

SIZES = (1, 2, 3, 65, 200, 513)
BICG = "bicg"
NAMES = ["k_cdn_row", "k_cdn_row_split", "k_cdn_col", "k_cdnm_mfma", "k_cdnm_mfma_split"]
# M x N of the product tests and the branch each is the smallest to reach (dense.hpp's plans with NP = ceil(N / 2) packs per row, restated
# below): 1 x 1, 1 x 2, 3 x 1, 5 x 3 a pad entry and a partial tile; 16 x 64 one full tile, 17 x 33 one row past it and odd N; 65 x 513
# the unrolled body plus a tail (NP = 257: 33 steps of eight packs over four wavefronts, the last of one pack); 33 x 2050 the plan splits
# by itself (NP = 1025: four strips); 200 x 64 splits when forced (two strips of 16 packs: wavefronts 2 and 3 of a tile walk nothing);
# 4100 x 7 the column form with RG > 1 row groups and RS > 1 strips of rows
SHAPES = [(1, 1), (1, 2), (3, 1), (5, 3), (16, 64), (17, 33), (65, 513), (33, 2050), (200, 64), (4100, 7)]


# ---- dense.hpp's plans, restated ------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def packs(n):
    return (n + 1) // 2


def row_plan(M, NP, split, forced):
    S = 1
    if split:
        cap = max(1, NP // 16 if forced else NP // 256)
        S = min(_cdiv(8192, M), cap)
    pps = _cdiv(NP, S)
    return dict(W=min(64, max(4, _pow2ceil(pps))), S=_cdiv(NP, pps), pps=pps)


def row_auto(M, NP):
    split = M < 1024 and row_plan(M, NP, True, False)["S"] >= 2
    return row_plan(M, NP, split, False)


def col_plan(M, NP):
    CW = min(256, _pow2ceil(NP))
    RG = 256 // CW
    CT = _cdiv(NP, CW)
    RS = max(1, min(_cdiv(1024, CT), _cdiv(M, RG * 16)))
    rps = _cdiv(_cdiv(M, RS), RG) * RG
    return dict(CW=CW, RG=RG, CT=CT, RS=_cdiv(M, rps), rps=rps)


def can_split(m, n):
    return row_plan(m, packs(n), True, True)["S"] >= 2


# ---- systems ----------------------------------------------------------------------------------------------------------------------------
_SYSTEMS = {}


def chain_product(K64, x, descending=False):
    """K.x as one sequential fp32 chain per row over the columns in ascending (descending) order, numpy complex64 arithmetic."""
    x = np.asarray(x, np.complex64)
    acc = np.zeros(K64.shape[0], np.complex64)
    order = range(K64.shape[1] - 1, -1, -1) if descending else range(K64.shape[1])
    for j in order:
        acc = (acc + K64[:, j] * x[j]).astype(np.complex64)
    return acc


def system(n):
    """dict(key, n, K (complex64), K128 (the same values), xt, b, ops: exact / asc / desc products and AH)."""
    if n not in _SYSTEMS:
        Z = zc.system(n)
        K64 = np.ascontiguousarray(Z["K"].astype(np.complex64))
        K128 = K64.astype(np.complex128)
        xt = Z["xt"].astype(np.complex64)
        KH = np.ascontiguousarray(K128.conj().T)
        ops = {"exact": lambda x: K128 @ np.asarray(x).astype(np.complex128),
               "asc": lambda x: chain_product(K64, x, False),
               "desc": lambda x: chain_product(K64, x, True),
               "AH": lambda x: KH @ np.asarray(x).astype(np.complex128)}
        _SYSTEMS[n] = dict(key=("cdense", n), n=n, K=K64, K128=K128, xt=xt, b=(K128 @ xt.astype(np.complex128)).astype(np.complex64), ops=ops)
    return _SYSTEMS[n]


def columns(S, k):
    return mc.columns(S, k)


def jacobi(S, dtype=np.complex64):
    """z = x .* (1 / diag) in the working precision, the reciprocal by cuCdivf's formula (c64_checker.Prec.div): what c64_checker.jacobi
    restates for CSR arrays, on the dense diagonal."""
    P = K.Prec(dtype)
    inv = np.array([P.div(P.C(1.0), P.C(d)) for d in np.diag(S["K"])], dtype)
    return lambda x: (inv * np.asarray(x, dtype)).astype(dtype)


# ---- the checker ------------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def checker_run(S, sid, bcol, tag, dtype=np.complex64, order="exact", **para):
    """The checker's run of one column alone from the zero guess with the product summed as `order` says; cached, never modified."""
    key = (S["key"], sid, tag, np.dtype(dtype).name, order, tuple(sorted(para.items())))
    if key not in _RUNS:
        m0 = np.zeros(S["n"], dtype)
        ax = S["ops"][order]
        with np.errstate(all="ignore"):
            if sid == PCG:
                _RUNS[key] = K.pcg(ax, jacobi(S, dtype), bcol, m0, para, dtype)
            elif sid == BICG:
                _RUNS[key] = K.bicg(ax, S["ops"]["AH"], bcol, m0, para, dtype)
            else:
                _RUNS[key] = K.bicg_sym(ax, bcol, m0, para, dtype)
    return _RUNS[key]


def _dist(a, b):
    return float(np.linalg.norm(a.astype(np.complex128) - b.astype(np.complex128)) / max(np.linalg.norm(b.astype(np.complex128)), 1e-30))


def tol_run(S, sid, bcol, tag, **para):
    """(the checker's complex64 run, tol, the two orders agree on code and count): tol = max(4 d, 64 x 2^-24), d the larger of the
    complex64 run's distance to its complex128 twin and of the ascending run's distance to the descending one (module docstring)."""
    a = checker_run(S, sid, bcol, tag, np.complex64, "exact", **para)
    e = checker_run(S, sid, bcol, tag, np.complex128, "exact", **para)
    # (BiCG's adjoint product is given exactly in every run: the orders are those of the forward product)
    up = checker_run(S, sid, bcol, tag, np.complex64, "asc", **para); dn = checker_run(S, sid, bcol, tag, np.complex64, "desc", **para)
    with np.errstate(all="ignore"):
        d = max(_dist(a["x"], e["x"]), _dist(up["x"], dn["x"]))
    agree = (up["ret"], up["iters"]) == (dn["ret"], dn["iters"]) == (a["ret"], a["iters"])
    return a, max(4.0 * d, 64 * U32), agree


# ---- the device -------------------------------------------------------------------------------------------------------------------------
def cmulti64_dense(lib, api, sid, D, M, B, mem="device", **para):
    """One batched solve on the complex64 dense handle D: (rc, ret[k], iterations[k], residual[k], M afterwards).  M, B: (n, k)
    complex64 numpy arrays."""
    import torch
    k = B.shape[1]
    p = api.clcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    fn = lib.clcg_hip_dense_lpcg_multi_c64 if sid == PCG else lib.clcg_hip_dense_lbicg_sym_multi_c64
    if mem == "device":
        Md = torch.from_numpy(np.ascontiguousarray(M, np.complex64).copy()).cuda()
        Bd = torch.from_numpy(np.ascontiguousarray(B, np.complex64)).cuda()
        rc = fn(D.h, k, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        out, Bh = aligned_block(M), aligned_block(B)
        rc = fn(D.h, k, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    return rc, list(ret), list(its), list(res), out


# ---- the staging header and its table ---------------------------------------------------------------------------------------------------
ENTRIES = sorted(["lcg_hip_dense_create_c64", "clcg_hip_dense_matvec_c64", "clcg_hip_dense_ax_c64", "clcg_hip_dense_jacobi_mx_c64",
                  "lcg_hip_dense_build_jacobi_c64", "clcg_hip_dense_matmat_c64", "clcg_hip_dense_op_multi_dot_c64",
                  "clcg_hip_dense_lbicg_sym_multi_c64", "clcg_hip_dense_lpcg_multi_c64", "clcg_hip_dense_kernel_name_c64"])


def staging_header():
    from conftest import ROOT
    return os.path.join(ROOT, "include", "lcg_hip_staging_dense_c64.h")


# The lines the staged entries will bring to stream_cases.STREAM_COVERAGE when they move to lcg_hip.h, in that table's format
_STREAMS = "test_gpu_dense_c64_solvers.py"
STAGING_COVERAGE = {
    "lcg_hip_dense_create_c64": _STREAMS + "::test_callers_stream",
    "clcg_hip_dense_matvec_c64": _STREAMS + "::test_callers_stream",
    "clcg_hip_dense_ax_c64": _STREAMS + "::test_callers_stream",
    "clcg_hip_dense_jacobi_mx_c64": _STREAMS + "::test_callers_stream",
    "lcg_hip_dense_build_jacobi_c64": _STREAMS + "::test_callers_stream",
    "clcg_hip_dense_matmat_c64": _STREAMS + "::test_callers_stream",
    "clcg_hip_dense_op_multi_dot_c64": _STREAMS + "::test_callers_stream",
    "clcg_hip_dense_lbicg_sym_multi_c64": _STREAMS + "::test_callers_stream",
    "clcg_hip_dense_lpcg_multi_c64": _STREAMS + "::test_callers_stream",
    "clcg_hip_dense_kernel_name_c64": ("exempt", "a query answered on the host: enqueues nothing"),
}
