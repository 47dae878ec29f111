"""Systems, shadow vectors, a numpy restatement and the drivers shared by the tests of the batched complex BiCGStab
(clcg_hip_lbicgstab_multi) and of the two product modes it takes its sums from (clcg_hip_spmm_inner, clcg_hip_spmm_dot2):
tests/test_gpu_multi_cbicgstab.py, tests/test_gpu_streams_cbicgstab.py and tests/test_multi_cbicg_cases_cpu.py, which shows with the
oracle alone that the cases are what they claim.  Modelled on tests/multi_bicg_cases.py; a helper of the tests, not a conftest.

Systems: those of tests/multi_cplx_cases.py with every strictly upper entry halved -- non-symmetric, non-Hermitian, and as diagonally
dominant as they were.  b = A.xt with multi_cplx_cases' xt.
  * "chain" 1, 2, 3: kernel edges only (BiCGStab ends such systems by an exact half step, and the 0 / 0 that follows is decided by
    one rounding);  "chain" 65: one block;  "chain" 513: a few blocks;
  * "helm" 40: n = 1600;  "helm" 182: 518 row blocks (the fold) and a second stride of a vector pass;
  * "band30" 1029: R = 16 with a partial last block;  "band30" 8197: R = 16 folded;  "band140" 2051: R = 4 folded;
    "band260" 261: R = 4, the last block of one row.
Columns and guesses: multi_cplx_cases.columns / guesses.

Shadow vectors.  The library's default draw is real (rbar0 in [1, 2] + 0i) and cannot tell conj(rb) from rb: every comparison hands
BOTH sides shadow(port, n, seed) = the oracle's vecrnd(n, seed, 1 + 1j, 2 + 2j), whose imaginary parts are not zero.  One case uses the
seed's own draw, port.vecrnd(n, seed).

pcbicgstab() restates the x-space loop of solvers_multi_cbicg.hip (plain: clcg.cpp:524-679 itself) in numpy, written new here.  Its
sums are cumulative sums in index order, as the oracle's are.

Caps.  A numpy probe on the CPU (numpy-drawn shadow, both rules) needs 7-13 iterations on the chains and helms, 4-8 on the bands
(Jacobi: 2-5): capped comparisons run 3 iterations at epsilon = 1e-20, the chains and helms also 6;
tests/test_multi_cbicg_cases_cpu.py asserts with the oracle that every plain capped case ends at its cap.
"""
import ctypes as C
import os
import re

import numpy as np
import scipy.sparse as sp

import multi_cplx_cases as cc

CONV, ALREADY, MAXIT, NANV = cc.CONV, cc.ALREADY, cc.MAXIT, cc.NANV      # (CLCG_NAN_VALUE and the cap's code share -1019)
NOPRE, BADEPS, BADMAXIT, E_ARG = cc.NOPRE, cc.BADEPS, cc.BADMAXIT, cc.E_ARG
M_NONE, M_JACOBI, M_IC0, M_ILU0 = -1, 0, 1, 2
BICGSTAB = 3                        # the oracle's solver id (CLCG_BICGSTAB)
KS = cc.KS
MM_MG = cc.MM_MG
RULES = {"rel": dict(abs_diff=0, epsilon=1e-20), "abs": dict(abs_diff=1, epsilon=1e-10)}    # the probe's two rules
CAP_EPS = 1e-20
SEED = 2024

TINY = [("chain", 1), ("chain", 2), ("chain", 3)]
CHAINS_HELMS = [("chain", 65), ("chain", 513), ("helm", 40), ("helm", 182)]
BANDS = [("band30", 1029), ("band30", 8197), ("band140", 2051), ("band260", 261)]
NON_TINY = CHAINS_HELMS + BANDS
# (kind, n) -> (R, folded: more than MM_MG row blocks)
CLASS = {("chain", 1): (64, False), ("chain", 2): (64, False), ("chain", 3): (64, False), ("chain", 65): (64, False),
         ("chain", 513): (64, False), ("helm", 40): (64, False), ("helm", 182): (64, True), ("band30", 1029): (16, False),
         ("band30", 8197): (16, True), ("band140", 2051): (4, True), ("band260", 261): (4, False)}
# every capped comparison: (system, cap)
CAPPED = [(key, 3) for key in NON_TINY] + [(key, 6) for key in CHAINS_HELMS]


def sys_id(key):
    return f"{key[0]}-{key[1]}"


def halve_upper(rp, ci, v):
    """multi_bicg_cases.halve_upper for complex values: the same pattern with every strictly upper entry halved."""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    out = np.array(v, np.complex128)
    out[np.asarray(ci) > rows] *= 0.5
    return out


_SYSTEMS = {}


def system(kind, n):
    """dict(key, n, rp, ci, v, A (scipy), xt, b, mean, R, blocks), as multi_cplx_cases.system; n: nx for "helm"."""
    key = (kind, n)
    if key not in _SYSTEMS:
        Z = cc.system(kind, n)
        v = halve_upper(Z["rp"], Z["ci"], Z["v"])
        A = sp.csr_matrix((v, Z["ci"], Z["rp"]), shape=(Z["n"], Z["n"]))
        _SYSTEMS[key] = {"key": ("cbicg",) + key, "n": Z["n"], "rp": Z["rp"], "ci": Z["ci"], "v": v, "A": A, "xt": Z["xt"],
                         "b": np.ascontiguousarray(A @ Z["xt"], np.complex128), "mean": Z["mean"], "R": Z["R"], "blocks": Z["blocks"]}
    return _SYSTEMS[key]


columns = cc.columns
guesses = cc.guesses
ulp_changes = cc.ulp_changes
aligned_block = cc.aligned_block
bits = cc.bits


def shadow(port, n, seed=SEED):
    """A shadow residual with non-zero imaginary parts (module docstring)."""
    return port.vecrnd(n, seed, 1.0 + 1.0j, 2.0 + 2.0j)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _csum(a):
    return np.cumsum(a)[-1]             # (a numpy scalar: x / 0 is Inf or NaN, as in C)


def _inner(a, b):
    return _csum(np.conj(a) * b)        # clcg_inner: the first argument conjugated


def _norm2(a):
    return float(_csum(a.real * a.real + a.imag * a.imag))


def pcbicgstab(A, inv, b, m0, rb, eps, abs_diff, cap):
    """Complex BiCGStab right-preconditioned in x-space with the reciprocal diagonal inv, one column alone; inv = None: plain,
    clcg.cpp:524-679 itself.
        p = r = b - A m; rho = <rb,r>;  loop: ph = inv p; v = A ph; ak = rho / <rb,v>; s = r - ak v; sh = inv s; t = A sh;
        wk = <t,s> / <t,t>; m += ak ph + wk sh; r = s - wk t; betak = rho' ak / (rho wk); p = r + betak (p - wk v)
    with the 4th-power stop rule at the loop head ((sum |r|^2)^2 / max((sum |m|^2)^2, 1), or sum |r|^2 / n), both "already optimised"
    criteria in the reference's order and the NaN scan of m.  cap = 0: no limit.  Returns dict(x, ret, iters, residual); a column that
    ends with NANV reports the iteration in which the NaN appeared (t after its t++), the batched loops' convention."""
    n = len(b)
    ap = (lambda x: x) if inv is None else (lambda x: inv * x)
    m = np.array(m0, np.complex128)
    r = b - A @ m
    p = r.copy()
    rho = _inner(rb, r)
    mm, r2 = _norm2(m), _norm2(r)
    m4, r4 = max(mm * mm, 1.0), r2 * r2
    if abs_diff and np.sqrt(r4) / n <= eps:
        return dict(x=m, ret=ALREADY, iters=0, residual=np.sqrt(r4) / n)
    if r4 / m4 <= eps:
        return dict(x=m, ret=ALREADY, iters=0, residual=r4 / m4)
    t = 0
    with np.errstate(all="ignore"):
        while True:
            res = np.sqrt(r4) / n if abs_diff else r4 / m4
            if res <= eps:
                return dict(x=m, ret=CONV, iters=t, residual=res)
            if cap > 0 and t + 1 > cap:
                return dict(x=m, ret=MAXIT, iters=t, residual=res)
            t += 1
            ph = ap(p)
            v = A @ ph
            ak = rho / _inner(rb, v)
            s = r - ak * v
            sh = ap(s)
            q = A @ sh
            wk = _inner(q, s) / _inner(q, q)
            m = m + (ak * ph + wk * sh)
            r = s - wk * q
            mm, r2 = _norm2(m), _norm2(r)
            m4, r4 = max(mm * mm, 1.0), r2 * r2
            if np.isnan(m.real + m.imag).any():
                return dict(x=m, ret=NANV, iters=t, residual=res)
            rho1 = _inner(rb, r)
            bk = rho1 * ak / (rho * wk)
            rho = rho1
            p = r + bk * (p - wk * v)


def jacobi_inv(S):
    return 1.0 / S["A"].diagonal()


_RUNS = {}


def restated_column(S, pre, bcol, tag, rb, m0=None, **para):
    """pcbicgstab on one column alone (pre: None or "jacobi"), cached per system, pre, `tag` (the caller's name of the column, the
    guess and the shadow vector) and parameters."""
    key = (S["key"], "restated", pre, tag, tuple(sorted(para.items())))
    if key not in _RUNS:
        _RUNS[key] = pcbicgstab(S["A"], jacobi_inv(S) if pre == "jacobi" else None, np.asarray(bcol, np.complex128),
                                np.zeros(S["n"], np.complex128) if m0 is None else m0, rb, para.get("epsilon", 1e-6),
                                para.get("abs_diff", 0), para.get("max_iterations", 0))
    return _RUNS[key]


def oracle_column(port, S, bcol, tag, rb, m0=None, **para):
    """The oracle's orc_clbicgstab on one column alone with the shadow vector rb, cached like restated_column."""
    from oracle import pyoracle as po
    key = (S["key"], "oracle", tag, tuple(sorted(para.items())))
    if key not in _RUNS:
        _RUNS[key] = port.csolve(BICGSTAB, S["rp"], S["ci"], S["v"], bcol, m0=m0, para=po.default_cpara(**para), rbar0=rb)
    return _RUNS[key]


def response(run, bcol, tag, samples=2):
    """The response of a solve to 1-ulp changes of b: max over the samples of |x(b') - x(b)| / |x(b)|.  run(b, tag) -> dict with x."""
    ref = run(bcol, ("col",) + tuple(tag))
    nx = np.linalg.norm(ref["x"])
    return max(np.linalg.norm(run(ulp_changes(bcol, s), ("pert", s) + tuple(tag))["x"] - ref["x"]) / nx for s in range(samples))


# ---------------------------------------------------------------------------------------------------------------- drivers (GPU)
def cbicg(lib, api, precond, A, M, B, rb=None, seed=None, mem="device", **para):
    """One clcg_hip_lbicgstab_multi solve: (rc, ret[k], iterations[k], residual[k], M afterwards); M, B (n, k) complex128 numpy
    arrays.  rb: the explicit shadow vector of this call; seed: lcg_hip_set_shadow_seed before it."""
    import torch
    k = B.shape[1]
    p = api.clcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    if seed is not None:
        assert lib.lcg_hip_set_shadow_seed(seed) == 0
    if rb is not None:
        rb = np.ascontiguousarray(rb, np.complex128)
        assert lib.lcg_hip_set_shadow_vector(rb.ctypes.data, len(rb)) == 0
    try:
        if mem == "device":
            Md, Bd = torch.from_numpy(np.ascontiguousarray(M).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(B)).cuda()
            rc = lib.clcg_hip_lbicgstab_multi(A.h, k, precond, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
            torch.cuda.synchronize()
            out = Md.cpu().numpy()
        else:
            out, Bh = aligned_block(M), aligned_block(B)
            rc = lib.clcg_hip_lbicgstab_multi(A.h, k, precond, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    finally:
        lib.lcg_hip_set_shadow_vector(None, 0)          # (a call refused before it drew its shadow vector leaves none behind)
    return rc, list(ret), list(its), list(res), out


# ------------------------------------------------------------------------------------------ the staging header and its table
def staging_header():
    from conftest import ROOT
    return os.path.join(ROOT, "include", "lcg_hip_staging.h")


def staged_prototypes():
    """name -> (return type, [argument types]) of every function include/lcg_hip_staging.h declares, comments removed, spelled as
    tests/test_streams_cpu.py spells them ("int", "void *")."""
    src = re.sub(r"/\*.*?\*/", "", open(staging_header()).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^\s*([a-z_ ]+?\*?)\s*(c?lcg_hip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = [a.strip() for a in args.split(",")]
        out[name] = (ret.strip(), [] if args == ["void"] else ["void *" if "*" in a else a.split()[0] for a in args])
    return out


# The lines the staged entries will bring to stream_cases.STREAM_COVERAGE when they move to lcg_hip.h, in that table's format
_STREAMS = "test_gpu_streams_cbicgstab.py"
STAGING_COVERAGE = {
    "clcg_hip_spmm_inner": _STREAMS + "::test_complex_block_products_with_conjugated_sums",
    "clcg_hip_spmm_dot2": _STREAMS + "::test_complex_block_products_with_conjugated_sums",
    "clcg_hip_lbicgstab_multi": _STREAMS + "::test_batched_complex_bicgstab",
}
