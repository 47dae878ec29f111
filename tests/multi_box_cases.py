"""Systems, bounds, right-hand sides, drivers and the per-column oracle of the batched box-constrained solvers
(lcg_hip_solver_constrained_multi, lcg_hip_dense_solver_constrained_multi): shared by tests/test_gpu_multi_box.py and
tests/test_multi_box_cases_cpu.py, which shows with the oracle alone that the cases are what they claim.  A helper of the tests, not a
conftest.

The case table (fixed): every system runs under epsilon = 1e-10, abs_diff = 1, default step / sigma / beta / maxi_m with the columns
of multi_cases.columns (b, 1e-6 b, random, zero, -b, 3 x random, 0.5 b, 2 b):
  * case_10K_A between -5 and 8, cap 40: bounds active in some columns, inactive in the 1e-6 b column; PG 41 products in every running
    column, SPG a different count in every column;
  * multi_cases' tiny 1, 2, 3 between -0.5 and 0.8, cap 2 (one block, n k / 2 pieces; from iteration 3 / 4 on the reference breaks down:
    BREAKDOWN below);
  * spd 65 and 513 between -0.5 and 0.8, cap 12 (odd sizes, one and three workgroups' worth);
  * spd 131075 between -0.5 and 0.8, cap 6 (k = 8: n k >= 2^20 doubles, the second stride of a pass).
On all of them the oracle's (ret, iterations, n_ax) does not move under four seeded 1-ulp perturbations of b (the CPU test).
"""
import ctypes as C
import os

import numpy as np

import multi_cases as mc
from oracle import pyoracle as po

CONV, ALREADY, MAXIT, NANV = 0, 2, -1019, -1017
E_ARG = -2003
PG, SPG = 5, 6
SOLVERS = (PG, SPG)
KS = (2, 4, 8)
RULE = dict(epsilon=1e-10, abs_diff=1)
MAXIM_BOUND = 64                    # include/lcg_hip_staging_box_multi.h
SEEDS = 4
FACTOR, FLOOR = 50.0, 1e-9          # the band of tests/test_gpu_multi_solvers.py

# (kind, n) -> (low, hig, cap)
TABLE = {("case10k", 10000): (-5.0, 8.0, 40),
         ("tiny", 1): (-0.5, 0.8, 2), ("tiny", 2): (-0.5, 0.8, 2), ("tiny", 3): (-0.5, 0.8, 2),
         ("spd", 65): (-0.5, 0.8, 12), ("spd", 513): (-0.5, 0.8, 12),
         ("spd", 131075): (-0.5, 0.8, 6)}
# (system, low, hig): column b breaks down -- its iterate stops moving, s.y = 0 -- at an iteration that no 1-ulp change of b moves.
# spd 65 between -0.5 and 0.8 breaks down too (the oracle: first NaN iterate at cap 46 for PG, 49 for SPG) but WHEN its iterate
# becomes stationary to the last bit moves with 1-ulp changes of b (44 .. 57 over four seeds): it is replaced here by the same system
# in a box that the whole solution lies outside of, and kept as the case whose count is not pinned (UNPINNED_BREAKDOWN).
BREAKDOWN = [(("tiny", 1), -0.5, 0.8), (("tiny", 2), -0.5, 0.8), (("tiny", 3), -0.5, 0.8), (("spd", 65), -3.0, -2.0)]
UNPINNED_BREAKDOWN = (("spd", 65), -0.5, 0.8)
BREAKDOWN_IDS = [f"{c[0][0]}-{c[0][1]}" for c in BREAKDOWN]
IDS = {c: f"{c[0]}-{c[1]}" for c in TABLE}

_SYSTEMS = {}


def case10k():
    """case_10K_A/B as conftest's fixture reads them: (n, rp, ci, v, b)."""
    from conftest import GOLDEN
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    n, row, col, val, b = read_coo_system(os.path.join(GOLDEN, "case_10K_A"))
    rp, ci, v = coo_to_csr_host(n, row, col, val)
    return n, rp, ci, v, b


def system(kind, n=None):
    """dict(key, n, rp, ci, v, b): case_10K_A, or multi_cases' system."""
    if kind == "case10k":
        if "case10k" not in _SYSTEMS:
            nn, rp, ci, v, b = case10k()
            _SYSTEMS["case10k"] = {"key": ("case10k", nn), "n": nn, "rp": rp, "ci": ci, "v": v, "b": b}
        return _SYSTEMS["case10k"]
    return mc.system(kind, n)


def bounds(S, lo=None, hi=None):
    t = TABLE.get(S["key"], (-0.5, 0.8, 0))
    return np.full(S["n"], t[0] if lo is None else lo), np.full(S["n"], t[1] if hi is None else hi)


def columns(S, k):
    return mc.columns(S["n"], S["b"], k)


def perturbed(b, seed):
    """b with seeded changes of at most an ulp (conftest.check_converged_run's perturbation)."""
    return b * (1.0 + 1e-16 * np.random.default_rng(1000 + seed).standard_normal(len(b)))


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


bits = mc.bits

# ---------------------------------------------------------------------------------------------------------------- the oracle
_ORACLE = {}


def oracle_column(port, S, sid, bcol, low, hig, m0=None, **para):
    """The oracle's run of one column alone (port.solve_box) from the guess m0 (None: zeros); cached on the column's bytes.  Nobody
    writes into a cached result."""
    key = (S["key"], sid, bcol.tobytes(), float(low[0]), float(hig[0]), None if m0 is None else m0.tobytes(), tuple(sorted(para.items())))
    if key not in _ORACLE:
        r = port.solve_box(sid, S["rp"], S["ci"], S["v"], bcol, low, hig, m0=m0, para=po.default_para(**para))
        r["x"].setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


def response(port, S, sid, bcol, low, hig, m0=None, **para):
    """(the largest relative change of the oracle's iterate, the number of runs whose (ret, iterations, n_ax) changed) over SEEDS
    seeded 1-ulp perturbations of the column."""
    ref = oracle_column(port, S, sid, bcol, low, hig, m0=m0, **para)
    worst, flips = 0.0, 0
    for seed in range(SEEDS):
        r = oracle_column(port, S, sid, perturbed(bcol, seed), low, hig, m0=m0, **para)
        flips += (r["ret"], r["iters"], r["n_ax"]) != (ref["ret"], ref["iters"], ref["n_ax"])
        if np.isfinite(ref["x"]).all() and np.linalg.norm(ref["x"]) > 0.0:
            worst = max(worst, rel(r["x"], ref["x"]))
    return worst, flips


def band(port, S, sid, bcol, low, hig, m0=None, **para):
    """max(1e-9, 50 x the oracle's own response to 1-ulp changes of b at that cap)."""
    return max(FLOOR, FACTOR * response(port, S, sid, bcol, low, hig, m0=m0, **para)[0])


def first_nan_cap(port, S, sid, bcol, low, hig, limit=200, m0=None, **para):
    """The smallest cap at which the oracle's iterate holds a NaN (None: none up to `limit`)."""
    for cap in range(1, limit + 1):
        r = oracle_column(port, S, sid, bcol, low, hig, m0=m0, max_iterations=cap, **para)
        if r["ret"] != MAXIT:
            return None
        if np.isnan(r["x"]).any():
            return cap
    return None


# ---------------------------------------------------------------------------------------------------------------- drivers
def aligned(a):
    """A 16-byte aligned copy of a float64 array."""
    raw = np.zeros(a.size + 2)
    off = 0 if raw.ctypes.data % 16 == 0 else 1
    out = raw[off:off + a.size].reshape(a.shape)
    out[:] = a
    return out


def solve(lib, api, sid, A, M, B, low, hig, mem="device", normal=None, want_products=True, **para):
    """One batched solve: (rc, ret[k], iterations[k], products[k], residual[k], M afterwards).  A: a CsrMatrix, or with normal = 0 / 1
    a dense handle.  M, B: (n, k) numpy arrays; low, hig: n."""
    import torch
    k = B.shape[1]
    p = api.lcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); prods = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    if normal is None:
        fn, lead = lib.lcg_hip_solver_constrained_multi, (A.h, k, sid)
    else:
        fn, lead = lib.lcg_hip_dense_solver_constrained_multi, (A.h, k, normal, sid)
    pp = prods if want_products else None
    if mem == "device":
        Md, Bd = torch.from_numpy(np.ascontiguousarray(M).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(B)).cuda()
        ld, hd = torch.from_numpy(low).cuda(), torch.from_numpy(hig).cuda()
        rc = fn(*lead, Md.data_ptr(), Bd.data_ptr(), ld.data_ptr(), hd.data_ptr(), C.byref(p), ret, its, pp, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        out, Bh = aligned(M), aligned(B)
        lo, hi = np.ascontiguousarray(low), np.ascontiguousarray(hig)
        rc = fn(*lead, out.ctypes.data, Bh.ctypes.data, lo.ctypes.data, hi.ctypes.data, C.byref(p), ret, its, pp, res, 0)
    return rc, list(ret), list(its), list(prods), list(res), out


# ------------------------------------------------------------------------------------------ the staging header and its table
ENTRIES = ["lcg_hip_dense_solver_constrained_multi", "lcg_hip_solver_constrained_multi"]


def staging_header():
    from conftest import ROOT
    return os.path.join(ROOT, "include", "lcg_hip_staging_box_multi.h")


# The lines the staged entries will bring to stream_cases.STREAM_COVERAGE when they move to lcg_hip.h, in that table's format
_STREAMS = "test_gpu_multi_box.py"
STAGING_COVERAGE = {
    "lcg_hip_solver_constrained_multi": _STREAMS + "::test_callers_stream",
    "lcg_hip_dense_solver_constrained_multi": _STREAMS + "::test_callers_stream",
}
