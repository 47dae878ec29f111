"""Systems, a numpy restatement and the driver shared by the tests of the batched BiCGStab: tests/test_gpu_multi_bicgstab.py and
tests/test_multi_bicg_cases_cpu.py, which shows with the oracle alone that the cases are what they claim.  Modelled on
tests/multi_cases.py, whose columns, rules, residuals and drivers' conventions it reuses; a helper of the tests, not a conftest.

Systems (non-symmetric, diagonally dominant), by what they make the kernels do (csr_multi.hip: rows_per_block; multi.hpp: MM_MG):
  * "nonsym", n = 65, 513, 32771, 131075: stop_cases.system("nonsym", n), 5 entries per row, R = 64: one block; a few blocks; 513 row
    blocks (the fold runs; at k = 8 a second stride of the vector passes); n k >= 2^20 at k = 8 (the other publish mask and in-flight depth);
  * "band30" (n = 1029, 8197), "band140" (n = 2051): multi_cases.band_pattern with its strictly upper entries halved: R = 16 with a
    partial last block, R = 16 folded, R = 4 folded;
  * "tiny", n = 1, 2, 3: multi_cases._tiny with its strictly upper entries halved;
  * "convdiff": ilu0_checker.convdiff(40, 2.0), the system of the preconditioned runs (b = A.x*, x* uniform in [1, 2]).

pbicgstab() restates the x-space loop of solvers_multi_bicg.hip (plain: lcg.cpp:629-794 itself) in numpy, written new here as
ilu0_checker.lbicgstab is.  Its dots are added in index order (a cumulative sum), as the oracle's are.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

import ilu0_checker as K
import multi_cases as mc
import stop_cases as sc

CONV, ALREADY, MAXIT, NANV, NOPRE, BADEPS, BADIT, E_ARG = 0, 2, -1019, -1017, -1018, -1021, -1022, -2003
BICGSTAB = 3                        # the oracle's solver id (LCG_BICGSTAB)
M_NONE, M_JACOBI, M_IC0, M_ILU0 = -1, 0, 1, 2
KS = mc.KS
RULES = mc.RULES
CAP = 8

NONSYM = [("nonsym", 65), ("nonsym", 513), ("nonsym", 32771), ("nonsym", 131075)]
BANDS = [("band30", 1029), ("band30", 8197), ("band140", 2051)]
TINY = [("tiny", 1), ("tiny", 2), ("tiny", 3)]
CONVDIFF = ("convdiff", 1600)
NON_TINY = NONSYM + BANDS + [CONVDIFF]
# (kind, n) -> (R, folded: more than MM_MG row blocks)
CLASS = {("nonsym", 65): (64, False), ("nonsym", 513): (64, False), ("nonsym", 32771): (64, True), ("nonsym", 131075): (64, True),
         ("band30", 1029): (16, False), ("band30", 8197): (16, True), ("band140", 2051): (4, True), ("convdiff", 1600): (64, False),
         ("tiny", 1): (64, False), ("tiny", 2): (64, False), ("tiny", 3): (64, False)}


def sys_id(key):
    return f"{key[0]}-{key[1]}"


def halve_upper(rp, ci, v):
    """The same pattern with every strictly upper entry halved: non-symmetric, and where the matrix was diagonally dominant, still so."""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    out = np.array(v, np.float64)
    out[np.asarray(ci) > rows] *= 0.5
    return out


_SYSTEMS = {}


def system(kind, n):
    """dict(key, n, rp, ci, v, xt, b, mean, R, blocks), as multi_cases.system; b = A.xt row by row."""
    key = (kind, n)
    if key not in _SYSTEMS:
        if kind == "nonsym":
            S = sc.system("nonsym", n)
            rp, ci, v, xt = S["rp"], S["ci"], S["v"], S["xt"]
        elif kind == "tiny":
            rp, ci, v, xt = mc._tiny(n)
            v = halve_upper(rp, ci, v)
        elif kind == "convdiff":
            assert n == 1600
            rp, ci, v = K.convdiff(40, 2.0)
            xt = np.random.default_rng(3).uniform(1.0, 2.0, n)
        else:
            rp, ci, v = mc.band_pattern(n, int(kind[4:]))
            v = halve_upper(rp, ci, v)
            i = np.arange(n, dtype=np.float64)
            xt = np.sin(0.7 * i) + 0.3 * np.cos(0.013 * i)
        mean = float(rp[-1]) / n
        R = mc.rows_per_block(mean)
        _SYSTEMS[key] = {"key": ("bicg",) + key, "n": n, "rp": rp, "ci": ci, "v": v, "xt": xt, "b": sc._matvec(rp, ci, v, xt), "mean": mean,
                         "R": R, "blocks": (n + R - 1) // R}
    return _SYSTEMS[key]


def sparse(S):
    return sp.csr_matrix((S["v"], S["ci"], S["rp"]), shape=(S["n"], S["n"]))


columns = mc.columns
guesses = mc.guesses
host_residual = mc.host_residual
rounding_floor = mc.rounding_floor
bits = mc.bits


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _dot(a, b):
    return np.cumsum(a * b)[-1]         # (a numpy scalar: x / 0 is Inf or NaN, as in C)


def pbicgstab(As, apply, b, m0, eps, abs_diff, cap):
    """BiCGStab right-preconditioned in x-space, one column alone; apply = None: plain, lcg.cpp:629-794 itself.
        r0 = p = r = b - A m;   loop: ph = M^-1 p; v = A ph; ak = rho / v.r0; s = r - ak v; sh = M^-1 s; t = A sh; wk = t.s / t.t;
        m += ak ph + wk sh; r = s - wk t; betak = (ak / wk) rho' / rho; p = r + betak (p - wk v)
    with the reference's stop rule at the loop head (r.r / max(m.m, 1) or sqrt(r.r) / n), both "already optimised" criteria in its
    order and its NaN scan of m.  cap = 0: no limit.  Returns dict(x, ret, iters, residual); a column that ends with NANV reports
    the iteration in which the NaN appeared (t after its t++), the batched loops' convention -- one more than the oracle's `iters`."""
    n = len(b)
    ap = (lambda x: x) if apply is None else apply
    m = np.array(m0, np.float64)
    r = b - As @ m
    r0 = r.copy(); p = r.copy()
    rho = _dot(r, r0)
    m2 = max(_dot(m, m), 1.0)
    r2 = _dot(r, r)
    if abs_diff and np.sqrt(r2) / n <= eps:
        return dict(x=m, ret=ALREADY, iters=0, residual=np.sqrt(r2) / n)
    if r2 / m2 <= eps:
        return dict(x=m, ret=ALREADY, iters=0, residual=r2 / m2)
    t = 0
    with np.errstate(all="ignore"):
        while True:
            res = np.sqrt(r2) / n if abs_diff else r2 / m2
            if res <= eps:
                return dict(x=m, ret=CONV, iters=t, residual=res)
            if cap > 0 and t + 1 > cap:
                return dict(x=m, ret=MAXIT, iters=t, residual=res)
            t += 1
            ph = ap(p)
            v = As @ ph
            ak = rho / _dot(v, r0)
            s = r - ak * v
            sh = ap(s)
            q = As @ sh
            wk = _dot(q, s) / _dot(q, q)
            m = m + (ak * ph + wk * sh)
            m2 = max(_dot(m, m), 1.0)
            if np.isnan(m).any():
                return dict(x=m, ret=NANV, iters=t, residual=res)
            r = s - wk * q
            r2 = _dot(r, r)
            rho1 = _dot(r, r0)
            bk = (ak / wk) * rho1 / rho
            rho = rho1
            p = r + bk * (p - wk * v)


def jacobi_apply(S):
    d = sparse(S).diagonal()
    return lambda x: x / d


_RUNS = {}


def restated_column(S, apply_key, apply, bcol, tag, m0=None, **para):
    """pbicgstab on one column alone, cached per system, apply (named by apply_key), `tag` (the caller's name of the column) and
    parameters."""
    key = (S["key"], apply_key, tag, tuple(sorted(para.items())))
    if key not in _RUNS:
        _RUNS[key] = pbicgstab(sparse(S), apply, np.asarray(bcol, float), np.zeros(S["n"]) if m0 is None else m0, para["epsilon"],
                               para["abs_diff"], para.get("max_iterations", 0))
    return _RUNS[key]


def oracle_column(port, S, bcol, tag, m0=None, **para):
    """The oracle's lbicgstab on one column alone (multi_cases.oracle_column, cached there)."""
    return mc.oracle_column(port, S, BICGSTAB, bcol, tag, m0=m0, **para)


def perturbed(bcol, s):
    """b with every entry moved by about 1 ulp (conftest.check_converged_run's perturbation)."""
    return bcol * (1.0 + 1e-16 * np.random.default_rng(1000 + s).standard_normal(len(bcol)))


def response(run, bcol, tag, samples=2):
    """The response of a solve to 1-ulp changes of b: max over the samples of |x(b') - x(b)| / |x(b)|.  run(b, tag) -> dict with x."""
    ref = run(bcol, ("col",) + tuple(tag))
    nx = np.linalg.norm(ref["x"])
    return max(np.linalg.norm(run(perturbed(bcol, s), ("pert", s) + tuple(tag))["x"] - ref["x"]) / nx for s in range(samples))


# ---------------------------------------------------------------------------------------------------------------- driver (GPU)
def bicg(lib, api, precond, A, M, B, mem="device", **para):
    """One lcg_hip_lbicgstab_multi solve: (rc, ret[k], iterations[k], residual[k], M afterwards); M, B (n, k) numpy arrays."""
    import torch
    k = B.shape[1]
    p = api.lcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    if mem == "device":
        Md, Bd = torch.from_numpy(M.copy()).cuda(), torch.from_numpy(np.ascontiguousarray(B)).cuda()
        rc = lib.lcg_hip_lbicgstab_multi(A.h, k, precond, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        raw = np.zeros(M.size + 2); off = 0 if raw.ctypes.data % 16 == 0 else 1
        out = raw[off:off + M.size].reshape(M.shape); out[:] = M
        rawb = np.zeros(B.size + 2); offb = 0 if rawb.ctypes.data % 16 == 0 else 1
        Bh = rawb[offb:offb + B.size].reshape(B.shape); Bh[:] = B
        rc = lib.lcg_hip_lbicgstab_multi(A.h, k, precond, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    return rc, list(ret), list(its), list(res), out
