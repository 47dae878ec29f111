"""Systems, right-hand sides and drivers shared by the tests of the multi-vector path: tests/test_gpu_multi_solvers.py (the driver),
tests/test_gpu_multi_edges.py, tests/test_gpu_multi_product.py (the band patterns) and tests/test_multi_cases_cpu.py, which shows
with the oracle alone that the cases are what they claim.  Modelled on tests/stop_cases.py; a helper of the tests, not a conftest.

Systems, by the class of rows_per_block (csr_multi.hip: mean row length <= 48 -> R = 64 rows per block, <= 256 -> 16, more -> 4):
  * "spd", n >= 65: stop_cases.system("spd", n), about 5 entries per row: R = 64;
  * "tiny", n = 1, 2, 3: dense, SPD by a dominant diagonal (n = 1: the matrix [2.5]): R = 64, one block, n * k / 2 pieces;
  * "band30" / "band140": band(n, h), every offset 1 .. h filled: mean about 2 h + 1 = 61 (R = 16) and, from n = 2051 on, 271 (R = 4).
Each system carries nnz / n, its class R and its block count ceil(n / R): the product sets no kernel name, so the class asserted
here is the only statement of which instantiation ran.  More than MM_MG = 512 blocks: d.Ad goes through k_mm_fold.

Columns: b = A.xt (|m|^2 ends well above 1), 1e-6 b (|m|^2 stays below 1: clamp1 decides m2), a seeded random vector, a zero
column, and for k = 8 also -b, 3 x another random vector, 0.5 b and 2 b.  k = 2: b and 1e-6 b, so both sides of the clamp are
there for every k.
"""
import ctypes as C

import numpy as np

import exact_ref as X
import stop_cases as sc
from oracle import pyoracle as po

CONV, ALREADY, MAXIT, NANV = 0, 2, -1019, -1017
CG, PCG = 0, 1
KS = (2, 4, 8)
MM_MG = 512                         # multi.hpp
RULES = {"rel": dict(abs_diff=0, epsilon=1e-14), "abs": dict(abs_diff=1, epsilon=1e-10)}


def rows_per_block(mean):
    """csr_multi.hip: rows_per_block."""
    return 64 if mean <= 48.0 else (16 if mean <= 256.0 else 4)


# ---------------------------------------------------------------------------------------------------------------- systems
def band_pattern(n, h, seed=5):
    """CSR (rowptr, col, val) of the dense band: offsets 1 .. h with values from U(-1, -0.2) / h, symmetrised; diagonal = the row's
    absolute sum x (1.1 + 0.5 (1 + sin 0.37 i)): SPD by diagonal dominance."""
    rng = np.random.default_rng(seed + 1000 * h)
    i = np.arange(n, dtype=np.int64)
    rows, cols, vals = [], [], []
    for off in range(1, min(h, n - 1) + 1):
        w = rng.uniform(-1.0, -0.2, n - off) / h
        rows += [i[:n - off], i[off:]]; cols += [i[off:], i[:n - off]]; vals += [w, w]
    row = np.concatenate(rows); col = np.concatenate(cols); val = np.concatenate(vals)
    absum = np.zeros(n); np.add.at(absum, row, np.abs(val))
    row = np.concatenate([row, i]); col = np.concatenate([col, i])
    val = np.concatenate([val, absum * (1.1 + 0.5 * (1.0 + np.sin(0.37 * i)))])
    order = np.lexsort((col, row))
    row, col, val = row[order], col[order].astype(np.int32), val[order]
    rp = np.zeros(n + 1, np.int64); np.add.at(rp, row + 1, 1)
    return np.cumsum(rp).astype(np.int32), col, val


def _tiny(n):
    """Dense n x n, off-diagonal -0.5, diagonal 2.5 + 0.5 i; xt = (2, -1.5, 1): |xt|^2 >= 4 and |A.xt|^2 < 100 (so 1e-6 b meets
    the SECOND "already optimised" criterion under abs_diff = 1, epsilon = 1e-10: 1e-12 |b|^2 / 1 <= 1e-10)."""
    A = np.full((n, n), -0.5); A[np.arange(n), np.arange(n)] = 2.5 + 0.5 * np.arange(n)
    rp = (np.arange(n + 1) * n).astype(np.int32)
    ci = np.tile(np.arange(n), n).astype(np.int32)
    return rp, ci, A.ravel().copy(), np.array([2.0, -1.5, 1.0])[:n]


_SYSTEMS = {}


def system(kind, n):
    """kind: 'spd', 'tiny', 'band30', 'band140'.  dict(key, n, rp, ci, v, xt, b, mean, R, blocks); b = A.xt row by row."""
    key = (kind, n)
    if key not in _SYSTEMS:
        if kind == "spd":
            S = sc.system("spd", n)
            rp, ci, v, xt = S["rp"], S["ci"], S["v"], S["xt"]
        elif kind == "tiny":
            rp, ci, v, xt = _tiny(n)
        else:
            rp, ci, v = band_pattern(n, int(kind[4:]))
            i = np.arange(n, dtype=np.float64)
            xt = np.sin(0.7 * i) + 0.3 * np.cos(0.013 * i)
        mean = float(rp[-1]) / n
        R = rows_per_block(mean)
        _SYSTEMS[key] = {"key": key, "n": n, "rp": rp, "ci": ci, "v": v, "xt": xt, "b": sc._matvec(rp, ci, v, xt), "mean": mean, "R": R,
                         "blocks": (n + R - 1) // R}
    return _SYSTEMS[key]


# what each system is there for: (kind, n) -> (R, folded: more than MM_MG row blocks)
CLASS = {("tiny", 1): (64, False), ("tiny", 2): (64, False), ("tiny", 3): (64, False), ("spd", 65): (64, False), ("spd", 513): (64, False),
         ("spd", 32771): (64, True), ("spd", 65539): (64, True), ("spd", 131075): (64, True),
         ("band30", 1029): (16, False), ("band30", 8197): (16, True), ("band140", 2051): (4, True)}

# (kind, n, k) -> the branch the case is the smallest to reach
EDGE_CASES = {}
for _n in (1, 2, 3):
    for _k in KS:
        EDGE_CASES[("tiny", _n, _k)] = "tiny"
for _n in (65, 513):
    for _k in KS:
        EDGE_CASES[("spd", _n, _k)] = "edge"
for _k in KS:
    EDGE_CASES[("spd", 32771, _k)] = "fold_r64" + ("_stride2" if _k == 8 else "")
EDGE_CASES[("spd", 65539, 4)] = "stride2"
EDGE_CASES[("spd", 131075, 2)] = "stride2"
for _k in KS:
    EDGE_CASES[("band30", 1029, _k)] = "r16_partial_block"
EDGE_CASES[("band30", 8197, 4)] = "fold_r16"
EDGE_CASES[("band140", 2051, 2)] = "fold_r4"
EDGE_CASES[("band140", 2051, 8)] = "fold_r4"
EDGE_CASES[("spd", 131075, 8)] = "work_2p20_stride2"
EDGE_IDS = {c: f"{c[0]}-{c[1]}-k{c[2]}-{why}" for c, why in EDGE_CASES.items()}
STRIDE = 512 * 256                  # pieces one stride of a vector pass covers (grid_for's 512 workgroups of VB = 256 lanes)


# ---------------------------------------------------------------------------------------------------------------- columns
def columns(n, b, k):
    """The k right-hand sides of a batch (module docstring), (n, k) row-major."""
    r = np.random.default_rng(77)
    cols = [b, 1e-6 * b, r.standard_normal(n), np.zeros(n), -b, 3.0 * r.standard_normal(n), 0.5 * b, 2.0 * b]
    if k == 2:
        cols = cols[:2]
    return np.ascontiguousarray(np.stack(cols[:k], axis=1))


def solutions(xt, k):
    """The solution each column of columns() was made from (None: not known)."""
    sols = [xt, 1e-6 * xt, None, np.zeros(len(xt)), -xt, None, 0.5 * xt, 2.0 * xt]
    return sols[:k]


def guesses(S, k):
    """A non-zero block of guesses: column 0 zeros, column 1 a seeded random vector, the rest 0.5 xt."""
    M0 = np.zeros((S["n"], k))
    M0[:, 1] = np.random.default_rng(91).standard_normal(S["n"])
    for j in range(2, k):
        M0[:, j] = 0.5 * S["xt"]
    return M0


# ---------------------------------------------------------------------------------------------------------------- drivers
def multi(lib, api, sid, A, M, B, mem="device", **para):
    """One batched solve: (rc, ret[k], iterations[k], residual[k], M afterwards).  M, B: (n, k) numpy arrays."""
    import torch
    k = B.shape[1]
    p = api.lcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    fn = lib.lcg_hip_lpcg_multi if sid == PCG else lib.lcg_hip_lcg_multi
    if mem == "device":
        Md, Bd = torch.from_numpy(M.copy()).cuda(), torch.from_numpy(B).cuda()
        rc = fn(A.h, k, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        raw = np.zeros(M.size + 2); off = 0 if raw.ctypes.data % 16 == 0 else 1
        out = raw[off:off + M.size].reshape(M.shape); out[:] = M
        rawb = np.zeros(B.size + 2); offb = 0 if rawb.ctypes.data % 16 == 0 else 1
        Bh = rawb[offb:offb + B.size].reshape(B.shape); Bh[:] = B
        rc = fn(A.h, k, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    return rc, list(ret), list(its), list(res), out


_ORACLE = {}


def oracle_column(port, S, sid, bcol, tag, m0=None, **para):
    """The oracle's run of one column alone, from the guess m0 (None: zeros); cached per system, solver, tag and parameters.
    tag names (b, m0): the caller's statement of which column this is."""
    key = (S["key"], sid, tag, tuple(sorted(para.items())))
    if key not in _ORACLE:
        _ORACLE[key] = port.solve(sid, S["rp"], S["ci"], S["v"], bcol, m0=m0, para=po.default_para(**para), jacobi=(sid == PCG))
    return _ORACLE[key]


def host_residual(S, m, b, abs_diff, already_eps=None):
    """The stop rule's residual of the iterate m, from nothing the device summed: g = A.m - b with the product and both dots in
    extended precision (exact_ref), then g.g / max(m.m, 1) or sqrt(g.g) / n.  already_eps: the column was "already optimised" under
    that epsilon -- in abs_diff mode by the first criterion it meets, and the second reports g.g / max(m.m, 1) (lcg.cpp:178-203).
    Returns (residual, g.g, m.m)."""
    y, _, _ = X.hp_product(S["rp"], S["ci"], S["v"], m)
    if isinstance(y, X._DD):
        g = (y.hi - b) + y.lo
    else:
        g = (y - np.asarray(b, np.longdouble)).astype(np.float64)
    g2, _ = X.hp_dot(g, g)
    m2, _ = X.hp_dot(m, m)
    if abs_diff and already_eps is not None and np.sqrt(g2) / S["n"] > already_eps:
        abs_diff = 0
    return (np.sqrt(g2) / S["n"] if abs_diff else g2 / max(m2, 1.0)), g2, m2


def rounding_floor(S, m, b, abs_diff):
    """The residual that rounding alone can leave where A.m - b is exactly zero: every row of g within exact_ref's row bound
    gamma(L + 4) (|A||m| + |b|), through the same formulas.  A guess that IS the solution to rounding (m0 = 0.5 xt for 0.5 b) gives a
    residual below this on either side, each its own: the oracle's product reproduces b's order and leaves 0.0, a fused multiply-add
    leaves a few 1e-18."""
    absax = X._row_sum(np.abs(S["v"]) * np.abs(m)[S["ci"]], S["rp"])
    g = X.gamma(X.lengths(S["rp"]) + 4) * (absax + np.abs(b))
    g2 = float(g @ g)
    return np.sqrt(g2) / S["n"] if abs_diff else g2 / max(float(m @ m), 1.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------ both "already optimised" criteria
ALREADY_EPS = 1e-6


def already_batch(S):
    """(M0, B) of four columns under abs_diff = 1, epsilon = 1e-6 on the spd 65 system:
    0: m0 = xt + delta with |A.delta| = 1e-3 -- sqrt(g.g) / n = 1.5e-5 fails the first criterion, g.g / m.m = 2.7e-8 meets the second;
    1: m0 = xt, exact to rounding -- the first criterion;  2: the zero guess, which runs;  3: b = 0 with a guess of -0.0."""
    n, xt, b = S["n"], S["xt"], S["b"]
    delta = np.cos(1.3 * np.arange(n))
    delta *= 1e-3 / np.linalg.norm(sc._matvec(S["rp"], S["ci"], S["v"], delta))
    M0 = np.stack([xt + delta, xt, np.zeros(n), np.full(n, -0.0)], axis=1)
    B = np.stack([b, b, b, np.zeros(n)], axis=1)
    return np.ascontiguousarray(M0), np.ascontiguousarray(B)
