"""Systems, right-hand sides, drivers and a numpy restatement shared by the tests of the complex multi-vector path:
tests/test_gpu_multi_cplx_solvers.py, tests/test_gpu_multi_cplx_product.py and tests/test_multi_cplx_cases_cpu.py, which shows with
the oracle alone that the cases are what they claim.  Modelled on tests/multi_cases.py; a helper of the tests, not a conftest.

Systems, all complex-symmetric and non-Hermitian, by the class of rows_per_block (csr_multi.hip, the frame both products share: mean row length <= 48 -> R = 64
rows per block, <= 256 -> 16, more -> 4):
  * "helm", nx: the nx x nx five-point Laplacian plus a diagonal 0.05 + 0.3i (0.2 + u), u uniform from a fixed seed; b = A.xt.
    helm 40 is the issue's helm40 (n = 1600); helm 182 (n = 33124) has 518 row blocks of 64 (the folded d.Ad) and rows beyond
    tree_leaves' cap of 16384 (a second and third stride of a vector pass); helm 363 (n = 131769) has n k >= 2^20 at k = 8;
  * "chain", n: the 1-D chain tridiag(-1, 2, -1) plus the same kind of diagonal, for the size edges n = 1, 2, 3, 65, 513
    (n = 1: the matrix [2.05 + 0.3i (0.2 + u)]);
  * "band30" / "band140", n: multi_cases.band_pattern (real SPD, every offset 1 .. h filled) plus i 0.3 (0.2 + u) d_ii on the
    diagonal: mean about 61 (R = 16) and, from n = 2051 on, 271 (R = 4); "band260", 261 is the dense 261 x 261 matrix of that family
    (R = 4, 66 row blocks, the last of one row);
  * "case1kc": tests/golden/case_1K_cA, 1.2 entries per row; the oracle needs 310-514 iterations: capped runs only.
Each system carries its mean row length, its class R and its block count ceil(n / R); more than MM_MG = 512 blocks: d.Ad goes
through k_mm_fold.

Columns: b = A.xt (|m|^2 ends well above 1), 1e-2 b (|m|^2 stays below 1: the clamp decides; 1e-6 b would be "already optimised" under
BiCG-sym's 4th-power rule), a seeded random complex vector, a
zero column, and for k = 8 also -b, 3 x another random vector, 0.5 b and 2 b.  k = 2: b and 1e-2 b."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

import multi_cases as mc
from oracle import pyoracle as po

CONV, ALREADY, MAXIT, NANV = 0, 2, -1019, -1019     # (CLCG_NAN_VALUE and the real enum's cap code share -1019: SURVEY quirk 5)
NOPRE, BADEPS, BADMAXIT, E_ARG = -1018, -1021, -1022, -2003
BICG_SYM, PCG = "bicg_sym", "pcg"
SIDS = (BICG_SYM, PCG)
KS = (2, 4, 8)
MM_MG = 512                         # multi.hpp
CMM_W = 1536                        # multi_cplx.hpp: entries per LDS window of k_cspmm
SMALL = 1e-2                        # the scale of the column whose |m|^2 stays below 1
TREE_CAP = 32 * MM_MG               # multi.hpp: tree_leaves' cap for complex blocks -- rows beyond it are a thread's second piece

rows_per_block = mc.rows_per_block  # the complex product runs under csr_multi.hip's frame: the same classes


# ---------------------------------------------------------------------------------------------------------------- systems
def _shift(n, seed):
    return 0.05 + 0.3j * (0.2 + np.random.default_rng(seed).uniform(size=n))


def _helm(nx):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx))
    L = (sp.kron(sp.identity(nx), T) + sp.kron(T, sp.identity(nx))).tocsr().astype(np.complex128)
    A = (L + sp.diags(_shift(nx * nx, 4040))).tocsr()
    A.sort_indices()
    return A


def _chain(n):
    if n == 1:
        return sp.csr_matrix(np.array([[2.0 + _shift(1, 11)[0]]]))
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n)).tocsr().astype(np.complex128)
    A = (T + sp.diags(_shift(n, 11 + n))).tocsr()
    A.sort_indices()
    return A


def _band(n, h):
    rp, ci, v = mc.band_pattern(n, h)
    v = v.astype(np.complex128)
    rows = np.repeat(np.arange(n), np.diff(rp))
    dg = np.flatnonzero(rows == ci)
    assert len(dg) == n
    v[dg] = v[dg] * (1.0 + 0.3j * (0.2 + np.random.default_rng(77 + h).uniform(size=n)))
    return sp.csr_matrix((v, ci, rp), shape=(n, n))


_SYSTEMS = {}


def system(kind, n=0):
    """dict(key, n, rp, ci, v, A (scipy), xt, b, mean, R, blocks); n: nx for "helm"."""
    key = (kind, n)
    if key not in _SYSTEMS:
        if kind == "case1kc":
            from conftest import GOLDEN
            from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system, read_solution
            nn, row, col, val, b = read_coo_system(os.path.join(GOLDEN, "case_1K_cA"), True)
            rp, ci, v = coo_to_csr_host(nn, row, col, val)
            A = sp.csr_matrix((v, ci, rp), shape=(nn, nn))
            xt = read_solution(os.path.join(GOLDEN, "case_1K_cB"), True)
        else:
            A = _helm(n) if kind == "helm" else (_chain(n) if kind == "chain" else _band(n, int(kind[4:])))
            nn = A.shape[0]
            rng = np.random.default_rng(40 + nn)
            xt = rng.standard_normal(nn) + 1j * rng.standard_normal(nn)
            b = A @ xt
        mean = float(A.indptr[-1]) / nn
        R = rows_per_block(mean)
        _SYSTEMS[key] = {"key": key, "n": nn, "rp": A.indptr.astype(np.int32), "ci": A.indices.astype(np.int32),
                         "v": np.ascontiguousarray(A.data, np.complex128), "A": A, "xt": xt, "b": np.ascontiguousarray(b, np.complex128),
                         "mean": mean, "R": R, "blocks": (nn + R - 1) // R}
    return _SYSTEMS[key]


HELM40 = ("helm", 40)
# what each system is there for: key -> (R, folded: more than MM_MG row blocks, partial last block)
CLASS = {("chain", 1): (64, False), ("chain", 2): (64, False), ("chain", 3): (64, False), ("chain", 65): (64, False),
         ("chain", 513): (64, False), ("helm", 40): (64, False), ("helm", 182): (64, True), ("helm", 363): (64, True),
         ("band30", 1029): (16, False), ("band30", 8197): (16, True), ("band140", 2051): (4, True), ("band260", 261): (4, False),
         ("case1kc", 0): (64, False)}

# (kind, n, k) -> the branch the case is the smallest to reach
EDGE_CASES = {}
for _n in (1, 2, 3, 65, 513):
    for _k in KS:
        EDGE_CASES[("chain", _n, _k)] = "size_edge"
for _k in KS:
    EDGE_CASES[("helm", 182, _k)] = "fold_r64_stride3"
    EDGE_CASES[("band30", 1029, _k)] = "r16_partial_block"
EDGE_CASES[("band30", 8197, 4)] = "fold_r16"
EDGE_CASES[("band260", 261, 4)] = "r4_partial_block"
EDGE_CASES[("band140", 2051, 2)] = "fold_r4"
EDGE_CASES[("band140", 2051, 8)] = "fold_r4"
EDGE_CASES[("helm", 363, 8)] = "work_2p20"
EDGE_CASES[("case1kc", 0, 4)] = "golden_1K"
EDGE_IDS = {c: f"{c[0]}-{c[1]}-k{c[2]}-{why}" for c, why in EDGE_CASES.items()}


# ---------------------------------------------------------------------------------------------------------------- columns
def _crand(r, n):
    return r.standard_normal(n) + 1j * r.standard_normal(n)


def columns(n, b, k):
    """The k right-hand sides of a batch (module docstring), (n, k) row-major complex128."""
    r = np.random.default_rng(77)
    cols = [b, SMALL * b, _crand(r, n), np.zeros(n, np.complex128), -b, 3.0 * _crand(r, n), 0.5 * b, 2.0 * b]
    if k == 2:
        cols = cols[:2]
    return np.ascontiguousarray(np.stack(cols[:k], axis=1))


def guesses(S, k):
    """A non-zero block of guesses: column 0 zeros, column 1 a seeded random vector, the rest 0.5 xt."""
    M0 = np.zeros((S["n"], k), np.complex128)
    M0[:, 1] = _crand(np.random.default_rng(91), S["n"])
    for j in range(2, k):
        M0[:, j] = 0.5 * S["xt"]
    return M0


def ulp_changes(b, s):
    """b with every element moved by about one ulp, seeded by s (the oracle's own response to rounding is measured with these)."""
    r = np.random.default_rng(1000 + s)
    n = len(b)
    return (b.real * (1.0 + 1e-16 * r.standard_normal(n))) + 1j * (b.imag * (1.0 + 1e-16 * r.standard_normal(n)))


# ---------------------------------------------------------------------------------------------------------------- drivers
def aligned_block(a):
    """A copy of the complex block a whose base is 16-byte aligned."""
    raw = np.zeros(2 * a.size + 2)
    off = 0 if raw.ctypes.data % 16 == 0 else 1
    out = raw[off:off + 2 * a.size].view(np.complex128).reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 16 == 0
    return out


def cmulti(lib, api, sid, A, M, B, mem="device", **para):
    """One batched solve: (rc, ret[k], iterations[k], residual[k], M afterwards).  M, B: (n, k) complex128 numpy arrays."""
    import torch
    k = B.shape[1]
    p = api.clcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    fn = lib.clcg_hip_lpcg_multi if sid == PCG else lib.clcg_hip_lbicg_sym_multi
    if mem == "device":
        Md, Bd = torch.from_numpy(np.ascontiguousarray(M).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(B)).cuda()
        rc = fn(A.h, k, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        out, Bh = aligned_block(M), aligned_block(B)
        rc = fn(A.h, k, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    return rc, list(ret), list(its), list(res), out


_ORACLE = {}


def oracle_column(port, S, sid, bcol, tag, m0=None, **para):
    """The oracle's run of one column alone, from the guess m0 (None: zeros); cached per system, solver, tag and parameters.
    tag names (b, m0): the caller's statement of which column this is."""
    key = (S["key"], sid, tag, tuple(sorted(para.items())))
    if key not in _ORACLE:
        cp = po.default_cpara(**para)
        if sid == PCG:
            _ORACLE[key] = port.csolve_pcg(S["rp"], S["ci"], S["v"], bcol, m0=m0, para=cp)
        else:
            _ORACLE[key] = port.csolve(po.CLCG_BICG_SYM, S["rp"], S["ci"], S["v"], bcol, m0=m0, para=cp)
    return _ORACLE[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- restatement
def restate(sid, S, b, m0=None, epsilon=1e-6, abs_diff=0, max_iterations=0):
    """Both recurrences in numpy, as oracle/clcg_oracle.c states them (orc_clbicg_symmetric :264-300, orc_clpcg :172-211): unconjugated
    products, BiCG-sym's 4th-power stop rule with both "already optimised" criteria and its NaN scan, PCG's real-loop rule in which
    |m|^2 takes no part under abs_diff and no NaN scan.  Returns dict(x, ret, iters, residual, trace, already) with trace = the
    (sum |m|^2, sum |r|^2) the stop rule saw at the head of each iteration and already = which criterion (1, 2) said "already
    optimised" (0: none)."""
    A, n = S["A"], S["n"]
    m = np.zeros(n, np.complex128) if m0 is None else np.array(m0, np.complex128)
    b = np.asarray(b, np.complex128)
    inv = 1.0 / A.diagonal() if sid == PCG else None
    r = b - A @ m
    d = inv * r if sid == PCG else r.copy()
    rho = np.sum(r * d)
    mm, r2 = float(np.sum(np.abs(m) ** 2)), float(np.sum(np.abs(r) ** 2))

    def resid():
        if sid == PCG:
            return np.sqrt(r2) / n if abs_diff else r2 / max(mm, 1.0)
        m4, r4 = max(mm * mm, 1.0), r2 * r2
        return np.sqrt(r4) / n if abs_diff else r4 / m4

    out = dict(trace=[(mm, r2)], already=0)
    res = resid()
    if res <= epsilon:
        out["already"] = 1
    elif sid == BICG_SYM and abs_diff and (r2 * r2) / max(mm * mm, 1.0) <= epsilon:
        res = (r2 * r2) / max(mm * mm, 1.0)
        out["already"] = 2
    if out["already"]:
        out.update(x=m, ret=ALREADY, iters=0, residual=res)
        return out
    t = 0
    with np.errstate(all="ignore"):
        while True:
            res = resid()
            if res <= epsilon:
                ret = CONV; break
            if max_iterations > 0 and t + 1 > max_iterations:
                ret = MAXIT; break
            t += 1
            Ad = A @ d
            ak = rho / np.sum(d * Ad)
            m = m + ak * d
            r = r - ak * Ad
            mm, r2 = float(np.sum(np.abs(m) ** 2)), float(np.sum(np.abs(r) ** 2))
            out["trace"].append((mm, r2))
            if sid == BICG_SYM and np.isnan(m.real + m.imag).any():
                ret = NANV; break
            z = inv * r if sid == PCG else r
            new = np.sum(r * z)
            bk = new / rho
            rho = new
            d = z + bk * d
    out.update(x=m, ret=ret, iters=t, residual=res)
    return out


# ------------------------------------------------------------------------------------ both "already optimised" criteria
ALREADY_EPS = 1e-6


def already_batch(S):
    """(M0, B) of four columns under abs_diff = 1, epsilon = 1e-6 on helm40 (n = 1600, |xt|^2 about 3200):
    0: m0 = xt + delta with |A.delta| = 0.1 -- sum |r|^2 / n = 6.25e-6 fails BiCG-sym's first criterion and (|r|^2 / |m|^2)^2 about
       1e-11 meets its second; PCG, where |m|^2 takes no part under abs_diff, sees sqrt(|r|^2) / n = 6.25e-5 and runs;
    1: m0 = xt, exact to rounding -- the first criterion of both;  2: the zero guess, which runs;  3: b = 0 with a guess of -0.0."""
    n, xt, b = S["n"], S["xt"], S["b"]
    delta = np.cos(1.3 * np.arange(n)) * (1.0 + 0.5j)
    delta *= 0.1 / np.linalg.norm(S["A"] @ delta)
    M0 = np.stack([xt + delta, xt, np.zeros(n, np.complex128), np.full(n, -0.0 - 0.0j)], axis=1)
    B = np.stack([b, b, b, np.zeros(n, np.complex128)], axis=1)
    return np.ascontiguousarray(M0), np.ascontiguousarray(B)
