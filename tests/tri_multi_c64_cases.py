"""Systems, the fp32 sweep restated, drivers and the checker's runs shared by the tests of the batched complex64 IC(0) applies and of
batched complex64 PCG with that factor: tests/test_gpu_tri_multi_c64.py, tests/test_gpu_multi_c64_pcg_m.py and
tests/test_tri_multi_c64_cases_cpu.py, which shows with the checkers alone that the cases are what they claim.  A helper of the
tests, not a conftest.

Systems: the complex64 twins of tests/tri_multi_cases.py's IC(0) systems -- the same patterns ("laplace64", "chain<n>", "layered" with
its 1500-row level, "arrow700", "spd<n>", "window<k>"), the values made complex-symmetric: an off-diagonal entry (i, j) of value a
becomes a (1 + 0.3 i s_ij) with s_ij = s_ji a seeded draw from [-1, 1], a diagonal entry d becomes d (1.1 + 0.2 i s_ii).  The real
systems are at least weakly diagonally dominant (sum |a| <= d), so the twins are strictly dominant in modulus:
|d'| >= 1.1 d >= 1.1 sum |a| > sqrt(1.09) sum |a| >= sum |a'|.  The pattern, and with it every window edge and level set of
tri_multi_cases, is unchanged.

The geometry of the k-wide complex64 sweep is the real one's (a row of k complex64 columns is k / 2 16-byte pieces, a factor value is
8 bytes): tri_multi_cases.mrows, sweep_windows and window_cases apply as they are.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

import c64_checker as K
import ic0_c64_checker as Q
import ic0_checker as IC
import multi_c64_cases as cc
import tri_multi_cases as T

KS = T.KS
F32, F64 = np.float32, np.float64
M_JACOBI, M_IC0, M_ILU0, M_NONE = 0, 1, 2, -1      # lcg_hip.h: LCG_HIP_M_*
E_ARG = T.E_ARG
EXACT_SYSTEMS = ("laplace64", "chain3000", "layered")
SWEEP_SYSTEMS = T.SWEEP_SYSTEMS
SAMPLE14 = {"epsilon": 1e-6, "abs_diff": 0, "max_iterations": 5000}     # sample14.cu's stop rule (tests/test_gpu_ic0_c64.py)

_SYSTEMS = {}


def twin(rp, ci, v, seed=64):
    """The complex-symmetric complex64 twin of a real symmetric matrix (module docstring)."""
    rp, ci = np.asarray(rp), np.asarray(ci)
    n = len(rp) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    col = ci.astype(np.int64)
    key = np.minimum(row, col) * n + np.maximum(row, col)
    uniq, inv = np.unique(key, return_inverse=True)
    s = np.random.default_rng(seed).uniform(-1.0, 1.0, len(uniq))[inv]
    v = np.asarray(v, F64)
    out = np.where(row == col, v * (1.1 + 0.2j * s), v * (1.0 + 0.3j * s))
    return np.asarray(rp, np.int32), np.asarray(ci, np.int32), out.astype(np.complex64)


def system(name):
    """(rowptr, col, complex64 values) of the twin of tri_multi_cases.system("ic0", name)."""
    if name not in _SYSTEMS:
        _SYSTEMS[name] = twin(*T.system("ic0", name))
    return _SYSTEMS[name]


def is_complex_symmetric(rp, ci, v):
    n = len(rp) - 1
    A = sp.csr_matrix((v.astype(np.complex128), ci, rp), shape=(n, n))
    return abs(A - A.T).max() == 0.0


def modulus_dominance(rp, ci, v):
    """min over rows of |a_ii| - sum_{j != i} |a_ij|."""
    n = len(rp) - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    a = np.abs(v.astype(np.complex128))
    d = np.bincount(row[ci == row], a[ci == row], minlength=n)
    return float(np.min(2 * d - np.bincount(row, a, minlength=n)))


# ------------------------------------------------------------------------------------------ the fp32 sweep, restated
class Sweep64:
    """s Jacobi sweeps per triangle of the fp32 factor L (rows sorted, diagonal last), in fp32 on ic0_c64_checker's _vmul / _vdiv:
        y(1) = x / diag,    y(j+1)_i = (x_i - sum_c T(i,c) y(j)_c) / T(i,i)
    one accumulator from x_i, the products subtracted in column order, T = L or L^T.  All rows advance one entry at a time."""

    def __init__(self, n, rowptr, col, val, sweeps):
        self.n, self.s = n, sweeps
        L = sp.csr_matrix((np.asarray(val, np.complex64), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
        L.sort_indices()
        LT = L.T.tocsr()
        LT.sort_indices()
        self.tri = [self._prep(L, False), self._prep(LT, True)]

    @staticmethod
    def _prep(Tm, up):
        rp = Tm.indptr.astype(np.int64)
        s, e = rp[:-1], rp[1:]
        return {"col": Tm.indices.astype(np.int64), "re": Tm.data.real.astype(F32), "im": Tm.data.imag.astype(F32),
                "b": s + 1 if up else s, "f": e if up else e - 1, "dg": s if up else e - 1}

    @staticmethod
    def _one(t, xr, xi, yr, yi):
        b, f, dg, col, vr, vi = t["b"], t["f"], t["dg"], t["col"], t["re"], t["im"]
        ar, ai = xr.copy(), xi.copy()
        for q in range(int((f - b).max()) if len(b) else 0):
            m = q < f - b
            p = np.where(m, b + q, dg)
            pr, pi = Q._vmul(vr[p], vi[p], yr[col[p]], yi[col[p]])
            ar = np.where(m, ar - pr, ar)
            ai = np.where(m, ai - pi, ai)
        return Q._vdiv(ar, ai, vr[dg], vi[dg])

    def _apply(self, t, x, s):
        xr, xi = np.real(x).astype(F32), np.imag(x).astype(F32)
        yr, yi = Q._vdiv(xr, xi, t["re"][t["dg"]], t["im"][t["dg"]])
        for _ in range(s - 1):
            yr, yi = self._one(t, xr, xi, yr, yi)
        return (yr.astype(np.complex64) + 1j * yi.astype(np.complex64)).astype(np.complex64)

    def solve(self, x, which=2, sweeps=None):
        s = self.s if sweeps is None else sweeps
        x = np.asarray(x, np.complex64)
        with np.errstate(all="ignore"):
            if which == 0:
                return self._apply(self.tri[0], x, s)
            if which == 1:
                return self._apply(self.tri[1], x, s)
            return self._apply(self.tri[1], self._apply(self.tri[0], x, s), s)

    def mx(self, x):
        return self.solve(x, 2)


class Sweep128:
    """The same sweeps in complex128 on a complex128 factor L: the twin run of the tolerance rule."""

    def __init__(self, n, rowptr, col, val, sweeps):
        L = sp.csr_matrix((np.asarray(val, np.complex128), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
        self.s = sweeps
        self.tri = []
        for Tm in (L, L.T.tocsr()):
            d = Tm.diagonal()
            self.tri.append((d, (Tm - sp.diags(d)).tocsr()))

    def _apply(self, t, x):
        d, N = t
        y = x / d
        for _ in range(self.s - 1):
            y = (x - N @ y) / d
        return y

    def mx(self, x):
        x = np.asarray(x, np.complex128)
        return self._apply(self.tri[1], self._apply(self.tri[0], x))


# ------------------------------------------------------------------------------------------ the yardstick of the loop
_FACTORS, _RUNS = {}, {}


def solver_system(name):
    """multi_c64_cases' dict for the two systems of the loop's tests: "helmholtz40" and "case10k" (case_10K_cA cast to complex64;
    its b is the file's right-hand side)."""
    if name == "helmholtz40":
        return cc.system("helmholtz", 40)
    key = ("case_10K_cA", 0)
    if key not in cc._SYSTEMS:
        from test_gpu_c64 import case
        rp, ci, v, b, _ = case("10K")
        cc._SYSTEMS[key] = {"key": key, "n": len(rp) - 1, "rp": np.asarray(rp, np.int32), "ci": np.asarray(ci, np.int32), "v": v,
                            "ops": K.csr_ops(rp, ci, v, np.complex64), "xt": None, "b": b}
    return cc._SYSTEMS[key]


def chain_system(n):
    """A complex-symmetric tridiagonal of n rows (the n.k = 2^20 case and its cut): dict as solver_system's."""
    key = ("ctridiag", n)
    if key not in cc._SYSTEMS:
        i = np.arange(n)
        off = (-1.0 + 0.2 * np.sin(0.05 * i[:-1])) + 1j * (0.3 * np.cos(0.03 * i[:-1]))
        d = (3.0 + 0.5 * np.cos(0.01 * i)) + 1j * (0.8 + 0.1 * np.sin(0.02 * i))
        A = sp.diags([off, d, off], [-1, 0, 1], format="csr")
        A.sort_indices()
        rp, ci, v = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.complex64)
        ops = K.csr_ops(rp, ci, v, np.complex64)
        xt = (np.sin(0.001 * i) + 1j * np.cos(0.002 * i)).astype(np.complex64)
        cc._SYSTEMS[key] = {"key": key, "n": n, "rp": rp, "ci": ci, "v": v, "ops": ops, "xt": xt, "b": ops["A"](xt).astype(np.complex64)}
    return cc._SYSTEMS[key]


def checker_apply(S, sweeps, dtype=np.complex64):
    """z = M^-1 r of the checkers for S at a sweeps setting: complex64 -- ic0_c64_checker's fp32 factor with Ic64Apply.mx (exact) or
    Sweep64.mx; complex128 -- ic0_checker's factor of the same complex64 values with SciPy's solves or Sweep128.mx."""
    c64 = np.dtype(dtype) == np.complex64
    fk = (S["key"], c64)
    if fk not in _FACTORS:
        if c64:
            rp, cc_, vv, zp = Q.ic0(S["n"], S["rp"], S["ci"], S["v"])
        else:
            rp, cc_, vv, zp = IC.ic0(S["n"], S["rp"], S["ci"], np.asarray(S["v"], np.complex64).astype(np.complex128))
        assert zp == -1
        _FACTORS[fk] = (rp, cc_, vv)
    ak = (S["key"], c64, sweeps)
    if ak not in _FACTORS:
        f = _FACTORS[fk]
        if c64:
            _FACTORS[ak] = Q.Ic64Apply(S["n"], *f).mx if sweeps == 0 else Sweep64(S["n"], *f, sweeps).mx
        elif sweeps == 0:
            ap = IC.IcApply(IC.to_sparse(S["n"], *f))
            _FACTORS[ak] = lambda x: ap.solve(np.asarray(x, np.complex128), 2)
        else:
            _FACTORS[ak] = Sweep128(S["n"], *f, sweeps).mx
    return _FACTORS[ak]


def checker_column(S, sweeps, bcol, tag, dtype=np.complex64, **para):
    """c64_checker.pcg on one column alone from the zero guess with the matching apply; cached per system, sweeps, tag (the caller's
    name of the column), precision and parameters, and never modified."""
    key = (S["key"], "ic0", sweeps, tag, np.dtype(dtype).name, tuple(sorted(para.items())))
    if key not in _RUNS:
        with np.errstate(all="ignore"):
            _RUNS[key] = K.pcg(S["ops"]["A"], checker_apply(S, sweeps, dtype), bcol, np.zeros(S["n"], dtype), para, dtype)
    return _RUNS[key]


def tol_column(S, sweeps, bcol, tag, **para):
    """multi_c64_cases.tol_column's rule: (the checker's complex64 run, 4 x its distance to its complex128 twin, never below
    64 x 2^-24)."""
    a, e = checker_column(S, sweeps, bcol, tag, np.complex64, **para), checker_column(S, sweeps, bcol, tag, np.complex128, **para)
    d = np.linalg.norm(a["x"].astype(np.complex128) - e["x"]) / max(np.linalg.norm(e["x"]), 1e-30)
    return a, max(4.0 * d, 64 * cc.U32)


# ------------------------------------------------------------------------------------------ drivers (GPU)
def build(api, arrays, jacobi=False):
    A = api.CsrMatrix.from_csr_c64(*arrays)
    A.build_ic0()
    if jacobi:
        A.build_jacobi()
    return A


def cblock(n, k, seed=3):
    r = np.random.default_rng(seed)
    return np.ascontiguousarray((r.uniform(-1.0, 1.0, (n, k)) + 1j * r.uniform(-1.0, 1.0, (n, k))).astype(np.complex64))


def single(torch, lib, A, which, X):
    """lcg_hip_ic0_solve_c64 of every column of the (n, k) host block X: an (n, k) host block."""
    out = np.empty_like(X)
    for j in range(X.shape[1]):
        x = torch.from_numpy(np.ascontiguousarray(X[:, j])).cuda()
        y = torch.full_like(x, 7.0)
        assert lib.lcg_hip_ic0_solve_c64(A.h, which, x.data_ptr(), y.data_ptr()) == 0, lib.lcg_hip_last_error()
        torch.cuda.synchronize()
        out[:, j] = y.cpu().numpy()
    return out


def batched(torch, lib, A, which, X):
    """clcg_hip_ic0_solve_multi_c64 of the (n, k) host block X: an (n, k) host block."""
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    Yd = torch.full_like(Xd, 7.0)
    assert lib.clcg_hip_ic0_solve_multi_c64(A.h, X.shape[1], which, Xd.data_ptr(), Yd.data_ptr()) == 0, lib.lcg_hip_last_error()
    torch.cuda.synchronize()
    return Yd.cpu().numpy()


bits = cc.bits


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def multi_m(lib, api, precond, A, M, B, mem="device", **para):
    """One clcg_hip_lpcg_multi_m_c64 solve: (rc, ret[k], iterations[k], residual[k], M afterwards); M, B (n, k) complex64 arrays."""
    import torch
    k = B.shape[1]
    p = api.clcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    if mem == "device":
        Md = torch.from_numpy(np.ascontiguousarray(M, np.complex64).copy()).cuda()
        Bd = torch.from_numpy(np.ascontiguousarray(B, np.complex64)).cuda()
        rc = lib.clcg_hip_lpcg_multi_m_c64(A.h, k, precond, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        out, Bh = cc.aligned_block(M), cc.aligned_block(B)
        rc = lib.clcg_hip_lpcg_multi_m_c64(A.h, k, precond, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    return rc, list(ret), list(its), list(res), out
