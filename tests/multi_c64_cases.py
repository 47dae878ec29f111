"""Systems, right-hand sides, the driver and the checker's runs shared by the tests of the complex64 multi-vector path:
tests/test_gpu_multi_c64_solvers.py, tests/test_gpu_multi_c64_product.py and tests/test_multi_c64_cases_cpu.py, which shows with the
checker alone (tests/c64_checker.py, NumPy) that the solver cases are what they claim.  A helper of the tests, not a conftest.

Systems, all complex-symmetric, values complex64:
  * "helmholtz", nx: tests/test_gpu_c64.py's helmholtz(nx), the 5-point Laplacian with 4.3 + 0.8i on the diagonal;
  * every kind of tests/multi_cplx_cases.py ("helm", "chain", "band30", ...), its values cast to complex64.
xt is a seeded random complex64 vector and b = A.xt (the exact product of the rounded inputs, rounded to complex64).

Columns of a batch, (n, k) row-major complex64: b, 1e-2 b, a seeded random vector, a zero column, and for k = 8 also -b, 3 x another
random vector, 0.5 b and 2 b.  k = 2 holds the first two; PAIR_SMALL_ZERO is the k = 2 batch (1e-2 b, zero) of the freezing test."""
import ctypes as C

import numpy as np

import c64_checker as K
import multi_cplx_cases as mcc

CONV, ALREADY, MAXIT, NANV = 0, 2, -1019, -1019     # (CLCG_NAN_VALUE and the real enum's cap code share -1019)
NOPRE, BADEPS, BADMAXIT, E_ARG = -1018, -1021, -1022, -2003
BICG_SYM, PCG = "bicg_sym", "pcg"
SIDS = (BICG_SYM, PCG)
KS = (2, 4, 8)
SMALL = 1e-2
U32 = 2.0 ** -24
C64MM_W = 2304          # multi_c64.hpp: entries per LDS window of k_cspmm_c64

_SYSTEMS = {}


def system(kind, n=0):
    """dict(key, n, rp, ci, v (complex64), ops (c64_checker.csr_ops), xt, b)."""
    key = (kind, n)
    if key not in _SYSTEMS:
        if kind == "helmholtz":
            from test_gpu_c64 import helmholtz
            rp, ci, v = helmholtz(n)
        else:
            S = mcc.system(kind, n)
            rp, ci, v = S["rp"], S["ci"], S["v"].astype(np.complex64)
        nn = len(rp) - 1
        ops = K.csr_ops(rp, ci, v, np.complex64)
        rng = np.random.default_rng(47)     # (on helmholtz(40) at epsilon = 1e-8 the checker then needs 21 / 18 / 21 iterations)
        xt = (rng.standard_normal(nn) + 1j * rng.standard_normal(nn)).astype(np.complex64)
        _SYSTEMS[key] = {"key": key, "n": nn, "rp": np.asarray(rp, np.int32), "ci": np.asarray(ci, np.int32), "v": v, "ops": ops,
                         "xt": xt, "b": ops["A"](xt).astype(np.complex64)}
    return _SYSTEMS[key]


def _crand(r, n):
    return (r.standard_normal(n) + 1j * r.standard_normal(n)).astype(np.complex64)


def columns(S, k):
    """The k right-hand sides of a batch (module docstring), (n, k) row-major complex64."""
    n, b = S["n"], S["b"]
    r = np.random.default_rng(77)
    cols = [b, np.float32(SMALL) * b, _crand(r, n), np.zeros(n, np.complex64), -b, np.float32(3.0) * _crand(r, n),
            np.float32(0.5) * b, np.float32(2.0) * b]
    return np.ascontiguousarray(np.stack(cols[:k], axis=1).astype(np.complex64))


def pair_small_zero(S):
    """The k = 2 batch (1e-2 b, zero)."""
    B = columns(S, 4)
    return np.ascontiguousarray(B[:, [1, 3]])


# ---------------------------------------------------------------------------------------------------------------- the checker
_RUNS = {}


def _jacobi(S, dtype):
    key = (S["key"], "jac", np.dtype(dtype).name)
    if key not in _RUNS:
        _RUNS[key] = K.jacobi(S["rp"], S["ci"], S["v"], dtype)
    return _RUNS[key]


def checker_column(S, sid, bcol, tag, dtype=np.complex64, **para):
    """The checker's run of one column alone from the zero guess; cached per system, solver, tag (the caller's name of the column),
    precision and parameters and never modified."""
    key = (S["key"], sid, tag, np.dtype(dtype).name, tuple(sorted(para.items())))
    if key not in _RUNS:
        m0 = np.zeros(S["n"], dtype)
        with np.errstate(all="ignore"):
            if sid == PCG:
                _RUNS[key] = K.pcg(S["ops"]["A"], _jacobi(S, dtype), bcol, m0, para, dtype)
            else:
                _RUNS[key] = K.bicg_sym(S["ops"]["A"], bcol, m0, para, dtype)
    return _RUNS[key]


def tol_column(S, sid, bcol, tag, **para):
    """tests/test_gpu_c64.py's _tol rule for one column: (the checker's complex64 run, 4 x its distance to its complex128 twin,
    never below 64 x 2^-24)."""
    a, e = checker_column(S, sid, bcol, tag, np.complex64, **para), checker_column(S, sid, bcol, tag, np.complex128, **para)
    d = np.linalg.norm(a["x"].astype(np.complex128) - e["x"]) / max(np.linalg.norm(e["x"]), 1e-30)
    return a, max(4.0 * d, 64 * U32)


# ---------------------------------------------------------------------------------------------------------------- the driver
def aligned_block(a):
    """A complex64 copy of the block a whose base is 16-byte aligned."""
    raw = np.zeros(2 * a.size + 4, np.float32)
    off = (-raw.ctypes.data % 16) // 4
    out = raw[off:off + 2 * a.size].view(np.complex64).reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 16 == 0
    return out


def cmulti64(lib, api, sid, A, M, B, mem="device", **para):
    """One batched solve: (rc, ret[k], iterations[k], residual[k], M afterwards).  M, B: (n, k) complex64 numpy arrays."""
    import torch
    k = B.shape[1]
    p = api.clcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    fn = lib.clcg_hip_lpcg_multi_c64 if sid == PCG else lib.clcg_hip_lbicg_sym_multi_c64
    if mem == "device":
        Md = torch.from_numpy(np.ascontiguousarray(M, np.complex64).copy()).cuda()
        Bd = torch.from_numpy(np.ascontiguousarray(B, np.complex64)).cuda()
        rc = fn(A.h, k, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        out, Bh = aligned_block(M), aligned_block(B)
        rc = fn(A.h, k, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    return rc, list(ret), list(its), list(res), out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def row_bound(lens, R, absax):
    """The per-row bound of the complex64 k-wide product, 3 (len_i + 5 + T) 2^-24 (|A||x|)_i with T = 256 / R lanes per row: the
    derivation and the expression of tests/test_gpu_multi_c64_product.py::test_rounding_bound_on_full_mantissa_data, for the tests
    that anchor that product elsewhere (tests/test_gpu_streams_kwide.py)."""
    return 3.0 * (np.asarray(lens) + 5 + 256 // R) * U32 * absax + 1e-30
