"""CPU-side checks of the complex dense k-wide entries (clcg_hip_dense_matmat, clcg_hip_dense_op_multi_dot,
clcg_hip_dense_lbicg_sym_multi, clcg_hip_dense_lpcg_multi, clcg_hip_dense_multi_kernel_name): the header and the Python prototypes
carry them, the argument rules -- k in {2, 4, 8}, no null block, every base 16-byte aligned -- answer before the device or the
handle is looked at, the name list is what the header says, the example compiles; and, with the oracle alone, the systems of
tests/dense_multi_cplx_cases.py are what they claim.  Modelled on tests/test_dense_multi_cpu.py and
tests/test_multi_cplx_cases_cpu.py."""
import ctypes as C
import re

import numpy as np
import pytest

import dense_multi_cplx_cases as zc
import multi_cplx_cases as cc
from dense_multi_cplx_cases import ALREADY, BICG_SYM, CONV, KS, MAXIT, PCG, SIDS
from test_abi import HEADER

E_ARG = -2003
BLOCK_ENTRIES = ["clcg_hip_dense_matmat", "clcg_hip_dense_op_multi_dot", "clcg_hip_dense_lbicg_sym_multi", "clcg_hip_dense_lpcg_multi"]


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def test_header_declares_the_entries():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(src.split())
    assert "int clcg_hip_dense_matmat(lcg_hip_dense_t K, int k, const double *X, double *Y, int layout, int conjugate);" in flat
    assert "int clcg_hip_dense_op_multi_dot(lcg_hip_dense_t K, int k, const double *X, double *Y, const double *U, double *dots);" in flat
    assert "const char *clcg_hip_dense_multi_kernel_name(int index);" in flat
    for name in ("clcg_hip_dense_lbicg_sym_multi", "clcg_hip_dense_lpcg_multi"):
        assert (f"int {name}(lcg_hip_dense_t K, int k, double *M, const double *B, const clcg_para *param, "
                "int *ret, int *iterations, double *residual, int mem);") in flat


def test_python_prototypes_and_every_new_name_says_dense():
    """tests/test_gpu_dense.py takes its list of entries that must refuse a dense handle from the prototypes, by that word."""
    from liblcg_amd import _lib, api
    new = BLOCK_ENTRIES + ["clcg_hip_dense_multi_kernel_name"]
    assert all(n in _lib.SIGNATURES and "dense" in n for n in new)
    for front in ("dense_clbicg_sym_multi", "dense_clpcg_multi"):
        assert callable(getattr(api, front))
    for method in ("cmatmat", "cop_multi_dot", "cmulti_kernel_names"):
        assert callable(getattr(api.DenseMatrix, method))


def _calls(lib):
    """name -> call(k, a, b): the entry with blocks a, b (addresses) and no handle."""
    out = (C.c_double * 16)()
    return {
        "clcg_hip_dense_matmat": lambda k, a, b: lib.clcg_hip_dense_matmat(None, k, a, b, 0, 0),
        "clcg_hip_dense_op_multi_dot": lambda k, a, b: lib.clcg_hip_dense_op_multi_dot(None, k, a, b, a, out),
        "clcg_hip_dense_lbicg_sym_multi": lambda k, a, b: lib.clcg_hip_dense_lbicg_sym_multi(None, k, a, b, None, None, None, None, 0),
        "clcg_hip_dense_lpcg_multi": lambda k, a, b: lib.clcg_hip_dense_lpcg_multi(None, k, a, b, None, None, None, None, 0),
    }


def _aligned(n):
    """A float64 array whose base is 16-byte aligned, and a view of it whose base is 8 mod 16."""
    raw = np.zeros(n + 3)
    off = 0 if raw.ctypes.data % 16 == 0 else 1
    a = raw[off:off + n]
    odd = raw[off + 1:off + 1 + n]
    assert a.ctypes.data % 16 == 0 and odd.ctypes.data % 16 == 8
    return a, odd


@pytest.mark.parametrize("name", BLOCK_ENTRIES)
def test_argument_rules_come_before_the_device_and_the_handle(lib, name):
    call = _calls(lib)[name]
    a, odd = _aligned(128)
    b, _ = _aligned(128)
    pa, pb, po = a.ctypes.data, b.ctypes.data, odd.ctypes.data
    for k in (0, 1, 3, 16, -2, 5, 6, 7):
        assert call(k, pa, pb) == E_ARG, (name, k)
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "k must be 2, 4 or 8" in err, err
    for k in KS:
        for x, y in ((None, pb), (pa, None), (None, None)):
            assert call(k, x, y) == E_ARG, (name, k)
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and "null" in err, err
        for x, y in ((po, pb), (pa, po)):
            assert call(k, x, y) == E_ARG, (name, k)
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and "16-byte aligned" in err, err
        # well-formed blocks: the next thing looked at is the handle, still without a device
        assert call(k, pa, pb) == E_ARG
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "not a dense matrix" in err, err


def test_the_u_block_of_the_carried_sum_is_checked_too(lib):
    a, odd = _aligned(128)
    b, _ = _aligned(128)
    out = (C.c_double * 16)()
    assert lib.clcg_hip_dense_op_multi_dot(None, 4, a.ctypes.data, b.ctypes.data, odd.ctypes.data, out) == E_ARG
    assert "16-byte aligned" in lib.lcg_hip_last_error().decode()


def test_kernel_names_need_no_device(lib):
    names = []
    while lib.clcg_hip_dense_multi_kernel_name(len(names)) is not None:
        names.append(lib.clcg_hip_dense_multi_kernel_name(len(names)).decode())
    assert names == zc.NAMES == ["k_zdnm_row", "k_zdnm_row_split", "k_zdnm_col"]
    assert lib.clcg_hip_dense_multi_kernel_name(-1) is None
    # the real list stays what it was
    real = []
    while lib.lcg_hip_dense_multi_kernel_name(len(real)) is not None:
        real.append(lib.lcg_hip_dense_multi_kernel_name(len(real)).decode())
    assert real == ["k_dnm_row", "k_dnm_row_split", "k_dnm_col", "k_dnm_ata_two_pass"]


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu():
    import subprocess
    from test_dropin_cpp import _build
    exe = _build("sample_dense_complex_multi")
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 3 and "dense_create" in p.stderr


# ---------------------------------------------------------------------------------------------------- the cases are what they claim
@pytest.mark.parametrize("n", zc.SIZES)
def test_systems_are_symmetric_and_not_hermitian(n):
    S = zc.system(n)
    K = S["K"]
    assert np.array_equal(K, K.T)
    if n > 1:
        assert np.abs(K - K.conj().T).max() > 0.01 and np.abs(K.imag[~np.eye(n, dtype=bool)]).max() > 1e-3     # full complex off-diagonals
    else:
        assert K[0, 0].imag != 0.0
    assert S["xt"].real.min() >= 1.0 and S["xt"].imag.max() <= 2.0
    if n >= 65:
        assert 25.0 <= np.linalg.cond(K) <= 40.0, np.linalg.cond(K)
    B = zc.columns(S, 8)
    assert np.array_equal(B[:, 0], S["b"]) and np.array_equal(B[:, 1], zc.SMALL * S["b"]) and not B[:, 3].any()
    assert np.array_equal(zc.columns(S, 2), B[:, :2]) and np.array_equal(zc.columns(S, 4), B[:, :4])


@pytest.mark.parametrize("sid", SIDS)
@pytest.mark.parametrize("n", (65, 200, 513))
def test_counts_of_the_converged_runs_with_the_oracle_alone(n, sid):
    """epsilon = 1e-10, abs_diff = 1: every non-zero column of k = 8's columns converges inside the stated range of counts; the numpy
    restatement agrees with the oracle's count to within 3; the 1e-2 b column's |m|^2 stays below 1, b's ends above."""
    S = zc.system(n)
    B = zc.columns(S, 8)
    lo, hi = zc.COUNTS[sid]
    para = dict(epsilon=1e-10, abs_diff=1)
    for j in range(8 if n == 200 else 4):
        ref = zc.oracle(S, sid, B[:, j], **para)
        if j == 3:
            assert ref["ret"] == ALREADY and ref["iters"] == 0
            continue
        rs = cc.restate(sid, S, B[:, j], **para)
        print(n, sid, j, ref["ret"], ref["iters"], rs["iters"])
        assert ref["ret"] == CONV and rs["ret"] == CONV
        assert lo <= ref["iters"] <= hi and lo <= rs["iters"] <= hi, (n, sid, j, ref["iters"], rs["iters"])
        assert abs(ref["iters"] - rs["iters"]) <= 3
    assert np.linalg.norm(zc.oracle(S, sid, B[:, 1], **para)["x"]) ** 2 < 1.0 < np.linalg.norm(zc.oracle(S, sid, B[:, 0], **para)["x"]) ** 2


@pytest.mark.parametrize("sid", SIDS)
@pytest.mark.parametrize("n", zc.SIZES)
def test_capped_runs_with_the_oracle_alone(n, sid):
    """epsilon = 1e-20 capped at 6 and 25: at n >= 65 no non-zero column converges before the cap; n = 1, 2, 3 end by finite
    termination (converged, in at most n + 1 iterations); the zero column is "already optimised"."""
    S = zc.system(n)
    B = zc.columns(S, 4)
    for cap in (6, 25):
        for j in range(4):
            ref = zc.oracle(S, sid, B[:, j], epsilon=1e-20, max_iterations=cap)
            if j == 3:
                assert ref["ret"] == ALREADY
            elif n >= 65:
                assert ref["ret"] == MAXIT and ref["iters"] == cap, (n, sid, cap, j, ref["ret"], ref["iters"])
            else:
                assert ref["ret"] == CONV and 1 <= ref["iters"] <= n + 1, (n, sid, cap, j, ref["ret"], ref["iters"])
