"""CPU-side checks of the complex64 multi-vector entries (clcg_hip_spmm_c64, clcg_hip_spmm_dot_c64, clcg_hip_lbicg_sym_multi_c64,
clcg_hip_lpcg_multi_c64): the header declares them, and the argument rules -- k in {2, 4, 8}, no null block, every base 16-byte
aligned -- are enforced before the device or the handle is looked at, so they hold on a machine without a GPU."""
import ctypes as C
import re

import numpy as np
import pytest

from test_abi import HEADER

E_ARG = -2003
ENTRIES = ["clcg_hip_spmm_c64", "clcg_hip_spmm_dot_c64", "clcg_hip_lbicg_sym_multi_c64", "clcg_hip_lpcg_multi_c64"]


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def test_header_declares_the_entries():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(src.split())
    assert "int clcg_hip_spmm_c64(lcg_hip_csr_t A, int k, const float *X, float *Y);" in flat
    assert "int clcg_hip_spmm_dot_c64(lcg_hip_csr_t A, int k, const float *X, float *Y, const float *U, double *dots);" in flat
    assert ("int clcg_hip_lbicg_sym_multi_c64(lcg_hip_csr_t A, int k, float *M, const float *B, const clcg_para *param, "
            "int *ret, int *iterations, double *residual, int mem);") in flat
    assert ("int clcg_hip_lpcg_multi_c64(lcg_hip_csr_t A, int k, float *M, const float *B, const clcg_para *param, "
            "int *ret, int *iterations, double *residual, int mem);") in flat


def _calls(lib):
    """name -> call(k, a, b): the entry with blocks a, b (addresses) and no handle."""
    out = (C.c_double * 16)()
    return {
        "clcg_hip_spmm_c64": lambda k, a, b: lib.clcg_hip_spmm_c64(None, k, a, b),
        "clcg_hip_spmm_dot_c64": lambda k, a, b: lib.clcg_hip_spmm_dot_c64(None, k, a, b, a, out),
        "clcg_hip_lbicg_sym_multi_c64": lambda k, a, b: lib.clcg_hip_lbicg_sym_multi_c64(None, k, a, b, None, None, None, None, 0),
        "clcg_hip_lpcg_multi_c64": lambda k, a, b: lib.clcg_hip_lpcg_multi_c64(None, k, a, b, None, None, None, None, 0),
    }


def _aligned(n):
    """A float32 array whose base is 16-byte aligned, and a view of it whose base is 8 mod 16."""
    raw = np.zeros(n + 6, np.float32)
    off = (-raw.ctypes.data % 16) // 4
    a = raw[off:off + n]
    odd = raw[off + 2:off + 2 + n]
    assert a.ctypes.data % 16 == 0 and odd.ctypes.data % 16 == 8
    return a, odd


@pytest.mark.parametrize("name", ENTRIES)
def test_argument_rules_come_before_the_device(lib, name):
    call = _calls(lib)[name]
    a, odd = _aligned(256)
    b, _ = _aligned(256)
    pa, pb, po = a.ctypes.data, b.ctypes.data, odd.ctypes.data
    for k in (0, 1, 3, 5, 6, 7, 16, -2):
        assert call(k, pa, pb) == E_ARG, (name, k)
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "k must be 2, 4 or 8" in err, err
    for k in (2, 4, 8):
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
        assert name + ":" in err and "handle is null" in err, err


def test_the_dot_entry_wants_a_result_array(lib):
    a, _ = _aligned(256)
    assert lib.clcg_hip_spmm_dot_c64(None, 4, a.ctypes.data, a.ctypes.data, a.ctypes.data, None) == E_ARG
    err = lib.lcg_hip_last_error().decode()
    assert "clcg_hip_spmm_dot_c64:" in err and "result array" in err, err


def test_python_front_checks_the_complex64_blocks():
    from liblcg_amd import api
    z = np.zeros((8, 4), np.complex64)
    with pytest.raises(ValueError):
        api._block_k(np.zeros(8, np.complex64), cplx="c64")             # not 2-D
    with pytest.raises(ValueError):
        api._block_k(np.zeros((8, 4), np.float32), cplx="c64")          # real where complex is asked for
    with pytest.raises(ValueError):
        api._block_k(np.zeros((8, 4), np.complex128), cplx="c64")       # the other complex type
    with pytest.raises(ValueError):
        api._block_k(z, cplx=True)
    with pytest.raises(ValueError):
        api._block_k(np.zeros((4, 8), np.complex64).T, cplx="c64")      # not C-contiguous
    with pytest.raises(ValueError):
        api._block_k(z, np.zeros((8, 2), np.complex64), cplx="c64")
    assert api._block_k(z, z.copy(), cplx="c64") == 4
    for f in ("clbicg_sym_multi_c64", "clpcg_multi_c64"):
        assert callable(getattr(api, f))
    assert callable(api.CsrMatrix.cspmm_c64) and callable(api.CsrMatrix.cspmm_dot_c64)


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu():
    import subprocess
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_c64")
    import torch
    from conftest import GOLDEN
    if not torch.cuda.is_available():
        p = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
        assert p.returncode == 3 and "csr_create" in p.stderr
