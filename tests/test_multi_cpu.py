"""CPU-side checks of the multi-vector entries (lcg_hip_spmm, lcg_hip_spmm_dot, lcg_hip_lcg_multi, lcg_hip_lpcg_multi): the header
declares them, and the argument rules -- k in {2, 4, 8}, no null block, every base 16-byte aligned -- are enforced before the device
or the handle is looked at, so they hold on a machine without a GPU."""
import ctypes as C
import re

import numpy as np
import pytest

from test_abi import HEADER

E_ARG = -2003


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def test_header_declares_the_entries():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(src.split())
    assert "int lcg_hip_spmm(lcg_hip_csr_t A, int k, const double *X, double *Y);" in flat
    assert ("int lcg_hip_lcg_multi(lcg_hip_csr_t A, int k, double *M, const double *B, const lcg_para *param, "
            "int *ret, int *iterations, double *residual, int mem);") in flat
    assert ("int lcg_hip_lpcg_multi(lcg_hip_csr_t A, int k, double *M, const double *B, const lcg_para *param, "
            "int *ret, int *iterations, double *residual, int mem);") in flat
    assert "int lcg_hip_spmm_dot(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *U, double *dots);" in flat


def _calls(lib):
    """name -> call(k, a, b): the entry with blocks a, b (addresses) and no handle."""
    out3 = (C.c_double * 8)()
    return {
        "lcg_hip_spmm": lambda k, a, b: lib.lcg_hip_spmm(None, k, a, b),
        "lcg_hip_spmm_dot": lambda k, a, b: lib.lcg_hip_spmm_dot(None, k, a, b, a, out3),
        "lcg_hip_lcg_multi": lambda k, a, b: lib.lcg_hip_lcg_multi(None, k, a, b, None, None, None, None, 0),
        "lcg_hip_lpcg_multi": lambda k, a, b: lib.lcg_hip_lpcg_multi(None, k, a, b, None, None, None, None, 0),
    }


def _aligned(n):
    """A float64 array whose base is 16-byte aligned, and a view of it whose base is 8 mod 16."""
    raw = np.zeros(n + 3)
    off = 0 if raw.ctypes.data % 16 == 0 else 1
    a = raw[off:off + n]
    odd = raw[off + 1:off + 1 + n]
    assert a.ctypes.data % 16 == 0 and odd.ctypes.data % 16 == 8
    return a, odd


@pytest.mark.parametrize("name", ["lcg_hip_spmm", "lcg_hip_spmm_dot", "lcg_hip_lcg_multi", "lcg_hip_lpcg_multi"])
def test_argument_rules_come_before_the_device(lib, name):
    call = _calls(lib)[name]
    a, odd = _aligned(64)
    b, _ = _aligned(64)
    pa, pb, po = a.ctypes.data, b.ctypes.data, odd.ctypes.data
    for k in (0, 1, 3, 16, -2, 5, 6, 7):
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
        assert "handle is null" in lib.lcg_hip_last_error().decode()


def test_python_front_checks_the_blocks():
    from liblcg_amd import api
    with pytest.raises(ValueError):
        api._block_k(np.zeros(8))                               # not 2-D
    with pytest.raises(ValueError):
        api._block_k(np.zeros((8, 4), np.float32))
    with pytest.raises(ValueError):
        api._block_k(np.zeros((4, 8)).T)                        # not C-contiguous
    with pytest.raises(ValueError):
        api._block_k(np.zeros((8, 4)), np.zeros((8, 2)))
    assert api._block_k(np.zeros((8, 4)), np.zeros((8, 4))) == 4


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu():
    import os
    import subprocess
    from conftest import ROOT
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi")
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True)
        assert p.returncode == 3 and "csr_from_coo" in p.stderr
