"""CPU-side checks of the dense k-wide entries (lcg_hip_dense_matmat, lcg_hip_dense_ata_multi, lcg_hip_dense_op_multi_dot,
lcg_hip_dense_lcg_multi, lcg_hip_dense_lpcg_multi): the header declares them, and the argument rules -- k in {2, 4, 8}, no null
block, every base 16-byte aligned -- are enforced before the device or the handle is looked at, so they hold on a machine without
a GPU.  Modelled on tests/test_multi_cpu.py."""
import ctypes as C
import re

import numpy as np
import pytest

from test_abi import HEADER

E_ARG = -2003
BLOCK_ENTRIES = ["lcg_hip_dense_matmat", "lcg_hip_dense_ata_multi", "lcg_hip_dense_op_multi_dot", "lcg_hip_dense_lcg_multi",
                 "lcg_hip_dense_lpcg_multi"]


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def test_header_declares_the_entries():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(src.split())
    assert "int lcg_hip_dense_matmat(lcg_hip_dense_t K, int k, const double *X, double *Y, int layout);" in flat
    assert "int lcg_hip_dense_ata_multi(lcg_hip_dense_t K, int k, const double *X, double *Y);" in flat
    assert ("int lcg_hip_dense_op_multi_dot(lcg_hip_dense_t K, int k, int normal, const double *X, double *Y, const double *U, "
            "double *dots);") in flat
    assert "const char *lcg_hip_dense_multi_last_kernel(lcg_hip_dense_t K);" in flat
    assert "const char *lcg_hip_dense_multi_kernel_name(int index);" in flat
    flat = flat.replace(" (", "(")          # (the two prototypes are aligned under each other)
    for name in ("lcg_hip_dense_lcg_multi", "lcg_hip_dense_lpcg_multi"):
        assert (f"int {name}(lcg_hip_dense_t K, int k, int normal, double *M, const double *B, const lcg_para *param, "
                "int *ret, int *iterations, double *residual, int mem);") in flat


def test_every_new_name_says_dense():
    """tests/test_gpu_dense.py takes its list of entries that must refuse a dense handle from the prototypes, by that word."""
    from liblcg_amd import _lib
    new = BLOCK_ENTRIES + ["lcg_hip_dense_multi_last_kernel", "lcg_hip_dense_multi_kernel_name"]
    assert all(n in _lib.SIGNATURES and "dense" in n for n in new)


def _calls(lib):
    """name -> call(k, a, b): the entry with blocks a, b (addresses) and no handle."""
    out = (C.c_double * 8)()
    return {
        "lcg_hip_dense_matmat": lambda k, a, b: lib.lcg_hip_dense_matmat(None, k, a, b, 0),
        "lcg_hip_dense_ata_multi": lambda k, a, b: lib.lcg_hip_dense_ata_multi(None, k, a, b),
        "lcg_hip_dense_op_multi_dot": lambda k, a, b: lib.lcg_hip_dense_op_multi_dot(None, k, 1, a, b, a, out),
        "lcg_hip_dense_lcg_multi": lambda k, a, b: lib.lcg_hip_dense_lcg_multi(None, k, 1, a, b, None, None, None, None, 0),
        "lcg_hip_dense_lpcg_multi": lambda k, a, b: lib.lcg_hip_dense_lpcg_multi(None, k, 1, a, b, None, None, None, None, 0),
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
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "not a dense matrix" in err, err


def test_the_u_block_of_the_carried_sum_is_checked_too(lib):
    a, odd = _aligned(64)
    b, _ = _aligned(64)
    out = (C.c_double * 8)()
    assert lib.lcg_hip_dense_op_multi_dot(None, 4, 1, a.ctypes.data, b.ctypes.data, odd.ctypes.data, out) == E_ARG
    assert "16-byte aligned" in lib.lcg_hip_last_error().decode()


def test_kernel_names_need_no_device(lib):
    names = []
    while lib.lcg_hip_dense_multi_kernel_name(len(names)) is not None:
        names.append(lib.lcg_hip_dense_multi_kernel_name(len(names)).decode())
    assert names == ["k_dnm_row", "k_dnm_row_split", "k_dnm_col", "k_dnm_ata_two_pass"]
    assert lib.lcg_hip_dense_multi_kernel_name(-1) is None
    # the single-vector list stays what it was
    single = []
    while lib.lcg_hip_dense_kernel_name(len(single)) is not None:
        single.append(lib.lcg_hip_dense_kernel_name(len(single)).decode())
    assert single == ["k_dn_row", "k_dn_row_split", "k_dn_col", "k_dn_ata_two_pass", "k_dn_ata_one_pass", "k_dn_ata_small"]


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu():
    import subprocess
    from test_dropin_cpp import _build
    exe = _build("sample_dense_multi")
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 3 and "dense_create" in p.stderr
