"""Dense operators without a GPU: the numpy checker against the real liblcg bit for bit, the no-device path and the argument
checks of the dense entries."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import dense_checker as dc

SHAPES = [(1, 1), (7, 5), (100, 80), (300, 257)]


def _full_mantissa(rng, shape, cplx=False):
    v = rng.standard_normal(shape) * np.exp2(rng.integers(-8, 9, shape))
    if cplx:
        v = v + 1j * rng.standard_normal(shape) * np.exp2(rng.integers(-8, 9, shape))
    return v


@pytest.fixture(scope="module")
def ref_lib():
    from oracle import pyoracle as po
    if not po.have_ref():
        pytest.skip("oracle/_ref/liblcg_ref.so is not built")
    # exported under their C++ names: found by the demangled name, no mangling is spelled out here
    raw = re.findall(r" T (\S+)", subprocess.check_output(["nm", "-D", "--defined-only", po.REF_SO], text=True))
    nice = re.findall(r" T (.+)", subprocess.check_output(["nm", "-D", "-C", "--defined-only", po.REF_SO], text=True))
    assert len(raw) == len(nice)
    names = {}
    for want in ("lcg_matvec", "clcg_matvec"):
        hits = [r for r, d in zip(raw, nice) if d.startswith(want + "(")]
        assert len(hits) == 1, (want, hits)
        names[want] = hits[0]
    lib = C.CDLL(po.REF_SO)
    real = getattr(lib, names["lcg_matvec"]); cplx = getattr(lib, names["clcg_matvec"])
    real.restype = None; real.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    cplx.restype = None; cplx.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    return real, cplx


def _row_pointers(K):
    rows = [np.ascontiguousarray(K[i]) for i in range(K.shape[0])]
    return rows, (C.c_void_p * len(rows))(*[r.ctypes.data for r in rows])


@pytest.mark.parametrize("shape", SHAPES)
def test_checker_is_liblcg_bit_for_bit(ref_lib, shape):
    real, cplx = ref_lib
    m, n = shape
    rng = np.random.default_rng(m * 1000 + n)
    K = _full_mantissa(rng, (m, n))
    rows, ptrs = _row_pointers(K)
    for layout in (0, 1):
        x = _full_mantissa(rng, n if layout == 0 else m)
        y = np.zeros(m if layout == 0 else n)
        real(ptrs, x.ctypes.data, y.ctypes.data, m, n, layout)
        assert np.array_equal(y, dc.matvec(K, x, layout)), (shape, layout)
    Kc = _full_mantissa(rng, (m, n), cplx=True)
    rows, ptrs = _row_pointers(Kc)
    for layout in (0, 1):
        for conj in (0, 1):
            x = _full_mantissa(rng, n if layout == 0 else m, cplx=True)
            y = np.zeros(m if layout == 0 else n, np.complex128)
            cplx(ptrs, x.ctypes.data, y.ctypes.data, m, n, layout, conj)
            got = dc.cmatvec(Kc, x, layout, conj)
            assert np.array_equal(y.view(np.float64), got.view(np.float64)), (shape, layout, conj)


def test_checker_forms_mean_what_they_say():
    """The checker's forms against numpy's own products (loose: another summation order), so a swapped layout or a conjugated x
    cannot hide behind the bit-for-bit test's skip."""
    rng = np.random.default_rng(5)
    K = rng.standard_normal((9, 6)) + 1j * rng.standard_normal((9, 6))
    x6 = rng.standard_normal(6) + 1j * rng.standard_normal(6); x9 = rng.standard_normal(9) + 1j * rng.standard_normal(9)
    np.testing.assert_allclose(dc.cmatvec(K, x6, 0, 0), K @ x6, rtol=1e-13)
    np.testing.assert_allclose(dc.cmatvec(K, x6, 0, 1), K.conj() @ x6, rtol=1e-13)
    np.testing.assert_allclose(dc.cmatvec(K, x9, 1, 0), K.T @ x9, rtol=1e-13)
    np.testing.assert_allclose(dc.cmatvec(K, x9, 1, 1), K.conj().T @ x9, rtol=1e-13)
    np.testing.assert_allclose(dc.ata(K.real, x6.real), K.real.T @ (K.real @ x6.real), rtol=1e-13)
    np.testing.assert_allclose(dc.normal_diagonal(K.real), np.diag(K.real.T @ K.real), rtol=1e-13)


def _lib():
    from liblcg_amd import _lib
    return _lib.load()


def test_dense_create_fails_loudly_without_gpu():
    import torch
    lib = _lib()
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path cannot be exercised")
    K = np.ones((4, 3))
    h = C.c_void_p()
    assert lib.lcg_hip_dense_create(C.byref(h), 4, 3, K.ctypes.data, 3, 0, 0) == -2001
    assert not h.value and b"no" in lib.lcg_hip_last_error().lower()
    rows = (C.c_void_p * 4)(*[K[i].ctypes.data for i in range(4)])
    assert lib.lcg_hip_dense_create_rows(C.byref(h), 4, 3, rows, 0) == -2001


def test_dense_argument_checks():
    """Before any device work: they hold with and without a GPU."""
    lib = _lib()
    E_ARG = -2003
    K = np.ones((4, 3))
    h = C.c_void_p()
    assert lib.lcg_hip_dense_create(C.byref(h), 4, 3, K.ctypes.data, 2, 0, 0) == E_ARG      # ld < N
    assert b"ld" in lib.lcg_hip_last_error()
    assert lib.lcg_hip_dense_create(C.byref(h), 0, 3, K.ctypes.data, 3, 0, 0) == E_ARG
    assert lib.lcg_hip_dense_create(C.byref(h), 4, -1, K.ctypes.data, 3, 0, 0) == E_ARG
    assert lib.lcg_hip_dense_create(C.byref(h), 4, 3, None, 3, 0, 0) == E_ARG
    assert lib.lcg_hip_dense_create(None, 4, 3, K.ctypes.data, 3, 0, 0) == E_ARG
    assert lib.lcg_hip_dense_create(C.byref(h), 4, 3, K.ctypes.data, 3, 0, 7) == E_ARG
    assert lib.lcg_hip_dense_create_rows(C.byref(h), 4, 3, None, 0) == E_ARG
    rows = (C.c_void_p * 4)(K[0].ctypes.data, None, K[2].ctypes.data, K[3].ctypes.data)
    assert lib.lcg_hip_dense_create_rows(C.byref(h), 4, 3, rows, 0) == E_ARG
    assert b"row 1" in lib.lcg_hip_last_error()
    # something that is not a dense handle (here: plain memory) is told by its first word; nothing else of it is read
    fake = (C.c_double * 256)()
    x = (C.c_double * 8)(); y = (C.c_double * 8)()
    assert lib.lcg_hip_dense_matvec(fake, x, y, 0) == E_ARG
    assert b"not a dense matrix" in lib.lcg_hip_last_error()
    assert lib.clcg_hip_dense_matvec(fake, x, y, 0, 0) == E_ARG
    assert lib.lcg_hip_dense_ata(fake, x, y) == E_ARG
    assert lib.lcg_hip_dense_build_jacobi(fake, 1, None) == E_ARG
    assert lib.lcg_hip_dense_set_kernel(fake, 0) == E_ARG
    assert lib.lcg_hip_dense_destroy(fake) == E_ARG and lib.lcg_hip_dense_destroy(None) == E_ARG
    assert lib.lcg_hip_dense_rows(fake) == E_ARG and lib.lcg_hip_dense_cols(None) == E_ARG
    assert lib.lcg_hip_dense_last_kernel(fake) == b""
    names = []
    while lib.lcg_hip_dense_kernel_name(len(names)) is not None:
        names.append(lib.lcg_hip_dense_kernel_name(len(names)))
    assert len(names) == len(set(names)) >= 5 and lib.lcg_hip_dense_kernel_name(-1) is None
