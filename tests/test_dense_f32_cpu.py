"""CPU-side: the entries of include/lcg_hip_staging_dense_f32.h (a real dense matrix stored in fp32) are declared in their own header,
bound, exported, check their arguments before the device is touched and answer LCG_HIP_E_NO_DEVICE -- never a CPU result -- where
there is no device; the Python front casts nothing silently; the example compiles with plain g++; and the cases of
tests/dense_f32_cases.py are what they claim."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_f32_cases as X
from conftest import ROOT

HEADER = X.staging_header()
E_ARG = X.E_ARG


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def _err(lib):
    return lib.lcg_hip_last_error().decode()


def test_header_equals_the_python_prototypes_and_the_exports():
    from liblcg_amd import _lib
    protos = X.staged_prototypes()
    assert sorted(protos) == sorted(_lib.STAGING_DENSE_F32_SIGNATURES) == X.ENTRIES == sorted(X.STAGING_COVERAGE)
    assert protos["lcg_hip_dense_create_f32"] == ("int", ["void *", "int", "int", "void *", "int64_t", "int"])
    assert protos["lcg_hip_dense_value_bytes"] == ("int", ["void *"])
    for other in (_lib.SIGNATURES, _lib.STAGING_SIGNATURES, _lib.STAGING_IC0_C64_SIGNATURES, _lib.STAGING_BOX_MULTI_SIGNATURES,
                  _lib.STAGING_DENSE_C64_SIGNATURES, _lib.STAGING_CSR_NORMAL_SIGNATURES):
        assert not set(X.ENTRIES) & set(other)
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.STAGING_DENSE_F32_SIGNATURES[name]
        assert ret == "int" and res is C.c_int, name
        assert len(argtypes) == len(args), name
        for want, got in zip(args, argtypes):
            assert got is {"int": C.c_int, "int64_t": C.c_int64}.get(want, got) and (want != "void *" or got not in (C.c_int, C.c_int64)), (name, want, got)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.build()], text=True)
    exported = set(re.findall(r" T (\S+)", syms))
    assert not [n for n in X.ENTRIES if n not in exported]
    src = open(HEADER).read()
    flat = " ".join(src.split()).replace("* ", "")
    assert '#include "lcg_hip.h"' in src and "tests/stream_cases.py" in src and "file of its own" in src
    assert "moves into lcg_hip.h with its stream-coverage line" in flat
    assert "is the fp64 handle of the widened matrix" in flat and "gives the same bits" in flat
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != os.path.basename(HEADER):
            text = open(os.path.join(ROOT, "include", other)).read()
            assert not any(re.search(r"\b" + n + r"\s*\(", text) for n in X.ENTRIES), other
    # the value_bytes query is the table's one exemption: it is answered on the host
    assert [n for n, v in X.STAGING_COVERAGE.items() if isinstance(v, tuple)] == ["lcg_hip_dense_value_bytes"]


def test_load_attaches_the_prototypes(lib):
    from liblcg_amd import _lib
    for name, (res, args) in _lib.STAGING_DENSE_F32_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_create_checks_its_arguments_before_the_device(lib):
    """lcg_hip_dense_create's checks, in its order, with its codes and texts."""
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    h = C.c_void_p(12345)
    name = "lcg_hip_dense_create_f32"
    assert lib.lcg_hip_dense_create_f32(None, 2, 2, p, 2, 0) == E_ARG and name + ":" in _err(lib) and "handle pointer" in _err(lib)
    assert lib.lcg_hip_dense_create_f32(C.byref(h), 2, 2, None, 2, 0) == E_ARG and "val is NULL" in _err(lib) and h.value is None
    for m, n in ((0, 2), (2, 0), (-1, 2)):
        assert lib.lcg_hip_dense_create_f32(C.byref(h), m, n, p, 2, 0) == E_ARG and "positive" in _err(lib)
    assert lib.lcg_hip_dense_create_f32(C.byref(h), 2, 3, p, 2, 0) == E_ARG and "ld = 2 < N = 3" in _err(lib)
    for mem in (-1, 2):
        assert lib.lcg_hip_dense_create_f32(C.byref(h), 2, 2, p, 2, mem) == E_ARG and "mem" in _err(lib)
    assert h.value is None
    # the same calls on lcg_hip_dense_create give the same codes
    d = np.zeros(64)
    assert lib.lcg_hip_dense_create(C.byref(h), 2, 3, d.ctypes.data, 2, 0, 0) == E_ARG and "ld = 2 < N = 3" in _err(lib)
    assert lib.lcg_hip_dense_create(C.byref(h), 2, 2, None, 2, 0, 0) == E_ARG and lib.lcg_hip_dense_create(C.byref(h), 2, 2, d.ctypes.data, 2, 0, 2) == E_ARG


def test_no_device_is_an_error_not_a_cpu_result(lib):
    """A well-formed create: the next thing it does is to look for the device.  Without one that is LCG_HIP_E_NO_DEVICE and no handle."""
    import torch
    K = X.matrix(5, 7)
    h = C.c_void_p(12345)
    rc = lib.lcg_hip_dense_create_f32(C.byref(h), 5, 7, K.ctypes.data, 7, 0)
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        assert lib.lcg_hip_dense_value_bytes(h) == 4
        assert lib.lcg_hip_dense_destroy(h) == 0
    else:
        assert rc == X.E_NO_DEVICE and h.value is None and _err(lib)
    # the query is answered on the host: anything that is not a dense handle is an argument error, with or without a device
    assert lib.lcg_hip_dense_value_bytes(None) == E_ARG and "lcg_hip_dense_value_bytes:" in _err(lib)


def test_python_front_casts_nothing():
    from liblcg_amd import api
    assert callable(api.DenseMatrix.from_array_f32) and isinstance(api.DenseMatrix.value_bytes, property)
    for bad in (np.zeros((2, 2), np.float64), np.zeros((2, 2), np.complex64), np.zeros((2, 2), np.int32)):
        with pytest.raises(TypeError):
            api.DenseMatrix.from_array_f32(bad)
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError):
        api.DenseMatrix.from_array_f32(torch.zeros((2, 2), dtype=torch.float64))


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu(lib):
    bindir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "sample_dense_f32")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sample_dense_f32.cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", exe])
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe, "100", "80"], capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and p.stderr.strip(), p.stdout + p.stderr


# ------------------------------------------------------------------------------------------ the cases
def test_matrices_and_twins():
    for m, n in X.SHAPES + [X.PADDED[:2]]:
        K = X.matrix(m, n)
        assert K.dtype == np.float32 and K.shape == (m, n) and np.abs(K).max() <= 1.0
        T = X.twin(K)
        assert T.dtype == np.float64 and np.array_equal(T.astype(np.float32), K)          # the widening is exact
    V = X.padded(X.matrix(37, 29), 40)
    assert V.strides == (160, 4) and np.array_equal(V, X.matrix(37, 29))


def test_shapes_reach_their_branches():
    acc = {s: X.accepted(*s) for s in X.SHAPES + [X.PADDED[:2]]}
    full = list(range(7))
    assert acc[(100, 80)] == full and acc[(1000, 800)] == full and acc[(2048, 2048)] == full
    assert X.forced_strips(100, 80) == 2 and X.forced_strips(1000, 800) == 9 and X.forced_strips(8191, 1025) == 2
    assert acc[(8191, 1025)] == full and X.packs(1025) == 513
    assert acc[(1, 4097)] == [0, 1, 2, 3, 4] and acc[(3, 5000)] == [0, 1, 2, 3, 4]      # N > 2048: no one-pass form
    for s in ((1, 1), (4097, 1), (5000, 3), (5, 7), (37, 29)):
        assert acc[s] == [0, 1, 3, 4, 5, 6], s                                          # nothing to split
    assert X.packs(2048) == 1024 and X.packs(7) == 4 and X.packs(1) == 1


def test_special_matrix_holds_what_it_says():
    K = X.special_matrix()
    f = np.finfo(np.float32)
    assert K.shape == (64, 66) and K.dtype == np.float32
    sub = (K != 0) & (np.abs(K) < f.tiny)
    assert sub.sum() > 300 and K[0, 0] == np.float32(1e-40) and K[2, 0] == f.smallest_subnormal
    assert np.signbit(K[5, :10]).all() and not K[5, :10].any() and not np.signbit(K[4, :10]).any() and not K[4, :10].any()
    assert np.signbit(K[:, 12]).all() and not K[:, 12].any()
    assert K[6, 5] == f.max and K[7, 64] == -f.max
    assert np.isinf(K).sum() == 1 and np.isnan(K).sum() == 1
    T = X.twin(K)
    assert np.array_equal(T[sub].astype(np.float32), K[sub]) and (np.abs(T[sub]) >= np.finfo(np.float64).tiny).all()   # normal doubles
