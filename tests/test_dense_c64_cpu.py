"""CPU-side: the complex64 dense entries are declared in their own header, bound, exported, and check their arguments before the
device is touched; the example compiles with plain g++; and the cases of tests/dense_c64_cases.py are what they claim, shown with the
checker alone (tests/c64_checker.py, NumPy): the capped-run tolerance the GPU tests use comes out of the checker's own runs -- its
complex64 run against its complex128 twin, and its product summed ascending against descending -- and is printed here; every
summation order converges at epsilon = 1e-10 in 30 .. 36 iterations, within one iteration of the others."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_c64_cases as X
from conftest import ROOT

HEADER = X.staging_header()
E_ARG = X.E_ARG


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------ the header, the prototypes, the exports
def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^\s*([a-z_ ]+?\*?)\s*(c?lcg_hip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = [a.strip() for a in args.split(",")]
        out[name] = (ret.strip(), ["void *" if ("*" in a or a.split()[0].startswith("lcg_hip_")) else a.split()[-2] for a in args])
    return out


def test_header_equals_the_python_prototypes_and_the_exports():
    from liblcg_amd import _lib
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.STAGING_DENSE_C64_SIGNATURES) == X.ENTRIES == sorted(X.STAGING_COVERAGE)
    for other in (_lib.SIGNATURES, _lib.STAGING_SIGNATURES, _lib.STAGING_IC0_C64_SIGNATURES, _lib.STAGING_BOX_MULTI_SIGNATURES):
        assert not set(X.ENTRIES) & set(other)
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.STAGING_DENSE_C64_SIGNATURES[name]
        assert {"int": C.c_int, "void": None, "const char *": C.c_char_p}[ret] is res, name
        assert len(argtypes) == len(args), name
        for want, got in zip(args, argtypes):
            assert got is {"int": C.c_int, "int64_t": C.c_int64}.get(want, got) and (want != "void *" or got not in (C.c_int, C.c_int64)), (name, want, got)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.build()], text=True)
    exported = set(re.findall(r" T (\S+)", syms))
    assert not [n for n in X.ENTRIES if n not in exported]
    src = open(HEADER).read()
    assert '#include "lcg_hip.h"' in src and "tests/stream_cases.py" in src and "file of its own" in src
    assert "moves into lcg_hip.h with its stream-coverage line" in " ".join(src.split()).replace("* ", "")
    for other in ("lcg_hip.h", "lcg_hip_staging.h", "lcg_hip_staging_ic0_c64.h", "lcg_hip_staging_box_multi.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(r"\b" + n + r"\s*\(", text) for n in X.ENTRIES), other


def test_load_attaches_the_prototypes(lib):
    from liblcg_amd import _lib
    for name, (res, args) in _lib.STAGING_DENSE_C64_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_kernel_names(lib):
    from liblcg_amd import api
    assert api.DenseMatrix.kernel_names_c64() == X.NAMES
    assert lib.clcg_hip_dense_kernel_name_c64(-1) is None and lib.clcg_hip_dense_kernel_name_c64(len(X.NAMES)) is None
    # the existing tables are what they were
    assert "k_cdn_row" not in api.DenseMatrix.kernel_names() + api.DenseMatrix.multi_kernel_names() + api.DenseMatrix.cmulti_kernel_names()


# ------------------------------------------------------------------------------------------ refusals that need no device
def _err(lib):
    return lib.lcg_hip_last_error().decode()


def test_create_checks_its_arguments_before_the_device(lib):
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    h = C.c_void_p(12345)
    name = "lcg_hip_dense_create_c64"
    assert lib.lcg_hip_dense_create_c64(None, 2, 2, p, 2, 0) == E_ARG and name + ":" in _err(lib) and "handle pointer" in _err(lib)
    assert lib.lcg_hip_dense_create_c64(C.byref(h), 2, 2, None, 2, 0) == E_ARG and "val is NULL" in _err(lib) and h.value is None
    for m, n in ((0, 2), (2, 0), (-1, 2)):
        assert lib.lcg_hip_dense_create_c64(C.byref(h), m, n, p, 2, 0) == E_ARG and "positive" in _err(lib)
    assert lib.lcg_hip_dense_create_c64(C.byref(h), 2, 3, p, 2, 0) == E_ARG and "ld = 2 < N = 3" in _err(lib)
    for mem in (-1, 2):
        assert lib.lcg_hip_dense_create_c64(C.byref(h), 2, 2, p, 2, mem) == E_ARG and "mem" in _err(lib)
    assert h.value is None


def test_single_vector_entries_check_their_arguments_before_the_device(lib):
    a, b = np.zeros(8, np.float32), np.full(8, 3.0, np.float32)
    pa, pb = a.ctypes.data, b.ctypes.data
    name = "clcg_hip_dense_matvec_c64"
    for x, y in ((None, pb), (pa, None)):
        assert lib.clcg_hip_dense_matvec_c64(None, x, y, 0, 0) == E_ARG and name + ":" in _err(lib) and "NULL" in _err(lib)
    assert lib.clcg_hip_dense_matvec_c64(None, pa, pa, 0, 0) == E_ARG and "same vector" in _err(lib)
    for layout, conj in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        assert lib.clcg_hip_dense_matvec_c64(None, pa, pb, layout, conj) == E_ARG and "layout" in _err(lib) and "conjugate" in _err(lib)
    # well-formed: the next thing looked at is the handle, still without a device
    assert lib.clcg_hip_dense_matvec_c64(None, pa, pb, 0, 0) == E_ARG and "complex64 dense matrix" in _err(lib)
    assert lib.lcg_hip_dense_build_jacobi_c64(None, None) == E_ARG and "lcg_hip_dense_build_jacobi_c64:" in _err(lib) and "complex64" in _err(lib)
    assert np.all(b == 3.0)


def _kwide_calls(lib):
    p = lib.clcg_hip_default_parameters()
    ret = (C.c_int * 8)(*([99] * 8))
    return ret, {
        "clcg_hip_dense_matmat_c64": lambda k, x, y, conj=0: lib.clcg_hip_dense_matmat_c64(None, k, x, y, conj),
        "clcg_hip_dense_op_multi_dot_c64": lambda k, x, y: lib.clcg_hip_dense_op_multi_dot_c64(None, k, x, y, None, None),
        "clcg_hip_dense_lbicg_sym_multi_c64": lambda k, x, y: lib.clcg_hip_dense_lbicg_sym_multi_c64(None, k, y, x, C.byref(p), ret, None, None, 1),
        "clcg_hip_dense_lpcg_multi_c64": lambda k, x, y: lib.clcg_hip_dense_lpcg_multi_c64(None, k, y, x, C.byref(p), ret, None, None, 1),
    }


@pytest.mark.parametrize("name", ["clcg_hip_dense_matmat_c64", "clcg_hip_dense_op_multi_dot_c64", "clcg_hip_dense_lbicg_sym_multi_c64",
                                  "clcg_hip_dense_lpcg_multi_c64"])
def test_kwide_entries_check_their_arguments_before_the_device(lib, name):
    """A bad k, a null or misaligned block, a bad conjugate: LCG_HIP_E_ARG with the entry's name and the reason, in that order, with
    no device in the machine and no handle to look at; the outputs are untouched."""
    ret, calls = _kwide_calls(lib)
    call = calls[name]
    raw = np.zeros(2 * 64 + 8, np.float32)
    off = (-raw.ctypes.data % 16) // 4
    a, odd = raw[off:off + 64], raw[off + 2:off + 66]
    b = X.aligned_block(np.full((8, 4), 5 - 2j, np.complex64))
    pa, pb, podd = a.ctypes.data, b.ctypes.data, odd.ctypes.data
    assert pa % 16 == 0 and podd % 16 == 8
    for k in (0, 1, 3, 16, -2, 5, 6, 7):
        assert call(k, None, None) == E_ARG and name + ":" in _err(lib) and "k must be 2, 4 or 8" in _err(lib), (k, _err(lib))
    for k in X.KS:
        for x, y in ((None, pb), (pa, None)):
            assert call(k, x, y) == E_ARG and name + ":" in _err(lib) and "null" in _err(lib), _err(lib)
        for x, y in ((podd, pb), (pa, podd)):
            assert call(k, x, y) == E_ARG and name + ":" in _err(lib) and "16-byte aligned" in _err(lib), _err(lib)
        if name == "clcg_hip_dense_matmat_c64":
            for conj in (2, -1):
                assert call(k, pa, pb, conj) == E_ARG and "conjugate" in _err(lib), _err(lib)
        assert call(k, pa, pb) == E_ARG and name + ":" in _err(lib) and "complex64 dense matrix" in _err(lib), _err(lib)
    assert np.all(b == np.complex64(5 - 2j)) and list(ret) == [99] * 8


def test_python_front():
    import inspect
    from liblcg_amd import api
    assert list(inspect.signature(api.dense_clbicg_sym_multi_c64).parameters) == ["K", "M", "B", "param"]
    assert list(inspect.signature(api.dense_clpcg_multi_c64).parameters) == ["K", "M", "B", "param"]
    for m in ("from_array_c64", "matvec_c64", "build_jacobi_c64", "cmatmat_c64", "cop_multi_dot_c64"):
        assert callable(getattr(api.DenseMatrix, m)), m
    with pytest.raises(TypeError):
        api.DenseMatrix.from_array_c64(np.zeros((2, 2), np.complex128))        # nothing is narrowed or widened silently
    with pytest.raises(TypeError):
        api.DenseMatrix.from_array_c64(np.zeros((2, 2), np.float32))
    Z = np.zeros((8, 2), np.complex64)
    with pytest.raises(ValueError):
        api.dense_clbicg_sym_multi_c64(None, Z, np.zeros((8, 4), np.complex64), None)
    with pytest.raises(ValueError):
        api.dense_clpcg_multi_c64(None, Z.astype(np.complex128), Z.astype(np.complex128), None)


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu(lib):
    bindir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "sample_dense_c64")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sample_dense_c64.cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", exe])
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe, "64"], capture_output=True, text=True, timeout=60)
        assert p.returncode == 3 and p.stderr.strip(), p.stdout + p.stderr


# ------------------------------------------------------------------------------------------ the cases, with the checker alone
def test_shapes_reach_their_branches():
    ra, rp, cp, pk = X.row_auto, X.row_plan, X.col_plan, X.packs
    assert [pk(n) for n in (1, 2, 3, 33, 513, 2050)] == [1, 1, 2, 17, 257, 1025]
    assert set(X.SHAPES) >= {(1, 1), (1, 2), (3, 1), (5, 3), (16, 64), (17, 33), (65, 513), (33, 2050), (200, 64), (4100, 7)}
    assert ra(65, pk(513)) == dict(W=64, S=1, pps=257)                     # 4 x 64 lanes unrolled, then a tail of one pack
    assert ra(33, pk(2050))["S"] == 4                                       # the plan splits by itself
    assert all(ra(m, pk(n))["S"] == 1 for m, n in X.SHAPES if (m, n) != (33, 2050))
    assert rp(200, pk(64), True, True) == dict(W=16, S=2, pps=16)           # ROW_SPLIT forced
    assert [X.can_split(m, n) for m, n in X.SHAPES] == [False, False, False, False, True, False, True, True, True, False]
    c = cp(4100, pk(7))
    assert c["RG"] == 64 and c["RS"] > 1 and c["CT"] == 1
    assert cp(1, 1)["RS"] == 1 and cp(33, pk(2050)) == dict(CW=256, RG=1, CT=5, RS=3, rps=11)     # one row group, folded all the same
    assert 17 % 16 == 1 and 65 % 16 == 1 and 4100 % 16 == 4                 # rows past the last full tile of 16


def test_systems_are_the_complex128_ones_rounded():
    import dense_multi_cplx_cases as zc
    for n in X.SIZES:
        S, Z = X.system(n), zc.system(n)
        assert S["K"].dtype == np.complex64 and np.array_equal(S["K"], Z["K"].astype(np.complex64))
        assert np.array_equal(S["K"], S["K"].T)                                       # complex-symmetric after rounding too
        assert np.array_equal(S["b"], (S["K128"] @ S["xt"].astype(np.complex128)).astype(np.complex64))
        B = X.columns(S, 8)
        assert B.shape == (n, 8) and B.dtype == np.complex64 and np.array_equal(B[:, 0], S["b"]) and not B[:, 3].any()


@pytest.mark.parametrize("n", [65, 200, 513])
def test_tolerance_comes_out_of_the_checker(n, capsys):
    """The capped-run tolerance of tests/test_gpu_dense_c64_solvers.py for column b, printed: max(4 d, 64 u) with d measured on the
    checker alone.  The two summation orders move the iterate by no more than a few 1e-6 relative in 1 .. 6 iterations -- so the
    tolerance stays a rounding-level one -- agree on code and count at every cap, and converge at epsilon = 1e-10 in 30 .. 36
    iterations, within one iteration of each other and of the exactly summed run."""
    S = X.system(n)
    lines = []
    for sid in (X.BICG, X.BICG_SYM, X.PCG):
        for k in range(1, 7):
            a, tol, agree = X.tol_run(S, sid, S["b"], "b", epsilon=1e-30, max_iterations=k)
            assert a["ret"] == X.MAXIT and a["iters"] == k and agree
            assert 64 * X.U32 <= tol <= 2e-5, (n, sid, k, tol)
            lines.append(f"n={n} {sid} k={k} tol={tol:.3e}")
        runs = [X.checker_run(S, sid, S["b"], "b", np.complex64, o, epsilon=1e-10, max_iterations=3000) for o in ("exact", "asc", "desc")]
        assert all(r["ret"] == X.CONV for r in runs)
        its = [r["iters"] for r in runs]
        assert 30 <= min(its) and max(its) <= 36 and max(its) - min(its) <= 1, (n, sid, its)
        lines.append(f"n={n} {sid} converged in {its} iterations (exact / ascending / descending)")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_jacobi_is_the_checkers_formula():
    """dense_c64_cases.jacobi on the dense diagonal is c64_checker.jacobi on the same matrix as CSR arrays, bit for bit."""
    import c64_checker as K
    import dense_checker as dc
    S = X.system(65)
    rp, ci, v = dc.dense_as_csr(S["K"])
    r = np.random.default_rng(3)
    x = (r.standard_normal(65) + 1j * r.standard_normal(65)).astype(np.complex64)
    assert np.array_equal(X.jacobi(S)(x).view(np.uint64), K.jacobi(rp, ci, v)(x).view(np.uint64))
