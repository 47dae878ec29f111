"""CPU-side: the cases of tests/tri_multi_c64_cases.py are what they claim -- every complex64 twin is complex-symmetric, dominant in
modulus and factors in the fp32 checker; the window twins reach the window edges of the k-wide sweep; the restated fp32 sweep ends
in the exact solve's bits -- and the two batched complex64 IC(0) entries (clcg_hip_ic0_solve_multi_c64, clcg_hip_lpcg_multi_m_c64)
are declared in their own header, bound, exported, and check their arguments before the device or the handle is looked at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ic0_c64_checker as Q
import tri_multi_c64_cases as Z
import tri_multi_cases as T
from conftest import ROOT

E_ARG = Z.E_ARG
HEADER = os.path.join(ROOT, "include", "lcg_hip_staging_ic0_c64.h")
ENTRIES = ["clcg_hip_ic0_solve_multi_c64", "clcg_hip_lpcg_multi_m_c64"]
ALL_SYSTEMS = sorted(set(Z.SWEEP_SYSTEMS) | set(Z.EXACT_SYSTEMS))


# ------------------------------------------------------------------------------------------ the twins
@pytest.mark.parametrize("name", ALL_SYSTEMS)
def test_every_twin_is_complex_symmetric_dominant_and_factors(name):
    rp, ci, v = Z.system(name)
    rrp, rci, rv = T.system("ic0", name)
    assert v.dtype == np.complex64 and np.array_equal(rp, rrp) and np.array_equal(ci, rci)      # the pattern is the real system's
    assert Z.is_complex_symmetric(rp, ci, v)
    assert np.abs(v.imag).max() > 0.0
    assert Z.modulus_dominance(rp, ci, v) > 0.0
    n = len(rp) - 1
    lrp, lci, lv, zp = Q.ic0(n, rp, ci, v)
    assert zp == -1 and np.isfinite(lv.view(np.float32)).all()
    assert np.array_equal(lrp, T.tri_rowptrs("ic0", rp, ci)[0])                                  # the rowptr the window cases read


@pytest.mark.parametrize("k", T.KS)
def test_window_twins_reach_the_window_edges(k):
    rp, ci, v = Z.system(f"window{k}")
    n = len(rp) - 1
    lrp = Q.ic0(n, rp, ci, v)[0]
    want = {"full_aligned", "full_by_offset", "over_by_one", "over_by_offset", "partial_last_workgroup"}
    assert want <= T.window_cases(n, lrp, k), T.window_cases(n, lrp, k)
    assert [w[0] for w in T.sweep_windows(n, lrp, k)[1:5]] == list(T.WINDOW_LO)


# ------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("name", ["layered", "chain3"])
def test_restated_sweep_ends_in_the_exact_solves_bits(name):
    """A row whose inputs are final has the exact solve's bits; after `levels` sweeps every row has."""
    rp, ci, v = Z.system(name)
    n = len(rp) - 1
    L = Q.ic0(n, rp, ci, v)[:3]
    exact = Q.Ic64Apply(n, *L)
    fw, bw = T.level_widths("ic0", *T.system("ic0", name))
    levels = {0: len(fw), 1: len(bw), 2: max(len(fw), len(bw))}
    assert levels[0] == (9 if name == "layered" else 3)
    x = Z.cblock(n, 1, seed=5)[:, 0]
    for which in (0, 1, 2):
        sw = Z.Sweep64(n, *L, levels[which])
        assert Z.same_bits(sw.solve(x, which), exact.solve(x, which)), (name, which)
    # one sweep is x / diag, which is not the solve
    d = L[2][np.asarray(L[0][1:]) - 1]
    want = Q._vdiv(x.real.astype(np.float32), x.imag.astype(np.float32), d.real.astype(np.float32), d.imag.astype(np.float32))
    one = Z.Sweep64(n, *L, 1).solve(x, 0)
    assert np.array_equal(one.real, want[0]) and np.array_equal(one.imag, want[1])
    assert not Z.same_bits(one, exact.solve(x, 0))


def test_complex128_twin_of_the_sweep_follows_the_fp32_one():
    rp, ci, v = Z.system("layered")
    n = len(rp) - 1
    S = {"key": ("tri_c64", "layered"), "n": n, "rp": rp, "ci": ci, "v": v}
    x = Z.cblock(n, 1, seed=6)[:, 0]
    for sweeps in (0, 2, 4):
        a, e = Z.checker_apply(S, sweeps, np.complex64)(x), Z.checker_apply(S, sweeps, np.complex128)(x)
        assert a.dtype == np.complex64 and e.dtype == np.complex128
        assert np.linalg.norm(a - e) <= 1e-5 * np.linalg.norm(e), sweeps


# ------------------------------------------------------------------------------------------ the entries
@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^\s*([a-z_ ]+?\*?)\s*(c?lcg_hip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = [a.strip() for a in args.split(",")]
        out[name] = (ret.strip(), ["void *" if "*" in a else a.split()[0] for a in args])
    return out


def test_header_equals_the_python_prototypes_and_the_exports():
    from liblcg_amd import _lib
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.STAGING_IC0_C64_SIGNATURES) == ENTRIES
    assert not set(ENTRIES) & set(_lib.SIGNATURES) and not set(ENTRIES) & set(_lib.STAGING_SIGNATURES)
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.STAGING_IC0_C64_SIGNATURES[name]
        assert ret == "int" and res is C.c_int and len(argtypes) == len(args), name
        for want, got in zip(args, argtypes):
            assert (got is C.c_int) if want == "int" else (got is not C.c_int), (name, want, got)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.build()], text=True)
    exported = set(re.findall(r" T (\S+)", syms))
    assert not [n for n in ENTRIES if n not in exported]
    src = open(HEADER).read()
    assert '#include "lcg_hip.h"' in src and "tests/stream_cases.py" in src and "file of its own" in src
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    assert "int clcg_hip_ic0_solve_multi_c64(lcg_hip_csr_t A, int k, int which, const float *X, float *Y);" in flat
    assert ("int clcg_hip_lpcg_multi_m_c64(lcg_hip_csr_t A, int k, int precond, float *M, const float *B, const clcg_para *param, "
            "int *ret, int *iterations, double *residual, int mem);") in flat
    for other in ("lcg_hip.h", "lcg_hip_staging.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(r"\b" + n + r"\s*\(", text) for n in ENTRIES), other


def test_load_attaches_the_prototypes(lib):
    from liblcg_amd import _lib
    for name, (res, args) in _lib.STAGING_IC0_C64_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def _aligned64(n):
    """(a 16-byte aligned complex64 block of n elements, the same memory 8 bytes on)."""
    raw = np.zeros(2 * n + 8, np.float32)
    off = (-raw.ctypes.data % 16) // 4
    a, odd = raw[off:off + 2 * n], raw[off + 2:off + 2 + 2 * n]
    assert a.ctypes.data % 16 == 0 and odd.ctypes.data % 16 == 8
    return a, odd


def _calls(lib):
    return {
        "clcg_hip_ic0_solve_multi_c64": lambda k, a, b, w=2: lib.clcg_hip_ic0_solve_multi_c64(None, k, w, a, b),
        "clcg_hip_lpcg_multi_m_c64": lambda k, a, b, w=2: lib.clcg_hip_lpcg_multi_m_c64(None, k, Z.M_IC0, a, b, None, None, None, None, 0),
    }


@pytest.mark.parametrize("name", ENTRIES)
def test_argument_rules_come_before_the_device(lib, name):
    """A bad k, a null block, a block misaligned by 8 bytes, a bad which: LCG_HIP_E_ARG with the entry's name and the reason, with no
    device in the machine and no handle to look at."""
    call = _calls(lib)[name]
    a, odd = _aligned64(64)
    b, _ = _aligned64(64)
    keep = b.copy()
    pa, pb, po = a.ctypes.data, b.ctypes.data, odd.ctypes.data
    for k in (0, 1, 3, 16, -2, 5, 6, 7):
        assert call(k, pa, pb) == E_ARG, (name, k)
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "k must be 2, 4 or 8" in err, err
    for k in T.KS:
        for x, y in ((None, pb), (pa, None), (None, None)):
            assert call(k, x, y) == E_ARG, (name, k)
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and "null" in err, err
        for x, y in ((po, pb), (pa, po)):
            assert call(k, x, y) == E_ARG, (name, k)
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and "16-byte aligned" in err, err
        for which in (3, -1):                           # (the loop's entry has no which: the same call again)
            assert call(k, pa, pb, which) == E_ARG, (name, k, which)
        # well-formed blocks: the next thing looked at is the handle, still without a device
        assert call(k, pa, pb) == E_ARG
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "handle is null" in err, err
    assert np.array_equal(b, keep)


def test_python_front_names_the_preconditioners():
    import inspect
    from liblcg_amd import api
    assert list(inspect.signature(api.clpcg_multi_c64).parameters) == ["A", "M", "B", "param", "precond"]
    assert inspect.signature(api.clpcg_multi_c64).parameters["precond"].default == "jacobi"
    assert inspect.signature(api.CsrMatrix.ic0_solve_multi_c64).parameters["which"].default == 2
    Z0 = np.zeros((8, 2), np.complex64)
    for bad in ("ssor", "ilu0", None):
        with pytest.raises(ValueError):
            api.clpcg_multi_c64(None, Z0, Z0, None, precond=bad)


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu():
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_c64_ic0")
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True)
        assert p.returncode != 0 and p.stderr.strip()
