"""Not gpu: the cases of tests/multi_cbicg_cases.py are what they claim -- shown with the oracle and the numpy restatement alone, so a
GPU test that passes on them passes for the stated reason -- and the CPU side of the three staged entries (clcg_hip_spmm_inner,
clcg_hip_spmm_dot2, clcg_hip_lbicgstab_multi): include/lcg_hip_staging.h against _lib.STAGING_SIGNATURES and the library's exports,
the argument rules before the device, the loud failure without one, and the stream-coverage lines the entries will bring along."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import multi_cbicg_cases as zb

ENTRIES = ["clcg_hip_spmm_inner", "clcg_hip_spmm_dot2", "clcg_hip_lbicgstab_multi"]


# ------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("key", sorted(zb.CLASS), ids=zb.sys_id)
def test_systems_have_their_class(key):
    S = zb.system(*key)
    R, folded = zb.CLASS[key]
    assert S["R"] == R and (S["blocks"] > zb.MM_MG) == folded, (S["mean"], S["blocks"])
    A = S["A"]
    if S["n"] > 1:
        up = abs(sp.triu(A, 1)).max()                               # (the halved entries: the lower ones are twice as large)
        assert up > 0.0 and abs(A - A.T).max() >= 0.99 * up         # not symmetric ...
        assert abs(A - A.conj().T).max() >= 0.99 * up               # ... and not Hermitian
        off = abs(A).sum(axis=1).A1 - abs(A.diagonal())
        assert (abs(A.diagonal()) > off).all()                      # diagonally dominant, row by row
    assert np.abs(A.diagonal().imag).min() > 0.0
    if key == ("helm", 182):
        assert S["blocks"] == 518 and S["n"] > zb.cc.TREE_CAP       # the fold; a second stride of a vector pass
    if key == ("band260", 261):
        assert S["n"] % R == 1 and S["blocks"] == 66                # the last block holds one row
    if key in (("band30", 1029), ("band30", 8197), ("band140", 2051)):
        assert S["n"] % R != 0                                      # a partial last block
    assert np.array_equal(S["b"], A @ S["xt"])


def test_the_shadow_vector_tells_a_conjugate_from_none(port):
    rb = zb.shadow(port, 100)
    assert np.abs(rb.imag).min() >= 1.0 and np.abs(rb.real).min() >= 1.0
    assert not port.vecrnd(100, zb.SEED).imag.any()                 # the default draw is real


@pytest.mark.parametrize("case", zb.CAPPED, ids=lambda c: f"{c[0][0]}-{c[0][1]}-cap{c[1]}" if isinstance(c, tuple) else str(c))
def test_capped_cases_end_at_their_cap_and_the_restatement_is_the_oracle(port, case):
    """Plain, every non-zero column of a batch of 8: the oracle runs to the cap (neither converged nor broken down), and the numpy
    restatement agrees with it in code, count, iterate and residual.  The zero column is "already optimised" at count 0."""
    key, cap = case
    S = zb.system(*key)
    n = S["n"]
    rb = zb.shadow(port, n)
    B = zb.columns(n, S["b"], 8)
    para = dict(epsilon=zb.CAP_EPS, max_iterations=cap)
    for j in range(8):
        ref = zb.oracle_column(port, S, B[:, j], ("col", j), rb, **para)
        mine = zb.restated_column(S, None, B[:, j], ("col", j), rb, **para)
        if not B[:, j].any():
            assert ref["ret"] == mine["ret"] == zb.ALREADY and ref["iters"] == mine["iters"] == 0
            continue
        assert ref["ret"] == zb.MAXIT and ref["iters"] == cap, (key, j, ref["ret"], ref["iters"])
        assert np.isfinite(ref["x"].view(np.float64)).all()
        assert mine["ret"] == ref["ret"] and mine["iters"] == ref["iters"], (key, j, mine["ret"], mine["iters"])
        assert np.linalg.norm(mine["x"] - ref["x"]) <= 1e-10 * np.linalg.norm(ref["x"]), (key, j)
        assert abs(mine["residual"] - ref["residual"]) <= 1e-6 * ref["residual"], (key, j, mine["residual"], ref["residual"])


@pytest.mark.parametrize("rule", sorted(zb.RULES))
@pytest.mark.parametrize("key", zb.NON_TINY, ids=zb.sys_id)
def test_every_system_converges_under_both_rules(port, key, rule):
    """The counts the caps rest on: 7-13 iterations on the chains and helms, 4-8 on the bands; with Jacobi 7-13 and 2-5."""
    S = zb.system(*key)
    rb = zb.shadow(port, S["n"])
    para = zb.RULES[rule]
    ref = zb.oracle_column(port, S, S["b"], ("conv", rule), rb, **para)
    mine = zb.restated_column(S, None, S["b"], ("conv", rule), rb, **para)
    jac = zb.restated_column(S, "jacobi", S["b"], ("conv", rule), rb, **para)
    print(key, rule, "oracle", ref["iters"], "restated", mine["iters"], "jacobi", jac["iters"])
    assert ref["ret"] == mine["ret"] == jac["ret"] == zb.CONV
    assert abs(mine["iters"] - ref["iters"]) <= 1
    lo, hi = (7, 13) if key in zb.CHAINS_HELMS else (4, 8)
    assert lo <= ref["iters"] <= hi, (key, rule, ref["iters"])
    lo, hi = (7, 13) if key in zb.CHAINS_HELMS else (2, 5)
    assert lo <= jac["iters"] <= hi, (key, rule, jac["iters"])
    for run in (ref, mine, jac):
        assert np.linalg.norm(run["x"] - S["xt"]) <= 1e-4 * np.linalg.norm(S["xt"])


def test_the_restatement_counts_a_nan_where_it_appears():
    S = zb.system("chain", 65)
    b = S["b"].copy(); b[7] = complex(np.nan, 0.0)
    run = zb.pcbicgstab(S["A"], None, b, np.zeros(65, np.complex128), np.ones(65, np.complex128), 1e-10, 1, 0)
    assert run["ret"] == zb.NANV and run["iters"] == 1


# ------------------------------------------------------------------------------------------------------------ the staged entries
@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def test_staging_header_equals_the_python_prototypes_and_the_exports():
    from liblcg_amd import _lib
    from test_streams_cpu import CTYPE
    protos = zb.staged_prototypes()
    assert sorted(protos) == sorted(_lib.STAGING_SIGNATURES) == sorted(ENTRIES)
    assert not set(protos) & set(_lib.SIGNATURES)                  # an entry is declared in one of the two headers
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.STAGING_SIGNATURES[name]
        assert res is CTYPE[ret] and len(argtypes) == len(args), name
        for want, got in zip(args, argtypes):                       # pointers: void *, or the typed pointer the front passes arrays by
            assert (got is C.c_int) if want == "int" else (got is not C.c_int), (name, want, got)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.build()], text=True)
    exported = set(re.findall(r" T (\S+)", syms))
    assert not [n for n in protos if n not in exported]
    src = open(zb.staging_header()).read()
    assert '#include "lcg_hip.h"' in src and "tests/stream_cases.py" in src and "moves" in src
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    assert "int clcg_hip_spmm_inner(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *u, double *dots);" in flat
    assert "int clcg_hip_spmm_dot2(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *U, double *dots3);" in flat
    assert ("int clcg_hip_lbicgstab_multi(lcg_hip_csr_t A, int k, int precond, double *M, const double *B, const clcg_para *param, "
            "int *ret, int *iterations, double *residual, int mem);") in flat


def test_load_attaches_the_staged_prototypes(lib):
    from liblcg_amd import _lib
    for name, (res, args) in _lib.STAGING_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_staged_entries_have_their_stream_tests():
    """tests/test_streams_cpu.py's check of the coverage table, run over the staged entries and the lines they will bring."""
    from test_streams_cpu import stream_coverage_gaps
    assert stream_coverage_gaps(zb.STAGING_COVERAGE, sorted(zb.staged_prototypes())) == []
    table = dict(zb.STAGING_COVERAGE)
    del table["clcg_hip_spmm_dot2"]
    assert len(stream_coverage_gaps(table, sorted(zb.staged_prototypes()))) == 1


def _aligned(n):
    raw = np.zeros(n + 3)
    off = 0 if raw.ctypes.data % 16 == 0 else 1
    a, odd = raw[off:off + n], raw[off + 1:off + 1 + n]
    assert a.ctypes.data % 16 == 0 and odd.ctypes.data % 16 == 8
    return a, odd


def _calls(lib):
    """name -> call(k, a, b, c): the entry with blocks a, b (and c, the third array of a product) and no handle."""
    out = (C.c_double * 24)()
    return {
        "clcg_hip_spmm_inner": lambda k, a, b, c: lib.clcg_hip_spmm_inner(None, k, a, b, c, out),
        "clcg_hip_spmm_dot2": lambda k, a, b, c: lib.clcg_hip_spmm_dot2(None, k, a, b, c, out),
        "clcg_hip_lbicgstab_multi": lambda k, a, b, c: lib.clcg_hip_lbicgstab_multi(None, k, zb.M_NONE, a, b, None, None, None, None, 0),
    }


@pytest.mark.parametrize("name", ENTRIES)
def test_argument_rules_come_before_the_device(lib, name):
    call = _calls(lib)[name]
    a, odd = _aligned(128)
    b, _ = _aligned(128)
    u, _ = _aligned(128)
    pa, pb, pu, po = a.ctypes.data, b.ctypes.data, u.ctypes.data, odd.ctypes.data
    for k in (0, 1, 3, 5, 6, 7, 16, -2):
        assert call(k, pa, pb, pu) == zb.E_ARG, (name, k)
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "k must be 2, 4 or 8" in err, err
    third = name != "clcg_hip_lbicgstab_multi"
    for k in (2, 4, 8):
        for x, y, z in [(None, pb, pu), (pa, None, pu)] + ([(pa, pb, None)] if third else []):
            assert call(k, x, y, z) == zb.E_ARG, (name, k)
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and "null" in err, err
        for x, y, z in [(po, pb, pu), (pa, po, pu)] + ([(pa, pb, po)] if third else []):
            assert call(k, x, y, z) == zb.E_ARG, (name, k)
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and "16-byte aligned" in err, err
        # well-formed arrays: the next thing looked at is the handle, still without a device
        assert call(k, pa, pb, pu) == zb.E_ARG
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "handle is null" in err, err


def test_the_product_entries_want_a_result_array(lib):
    a, _ = _aligned(128)
    p = a.ctypes.data
    for name in ENTRIES[:2]:
        assert getattr(lib, name)(None, 4, p, p, p, None) == zb.E_ARG
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "result array" in err, err


def test_python_front_checks_its_arguments():
    from liblcg_amd import api
    z = np.zeros((8, 4), np.complex128)
    A = api.CsrMatrix(0, 8, True)                   # a null handle: the front's own checks come before it is looked at
    for u in (np.zeros(8), np.zeros((8, 1), np.complex128), np.zeros(7, np.complex128), np.zeros(16, np.complex128)[::2]):
        with pytest.raises(ValueError):
            A.cspmm_inner(z, z.copy(), u)
    with pytest.raises(ValueError):
        A.cspmm_dot2(z, z.copy(), np.zeros((8, 2), np.complex128))
    with pytest.raises(ValueError):
        api.clbicgstab_multi(A, z, z.copy(), None, precond="ilu0")
    with pytest.raises(ValueError):
        api.clbicgstab_multi(A, z, np.zeros((8, 4)), None)


def test_without_a_device_the_entries_fail_loudly():
    """No quiet fall-back: without a GPU the Python front raises where the handle would be made, and the sample program, compiled
    with plain g++ against the staging header, ends with status 3 and says where."""
    import torch
    from liblcg_amd import api
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_c128_bicgstab")
    if torch.cuda.is_available():
        return
    S = zb.system("chain", 65)
    with pytest.raises(api.LcgHipError):
        api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 3 and "csr_create" in p.stderr
