"""CPU-side: the cases of tests/csr_normal_cases.py are what they claim, shown with numpy and the oracle alone -- no system has an
empty column, the edges the table names are there, CG converges within the table's counts -- and the entries of
include/lcg_hip_staging_csr_normal.h are declared in their own header, bound, exported, and answer LCG_HIP_E_NO_DEVICE (never a CPU
result) where there is no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import csr_normal_cases as X
from conftest import ROOT

HEADER = X.staging_header()


# ------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("name", list(X.TABLE))
def test_systems_are_what_the_table_says(name):
    S = X.system(name)
    m0, n, t, dense_col, dense_row, lam = X.TABLE[name]
    assert S["n"] == n and S["m"] == m0 + (n if lam is not None else 0)
    lens, lensT = np.diff(S["rp"]), np.diff(S["rpT"])
    assert lensT.min() >= 1, "an empty column: K^T.K would be singular"
    assert np.all(lens[:m0][np.arange(m0) != (-1 if dense_row is None else dense_row)] == t)
    for i in range(S["m"]):
        c = S["ci"][S["rp"][i]:S["rp"][i + 1]]
        assert np.all(np.diff(c) > 0) and c.min() >= 0 and c.max() < n
    if dense_col:
        assert lensT[0] == m0 and lensT[1:].max() < m0
    if dense_row is not None:
        assert lens[dense_row] == n
    if lam is not None:
        assert np.all(lens[m0:] == 1) and np.array_equal(S["ci"][S["rp"][m0]:], np.arange(n)) and np.all(S["v"][S["rp"][m0]:] == lam)
    # K^T of the table is the transposition, and b is what the module says
    K = X.dense(S)
    KT = np.zeros((n, S["m"]))
    np.add.at(KT, (np.repeat(np.arange(n), lensT), S["ciT"]), S["vT"])
    assert np.array_equal(KT, K.T)
    for c in range(n):
        assert np.all(np.diff(S["ciT"][S["rpT"][c]:S["rpT"][c + 1]]) > 0)
    tol = 1e-12 * np.abs(S["b"]).max()         # (elements of b cancel: against the largest one)
    np.testing.assert_allclose(S["b"], K.T @ (K @ S["xt"]), rtol=0, atol=tol)
    np.testing.assert_allclose(X.ata(S, S["xt"], serial=False), S["b"], rtol=0, atol=tol)
    np.testing.assert_allclose(X.normal_diagonal(S), (K * K).sum(axis=0), rtol=1e-13)
    assert 1.0 <= S["xt"].min() and S["xt"].max() <= 2.0


def test_the_edges_the_table_names():
    assert int(np.diff(X.system("dense3000")["rpT"]).max()) == 3000 > 2304          # longer than k_spmm's window
    assert int(np.diff(X.system("dense3000")["rp"]).max()) == 513
    assert int(np.diff(X.system("tall9000")["rpT"]).max()) == 9000 > 8192           # beyond the LDS-resident sort of the build
    assert int(np.diff(X.system("edge65")["rpT"]).max()) > 32                        # and beyond the one-thread sort
    assert int(np.diff(X.system("main")["rpT"]).max()) <= 32
    assert int((np.diff(X.system("wide513")["rp"]) == 1).sum()) == 513


@pytest.mark.parametrize("name", list(X.TABLE))
def test_cg_converges_within_the_tables_count(name):
    S = X.system(name)
    ref, alt = X.oracle(S, X.CG, S["b"], 600), X.oracle(S, X.CG, S["b"], 600, serial=False)
    assert ref["ret"] == alt["ret"] == X.CONV
    want = X.CG_COUNTS[name]
    assert 0.8 * want - 1 <= ref["iters"] <= want and abs(alt["iters"] - ref["iters"]) <= 2, (name, ref["iters"], alt["iters"])
    assert X.rel(ref["x"], S["xt"]) <= 1e-4
    if name in X.CONDS:
        K = X.dense(S)
        assert abs(np.linalg.cond(K.T @ K) / X.CONDS[name] - 1.0) <= 0.05
    pcg = X.oracle(S, X.PCG, S["b"], 600)
    assert pcg["ret"] == X.CONV and X.rel(pcg["x"], S["xt"]) <= 1e-4


def test_touchy_system_is_touchy_by_the_oracle_alone():
    """Why X.TOUCHY: on dense3000 two roundings of the SAME run -- the oracle on 1e-3 b against 1e-3 x the oracle on b -- are further
    apart at 15 iterations than 50 x the serial / pairwise spread, and CGS at 5 iterations moves further under 1-ulp changes of b than
    50 x its spread.  On the main system neither happens."""
    assert X.TOUCHY == ("dense3000",)
    S = X.system("dense3000")
    b7 = np.ascontiguousarray(X.columns(S, 8)[:, 7])
    x0, x7, a7 = X.oracle(S, X.CG, S["b"], 15)["x"], X.oracle(S, X.CG, b7, 15)["x"], X.oracle(S, X.CG, b7, 15, serial=False)["x"]
    assert X.rel(x7 / 1e-3, x0) > X.FACTOR * X.rel(a7, x7) > 0.0
    ref, alt = X.oracle(S, X.CGS, S["b"], 5), X.oracle(S, X.CGS, S["b"], 5, serial=False)
    moved = max(X.rel(X.oracle(S, X.CGS, X.perturbed(S["b"], seed), 5)["x"], ref["x"]) for seed in range(4))
    assert moved > X.FACTOR * X.rel(alt["x"], ref["x"])
    M = X.system("main")
    m7 = np.ascontiguousarray(X.columns(M, 8)[:, 7])
    for cap in (5, 20):
        twin = X.rel(X.oracle(M, X.CG, m7, cap)["x"] / 1e-3, X.oracle(M, X.CG, M["b"], cap)["x"])
        assert twin <= max(X.FLOOR, X.FACTOR * X.rel(X.oracle(M, X.CG, m7, cap, serial=False)["x"], X.oracle(M, X.CG, m7, cap)["x"]))


def test_product_only_system_has_its_empty_rows_columns_and_duplicates():
    P = X.product_only()
    lens, lensT = np.diff(P["rp"]), np.diff(P["rpT"])
    assert [i for i in range(200) if lens[i] == 0] == [3, 50, 199]
    assert {0, 17, 299} <= set(np.flatnonzero(lensT == 0).tolist())
    dup = 0
    for i in range(200):
        c = P["ci"][P["rp"][i]:P["rp"][i + 1]]
        dup += len(c) - len(set(c.tolist()))
    assert dup == 3 * len([i for i in range(0, 200, 5) if lens[i]])
    # the transposition keeps duplicates in K's own entry order: values of equal (column, row) in the order K holds them
    i = 5
    c, v = P["ci"][P["rp"][i]:P["rp"][i + 1]], P["v"][P["rp"][i]:P["rp"][i + 1]]
    col = c[1]
    sel = P["ciT"][P["rpT"][col]:P["rpT"][col + 1]] == i
    assert sel.sum() == 3 and np.array_equal(P["vT"][P["rpT"][col]:P["rpT"][col + 1]][sel], v[c == col])


def test_columns_follow_the_dense_recipe():
    import dense_multi_cases as dm
    S = X.system("small")
    B = X.columns(S, 8)
    assert np.array_equal(B, dm.columns(dict(n=S["n"], b=S["b"]), 8))
    assert np.array_equal(X.columns(S, 2), B[:, :2]) and not B[:, 3].any()


# ------------------------------------------------------------------------------------------ the entries
@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^\s*([a-z_ 0-9]+?\*?)\s*(c?lcg_hip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = [a.strip() for a in args.split(",")]
        out[name] = (ret.strip(), ["void *" if ("*" in a or a.split()[0].endswith("_t")) else a.split()[-2] for a in args])
    return out


def test_header_equals_the_python_prototypes_and_the_exports():
    from liblcg_amd import _lib
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.STAGING_CSR_NORMAL_SIGNATURES) == X.ENTRIES == sorted(X.STAGING_COVERAGE)
    for other in (_lib.SIGNATURES, _lib.STAGING_SIGNATURES, _lib.STAGING_IC0_C64_SIGNATURES, _lib.STAGING_BOX_MULTI_SIGNATURES,
                  _lib.STAGING_DENSE_C64_SIGNATURES):
        assert not set(X.ENTRIES) & set(other)
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.STAGING_CSR_NORMAL_SIGNATURES[name]
        assert (ret, res) in (("int", C.c_int), ("void", None)), name
        assert len(argtypes) == len(args), name
        for want, got in zip(args, argtypes):
            assert (got is C.c_int) if want == "int" else (got is not C.c_int), (name, want, got)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.build()], text=True)
    exported = set(re.findall(r" T (\S+)", syms))
    assert not [n for n in X.ENTRIES if n not in exported]
    src = open(HEADER).read()
    assert '#include "lcg_hip.h"' in src and "tests/stream_cases.py" in src and "file of its own" in src
    assert "moves into lcg_hip.h with its stream-coverage line" in " ".join(src.split()).replace("* ", "")
    flat = " ".join(src.split()).replace("* ", "")
    assert "K' = [K; sqrt(lambda) I]" in flat and "K's own entry order" in flat
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != os.path.basename(HEADER):
            text = open(os.path.join(ROOT, "include", other)).read()
            assert not any(re.search(r"\b" + n + r"\s*\(", text) for n in X.ENTRIES), other


def test_load_attaches_the_prototypes(lib):
    from liblcg_amd import _lib
    for name, (res, args) in _lib.STAGING_CSR_NORMAL_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def _calls(lib, a, b, u):
    """Every compute entry with a null handle and well-formed vectors."""
    out = (C.c_double * 8)()
    return {
        "lcg_hip_csr_build_normal": lambda: lib.lcg_hip_csr_build_normal(None),
        "lcg_hip_csr_normal_info": lambda: lib.lcg_hip_csr_normal_info(None, None, None, None),
        "lcg_hip_csr_normal_arrays": lambda: lib.lcg_hip_csr_normal_arrays(None, None, None, None),
        "lcg_hip_spmv_t": lambda: lib.lcg_hip_spmv_t(None, a, b),
        "lcg_hip_csr_ata": lambda: lib.lcg_hip_csr_ata(None, a, b),
        "lcg_hip_csr_build_jacobi_normal": lambda: lib.lcg_hip_csr_build_jacobi_normal(None, None),
        "lcg_hip_spmm_t": lambda: lib.lcg_hip_spmm_t(None, 4, a, b),
        "lcg_hip_csr_ata_multi": lambda: lib.lcg_hip_csr_ata_multi(None, 4, a, b),
        "lcg_hip_csr_ata_multi_dot": lambda: lib.lcg_hip_csr_ata_multi_dot(None, 4, a, b, u, out),
        "lcg_hip_csr_normal_lcg_multi": lambda: lib.lcg_hip_csr_normal_lcg_multi(None, 4, a, b, None, None, None, None, 0),
        "lcg_hip_csr_normal_lpcg_multi": lambda: lib.lcg_hip_csr_normal_lpcg_multi(None, 4, a, b, None, None, None, None, 0),
        "lcg_hip_csr_normal_solver_constrained_multi":
            lambda: lib.lcg_hip_csr_normal_solver_constrained_multi(None, 4, X.SPG, a, b, u, u, None, None, None, None, None, 0),
    }


def test_no_device_is_an_error_not_a_cpu_result(lib):
    """A null handle and well-formed vectors: the next thing an entry does is to look for the device.  Without one that is
    LCG_HIP_E_NO_DEVICE; with one the null handle is refused."""
    import torch
    gpu = torch.cuda.is_available()
    bufs = [X.aligned(np.arange(32.0)) for _ in range(3)]
    keep = [w.copy() for w in bufs]
    a, b, u = (w.ctypes.data for w in bufs)
    calls = _calls(lib, a, b, u)
    assert sorted(list(calls) + ["lcg_hip_csr_ata_ax", "lcg_hip_csr_jacobi_normal_mx"]) == sorted(X.COMPUTE)
    for name, call in calls.items():
        assert call() == (X.E_ARG if gpu else X.E_NO_DEVICE), name
        if gpu:
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and "handle is null" in err, err
    assert lib.lcg_hip_csr_cols(None) == 0
    assert all(np.array_equal(w, k) for w, k in zip(bufs, keep))


def test_argument_rules_of_the_k_wide_entries_come_before_the_device(lib):
    """k, a null or misaligned block: LCG_HIP_E_ARG with the entry's name and the reason, with or without a device."""
    raw = np.zeros(64 + 4)
    off = (-raw.ctypes.data % 16) // 8
    pa, podd = raw[off:off + 32].ctypes.data, raw[off + 1:off + 33].ctypes.data
    pb = X.aligned(np.arange(32.0))
    keep = pb.copy()
    out = (C.c_double * 8)()
    entries = {
        "lcg_hip_spmm_t": lambda k, x, y: lib.lcg_hip_spmm_t(None, k, x, y),
        "lcg_hip_csr_ata_multi": lambda k, x, y: lib.lcg_hip_csr_ata_multi(None, k, x, y),
        "lcg_hip_csr_ata_multi_dot": lambda k, x, y: lib.lcg_hip_csr_ata_multi_dot(None, k, x, y, pa, out),
        "lcg_hip_csr_normal_lcg_multi": lambda k, x, y: lib.lcg_hip_csr_normal_lcg_multi(None, k, x, y, None, None, None, None, 0),
        "lcg_hip_csr_normal_lpcg_multi": lambda k, x, y: lib.lcg_hip_csr_normal_lpcg_multi(None, k, x, y, None, None, None, None, 0),
        "lcg_hip_csr_normal_solver_constrained_multi":
            lambda k, x, y: lib.lcg_hip_csr_normal_solver_constrained_multi(None, k, X.PG, x, y, pa, pa, None, None, None, None, None, 0),
    }

    def err():
        return lib.lcg_hip_last_error().decode()
    for name, call in entries.items():
        for k in (0, 1, 3, 16, -2):
            assert call(k, pa, pb.ctypes.data) == X.E_ARG and name + ":" in err() and "k must be 2, 4 or 8" in err(), (name, k, err())
        for x, y in ((None, pa), (pa, None)):
            assert call(4, x, y) == X.E_ARG and name + ":" in err() and "null" in err(), (name, err())
        for x, y in ((podd, pa), (pa, podd)):
            assert call(4, x, y) == X.E_ARG and name + ":" in err() and "16-byte aligned" in err(), (name, err())
    assert lib.lcg_hip_csr_ata_multi_dot(None, 4, pa, pa, None, out) == X.E_ARG and "null" in err()
    assert lib.lcg_hip_csr_ata_multi_dot(None, 4, pa, pa, pa, None) == X.E_ARG and "result array" in err()
    assert lib.lcg_hip_csr_normal_solver_constrained_multi(None, 4, X.PG, pa, pa, None, pa, None, None, None, None, None, 0) == X.E_ARG and "low or hig is null" in err()
    for name in ("lcg_hip_csr_normal_lcg_multi", "lcg_hip_csr_normal_lpcg_multi"):
        assert getattr(lib, name)(None, 4, pa, pa, None, None, None, None, 7) == X.E_ARG and "mem is neither" in err()
    assert lib.lcg_hip_spmv_t(None, None, pa) == X.E_ARG and "lcg_hip_spmv_t: x or y is NULL" in err()
    assert lib.lcg_hip_csr_ata(None, pa, None) == X.E_ARG and "lcg_hip_csr_ata: x or y is NULL" in err()
    assert np.array_equal(pb, keep)


def test_python_front():
    import inspect
    from liblcg_amd import api
    for name in ("n_cols", "build_normal", "normal_info", "normal_to_host", "spmv_t", "spmm_t", "ata", "ata_multi", "ata_multi_dot",
                 "build_jacobi_normal"):
        assert hasattr(api.CsrMatrix, name), name
    assert list(inspect.signature(api.csr_normal_lcg_multi).parameters) == ["K", "M", "B", "param"]
    assert list(inspect.signature(api.csr_normal_lpcg_multi).parameters) == ["K", "M", "B", "param"]
    assert list(inspect.signature(api.csr_normal_solver_constrained_multi).parameters) == ["K", "M", "B", "low", "hig", "param", "solver_id"]
    Z0 = np.zeros((8, 2))
    with pytest.raises(ValueError):
        api.csr_normal_lcg_multi(None, Z0, np.zeros((8, 4)), None)
    with pytest.raises(ValueError):
        api.csr_normal_solver_constrained_multi(None, Z0, Z0, np.zeros(7), np.zeros(8), None)


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu():
    from test_dropin_cpp import _build
    exe = _build("sample_csr_normal")
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode != 0 and p.stderr.strip()
