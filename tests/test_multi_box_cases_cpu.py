"""CPU-side: the cases of tests/multi_box_cases.py are what they claim, shown with the oracle alone -- SPG's product counts differ from
column to column, the bounds are active in some columns and inactive in the 1e-6 b column, no (ret, iterations, n_ax) moves under
four seeded 1-ulp perturbations of b, the breakdown cases break down where the table says -- and the two batched box-constrained
entries are declared in their own header, bound, exported, and check their arguments before the device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import multi_box_cases as X
from conftest import ROOT

HEADER = X.staging_header()
E_ARG = X.E_ARG


# ------------------------------------------------------------------------------------------ the case table
def _runs(port, key, sid, k=8):
    S = X.system(*key)
    lo, hi, cap = X.TABLE[key]
    low, hig = X.bounds(S)
    B = X.columns(S, k)
    return S, low, hig, B, [X.oracle_column(port, S, sid, np.ascontiguousarray(B[:, j]), low, hig, max_iterations=cap, **X.RULE) for j in range(k)]


def test_case10k_counts_are_the_tables(port):
    S, low, hig, B, pg = _runs(port, ("case10k", 10000), X.PG)
    assert S["n"] == 10000
    assert [(r["ret"], r["iters"], r["n_ax"]) for j, r in enumerate(pg) if j != 3] == [(X.MAXIT, 40, 41)] * 7
    assert (pg[3]["ret"], pg[3]["iters"], pg[3]["n_ax"]) == (X.ALREADY, 0, 1)
    spg = _runs(port, ("case10k", 10000), X.SPG)[4]
    assert [r["n_ax"] for r in spg] == [125, 198, 183, 1, 141, 151, 159, 106]
    assert spg[3]["ret"] == X.ALREADY and all(r["ret"] == X.MAXIT and r["iters"] == 40 for j, r in enumerate(spg) if j != 3)
    for runs in (pg, spg):
        active = [int(((r["x"] <= -5.0) | (r["x"] >= 8.0)).sum()) for r in runs]
        assert active[0] > 0 and active[1] == 0 and active[3] == 0, active     # b: cut by the box; 1e-6 b and zero: inside it


@pytest.mark.parametrize("key", [("spd", 65), ("spd", 513), ("spd", 131075)], ids=lambda c: X.IDS[c])
def test_spd_line_searches_differ_from_column_to_column(port, key):
    S, low, hig, B, spg = _runs(port, key, X.SPG)
    cap = X.TABLE[key][2]
    running = [r for j, r in enumerate(spg) if j != 3]
    counts = [r["n_ax"] for r in running]
    assert all(r["ret"] == X.MAXIT and r["iters"] == cap for r in running)
    # every column shrinks, each its own number of times (at 513 and 131075 rows b and -b share one count: six values in seven columns)
    assert len(set(counts)) >= len(counts) - (0 if key[1] == 65 else 1) and min(counts) > cap + 1, counts
    assert (24 <= min(counts) and max(counts) <= 54) if key[1] == 131075 else (29 <= min(counts) and max(counts) <= 61), counts
    active = [int(((r["x"] <= -0.5) | (r["x"] >= 0.8)).sum()) for r in spg]
    assert active[0] > 0 and active[1] == 0, active


@pytest.mark.parametrize("sid", X.SOLVERS)
@pytest.mark.parametrize("key", list(X.TABLE), ids=lambda c: X.IDS[c])
def test_no_verdict_moves_under_one_ulp_of_b(port, key, sid):
    S = X.system(*key)
    low, hig = X.bounds(S)
    cap = X.TABLE[key][2]
    B = X.columns(S, 8)
    worst = 0.0
    for j in range(8):
        sens, flips = X.response(port, S, sid, np.ascontiguousarray(B[:, j]), low, hig, max_iterations=cap, **X.RULE)
        assert flips == 0, (key, sid, j)
        worst = max(worst, sens)
    limit = {"case10k": 1e-11, "tiny": 1e-14, "spd": 1e-13}[key[0]]
    assert worst <= limit, (key, sid, worst)


SPG_SETTINGS = [dict(maxi_m=1), dict(maxi_m=3), dict(maxi_m=X.MAXIM_BOUND), dict(sigma=0.5, beta=0.5)]


@pytest.mark.parametrize("setting", SPG_SETTINGS, ids=lambda s: "-".join(f"{a}{b}" for a, b in s.items()))
def test_spg_settings_do_not_flip_either(port, setting):
    S = X.system("spd", 65)
    low, hig = X.bounds(S)
    B = X.columns(S, 4)
    counts = []
    for j in range(4):
        bcol = np.ascontiguousarray(B[:, j])
        assert X.response(port, S, X.SPG, bcol, low, hig, max_iterations=12, **X.RULE, **setting)[1] == 0, (setting, j)
        counts.append(X.oracle_column(port, S, X.SPG, bcol, low, hig, max_iterations=12, **X.RULE, **setting)["n_ax"])
    assert counts != [X.oracle_column(port, S, X.SPG, np.ascontiguousarray(B[:, j]), low, hig, max_iterations=12, **X.RULE)["n_ax"]
                      for j in range(4)] or setting == dict(maxi_m=X.MAXIM_BOUND), (setting, counts)


@pytest.mark.parametrize("case", X.BREAKDOWN, ids=X.BREAKDOWN_IDS)
def test_breakdown_cases_break_down_where_the_table_says(port, case):
    """The reference has no guard for s.y = 0: the first NaN iterate of column b, the same under four 1-ulp perturbations of b."""
    key, lo, hi = case
    S = X.system(*key)
    low, hig = X.bounds(S, lo, hi)
    want = (2, 2) if key == ("spd", 65) else (3, 4)
    got = tuple(X.first_nan_cap(port, S, sid, S["b"], low, hig, **X.RULE) for sid in X.SOLVERS)
    assert got == want, (key, got)
    for sid, cap in zip(X.SOLVERS, got):
        assert [X.first_nan_cap(port, S, sid, X.perturbed(S["b"], seed), low, hig, **X.RULE) for seed in range(X.SEEDS)] == [cap] * X.SEEDS
        # one iteration earlier: finite, inside the box, stable under 1 ulp of b
        r = X.oracle_column(port, S, sid, S["b"], low, hig, max_iterations=cap - 1, **X.RULE)
        assert np.isfinite(r["x"]).all() and r["x"].min() >= lo and r["x"].max() <= hi
        assert X.response(port, S, sid, S["b"], low, hig, max_iterations=cap - 1, **X.RULE)[1] == 0


def test_the_65_row_breakdown_between_the_tables_bounds_moves_with_one_ulp_of_b(port):
    """Why spd 65 between -0.5 and 0.8 is not a pinned breakdown case: the first NaN iterate is at cap 46 (PG) and 49 (SPG), and four
    1-ulp perturbations of b move it.  The iterate it stops at is the same constrained solution every time."""
    key, lo, hi = X.UNPINNED_BREAKDOWN
    S = X.system(*key)
    low, hig = X.bounds(S, lo, hi)
    for sid, want in zip(X.SOLVERS, (46, 49)):
        cap = X.first_nan_cap(port, S, sid, S["b"], low, hig, **X.RULE)
        assert cap == want
        caps = [X.first_nan_cap(port, S, sid, X.perturbed(S["b"], seed), low, hig, **X.RULE) for seed in range(X.SEEDS)]
        assert len(set(caps + [cap])) > 1 and min(caps) >= 40 and max(caps) <= 60, caps
        last = X.oracle_column(port, S, sid, S["b"], low, hig, max_iterations=cap - 1, **X.RULE)["x"]
        for seed, c in enumerate(caps):
            x = X.oracle_column(port, S, sid, X.perturbed(S["b"], seed), low, hig, max_iterations=c - 1, **X.RULE)["x"]
            assert X.rel(x, last) <= 1e-12


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
        out[name] = (ret.strip(), ["void *" if ("*" in a or a.split()[0].endswith("_t")) else a.split()[0] for a in args])
    return out


def test_header_equals_the_python_prototypes_and_the_exports():
    from liblcg_amd import _lib
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.STAGING_BOX_MULTI_SIGNATURES) == X.ENTRIES == sorted(X.STAGING_COVERAGE)
    for other in (_lib.SIGNATURES, _lib.STAGING_SIGNATURES, _lib.STAGING_IC0_C64_SIGNATURES):
        assert not set(X.ENTRIES) & set(other)
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.STAGING_BOX_MULTI_SIGNATURES[name]
        assert ret == "int" and res is C.c_int and len(argtypes) == len(args), name
        for want, got in zip(args, argtypes):
            assert (got is C.c_int) if want == "int" else (got is not C.c_int), (name, want, got)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.build()], text=True)
    exported = set(re.findall(r" T (\S+)", syms))
    assert not [n for n in X.ENTRIES if n not in exported]
    src = open(HEADER).read()
    assert '#include "lcg_hip.h"' in src and "tests/stream_cases.py" in src and "file of its own" in src
    assert "moves into lcg_hip.h with its stream-coverage line" in " ".join(src.split()).replace("* ", "")
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    assert ("int lcg_hip_solver_constrained_multi(lcg_hip_csr_t A, int k, int solver_id, double *M, const double *B, const double *low, "
            "const double *hig, const lcg_para *param, int *ret, int *iterations, int *products, double *residual, int mem);") in flat
    assert ("int lcg_hip_dense_solver_constrained_multi(lcg_hip_dense_t K, int k, int normal, int solver_id, double *M, const double *B, "
            "const double *low, const double *hig, const lcg_para *param, int *ret, int *iterations, int *products, double *residual, "
            "int mem);") in flat
    for other in ("lcg_hip.h", "lcg_hip_staging.h", "lcg_hip_staging_ic0_c64.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(r"\b" + n + r"\s*\(", text) for n in X.ENTRIES), other


def test_load_attaches_the_prototypes(lib):
    from liblcg_amd import _lib
    for name, (res, args) in _lib.STAGING_BOX_MULTI_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def _calls(lib):
    return {
        "lcg_hip_solver_constrained_multi":
            lambda k, m, b, lo, hi, sid=X.SPG: lib.lcg_hip_solver_constrained_multi(None, k, sid, m, b, lo, hi, None, None, None, None, None, 0),
        "lcg_hip_dense_solver_constrained_multi":
            lambda k, m, b, lo, hi, sid=X.SPG: lib.lcg_hip_dense_solver_constrained_multi(None, k, 1, sid, m, b, lo, hi, None, None, None, None, None, 0),
    }


@pytest.mark.parametrize("name", X.ENTRIES)
def test_argument_rules_come_before_the_device(lib, name):
    """A bad k, a null or misaligned block, a null bound: LCG_HIP_E_ARG with the entry's name and the reason, in that order, with no
    device in the machine and no handle to look at."""
    call = _calls(lib)[name]
    raw = np.zeros(64 + 4)
    off = (-raw.ctypes.data % 16) // 8
    a, odd = raw[off:off + 32], raw[off + 1:off + 33]
    b = X.aligned(np.arange(32.0))
    lo, hi = np.full(16, -1.0), np.full(16, 1.0)
    keep = b.copy()
    pa, pb, podd, pl, ph = a.ctypes.data, b.ctypes.data, odd.ctypes.data, lo.ctypes.data, hi.ctypes.data
    assert pa % 16 == 0 and podd % 16 == 8

    def err():
        return lib.lcg_hip_last_error().decode()
    for k in (0, 1, 3, 16, -2, 5, 6, 7):
        assert call(k, None, None, None, None) == E_ARG and name + ":" in err() and "k must be 2, 4 or 8" in err(), (k, err())
    for k in X.KS:
        for sid in X.SOLVERS:
            for m, bb in ((None, pb), (pa, None)):
                assert call(k, m, bb, None, None, sid) == E_ARG and name + ":" in err() and "null" in err(), err()
            for m, bb in ((podd, pb), (pa, podd)):
                assert call(k, m, bb, None, None, sid) == E_ARG and name + ":" in err() and "16-byte aligned" in err(), err()
            for l, h in ((None, ph), (pl, None)):
                assert call(k, pa, pb, l, h, sid) == E_ARG and name + ":" in err() and "low or hig is null" in err(), err()
            # well-formed vectors: the next thing looked at is the handle, still without a device
            assert call(k, pa, pb, pl, ph, sid) == E_ARG and name + ":" in err() and "handle" in err(), err()
    assert np.array_equal(b, keep)


def test_python_front():
    import inspect
    from liblcg_amd import api
    assert list(inspect.signature(api.lcg_solver_constrained_multi).parameters) == ["A", "M", "B", "low", "hig", "param", "solver_id"]
    assert list(inspect.signature(api.dense_solver_constrained_multi).parameters) == ["K", "M", "B", "low", "hig", "param", "solver_id", "normal"]
    assert [f for f in api.BoxSolveInfo.__dataclass_fields__] == ["ret", "iterations", "residual", "products"]
    Z0 = np.zeros((8, 2))
    with pytest.raises(ValueError):
        api.lcg_solver_constrained_multi(None, Z0, np.zeros((8, 4)), np.zeros(8), np.zeros(8), None)
    with pytest.raises(ValueError):
        api.lcg_solver_constrained_multi(None, Z0, Z0, np.zeros(7), np.zeros(8), None)


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu():
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_box")
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True)
        assert p.returncode != 0 and p.stderr.strip()
