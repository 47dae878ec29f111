"""CPU-side: the cases of tests/tri_multi_cases.py reach the branches of the batched triangular applies they are named for -- shown
with the checkers alone -- and the three new entries (lcg_hip_ic0_solve_multi, lcg_hip_ilu0_solve_multi, lcg_hip_lpcg_multi_m)
are declared, and check their arguments before the device or the handle is looked at, as tests/test_multi_cpu.py shows for the
entries before them."""
import re

import numpy as np
import pytest

import ic0_checker as IC
import ilu0_checker as K
import tri_multi_cases as T
from test_abi import HEADER
from test_multi_cpu import _aligned

E_ARG = T.E_ARG


# ------------------------------------------------------------------------------------------ the helper's constants
def test_constants_are_the_kernels_own():
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "liblcg_amd", "csrc", "csr_tri.hpp")).read()
    assert re.search(r"constexpr int IC_MT = (\d+);", src).group(1) == str(T.IC_MT)
    assert re.search(r"constexpr int IC_MCH = (\d+);", src).group(1) == str(T.IC_MCH)
    assert re.search(r"constexpr int IC_WG = (\d+);", src).group(1) == str(T.IC_WG)
    assert "constexpr int ic_mrows(int k) { return IC_MT * 2 / k; }" in src
    assert [T.mrows(k) for k in T.KS] == [256, 128, 64]
    # at least four workgroups per CU: 12 bytes per window entry against 160 KiB of LDS
    assert 4 * 12 * T.IC_MCH <= 160 * 1024


# ------------------------------------------------------------------------------------------ window edges
@pytest.mark.parametrize("k", T.KS)
@pytest.mark.parametrize("factor", T.FACTORS)
def test_window_matrices_reach_every_edge(factor, k):
    rp, ci, v = T.system(factor, f"window{k}")
    n = len(rp) - 1
    assert n == 5 * T.mrows(k) + T.WINDOW_TAIL
    lo, up = T.tri_rowptrs(factor, rp, ci)
    wins = T.sweep_windows(n, lo, k)
    assert [w[0] for w in wins[1:5]] == list(T.WINDOW_LO)
    assert [w[1] for w in wins[1:5]] == [2048, 2049, 2049, 2048] and [w[2] for w in wins[1:5]] == [0, 0, 1, 1]
    want = {"full_aligned", "full_by_offset", "over_by_one", "over_by_offset", "global_walk", "partial_last_workgroup"}
    assert T.window_cases(n, lo, k) == want
    assert lo[-1] % 4 != 0                              # the last staged 16-byte unit of col ends in the arrays' slack
    if factor == "ilu0":
        assert [w[0] for w in T.sweep_windows(n, up, k)[:5]] == list(T.WINDOW_UP)
        assert T.window_cases(n, up, k) == want
    else:
        assert {"global_walk", "partial_last_workgroup"} <= T.window_cases(n, up, k)
    # the pattern-only rowptrs are the checkers' factors' own
    if k == 8:
        if factor == "ic0":
            L = IC.ic0(n, rp, ci, v)
            assert L[3] == -1 and np.array_equal(L[0], lo)
        else:
            L, U, zp = K.ilu0(n, rp, ci, v)
            assert zp == -1 and np.array_equal(L[0], lo) and np.array_equal(U[0], up)


@pytest.mark.parametrize("factor", T.FACTORS)
def test_dense_row_is_staged_at_every_k(factor):
    """arrow700's last row of lo holds 699 entries (IC(0): and its diagonal): its workgroup's slice fits the window, so the k / 2
    lanes of that ONE row walk 699 entries out of LDS while the other rows' lanes are done after one or two.  (A slice over the
    window is the window matrices' business.)"""
    rp, ci, v = T.system(factor, "arrow700")
    lo, up = T.tri_rowptrs(factor, rp, ci)
    assert lo[700] - lo[699] == (700 if factor == "ic0" else 699)
    for k in T.KS:
        own, cnt, off, nrows = T.sweep_windows(700, lo, k)[-1]
        assert own >= 699 and cnt <= T.IC_MCH and nrows == 700 % T.mrows(k)


# ------------------------------------------------------------------------------------------ rows at the edges of a workgroup
def test_edge_rows_cover_both_sides_of_every_workgroup_size():
    assert T.EDGE_ROWS == [63, 64, 65, 127, 128, 129, 255, 256, 257]
    for k in T.KS:
        R = T.mrows(k)
        for n, groups, last in ((R - 1, 1, R - 1), (R, 1, R), (R + 1, 2, 1)):
            rp, ci, v = T.system("ic0", f"spd{n}")
            wins = T.sweep_windows(n, T.tri_rowptrs("ic0", rp, ci)[0], k)
            assert len(wins) == groups and wins[-1][3] == last
    for n in (1, 2, 3):
        rp, ci, v = T.system("ilu0", f"chain{n}")
        assert len(rp) - 1 == n
        assert all(len(T.sweep_windows(n, T.tri_rowptrs("ilu0", rp, ci)[0], k)) == 1 for k in T.KS)
    for name in T.SWEEP_SYSTEMS:
        for factor in T.FACTORS:
            rp, ci, v = T.system(factor, name)
            assert len(T.tri_rowptrs(factor, rp, ci)[0]) == len(rp)


# ------------------------------------------------------------------------------------------ level widths
@pytest.mark.parametrize("factor", T.FACTORS)
def test_level_widths(factor):
    fw, bw = T.level_widths(factor, *T.system(factor, "chain3000"))
    assert len(fw) == len(bw) == 3000 and fw.max() == bw.max() == 1             # 3000 levels: ONE narrow launch per triangle
    assert IC.segments(fw, T.IC_WG) == IC.segments(bw, T.IC_WG) == 1
    fw, bw = T.level_widths(factor, *T.system(factor, "layered"))
    for w in (fw, bw):
        assert (w > T.IC_WG).sum() == 1 and w.max() >= 1500                     # one wide level ...
    assert list(fw) == T.LAYERS and IC.segments(fw, T.IC_WG) == 3               # ... between two runs of narrow ones
    # (IC(0)'s L^T: the rows nobody reads come first, 1514 of them, then one run of narrow levels)
    assert IC.segments(bw, T.IC_WG) == (2 if factor == "ic0" else 3)
    fw, bw = T.level_widths(factor, *T.system(factor, "laplace64"))
    assert len(fw) == len(bw) == 127 and fw.max() == bw.max() == 64             # narrow groups; forced wide: 127 launches each
    assert IC.segments(fw, T.IC_WG) == 1 and IC.segments(fw, 0) == 127
    if factor == "ilu0":
        assert list(T.level_widths(factor, *T.system(factor, "layered"))[1]) == T.LAYERS_U


# ------------------------------------------------------------------------------------------ the entries
@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    _lib.build()
    return _lib.load()


def test_header_declares_the_entries():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(src.split())
    assert "int lcg_hip_ic0_solve_multi (lcg_hip_csr_t A, int k, int which, const double *X, double *Y);" in flat
    assert "int lcg_hip_ilu0_solve_multi(lcg_hip_csr_t A, int k, int which, const double *X, double *Y);" in flat
    assert "enum { LCG_HIP_M_JACOBI = 0, LCG_HIP_M_IC0 = 1, LCG_HIP_M_ILU0 = 2 };" in flat
    assert ("int lcg_hip_lpcg_multi_m(lcg_hip_csr_t A, int k, int precond, double *M, const double *B, const lcg_para *param, "
            "int *ret, int *iterations, double *residual, int mem);") in flat
    for name in ("lcg_hip_ic0_solve_multi", "lcg_hip_ilu0_solve_multi", "lcg_hip_lpcg_multi_m"):
        assert len(re.findall(r"\b" + name + r"\s*\(", src)) == 1, name            # declared exactly once


def _calls(lib):
    return {
        "lcg_hip_ic0_solve_multi": lambda k, a, b: lib.lcg_hip_ic0_solve_multi(None, k, 2, a, b),
        "lcg_hip_ilu0_solve_multi": lambda k, a, b: lib.lcg_hip_ilu0_solve_multi(None, k, 2, a, b),
        "lcg_hip_lpcg_multi_m": lambda k, a, b: lib.lcg_hip_lpcg_multi_m(None, k, T.M_IC0, a, b, None, None, None, None, 0),
    }


@pytest.mark.parametrize("name", ["lcg_hip_ic0_solve_multi", "lcg_hip_ilu0_solve_multi", "lcg_hip_lpcg_multi_m"])
def test_argument_rules_come_before_the_device(lib, name):
    call = _calls(lib)[name]
    a, odd = _aligned(64)
    b, _ = _aligned(64)
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
        # well-formed blocks: the next thing looked at is the handle, still without a device
        assert call(k, pa, pb) == E_ARG
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "handle is null" in err, err
    assert np.array_equal(b, keep)


def test_python_front_names_the_preconditioners():
    from liblcg_amd import api
    assert api.PRECONDS == {"jacobi": T.M_JACOBI, "ic0": T.M_IC0, "ilu0": T.M_ILU0}
    with pytest.raises(ValueError):
        api.lpcg_multi(None, np.zeros((8, 2)), np.zeros((8, 2)), None, precond="ssor")
    import inspect
    assert list(inspect.signature(api.lpcg_multi).parameters) == ["A", "M", "B", "param", "precond"]
    assert inspect.signature(api.lpcg_multi).parameters["precond"].default == "jacobi"
    assert inspect.signature(api.CsrMatrix.ic0_solve_multi).parameters["which"].default == 2
    assert inspect.signature(api.CsrMatrix.ilu0_solve_multi).parameters["which"].default == 2


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu():
    import os
    import subprocess
    from conftest import ROOT
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_ic0")
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True)
        assert p.returncode == 3 and "csr_from_coo" in p.stderr
