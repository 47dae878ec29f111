"""No GPU: the cases of tests/multi_bicg_cases.py are what they claim, shown with the oracle alone.

  * every system is non-symmetric and lands in the class (rows per block, folded or not) it is there for;
  * pbicgstab without an apply IS the oracle's lbicgstab per column: same code, same count, x within 1e-12 relative;
  * every non-zero column of every non-tiny system runs more than 8 iterations to convergence under both rules, except the 1e-6 b
    column, which stops at least 2 iterations before column 0 (two verdicts can meet in one call);
  * the oracle's response at a cap of 8 to 1-ulp changes of b stays below 2e-11, so the GPU test's band max(1e-9, 50 x response)
    is its floor on these systems;
  * the preconditioned restatement in x-space walks ilu0_checker's u-space run (the counts the GPU test's statements lean on)."""
import numpy as np
import pytest

import ilu0_checker as K
import multi_bicg_cases as bc
import tri_multi_cases as tm

K4 = 4


@pytest.mark.parametrize("key", bc.NON_TINY + bc.TINY, ids=bc.sys_id)
def test_systems_are_nonsymmetric_and_in_their_class(key):
    S = bc.system(*key)
    As = bc.sparse(S)
    if S["n"] > 1:
        assert abs(As - As.T).max() > 0.0
    assert (S["R"], S["blocks"] > bc.mc.MM_MG) == bc.CLASS[key], (S["R"], S["blocks"])
    d = As.diagonal()
    off = np.asarray(abs(As).sum(axis=1)).ravel() - np.abs(d)
    assert (d > 0).all() and (key[0] == "convdiff" or (np.abs(d) > off).all())      # (convdiff: an M-matrix, weakly dominant)
    if key == ("nonsym", 32771):
        assert S["blocks"] == 513 and S["n"] * 8 // 2 > bc.mc.STRIDE             # the fold; at k = 8 a second stride
    if key == ("nonsym", 131075):
        assert S["n"] * 8 >= 1 << 20 > S["n"] * 4


@pytest.mark.parametrize("rule", sorted(bc.RULES))
@pytest.mark.parametrize("key", bc.NON_TINY, ids=bc.sys_id)
def test_restatement_is_the_oracle_and_counts_are_as_claimed(port, key, rule):
    S = bc.system(*key)
    para = bc.RULES[rule]
    B = bc.columns(S["n"], S["b"], 8)
    its = []
    for j in range(8):
        ref = bc.oracle_column(port, S, B[:, j], ("col", j), **para)
        mine = bc.restated_column(S, "plain", None, B[:, j], ("col", j), **para)
        assert (mine["ret"], mine["iters"]) == (ref["ret"], ref["iters"]), (j, mine["ret"], mine["iters"], ref["ret"], ref["iters"])
        assert np.linalg.norm(mine["x"] - ref["x"]) <= 1e-12 * np.linalg.norm(ref["x"]), j
        its.append(ref["iters"])
        if j == 3:
            assert ref["ret"] == bc.ALREADY and ref["iters"] == 0
        else:
            assert ref["ret"] == bc.CONV
            if j != 1:
                assert ref["iters"] > bc.CAP, (j, ref["iters"])
    print(key, rule, "iterations", its)
    assert 0 < its[1] and its[1] + 2 <= its[0], its


@pytest.mark.parametrize("key", bc.TINY, ids=bc.sys_id)
def test_restatement_on_tiny_systems(port, key):
    """Codes as the oracle's; a NaN column's count is one more than the oracle's (the iteration in which the NaN appeared)."""
    S = bc.system(*key)
    for rule, para in bc.RULES.items():
        B = bc.columns(S["n"], S["b"], K4)
        for j in range(K4):
            ref = bc.oracle_column(port, S, B[:, j], ("col", j), **para)
            mine = bc.restated_column(S, "plain", None, B[:, j], ("col", j), **para)
            assert mine["ret"] == ref["ret"], (rule, j)
            assert mine["iters"] == ref["iters"] + (1 if ref["ret"] == bc.NANV else 0), (rule, j)


@pytest.mark.parametrize("key", [("nonsym", 65), ("nonsym", 513), ("nonsym", 32771), bc.CONVDIFF], ids=bc.sys_id)
def test_response_at_the_cap_stays_under_the_floor(port, key):
    S = bc.system(*key)
    B = bc.columns(S["n"], S["b"], K4)
    para = dict(max_iterations=bc.CAP, **bc.RULES["abs"])
    worst = 0.0
    for j in (0, 1, 2):
        worst = max(worst, bc.response(lambda b, tag: bc.oracle_column(port, S, b, tag, **para), B[:, j], (j,)))
    print(key, "response at cap", bc.CAP, worst)
    assert worst < 2e-11


def test_x_space_restatement_walks_the_u_space_run():
    """m = M^-1 u in exact arithmetic: with the exact ILU(0) apply and with 2 and 4 sweeps, pbicgstab from m0 = 0 stops where
    ilu0_checker.lbicgstab on A.M^-1 stops (relative rule on |u| there, on |m| here: both clamped to 1 or far above eps either way;
    counts within 2) and solves the system; the counts are the ones the GPU test's statements leave room for."""
    S = bc.system(*bc.CONVDIFF)
    As = bc.sparse(S)
    n = S["n"]
    plain = bc.restated_column(S, "plain", None, S["b"], ("col", 0), **bc.RULES["rel"])["iters"]
    counts = {}
    for sweeps in (0, 2, 4):
        apply = tm.checker_apply("ilu0", S["key"], n, S["rp"], S["ci"], S["v"], sweeps)
        _, t_u = K.lbicgstab(lambda x: As @ apply(x), S["b"], 1e-14)
        mine = bc.restated_column(S, ("ilu0", sweeps), apply, S["b"], ("col", 0), **bc.RULES["rel"])
        assert mine["ret"] == bc.CONV and abs(mine["iters"] - t_u) <= 2, (sweeps, mine["iters"], t_u)
        assert np.linalg.norm(S["b"] - As @ mine["x"]) <= 1e-6 * np.linalg.norm(S["b"])
        counts[sweeps] = mine["iters"]
    print("plain", plain, "ILU(0) exact / 2 / 4 sweeps", counts)
    assert 2 * counts[0] <= plain and 2 * counts[4] <= plain and counts[2] < plain


def test_sample_compiles_with_plain_gxx_and_fails_loudly_without_gpu():
    import subprocess
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_bicgstab")
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 3 and "csr_create" in p.stderr
