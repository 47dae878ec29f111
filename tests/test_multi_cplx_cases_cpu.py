"""Not gpu: the cases of tests/multi_cplx_cases.py are what they claim -- shown with the oracle and the numpy restatement alone, so a
GPU test that passes on them passes for the stated reason.  Each system has the row-block class, fold and partial block its id
names; the restatement of both recurrences equals the oracle (codes, counts, iterates); the columns of a batch sit on both sides of
|m| = 1; both "already optimised" criteria are met by the columns that claim them; helm40 converges where the issue says."""
import numpy as np
import pytest

import multi_cplx_cases as cc


@pytest.mark.parametrize("key", sorted(cc.CLASS), ids=lambda k: f"{k[0]}-{k[1]}")
def test_systems_have_their_class(key):
    S = cc.system(*key)
    R, folded = cc.CLASS[key]
    assert S["R"] == R and (S["blocks"] > cc.MM_MG) == folded, (S["mean"], S["blocks"])
    A = S["A"]
    assert abs(A - A.T).max() == 0.0                            # complex-symmetric ...
    assert abs(A - A.conj().T).max() > 1e-3                     # ... and not Hermitian
    if key[0] != "chain" and key != ("case1kc", 0) and key != cc.HELM40:
        assert S["n"] % R != 0                                  # a partial last block
    if key == ("helm", 182):
        assert S["n"] > 2 * cc.TREE_CAP                         # a thread of a vector pass walks three rows
    if key == ("helm", 363):
        assert S["n"] * 8 >= 2 ** 20


def test_every_class_has_a_folded_and_a_partial_case():
    for R in (64, 16, 4):
        mine = [(S, f) for S, (r, f) in ((cc.system(*key), v) for key, v in cc.CLASS.items()) if r == R]
        assert any(f for _, f in mine), R                                       # more than MM_MG row blocks: the folded d.Ad
        assert any(S["n"] % R != 0 and S["blocks"] > 1 for S, _ in mine), R     # a partial last block behind full ones
        for c in cc.EDGE_CASES:
            assert (c[0], c[1]) in cc.CLASS, c
    assert cc.system("band140", 2051)["blocks"] == cc.MM_MG + 1 and cc.system("band30", 8197)["blocks"] == cc.MM_MG + 1


@pytest.mark.parametrize("sid", cc.SIDS)
@pytest.mark.parametrize("mode", ["capped6", "capped25", "abs", "rel"])
def test_restatement_equals_the_oracle_on_helm40(port, sid, mode):
    S = cc.system(*cc.HELM40)
    para = {"capped6": dict(epsilon=1e-20, max_iterations=6), "capped25": dict(epsilon=1e-20, max_iterations=25),
            "abs": dict(epsilon=1e-10, abs_diff=1), "rel": dict(epsilon=1e-10)}[mode]
    for tag, b in (("b", S["b"]), ("small", cc.SMALL * S["b"])):
        ref = cc.oracle_column(port, S, sid, b, ("cpu", tag), **para)
        mine = cc.restate(sid, S, b, **para)
        assert mine["ret"] == ref["ret"] and mine["iters"] == ref["iters"], (tag, mine["ret"], ref["ret"], mine["iters"], ref["iters"])
        assert np.linalg.norm(mine["x"] - ref["x"]) <= 1e-11 * np.linalg.norm(ref["x"]), tag
        assert abs(mine["residual"] - ref["residual"]) <= 1e-7 * ref["residual"], (tag, mine["residual"], ref["residual"])


def test_helm40_converges_where_the_issue_says(port):
    """The issue's table (its own draw of u and x_true): 27 / 45 iterations under the relative rule, 50 / 76 under abs_diff at
    epsilon = 1e-10.  This module's draw: 24 / 42 and 46 / 75 -- so capped runs of 6 and 25 iterations stop short of convergence
    (their epsilon is 1e-20), and the converged abs_diff runs are long enough to differ between columns."""
    S = cc.system(*cc.HELM40)
    want = {(cc.BICG_SYM, 0): 27, (cc.PCG, 0): 45, (cc.BICG_SYM, 1): 50, (cc.PCG, 1): 76}
    for (sid, ad), its in want.items():
        ref = cc.oracle_column(port, S, sid, S["b"], ("cpu", "b"), epsilon=1e-10, abs_diff=ad)
        print(sid, ad, ref["iters"])
        assert ref["ret"] == cc.CONV and abs(ref["iters"] - its) <= 5, (sid, ad, ref["iters"])


@pytest.mark.parametrize("sid", cc.SIDS)
def test_the_relative_rule_sees_both_sides_of_the_clamp(sid):
    S = cc.system(*cc.HELM40)
    big = cc.restate(sid, S, S["b"], epsilon=1e-10)
    small = cc.restate(sid, S, cc.SMALL * S["b"], epsilon=1e-10)
    assert big["ret"] == small["ret"] == cc.CONV
    assert big["trace"][-1][0] > 100.0 and big["trace"][0][0] == 0.0        # |m|^2 crosses 1 on its way
    assert all(mm < 1.0 for mm, _ in small["trace"])                         # the clamp decides throughout
    assert small["iters"] < big["iters"]                                     # (so one batch holds an early and a late column)


def test_already_optimised_columns_meet_the_criterion_they_claim(port):
    S = cc.system(*cc.HELM40)
    M0, B = cc.already_batch(S)
    para = dict(epsilon=cc.ALREADY_EPS, abs_diff=1)
    got = {sid: [cc.restate(sid, S, B[:, j], m0=M0[:, j], **para) for j in range(4)] for sid in cc.SIDS}
    assert [g["already"] for g in got[cc.BICG_SYM]] == [2, 1, 0, 1]
    assert [g["already"] for g in got[cc.PCG]] == [0, 1, 0, 1]              # |m|^2 takes no part under abs_diff
    for sid in cc.SIDS:
        for j in range(4):
            ref = cc.oracle_column(port, S, sid, B[:, j], ("already", j), m0=M0[:, j], **para)
            assert ref["ret"] == got[sid][j]["ret"] and ref["iters"] == got[sid][j]["iters"], (sid, j)


@pytest.mark.parametrize("case", sorted(cc.EDGE_CASES), ids=lambda c: cc.EDGE_IDS[c])
def test_edge_cases_run_to_their_cap_on_the_oracle(port, case):
    """Capped at 6 the oracle neither converges nor breaks down on any column that is not zero (n <= 3: it converges to rounding in
    at most n iterations, far below any epsilon): the GPU test compares iterates, codes and counts."""
    kind, n, k = case
    S = cc.system(kind, n)
    B = cc.columns(S["n"], S["b"], k)
    for sid in cc.SIDS:
        for j in (0, 1):
            ref = cc.oracle_column(port, S, sid, B[:, j], ("col", j), epsilon=1e-20, max_iterations=6)
            if S["n"] <= 3:
                assert ref["ret"] == cc.CONV and 1 <= ref["iters"] <= S["n"] and ref["residual"] < 1e-25, (sid, j, ref["ret"], ref["iters"], ref["residual"])
            else:
                assert ref["ret"] == cc.MAXIT and ref["iters"] == 6, (sid, j, ref["ret"], ref["iters"])
            assert np.isfinite(ref["x"].view(np.float64)).all()
