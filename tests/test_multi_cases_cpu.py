"""The cases of tests/multi_cases.py are what they claim, shown with the oracle alone (no GPU): every system lies in its class of
rows_per_block and on its side of the 512-block fold; every column of every batch gets the verdict the GPU tests count on under
both stop rules, in 1 ... 60 iterations where it runs; both sides of clamp1 are present in every batch; the oracle's own reported
residual is the host's recomputation from its iterate (tests/test_gpu_multi_edges.py asks the same of the device); and the batch
multi_cases.already_batch stops where it should, each column by the criterion it is there for."""
import numpy as np
import pytest

import multi_cases as mc

SYSTEMS = sorted(mc.CLASS)
SYSTEM_IDS = [f"{kind}-{n}" for kind, n in SYSTEMS]


@pytest.mark.parametrize("kind,n", SYSTEMS, ids=SYSTEM_IDS)
def test_row_length_class_and_block_count(kind, n):
    S = mc.system(kind, n)
    R, folded = mc.CLASS[(kind, n)]
    print(kind, n, "nnz/n", S["mean"], "R", S["R"], "blocks", S["blocks"])
    assert {64: S["mean"] <= 48.0, 16: 48.0 < S["mean"] <= 256.0, 4: S["mean"] > 256.0}[R], (kind, n, S["mean"])
    assert S["R"] == R and S["blocks"] == -(-n // R)
    assert (S["blocks"] > mc.MM_MG) == folded, (kind, n, S["blocks"])
    if folded and n < 65539:
        assert S["blocks"] == mc.MM_MG + 1              # the smallest folded size of its class
    if kind != "tiny":
        assert n % R != 0                               # a partial last block
    # symmetric, with a dominant diagonal
    import scipy.sparse as sp
    A = sp.csr_matrix((S["v"], S["ci"], S["rp"]), shape=(n, n))
    assert abs(A - A.T).max() == 0.0 if n > 1 else True
    d = A.diagonal()
    assert np.all(d > (abs(A).sum(axis=1).A1 - d))


def test_band140_at_515_rows_is_not_the_r4_class():
    rp, _, _ = mc.band_pattern(515, 140)
    assert 48.0 < rp[-1] / 515 <= 256.0


def test_the_cases_reach_their_branches():
    for (kind, n, k), why in mc.EDGE_CASES.items():
        S = mc.system(kind, n)
        pieces = n * k // 2
        assert ("stride2" in why) == (pieces > mc.STRIDE), (kind, n, k, pieces)
        assert ("2p20" in why) == (n * k >= 1 << 20), (kind, n, k)
        assert ("fold" in why or n >= 65539) == (S["blocks"] > mc.MM_MG), (kind, n, k)
        for R in (64, 16, 4):
            if f"r{R}" in why:
                assert S["R"] == R
    # a wavefront edge and a workgroup edge of the pieces: k = 2 at n = 65 is 65 pieces, at n = 513 it is 513; k = 8 makes a row four
    assert ("spd", 65, 2) in mc.EDGE_CASES and ("spd", 513, 2) in mc.EDGE_CASES and ("tiny", 1, 8) in mc.EDGE_CASES


@pytest.mark.parametrize("rule", sorted(mc.RULES))
@pytest.mark.parametrize("sid", [mc.CG, mc.PCG], ids=["cg", "pcg"])
@pytest.mark.parametrize("kind,n", SYSTEMS, ids=SYSTEM_IDS)
def test_oracle_verdicts_and_counts(port, kind, n, sid, rule):
    S = mc.system(kind, n)
    para = mc.RULES[rule]
    B = mc.columns(n, S["b"], 8)
    counts = []
    for j in range(8):
        r = mc.oracle_column(port, S, sid, B[:, j], ("col", j), **para)
        counts.append(r["iters"])
        if not B[:, j].any():
            assert (r["ret"], r["iters"], r["residual"]) == (mc.ALREADY, 0, 0.0)
        elif j == 1 and kind == "tiny" and rule == "abs":
            # sqrt(g.g) / n = 1e-6 |b| / n > 1e-10, g.g / max(m.m, 1) = 1e-12 |b|^2 <= 1e-10: the second criterion
            g2 = float(B[:, j] @ B[:, j])
            assert np.sqrt(g2) / n > para["epsilon"] and g2 <= para["epsilon"]
            assert (r["ret"], r["iters"]) == (mc.ALREADY, 0) and abs(r["residual"] - g2) <= 1e-12 * g2
        else:
            assert r["ret"] == mc.CONV, (kind, n, sid, rule, j, r["ret"])
            assert 1 <= r["iters"] <= 60, (kind, n, sid, rule, j, r["iters"])
            assert r["residual"] <= para["epsilon"]
        # clamp1: column 0 ends with |m|^2 well above 1, column 1 with |m|^2 below 1
        if j == 0:
            assert r["x"] @ r["x"] >= 4.0
        if j == 1:
            assert r["x"] @ r["x"] < 1e-6
    print(kind, n, "cg" if sid == mc.CG else "pcg", rule, "oracle counts", counts)


# the oracle's counts for column b, ((CG, PCG) under abs_diff = 0, (CG, PCG) under abs_diff = 1), measured when the cases were chosen
COUNTS = {("spd", 65): ((22, 15), (26, 18)), ("spd", 513): ((25, 17), (30, 21)), ("spd", 32771): ((23, 15), (25, 17)),
          ("spd", 131075): ((22, 15), (23, 15)), ("band30", 1029): ((18, 12), (21, 15)), ("band30", 8197): ((18, 12), (20, 14)),
          ("band140", 2051): ((17, 12), (20, 14))}


@pytest.mark.parametrize("kind,n", sorted(COUNTS), ids=[f"{k}-{n}" for k, n in sorted(COUNTS)])
def test_oracle_counts_of_column_b_stay_small(port, kind, n):
    """Every solve of these cases ends in under 35 iterations (the counts measured when the cases were chosen, for the stencil
    system exactly; the band's values are this module's own draw, so its counts are held to the same small window)."""
    S = mc.system(kind, n)
    for ri, rule in enumerate(("rel", "abs")):
        got = tuple(mc.oracle_column(port, S, sid, S["b"], ("col", 0), **mc.RULES[rule])["iters"] for sid in (mc.CG, mc.PCG))
        print(kind, n, rule, "CG / PCG", got, "table", COUNTS[(kind, n)][ri])
        if kind == "spd":
            assert got == COUNTS[(kind, n)][ri]
        else:
            assert all(abs(g - w) <= 3 for g, w in zip(got, COUNTS[(kind, n)][ri])), (got, COUNTS[(kind, n)][ri])
        assert max(got) < 35


@pytest.mark.parametrize("rule", sorted(mc.RULES))
@pytest.mark.parametrize("sid", [mc.CG, mc.PCG], ids=["cg", "pcg"])
@pytest.mark.parametrize("kind,n", SYSTEMS, ids=SYSTEM_IDS)
def test_oracle_capped_residual_is_the_hosts_recomputation(port, kind, n, sid, rule):
    """Six iterations in, the residual the loop reports (from its recurrence's g or r) is the residual of its iterate (g = A.m - b
    in extended precision) to 1e-9 -- for every column the cap stops and for the columns that stopped before it; at n <= 3 a column
    has converged EXACTLY by then and reports a recurrence's g that lies below the rounding of A.m - b: those are left out."""
    S = mc.system(kind, n)
    para = dict(mc.RULES[rule], max_iterations=6)
    B = mc.columns(n, S["b"], 8)
    for j in range(8):
        r = mc.oracle_column(port, S, sid, B[:, j], ("col", j), **para)
        if n <= 3 and r["ret"] == mc.CONV:
            continue
        assert r["ret"] in (mc.MAXIT, mc.CONV, mc.ALREADY) and r["iters"] <= 6
        host, g2, m2 = mc.host_residual(S, r["x"], B[:, j], para["abs_diff"], para["epsilon"] if r["ret"] == mc.ALREADY else None)
        print(kind, n, sid, rule, j, "reported", r["residual"], "host", host, "m.m", m2)
        assert abs(r["residual"] - host) <= 1e-9 * host, (kind, n, sid, rule, j, r["residual"], host)


def test_both_already_optimised_criteria(port):
    S = mc.system("spd", 65)
    M0, B = mc.already_batch(S)
    eps = mc.ALREADY_EPS
    n = S["n"]
    for sid in (mc.CG, mc.PCG):
        r = [mc.oracle_column(port, S, sid, B[:, j], ("already", j), m0=M0[:, j], abs_diff=1, epsilon=eps) for j in range(4)]
        # column 0: the second criterion, with the residual g.g / max(m.m, 1)
        _, g2, m2 = mc.host_residual(S, M0[:, 0], B[:, 0], 1)
        print("sqrt(g.g)/n", np.sqrt(g2) / n, "g.g/m.m", g2 / m2, "oracle", r[0]["residual"])
        assert np.sqrt(g2) / n > eps and g2 / max(m2, 1.0) <= eps
        assert (r[0]["ret"], r[0]["iters"]) == (mc.ALREADY, 0)
        assert abs(r[0]["residual"] - g2 / max(m2, 1.0)) <= 1e-9 * r[0]["residual"]
        assert np.array_equal(mc.bits(r[0]["x"]), mc.bits(M0[:, 0]))
        # column 1: the first
        assert (r[1]["ret"], r[1]["iters"]) == (mc.ALREADY, 0) and r[1]["residual"] <= eps
        assert (r[2]["ret"] == mc.CONV) and 1 <= r[2]["iters"] <= 60
        assert (r[3]["ret"], r[3]["iters"], r[3]["residual"]) == (mc.ALREADY, 0, 0.0)
