"""-m gpu: the batched CG and PCG loops (lcg_hip_lcg_multi, lcg_hip_lpcg_multi) at every size class, under both stop rules and at
the edges, on the systems of tests/multi_cases.py (tests/test_multi_cases_cpu.py shows with the oracle alone that each case is what
its id says).  Each case (system, n, k) is the smallest that reaches its branch:

  tiny / edge        n = 1, 2, 3 (a pass of n k / 2 pieces; columns that converge exactly after n iterations or are "already
                     optimised" by the second criterion) and n = 65, 513 (one wavefront + 1, two workgroups + 1 of pieces at k = 2)
  stride2            n k / 2 > 512 * 256: k_mvecf walks a second stride
  fold_r64/r16/r4    513 row blocks: d.Ad goes through k_mm_fold inside the loop, with the product's live stop pointer
  r16_partial_block  R = 16 in the loop, 5 rows in the last block;  fold_r4: R = 4, 3 rows in the last block
  work_2p20          n k >= 2^20: the host status is published every iteration and the host runs 6 bodies ahead

Every case runs CG and PCG under abs_diff = 0, epsilon = 1e-14 (the residual is g.g / max(m.m, 1): the running sum m.m and its
clamp decide the reported residual and the stop) and under abs_diff = 1, epsilon = 1e-10.

Bands.  Six capped iterations: the iterate within max(CAPPED_ITERATES_RTOL = 1e-13, 50 x the oracle's own response to 1-ulp changes
of b at that count) of the oracle's, relative to |x|; the reported residual within 1e-9 of the oracle's (test_capped_at_25_iterations'
band) AND within 1e-9 of the host's recomputation from the returned iterate in extended precision (multi_cases.host_residual), which
shares nothing with the device's sums.  Three places where that statement cannot be made, and what is asserted instead: a column at
n <= 3 that has converged inside the cap reports the rounding residue of an exact zero (each side its own: <= epsilon on both); a
guess that is the solution to rounding (0.5 xt for 0.5 b) is "already optimised" with a residual that is rounding alone (both below
multi_cases.rounding_floor); and for a run from a guess the oracle's response is measured to 1-ulp changes of b AND of the guess (1 ulp of 1e-6 b vanishes in
A.m0 - b for a guess of size 1, so b alone would give a response of exactly 0).  Converged runs: conftest.check_converged_run per column with late=True (the batched
schedule is the classic one).

Measured on one MI355X (distance of the six-iteration iterate to the oracle's, relative to |x|, the largest over columns, solvers
and rules; every test prints its own): band30 at 1029 rows 3.4e-16, at 8197 rows 5.2e-16, band140 at 2051 rows 6.7e-16 -- the
long-row cases sit three orders below the 1e-13 floor.  From a guess (column 1, a random guess for 1e-6 b, where the iterate is a
small difference of large numbers): 1.8e-13 ... 1.1e-11 against 50 x responses of 3.7e-12 ... 8.8e-11."""
import numpy as np
import pytest

import multi_cases as mc
from conftest import check_converged_run
from multi_cases import ALREADY, CG, CONV, MAXIT, NANV, PCG, bits, multi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CAP = 6
RESIDUAL_RTOL = 1e-9
CASES = list(mc.EDGE_CASES)
CASE_IDS = [mc.EDGE_IDS[c] for c in CASES]
GUESS_CASES = [("tiny", 3, 4), ("spd", 513, 4), ("band30", 1029, 8), ("band140", 2051, 2)]      # one k per system class
SOLVERS = pytest.mark.parametrize("sid", [CG, PCG], ids=["cg", "pcg"])
RULES = pytest.mark.parametrize("rule", sorted(mc.RULES))


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def handle(api):
    """(kind, n) -> (system, handle with its Jacobi diagonal), built once per module."""
    made = {}

    def get(kind, n):
        if (kind, n) not in made:
            S = mc.system(kind, n)
            assert (S["R"], S["blocks"] > mc.MM_MG) == mc.CLASS[(kind, n)], (kind, n, S["mean"], S["blocks"])
            A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
            A.build_jacobi()
            made[(kind, n)] = (S, A)
        return made[(kind, n)]
    yield get
    for _, A in made.values():
        A.destroy()


def _tol():
    from test_gpu_fuzz_solvers import CAPPED_ITERATES_RTOL
    return CAPPED_ITERATES_RTOL


def _perturbed(b, s):
    return b * (1.0 + 1e-16 * np.random.default_rng(1000 + s).standard_normal(len(b)))


def capped_walk(lib, api, port, S, A, sid, rule, k, M0, guess):
    """Six capped iterations of one batch against the oracle's run of every column alone (module docstring)."""
    n = S["n"]
    B = mc.columns(n, S["b"], k)
    para = dict(mc.RULES[rule], max_iterations=CAP)
    rc, ret, its, res, M = multi(lib, api, sid, A, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    worst = 0.0
    for j in range(k):
        ref = mc.oracle_column(port, S, sid, B[:, j], (guess, "col", j), m0=M0[:, j], **para)
        print(S["key"], sid, rule, k, j, "ret", ret[j], ref["ret"], "its", its[j], ref["iters"], "residual", res[j], ref["residual"])
        assert ret[j] == ref["ret"] and its[j] == ref["iters"], (j, ret[j], ref["ret"], its[j], ref["iters"])
        if ret[j] == ALREADY:
            assert its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j])), j
        elif ret[j] == MAXIT:
            assert its[j] == CAP
        else:
            assert ret[j] == CONV and 0 < its[j] <= CAP      # the oracle's own verdict, earlier than the cap
        nx = np.linalg.norm(ref["x"])
        if nx > 0.0:
            # (a run from a guess: the guess is input as b is -- |A.m0 - b| swallows 1 ulp of a small b whole -- and moves by 1 ulp too)
            sens = max(np.linalg.norm(mc.oracle_column(port, S, sid, _perturbed(B[:, j], s), (guess, "pert", j, s),
                                                       m0=_perturbed(M0[:, j], 1000 + s) if guess else M0[:, j], **para)["x"] - ref["x"]) / nx
                       for s in range(2))
            d = np.linalg.norm(M[:, j] - ref["x"]) / nx
            worst = max(worst, d)
            print("   distance", d, "oracle's response", sens)
            assert d <= max(_tol(), 50.0 * sens), (j, d, sens)
        else:
            assert not M[:, j].any()
        if ret[j] == ALREADY and max(res[j], ref["residual"]) <= mc.rounding_floor(S, M0[:, j], B[:, j], para["abs_diff"]):
            continue        # the guess is the solution to rounding: the residual is each side's own rounding (multi_cases.rounding_floor)
        if n <= 3 and ret[j] == CONV:
            # n iterations span the whole space: g is what rounding left of an exact zero, on either side its own (n = 1: the oracle's
            # g + a Ad is 0.0, the device's fused multiply-add leaves 2.8e-16), and lies below the rounding of A.m - b
            assert 0.0 <= res[j] <= para["epsilon"] and ref["residual"] <= para["epsilon"], (j, res[j], ref["residual"])
            continue
        assert abs(res[j] - ref["residual"]) <= RESIDUAL_RTOL * ref["residual"], (j, res[j], ref["residual"])
        host, g2, m2 = mc.host_residual(S, M[:, j], B[:, j], para["abs_diff"], para["epsilon"] if ret[j] == ALREADY else None)
        print("   host residual", host, "g.g", g2, "m.m", m2)
        assert abs(res[j] - host) <= RESIDUAL_RTOL * host, (j, res[j], host, g2, m2)
    assert lib.lcg_hip_last_iterations() == max(its)
    print(S["key"], sid, rule, k, "largest distance", worst)


@RULES
@SOLVERS
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_six_capped_iterations_walk_the_oracle(lib, api, port, handle, case, sid, rule):
    kind, n, k = case
    S, A = handle(kind, n)
    capped_walk(lib, api, port, S, A, sid, rule, k, np.zeros((n, k)), "")


def converged_columns(lib, api, port, S, A, sid, rule, k, M0, guess):
    """A batch run to convergence, column by column through conftest.check_converged_run (late=True: the classic schedule); the
    columns that are "already optimised" (a zero column from a zero guess; 1e-6 b at n <= 3 under abs_diff = 1) against the
    oracle's verdict, untouched."""
    n = S["n"]
    B = mc.columns(n, S["b"], k)
    para = mc.RULES[rule]
    sols = mc.solutions(S["xt"], k)
    runs = {}

    def batch(cap):
        if cap not in runs:
            rc, ret, its, res, M = multi(lib, api, sid, A, M0, B, max_iterations=cap, **para)
            assert rc == 0, lib.lcg_hip_last_error()
            runs[cap] = (ret, its, res, M)
        return runs[cap]

    ret, its, res, M = batch(0)
    print(S["key"], sid, rule, k, "ret", ret, "its", its)
    longest = int(np.argmax(its))
    assert lib.lcg_hip_last_iterations() == its[longest] and lib.lcg_hip_last_residual() == res[longest]
    for j in range(k):
        ref = mc.oracle_column(port, S, sid, B[:, j], (guess, "col", j), m0=M0[:, j], **para)
        if ref["ret"] == ALREADY:
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j])), j
            if max(res[j], ref["residual"]) > mc.rounding_floor(S, M0[:, j], B[:, j], para["abs_diff"]):
                assert abs(res[j] - ref["residual"]) <= RESIDUAL_RTOL * ref["residual"], (j, res[j], ref["residual"])
            continue

        class Port:     # the oracle's run of THIS column from its guess (check_converged_run hands over b and the cap)
            @staticmethod
            def solve(sid_, rp, ci, v, b, para=None, jacobi=False):
                return port.solve(sid_, rp, ci, v, b, m0=M0[:, j], para=para, jacobi=jacobi)

        def solve_gpu(cap):
            r = batch(cap)
            return r[0][j], r[1][j], r[2][j], np.ascontiguousarray(r[3][:, j])
        check_converged_run(Port, solve_gpu, sid, S["rp"], S["ci"], S["v"], np.ascontiguousarray(B[:, j]), para["epsilon"], para["abs_diff"],
                            jacobi=(sid == PCG), tag=(S["key"], sid, rule, k, j), xt=sols[j], late=True)


@RULES
@SOLVERS
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_converged_columns(lib, api, port, handle, case, sid, rule):
    kind, n, k = case
    S, A = handle(kind, n)
    converged_columns(lib, api, port, S, A, sid, rule, k, np.zeros((n, k)), "")


@RULES
@SOLVERS
@pytest.mark.parametrize("case", GUESS_CASES, ids=[f"{c[0]}-{c[1]}-k{c[2]}" for c in GUESS_CASES])
def test_a_block_of_guesses(lib, api, port, handle, case, sid, rule):
    """Column 0 from zeros, column 1 from a random guess, the others from half the solution: against the oracle's m0 runs."""
    kind, n, k = case
    S, A = handle(kind, n)
    M0 = mc.guesses(S, k)
    capped_walk(lib, api, port, S, A, sid, rule, k, M0, "guess")
    converged_columns(lib, api, port, S, A, sid, rule, k, M0, "guess")


@SOLVERS
def test_both_already_optimised_criteria_in_one_batch(lib, api, port, handle, sid):
    """abs_diff = 1 tries sqrt(g.g) / n and then g.g / max(m.m, 1) (lcg.cpp:178-203): column 0 stops by the second with that
    residual, column 1 by the first, column 2 runs, column 3 is b = 0 from a guess of -0.0."""
    S, A = handle("spd", 65)
    n = S["n"]
    M0, B = mc.already_batch(S)
    para = dict(abs_diff=1, epsilon=mc.ALREADY_EPS)
    rc, ret, its, res, M = multi(lib, api, sid, A, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    ref = [mc.oracle_column(port, S, sid, B[:, j], ("already", j), m0=M0[:, j], **para) for j in range(4)]
    print("ret", ret, [r["ret"] for r in ref], "its", its, [r["iters"] for r in ref], "residual", res, [r["residual"] for r in ref])
    assert ret == [r["ret"] for r in ref] == [ALREADY, ALREADY, CONV, ALREADY]
    assert its == [r["iters"] for r in ref] and its[0] == its[1] == its[3] == 0
    for j in (0, 1, 3):
        assert np.array_equal(bits(M[:, j]), bits(M0[:, j])), j         # untouched, the sign of -0.0 included
    host, g2, m2 = mc.host_residual(S, M0[:, 0], B[:, 0], 1, para["epsilon"])
    assert np.sqrt(g2) / n > para["epsilon"] and host == g2 / max(m2, 1.0)
    assert abs(res[0] - ref[0]["residual"]) <= RESIDUAL_RTOL * ref[0]["residual"] and abs(res[0] - host) <= RESIDUAL_RTOL * host
    assert 0.0 <= res[1] <= mc.rounding_floor(S, M0[:, 1], B[:, 1], 1) <= para["epsilon"]      # g = A.xt - b is rounding alone, each side's own
    assert abs(res[2] - ref[2]["residual"]) <= RESIDUAL_RTOL * ref[2]["residual"] and res[2] <= para["epsilon"]
    assert np.linalg.norm(M[:, 2] - ref[2]["x"]) <= 1e-9 * np.linalg.norm(ref[2]["x"])
    assert res[3] == 0.0
    assert lib.lcg_hip_last_iterations() == its[2] and lib.lcg_hip_last_residual() == res[2]


@RULES
@SOLVERS
@pytest.mark.parametrize("n", [32771, 131075])
def test_frozen_means_final_where_the_host_runs_ahead(lib, api, handle, n, sid, rule):
    """Columns that stop at different counts while the host enqueues bodies ahead (24, and 6 at n k >= 2^20): a column that stopped at
    t in the converged run is, bit for bit, that column of the same batch capped at t."""
    S, A = handle("spd", n)
    k = 8
    B = mc.columns(n, S["b"], k)
    para = mc.RULES[rule]
    Z = np.zeros((n, k))
    rc, ret, its, res, M = multi(lib, api, sid, A, Z, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    print(n, sid, rule, "ret", ret, "counts", its)
    assert ret == [CONV, CONV, CONV, ALREADY, CONV, CONV, CONV, CONV]
    counts = sorted({t for t in its if t > 0})
    assert len(counts) >= 3 and counts[0] + 2 <= counts[-1], its
    for t in counts:
        rc, ret_c, its_c, res_c, M_c = multi(lib, api, sid, A, Z, B, max_iterations=t, **para)
        assert rc == 0
        for j in range(k):
            if its[j] <= t:     # stopped by then: final
                assert (ret_c[j], its_c[j], res_c[j]) == (ret[j], its[j], res[j]), (t, j)
                assert np.array_equal(bits(M_c[:, j]), bits(M[:, j])), (t, j)
            else:
                assert (ret_c[j], its_c[j]) == (MAXIT, t), (t, j, ret_c[j], its_c[j])
    cap = counts[len(counts) // 2]
    r1 = multi(lib, api, sid, A, Z, B, max_iterations=cap, **para)
    r2 = multi(lib, api, sid, A, Z, B, max_iterations=cap, **para)
    r3 = multi(lib, api, sid, A, Z, B, mem="host", max_iterations=cap, **para)
    for r in (r2, r3):
        assert r[0] == r1[0] == 0 and r[1:4] == r1[1:4]
        assert np.array_equal(bits(r[4]), bits(r1[4]))


@SOLVERS
@pytest.mark.parametrize("case", [("spd", 32771, 4), ("band140", 2051, 2)], ids=["spd-32771-k4-fold_r64", "band140-2051-k2-fold_r4"])
def test_a_nan_stays_in_its_column_at_the_folded_size(lib, api, handle, case, sid):
    kind, n, k = case
    S, A = handle(kind, n)
    B = mc.columns(n, S["b"], k)
    para = dict(mc.RULES["abs"], max_iterations=60)
    rc, ret, its, res, M = multi(lib, api, sid, A, np.zeros((n, k)), B, **para)
    Bn = B.copy(); Bn[n // 2, 1] = np.nan
    rc_n, ret_n, its_n, res_n, M_n = multi(lib, api, sid, A, np.zeros((n, k)), Bn, **para)
    assert rc == 0 and rc_n == 0
    assert ret_n[1] == NANV and its_n[1] == 1
    for j in range(k):
        if j == 1:
            continue
        assert ret_n[j] == ret[j] and its_n[j] == its[j] and res_n[j] == res[j], j
        assert np.array_equal(bits(M_n[:, j]), bits(M[:, j])), j
        assert np.isfinite(M_n[:, j]).all()
    assert ret[0] == CONV
