"""-m gpu: batched PCG with the handle's IC(0) / ILU(0) factor as M (lcg_hip_lpcg_multi_m) for k = 2, 4, 8 on case_10K_A and the
40 x 40 Laplacian, exact applies and 2 / 4 sweeps: every column against ic0_checker.lpcg run on that column alone with the matching
checker apply (ic0_checker.IcApply, ic0_sweeps_checker.SweepApply, ilu0_checker.IluApply / SweepApply -- what the single-vector
IC(0) / ILU(0) PCG tests hold the library to); then what makes a batch a batch, the Jacobi forwarding, n.k >= 2^20, R = 16, the error
returns, the Python front and the example program.

Bands: tests/test_gpu_multi_solvers.py's own.  Capped at 25 iterations: code and count equal, |x - x_ref| <= max(1e-9, 50 x the
checker's response to 1-ulp changes of b) |x_ref|, residual to 1e-9 relative.  Converged (abs_diff = 1, epsilon = 1e-10): count
within 3, distance <= 1e-9, reported residual <= epsilon."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import multi_cases as MC
import tri_multi_cases as T
from test_gpu_multi_solvers import columns, fast_and_slow

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CONV, ALREADY, MAXIT, NANV, NOPRE, BADEPS, BADIT, E_ARG = 0, 2, -1019, -1017, -1018, -1021, -1022, -2003
KS = T.KS
SWEEPS = (0, 2, 4)


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
def systems(api, case10k):
    """name -> (n, rowptr, col, val, b, handle holding the Jacobi diagonal, an IC(0) and an ILU(0) factor)"""
    n, rp, ci, v, b, _ = case10k
    out = {"case10k": (n, rp, ci, v, b)}
    Tm = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(40, 40))
    L = (sp.kron(sp.identity(40), Tm) + sp.kron(Tm, sp.identity(40))).tocsr(); L.sort_indices()
    xt = np.random.default_rng(40).standard_normal(1600)
    out["laplace40"] = (1600, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.copy(), L @ xt)
    full = {}
    for name, (n, rp, ci, v, b) in out.items():
        A = api.CsrMatrix.from_csr(rp, ci, v)
        A.build_jacobi(); A.build_ic0(); A.build_ilu0()
        full[name] = (n, rp, ci, v, b, A)
    yield full
    for s in full.values():
        s[5].destroy()


def column_tag(k, j):
    """columns(n, b, 2) is columns 0 and 2 of the longer batches: one name per distinct column, so that the checker's runs are shared."""
    return (0, 2)[j] if k == 2 else j


def run(lib, api, factor, sweeps, A, M0, B, **para):
    T.set_sweeps(A, factor, sweeps)
    return T.multi_m(lib, api, T.PRECOND[factor], A, M0, B, **para)


def checker(name, sysd, factor, sweeps, bcol, tag, **para):
    return T.checker_column(factor, name, sysd[:4], sweeps, bcol, tag, para["epsilon"], para["abs_diff"], para.get("max_iterations", 0))


# ------------------------------------------------------------------------------------------ 1. every column against the checker
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sweeps", SWEEPS)
@pytest.mark.parametrize("factor", T.FACTORS)
@pytest.mark.parametrize("name", ["case10k", "laplace40"])
def test_capped_at_25_iterations(lib, api, systems, name, factor, sweeps, k):
    n, rp, ci, v, b, A = systems[name]
    B = columns(n, b, k)
    para = dict(epsilon=1e-20, abs_diff=1, max_iterations=25)
    rc, ret, its, res, M = run(lib, api, factor, sweeps, A, np.zeros((n, k)), B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        tag = column_tag(k, j)
        ref = checker(name, systems[name], factor, sweeps, B[:, j], ("col", tag), **para)
        print(name, factor, sweeps, k, j, "ret", ret[j], ref["ret"], "its", its[j], ref["iters"])
        assert ret[j] == ref["ret"] and its[j] == ref["iters"], (j, ret[j], ref["ret"], its[j], ref["iters"])
        if not B[:, j].any():
            assert ret[j] == ALREADY and its[j] == 0 and not M[:, j].any()
            continue
        assert ret[j] == MAXIT and its[j] == 25
        nx = np.linalg.norm(ref["x"])
        sens = max(np.linalg.norm(checker(name, systems[name], factor, sweeps,
                                          B[:, j] * (1.0 + 1e-16 * np.random.default_rng(1000 + s).standard_normal(n)),
                                          ("pert", tag, s), **para)["x"] - ref["x"]) / nx for s in range(2))
        d = np.linalg.norm(M[:, j] - ref["x"]) / nx
        print("   distance", d, "checker's response", sens, "residual", res[j], ref["residual"])
        assert d <= max(1e-9, 50.0 * sens), (j, d, sens)
        assert abs(res[j] - ref["residual"]) <= 1e-9 * ref["residual"], (j, res[j], ref["residual"])
    assert lib.lcg_hip_last_iterations() == 25
    # what the solve enqueued: per body (and for the set-up) one product, three vector passes and the apply's launches
    vec, prod = C.c_int(), C.c_int()
    lib.lcg_hip_last_launches(C.byref(vec), None, None, C.byref(prod))
    L = T.info(A, factor)["launches"]
    assert prod.value == 26 and vec.value == 26 * (3 + L), (vec.value, prod.value, L)
    if sweeps:
        assert L == (2 * sweeps if factor == "ic0" else max(sweeps - 1, 1) + sweeps)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sweeps", SWEEPS)
@pytest.mark.parametrize("factor", T.FACTORS)
@pytest.mark.parametrize("name", ["case10k", "laplace40"])
def test_converged_columns_match_the_checker(lib, api, systems, name, factor, sweeps, k):
    n, rp, ci, v, b, A = systems[name]
    B = columns(n, b, k)
    eps = 1e-10
    para = dict(epsilon=eps, abs_diff=1)
    M0 = np.zeros((n, k))
    zero = [j for j in range(k) if not B[:, j].any()]
    for j in zero:
        M0[:, j] = -0.0         # a guess of zeros that shows a write
    rc, ret, its, res, M = run(lib, api, factor, sweeps, A, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        ref = checker(name, systems[name], factor, sweeps, B[:, j], ("col", column_tag(k, j)), **para)
        print(name, factor, sweeps, k, j, "ret", ret[j], ref["ret"], "its", its[j], ref["iters"], "residual", res[j])
        if j in zero:
            assert ret[j] == ref["ret"] == ALREADY and its[j] == 0
            assert np.array_equal(T.bits(M[:, j]), T.bits(M0[:, j]))                # untouched, sign bits included
            continue
        assert ret[j] == ref["ret"] == CONV
        assert abs(its[j] - ref["iters"]) <= 3, (j, its[j], ref["iters"])
        d = np.linalg.norm(M[:, j] - ref["x"]) / np.linalg.norm(ref["x"])
        print("   distance", d)
        assert d <= 1e-9, (j, d)
        assert res[j] <= eps, (j, res[j])
    longest = int(np.argmax(its))
    assert lib.lcg_hip_last_iterations() == its[longest] and lib.lcg_hip_last_residual() == res[longest]


def test_converged_under_the_relative_rule(lib, api, systems):
    """abs_diff = 0: the residual is r.r / max(m.m, 1), and for the 1e-6 b column m.m stays below 1 (clamp1 decides)."""
    name, factor, sweeps, k = "laplace40", "ic0", 2, 4
    n, rp, ci, v, b, A = systems[name]
    B = MC.columns(n, b, k)                                 # b, 1e-6 b, a random vector, zeros
    para = dict(MC.RULES["rel"])
    rc, ret, its, res, M = run(lib, api, factor, sweeps, A, np.zeros((n, k)), B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        ref = checker(name, systems[name], factor, sweeps, B[:, j], ("rel", j), **para)
        print("rel", j, "ret", ret[j], ref["ret"], "its", its[j], ref["iters"], "residual", res[j], ref["residual"])
        if j == 3:
            assert ret[j] == ALREADY and its[j] == 0
            continue
        assert ret[j] == ref["ret"] == CONV and abs(its[j] - ref["iters"]) <= 3, (j, its[j], ref["iters"])
        assert np.linalg.norm(M[:, j] - ref["x"]) <= 1e-9 * np.linalg.norm(ref["x"]), j
        assert res[j] <= para["epsilon"]
    assert float(M[:, 1] @ M[:, 1]) < 1.0 < float(M[:, 0] @ M[:, 0])
    assert its[1] < its[0]                                  # judged against max(m.m, 1) = 1, the small column stops earlier


# ------------------------------------------------------------------------------------------ 2. in a batch
@pytest.mark.parametrize("sweeps", [0, 2])
@pytest.mark.parametrize("factor", T.FACTORS)
def test_verdicts_differ_and_stopped_columns_are_final(lib, api, systems, factor, sweeps):
    n, rp, ci, v, b, A = systems["case10k"]
    k = 4
    B = fast_and_slow(n, b, k)
    para = dict(epsilon=1e-10, abs_diff=1)
    rc, ret, its, res, M = run(lib, api, factor, sweeps, A, np.zeros((n, k)), B, **para)
    assert rc == 0 and ret[0] == ret[1] == CONV
    t_fast, t_slow = its[1], its[0]
    print(factor, sweeps, "counts", its)
    assert 0 < t_fast and t_fast + 2 <= t_slow, its
    cap = (t_fast + t_slow) // 2                            # a cap between the two counts: both verdicts in one call
    rc, ret_c, its_c, res_c, M_c = run(lib, api, factor, sweeps, A, np.zeros((n, k)), B, max_iterations=cap, **para)
    assert rc == 0
    assert ret_c[1] == CONV and its_c[1] == t_fast
    assert ret_c[0] == MAXIT and its_c[0] == cap
    assert ret_c[3] == ALREADY and its_c[3] == 0
    assert np.array_equal(T.bits(M_c[:, 1]), T.bits(M[:, 1])) and res_c[1] == res[1]
    # frozen means final: the column that converged at t_fast while the others went on = the same B capped at t_fast
    rc, ret_f, its_f, res_f, M_f = run(lib, api, factor, sweeps, A, np.zeros((n, k)), B, max_iterations=t_fast, **para)
    assert rc == 0 and ret_f[1] == CONV and its_f[1] == t_fast and ret_f[0] == MAXIT and its_f[0] == t_fast
    assert np.array_equal(T.bits(M_f[:, 1]), T.bits(M[:, 1])) and res_f[1] == res[1]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sweeps", [0, 2])
@pytest.mark.parametrize("factor", T.FACTORS)
def test_a_nan_stays_in_its_column(lib, api, systems, factor, sweeps, k):
    n, rp, ci, v, b, A = systems["case10k"]
    B = fast_and_slow(n, b, k)
    para = dict(epsilon=1e-10, abs_diff=1, max_iterations=40)
    rc, ret, its, res, M = run(lib, api, factor, sweeps, A, np.zeros((n, k)), B, **para)
    Bn = B.copy(); Bn[n // 2, 1] = np.nan
    rc_n, ret_n, its_n, res_n, M_n = run(lib, api, factor, sweeps, A, np.zeros((n, k)), Bn, **para)
    assert rc == 0 and rc_n == 0
    assert ret_n[1] == NANV and its_n[1] == 1
    for j in range(k):
        if j == 1:
            continue
        assert ret_n[j] == ret[j] and its_n[j] == its[j] and res_n[j] == res[j], j
        assert np.array_equal(T.bits(M_n[:, j]), T.bits(M[:, j])), j
        assert np.isfinite(M_n[:, j]).all()


@pytest.mark.parametrize("sweeps", [0, 2])
@pytest.mark.parametrize("factor", T.FACTORS)
@pytest.mark.parametrize("name", ["case10k", "laplace40"])
def test_independence_and_repeatability(lib, api, systems, name, factor, sweeps):
    n, rp, ci, v, b, A = systems[name]
    k = 4
    B = columns(n, b, k)
    para = dict(epsilon=1e-10, abs_diff=1, max_iterations=30)
    r1 = run(lib, api, factor, sweeps, A, np.zeros((n, k)), B, **para)
    r2 = run(lib, api, factor, sweeps, A, np.zeros((n, k)), B, **para)
    r3 = run(lib, api, factor, sweeps, A, np.zeros((n, k)), B, mem="host", **para)
    for r in (r2, r3):
        assert r[0] == r1[0] == 0 and r[1:4] == r1[1:4]
        assert np.array_equal(T.bits(r[4]), T.bits(r1[4]))
    # other neighbours
    B2 = B.copy()
    rng = np.random.default_rng(8)
    B2[:, 1] = rng.standard_normal(n) * 1e3; B2[:, 2] = 0.0; B2[:, 3] = 1e-6 * b
    M2 = np.zeros((n, k)); M2[:, 1] = rng.standard_normal(n)
    r4 = run(lib, api, factor, sweeps, A, M2, B2, **para)
    assert r4[0] == 0 and (r4[1][0], r4[2][0], r4[3][0]) == (r1[1][0], r1[2][0], r1[3][0])
    assert np.array_equal(T.bits(r4[4][:, 0]), T.bits(r1[4][:, 0]))
    # the same columns in another order (the same k: a column's sums are added in an order that k fixes)
    perm = [2, 0, 3, 1]
    r5 = run(lib, api, factor, sweeps, A, np.zeros((n, k)), np.ascontiguousarray(B[:, perm]), **para)
    assert r5[0] == 0
    for jn, jo in enumerate(perm):
        assert (r5[1][jn], r5[2][jn], r5[3][jn]) == (r1[1][jo], r1[2][jo], r1[3][jo]), (jn, jo)
        assert np.array_equal(T.bits(r5[4][:, jn]), T.bits(r1[4][:, jo])), (jn, jo)


# ------------------------------------------------------------------------------------------ 3. Jacobi forwarding
@pytest.mark.parametrize("k", KS)
def test_jacobi_is_lpcg_multi_itself(lib, api, systems, k):
    n, rp, ci, v, b, A = systems["case10k"]
    B = fast_and_slow(n, b, k)
    for para in (dict(epsilon=1e-10, abs_diff=1), dict(epsilon=1e-20, abs_diff=1, max_iterations=25)):
        old = MC.multi(lib, api, MC.PCG, A, np.zeros((n, k)), B, **para)
        new = T.multi_m(lib, api, T.M_JACOBI, A, np.zeros((n, k)), B, **para)
        assert old[0] == new[0] == 0 and old[1:4] == new[1:4], (old[1:4], new[1:4])
        assert np.array_equal(T.bits(old[4]), T.bits(new[4]))


# ------------------------------------------------------------------------------------------ 4. other branches
def _tridiagonal(n):
    i = np.arange(n)
    off = -1.0 + 0.2 * np.sin(0.05 * i[:-1])
    d = 3.0 + 0.5 * np.cos(0.01 * i)
    A = sp.diags([off, d, off], [-1, 0, 1], format="csr"); A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def test_work_of_two_to_the_twenty(lib, api):
    """n = 131,072 at k = 8: n.k = 2^20, so six bodies are in flight and the mapped mirror is refreshed every iteration
    (pub_mask = 0); 512 row blocks of 256, 2048 workgroups of the 8-wide sweep."""
    n, k, sweeps = 131072, 8, 2
    rp, ci, v = _tridiagonal(n)
    As = sp.csr_matrix((v, ci, rp), shape=(n, n))
    b = As @ np.sin(0.001 * np.arange(n))
    B = MC.columns(n, b, k)
    para = dict(epsilon=1e-20, abs_diff=1, max_iterations=10)
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ic0()
        r1 = run(lib, api, "ic0", sweeps, A, np.zeros((n, k)), B, **para)
        r2 = run(lib, api, "ic0", sweeps, A, np.zeros((n, k)), B, **para)
        assert r1[0] == r2[0] == 0 and r1[1:4] == r2[1:4] and np.array_equal(T.bits(r1[4]), T.bits(r2[4]))
        assert r1[1] == [MAXIT, MAXIT, MAXIT, ALREADY, MAXIT, MAXIT, MAXIT, MAXIT] and r1[2] == [10, 10, 10, 0, 10, 10, 10, 10]
        # column 0 against the checker (the checker's factor and sweeps of 131,072 rows take seconds: one column, one perturbed run)
        key, sysd, j = "tri131072", (n, rp, ci, v), 0
        ref = T.checker_column("ic0", key, sysd, sweeps, B[:, j], ("col", j), 1e-20, 1, 10)
        assert ref["ret"] == MAXIT and ref["iters"] == 10
        nx = np.linalg.norm(ref["x"])
        pert = T.checker_column("ic0", key, sysd, sweeps, B[:, j] * (1.0 + 1e-16 * np.random.default_rng(1000).standard_normal(n)),
                                ("pert", j), 1e-20, 1, 10)
        sens = np.linalg.norm(pert["x"] - ref["x"]) / nx
        d = np.linalg.norm(r1[4][:, j] - ref["x"]) / nx
        print("2^20 column", j, "distance", d, "checker's response", sens, "residual", r1[3][j], ref["residual"])
        assert d <= max(1e-9, 50.0 * sens), (j, d, sens)
        assert abs(r1[3][j] - ref["residual"]) <= 1e-9 * ref["residual"], j
        # columns 4, 6, 7 are -b, 0.5 b, 2 b: the recurrence is linear in b up to rounding
        for jj, f in ((4, -1.0), (6, 0.5), (7, 2.0)):
            assert np.linalg.norm(r1[4][:, jj] - f * r1[4][:, 0]) <= 1e-9 * abs(f) * nx, jj
    finally:
        A.destroy()


def test_sixteen_rows_per_block(lib, api):
    """multi_cases' band30 system: the product runs at R = 16 rows per block, the factor's rows hold about 31 entries."""
    S = MC.system("band30", 1029)
    assert S["R"] == 16
    n, k = S["n"], 4
    B = MC.columns(n, S["b"], k)
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    try:
        A.build_ic0(); A.build_ilu0()
        for factor, sweeps in (("ic0", 2), ("ilu0", 4)):
            para = dict(epsilon=1e-10, abs_diff=1)
            rc, ret, its, res, M = run(lib, api, factor, sweeps, A, np.zeros((n, k)), B, **para)
            assert rc == 0, lib.lcg_hip_last_error()
            for j in range(k):
                ref = T.checker_column(factor, "band30", (n, S["rp"], S["ci"], S["v"]), sweeps, B[:, j], ("col", j), 1e-10, 1)
                print("band30", factor, sweeps, j, ret[j], its[j], ref["iters"], res[j])
                if j == 3:
                    assert ret[j] == ALREADY and its[j] == 0
                    continue
                assert ret[j] == ref["ret"] == CONV and abs(its[j] - ref["iters"]) <= 3, (j, its[j], ref["iters"])
                assert np.linalg.norm(M[:, j] - ref["x"]) <= 1e-9 * np.linalg.norm(ref["x"]), j
                assert res[j] <= 1e-10
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 5. error returns
def test_error_returns_release_the_solver(lib, api, systems, case10k, case1kc):
    n, rp, ci, v, b, A = systems["case10k"]
    k = 4
    B = columns(n, b, k)
    good = dict(epsilon=1e-10, abs_diff=1, max_iterations=10)
    ref = run(lib, api, "ic0", 2, A, np.zeros((n, k)), B, **good)
    assert ref[0] == 0

    def still_works():
        r = run(lib, api, "ic0", 2, A, np.zeros((n, k)), B, **good)
        assert r[0] == 0 and r[1:4] == ref[1:4] and np.array_equal(T.bits(r[4]), T.bits(ref[4]))

    for precond in (3, -1, 99):
        r = T.multi_m(lib, api, precond, A, np.zeros((n, k)), B, **good)
        assert r[0] == E_ARG and r[1] == [99] * k and "precond" in lib.lcg_hip_last_error().decode()
        assert np.array_equal(r[4], np.zeros((n, k)))
        still_works()
    bare = api.CsrMatrix.from_csr(rp, ci, v)                # no factor, no Jacobi diagonal
    for precond in (T.M_JACOBI, T.M_IC0, T.M_ILU0):
        r = T.multi_m(lib, api, precond, bare, np.zeros((n, k)), B, **good)
        assert r[0] == NOPRE and r[1] == [99] * k           # nothing ran, nothing was reported
    bare.build_ic0()                                        # the other factor is still missing
    assert T.multi_m(lib, api, T.M_ILU0, bare, np.zeros((n, k)), B, **good)[0] == NOPRE
    assert T.multi_m(lib, api, T.M_IC0, bare, np.zeros((n, k)), B, **good)[0] == 0
    bare.destroy()
    still_works()
    # a factor on a handle of another type
    nc, rpc, cic, vc = case1kc[:4]
    Ac = api.CsrMatrix.from_csr(rpc, cic, vc)
    Ac.build_ic0()
    r = T.multi_m(lib, api, T.M_IC0, Ac, np.zeros((nc, k)), np.ones((nc, k)), **good)
    assert r[0] == E_ARG and "complex" in lib.lcg_hip_last_error().decode()
    Ac.destroy()
    still_works()
    for factor in T.FACTORS:
        assert run(lib, api, factor, 2, A, np.zeros((n, k)), B, epsilon=0.0)[0] == BADEPS
        still_works()
        assert run(lib, api, factor, 2, A, np.zeros((n, k)), B, epsilon=1.0)[0] == BADEPS
        assert run(lib, api, factor, 2, A, np.zeros((n, k)), B, max_iterations=-1)[0] == BADIT
        still_works()
    # the single-vector path beside it
    m = np.zeros(n)
    T.set_sweeps(A, "ic0", 2)
    info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", None, m, b, n,
                                         api.lcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=10), A)
    assert info.ret == MAXIT and info.iterations == 10
    assert np.linalg.norm(m - ref[4][:, 0]) <= 1e-9 * np.linalg.norm(m)        # column 0 is b: the same recurrence, other sums


# ------------------------------------------------------------------------------------------ 6. front ends
def test_python_front(api, systems):
    n, rp, ci, v, b, A = systems["laplace40"]
    B = torch.from_numpy(columns(n, b, 4)).cuda()
    para = api.lcg_default_parameters(epsilon=1e-10, abs_diff=1)
    A.ic0_set_sweeps(4); A.ilu0_set_sweeps(0)
    counts = {}
    for precond in ("jacobi", "ic0", "ilu0"):
        M = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
        infos = api.lpcg_multi(A, M, B, para, precond=precond)
        assert [i.ret for i in infos] == [CONV, CONV, CONV, ALREADY] and infos[3].iterations == 0
        Y = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda")
        A.spmm(M, Y)
        api.synchronize()
        r = (Y - B).cpu().numpy()
        assert np.linalg.norm(r[:, 0]) / n <= 2e-10, precond
        counts[precond] = infos[0].iterations
    print("iterations of column 0:", counts)
    assert counts["ilu0"] <= counts["ic0"] < counts["jacobi"]       # the exact factor, 4 sweeps of it, the diagonal
    M = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    assert [i.iterations for i in api.lpcg_multi(A, M, B, para)][0] == counts["jacobi"]    # the old call signature
    with pytest.raises(ValueError):
        api.lpcg_multi(A, M, B, para, precond="ssor")
    # the batched apply through the front: z = M^-1 B, column by column the single apply
    Z = torch.zeros_like(B)
    A.ic0_solve_multi(B, Z)
    z0 = torch.zeros(n, dtype=torch.float64, device="cuda")
    A.ic0_solve(B[:, 0].contiguous(), z0)
    api.synchronize()
    assert np.array_equal(T.bits(Z[:, 0].cpu().numpy()), T.bits(z0.cpu().numpy()))
    Mh = np.zeros((n, 4))
    infos_h = api.lpcg_multi(A, Mh, B.cpu().numpy(), para, precond="ic0")
    assert [i.ret for i in infos_h] == [CONV, CONV, CONV, ALREADY]


def test_sample_program_solves_four_right_hand_sides():
    from conftest import ROOT
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_ic0")
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = re.findall(r"^column (\d): ret=(-?\d+) iterations=(\d+) residual=\S+ true_residual=(\S+)", p.stdout, flags=re.M)
    assert [(int(j), int(r)) for j, r, _, _ in got] == [(0, CONV), (1, CONV), (2, CONV), (3, ALREADY)]
    assert all(float(t) <= 2e-10 for _, _, _, t in got)
    # 4 sweeps of IC(0): a third of Jacobi's 181 iterations, never more than half
    assert 20 <= int(got[0][2]) <= 90 and int(got[3][2]) == 0
