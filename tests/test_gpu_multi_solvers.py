"""-m gpu: batched CG and PCG (lcg_hip_lcg_multi, lcg_hip_lpcg_multi) for k = 2, 4, 8 on case_10K_A and a 40 x 40 Laplacian, every
column against the oracle's run of that column alone; then what makes a batch a batch: different verdicts in one call, a NaN that
stays in its column, stopped columns that are final, columns that do not depend on their neighbours, and the error returns.

Bands.  Capped at 25 iterations: conftest.check_converged_run's band for a capped iterate of a recurrence that IS the oracle's
(max(floor 1e-9, 50 x the oracle's own response to 1-ulp changes of b at that count)), without its third term (a quarter of the
error left), which 25 iterations into a solve would allow anything.  Converged (abs_diff = 1, epsilon = 1e-10): SURVEY section 8c's
parity statement per column -- count within 3 of the oracle's, |x - x_oracle| <= 1e-9 |x_oracle|, reported residual <= epsilon.

These two systems run the loops at R = 64 rows per block, without the fold, in one stride of a vector pass and under abs_diff = 1
only.  The other branches -- the relative rule and m.m, the folded d.Ad, R = 16 and R = 4, a second stride, n.k >= 2^20, n = 1, 2, 3,
non-zero guesses, both "already optimised" criteria -- are pinned by tests/test_gpu_multi_edges.py on the systems of
tests/multi_cases.py, which also holds the driver multi()."""
import numpy as np
import pytest
import scipy.sparse as sp

from multi_cases import multi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CONV, ALREADY, MAXIT, NANV, NOPRE, BADEPS, E_ARG = 0, 2, -1019, -1017, -1018, -1021, -2003
CG, PCG = 0, 1
KS = (2, 4, 8)


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
    """name -> (n, rowptr, col, val, b, handle with its Jacobi diagonal)"""
    n, rp, ci, v, b, _ = case10k
    out = {"case10k": (n, rp, ci, v, b)}
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(40, 40))
    L = (sp.kron(sp.identity(40), T) + sp.kron(T, sp.identity(40))).tocsr(); L.sort_indices()
    xt = np.random.default_rng(40).standard_normal(1600)
    out["laplace40"] = (1600, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.copy(), L @ xt)
    full = {}
    for name, (n, rp, ci, v, b) in out.items():
        A = api.CsrMatrix.from_csr(rp, ci, v)
        A.build_jacobi()
        full[name] = (n, rp, ci, v, b, A)
    yield full
    for s in full.values():
        s[5].destroy()


def columns(n, b, k):
    """The right-hand sides of a batch: for k = 4 {b, 2 b, a seeded random vector, 0}."""
    r = np.random.default_rng(77)
    cols = [b, 2.0 * b, r.standard_normal(n), np.zeros(n), -b, r.standard_normal(n) * 3.0, 0.5 * b, b]
    if k == 2:
        cols = [cols[0], cols[2]]
    return np.ascontiguousarray(np.stack(cols[:k], axis=1))


_ORACLE = {}


def oracle(port, name, sysd, sid, bcol, tag, **para):
    """The oracle's run of one column alone (cached per system, solver, column and parameters)."""
    from oracle import pyoracle as po
    key = (name, sid, tag, tuple(sorted(para.items())))
    if key not in _ORACLE:
        n, rp, ci, v = sysd[:4]
        _ORACLE[key] = port.solve(sid, rp, ci, v, bcol, para=po.default_para(**para), jacobi=(sid == PCG))
    return _ORACLE[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", [CG, PCG])
@pytest.mark.parametrize("name", ["case10k", "laplace40"])
def test_capped_at_25_iterations(lib, api, port, systems, name, sid, k):
    n, rp, ci, v, b, A = systems[name]
    B = columns(n, b, k)
    para = dict(epsilon=1e-20, abs_diff=1, max_iterations=25)
    rc, ret, its, res, M = multi(lib, api, sid, A, np.zeros((n, k)), B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        ref = oracle(port, name, systems[name], sid, B[:, j], ("col", k, j), **para)
        print(name, sid, k, j, "ret", ret[j], ref["ret"], "its", its[j], ref["iters"])
        assert ret[j] == ref["ret"] and its[j] == ref["iters"], (j, ret[j], ref["ret"], its[j], ref["iters"])
        if not B[:, j].any():
            assert ret[j] == ALREADY and its[j] == 0 and not M[:, j].any()
            continue
        assert ret[j] == MAXIT and its[j] == 25
        nx = np.linalg.norm(ref["x"])
        sens = max(np.linalg.norm(oracle(port, name, systems[name], sid,
                                         B[:, j] * (1.0 + 1e-16 * np.random.default_rng(1000 + s).standard_normal(n)),
                                         ("pert", k, j, s), **para)["x"] - ref["x"]) / nx for s in range(2))
        d = np.linalg.norm(M[:, j] - ref["x"]) / nx
        print("   distance", d, "oracle's response", sens, "residual", res[j], ref["residual"])
        assert d <= max(1e-9, 50.0 * sens), (j, d, sens)
        assert abs(res[j] - ref["residual"]) <= 1e-9 * ref["residual"], (j, res[j], ref["residual"])
    assert lib.lcg_hip_last_iterations() == 25


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", [CG, PCG])
@pytest.mark.parametrize("name", ["case10k", "laplace40"])
def test_converged_columns_match_the_oracle(lib, api, port, systems, name, sid, k):
    n, rp, ci, v, b, A = systems[name]
    B = columns(n, b, k)
    eps = 1e-10
    para = dict(epsilon=eps, abs_diff=1)
    M0 = np.zeros((n, k))
    zero = [j for j in range(k) if not B[:, j].any()]
    for j in zero:
        M0[:, j] = -0.0         # a guess of zeros that shows a write: -0 + a d would come back as +0
    rc, ret, its, res, M = multi(lib, api, sid, A, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        ref = oracle(port, name, systems[name], sid, B[:, j], ("col", k, j), **para)
        print(name, sid, k, j, "ret", ret[j], ref["ret"], "its", its[j], ref["iters"], "residual", res[j])
        if j in zero:
            assert ret[j] == ref["ret"] == ALREADY and its[j] == 0
            assert np.array_equal(bits(M[:, j]), bits(M0[:, j]))            # untouched, sign bits included
            continue
        assert ret[j] == ref["ret"] == CONV
        assert abs(its[j] - ref["iters"]) <= 3, (j, its[j], ref["iters"])
        d = np.linalg.norm(M[:, j] - ref["x"]) / np.linalg.norm(ref["x"])
        print("   distance", d)
        assert d <= 1e-9, (j, d)
        assert res[j] <= eps, (j, res[j])
    longest = int(np.argmax(its))
    assert lib.lcg_hip_last_iterations() == its[longest] and lib.lcg_hip_last_residual() == res[longest]
    # the same zero column with a plain +0 guess
    rc, ret2, its2, _, M2 = multi(lib, api, sid, A, np.zeros((n, k)), B, **para)
    assert rc == 0 and ret2 == ret and its2 == its
    for j in zero:
        assert np.array_equal(bits(M2[:, j]), bits(np.zeros(n)))


def fast_and_slow(n, b, k):
    """Columns that converge at different counts under abs_diff = 1: column 1 is b scaled down (its gradient starts near the bound)."""
    B = columns(n, b, k)
    B[:, 1] = 1e-6 * b
    return B


@pytest.mark.parametrize("sid", [CG, PCG])
@pytest.mark.parametrize("name", ["case10k", "laplace40"])
def test_verdicts_differ_and_stopped_columns_are_final(lib, api, systems, name, sid):
    n, rp, ci, v, b, A = systems[name]
    k = 4
    B = fast_and_slow(n, b, k)
    para = dict(epsilon=1e-10, abs_diff=1)
    rc, ret, its, res, M = multi(lib, api, sid, A, np.zeros((n, k)), B, **para)
    assert rc == 0 and ret[0] == ret[1] == CONV
    t_fast, t_slow = its[1], its[0]
    print(name, sid, "counts", its)
    assert 0 < t_fast and t_fast + 2 <= t_slow, its
    # a cap between the two counts: both verdicts in one call
    cap = (t_fast + t_slow) // 2
    rc, ret_c, its_c, res_c, M_c = multi(lib, api, sid, A, np.zeros((n, k)), B, max_iterations=cap, **para)
    assert rc == 0
    assert ret_c[1] == CONV and its_c[1] == t_fast
    assert ret_c[0] == MAXIT and its_c[0] == cap
    assert ret_c[3] == ALREADY and its_c[3] == 0
    assert np.array_equal(bits(M_c[:, 1]), bits(M[:, 1])) and res_c[1] == res[1]
    # frozen means final: the column that converged at t_fast while the others went on = the same B capped at t_fast
    rc, ret_f, its_f, res_f, M_f = multi(lib, api, sid, A, np.zeros((n, k)), B, max_iterations=t_fast, **para)
    assert rc == 0 and ret_f[1] == CONV and its_f[1] == t_fast and ret_f[0] == MAXIT and its_f[0] == t_fast
    assert np.array_equal(bits(M_f[:, 1]), bits(M[:, 1])) and res_f[1] == res[1]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", [CG, PCG])
def test_a_nan_stays_in_its_column(lib, api, systems, sid, k):
    n, rp, ci, v, b, A = systems["case10k"]
    B = fast_and_slow(n, b, k)
    para = dict(epsilon=1e-10, abs_diff=1, max_iterations=60)
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


@pytest.mark.parametrize("sid", [CG, PCG])
@pytest.mark.parametrize("name", ["case10k", "laplace40"])
def test_independence_and_repeatability(lib, api, systems, name, sid):
    n, rp, ci, v, b, A = systems[name]
    k = 4
    B = columns(n, b, k)
    para = dict(epsilon=1e-10, abs_diff=1, max_iterations=40)
    r1 = multi(lib, api, sid, A, np.zeros((n, k)), B, **para)
    r2 = multi(lib, api, sid, A, np.zeros((n, k)), B, **para)
    r3 = multi(lib, api, sid, A, np.zeros((n, k)), B, mem="host", **para)
    for r in (r2, r3):
        assert r[0] == r1[0] == 0 and r[1:4] == r1[1:4]
        assert np.array_equal(bits(r[4]), bits(r1[4]))
    B2 = B.copy()
    rng = np.random.default_rng(8)
    B2[:, 1] = rng.standard_normal(n) * 1e3; B2[:, 2] = 0.0; B2[:, 3] = 1e-6 * b
    M2 = np.zeros((n, k)); M2[:, 1] = rng.standard_normal(n)
    r4 = multi(lib, api, sid, A, M2, B2, **para)
    assert r4[0] == 0 and (r4[1][0], r4[2][0], r4[3][0]) == (r1[1][0], r1[2][0], r1[3][0])
    assert np.array_equal(bits(r4[4][:, 0]), bits(r1[4][:, 0]))


def test_error_returns_release_the_solver(lib, api, systems, case10k):
    n, rp, ci, v, b, A = systems["case10k"]
    k = 4
    B = columns(n, b, k)
    good = dict(epsilon=1e-10, abs_diff=1, max_iterations=10)
    ref = multi(lib, api, CG, A, np.zeros((n, k)), B, **good)
    assert ref[0] == 0

    def still_works():
        r = multi(lib, api, CG, A, np.zeros((n, k)), B, **good)
        assert r[0] == 0 and r[1:4] == ref[1:4] and np.array_equal(bits(r[4]), bits(ref[4]))
        m = np.zeros(n)
        info = api.lcg_solver("lcg_hip_csr_ax", None, m, b, n, api.lcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=10), A, api.LCG_CG)
        assert info.ret == MAXIT and info.iterations == 10

    bare = api.CsrMatrix.from_csr(rp, ci, v)            # no Jacobi diagonal
    r = multi(lib, api, PCG, bare, np.zeros((n, k)), B, **good)
    assert r[0] == NOPRE and r[1] == [99] * k           # nothing ran, nothing was reported
    still_works()
    assert multi(lib, api, CG, bare, np.zeros((n, k)), B, **good)[0] == 0          # plain CG needs no diagonal
    bare.destroy()
    for sid in (CG, PCG):
        assert multi(lib, api, sid, A, np.zeros((n, k)), B, epsilon=0.0)[0] == BADEPS
        still_works()
        assert multi(lib, api, sid, A, np.zeros((n, k)), B, epsilon=1.0)[0] == BADEPS
        assert multi(lib, api, sid, A, np.zeros((n, k)), B, max_iterations=-1)[0] == -1022
        still_works()


def test_python_front(api, systems):
    n, rp, ci, v, b, A = systems["laplace40"]
    B = torch.from_numpy(columns(n, b, 4)).cuda()
    M = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    infos = api.lpcg_multi(A, M, B, api.lcg_default_parameters(epsilon=1e-10, abs_diff=1))
    assert [i.ret for i in infos] == [CONV, CONV, CONV, ALREADY] and infos[3].iterations == 0
    Y = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda")
    A.spmm(M, Y)
    api.synchronize()
    r = (Y - B).cpu().numpy()
    assert np.linalg.norm(r[:, 0]) / n <= 2e-10
    Mh = np.zeros((n, 4))
    infos_h = api.lcg_multi(A, Mh, B.cpu().numpy(), api.lcg_default_parameters(epsilon=1e-10, abs_diff=1))
    assert [i.ret for i in infos_h] == [CONV, CONV, CONV, ALREADY]
    assert np.linalg.norm(Mh[:, 0] - M[:, 0].cpu().numpy()) <= 1e-8 * np.linalg.norm(Mh[:, 0])


def test_sample_program_solves_four_right_hand_sides():
    import os
    import re
    import subprocess
    from conftest import ROOT
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi")
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = re.findall(r"^column (\d): ret=(-?\d+) iterations=(\d+)", p.stdout, flags=re.M)
    assert [(int(j), int(r)) for j, r, _ in got] == [(0, CONV), (1, CONV), (2, CONV), (3, ALREADY)]
    assert abs(int(got[0][2]) - 181) <= 3 and int(got[3][2]) == 0      # PCG 181 on the real liblcg
