"""-m gpu: batched CG and PCG on a dense handle (lcg_hip_dense_lcg_multi, lcg_hip_dense_lpcg_multi) for k = 2, 4, 8: every column
against the oracle's own loop (orc_lcg, orc_lpcg) run on that column alone, fed tests/dense_checker.py's serial-order product and,
as the oracle's own response, numpy's K.T @ (K @ x); then what makes a batch a batch.  Systems, columns and drivers:
tests/dense_multi_cases.py.

Bands (the project's: tests/test_gpu_dense.py, tests/conftest.py: check_converged_run).  Capped at 5 and 20 iterations:
|x - x_oracle| / |x_oracle| <= max(1e-9, 50 x the oracle's serial-against-numpy spread at that count).  Converged (relative rule,
epsilon = 1e-10, cap 600; the oracle must converge): the code equal, the count within max(3, 3 |serial count - numpy count|, 5 %),
the reported residual <= epsilon, the distance to the solution within 10 x the oracle's, and the iterate two short of the earlier
stop within _late_band.  The worst ratio of a difference to its band is printed."""
import numpy as np
import pytest

import dense_multi_cases as mc
from dense_multi_cases import ALREADY, BADCAP, BADEPS, CG, CONV, E_ARG, KS, MAXIT, NANV, NOPRE, PCG, bits, multi, oracle, rel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS, CAP = 1e-10, 600


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
def handles(api):
    """(m, n, normal) -> the dense handle with the Jacobi reciprocals of its operator"""
    made = {}

    def get(m, n, normal=True):
        key = (m, n, normal)
        if key not in made:
            S = mc.system(m, n, normal)
            D = api.DenseMatrix.from_array(S["K"])
            D.build_jacobi(normal)
            made[key] = D
        return made[key]
    yield get
    for D in made.values():
        D.destroy()


def _check_capped(lib, api, D, S, sid, k, cap):
    B = mc.columns(S, k)
    rc, ret, its, res, M = multi(lib, api, sid, D, S["normal"], np.zeros((S["n"], k)), B, epsilon=EPS, max_iterations=cap)
    assert rc == 0, lib.lcg_hip_last_error()
    worst = 0.0
    for j in range(k):
        ref, alt = oracle(S, sid, B[:, j], cap, EPS), oracle(S, sid, B[:, j], cap, EPS, serial=False)
        if not B[:, j].any():
            assert ret[j] == ref["ret"] == ALREADY and its[j] == 0 and not M[:, j].any()
            continue
        band = max(mc.FLOOR, mc.FACTOR * rel(alt["x"], ref["x"]))
        r = rel(M[:, j], ref["x"]); worst = max(worst, r / band)
        print(f"{S['key']} solver {sid} k {k} column {j} cap {cap}: ret {ret[j]} its {its[j]} (oracle {ref['ret']} {ref['iters']}) rel diff {r:.2e} band {band:.2e}")
        assert r <= band, (j, cap, r, band)
        if ref["ret"] == alt["ret"] == MAXIT:
            assert ret[j] == MAXIT and its[j] == cap == ref["iters"], (j, ret[j], its[j])
    return worst


def _check_converged(lib, api, D, S, sid, k):
    B = mc.columns(S, k)
    n = S["n"]
    M0 = np.zeros((n, k))
    zero = [j for j in range(k) if not B[:, j].any()]
    for j in zero:
        M0[:, j] = -0.0         # a guess of zeros that shows a write
    rc, ret, its, res, M = multi(lib, api, sid, D, S["normal"], M0, B, epsilon=EPS, max_iterations=CAP)
    assert rc == 0, lib.lcg_hip_last_error()
    worst, late = 0.0, {}
    for j in range(k):
        if j in zero:
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            continue
        ref, alt = oracle(S, sid, B[:, j], CAP, EPS), oracle(S, sid, B[:, j], CAP, EPS, serial=False)
        assert ref["ret"] == alt["ret"] == CONV, (S["key"], sid, j, "the oracle did not converge", ref["ret"], alt["ret"])
        assert ret[j] == CONV, (j, ret[j])
        dit = abs(ref["iters"] - alt["iters"])
        assert abs(its[j] - ref["iters"]) <= max(3, 3 * dit, 0.05 * ref["iters"]), (j, its[j], ref["iters"], dit)
        assert res[j] <= EPS, (j, res[j])
        xt = mc.solution(S, B[:, j])
        e_gpu, e_ref = np.linalg.norm(M[:, j] - xt), np.linalg.norm(ref["x"] - xt)
        assert e_gpu <= 10.0 * max(e_ref, 1e-14 * np.linalg.norm(xt)), (j, "distance to the solution", e_gpu, e_ref)
        late[j] = (min(its[j], ref["iters"], alt["iters"]) - 2, xt)
        print(f"{S['key']} solver {sid} k {k} column {j}: converged in {its[j]} (oracle {ref['iters']} / {alt['iters']}), residual {res[j]:.2e}, "
              f"distance to the solution {e_gpu:.2e} (oracle {e_ref:.2e})")
    # the iterate two short of the earlier stop: one capped batch per distinct count
    for Kc in sorted({v[0] for v in late.values() if v[0] >= 1}):
        rc, retK, itsK, _, MK = multi(lib, api, sid, D, S["normal"], np.zeros((n, k)), B, epsilon=EPS, max_iterations=Kc)
        assert rc == 0
        for j, (kc, xt) in late.items():
            if kc != Kc:
                continue
            rK, aK = oracle(S, sid, B[:, j], Kc, EPS), oracle(S, sid, B[:, j], Kc, EPS, serial=False)
            assert retK[j] == rK["ret"] == aK["ret"] == MAXIT and itsK[j] == rK["iters"] == aK["iters"] == Kc, (j, Kc, retK[j], rK["ret"], itsK[j])
            band = mc.late_band(rK["x"], aK["x"], xt)
            r = rel(MK[:, j], rK["x"]); worst = max(worst, r / band)
            print(f"   column {j} at {Kc}: rel diff {r:.2e} band {band:.2e}")
            assert r <= band, (j, Kc, r, band)
    return worst


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", [CG, PCG])
def test_main_system_against_the_oracle(lib, api, handles, sid, k):
    S = mc.system(*mc.MAIN)
    D = handles(*mc.MAIN)
    worst = max(_check_capped(lib, api, D, S, sid, k, 5), _check_capped(lib, api, D, S, sid, k, 20), _check_converged(lib, api, D, S, sid, k))
    print(f"worst ratio to a band: {worst:.3g}")


@pytest.mark.parametrize("shape", mc.EDGES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sid", [CG, PCG])
def test_edge_systems_against_the_oracle(lib, api, handles, sid, shape):
    """Vector passes over n k / 2 pieces at 1, 2, 3, 65 and 513 rows; k alternates so that every k meets a tiny and a larger system."""
    S = mc.system(*shape)
    D = handles(*shape)
    worst = 0.0
    for k in (KS if shape[1] <= 3 else (KS[mc.EDGES.index(shape) % 3],)):
        worst = max(worst, _check_capped(lib, api, D, S, sid, k, 5), _check_converged(lib, api, D, S, sid, k))
    print(f"worst ratio to a band: {worst:.3g}")


@pytest.mark.parametrize("sid", [CG, PCG])
def test_square_operator_against_the_oracle(lib, api, handles, sid):
    """normal = 0: A = K itself, K = G^T.G / 200 + I."""
    S = mc.system(200, 200, normal=False)
    D = handles(200, 200, False)
    worst = max(_check_capped(lib, api, D, S, sid, 4, 5), _check_capped(lib, api, D, S, sid, 4, 20), _check_converged(lib, api, D, S, sid, 4))
    print(f"worst ratio to a band: {worst:.3g}")


def _fast_and_slow(S, k):
    """Columns that converge at different counts: column 1 lies in the span of the operator's three dominant eigenvectors."""
    B = mc.columns(S, k)
    K = S["K"]
    w, V = np.linalg.eigh(K.T @ K)
    B[:, 1] = (K.T @ K) @ (V[:, -1] + 0.5 * V[:, -2] + 0.25 * V[:, -3])
    return B


@pytest.mark.parametrize("sid", [CG, PCG])
def test_verdicts_differ_and_stopped_columns_are_final(lib, api, handles, sid):
    S = mc.system(*mc.MAIN)
    D = handles(*mc.MAIN)
    n, k = S["n"], 4
    B = _fast_and_slow(S, k)
    rc, ret, its, res, M = multi(lib, api, sid, D, True, np.zeros((n, k)), B, epsilon=EPS, max_iterations=CAP)
    assert rc == 0 and ret[0] == ret[1] == CONV
    t_fast, t_slow = its[1], its[0]
    print(sid, "counts", its)
    assert 0 < t_fast and t_fast + 2 <= t_slow, its
    cap = (t_fast + t_slow) // 2             # a cap between the two counts: three verdicts in one call
    rc, ret_c, its_c, res_c, M_c = multi(lib, api, sid, D, True, np.zeros((n, k)), B, epsilon=EPS, max_iterations=cap)
    assert rc == 0
    assert ret_c[1] == CONV and its_c[1] == t_fast
    assert ret_c[0] == MAXIT and its_c[0] == cap
    assert ret_c[3] == ALREADY and its_c[3] == 0 and not M_c[:, 3].any()
    assert np.array_equal(bits(M_c[:, 1]), bits(M[:, 1])) and res_c[1] == res[1]
    # frozen means final: the column that converged at t_fast while the others went on = the same B capped at t_fast
    rc, ret_f, its_f, res_f, M_f = multi(lib, api, sid, D, True, np.zeros((n, k)), B, epsilon=EPS, max_iterations=t_fast)
    assert rc == 0 and ret_f[1] == CONV and its_f[1] == t_fast and ret_f[0] == MAXIT and its_f[0] == t_fast
    assert np.array_equal(bits(M_f[:, 1]), bits(M[:, 1])) and res_f[1] == res[1]
    assert lib.lcg_hip_last_iterations() == t_fast


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", [CG, PCG])
def test_a_nan_stays_in_its_column(lib, api, handles, sid, k):
    S = mc.system(*mc.MAIN)
    D = handles(*mc.MAIN)
    n = S["n"]
    B = _fast_and_slow(S, k)
    para = dict(epsilon=EPS, max_iterations=40)
    rc, ret, its, res, M = multi(lib, api, sid, D, True, np.zeros((n, k)), B, **para)
    Bn = B.copy(); Bn[n // 2, 1] = np.nan
    rc_n, ret_n, its_n, res_n, M_n = multi(lib, api, sid, D, True, np.zeros((n, k)), Bn, **para)
    assert rc == 0 and rc_n == 0
    assert ret_n[1] == NANV and its_n[1] == 1
    for j in range(k):
        if j == 1:
            continue
        assert ret_n[j] == ret[j] and its_n[j] == its[j] and res_n[j] == res[j], j
        assert np.array_equal(bits(M_n[:, j]), bits(M[:, j])), j
        assert np.isfinite(M_n[:, j]).all()


@pytest.mark.parametrize("sid", [CG, PCG])
@pytest.mark.parametrize("shape", [mc.MAIN, (7, 3), (600, 513)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_independence_memory_and_guesses(lib, api, handles, shape, sid):
    """Column j: the same bits at k = 2, 4, 8, with other neighbours, at another position, from host or device memory and from
    call to call; from a non-zero guess within the capped band of the oracle started from that guess."""
    S = mc.system(*shape)
    D = handles(*shape)
    n = S["n"]
    para = dict(epsilon=EPS, max_iterations=30)
    rng = np.random.default_rng(8)
    B8 = mc.columns(S, 8)
    M8 = np.zeros((n, 8)); M8[:, 1] = rng.standard_normal(n); M8[:, 2] = 0.5 * S["xt"]
    r8 = multi(lib, api, sid, D, True, M8, B8, **para)
    assert r8[0] == 0
    for again in (multi(lib, api, sid, D, True, M8, B8, **para), multi(lib, api, sid, D, True, M8, B8, mem="host", **para)):
        assert again[0] == 0 and again[1:4] == r8[1:4] and np.array_equal(bits(again[4]), bits(r8[4]))
    for k, picks in ((2, (0, 1)), (2, (2, 5)), (4, (4, 2, 1, 7)), (4, (3, 0, 6, 2)), (8, (7, 6, 5, 4, 3, 2, 1, 0))):
        B = np.ascontiguousarray(B8[:, picks]); M = np.ascontiguousarray(M8[:, picks])
        r = multi(lib, api, sid, D, True, M, B, **para)
        assert r[0] == 0
        for pos, j in enumerate(picks):
            assert (r[1][pos], r[2][pos], r[3][pos]) == (r8[1][j], r8[2][j], r8[3][j]), (k, pos, j)
            assert np.array_equal(bits(r[4][:, pos]), bits(r8[4][:, j])), (k, pos, j)
    # other neighbours: huge, zero, NaN
    B = B8[:, :4].copy(); M = M8[:, :4].copy()
    B[:, 0] = rng.standard_normal(n) * 1e3; B[:, 2] = 0.0; M[:, 2] = 0.0; B[0, 3] = np.nan
    r = multi(lib, api, sid, D, True, M, B, **para)
    assert r[0] == 0 and (r[1][1], r[2][1], r[3][1]) == (r8[1][1], r8[2][1], r8[3][1]) and np.array_equal(bits(r[4][:, 1]), bits(r8[4][:, 1]))
    # the non-zero guesses against the oracle from the same guess
    for j in (1, 2):
        cap = 20
        rc, ret, its, res, Mc = multi(lib, api, sid, D, True, M8[:, :4], B8[:, :4], epsilon=EPS, max_iterations=cap)
        ref = oracle(S, sid, B8[:, j], cap, EPS, m0=M8[:, j]); alt = oracle(S, sid, B8[:, j], cap, EPS, serial=False, m0=M8[:, j])
        band = max(mc.FLOOR, mc.FACTOR * rel(alt["x"], ref["x"]))
        assert rc == 0 and rel(Mc[:, j], ref["x"]) <= band, (j, rel(Mc[:, j], ref["x"]), band)


def test_error_returns(lib, api, handles):
    S = mc.system(*mc.MAIN)
    D = handles(*mc.MAIN)
    n, k = S["n"], 4
    B = mc.columns(S, k)
    Z = np.zeros((n, k))
    good = dict(epsilon=EPS, max_iterations=10)
    ref = multi(lib, api, CG, D, True, Z, B, **good)
    assert ref[0] == 0

    def still_works():
        r = multi(lib, api, CG, D, True, Z, B, **good)
        assert r[0] == 0 and r[1:4] == ref[1:4] and np.array_equal(bits(r[4]), bits(ref[4]))

    rp = np.arange(n + 1, dtype=np.int32); ci = np.arange(n, dtype=np.int32)
    A = api.CsrMatrix.from_csr(rp, ci, np.ones(n))
    Dc = api.DenseMatrix.from_array(np.eye(n) + 0j)
    bare = api.DenseMatrix.from_array(S["K"])                  # no diagonal
    sq = api.DenseMatrix.from_array(np.eye(n) * 2.0)
    for sid in (CG, PCG):
        name = "lcg_hip_dense_lpcg_multi" if sid == PCG else "lcg_hip_dense_lcg_multi"
        for h, why in ((A, "not a dense matrix"), (Dc, "complex")):
            r = multi(lib, api, sid, h, True, Z, B, **good)
            assert r[0] == E_ARG and r[1] == [99] * k, (sid, why)
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and why in err, err
        r = multi(lib, api, sid, D, False, Z, B, **good)       # normal = 0 on a 300 x 240 matrix
        assert r[0] == E_ARG and "square" in lib.lcg_hip_last_error().decode()
        assert multi(lib, api, sid, D, True, Z, B, epsilon=0.0)[0] == BADEPS
        assert multi(lib, api, sid, D, True, Z, B, epsilon=1.0)[0] == BADEPS
        assert multi(lib, api, sid, D, True, Z, B, epsilon=EPS, max_iterations=-1)[0] == BADCAP
        still_works()
    # PCG: no diagonal, or the other operator's
    assert multi(lib, api, PCG, bare, True, Z, B, **good)[0] == NOPRE
    assert multi(lib, api, CG, bare, True, Z, B, **good)[0] == 0           # plain CG needs none
    sq.build_jacobi(True)
    assert multi(lib, api, PCG, sq, False, Z, B, **good)[0] == NOPRE       # built for K^T.K, asked for K
    assert multi(lib, api, PCG, sq, True, Z, B, **good)[0] == 0
    sq.build_jacobi(False)
    assert multi(lib, api, PCG, sq, True, Z, B, **good)[0] == NOPRE
    assert multi(lib, api, PCG, sq, False, Z, B, **good)[0] == 0
    still_works()
    for h in (A, Dc, bare, sq):
        h.destroy()


def test_python_front(api, handles):
    S = mc.system(*mc.MAIN)
    D = handles(*mc.MAIN)
    n = S["n"]
    B = torch.from_numpy(mc.columns(S, 4)).cuda()
    M = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    infos = api.dense_lpcg_multi(D, M, B, api.lcg_default_parameters(epsilon=EPS, abs_diff=0, max_iterations=CAP))
    assert [i.ret for i in infos] == [CONV, CONV, CONV, ALREADY] and infos[3].iterations == 0
    Y = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda")
    D.ata_multi(M, Y)
    api.synchronize()
    r = (Y - B).cpu().numpy()
    assert np.linalg.norm(r[:, 0]) <= 1e-4 * np.linalg.norm(B[:, 0].cpu().numpy())
    Mh = np.zeros((n, 4))
    infos_h = api.dense_lcg_multi(D, Mh, B.cpu().numpy(), api.lcg_default_parameters(epsilon=EPS, abs_diff=0, max_iterations=CAP))
    assert [i.ret for i in infos_h] == [CONV, CONV, CONV, ALREADY]
    assert np.linalg.norm(Mh[:, 0] - M[:, 0].cpu().numpy()) <= 1e-4 * np.linalg.norm(Mh[:, 0])


def test_sample_program_solves_eight_data_vectors():
    import subprocess
    from test_dropin_cpp import _build
    exe = _build("sample_dense_multi")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "one lcg_hip_dense_lcg_multi, iterations:" in p.stdout


def test_launches_are_reported(lib, api, handles):
    """lcg_hip_last_launches after 10 iterations on the 300 x 240 system: the operator is the row form (one launch: 120
    packs per row are not split), the column form with its fold (two) and the k-wide sum (one) -- four kernels per iteration, three
    for the setup's product, which carries no sum -- and there are two vector passes per iteration and for the setup."""
    import ctypes as C
    S = mc.system(*mc.MAIN)
    D = handles(*mc.MAIN)
    for sid in (CG, PCG):
        rc, ret, its, _, _ = multi(lib, api, sid, D, True, np.zeros((S["n"], 8)), mc.columns(S, 8), epsilon=EPS, max_iterations=10)
        assert rc == 0 and its[0] == 10
        vec, prod = C.c_int(), C.c_int()
        lib.lcg_hip_last_launches(C.byref(vec), None, None, C.byref(prod))
        assert (prod.value, vec.value) == (3 + 10 * 4, 2 + 10 * 2), (prod.value, vec.value)
        assert D.multi_last_kernel == "k_dnm_ata_two_pass"
