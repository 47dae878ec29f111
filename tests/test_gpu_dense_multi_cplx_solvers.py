"""-m gpu: batched complex BiCG-sym and PCG on a complex128 dense handle (clcg_hip_dense_lbicg_sym_multi,
clcg_hip_dense_lpcg_multi) for k = 2, 4, 8: every column against the oracle's own loop (orc_clbicg_symmetric, orc_clpcg) run on that
column alone, fed tests/dense_checker.py's serial-order product and, as the oracle's own response, numpy's K @ x; then what makes a
batch a batch.  Systems, columns and drivers: tests/dense_multi_cplx_cases.py (tests/test_dense_multi_cplx_cpu.py shows with the
oracle alone that the cases are what they claim).

Bands.  Capped at 6 and 25 iterations (epsilon = 1e-20), n = 1, 2, 3, 65, 200, 513: codes and counts equal the oracle's; the iterate
within dense_multi_cases.late_band's rule of the oracle's: max(1e-9, 50 x the oracle's own response to swapping the product's
summation order, 0.25 x its distance to the column's solution); the reported residual within 1e-9 relative.  Converged (abs_diff = 1,
epsilon = 1e-10, n = 200): check_converged_run's rules 1 and 2 -- code 0, the count within max(3, 3 x the oracle's own spread between
the two summation orders, 5 %), the reported residual <= epsilon, the distance to the solution within 10 x the oracle's.

Measured on the MI355X: the worst ratio of a difference to its band over the capped runs is printed by every capped test
(DESIGN.md section 20 records it)."""
import ctypes as C

import numpy as np
import pytest

import dense_multi_cplx_cases as zc
from dense_multi_cplx_cases import ALREADY, BADEPS, BADMAXIT, BICG_SYM, CONV, E_ARG, KS, MAXIT, NANV, NOPRE, PCG, SIDS, bits, oracle, rel, zmulti

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = 1e-10
NAN = complex(np.nan, np.nan)


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
    """n -> the complex dense handle with the reciprocals of its diagonal"""
    made = {}

    def get(n):
        if n not in made:
            D = api.DenseMatrix.from_array(zc.system(n)["K"])
            D.build_jacobi(False)
            made[n] = D
        return made[n]
    yield get
    for D in made.values():
        D.destroy()


def _check_capped(lib, api, D, S, sid, k, cap, M0=None):
    n = S["n"]
    B = zc.columns(S, k)
    para = dict(epsilon=1e-20, max_iterations=cap)
    M0 = np.zeros((n, k), np.complex128) if M0 is None else M0
    rc, ret, its, res, M = zmulti(lib, api, sid, D, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    worst = 0.0
    for j in range(k):
        m0 = M0[:, j].copy()
        ref, alt = oracle(S, sid, B[:, j], m0=m0, **para), oracle(S, sid, B[:, j], serial=False, m0=m0, **para)
        print(S["key"], sid, k, j, "cap", cap, "ret", ret[j], ref["ret"], "its", its[j], ref["iters"])
        assert ret[j] == ref["ret"] and its[j] == ref["iters"], (j, ret[j], ref["ret"], its[j], ref["iters"])
        if ret[j] == ALREADY:
            assert its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            continue
        band = zc.late_band(ref["x"], alt["x"], zc.solution(S, B[:, j]))
        d = rel(M[:, j], ref["x"]); worst = max(worst, d / band)
        print(f"   rel diff {d:.2e} band {band:.2e} residual {res[j]:.6e} (oracle {ref['residual']:.6e})")
        assert d <= band, (j, cap, d, band)
        if ref["residual"] > 1e-25:          # (n <= 3: converged to rounding, the residual is rounding itself)
            assert abs(res[j] - ref["residual"]) <= 1e-9 * ref["residual"], (j, res[j], ref["residual"])
    print(f"worst ratio of a difference to its band: {worst:.3g}")
    return ret, its


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", SIDS)
@pytest.mark.parametrize("n", zc.SIZES)
def test_capped_runs_against_the_oracle(lib, api, handles, n, sid, k):
    S, D = zc.system(n), handles(n)
    for cap in (6, 25):
        ret, its = _check_capped(lib, api, D, S, sid, k, cap)
        if n >= 65:
            assert ret[0] == ret[1] == MAXIT and its[0] == its[1] == cap
            assert lib.lcg_hip_last_iterations() == cap
        if k >= 4:
            assert ret[3] == ALREADY
    # (513 rows of 513 packs are split in two strips by the automatic choice: the loop's operator is the split form and its fold)
    assert D.multi_last_kernel == ("k_zdnm_row_split" if n == 513 else "k_zdnm_row")


@pytest.mark.parametrize("sid", SIDS)
def test_non_zero_guesses(lib, api, handles, sid):
    import multi_cplx_cases as cc
    for n, k in ((200, 4), (65, 8), (3, 2)):
        S = zc.system(n)
        _check_capped(lib, api, handles(n), S, sid, k, 6, M0=cc.guesses(S, k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", SIDS)
def test_converged_columns_match_the_oracle(lib, api, handles, sid, k):
    """abs_diff = 1, epsilon = 1e-10, n = 200: check_converged_run's rules 1 and 2 per column."""
    S, D = zc.system(200), handles(200)
    n = S["n"]
    B = zc.columns(S, k)
    para = dict(epsilon=EPS, abs_diff=1)
    M0 = np.zeros((n, k), np.complex128)
    zero = [j for j in range(k) if not B[:, j].any()]
    for j in zero:
        M0[:, j] = -0.0 - 0.0j      # a guess of zeros that shows a write
    rc, ret, its, res, M = zmulti(lib, api, sid, D, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        if j in zero:
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            continue
        ref, alt = oracle(S, sid, B[:, j], **para), oracle(S, sid, B[:, j], serial=False, **para)
        dit = abs(ref["iters"] - alt["iters"])
        print(S["key"], sid, k, j, "ret", ret[j], ref["ret"], "its", its[j], ref["iters"], alt["iters"], "residual", res[j])
        assert ret[j] == ref["ret"] == CONV, (j, ret[j], ref["ret"])
        assert abs(its[j] - ref["iters"]) <= max(3, 3 * dit, 0.05 * ref["iters"]), (j, its[j], ref["iters"], dit)
        assert res[j] <= EPS, (j, res[j])
        xt = zc.solution(S, B[:, j])
        e_gpu, e_ref = np.linalg.norm(M[:, j] - xt), np.linalg.norm(ref["x"] - xt)
        print("   distance to the solution", e_gpu, "oracle's", e_ref)
        assert e_gpu <= 10.0 * max(e_ref, 1e-14 * np.linalg.norm(xt)), (j, e_gpu, e_ref)
    longest = int(np.argmax(its))
    assert lib.lcg_hip_last_iterations() == its[longest] and lib.lcg_hip_last_residual() == res[longest]


def _already_batch(S):
    """multi_cplx_cases.already_batch on the dense system (n = 200, |xt|^2 about 930) under abs_diff = 1, epsilon = 1e-6:
    0: m0 = xt + delta with |K.delta| = 0.02 -- sum |r|^2 / n = 2e-6 fails BiCG-sym's first criterion and (|r|^2 / |m|^2)^2 about
       2e-13 meets its second; PCG sees sqrt(|r|^2) / n = 1e-4 and runs;
    1: m0 = xt, exact to rounding -- the first criterion of both;  2: the zero guess, which runs;  3: b = 0 with a guess of -0.0."""
    n, xt, b, K = S["n"], S["xt"], S["b"], S["K"]
    delta = np.cos(1.3 * np.arange(n)) * (1.0 + 0.5j)
    delta *= 0.02 / np.linalg.norm(K @ delta)
    M0 = np.stack([xt + delta, xt, np.zeros(n, np.complex128), np.full(n, -0.0 - 0.0j)], axis=1)
    B = np.stack([b, b, b, np.zeros(n, np.complex128)], axis=1)
    return np.ascontiguousarray(M0), np.ascontiguousarray(B)


@pytest.mark.parametrize("sid", SIDS)
def test_both_already_optimised_criteria(lib, api, handles, sid):
    S, D = zc.system(200), handles(200)
    M0, B = _already_batch(S)
    para = dict(epsilon=1e-6, abs_diff=1)
    rc, ret, its, res, M = zmulti(lib, api, sid, D, M0, B, **para)
    assert rc == 0
    want = [ALREADY, ALREADY, CONV, ALREADY] if sid == BICG_SYM else [CONV, ALREADY, CONV, ALREADY]
    assert ret == want, ret
    for j in range(4):
        ref = oracle(S, sid, B[:, j], m0=M0[:, j], **para)
        assert ret[j] == ref["ret"], (j, ret[j], ref["ret"])
        if ret[j] == ALREADY:
            assert its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            if j == 0:      # the second criterion's value, far above rounding
                assert abs(res[j] - ref["residual"]) <= 1e-6 * ref["residual"], (res[j], ref["residual"])
        else:
            assert abs(its[j] - ref["iters"]) <= 3 and res[j] <= 1e-6


def _verdict_batch(S):
    """Four columns under abs_diff = 1: 0 late (b), 1 early (1e-2 b), 2 a NaN in B, 3 zero."""
    B = zc.columns(S, 4)
    B[S["n"] // 2, 2] = complex(np.nan, 1.0)
    return B


@pytest.mark.parametrize("sid", SIDS)
def test_one_batch_different_verdicts_and_frozen_means_final(lib, api, handles, sid):
    S, D = zc.system(200), handles(200)
    n, k = S["n"], 4
    B = _verdict_batch(S)
    M0 = np.zeros((n, k), np.complex128); M0[:, 3] = -0.0 - 0.0j
    para = dict(epsilon=EPS, abs_diff=1)
    rc, ret, its, res, M = zmulti(lib, api, sid, D, M0, B, **para)
    assert rc == 0
    print(sid, ret, its, res)
    assert ret == [CONV, CONV, NANV, ALREADY], ret
    assert its[2] == 1 and its[3] == 0 and np.array_equal(bits(M[:, 3]), bits(M0[:, 3]))
    t_fast, t_slow = its[1], its[0]
    assert 0 < t_fast and t_fast + 2 <= t_slow, its
    assert np.isfinite(M[:, :2]).all()
    # a cap between the two counts: all four verdicts in one call
    cap = (t_fast + t_slow) // 2
    rc, ret_c, its_c, res_c, M_c = zmulti(lib, api, sid, D, M0, B, max_iterations=cap, **para)
    assert rc == 0 and ret_c[1] == CONV and its_c[1] == t_fast and ret_c[0] == MAXIT and its_c[0] == cap
    assert np.array_equal(bits(M_c[:, 1]), bits(M[:, 1])) and res_c[1] == res[1]
    # frozen means final: the column that converged at t_fast while the others went on = the same B capped at t_fast
    rc, ret_f, its_f, res_f, M_f = zmulti(lib, api, sid, D, M0, B, max_iterations=t_fast, **para)
    assert rc == 0 and ret_f[1] == CONV and its_f[1] == t_fast and ret_f[0] == MAXIT and its_f[0] == t_fast
    assert np.array_equal(bits(M_f[:, 1]), bits(M[:, 1])) and res_f[1] == res[1]
    # max_iterations = 0 (no cap): the NaN column must not keep the batch alive -- the first call returned
    assert lib.lcg_hip_last_iterations() == t_fast


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", SIDS)
def test_a_nan_stays_in_its_column(lib, api, handles, sid, k):
    S, D = zc.system(200), handles(200)
    n = S["n"]
    B = zc.columns(S, k)
    para = dict(epsilon=EPS, abs_diff=1, max_iterations=30)
    Z = np.zeros((n, k), np.complex128)
    rc, ret, its, res, M = zmulti(lib, api, sid, D, Z, B, **para)
    Bn = B.copy(); Bn[n // 2, 1] = NAN
    rc_n, ret_n, its_n, res_n, M_n = zmulti(lib, api, sid, D, Z, Bn, **para)
    assert rc == 0 and rc_n == 0
    assert ret_n[1] == NANV and its_n[1] == 1
    for j in range(k):
        if j == 1:
            continue
        assert ret_n[j] == ret[j] and its_n[j] == its[j] and res_n[j] == res[j], j
        assert np.array_equal(bits(M_n[:, j]), bits(M[:, j])), j
        assert np.isfinite(M_n[:, j]).all()


@pytest.mark.parametrize("n", [200, 3, 513])
@pytest.mark.parametrize("sid", SIDS)
def test_independence_of_neighbours_k_memory_and_calls(lib, api, handles, sid, n):
    """Column j: the same bits at k = 2, 4, 8, with other neighbours (NaN, zero, huge), at another position, from host or device
    memory and from call to call, from non-zero guesses; and under the forced split row form its own bits, the same at every k."""
    S, D = zc.system(n), handles(n)
    import multi_cplx_cases as cc
    para = dict(epsilon=EPS, abs_diff=1, max_iterations=20)
    rng = np.random.default_rng(8)
    B8 = zc.columns(S, 8)
    M8 = cc.guesses(S, 8)
    r8 = zmulti(lib, api, sid, D, M8, B8, **para)
    assert r8[0] == 0
    for again in (zmulti(lib, api, sid, D, M8, B8, **para), zmulti(lib, api, sid, D, M8, B8, mem="host", **para)):
        assert again[0] == 0 and again[1:4] == r8[1:4] and np.array_equal(bits(again[4]), bits(r8[4]))
    for k, picks in ((2, (0, 1)), (2, (2, 5)), (4, (4, 2, 1, 7)), (4, (3, 0, 6, 2)), (8, (7, 6, 5, 4, 3, 2, 1, 0))):
        B = np.ascontiguousarray(B8[:, picks]); M = np.ascontiguousarray(M8[:, picks])
        r = zmulti(lib, api, sid, D, M, B, **para)
        assert r[0] == 0
        for pos, j in enumerate(picks):
            assert (r[1][pos], r[2][pos], r[3][pos]) == (r8[1][j], r8[2][j], r8[3][j]), (k, pos, j)
            assert np.array_equal(bits(r[4][:, pos]), bits(r8[4][:, j])), (k, pos, j)
    # other neighbours: huge, zero, NaN, Inf
    B = B8[:, :4].copy(); M = M8[:, :4].copy()
    B[:, 0] = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 1e3; B[:, 2] = 0.0; M[:, 2] = 0.0; B[0, 3] = NAN
    r = zmulti(lib, api, sid, D, M, B, **para)
    assert r[0] == 0 and (r[1][1], r[2][1], r[3][1]) == (r8[1][1], r8[2][1], r8[3][1]) and np.array_equal(bits(r[4][:, 1]), bits(r8[4][:, 1]))
    B[:, 0] = complex(np.inf, -np.inf)
    r = zmulti(lib, api, sid, D, M, B, **para)
    assert r[0] == 0 and np.array_equal(bits(r[4][:, 1]), bits(r8[4][:, 1]))
    if n == 513:            # the forced split row form (lcg_hip_dense_set_kernel 2: sixteen strips, not the automatic two) inside the loop
        D.set_kernel(2)
        try:
            f8 = zmulti(lib, api, sid, D, M8, B8, **para)
            assert f8[0] == 0 and D.multi_last_kernel == "k_zdnm_row_split"
            f2 = zmulti(lib, api, sid, D, np.ascontiguousarray(M8[:, [5, 1]]), np.ascontiguousarray(B8[:, [5, 1]]), **para)
            assert np.array_equal(bits(f2[4][:, 0]), bits(f8[4][:, 5])) and np.array_equal(bits(f2[4][:, 1]), bits(f8[4][:, 1]))
        finally:
            D.set_kernel(0)


def test_error_returns_release_the_solver(lib, api, handles):
    S, D = zc.system(200), handles(200)
    n, k = S["n"], 4
    B = zc.columns(S, k)
    Z = np.zeros((n, k), np.complex128)
    good = dict(epsilon=EPS, abs_diff=1, max_iterations=10)
    ref = zmulti(lib, api, BICG_SYM, D, Z, B, **good)
    assert ref[0] == 0

    def still_works():
        r = zmulti(lib, api, BICG_SYM, D, Z, B, **good)
        assert r[0] == 0 and r[1:4] == ref[1:4] and np.array_equal(bits(r[4]), bits(ref[4]))
        m = torch.zeros(n, dtype=torch.complex128, device="cuda")
        info = api.clcg_solver("clcg_hip_dense_ax", None, m, torch.from_numpy(S["b"]).cuda(), n,
                               api.clcg_default_parameters(epsilon=EPS, abs_diff=1, max_iterations=10), D, api.CLCG_BICG_SYM)
        assert info.ret == MAXIT and info.iterations == 10

    rp = np.arange(n + 1, dtype=np.int32); ci = np.arange(n, dtype=np.int32)
    A = api.CsrMatrix.from_csr(rp, ci, np.ones(n) + 0j)
    Dr = api.DenseMatrix.from_array(np.eye(n))
    bare = api.DenseMatrix.from_array(S["K"])                  # no reciprocals
    rect = api.DenseMatrix.from_array(np.ones((n + 5, n)) + 0j)
    for sid in SIDS:
        name = "clcg_hip_dense_lpcg_multi" if sid == PCG else "clcg_hip_dense_lbicg_sym_multi"
        for h, why in ((A, "not a dense matrix"), (Dr, "real"), (rect, "square")):
            r = zmulti(lib, api, sid, h, Z, B, **good)
            assert r[0] == E_ARG and r[1] == [99] * k and not r[4].any(), (sid, why)
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and why in err, err
        still_works()
        assert zmulti(lib, api, sid, D, Z, B, epsilon=0.0)[0] == BADEPS
        assert zmulti(lib, api, sid, D, Z, B, epsilon=1.0)[0] == BADEPS
        assert zmulti(lib, api, sid, D, Z, B, max_iterations=-1)[0] == BADMAXIT
        still_works()
        fn = lib.clcg_hip_dense_lpcg_multi if sid == PCG else lib.clcg_hip_dense_lbicg_sym_multi
        Zd = torch.zeros((n, k), dtype=torch.complex128, device="cuda")
        assert fn(D.h, k, Zd.data_ptr(), Zd.data_ptr(), None, None, None, None, 7) == E_ARG and "mem" in lib.lcg_hip_last_error().decode()
        still_works()
    # PCG without reciprocals: after the parameter checks
    r = zmulti(lib, api, PCG, bare, Z, B, **good)
    assert r[0] == NOPRE and r[1] == [99] * k and not r[4].any()
    assert zmulti(lib, api, PCG, bare, Z, B, epsilon=0.0)[0] == BADEPS
    still_works()
    assert zmulti(lib, api, BICG_SYM, bare, Z, B, **good)[0] == 0           # BiCG-sym needs none
    bare.build_jacobi(False)
    rb = zmulti(lib, api, PCG, bare, Z, B, **good)
    rd = zmulti(lib, api, PCG, D, Z, B, **good)
    assert rb[0] == 0 and rb[1:4] == rd[1:4] and np.array_equal(bits(rb[4]), bits(rd[4]))
    # the CSR entries keep refusing the dense handle
    r = lib.clcg_hip_lbicg_sym_multi(D.h, k, 16, 16, None, None, None, None, 1)
    assert r == E_ARG and "dense" in lib.lcg_hip_last_error().decode()
    for h in (A, Dr, bare, rect):
        h.destroy()


def test_launches_are_reported(lib, api, handles):
    """lcg_hip_last_launches after 10 iterations at n = 200 (one strip: the row form alone) and n = 513 (split: the row form and
    its fold): the operator is one or two launches plus the k-wide sum inside the loop, one or two for the setup's
    product, which carries no sum; two vector passes per iteration and for the setup."""
    for n, variant, per in ((200, 0, 1), (513, 0, 2), (513, 2, 2)):
        S, D = zc.system(n), handles(n)
        D.set_kernel(variant)
        try:
            for sid in SIDS:
                rc, ret, its, _, _ = zmulti(lib, api, sid, D, np.zeros((n, 8), np.complex128), zc.columns(S, 8), epsilon=1e-20, max_iterations=10)
                assert rc == 0 and its[0] == 10
                vec, prod = C.c_int(), C.c_int()
                lib.lcg_hip_last_launches(C.byref(vec), None, None, C.byref(prod))
                assert (prod.value, vec.value) == (per + 10 * (per + 1), 2 + 10 * 2), (n, sid, prod.value, vec.value)
                assert D.multi_last_kernel == zc.NAMES[per - 1]
        finally:
            D.set_kernel(0)


def test_python_front(api, handles):
    S, D = zc.system(200), handles(200)
    n = S["n"]
    B = torch.from_numpy(zc.columns(S, 4)).cuda()
    p = api.clcg_default_parameters(epsilon=EPS, abs_diff=1)
    for f in (api.dense_clbicg_sym_multi, api.dense_clpcg_multi):
        M = torch.zeros((n, 4), dtype=torch.complex128, device="cuda")
        infos = f(D, M, B, p)
        assert [i.ret for i in infos] == [CONV, CONV, CONV, ALREADY] and infos[3].iterations == 0
        Y = torch.full((n, 4), NAN, dtype=torch.complex128, device="cuda")
        D.cmatmat(M, Y)
        api.synchronize()
        r = (Y - B).cpu().numpy()
        assert np.linalg.norm(r[:, 0]) / n <= 2e-5                      # (BiCG-sym's abs rule is sum |r|^2 / n <= 1e-10)
        Mh = np.zeros((n, 4), np.complex128)
        infos_h = f(D, Mh, B.cpu().numpy(), p)
        assert [i.ret for i in infos_h] == [CONV, CONV, CONV, ALREADY]
        assert np.array_equal(bits(Mh), bits(M.cpu().numpy()))
    U = torch.from_numpy(zc.columns(S, 4)).cuda()
    dots = D.cop_multi_dot(M, Y, U)
    assert dots.dtype == np.complex128 and dots.shape == (4,)
    Yh, Uh = Y.cpu().numpy(), U.cpu().numpy()
    assert np.all(np.abs(dots - np.sum(Yh * Uh, axis=0)) <= 1e-12 * np.sum(np.abs(Yh * Uh), axis=0) + 1e-300)
    with pytest.raises(ValueError):
        D.cmatmat(M.real.contiguous(), Y)


def test_sample_program_solves_four_sources_with_both_loops():
    import re
    import subprocess
    from test_dropin_cpp import _build
    exe = _build("sample_dense_complex_multi")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = re.findall(r"^column (\d): ret=(-?\d+) iterations=(\d+)", p.stdout, flags=re.M)
    assert [(int(j), int(r)) for j, r, _ in got] == [(0, CONV), (1, CONV), (2, CONV), (3, ALREADY)] * 2
    assert "clcg_hip_dense_lbicg_sym_multi" in p.stdout and "clcg_hip_dense_lpcg_multi" in p.stdout and "distance_to_truth" in p.stdout
