"""-m gpu: solvers on K^T.K of a rectangular CSR matrix (include/lcg_hip_staging_csr_normal.h; systems, columns and the Python-product
oracle: tests/csr_normal_cases.py).

Callbacks: the seven real solvers on lcg_hip_csr_ata_ax (PCG with lcg_hip_csr_jacobi_normal_mx, PG / SPG in the box 1 <= m <= 2)
against the oracle's loops fed the Python product, under test_real_solvers_through_the_normal_equations_callback's rules
(tests/test_gpu_dense.py): capped at 5 and 20 within max(1e-9, 50 x the oracle's own response: its spread between the serial and the
pairwise product order, and on dense3000 also its response to 1-ulp changes of b -- csr_normal_cases.response); converged runs by
check_converged_run's rule (code, count band, residual, distance to the solution, the iterate two short of the earlier stop within
the late band).
Batched CG / PCG: every column against the oracle's run of that column alone by the same bands (tests/test_gpu_dense_multi_solvers.py).
Box loops: every column against the oracle's run of that column alone at cap 12 between bounds that cut the solution, within
max(1e-9, 50 x the oracle's response to 1-ulp changes of b) (tests/test_gpu_multi_box.py's band); code, count and products are pinned
where the oracle's do not move under four seeded 1-ulp changes of b.
The worst ratio of a difference to its band is printed."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import csr_normal_cases as X
import stream_cases as st
from csr_normal_cases import ALREADY, CG, CONV, EPS, KS, MAXIT, NANV, NOPRE, PCG, PG, SPG, bits, multi, oracle, rel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CAP = 600
EDGES = ["tiny7x3", "tiny5x2", "tiny3x1", "edge65", "wide513", "dense3000", "tall9000", "small"]


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
    made = {}

    def get(name):
        if name not in made:
            made[name] = X.handle(api, X.system(name))
        return made[name]
    yield get
    for A in made.values():
        A.destroy()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a C-ordered copy: the cases' arrays are read-only)


# ================================================================================================ 1. the callbacks
def _gpu_real(api, A, sid, b, n, cap, low, hig, device):
    para = api.lcg_default_parameters(epsilon=EPS, abs_diff=0, max_iterations=cap)
    if device:
        m = torch.zeros(n, dtype=torch.float64, device="cuda"); bb = dev(b); lo, hi = dev(low), dev(hig)
    else:
        m = np.zeros(n); bb = np.ascontiguousarray(b); lo, hi = low, hig
    if sid == PCG:
        info = api.lcg_solver_preconditioned("lcg_hip_csr_ata_ax", "lcg_hip_csr_jacobi_normal_mx", None, m, bb, n, para, A)
    elif sid >= PG:
        info = api.lcg_solver_constrained("lcg_hip_csr_ata_ax", None, m, bb, lo, hi, n, para, A, sid)
    else:
        info = api.lcg_solver("lcg_hip_csr_ata_ax", None, m, bb, n, para, A, sid)
    return info, (m.cpu().numpy() if device else m)


@pytest.mark.parametrize("name", ["main", "edge65", "dense3000"])
def test_real_solvers_through_the_callback(api, lib, handles, name):
    S = X.system(name)
    A = handles(name)
    n, b, xt = S["n"], S["b"], S["xt"]
    low, hig = np.full(n, 1.0), np.full(n, 2.0)
    worst, capped_only = 0.0, []
    for sid in range(7):
        wide = sid in (X.CGS, X.BICGSTAB, X.BICGSTAB2)
        box = dict(low=low, hig=hig) if sid >= PG else {}
        for cap in (5, 20):
            ref = oracle(S, sid, b, cap, **box)
            band = max(X.FLOOR, X.FACTOR * X.response(S, sid, b, cap, **box))
            for device in ((True, False) if sid in (CG, PG) else (True,)):
                info, x = _gpu_real(api, A, sid, b, n, cap, low, hig, device)
                r = rel(x, ref["x"]); worst = max(worst, r / band)
                print(f"{name} solver {sid} cap {cap} device {device}: rel diff {r:.2e} band {band:.2e}")
                assert r <= band, (sid, cap, device, r, band)
                if sid in (CG, PCG) and ref["ret"] == MAXIT:
                    vec, prod = C.c_int(), C.c_int()
                    lib.lcg_hip_last_launches(C.byref(vec), None, None, C.byref(prod))
                    # both products of every application are counted (a guess of zeros: the loop may leave the setup's product out)
                    assert prod.value in (2 * cap, 2 * (cap + 1)), (sid, cap, prod.value)
        ref, alt = oracle(S, sid, b, CAP, **box), oracle(S, sid, b, CAP, serial=False, **box)
        if ref["ret"] != 0 or alt["ret"] != 0:
            capped_only.append(sid)
            continue
        info, x = _gpu_real(api, A, sid, b, n, CAP, low, hig, True)
        assert info.ret == ref["ret"] == 0, (sid, info.ret)
        dit = abs(ref["iters"] - alt["iters"])
        cnt = max(3, 4 * dit, 0.3 * ref["iters"]) if wide else max(3, 3 * dit, 0.05 * ref["iters"])
        assert abs(info.iterations - ref["iters"]) <= cnt, (sid, info.iterations, ref["iters"], dit)
        assert info.residual <= EPS
        e_gpu, e_ref = np.linalg.norm(x - xt), np.linalg.norm(ref["x"] - xt)
        assert e_gpu <= (100.0 if wide else 10.0) * max(e_ref, 1e-14 * np.linalg.norm(xt)), (sid, "distance to the solution", e_gpu, e_ref)
        Kc = min(info.iterations, ref["iters"], alt["iters"]) - 2
        if Kc >= 1:
            rK, aK = oracle(S, sid, b, Kc, **box), oracle(S, sid, b, Kc, serial=False, **box)
            band = X.late_band(rK["x"], X.response(S, sid, b, Kc, **box), xt)
            iK, xK = _gpu_real(api, A, sid, b, n, Kc, low, hig, True)
            assert iK.ret == rK["ret"] == aK["ret"] == MAXIT and iK.iterations == rK["iters"] == aK["iters"] == Kc, \
                (sid, Kc, iK.ret, rK["ret"], iK.iterations, rK["iters"], aK["iters"])
            r = rel(xK, rK["x"]); worst = max(worst, r / band)
            print(f"{name} solver {sid} converged in {info.iterations} (oracle {ref['iters']} / {alt['iters']}); at {Kc}: rel diff {r:.2e} band {band:.2e}")
            assert r <= band, (sid, Kc, r, band)
    print(f"{name}: worst ratio to the band: {worst:.3g}; compared capped only (the oracle does not converge in {CAP}): {capped_only}")
    assert CG not in capped_only and PCG not in capped_only


# ================================================================================================ 2. the batched CG / PCG
def _check_capped(lib, api, A, S, sid, k, cap):
    B = X.columns(S, k)
    rc, ret, its, res, M = multi(lib, api, sid, A, np.zeros((S["n"], k)), B, epsilon=EPS, max_iterations=cap)
    assert rc == 0, lib.lcg_hip_last_error()
    worst = 0.0
    for j in range(k):
        ref, alt = oracle(S, sid, B[:, j], cap), oracle(S, sid, B[:, j], cap, serial=False)
        if not B[:, j].any():
            assert ret[j] == ref["ret"] == ALREADY and its[j] == 0 and not M[:, j].any()
            continue
        band = max(X.FLOOR, X.FACTOR * X.response(S, sid, np.ascontiguousarray(B[:, j]), cap))
        r = rel(M[:, j], ref["x"]); worst = max(worst, r / band)
        print(f"{S['key']} solver {sid} k {k} column {j} cap {cap}: ret {ret[j]} its {its[j]} (oracle {ref['ret']} {ref['iters']}) rel diff {r:.2e} band {band:.2e}")
        assert r <= band, (j, cap, r, band)
        if ref["ret"] == alt["ret"] == MAXIT:
            assert ret[j] == MAXIT and its[j] == cap == ref["iters"], (j, ret[j], its[j])
    return worst


def _check_converged(lib, api, A, S, sid, k):
    B = X.columns(S, k)
    n = S["n"]
    M0 = np.zeros((n, k))
    zero = [j for j in range(k) if not B[:, j].any()]
    for j in zero:
        M0[:, j] = -0.0         # a guess of zeros that shows a write
    rc, ret, its, res, M = multi(lib, api, sid, A, M0, B, epsilon=EPS, max_iterations=CAP)
    assert rc == 0, lib.lcg_hip_last_error()
    worst, late = 0.0, {}
    for j in range(k):
        if j in zero:
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            continue
        ref, alt = oracle(S, sid, B[:, j], CAP), oracle(S, sid, B[:, j], CAP, serial=False)
        assert ref["ret"] == alt["ret"] == CONV, (S["key"], sid, j, "the oracle did not converge", ref["ret"], alt["ret"])
        assert ret[j] == CONV, (j, ret[j])
        dit = abs(ref["iters"] - alt["iters"])
        assert abs(its[j] - ref["iters"]) <= max(3, 3 * dit, 0.05 * ref["iters"]), (j, its[j], ref["iters"], dit)
        assert res[j] <= EPS, (j, res[j])
        xt = X.solution(S, B[:, j])
        e_gpu, e_ref = np.linalg.norm(M[:, j] - xt), np.linalg.norm(ref["x"] - xt)
        assert e_gpu <= 10.0 * max(e_ref, 1e-14 * np.linalg.norm(xt)), (j, "distance to the solution", e_gpu, e_ref)
        late[j] = (min(its[j], ref["iters"], alt["iters"]) - 2, xt)
        print(f"{S['key']} solver {sid} k {k} column {j}: converged in {its[j]} (oracle {ref['iters']} / {alt['iters']}), residual {res[j]:.2e}, "
              f"distance to the solution {e_gpu:.2e} (oracle {e_ref:.2e})")
    for Kc in sorted({v[0] for v in late.values() if v[0] >= 1}):
        rc, retK, itsK, _, MK = multi(lib, api, sid, A, np.zeros((n, k)), B, epsilon=EPS, max_iterations=Kc)
        assert rc == 0
        for j, (kc, xt) in late.items():
            if kc != Kc:
                continue
            rK, aK = oracle(S, sid, B[:, j], Kc), oracle(S, sid, B[:, j], Kc, serial=False)
            assert retK[j] == rK["ret"] == aK["ret"] == MAXIT and itsK[j] == rK["iters"] == aK["iters"] == Kc, (j, Kc, retK[j], rK["ret"], itsK[j])
            band = X.late_band(rK["x"], X.response(S, sid, np.ascontiguousarray(B[:, j]), Kc), xt)
            r = rel(MK[:, j], rK["x"]); worst = max(worst, r / band)
            print(f"   column {j} at {Kc}: rel diff {r:.2e} band {band:.2e}")
            assert r <= band, (j, Kc, r, band)
    return worst


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", [CG, PCG])
def test_main_system_against_the_oracle(lib, api, handles, sid, k):
    S = X.system("main")
    A = handles("main")
    worst = max(_check_capped(lib, api, A, S, sid, k, 5), _check_capped(lib, api, A, S, sid, k, 20), _check_converged(lib, api, A, S, sid, k))
    print(f"worst ratio to a band: {worst:.3g}")


@pytest.mark.parametrize("name", EDGES)
@pytest.mark.parametrize("sid", [CG, PCG])
def test_edge_systems_against_the_oracle(lib, api, handles, sid, name):
    """The tiny systems at every k; the others at one k each, so that every k meets long rows of K^T and the 65 / 513 edges."""
    S = X.system(name)
    A = handles(name)
    worst = 0.0
    for k in (KS if name in X.TINY else (KS[EDGES.index(name) % 3],)):
        worst = max(worst, _check_capped(lib, api, A, S, sid, k, 5), _check_converged(lib, api, A, S, sid, k))
    print(f"worst ratio to a band: {worst:.3g}")


def _fast_and_slow(S, k):
    """Columns that converge at different counts: column 1 lies in the span of the operator's three dominant eigenvectors."""
    B = X.columns(S, k)
    K = X.dense(S)
    w, V = np.linalg.eigh(K.T @ K)
    B[:, 1] = (K.T @ K) @ (V[:, -1] + 0.5 * V[:, -2] + 0.25 * V[:, -3])
    return B


@pytest.mark.parametrize("sid", [CG, PCG])
def test_verdicts_differ_and_stopped_columns_are_final(lib, api, handles, sid):
    S = X.system("main")
    A = handles("main")
    n, k = S["n"], 4
    B = _fast_and_slow(S, k)
    rc, ret, its, res, M = multi(lib, api, sid, A, np.zeros((n, k)), B, epsilon=EPS, max_iterations=CAP)
    assert rc == 0 and ret[0] == ret[1] == CONV
    t_fast, t_slow = its[1], its[0]
    print(sid, "counts", its)
    assert 0 < t_fast and t_fast + 2 <= t_slow, its
    cap = (t_fast + t_slow) // 2             # a cap between the two counts: three verdicts in one call
    rc, ret_c, its_c, res_c, M_c = multi(lib, api, sid, A, np.zeros((n, k)), B, epsilon=EPS, max_iterations=cap)
    assert rc == 0
    assert ret_c[1] == CONV and its_c[1] == t_fast
    assert ret_c[0] == MAXIT and its_c[0] == cap
    assert ret_c[3] == ALREADY and its_c[3] == 0 and not M_c[:, 3].any()
    assert np.array_equal(bits(M_c[:, 1]), bits(M[:, 1])) and res_c[1] == res[1]
    # frozen means final: the column that converged at t_fast while the others went on = the same B capped at t_fast
    rc, ret_f, its_f, res_f, M_f = multi(lib, api, sid, A, np.zeros((n, k)), B, epsilon=EPS, max_iterations=t_fast)
    assert rc == 0 and ret_f[1] == CONV and its_f[1] == t_fast and ret_f[0] == MAXIT and its_f[0] == t_fast
    assert np.array_equal(bits(M_f[:, 1]), bits(M[:, 1])) and res_f[1] == res[1]
    assert lib.lcg_hip_last_iterations() == t_fast


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", [CG, PCG])
def test_a_nan_stays_in_its_column(lib, api, handles, sid, k):
    S = X.system("main")
    A = handles("main")
    n = S["n"]
    B = _fast_and_slow(S, k)
    para = dict(epsilon=EPS, max_iterations=40)
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
@pytest.mark.parametrize("name", ["main", "tiny7x3", "dense3000", "tall9000"])
def test_independence_memory_and_guesses(lib, api, handles, name, sid):
    """Column j: the same bits at k = 2, 4, 8, with other neighbours, at another position, from host or device memory and from
    call to call; from a non-zero guess within the capped band of the oracle started from that guess."""
    S = X.system(name)
    A = handles(name)
    n = S["n"]
    para = dict(epsilon=EPS, max_iterations=30)
    rng = np.random.default_rng(8)
    B8 = X.columns(S, 8)
    M8 = np.zeros((n, 8)); M8[:, 1] = rng.standard_normal(n); M8[:, 2] = 0.5 * S["xt"]
    r8 = multi(lib, api, sid, A, M8, B8, **para)
    assert r8[0] == 0
    for again in (multi(lib, api, sid, A, M8, B8, **para), multi(lib, api, sid, A, M8, B8, mem="host", **para)):
        assert again[0] == 0 and again[1:4] == r8[1:4] and np.array_equal(bits(again[4]), bits(r8[4]))
    for k, picks in ((2, (0, 1)), (2, (2, 5)), (4, (4, 2, 1, 7)), (4, (3, 0, 6, 2)), (8, (7, 6, 5, 4, 3, 2, 1, 0))):
        B = np.ascontiguousarray(B8[:, picks]); M = np.ascontiguousarray(M8[:, picks])
        r = multi(lib, api, sid, A, M, B, **para)
        assert r[0] == 0
        for pos, j in enumerate(picks):
            assert (r[1][pos], r[2][pos], r[3][pos]) == (r8[1][j], r8[2][j], r8[3][j]), (k, pos, j)
            assert np.array_equal(bits(r[4][:, pos]), bits(r8[4][:, j])), (k, pos, j)
    # other neighbours: huge, zero, NaN
    B = B8[:, :4].copy(); M = M8[:, :4].copy()
    B[:, 0] = rng.standard_normal(n) * 1e3; B[:, 2] = 0.0; M[:, 2] = 0.0; B[0, 3] = np.nan
    r = multi(lib, api, sid, A, M, B, **para)
    assert r[0] == 0 and (r[1][1], r[2][1], r[3][1]) == (r8[1][1], r8[2][1], r8[3][1]) and np.array_equal(bits(r[4][:, 1]), bits(r8[4][:, 1]))
    # the non-zero guesses against the oracle from the same guess
    for j in (1, 2):
        cap = 20
        rc, ret, its, res, Mc = multi(lib, api, sid, A, M8[:, :4], B8[:, :4], epsilon=EPS, max_iterations=cap)
        ref = oracle(S, sid, B8[:, j], cap, m0=M8[:, j]); alt = oracle(S, sid, B8[:, j], cap, serial=False, m0=M8[:, j])
        band = max(X.FLOOR, X.FACTOR * X.response(S, sid, np.ascontiguousarray(B8[:, j]), cap, m0=M8[:, j]))
        assert rc == 0 and rel(Mc[:, j], ref["x"]) <= band, (j, rel(Mc[:, j], ref["x"]), band)


def test_launches_are_counted_and_no_diagonal_is_refused(lib, api, handles):
    S = X.system("main")
    A = handles("main")
    for sid in (CG, PCG):
        rc, ret, its, _, _ = multi(lib, api, sid, A, np.zeros((S["n"], 8)), X.columns(S, 8), epsilon=EPS, max_iterations=10)
        assert rc == 0 and its[0] == 10
        vec, prod = C.c_int(), C.c_int()
        lib.lcg_hip_last_launches(C.byref(vec), None, None, C.byref(prod))
        assert (prod.value, vec.value) == (2 + 10 * 2, 2 + 10 * 2), (prod.value, vec.value)
    bare = X.handle(api, S, jacobi=False)
    Z, B = np.zeros((S["n"], 4)), X.columns(S, 4)
    assert multi(lib, api, PCG, bare, Z, B, epsilon=EPS, max_iterations=10)[0] == NOPRE
    assert multi(lib, api, CG, bare, Z, B, epsilon=EPS, max_iterations=10)[0] == 0           # plain CG needs none
    bare.destroy()


# ================================================================================================ 3. the box loops
BOX_RULE = dict(epsilon=EPS, abs_diff=1)
BOX_CAP = 12
BOX_SEEDS = 4


def _bounds(S):
    """-0.3 <= m <= 1.7 cuts the solution of column b (xt fills [1, 2]), leaves the small columns' inside and puts the whole of column
    -b's (and most of 2 b's) on a bound: on the 65-column system those iterates stop moving and the reference breaks down."""
    return np.full(S["n"], -0.3), np.full(S["n"], 1.7)


def _first_nan_cap(S, sid, bcol, low, hig):
    """The smallest cap at which the oracle's iterate holds a NaN (None: none up to BOX_CAP)."""
    for cap in range(1, BOX_CAP + 1):
        if np.isnan(oracle(S, sid, bcol, cap, low=low, hig=hig, abs_diff=1)["x"]).any():
            return cap
    return None


def _box_against_oracle(lib, api, A, S, sid, k, mem="device"):
    low, hig = _bounds(S)
    B = X.columns(S, k)
    r = X.box(lib, api, sid, A, np.zeros((S["n"], k)), B, low, hig, mem=mem, max_iterations=BOX_CAP, **BOX_RULE)
    rc, ret, its, prods, res, out = r
    assert rc == 0, lib.lcg_hip_last_error()
    worst = 0.0
    for j in range(k):
        bcol = np.ascontiguousarray(B[:, j])
        x = out[:, j]
        assert np.isfinite(x).all() and (x >= low).all() and (x <= hig).all(), (sid, k, j, "outside the box")
        cap, want = BOX_CAP, None
        c = _first_nan_cap(S, sid, bcol, low, hig)
        if c is not None:
            # the reference broke down before the cap and ran on with NaN (deviation 1): the batch column ends with LCG_NAN_VALUE one
            # iteration before the reference's first NaN iterate, and is held to the oracle's run capped there
            assert c >= 2, (sid, k, j, c)
            moved = [_first_nan_cap(S, sid, X.perturbed(bcol, seed), low, hig) for seed in range(BOX_SEEDS)]
            cap = c - 1
            if moved == [c] * BOX_SEEDS:
                want = (NANV, c - 1)
            else:
                print(f"{S['key']} box {sid} k {k} column {j}: the reference's breakdown moves with 1 ulp of b ({c}, {moved}): in the box, not compared")
                assert ret[j] in (NANV, MAXIT)
                continue
        ref = oracle(S, sid, bcol, cap, low=low, hig=hig, abs_diff=1)
        sens, stable = 0.0, True
        for seed in range(BOX_SEEDS):
            p = oracle(S, sid, X.perturbed(bcol, seed), cap, low=low, hig=hig, abs_diff=1)
            stable = stable and (p["ret"], p["iters"], p["n_ax"]) == (ref["ret"], ref["iters"], ref["n_ax"])
            if np.linalg.norm(ref["x"]) > 0.0:
                sens = max(sens, rel(p["x"], ref["x"]))
        band = max(X.FLOOR, X.FACTOR * sens)
        d = rel(x, ref["x"]); worst = max(worst, d / band)
        print(f"{S['key']} box {sid} k {k} column {j}: ret {ret[j]} its {its[j]} products {prods[j]} (oracle {ref['ret']} {ref['iters']} {ref['n_ax']}, "
              f"{'stable' if stable else 'moves with 1 ulp of b'}{', breakdown' if want else ''}) distance {d:.2e} band {band:.2e}")
        assert d <= band, (sid, k, j, d, band)
        if want is not None:
            assert (ret[j], its[j]) == want, (sid, k, j, ret[j], its[j], want)
        elif stable:
            assert (ret[j], its[j], prods[j]) == (ref["ret"], ref["iters"], ref["n_ax"]), (sid, k, j, ret[j], its[j], prods[j], ref["ret"], ref["iters"], ref["n_ax"])
    return r, worst


@pytest.mark.parametrize("sid", [PG, SPG])
@pytest.mark.parametrize("name", ["edge65", "main", "dense3000"])
def test_box_loops_against_the_oracle(lib, api, handles, name, sid):
    S = X.system(name)
    A = handles(name)
    low, hig = _bounds(S)
    assert (S["xt"] > hig).any() and (S["xt"] < hig).any(), "the bounds cut the solution"
    runs, worst = {}, 0.0
    for k in (KS if name == "edge65" else (4,)):
        runs[k], w = _box_against_oracle(lib, api, A, S, sid, k)
        worst = max(worst, w)
    print(f"worst ratio to a band: {worst:.3g}")
    if name != "edge65":
        return
    # a column's bits do not depend on k; host memory; call to call
    r8 = runs[8]
    for k in (2, 4):
        for j in range(k):
            assert [runs[k][q][j] for q in (1, 2, 3, 4)] == [r8[q][j] for q in (1, 2, 3, 4)] and np.array_equal(bits(runs[k][5][:, j]), bits(r8[5][:, j])), (k, j)
    B8 = X.columns(S, 8)
    picks = (7, 6, 5, 4, 3, 2, 1, 0)
    rp = X.box(lib, api, sid, A, np.zeros((S["n"], 8)), np.ascontiguousarray(B8[:, picks]), low, hig, mem="host", max_iterations=BOX_CAP, **BOX_RULE)
    for pos, j in enumerate(picks):
        assert [rp[q][pos] for q in (1, 2, 3, 4)] == [r8[q][j] for q in (1, 2, 3, 4)] and np.array_equal(bits(rp[5][:, pos]), bits(r8[5][:, j])), (pos, j)
    Bn = B8[:, :4].copy(); Bn[3, 0] = np.nan; Bn[:, 2] = np.inf
    rn = X.box(lib, api, sid, A, np.zeros((S["n"], 4)), Bn, low, hig, max_iterations=BOX_CAP, **BOX_RULE)
    assert rn[0] == 0 and rn[1][0] == NANV and [rn[q][1] for q in (1, 2, 3, 4)] == [r8[q][1] for q in (1, 2, 3, 4)]
    assert np.array_equal(bits(rn[5][:, 1]), bits(r8[5][:, 1]))


# ================================================================================================ 4. the rewrite protocol
def test_state_survives_the_setters_and_follows_a_rewrite(lib, api):
    """lcg_hip_csr_set_packed(K, 0) (and its three siblings) leave the normal state usable; values rewritten in place after it are
    what the next product multiplies by, Jacobi included."""
    S = X.system("small")
    A = X.handle(api, S)
    n = S["n"]
    x = dev(S["xt"]); y = torch.empty_like(x)
    A.ata(x, y); api.synchronize()
    y0 = y.cpu().numpy().copy()
    for setter in (lib.lcg_hip_csr_set_packed, lib.lcg_hip_csr_set_tiled, lib.lcg_hip_csr_set_binned, lib.lcg_hip_csr_set_ranges):
        assert setter(A.h, 0) == 0
        y.fill_(float("nan"))
        A.ata(x, y); api.synchronize()
        assert np.array_equal(bits(y.cpu().numpy()), bits(y0))
        assert setter(A.h, -1) == 0
    rc, ret, its, res, M = multi(lib, api, PCG, A, np.zeros((n, 2)), X.columns(S, 2), epsilon=EPS, max_iterations=CAP)
    assert rc == 0 and ret == [CONV, CONV]
    # rewrite: every value doubled in place, between set_packed(0) and the next use
    assert lib.lcg_hip_csr_set_packed(A.h, 0) == 0
    pv = C.c_void_p()
    lib.lcg_hip_csr_arrays(A.h, None, None, C.byref(pv))
    v2 = np.ascontiguousarray(2.0 * S["v"])
    assert lib.lcg_hip_memcpy(pv, v2.ctypes.data, v2.nbytes, 1) == 0
    assert lib.lcg_hip_csr_set_packed(A.h, -1) == 0
    A.ata(x, y); api.synchronize()
    assert np.array_equal(bits(y.cpu().numpy()), bits(4.0 * y0))
    rpT, ciT, vT = A.normal_to_host()
    assert np.array_equal(bits(vT), bits(2.0 * S["vT"])) and np.array_equal(ciT, S["ciT"])
    d = torch.empty(n, dtype=torch.float64, device="cuda")
    z = torch.empty_like(d)
    lib.lcg_hip_csr_jacobi_normal_mx(A.h, dev(np.ones(n)).data_ptr(), z.data_ptr(), n); api.synchronize()
    A.build_jacobi_normal(d); api.synchronize()
    assert np.array_equal(z.cpu().numpy(), 1.0 / d.cpu().numpy())
    np.testing.assert_allclose(d.cpu().numpy(), 4.0 * X.normal_diagonal(S), rtol=1e-13)
    A.destroy()


# ================================================================================================ 5. the caller's stream
@pytest.fixture(scope="module")
def env(api, lib):
    e = st.make_env(torch, api, lib)
    yield e
    st.close_env(e)


def test_callers_stream(env, api, lib, handles):
    """tests/test_gpu_streams_kwide.py's pattern: run (b) on the accepted side stream, entered while the delay runs on it with the
    inputs written behind the delay, has run (a)'s results bit for bit -- for the products, the Jacobi callback, the build of K^T from
    arrays written late, and the three batched loops."""
    S = X.system("main")
    A = handles("main")
    n, m, k = S["n"], S["m"], 4
    Bh = X.columns(S, k)
    rng = np.random.default_rng(4)
    xh, th, Xh, Th, Uh = S["xt"], rng.standard_normal(m), rng.standard_normal((n, k)), rng.standard_normal((m, k)), rng.standard_normal((n, k))
    x, t, Xd, Td, Ud = (torch.empty_like(dev(a)) for a in (xh, th, Xh, Th, Uh))
    y, Y = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty((n, k), dtype=torch.float64, device="cuda")
    def finite(tag):
        def anchor(r, outs):
            assert r in (0, None), (tag, r, lib.lcg_hip_last_error())
            st.no_nan(outs, tag)
        return anchor
    env.pair([(x, dev(xh))], lambda: lib.lcg_hip_csr_ata(A.h, x.data_ptr(), y.data_ptr()), [y], True, tag="ata", anchor=finite("ata"))
    env.pair([(t, dev(th))], lambda: lib.lcg_hip_spmv_t(A.h, t.data_ptr(), y.data_ptr()), [y], True, tag="spmv_t", anchor=finite("spmv_t"))
    env.pair([(x, dev(xh))], lambda: lib.lcg_hip_csr_ata_ax(A.h, x.data_ptr(), y.data_ptr(), n), [y], True, tag="ata_ax", anchor=finite("ata_ax"))
    env.pair([(x, dev(xh))], lambda: lib.lcg_hip_csr_jacobi_normal_mx(A.h, x.data_ptr(), y.data_ptr(), n), [y], True, tag="jacobi_mx", anchor=finite("jacobi_mx"))
    env.pair([(Td, dev(Th))], lambda: lib.lcg_hip_spmm_t(A.h, k, Td.data_ptr(), Y.data_ptr()), [Y], True, tag="spmm_t", anchor=finite("spmm_t"))
    env.pair([(Xd, dev(Xh))], lambda: lib.lcg_hip_csr_ata_multi(A.h, k, Xd.data_ptr(), Y.data_ptr()), [Y], True, tag="ata_multi", anchor=finite("ata_multi"))

    def dot_call():
        out = (C.c_double * k)()
        rc = lib.lcg_hip_csr_ata_multi_dot(A.h, k, Xd.data_ptr(), Y.data_ptr(), Ud.data_ptr(), out)
        return (rc,) + tuple(out)
    env.pair([(Xd, dev(Xh)), (Ud, dev(Uh))], dot_call, [Y], False, tag="ata_multi_dot",
             anchor=lambda r, outs: finite("ata_multi_dot")(r[0] if np.isfinite(r[1:]).all() else r, outs))

    # the build: K's values written late into adopted device arrays, K^T and the sums of squares built on the side stream
    rpd, cid = dev(S["rp"]), dev(S["ci"])
    vd = torch.empty_like(dev(S["v"]))
    D = api.CsrMatrix.from_csr(rpd, cid, vd, n_cols=n, adopt=True)
    dsq = torch.empty(n, dtype=torch.float64, device="cuda")
    vT = torch.empty(len(S["v"]), dtype=torch.float64, device="cuda")

    def build_call():
        lib.lcg_hip_csr_set_packed(D.h, 0)          # (the arrays are about to be different ones: a state from run (a) is stale)
        rc = lib.lcg_hip_csr_build_normal(D.h)
        rc = rc or lib.lcg_hip_csr_build_jacobi_normal(D.h, dsq.data_ptr())
        pv, longest = C.c_void_p(), C.c_int()
        rc = rc or lib.lcg_hip_csr_normal_arrays(D.h, None, None, C.byref(pv))
        rc = rc or lib.lcg_hip_csr_normal_info(D.h, C.byref(longest), None, None) or int(longest.value != int(np.diff(S["rpT"]).max()))
        rc = rc or lib.lcg_hip_memcpy(vT.data_ptr(), pv, 8 * len(S["v"]), 3)
        return rc

    def build_anchor(r, outs):
        assert r == 0, lib.lcg_hip_last_error()
        assert np.array_equal(bits(outs[0]), bits(S["vT"]))
    env.pair([(vd, dev(S["v"]))], build_call, [vT, dsq], False, tag="build", anchor=build_anchor)
    D.destroy()

    # the loops
    para = api.lcg_default_parameters(epsilon=EPS, abs_diff=0, max_iterations=12)
    low, hig = _bounds(S)
    Md, Bd, ld, hd = (torch.empty_like(dev(a)) for a in (Bh, Bh, low, hig))
    for name in ("lcg_hip_csr_normal_lcg_multi", "lcg_hip_csr_normal_lpcg_multi", "pg", "spg"):
        def call(name=name):
            ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); prods = (C.c_int * k)(); res = (C.c_double * k)()
            if name in ("pg", "spg"):
                rc = lib.lcg_hip_csr_normal_solver_constrained_multi(A.h, k, SPG if name == "spg" else PG, Md.data_ptr(), Bd.data_ptr(), ld.data_ptr(),
                                                                     hd.data_ptr(), C.byref(para), ret, its, prods, res, 1)
            else:
                rc = getattr(lib, name)(A.h, k, Md.data_ptr(), Bd.data_ptr(), C.byref(para), ret, its, res, 1)
            return rc, list(ret), list(its), list(prods), list(res)

        def anchor(r, outs, name=name):
            assert r[0] == 0 and 99 not in r[1] and max(r[2]) == 12, (name, r, lib.lcg_hip_last_error())
            st.no_nan(outs, name)
        env.pair([(Md, dev(np.zeros_like(Bh))), (Bd, dev(Bh)), (ld, dev(low)), (hd, dev(hig))], call, [Md], False, tag=name, anchor=anchor)


# ================================================================================================ 6. the Python front, the example
def test_python_front(api, handles):
    S = X.system("main")
    A = handles("main")
    n = S["n"]
    B = dev(X.columns(S, 4))
    M = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    para = api.lcg_default_parameters(epsilon=EPS, abs_diff=0, max_iterations=CAP)
    infos = api.csr_normal_lpcg_multi(A, M, B, para)
    assert [i.ret for i in infos] == [CONV, CONV, CONV, ALREADY] and infos[3].iterations == 0
    Y = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda")
    A.ata_multi(M, Y); api.synchronize()
    r = (Y - B).cpu().numpy()
    assert np.linalg.norm(r[:, 0]) <= 1e-4 * np.linalg.norm(B[:, 0].cpu().numpy())
    Mh = np.zeros((n, 4))
    infos_h = api.csr_normal_lcg_multi(A, Mh, B.cpu().numpy(), para)
    assert [i.ret for i in infos_h] == [CONV, CONV, CONV, ALREADY]
    assert np.linalg.norm(Mh[:, 0] - M[:, 0].cpu().numpy()) <= 1e-4 * np.linalg.norm(Mh[:, 0])
    low, hig = _bounds(S)
    Mb = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    box = api.csr_normal_solver_constrained_multi(A, Mb, B, dev(low), dev(hig), api.lcg_default_parameters(max_iterations=12, **BOX_RULE), api.LCG_SPG)
    assert [i.ret for i in box][3] == ALREADY and all(i.products >= 1 for i in box) and float(Mb.max()) <= 1.7
    # b = K^T d, the single products, the queries
    d = torch.from_numpy(X.kx(S, S["xt"])).cuda()
    b = torch.empty(n, dtype=torch.float64, device="cuda")
    A.spmv_t(d, b); api.synchronize()
    np.testing.assert_allclose(b.cpu().numpy(), S["b"], rtol=0, atol=1e-12 * np.abs(S["b"]).max())
    y = torch.empty_like(b)
    A.ata(dev(S["xt"]), y); api.synchronize()
    np.testing.assert_allclose(y.cpu().numpy(), S["b"], rtol=0, atol=1e-12 * np.abs(S["b"]).max())
    assert A.n_cols == n and A.normal_info()["longest_column"] == int(np.diff(S["rpT"]).max())
    U = dev(np.ones((n, 4)))
    dots = A.ata_multi_dot(M, Y, U); api.synchronize()
    np.testing.assert_allclose(dots, Y.cpu().numpy().sum(axis=0), rtol=1e-10, atol=1e-10)
    T = torch.empty((S["m"], 4), dtype=torch.float64, device="cuda")
    A.spmm(M, T)
    Y2 = torch.empty_like(Y)
    A.spmm_t(T, Y2); api.synchronize()
    assert np.array_equal(bits(Y2.cpu().numpy()), bits(Y.cpu().numpy()))


def test_sample_program_runs():
    from test_dropin_cpp import _build
    exe = _build("sample_csr_normal")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "one lcg_hip_csr_normal_lcg_multi, iterations:" in p.stdout and "CG through lcg_hip_csr_ata_ax" in p.stdout
