"""-m gpu: solvers on a real dense matrix stored in fp32 (lcg_hip_dense_create_f32) against the fp64 handle of the widened matrix: the
return code, the iteration count, the reported residual and the iterate are the twin's, bit for bit -- the single-vector loops through
the callbacks lcg_hip_dense_ata_ax, lcg_hip_dense_ax and lcg_hip_dense_jacobi_mx, and the batched loops lcg_hip_dense_lcg_multi,
lcg_hip_dense_lpcg_multi and lcg_hip_dense_solver_constrained_multi at k = 2, 4, 8.  One run is anchored on liblcg's own loop
(tests/dense_multi_cases.py: oracle) so that the pair cannot drift together.

Systems: tests/dense_multi_cases.py's, cast to float32 first: K32 = system["K"].astype(float32), the twin and every reference work on
K32.astype(float64), b is made from that matrix."""
import numpy as np
import pytest

import dense_checker as dc
import dense_f32_cases as X
import dense_multi_cases as mc
import multi_box_cases as bx
from dense_multi_cases import CG, MAXIT, NOPRE, PCG, bits, rel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = 1e-10
KS = X.KS
_SYSTEMS = {}


def fsystem(m, n, normal=True):
    """dense_multi_cases.system(m, n, normal) on the float-cast matrix: dict(K (the widened matrix), K32, xt, b, normal, n, key)."""
    key = ("f32", m, n, normal)
    if key not in _SYSTEMS:
        S = mc.system(m, n, normal)
        K32 = S["K"].astype(np.float32)
        K = X.twin(K32)
        b = dc.ata(K, S["xt"]) if normal else dc.matvec(K, S["xt"])
        _SYSTEMS[key] = dict(K=K, K32=K32, xt=S["xt"], b=b, normal=normal, n=n, key=key)
    return _SYSTEMS[key]


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib(api):
    return api.L.load()


@pytest.fixture(scope="module")
def pairs(api):
    """(m, n, normal) -> (the fp32 handle, the fp64 twin), both with the Jacobi reciprocals of their operator."""
    made = {}

    def get(m, n, normal=True):
        key = (m, n, normal)
        if key not in made:
            S = fsystem(m, n, normal)
            F, D = api.DenseMatrix.from_array_f32(S["K32"]), api.DenseMatrix.from_array(S["K"])
            F.build_jacobi(normal); D.build_jacobi(normal)
            assert (F.value_bytes, D.value_bytes) == (4, 8)
            made[key] = (F, D)
        return made[key]
    yield get
    for F, D in made.values():
        F.destroy(); D.destroy()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def single(api, H, kind, S, cap, eps, ax="lcg_hip_dense_ata_ax"):
    """One single-vector solve from zeros on device vectors: ((ret, iterations, residual bits), the iterate)."""
    n = S["n"]
    para = api.lcg_default_parameters(epsilon=eps, abs_diff=0, max_iterations=cap)
    m, b = torch.zeros(n, dtype=torch.float64, device="cuda"), dev(S["b"])
    if kind == "pcg":
        info = api.lcg_solver_preconditioned(ax, "lcg_hip_dense_jacobi_mx", None, m, b, n, para, H)
    elif kind in ("pg", "spg"):
        lo, hi = dev(np.full(n, 1.0)), dev(np.full(n, 2.0))
        info = api.lcg_solver_constrained(ax, None, m, b, lo, hi, n, para, H, api.LCG_PG if kind == "pg" else api.LCG_SPG)
    else:
        info = api.lcg_solver(ax, None, m, b, n, para, H, {"cg": api.LCG_CG, "cgs": api.LCG_CGS, "bicgstab": api.LCG_BICGSTAB}[kind])
    api.synchronize()
    return (info.ret, info.iterations, np.float64(info.residual).view(np.uint64)), m.cpu().numpy()


def same_single(api, F, D, kind, S, cap, eps, ax="lcg_hip_dense_ata_ax"):
    (rf, xf), (rd, xd) = single(api, F, kind, S, cap, eps, ax), single(api, D, kind, S, cap, eps, ax)
    assert rf == rd, (S["key"], kind, cap, rf, rd)
    assert np.array_equal(bits(xf), bits(xd)), (S["key"], kind, cap, "iterates differ in", int((bits(xf) != bits(xd)).sum()), "values")
    assert rd[1] > 0 and np.isfinite(xd).all() and xd.any(), (S["key"], kind, cap, rd)     # the twin did run
    return rd, xd


@pytest.mark.parametrize("shape", [(100, 80), (300, 240)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_vector_solvers_through_the_normal_equations_callback(api, pairs, shape):
    F, D = pairs(*shape)
    S = fsystem(*shape)
    for kind in ("cg", "cgs", "bicgstab", "pcg", "pg", "spg"):
        for cap in (5, 20):
            same_single(api, F, D, kind, S, cap, EPS)
    # every forced K^T.K.x form, and the row forms under the two-pass one
    for variant in X.accepted(*shape)[1:]:
        F.set_kernel(variant); D.set_kernel(variant)
        same_single(api, F, D, "cg", S, 5, EPS)
        assert F.last_kernel == D.last_kernel
    F.set_kernel(0); D.set_kernel(0)


def test_cg_to_convergence(api, pairs):
    F, D = pairs(300, 240)
    (ret, its, _), x = same_single(api, F, D, "cg", fsystem(300, 240), 600, EPS)
    assert ret == 0 and 20 < its < 600 and rel(x, fsystem(300, 240)["xt"]) <= 1e-4


def test_square_operator_through_lcg_hip_dense_ax(api, pairs):
    """dense_multi_cases.system(200, 200, False), cast to float32 and widened for the twin: K itself is the operator."""
    F, D = pairs(200, 200, False)
    S = fsystem(200, 200, False)
    assert np.array_equal(S["K32"], S["K32"].T)
    for kind in ("cg", "pcg", "bicgstab"):
        for cap in (5, 20):
            same_single(api, F, D, kind, S, cap, EPS, ax="lcg_hip_dense_ax")
    # (the stop rule |g|^2 / max(|m|^2, 1) <= 1e-10 leaves a residual of 1e-5 |m|; cond(K) is below 10, so the error is below 1e-4 |m|)
    (ret, its, _), x = same_single(api, F, D, "cg", S, 600, EPS, ax="lcg_hip_dense_ax")
    assert ret == 0 and rel(x, S["xt"]) <= 1e-4


def _same_batch(a, b, tag):
    assert a[0] == b[0] == 0, (tag, a[0], b[0])
    for u, v in zip(a[1:-1], b[1:-1]):          # ret, iterations, (products,) residual: per column
        if isinstance(u[0], float):
            assert np.array_equal(bits(np.array(u)), bits(np.array(v))), (tag, u, v)
        else:
            assert u == v, (tag, u, v)
    assert np.array_equal(bits(a[-1]), bits(b[-1])), (tag, "iterates differ in", int((bits(a[-1]) != bits(b[-1])).sum()), "values")


SHAPES = [(300, 240, True), (200, 200, False)] + [(m, n, True) for m, n in mc.EDGES]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-normal{int(s[2])}")
def test_batched_solvers(lib, api, pairs, shape):
    m, n, normal = shape
    F, D = pairs(m, n, normal)
    S = fsystem(m, n, normal)
    low, hig = np.full(n, 1.0), np.full(n, 2.0)
    for k in KS:
        B = mc.columns(S, k)
        Z = np.zeros((n, k))
        for cap in (5, 20):
            for sid in (CG, PCG):
                a = mc.multi(lib, api, sid, F, normal, Z, B, epsilon=EPS, max_iterations=cap)
                b = mc.multi(lib, api, sid, D, normal, Z, B, epsilon=EPS, max_iterations=cap)
                _same_batch(a, b, (shape, k, cap, sid))
                assert b[2][0] > 0 and np.isfinite(b[4][:, 0]).all() and b[4][:, 0].any(), (shape, k, cap, sid, b[1], b[2])
            for sid in (bx.PG, bx.SPG):
                a = bx.solve(lib, api, sid, F, Z, B, low, hig, normal=int(normal), epsilon=EPS, max_iterations=cap)
                b = bx.solve(lib, api, sid, D, Z, B, low, hig, normal=int(normal), epsilon=EPS, max_iterations=cap)
                _same_batch(a, b, (shape, k, cap, "box", sid))
                assert (b[5] >= 1.0).all() and (b[5] <= 2.0).all() and b[3][0] >= 1, (shape, k, cap, sid, b[1], b[2], b[3])
    if (m, n) == (300, 240):        # to convergence, and the host-memory path
        B = mc.columns(S, 4)
        for sid in (CG, PCG):
            a = mc.multi(lib, api, sid, F, normal, np.zeros((n, 4)), B, epsilon=EPS, max_iterations=600)
            b = mc.multi(lib, api, sid, D, normal, np.zeros((n, 4)), B, epsilon=EPS, max_iterations=600)
            _same_batch(a, b, (shape, "converged", sid))
            assert b[1][0] == 0 and rel(b[4][:, 0], S["xt"]) <= 1e-4
            h = mc.multi(lib, api, sid, F, normal, np.zeros((n, 4)), B, mem="host", epsilon=EPS, max_iterations=20)
            d = mc.multi(lib, api, sid, D, normal, np.zeros((n, 4)), B, mem="host", epsilon=EPS, max_iterations=20)
            _same_batch(h, d, (shape, "host", sid))


def test_pcg_without_reciprocals(lib, api):
    S = fsystem(300, 240)
    F, D = api.DenseMatrix.from_array_f32(S["K32"]), api.DenseMatrix.from_array(S["K"])
    B = mc.columns(S, 4)
    Z = np.zeros((240, 4))
    for H in (F, D):
        assert mc.multi(lib, api, PCG, H, True, Z, B, epsilon=EPS, max_iterations=5)[0] == NOPRE
        assert mc.multi(lib, api, CG, H, True, Z, B, epsilon=EPS, max_iterations=5)[0] == 0
    sq = fsystem(200, 200, False)
    Fs, Ds = api.DenseMatrix.from_array_f32(sq["K32"]), api.DenseMatrix.from_array(sq["K"])
    Bs, Zs = mc.columns(sq, 2), np.zeros((200, 2))
    for H in (Fs, Ds):
        H.build_jacobi(True)                    # built for K^T.K, asked for K
        assert mc.multi(lib, api, PCG, H, False, Zs, Bs, epsilon=EPS, max_iterations=5)[0] == NOPRE
        assert mc.multi(lib, api, PCG, H, True, Zs, Bs, epsilon=EPS, max_iterations=5)[0] == 0
    for H in (F, D, Fs, Ds):
        H.destroy()


def test_cg_agrees_with_liblcgs_loop(api, pairs):
    """The anchor: CG on (300, 240), capped at 20, against the oracle's own loop on the widened K (the checker's serial-order product)
    within dense_multi_cases.late_band, as the fp64 dense tests hold their runs to it."""
    F, _ = pairs(300, 240)
    S = fsystem(300, 240)
    ref, alt = mc.oracle(S, CG, S["b"], 20, EPS), mc.oracle(S, CG, S["b"], 20, EPS, serial=False)
    assert ref["ret"] == alt["ret"] == MAXIT and ref["iters"] == alt["iters"] == 20
    (ret, its, _), x = single(api, F, "cg", S, 20, EPS)
    assert ret == MAXIT and its == 20
    band = mc.late_band(ref["x"], alt["x"], S["xt"])
    r = rel(x, ref["x"])
    print(f"fp32 handle, CG capped at 20: rel diff to the oracle {r:.2e}, band {band:.2e}")
    assert r <= band, (r, band)
