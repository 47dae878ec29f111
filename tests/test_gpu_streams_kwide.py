"""-m gpu: the library on a caller's stream, for what tests/test_gpu_streams.py was written before: the dense operators over k right-hand
sides (real and complex128), the complex64 k-wide product and loops, symmetric run stretches, the dense Jacobi build, a dense handle
made from device memory, batched loops with vectors in host memory, and a few older entries that no stream test had run.

The pattern, its premise and the controls are tests/stream_cases.py's, unchanged: run (a) on the library's own stream with the inputs
ready, held to tests/exact_ref.py (exact sums on integer data, per-row bounds on full-mantissa data) or to the loops' properties; run
(b) on the accepted side stream S, entered while a >= 100 ms chain of filler kernels is running on S with the inputs written BEHIND
it.  (b) has (a)'s bytes in every output and every returned scalar, and an entry that the header says only enqueues returns while the
delay is still running.  No tolerance is introduced here.

Only FLOATING data is ever written late.  Row pointers, column indices and everything else a plan's shape is derived from are in
place before the delay starts: stream_cases.nan_fill gives an integer tensor zeros, and a plan that was built from a zeroed pattern
and is later used with the real one indexes by the real one -- that must never be run on a shared machine.

Where run (a) leaves the right intermediate in scratch that the handle owns (DenseMulti::t, DenseMulti::part), the same call with NaN
inputs runs between (a) and (b) (Env.pair's `between`): a launch of run (b) that reads the scratch too early finds NaN there, not run
(a)'s values."""
import ctypes as C
import zlib

import numpy as np
import pytest

import dense_checker as dc
import dense_multi_cases as dm
import dense_multi_cplx_cases as dz
import exact_ref as X
import multi_c64_cases as c6
import multi_cases as mc
import stop_cases as sc
import stream_cases as st
import tri_multi_cases as tm
from test_gpu_dense_multi_cplx_product import col_plan, row_auto, row_plan
from test_gpu_dense_multi_product import _ata_bits, _exact
from test_gpu_sym_runs import P7, P16, plan as sym_plan, rows_for, system as sym_system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KS = (2, 8)
CAP = 6


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def env(api, lib):
    """The calibrated delay and the side stream the controls accepted (stream_cases.make_env)."""
    e = st.make_env(torch, api, lib)
    yield e
    st.close_env(e)


@pytest.fixture(scope="module")
def second(env):
    """A second side stream that runs beside the first (stream_cases.pick_second)."""
    return st.pick_second(env)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def seed_of(*name):
    return zlib.crc32(repr(name).encode())


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def col(Y, j):
    return np.ascontiguousarray(Y[:, j])


def nan_words(a):
    return int(np.isnan(a.view(np.float32 if a.dtype == np.complex64 else np.float64)).sum())


def same_bytes(a, b, tag):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (tag, "differs from the run on the own stream", nan_words(b), "NaN words")


def poison(inputs, call):
    """Env.pair's `between`: the same call with NaN inputs, so that the handle's scratch holds NaN when run (b) starts."""
    def run():
        for d, _ in inputs:
            st.nan_fill(d)
        call()
    return run


def assert_cdot(s, y, u, tag):
    """An unconjugated complex sum s = sum y_i u_i of the kernel's own y, component by component within exact_ref.assert_dot's bound."""
    y, u = y.astype(np.complex128), u.astype(np.complex128)
    X.assert_dot(s.real, np.concatenate([y.real, -y.imag]), np.concatenate([u.real, u.imag]), (tag, "re"))
    X.assert_dot(s.imag, np.concatenate([y.real, y.imag]), np.concatenate([u.imag, u.real]), (tag, "im"))


# ================================================================================================ real dense k-wide products
REAL_SHAPES = [dm.MAIN, (257, 257), (40, 1100)]


def test_the_dense_shapes_reach_their_branches():
    """dense.hpp's row_plan / col_plan (restated in tests/test_gpu_dense_multi_cplx_product.py; a real row holds NP = ceil(N / 2)
    packs, a complex one N): what each shape of this module is there for."""
    m, n = dm.MAIN
    assert row_plan(m, (n + 1) // 2, True, True)["S"] == 7 and col_plan(m, (n + 1) // 2)["RS"] == 10 and row_auto(m, (n + 1) // 2)["S"] == 1
    assert row_auto(40, 550)["S"] >= 2 and 550 >= 512 and 40 < 1024             # the automatic choice splits
    assert row_auto(257, 129)["S"] == 1 and row_plan(257, 129, True, True)["S"] >= 2
    assert row_plan(200, 200, True, True)["S"] == 12 and col_plan(200, 200)["RS"] == 13 and row_auto(200, 200)["S"] == 1
    assert row_plan(65, 65, True, True)["S"] >= 2 and row_auto(65, 65)["S"] == 1


@pytest.mark.parametrize("shape", REAL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_real_dense_block_products(env, api, lib, shape):
    """lcg_hip_dense_matmat (layout 0 automatic, forced row, forced split; layout 1), lcg_hip_dense_ata_multi (automatic, forced
    split) and the three forms of lcg_hip_dense_op_multi_dot at k = 2 and 8, on integer data: run (a) is the exact sum bit for bit.
    The sums of the form that reads back are returned scalars; the two other forms only enqueue."""
    m, n = shape
    square = m == n
    auto_split = row_auto(m, (n + 1) // 2)["S"] > 1
    rng = np.random.default_rng(seed_of("dnm", shape))
    p, pa = X.int_bits(max(m, n)), _ata_bits(m, n)
    K, Ka = X.int_values(rng, (m, n), p), X.int_values(rng, (m, n), pa)
    D, Da = api.DenseMatrix.from_array(K), api.DenseMatrix.from_array(Ka)
    names = api.DenseMatrix.multi_kernel_names()
    assert names == ["k_dnm_row", "k_dnm_row_split", "k_dnm_col", "k_dnm_ata_two_pass"], names
    try:
        for k in KS:
            Xh, Xth, Xah = X.int_values(rng, (n, k), p), X.int_values(rng, (m, k), p), X.int_values(rng, (n, k), pa)
            Uh = X.int_values(rng, (n, k), 4, zeros=0)
            want, want_t, want_a = _exact(K, Xh), _exact(K.T, Xth), _exact(Ka.T, _exact(Ka, Xah))
            Xs, Xts, Xas, Us = dev(Xh), dev(Xth), dev(Xah), dev(Uh)
            Xd, Xtd, Xad, Ud = (torch.empty_like(t) for t in (Xs, Xts, Xas, Us))
            Ym = torch.empty((m, k), dtype=torch.float64, device="cuda")
            Yn = torch.empty((n, k), dtype=torch.float64, device="cuda")

            def held(H, name, exact, tag):
                def anchor(r, outs):
                    assert H.multi_last_kernel == name, (tag, H.multi_last_kernel)
                    X.assert_exact(outs[0], exact, tag)
                return anchor

            for variant in (0, 1, 2):
                D.set_kernel(variant)
                name = names[1] if variant == 2 or (variant == 0 and auto_split) else names[0]
                call = lambda: D.matmat(Xd, Ym, 0)                                     # noqa: E731
                env.pair([(Xd, Xs)], call, [Ym], True, tag=(shape, k, "K.X", variant), anchor=held(D, name, want, (shape, k, "K.X", variant)),
                         between=poison([(Xd, Xs)], call))
            D.set_kernel(0)
            call = lambda: D.matmat(Xtd, Yn, 1)                                        # noqa: E731
            env.pair([(Xtd, Xts)], call, [Yn], True, tag=(shape, k, "K^T.X"), anchor=held(D, names[2], want_t, (shape, k, "K^T.X")),
                     between=poison([(Xtd, Xts)], call))
            for variant in (0, 2):
                Da.set_kernel(variant)
                call = lambda: Da.ata_multi(Xad, Yn)                                   # noqa: E731
                env.pair([(Xad, Xas)], call, [Yn], True, tag=(shape, k, "ata", variant),
                         anchor=held(Da, names[3], want_a, (shape, k, "ata", variant)), between=poison([(Xad, Xas)], call))
            Da.set_kernel(0)
            for H, normal, Xb, Xsrc, exact in [(Da, 1, Xad, Xas, want_a)] + ([(D, 0, Xd, Xs, want)] if square else []):
                tag = (shape, k, "op_multi_dot", normal)
                both = [(Xb, Xsrc), (Ud, Us)]

                def read_out():
                    return H.op_multi_dot(Xb, Yn, Ud, normal=bool(normal))

                def enqueue(U):
                    def run():
                        assert lib.lcg_hip_dense_op_multi_dot(H.h, k, normal, Xb.data_ptr(), Yn.data_ptr(), U.data_ptr() if U is not None else None,
                                                              None) == 0, lib.lcg_hip_last_error()
                    return run

                def anchor(r, outs):
                    X.assert_exact(outs[0], exact, tag)
                    if r is not None:
                        for j in range(k):
                            X.assert_dot(r[j], col(outs[0], j), col(Uh, j), (tag, j))
                env.pair(both, read_out, [Yn], False, tag=(tag, "U and dots"), anchor=anchor, between=poison(both, read_out))
                env.pair(both, enqueue(Ud), [Yn], True, tag=(tag, "U, dots = NULL"), anchor=anchor, between=poison(both, enqueue(Ud)))
                env.pair([(Xb, Xsrc)], enqueue(None), [Yn], True, tag=(tag, "U = NULL"), anchor=anchor, between=poison([(Xb, Xsrc)], enqueue(None)))
    finally:
        D.destroy(); Da.destroy()


def test_dense_work_memory_regrows_on_a_side_stream(env, api, lib):
    """dnm_reserve at a larger k synchronises, frees and allocates.  A fresh handle that has only ever run k = 2 makes its first
    k = 8 product (lcg_hip_dense_ata_multi) on S behind the delay: the bytes of a warmed handle's own-stream run; and the k = 2 product
    that follows has the bytes it had before the regrow."""
    m, n = dm.MAIN
    rng = np.random.default_rng(seed_of("regrow"))
    pa = _ata_bits(m, n)
    Ka = X.int_values(rng, (m, n), pa)
    X8, X2 = X.int_values(rng, (n, 8), pa), X.int_values(rng, (n, 2), pa)
    X8s, X2s = dev(X8), dev(X2)
    X8d, X2d = torch.empty_like(X8s), torch.empty_like(X2s)
    Y8, Y2 = torch.empty_like(X8s), torch.empty_like(X2s)
    W, F = api.DenseMatrix.from_array(Ka), api.DenseMatrix.from_array(Ka)
    try:
        W.set_kernel(2); F.set_kernel(2)
        _, o8 = env.pair([(X8d, X8s)], lambda: W.ata_multi(X8d, Y8), [Y8], True, tag="warmed, k = 8",
                         anchor=lambda r, o: X.assert_exact(o[0], _exact(Ka.T, _exact(Ka, X8)), "k = 8"))
        _, o2 = env.pair([(X2d, X2s)], lambda: W.ata_multi(X2d, Y2), [Y2], True, tag="warmed, k = 2",
                         anchor=lambda r, o: X.assert_exact(o[0], _exact(Ka.T, _exact(Ka, X2)), "k = 2"))
        _, f2 = env.reference([(X2d, X2s)], lambda: F.ata_multi(X2d, Y2), [Y2])
        same_bytes(o2[0], f2[0], "the fresh handle at k = 2, before the regrow")
        _, f8 = env.late([(X8d, X8s)], lambda: F.ata_multi(X8d, Y8), [Y8], enqueue_only=False)
        same_bytes(o8[0], f8[0], "the first k = 8 product of a handle that had only run k = 2, on the side stream")
        _, g2 = env.late([(X2d, X2s)], lambda: F.ata_multi(X2d, Y2), [Y2], enqueue_only=True)
        same_bytes(o2[0], g2[0], "k = 2 after the regrow")
    finally:
        W.destroy(); F.destroy()


def test_dense_handle_made_from_device_memory_written_late(env, api, lib):
    """lcg_hip_dense_create from a CUDA tensor: the handle is created inside the pattern, its copy of K is made on S behind the late
    write, and a product on it is the exact sum."""
    m, n, k = 37, 29, 2
    rng = np.random.default_rng(seed_of("from device"))
    p = X.int_bits(max(m, n))
    K, Xh = X.int_values(rng, (m, n), p), X.int_values(rng, (n, k), p)
    Ks, Xs = dev(K), dev(Xh)
    Kd, Xd = torch.empty_like(Ks), torch.empty_like(Xs)
    Y = torch.empty((m, k), dtype=torch.float64, device="cuda")
    made = []

    def call():
        made.append(api.DenseMatrix.from_array(Kd))
        made[-1].matmat(Xd, Y, 0)
    try:
        env.pair([(Kd, Ks), (Xd, Xs)], call, [Y], False, tag="dense_create from device memory",
                 anchor=lambda r, o: X.assert_exact(o[0], _exact(K, Xh), "from device memory"))
        assert len(made) == 2
    finally:
        for D in made:
            D.destroy()


@pytest.mark.parametrize("normal", [True, False], ids=["normal", "diagonal"])
def test_dense_jacobi_built_on_a_side_stream(env, api, lib, normal):
    """lcg_hip_dense_build_jacobi launches, reads back, writes diag_out and uploads the reciprocals, all on the stream: entered
    while the delay runs, diag_out cloned on S and a following lcg_hip_dense_jacobi_mx of a vector written late have the own-stream
    bytes -- the exact diagonal and x times its stored reciprocal."""
    m, n = dm.MAIN if normal else (257, 257)
    rng = np.random.default_rng(seed_of("dense jacobi", normal))
    K = X.int_values(rng, (m, n), _ata_bits(m, n))
    if not normal:
        K[np.arange(n), np.arange(n)] = rng.integers(1, 9, n) * rng.choice([-1.0, 1.0], n)
    d = (K.astype(np.int64) ** 2).sum(0).astype(np.float64) if normal else np.diag(K).copy()
    assert np.all(d != 0)
    x = X.int_values(rng, n, 8)
    xs = dev(x); xd, y, diag = torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs)
    D = api.DenseMatrix.from_array(K)
    try:
        def call():
            D.build_jacobi(normal, diag)
            lib.lcg_hip_dense_jacobi_mx(D.h, xd.data_ptr(), y.data_ptr(), n)

        def anchor(r, o):
            X.assert_exact(o[1], d, "the diagonal")
            X.assert_exact(o[0], (1.0 / d) * x, "x over the diagonal, as the stored reciprocal times x")
        env.pair([(xd, xs)], call, [y, diag], False, tag=("dense jacobi", normal), anchor=anchor)
    finally:
        D.destroy()


# ================================================================================================ complex dense k-wide products
ZFORMS = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (0, 1, 1), (0, 0, 2), (0, 1, 2)]       # (layout, conjugate, variant)


@pytest.mark.parametrize("n", [200, 65])
def test_complex_dense_block_products(env, api, lib, n):
    """clcg_hip_dense_matmat in its four forms, layout 0 also under the forced row and split forms, clcg_hip_dense_op_multi_dot with
    the read-out and with dots = NULL, and the single-vector clcg_hip_dense_matvec, on dense_multi_cplx_cases.system(n): every column of
    run (a) within exact_ref's per-row bound."""
    S = dz.system(n)
    K = S["K"]
    D = api.DenseMatrix.from_array(K)
    names = api.DenseMatrix.cmulti_kernel_names()
    assert names == dz.NAMES
    csr = {}
    for layout, conj in {(f[0], f[1]) for f in ZFORMS}:
        A = K.conj() if conj else K
        csr[layout, conj] = dc.dense_as_csr(np.ascontiguousarray(A.T if layout else A))
    try:
        for k in KS:
            rng = np.random.default_rng(seed_of("zdnm", n, k))
            Xh, Uh = crand(rng, n, k), crand(rng, n, k)
            Xs, Us = dev(Xh), dev(Uh)
            Xd, Ud, Y = torch.empty_like(Xs), torch.empty_like(Us), torch.empty_like(Xs)

            def rows(form, outs, tag):
                for j in range(k):
                    X.assert_rows(col(outs[0], j), *csr[form], col(Xh, j), (tag, j))

            for layout, conj, variant in ZFORMS:
                D.set_kernel(variant)
                name = names[2] if layout else names[variant - 1 if variant else 0]
                tag = ("zdnm", n, k, layout, conj, variant)

                def anchor(r, outs):
                    assert D.multi_last_kernel == name, (tag, D.multi_last_kernel)
                    rows((layout, conj), outs, tag)
                call = lambda: D.cmatmat(Xd, Y, layout, conj)                          # noqa: E731
                env.pair([(Xd, Xs)], call, [Y], True, tag=tag, anchor=anchor, between=poison([(Xd, Xs)], call))
            D.set_kernel(0)
            both = [(Xd, Xs), (Ud, Us)]

            def anchor_dot(r, outs):
                rows((0, 0), outs, ("zdnm op", n, k))
                if r is not None:
                    for j in range(k):
                        assert_cdot(r[j], col(outs[0], j), col(Uh, j), ("zdnm op", n, k, j))
            read_out = lambda: D.cop_multi_dot(Xd, Y, Ud)                              # noqa: E731

            def enqueue():
                assert lib.clcg_hip_dense_op_multi_dot(D.h, k, Xd.data_ptr(), Y.data_ptr(), Ud.data_ptr(), None) == 0, lib.lcg_hip_last_error()
            _, oa = env.pair(both, read_out, [Y], False, tag=("zdnm op", n, k, "dots"), anchor=anchor_dot, between=poison(both, read_out))
            _, ob = env.pair(both, enqueue, [Y], True, tag=("zdnm op", n, k, "dots = NULL"), anchor=anchor_dot, between=poison(both, enqueue))
            same_bytes(oa[0], ob[0], "the operator with and without the read-out")
        rng = np.random.default_rng(seed_of("zdn", n))
        xh = crand(rng, n)
        xs = dev(xh); xd, y = torch.empty_like(xs), torch.empty_like(xs)
        for layout, conj in ((0, 0), (1, 1)):
            env.pair([(xd, xs)], lambda: D.matvec(xd, y, layout, conj), [y], True, tag=("zdn matvec", n, layout, conj),
                     anchor=lambda r, o: X.assert_rows(o[0], *csr[layout, conj], xh, ("zdn matvec", n, layout, conj)))
    finally:
        D.destroy()


# ================================================================================================ complex64 k-wide products
C64_SYSTEMS = {("helmholtz", 40): (64, 25), ("helm", 182): (64, 518), ("band140", 2051): (4, 513)}     # key -> (rows per block, blocks)


@pytest.mark.parametrize("key", list(C64_SYSTEMS), ids=lambda k: f"{k[0]}-{k[1]}")
def test_complex64_block_products(env, api, lib, key):
    """clcg_hip_spmm_c64 (only enqueues) and clcg_hip_spmm_dot_c64 (reads back) at k = 2 and 8: 25 blocks of 64 rows, 518 blocks (more
    than MM_MG: the temporary table and the fold launch) and 513 blocks of 4 rows.  Run (a): every column within the per-row fp32
    bound of tests/test_gpu_multi_c64_product.py (multi_c64_cases.row_bound), the sums within exact_ref.assert_dot's."""
    S = c6.system(*key)
    n, rp, ci, v = S["n"], S["rp"], S["ci"], S["v"]
    R = mc.rows_per_block(float(rp[-1]) / n)
    blocks = -(-n // R)
    assert (R, blocks) == C64_SYSTEMS[key] and (blocks > mc.MM_MG) == (key[0] != "helmholtz"), (key, R, blocks)
    lens = np.diff(rp)
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    try:
        for k in KS:
            rng = np.random.default_rng(seed_of("c64mm", key, k))
            Xh, Uh = crand(rng, n, k).astype(np.complex64), crand(rng, n, k).astype(np.complex64)
            refs = [X.hp_product(rp, ci, v.astype(np.complex128), col(Xh, j).astype(np.complex128)) for j in range(k)]
            Xs, Us = dev(Xh), dev(Uh)
            Xd, Ud, Y = torch.empty_like(Xs), torch.empty_like(Us), torch.empty_like(Xs)

            def anchor(r, outs):
                for j in range(k):
                    err = X.row_errors(col(outs[0], j).astype(np.complex128), refs[j])
                    bound = c6.row_bound(lens, R, refs[j][2])
                    assert np.all(err <= bound), (key, k, j, float(np.max(err / bound)))
                    if r is not None:
                        assert_cdot(r[j], col(outs[0], j), col(Uh, j), (key, k, j))
            _, oa = env.pair([(Xd, Xs)], lambda: A.cspmm_c64(Xd, Y), [Y], True, tag=("cspmm_c64", key, k), anchor=anchor)
            _, ob = env.pair([(Xd, Xs), (Ud, Us)], lambda: A.cspmm_dot_c64(Xd, Y, Ud), [Y], False, tag=("cspmm_dot_c64", key, k), anchor=anchor)
            same_bytes(oa[0], ob[0], (key, k, "the product carrying the sums against the plain one"))
    finally:
        A.destroy()


# ================================================================================================ symmetric run stretches
SYM = {"7 pairs": (P7, -64), "16 pairs": (P16, 0)}      # offsets, and the kernel variant of the spmv_dot case (0: the dot rides in the product)
_SYM = {}


def mirrored_ints(n, rp, ci, p, salt):
    """Integer values in [-2^p, 2^p] that depend on the unordered pair (row, column) alone: A(i, j) == A(j, i) bit for bit."""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    lo, hi = np.minimum(rows, ci), np.maximum(rows, ci.astype(np.int64))
    return ((lo * 2654435761 + hi * 40503 + salt * 97) % (2 ** (p + 1) + 1) - 2 ** p).astype(np.float64)


def sym_case(name):
    """(n, rowptr, col, p): the smallest system of these offsets with a sliced range, an apron and a partial last block; p bits keep
    the product and the sums y.u, y.y exact (tests/test_gpu_exact_products.py: dot_data)."""
    if name not in _SYM:
        offs = SYM[name][0]
        n = rows_for(offs, 1)
        rp, ci, _ = sym_system(n, offs, np.random.default_rng(1))
        q = (52 - int(np.ceil(np.log2(n)))) // 2
        p = (q - int(np.ceil(np.log2(2 * len(offs) + 1)))) // 2
        assert p >= 4 and n % 64 != 0
        _SYM[name] = (n, rp, ci, p)
    return _SYM[name]


def sym_setup(api, lib, A, nx, variant=-64):
    A.set_kernel(variant)
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    A.set_sym_runs(1, nx)


def sym_reached(lib, A, name, nx, carried=False):
    kern = lib.lcg_hip_csr_last_kernel(A.h).decode()
    took = A.sym_runs()
    n = sym_case(name)[0]
    assert "k_spmv_ldsp_sym" in kern and (not carried or "carrying the dot" in kern), (name, nx, kern)
    assert took == (nx, nx * sym_plan(n, SYM[name][0], nx)[4], "taken"), (name, nx, took)


def test_the_symmetric_systems_are_the_smallest_of_their_kind():
    assert sym_case("7 pairs")[0] == 1379 and sym_case("16 pairs")[0] > 1379
    for name, (offs, _) in SYM.items():
        b0, b1, Q, inner0, S = sym_plan(sym_case(name)[0], offs, 8)
        assert S == 1 and Q >= 2 and (b0 + Q) % 8 != 0


@pytest.mark.parametrize("nx", [1, 8])
@pytest.mark.parametrize("name", list(SYM))
def test_symmetric_run_stretch_family(env, api, lib, name, nx):
    """test_gpu_streams.test_real_product_families' pattern for the family it has not got: lcg_hip_spmv from the half store
    (k_spmv_ldsp_sym plus the skipping k_spmv_ldsp launch), mirrored integer values, the exact sum.  A warmed handle only enqueues; a
    fresh handle whose first product -- the plan build, the mirror check, the pack and both launches -- happens on S has the same
    bytes."""
    n, rp, ci, p = sym_case(name)
    rng = np.random.default_rng(seed_of("sym", name, nx))
    val = mirrored_ints(n, rp, ci, p, nx)
    x = X.int_values(rng, n, p, zeros=0.02)
    exact = X.exact_int_product(rp, ci, val, x)
    xs = dev(x); xd, y = torch.empty_like(xs), torch.empty_like(xs)
    A, F = api.CsrMatrix.from_csr(rp, ci, val), api.CsrMatrix.from_csr(rp, ci, val)
    try:
        sym_setup(api, lib, A, nx); sym_setup(api, lib, F, nx)

        def anchor(r, outs):
            sym_reached(lib, A, name, nx)
            X.assert_exact(outs[0], exact, (name, nx, "own stream"))
        _, oa = env.pair([(xd, xs)], lambda: A.spmv(xd, y), [y], True, tag=("sym", name, nx), anchor=anchor)
        sym_reached(lib, A, name, nx)
        _, ob = env.late([(xd, xs)], lambda: F.spmv(xd, y), [y], enqueue_only=False)
        sym_reached(lib, F, name, nx)
        same_bytes(oa[0], ob[0], (name, nx, "a fresh handle whose plan and half store were built on the side stream"))
    finally:
        A.destroy(); F.destroy()


@pytest.mark.parametrize("nx", [1, 8])
@pytest.mark.parametrize("name", list(SYM))
def test_symmetric_run_stretch_carried_dot(env, api, lib, name, nx):
    """lcg_hip_spmv_dot on such handles with u = x and u != x: y and both sums are exact, on S as on the own stream.  7 pairs with
    the kernel forced (product and reduction are two launches), 16 pairs with the automatic choice (the sums ride in the product)."""
    n, rp, ci, p = sym_case(name)
    variant = SYM[name][1]
    rng = np.random.default_rng(seed_of("sym dot", name, nx))
    val = mirrored_ints(n, rp, ci, p, 10 + nx)
    x = X.int_values(rng, n, p, zeros=0.02)
    u = X.int_values(rng, n, 4, zeros=0)
    exact = X.exact_int_product(rp, ci, val, x)
    xs, us = dev(x), dev(u)
    xd, ud, y = torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs)
    A, F = api.CsrMatrix.from_csr(rp, ci, val), api.CsrMatrix.from_csr(rp, ci, val)
    try:
        sym_setup(api, lib, A, nx, variant); sym_setup(api, lib, F, nx, variant)

        def sums(H, up):
            def run():
                out = (C.c_double * 2)()
                assert lib.lcg_hip_spmv_dot(H.h, xd.data_ptr(), y.data_ptr(), up.data_ptr(), out) == 0, lib.lcg_hip_last_error()
                return out[0], out[1]
            return run
        for uname, up, uh, inputs in (("u = x", xd, x, [(xd, xs)]), ("u", ud, u, [(xd, xs), (ud, us)])):
            def anchor(r, outs):
                sym_reached(lib, A, name, nx, carried=variant == 0)
                X.assert_exact(outs[0], exact, (name, nx, uname))
                assert r == (float(np.dot(exact, uh)), float(np.dot(exact, exact))), (name, nx, uname, r)      # integer data: exact sums
            ra, oa = env.pair(inputs, sums(A, up), [y], False, tag=("sym dot", name, nx, uname), anchor=anchor)
            rb, ob = env.late(inputs, sums(F, up), [y], enqueue_only=False)
            sym_reached(lib, F, name, nx, carried=variant == 0)
            assert st.same_scalars(ra, rb), (name, nx, uname, "the other handle, on the side stream", ra, rb)
            same_bytes(oa[0], ob[0], (name, nx, uname, "the other handle, on the side stream"))
    finally:
        A.destroy(); F.destroy()


def _adopted(n, rp, ci):
    """Device arrays for lcg_hip_csr_create(adopt = 2): row pointers and columns in place, 64 readable bytes behind col and val; the
    values' view is what gets written late."""
    pad = 32
    rpd = dev(rp)
    colb = torch.zeros(len(ci) + pad, dtype=torch.int32, device="cuda"); colb[:len(ci)] = dev(ci)
    valb = torch.zeros(len(ci) + pad, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return rpd, colb[:len(ci)], valb[:len(ci)]


def test_symmetric_run_stretch_adopted_values_written_late(env, api, lib):
    """An adopted matrix whose VALUES are written behind the delay (row pointers and columns are ready): the fresh handle's first
    product on S must report "taken" and give the exact sum.  A build that ran anywhere else would see the NaN fill -- identical NaN
    words mirror each other, so it would be "taken" with a NaN half store.  Then the rewrite protocol of include/lcg_hip.h on S: new
    mirrored values written late, lcg_hip_csr_set_packed(A, 0) and (A, 1), and the product follows the new values from a new half
    store.  (What no test through the C ABI can see: the stream of the k_sym_pack launch alone.  sym_runs_build waits for the stream
    twice before that launch -- the offsets and the verdict of the mirror check are read back -- and frees the check's flag behind it,
    which waits for the whole device: wherever the pack runs, it has the final values and is done before the product starts.)"""
    name, nx = "7 pairs", 8
    n, rp, ci, p = sym_case(name)
    rng = np.random.default_rng(seed_of("sym adopted"))
    val, val2 = mirrored_ints(n, rp, ci, p, 21), mirrored_ints(n, rp, ci, p, 22)
    assert not np.array_equal(val, val2)
    x = X.int_values(rng, n, p, zeros=0.02)
    rpd, cold, vald = _adopted(n, rp, ci)
    vs, vs2, xs = dev(val), dev(val2), dev(x)
    xd, y = torch.empty_like(xs), torch.empty_like(xs)
    handles = []

    def fresh():
        A = api.CsrMatrix.from_csr(rpd, cold, vald, adopt=2)
        sym_setup(api, lib, A, nx)
        handles.append(A)
        A.spmv(xd, y)
        return A.sym_runs(), "k_spmv_ldsp_sym" in lib.lcg_hip_csr_last_kernel(A.h).decode()

    def rewritten():
        A = handles[-1]
        assert lib.lcg_hip_csr_set_packed(A.h, 0) == 0 and lib.lcg_hip_csr_set_packed(A.h, 1) == 0
        A.spmv(xd, y)
        return A.sym_runs(), "k_spmv_ldsp_sym" in lib.lcg_hip_csr_last_kernel(A.h).decode()

    def held(v, tag):
        def anchor(r, outs):
            assert r == ((nx, nx, "taken"), True), (tag, r)
            X.assert_exact(outs[0], X.exact_int_product(rp, ci, v, x), tag)
        return anchor
    try:
        env.pair([(vald, vs), (xd, xs)], fresh, [y], False, tag="adopted, values late", anchor=held(val, "adopted, own stream"))
        assert len(handles) == 2

        def back_to_the_first_values():         # so that run (b), too, starts from a half store that holds OTHER values
            vald.copy_(vs); xd.copy_(xs)
            torch.cuda.synchronize()
            assert rewritten() == ((nx, nx, "taken"), True)
            api.synchronize()
            X.assert_exact(y.cpu().numpy(), X.exact_int_product(rp, ci, val, x), "back to the first values")
        env.pair([(vald, vs2), (xd, xs)], rewritten, [y], False, tag="values rewritten", anchor=held(val2, "rewritten, own stream"),
                 between=back_to_the_first_values)
    finally:
        torch.cuda.synchronize()
        for A in handles:
            A.destroy()


def test_symmetric_run_stretch_capped_cg(env, api, lib, port):
    """One CG solve capped at 6 iterations on the 16-pair system through Bench.solve (tests/test_gpu_stop_contract.py), b and the
    guess written late: verdict, count, residual and iterate are the own-stream bytes, and the loop's product ran from the half store."""
    import test_gpu_stop_contract as T
    n = rows_for(P16, 1)
    rng = np.random.default_rng(seed_of("sym cg"))
    rp, ci, val = sym_system(n, P16, rng)
    xt = rng.standard_normal(n)
    S = {"n": n, "rp": rp, "ci": ci, "v": val, "xt": xt, "b": rng.standard_normal(n)}
    B = T.Bench(api, lib, port, sc.BY_NAME["cg_auto"], n, S)
    try:
        sym_setup(api, lib, B.A, 8, 0)
        a = st.bench_solve(env, T, B, late=False, cap=CAP)
        assert (a["ret"], a["iters"]) == (T.CAP, CAP), (a["ret"], a["iters"])
        kern = lib.lcg_hip_csr_last_kernel(B.A.h).decode()
        assert "k_spmv_ldsp_sym" in kern and B.A.sym_runs()[2] == "taken", (kern, B.A.sym_runs())
        st.no_nan([a["x"]])
        b = st.bench_solve(env, T, B, late=True, cap=CAP)
        st.same_solve(a, b, "CG on a symmetric run stretch")
    finally:
        B.A.destroy()


# ================================================================================================ batched loops of the new families
def _loop_cases():
    out = []
    for loop in ("dense_lcg_multi", "dense_lpcg_multi"):
        out += [(loop, ("normal",) + dm.MAIN), (loop, ("spd", 200, 200))]
    for loop in ("zdense_lbicg_sym_multi", "zdense_lpcg_multi"):
        out += [(loop, ("zdense", 200)), (loop, ("zdense", 65))]
    for loop in ("lbicg_sym_multi_c64", "lpcg_multi_c64"):
        out += [(loop, ("helmholtz", 40)), (loop, ("helm", 182))]
    return out


LOOP_CASES = _loop_cases()


@pytest.mark.parametrize("loop,key", LOOP_CASES, ids=[f"{l}-{'-'.join(map(str, k))}" for l, k in LOOP_CASES])
def test_batched_loops_of_the_new_families(env, api, lib, loop, key):
    """test_gpu_streams.test_batched_loops' pattern for the loops it has not got, at k = 2 and 8, capped at 6 and converged (epsilon
    and cap as each family's own tests), M and B written late: per column code, count, residual and the iterate are identities.
    Run (a): no NaN, every column answered, column 0 converges when the run is not capped at 6, max(its) == 6 when it is."""
    pcg = "lpcg" in loop
    if loop.startswith("dense"):
        normal = key[0] == "normal"
        S = dm.system(key[1], key[2], normal)
        H = api.DenseMatrix.from_array(S["K"])
        if pcg:
            H.build_jacobi(normal)
        fn = lib.lcg_hip_dense_lpcg_multi if pcg else lib.lcg_hip_dense_lcg_multi
        lead = lambda k: (H.h, k, int(normal))                                         # noqa: E731
        para_of = lambda cap: api.lcg_default_parameters(max_iterations=cap or 600, epsilon=1e-10, abs_diff=0)      # noqa: E731
        blocks = lambda k: (dm.columns(S, k), np.zeros((S["n"], k)))                   # noqa: E731
    elif loop.startswith("zdense"):
        S = dz.system(key[1])
        H = api.DenseMatrix.from_array(S["K"])
        if pcg:
            H.build_jacobi(False)
        fn = lib.clcg_hip_dense_lpcg_multi if pcg else lib.clcg_hip_dense_lbicg_sym_multi
        lead = lambda k: (H.h, k)                                                      # noqa: E731
        para_of = lambda cap: api.clcg_default_parameters(max_iterations=cap or 600, epsilon=1e-10, abs_diff=1)     # noqa: E731
        blocks = lambda k: (dz.columns(S, k), np.zeros((S["n"], k), np.complex128))    # noqa: E731
    else:
        S = c6.system(*key)
        H = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"])
        if pcg:
            H.build_jacobi()
        fn = lib.clcg_hip_lpcg_multi_c64 if pcg else lib.clcg_hip_lbicg_sym_multi_c64
        lead = lambda k: (H.h, k)                                                      # noqa: E731
        para_of = lambda cap: api.clcg_default_parameters(max_iterations=cap or 3000, epsilon=1e-8)                 # noqa: E731
        blocks = lambda k: (c6.columns(S, k), np.zeros((S["n"], k), np.complex64))     # noqa: E731
    try:
        for k in KS:
            Bh, M0 = blocks(k)
            Bs, M0s = dev(Bh), dev(M0)
            Bd, Md = torch.empty_like(Bs), torch.empty_like(M0s)
            for cap in (CAP, 0):
                para = para_of(cap)

                def call():
                    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
                    rc = fn(*lead(k), Md.data_ptr(), Bd.data_ptr(), C.byref(para), ret, its, res, 1)
                    return rc, list(ret), list(its), list(res)

                def anchor(r, outs):
                    rc, ret, its, res = r
                    assert rc == 0 and 99 not in ret and -1 not in its, (loop, key, k, cap, r, lib.lcg_hip_last_error())
                    st.no_nan(outs, (loop, key, k, cap))
                    if cap == 0:        # column 0 (b itself from a zero guess) converges
                        assert ret[0] == 0 and 0 < its[0] < para.max_iterations, (loop, key, k, r)
                    else:
                        assert max(its) == cap, (loop, key, k, r)
                env.pair([(Md, M0s), (Bd, Bs)], call, [Md], False, tag=(loop, key, k, cap), anchor=anchor)
    finally:
        H.destroy()


def test_batched_loops_with_vectors_in_host_memory(env, api, lib):
    """mem = LCG_HIP_MEM_HOST, in the shape of test_gpu_streams.test_host_vectors: lcg_hip_lcg_multi on multi_cases' ("spd", 65) and
    clcg_hip_lpcg_multi_c64 on ("helmholtz", 40) with blocks from aligned_block, entered while the delay runs on S.  The library
    copies in and out on its stream: codes, counts, residuals and the iterate equal the own-stream run's."""
    S = mc.system("spd", 65)
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    try:
        run = lambda: mc.multi(lib, api, mc.CG, A, mc.guesses(S, 4), mc.columns(S["n"], S["b"], 4), mem="host", max_iterations=600, **mc.RULES["abs"])       # noqa: E731
        ra, _ = env.reference([], run, [])
        assert ra[0] == 0 and ra[1][0] == 0 and 99 not in ra[1] and ra[2][0] > 0 and not np.isnan(ra[4]).any(), ra[:4]
        rb, _ = env.late([], run, [], enqueue_only=False)
        assert st.same_scalars(ra, rb), ("lcg_hip_lcg_multi, host memory", ra[:4], rb[:4], nan_words(rb[4]), "NaN words")
    finally:
        A.destroy()
    S = c6.system("helmholtz", 40)
    A = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"])
    try:
        A.build_jacobi()
        run = lambda: c6.cmulti64(lib, api, c6.PCG, A, np.zeros((S["n"], 4), np.complex64), c6.columns(S, 4), mem="host", epsilon=1e-8, max_iterations=3000)  # noqa: E731
        ra, _ = env.reference([], run, [])
        assert ra[0] == 0 and ra[1] == [c6.CONV, c6.CONV, c6.CONV, c6.ALREADY] and nan_words(ra[4]) == 0, ra[:4]
        rb, _ = env.late([], run, [], enqueue_only=False)
        assert st.same_scalars(ra, rb), ("clcg_hip_lpcg_multi_c64, host memory", ra[:4], rb[:4], nan_words(rb[4]), "NaN words")
    finally:
        A.destroy()


# ================================================================================================ switches over k-wide scratch
def _switch(env, api, S2, first, then, outputs, late_input, ref_names, after=None):
    """test_gpu_streams.test_switch_between_two_applies_of_one_factor's shape.  The own-stream run of first(), then() and after() is
    the reference (the caller anchors it); then on S1 the delay, the late input and first(); the switch to S2 and then(), which must
    return with the delay still running; after() on S2 (an entry that reads back: it may wait); clones on S2.  Asserts the identities
    and returns (the reference's outputs, what after() returned there)."""
    torch = env.torch
    S1 = env.need_stream()
    d, s = late_input
    d.copy_(s)
    torch.cuda.synchronize()
    first(); then()
    ra = after() if after else None
    api.synchronize(); torch.cuda.synchronize()
    ref = [t.cpu().numpy().copy() for t in outputs]
    for t in [d] + list(outputs):
        st.nan_fill(t)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(S1):
            api.use_torch_stream()
            E = env.delay.enqueue()
            d.copy_(s, non_blocking=True)
            assert not E.query(), st.PREMISE
            first()
        with torch.cuda.stream(S2):
            api.use_torch_stream()          # S1 -> S2
            then()
            assert not E.query(), "the switch or the call behind it drained the first stream"
            rb = after() if after else None
            got = [t.clone() for t in outputs]
            S2.synchronize()
        got = [t.cpu().numpy() for t in got]
    finally:
        api.use_own_stream()
        S1.synchronize()
    assert st.same_scalars(ra, rb), ("what the entry behind the switch read back", ra, rb)
    for name, a, b in zip(ref_names, ref, got):
        same_bytes(a, b, name)
    return ref, ra


def test_switch_between_two_real_dense_products_of_one_handle(env, api, lib, second):
    """300 x 240, the forced split, k = 8: lcg_hip_dense_ata_multi of a block written late on S1, the switch, the same handle's
    product of another block on S2 -- both use the handle's M x k block and its slot table.  Both are the exact sums."""
    m, n = dm.MAIN
    rng = np.random.default_rng(seed_of("switch dnm"))
    pa = _ata_bits(m, n)
    Ka, X1, X2 = X.int_values(rng, (m, n), pa), X.int_values(rng, (n, 8), pa), X.int_values(rng, (n, 8), pa)
    X1s, X2d = dev(X1), dev(X2)
    X1d, Y1, Y2 = torch.empty_like(X1s), torch.empty_like(X1s), torch.empty_like(X1s)
    D = api.DenseMatrix.from_array(Ka)
    try:
        D.set_kernel(2)
        ref, _ = _switch(env, api, second, lambda: D.ata_multi(X1d, Y1), lambda: D.ata_multi(X2d, Y2), [Y1, Y2], (X1d, X1s),
                         ("the product enqueued before the switch", "the product after it"))
        assert D.multi_last_kernel == "k_dnm_ata_two_pass"
        X.assert_exact(ref[0], _exact(Ka.T, _exact(Ka, X1)), "before the switch")
        X.assert_exact(ref[1], _exact(Ka.T, _exact(Ka, X2)), "after the switch")
    finally:
        torch.cuda.synchronize()
        D.destroy()


def test_switch_between_two_complex_dense_products_of_one_handle(env, api, lib, second):
    """n = 200, the forced split, k = 8: clcg_hip_dense_matmat on S1 and, after the switch, on S2, over the handle's one slot table."""
    S = dz.system(200)
    K, n = S["K"], 200
    rng = np.random.default_rng(seed_of("switch zdnm"))
    X1, X2 = crand(rng, n, 8), crand(rng, n, 8)
    X1s, X2d = dev(X1), dev(X2)
    X1d, Y1, Y2 = torch.empty_like(X1s), torch.empty_like(X1s), torch.empty_like(X1s)
    D = api.DenseMatrix.from_array(K)
    try:
        D.set_kernel(2)
        ref, _ = _switch(env, api, second, lambda: D.cmatmat(X1d, Y1), lambda: D.cmatmat(X2d, Y2), [Y1, Y2], (X1d, X1s),
                         ("the product enqueued before the switch", "the product after it"))
        assert D.multi_last_kernel == "k_zdnm_row_split"
        csr = dc.dense_as_csr(K)
        for j in range(8):
            X.assert_rows(col(ref[0], j), *csr, col(X1, j), ("before the switch", j))
            X.assert_rows(col(ref[1], j), *csr, col(X2, j), ("after the switch", j))
    finally:
        torch.cuda.synchronize()
        D.destroy()


def test_switch_between_complex64_block_products(env, api, lib, second):
    """("helm", 182), k = 8: clcg_hip_spmm_c64 on S1 with X written late, the switch, clcg_hip_spmm_c64 on S2 -- and then, on S2,
    clcg_hip_spmm_dot_c64, which reads back (so it is called once the delay is known to be still running).  Outputs and sums are
    the own-stream bytes."""
    S = c6.system("helm", 182)
    n, rp, ci, v = S["n"], S["rp"], S["ci"], S["v"]
    lens = np.diff(rp)
    rng = np.random.default_rng(seed_of("switch c64"))
    X1, X2, U = (crand(rng, n, 8).astype(np.complex64) for _ in range(3))
    X1s, X2d, Ud = dev(X1), dev(X2), dev(U)
    X1d, Y1, Y2, Y3 = (torch.empty_like(X1s) for _ in range(4))
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    try:
        ref, sums = _switch(env, api, second, lambda: A.cspmm_c64(X1d, Y1), lambda: A.cspmm_c64(X2d, Y2), [Y1, Y2, Y3], (X1d, X1s),
                            ("the product enqueued before the switch", "the product after it", "the product with its sums"),
                            after=lambda: A.cspmm_dot_c64(X2d, Y3, Ud))
        for Yr, Xh in ((ref[0], X1), (ref[1], X2)):
            for j in range(8):
                hp = X.hp_product(rp, ci, v.astype(np.complex128), col(Xh, j).astype(np.complex128))
                assert np.all(X.row_errors(col(Yr, j).astype(np.complex128), hp) <= c6.row_bound(lens, 64, hp[2])), j
        same_bytes(ref[1], ref[2], "the product carrying the sums against the plain one")
        for j in range(8):
            assert_cdot(sums[j], col(ref[2], j), col(U, j), ("switch c64", j))
    finally:
        torch.cuda.synchronize()
        A.destroy()


# ================================================================================================ older entries no stream test ran
def test_complex_level_one(env, api, lib):
    """clcg_hip_axpy and clcg_hip_vecdiv (tests/test_gpu_streams.py::test_level_one runs the real ones and the complex dots): integer
    data, a multiplier and divisors that are powers of two -- exact under every order of operations."""
    n = 1001
    rng = np.random.default_rng(seed_of("complex level one"))
    a, b = X.int_values(rng, n, 20, cplx=True), X.int_values(rng, n, 20, cplx=True)
    div = rng.choice(np.array([2.0, -4.0, 2.0j, -0.5j]), n)
    As, Bs, Ds = dev(a), dev(b), dev(div)
    ad, dd, out = torch.empty_like(As), torch.empty_like(As), torch.empty_like(As)
    alpha = (C.c_double * 2)(0.5, -2.0)

    def exact_out(want, what):
        def anchor(r, o):
            assert r == 0, (what, r, lib.lcg_hip_last_error())
            X.assert_exact(o[0], want, what)
        return anchor
    env.pair([(ad, As), (out, Bs)], lambda: lib.clcg_hip_axpy(n, alpha, ad.data_ptr(), out.data_ptr()), [out], True, tag="clcg_hip_axpy",
             anchor=exact_out(b + (0.5 - 2.0j) * a, "y + alpha x"))
    env.pair([(ad, As), (dd, Ds)], lambda: lib.clcg_hip_vecdiv(n, ad.data_ptr(), dd.data_ptr(), out.data_ptr()), [out], True, tag="clcg_hip_vecdiv",
             anchor=exact_out(a / div, "a / b"))


def test_ready_made_callbacks_called_directly(env, api, lib):
    """The callbacks that no loop of tests/stop_cases.py passes, called as a caller's own Afp / Mfp would forward to them, with x
    written late: clcg_hip_ic0_mx, clcg_hip_ilu0_mx, clcg_hip_csr_ax_ilu0 (complex128), clcg_hip_ic0_mx_c64, lcg_hip_dense_ax,
    clcg_hip_dense_ax, clcg_hip_dense_jacobi_mx.  Run (a) has the bytes of the entry the callback stands for."""
    rp, ci, v = tm.system("ic0", "layered")
    n = len(rp) - 1
    vz = v + 0.25j * np.abs(v) * (ci == np.repeat(np.arange(n), np.diff(rp)))
    rng = np.random.default_rng(seed_of("callbacks"))
    for c64 in (False, True):
        x = crand(rng, n).astype(np.complex64 if c64 else np.complex128)
        xs = dev(x); xd, y, z = (torch.empty_like(xs) for _ in range(3))
        A = api.CsrMatrix.from_csr_c64(rp, ci, vz.astype(np.complex64)) if c64 else api.CsrMatrix.from_csr(rp, ci, vz)
        try:
            A.build_ic0()
            cases = [("ic0_mx", lib.clcg_hip_ic0_mx_c64 if c64 else lib.clcg_hip_ic0_mx, lambda: A.ic0_solve(xs, z, 2))]
            if not c64:
                A.build_ilu0()
                cases += [("ilu0_mx", lib.clcg_hip_ilu0_mx, lambda: A.ilu0_solve(xs, z, 2)),
                          ("csr_ax_ilu0", lib.clcg_hip_csr_ax_ilu0, lambda: A.ilu0_solve(xs, z, 2))]
            for name, cb, entry in cases:
                def anchor(r, o):
                    st.no_nan(o, name)
                    entry(); api.synchronize(); torch.cuda.synchronize()
                    if name == "csr_ax_ilu0":       # y = A.(U^-1 L^-1 x): the product of the solve's result, within the row bound
                        X.assert_rows(o[0], rp, ci, vz, z.cpu().numpy(), name)
                    else:
                        same_bytes(z.cpu().numpy(), o[0], (name, c64, "the callback against the entry it stands for"))
                env.pair([(xd, xs)], lambda: cb(A.h, xd.data_ptr(), y.data_ptr(), n, 0, 0), [y], True, tag=(name, c64), anchor=anchor)
        finally:
            A.destroy()
    # dense
    m = 257
    K = X.int_values(rng, (m, m), X.int_bits(m))
    x = X.int_values(rng, m, X.int_bits(m))
    xs = dev(x); xd, y = torch.empty_like(xs), torch.empty_like(xs)
    D = api.DenseMatrix.from_array(K)
    try:
        env.pair([(xd, xs)], lambda: lib.lcg_hip_dense_ax(D.h, xd.data_ptr(), y.data_ptr(), m), [y], True, tag="lcg_hip_dense_ax",
                 anchor=lambda r, o: X.assert_exact(o[0], _exact(K, x[:, None])[:, 0], "lcg_hip_dense_ax"))
    finally:
        D.destroy()
    S = dz.system(65)
    xh = crand(rng, 65)
    xs = dev(xh); xd, y = torch.empty_like(xs), torch.empty_like(xs)
    D = api.DenseMatrix.from_array(S["K"])
    try:
        D.build_jacobi(False)
        env.pair([(xd, xs)], lambda: lib.clcg_hip_dense_ax(D.h, xd.data_ptr(), y.data_ptr(), 65, 0, 0), [y], True, tag="clcg_hip_dense_ax",
                 anchor=lambda r, o: X.assert_rows(o[0], *dc.dense_as_csr(S["K"]), xh, "clcg_hip_dense_ax"))

        # (x times the stored reciprocal: held to its reference by tests/test_gpu_dense.py; here no NaN, and the identity)
        env.pair([(xd, xs)], lambda: lib.clcg_hip_dense_jacobi_mx(D.h, xd.data_ptr(), y.data_ptr(), 65, 0, 0), [y], True,
                 tag="clcg_hip_dense_jacobi_mx", anchor=lambda r, o: st.no_nan(o, "clcg_hip_dense_jacobi_mx"))
    finally:
        D.destroy()


def test_csr_handles_made_from_device_memory_written_late(env, api, lib):
    """lcg_hip_csr_create and lcg_hip_csr_create_c64 copying device arrays, and lcg_hip_csr_from_coo from device memory: the handle is
    made inside the pattern with its VALUES written late (row pointers, rows and columns are ready), and its first product is the
    exact sum."""
    S = sc.system("spd", 513)
    n, rp, ci = S["n"], S["rp"], S["ci"]
    rng = np.random.default_rng(seed_of("csr from device"))
    p = X.int_bits(int(np.diff(rp).max()), "c64")
    val, x = X.int_values(rng, len(ci), p), X.int_values(rng, n, p, zeros=0.02)
    exact = X.exact_int_product(rp, ci, val, x)
    rpd, cid, rowd = dev(rp), dev(ci), dev(np.repeat(np.arange(n, dtype=np.int32), np.diff(rp)))
    made = []

    def real():
        made.append(api.CsrMatrix.from_csr(rpd, cid, vd))
        made[-1].spmv(xd, y)

    def c64():
        made.append(api.CsrMatrix.from_csr_c64(rpd, cid, vd))
        made[-1].spmv_c64(xd, y)

    def coo():
        h = C.c_void_p()
        assert lib.lcg_hip_csr_from_coo(C.byref(h), n, len(ci), rowd.data_ptr(), cid.data_ptr(), vd.data_ptr(), 0, 1) == 0, lib.lcg_hip_last_error()
        made.append(api.CsrMatrix(h.value, n, False))
        made[-1].spmv(xd, y)
    try:
        for name, call, dtype in (("lcg_hip_csr_create", real, np.float64), ("lcg_hip_csr_create_c64", c64, np.complex64),
                                  ("lcg_hip_csr_from_coo", coo, np.float64)):
            vs, xs = dev(val.astype(dtype)), dev(x.astype(dtype))
            vd, xd, y = torch.empty_like(vs), torch.empty_like(xs), torch.empty_like(xs)
            env.pair([(vd, vs), (xd, xs)], call, [y], False, tag=name, anchor=lambda r, o: X.assert_exact(o[0], exact.astype(dtype), name))
    finally:
        torch.cuda.synchronize()
        for A in made:
            A.destroy()
