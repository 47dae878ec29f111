"""-m gpu: the library on a caller's stream (lcg_hip_set_stream, api.use_torch_stream / use_own_stream).

The pattern, its premise and the control that proves it can see a fault: tests/stream_cases.py.  Every case runs (a) on the
library's own stream with the inputs ready -- that run is held to tests/exact_ref.py (products) or to the properties the other
modules pin (factors, loops) -- and (b) on a non-blocking torch side stream S, entered while a >= 100 ms chain of filler kernels
is still running on S and the real inputs are written BEHIND it.  (b) must give (a)'s bits, in every output and every returned
scalar.  Entries that only enqueue must also return while the delay is still running.  Then: what the rest of the suite assumes of
torch's default stream, and switches between streams (lcg_hip_set_stream: the new stream waits for the previous one).
No tolerance anywhere: identities, and exact_ref's own bounds for run (a)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import exact_ref as X
import multi_bicg_cases as mb
import multi_cases as mc
import multi_cplx_cases as mz
import stop_cases as sc
import stream_cases as st
import tri_multi_cases as tm
from test_gpu_exact_products import _arrow, _family_matrices, _generated, data, dot_data, dot_u, max_line, op_csr
from test_gpu_kernels import _ragged
from test_gpu_ranges import mixed_system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def seed_of(*name):
    return zlib.crc32(repr(name).encode())


@pytest.fixture(scope="module")
def env(api, lib):
    """The calibrated delay and the side stream the controls accepted (stream_cases.make_env)."""
    e = st.make_env(torch, api, lib)
    yield e
    st.close_env(e)


# ================================================================================================ the control
@pytest.mark.parametrize("where", ["own", "null"])
def test_the_pattern_sees_work_on_another_stream(env, where):
    """A product deliberately left on the library's own stream, or a kernel put on the null stream (torch's default stream), while S
    runs the delay and writes x behind it: y comes out NaN.  Only then does an identity under the pattern say anything (two streams on one hardware queue
    would be serialised, and mis-streamed work there would see finished inputs).  Reads a buffer that is written later; nothing
    faults."""
    S = env.need_stream()
    A, xs, rp, col, val, x = env.control_system
    xd, y = torch.empty_like(xs), torch.empty_like(xs)
    assert env.control(S, where, A, xs, xd, y), f"work on the {where} stream saw finished inputs on the accepted stream"
    # and the same product ON S under the same pattern is the exact sum
    _, outs = env.late([(xd, xs)], lambda: A.spmv(xd, y), [y], enqueue_only=True)
    X.assert_exact(outs[0], X.exact_int_product(rp, col, val, x), ("control", where))


# ================================================================================================ products
def _extra_families(api, lib, rng):
    out = []
    L, nr = 5, 6400 + 13
    offs = np.sort(rng.choice(3000, L, replace=False))
    out.append(("run blocks + stretches", (np.arange(nr + 1) * L).astype(np.int32), (np.arange(nr)[:, None] + offs).ravel().astype(np.int32), nr + 3000,
                lambda A: (A.set_kernel(-64), lib.lcg_hip_csr_set_packed(A.h, 1), lib.lcg_hip_csr_set_run_stretches(A.h, 1)),
                "k_spmv_ldsp (LDS-staged, run blocks"))
    n, _, (rpm, cim, _) = mixed_system(rng, False, dims=(24, 26, 20))
    out.append(("mixed ranges", rpm, cim, n, lambda A: lib.lcg_hip_csr_set_ranges(A.h, 1), "rows [0, "))
    ra, ca = _arrow(rng)
    out.append(("arrow ranges", ra, ca, len(ra) - 1, lambda A: lib.lcg_hip_csr_set_ranges(A.h, -1), "rows [0, "))
    return out


FAMILIES = ["wave", "ldsw", "lds1", "ldsp", "templates", "run1", "tiled", "binned", "run blocks", "long rows", "ranges",
            "run blocks + stretches", "mixed ranges", "arrow ranges"]


@pytest.fixture(scope="module")
def families(api, lib):
    rng = np.random.default_rng(909)
    fam = {f[0]: f for f in _family_matrices(api, lib, rng) + _extra_families(api, lib, rng)}
    assert sorted(fam) == sorted(FAMILIES)
    return fam


@pytest.mark.parametrize("name", FAMILIES)
def test_real_product_families(env, api, lib, families, name):
    """lcg_hip_spmv of one matrix per kernel family lcg_hip_csr_last_kernel can name, on integer data (run (a) is the exact sum bit for
    bit); a warmed handle only enqueues; a FRESH handle whose first product -- and with it its plan build -- happens on S gives the
    same bits."""
    _, rp, col, ncols, setup, want = families[name]
    n = len(rp) - 1
    rng = np.random.default_rng(seed_of(name))
    val, x = data(rng, rp, ncols, False, True)
    exact = X.exact_int_product(rp, col, val, x)
    xs = dev(x); xd = torch.empty_like(xs)
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    handles = []

    def make():
        A = api.CsrMatrix.from_csr(rp, col, val, n_cols=ncols)
        setup(A)
        handles.append(A)
        return A

    def reached(A):
        kern = lib.lcg_hip_csr_last_kernel(A.h).decode()
        assert kern.startswith(want), (name, kern)
        if name == "templates":
            assert lib.lcg_hip_csr_packed_templates(A.h) > 0
        if name.startswith("run blocks"):
            assert lib.lcg_hip_csr_packed_runs(A.h, None) > 0
            assert (lib.lcg_hip_csr_run_stretches(A.h, None) > 0) == name.endswith("stretches"), name
        if name == "arrow ranges":
            assert "k_lr_" in kern, kern
        if "ranges" in name:
            assert lib.lcg_hip_csr_ranges(A.h, 0, None) >= 2
    try:
        A = make()

        def anchor(r, outs):
            reached(A)
            X.assert_exact(outs[0], exact, (name, "own stream"))
        _, oa = env.pair([(xd, xs)], lambda: A.spmv(xd, y), [y], enqueue_only=True, tag=(name,), anchor=anchor)
        reached(A)
        F = make()
        _, ob = env.late([(xd, xs)], lambda: F.spmv(xd, y), [y], enqueue_only=False)
        reached(F)
        assert ob[0].tobytes() == oa[0].tobytes(), (name, "a fresh handle whose plan was built on the side stream")
    finally:
        for H in handles:
            H.destroy()


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_spmv_op_all_forms(env, api, lib, cplx):
    """A, A^T, conj(A), A^H (the op(A) copies are built at the first use of a form: the fresh handle builds them on S)."""
    rng = np.random.default_rng(505 + cplx)
    n = 2500
    rp, col = _ragged(rng, n, n, 30, long_rows=[(7, 2400)])
    col[rp[100]:rp[100] + 10] = 3
    val, x = data(rng, rp, n, cplx, True, max_len=max_line(rp, col, n))
    xs = dev(x); xd = torch.empty_like(xs); y = torch.empty_like(xs)
    A, F = api.CsrMatrix.from_csr(rp, col, val), api.CsrMatrix.from_csr(rp, col, val)
    try:
        for form, (layout, conj) in (("A", (0, 0)), ("AT", (1, 0)), ("conj", (0, 1)), ("AH", (1, 1))):
            exact = X.exact_int_product(*op_csr(rp, col, val, n, form), x)

            def call(H=A):
                assert lib.lcg_hip_spmv_op(H.h, xd.data_ptr(), y.data_ptr(), layout, conj) == 0

            def anchor(r, outs):
                kern = lib.lcg_hip_csr_last_kernel(A.h).decode()
                assert kern.startswith(("k_spmv_lds1 ", "k_spmv_ldsw ", "k_spmv_run1 ", "k_spmv_wave")), (form, kern)
                X.assert_exact(outs[0], exact, (cplx, form))
            _, oa = env.pair([(xd, xs)], call, [y], enqueue_only=True, tag=(cplx, form), anchor=anchor)
            _, ob = env.late([(xd, xs)], lambda: call(F), [y], enqueue_only=False)
            assert ob[0].tobytes() == oa[0].tobytes(), (cplx, form, "fresh handle")
    finally:
        A.destroy(); F.destroy()


def test_c128_and_c64_products(env, api, lib):
    """lcg_hip_spmv on a complex128 matrix, lcg_hip_spmv_c64 (A and A^H) on a complex64 one."""
    rng = np.random.default_rng(606)
    n = 3001
    rp, col = _ragged(rng, n, n, 40, long_rows=[(5, 5000), (2999, 2500)])
    val, x = data(rng, rp, n, True, True)
    xs = dev(x); xd = torch.empty_like(xs); y = torch.empty_like(xs)
    A, F = api.CsrMatrix.from_csr(rp, col, val), api.CsrMatrix.from_csr(rp, col, val)
    try:
        def anchor(r, outs):
            assert lib.lcg_hip_csr_last_kernel(A.h).decode().startswith("k_spmv"), lib.lcg_hip_csr_last_kernel(A.h)
            X.assert_exact(outs[0], X.exact_int_product(rp, col, val, x), "c128")
        _, oa = env.pair([(xd, xs)], lambda: A.spmv(xd, y), [y], enqueue_only=True, tag="c128", anchor=anchor)
        _, ob = env.late([(xd, xs)], lambda: F.spmv(xd, y), [y], enqueue_only=False)
        assert ob[0].tobytes() == oa[0].tobytes(), "c128, fresh handle"
    finally:
        A.destroy(); F.destroy()
    n = 4001
    lens = rng.poisson(12.0, n).astype(np.int64); lens[0] = lens[-1] = 0; lens[n // 3] = 512; lens[n // 2] = 513
    rp = np.zeros(n + 1, np.int32); rp[1:] = np.cumsum(lens)
    col = rng.integers(0, n, rp[-1]).astype(np.int32)
    p = X.int_bits(max_line(rp, col, n), "c64")
    val = X.int_values(rng, int(rp[-1]), p, True).astype(np.complex64)
    x = X.int_values(rng, n, p, True, zeros=0).astype(np.complex64)
    xs = dev(x); xd = torch.empty_like(xs); y = torch.empty_like(xs)
    A, F = api.CsrMatrix.from_csr_c64(rp, col, val), api.CsrMatrix.from_csr_c64(rp, col, val)
    try:
        for form, (layout, conj) in (("A", (0, 0)), ("AH", (1, 1))):
            exact = X.exact_int_product(*op_csr(rp, col, val.astype(np.complex128), n, form), x.astype(np.complex128))

            def anchor(r, outs):
                kern = lib.lcg_hip_csr_last_kernel(A.h).decode()
                assert kern.startswith("k_c64_rows<"), kern
                X.assert_exact(outs[0].astype(np.complex128), exact, ("c64", form))
            _, oa = env.pair([(xd, xs)], lambda: A.spmv_c64(xd, y, layout, conj), [y], enqueue_only=True, tag=("c64", form), anchor=anchor)
            _, ob = env.late([(xd, xs)], lambda: F.spmv_c64(xd, y, layout, conj), [y], enqueue_only=False)
            assert ob[0].tobytes() == oa[0].tobytes(), ("c64", form, "fresh handle")
    finally:
        A.destroy(); F.destroy()


def test_spmv_dot(env, api, lib):
    """lcg_hip_spmv_dot where the sums ride in the product (k_spmv_lds1d, k_tile_spmv) -- with its two sums read back, and with
    result2 = NULL, which only enqueues."""
    for name, n, maker in (("lds1d", 5000, None), ("tiled", 8 * 1024 + 1, api.GEN_ROW_RANDOM_BAND)):
        rng = np.random.default_rng(seed_of("dot", name))
        rp, col = _ragged(rng, n, n, 30) if maker is None else _generated(api, n, maker, 3000, 2)
        val, x = dot_data(rng, rp, n, True)
        u = dot_u(rng, n, True, rp)
        exact = X.exact_int_product(rp, col, val, x)
        xs, us = dev(x), dev(u)
        xd, ud, y = torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs)
        A = api.CsrMatrix.from_csr(rp, col, val)
        if maker is not None:
            assert lib.lcg_hip_csr_set_tiled(A.h, 1) == 0
        try:
            def with_sums():
                sums = (C.c_double * 2)()
                assert lib.lcg_hip_spmv_dot(A.h, xd.data_ptr(), y.data_ptr(), ud.data_ptr(), sums) == 0
                return sums[0], sums[1]

            def anchor(r, outs):
                kern = lib.lcg_hip_csr_last_kernel(A.h).decode()
                assert ("k_spmv_lds1d" if maker is None else "k_tile_spmv") in kern, kern
                X.assert_exact(outs[0], exact, ("dot", name))
                assert r == (float(np.dot(exact, u)), float(np.dot(exact, exact))), (name, r)       # integer data: exact sums
            _, oa = env.pair([(xd, xs), (ud, us)], with_sums, [y], enqueue_only=False, tag=("dot", name), anchor=anchor)

            def sums_left_on_the_device():
                assert lib.lcg_hip_spmv_dot(A.h, xd.data_ptr(), y.data_ptr(), ud.data_ptr(), None) == 0
            _, ob = env.late([(xd, xs), (ud, us)], sums_left_on_the_device, [y], enqueue_only=True)
            assert ob[0].tobytes() == oa[0].tobytes(), (name, "result2 = NULL")
        finally:
            A.destroy()


@pytest.mark.parametrize("k", [2, 8])
def test_real_block_products(env, api, lib, k):
    """lcg_hip_spmm, lcg_hip_spmm_dot and lcg_hip_spmm_dot2 on the first system beyond MM_MG row blocks (the folded dot)."""
    S = mc.system("spd", 32771)
    assert S["blocks"] > mc.MM_MG
    rng = np.random.default_rng(seed_of("spmm", k))
    Xh = rng.standard_normal((S["n"], k)); Uh = rng.standard_normal((S["n"], k))
    Xs, Us = dev(Xh), dev(Uh)
    Xd, Ud, Y = torch.empty_like(Xs), torch.empty_like(Xs), torch.empty_like(Xs)
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    try:
        def rows(outs):
            for j in range(k):
                X.assert_rows(np.ascontiguousarray(outs[0][:, j]), S["rp"], S["ci"], S["v"], Xh[:, j], ("spmm", k, j))
        env.pair([(Xd, Xs)], lambda: A.spmm(Xd, Y), [Y], enqueue_only=True, tag=("spmm", k), anchor=lambda r, o: rows(o))

        def dot():
            out = (C.c_double * k)()
            assert lib.lcg_hip_spmm_dot(A.h, k, Xd.data_ptr(), Y.data_ptr(), Ud.data_ptr(), out) == 0
            return list(out)

        def anchor_dot(r, outs):
            rows(outs)
            for j in range(k):
                X.assert_dot(r[j], np.ascontiguousarray(outs[0][:, j]), np.ascontiguousarray(Uh[:, j]), ("spmm_dot", k, j))
        env.pair([(Xd, Xs), (Ud, Us)], dot, [Y], enqueue_only=False, tag=("spmm_dot", k), anchor=anchor_dot)

        def anchor_dot2(r, outs):
            rows(outs)
            for j in range(k):
                X.assert_dot(r[j], np.ascontiguousarray(outs[0][:, j]), np.ascontiguousarray(Uh[:, j]), ("spmm_dot2 y.u", k, j))
                X.assert_dot(r[k + j], np.ascontiguousarray(outs[0][:, j]), np.ascontiguousarray(outs[0][:, j]), ("spmm_dot2 y.y", k, j))
        env.pair([(Xd, Xs), (Ud, Us)], lambda: A.spmm_dot2(Xd, Y, Ud), [Y], enqueue_only=False, tag=("spmm_dot2", k), anchor=anchor_dot2)
    finally:
        A.destroy()


@pytest.mark.parametrize("key", [("helm", 182), ("band140", 2051)], ids=["R64", "R4"])
def test_complex_block_products(env, api, lib, key):
    """clcg_hip_spmm and clcg_hip_spmm_dot at 64 and 4 rows per block, k = 2 and 8."""
    S = mz.system(*key)
    assert S["R"] == (64 if key[0] == "helm" else 4)
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    try:
        for k in (2, 8):
            rng = np.random.default_rng(seed_of("cspmm", key, k))
            Xh = rng.standard_normal((S["n"], k)) + 1j * rng.standard_normal((S["n"], k))
            Uh = rng.standard_normal((S["n"], k)) + 1j * rng.standard_normal((S["n"], k))
            Xs, Us = dev(Xh), dev(Uh)
            Xd, Ud, Y = torch.empty_like(Xs), torch.empty_like(Xs), torch.empty_like(Xs)

            def rows(r, outs):
                for j in range(k):
                    X.assert_rows(np.ascontiguousarray(outs[0][:, j]), S["rp"], S["ci"], S["v"], Xh[:, j], ("cspmm", key, k, j))
            _, oa = env.pair([(Xd, Xs)], lambda: A.cspmm(Xd, Y), [Y], enqueue_only=True, tag=("cspmm", key, k), anchor=rows)
            _, ob = env.pair([(Xd, Xs), (Ud, Us)], lambda: A.cspmm_dot(Xd, Y, Ud), [Y], enqueue_only=False, tag=("cspmm_dot", key, k), anchor=rows)
            assert ob[0].tobytes() == oa[0].tobytes(), (key, k, "the product carrying the sums against the plain one")
    finally:
        A.destroy()


def test_dense_products(env, api, lib):
    """lcg_hip_dense_matvec in both layouts and lcg_hip_dense_ata, on integer data (exact)."""
    rng = np.random.default_rng(808)
    m, n = 1000, 800
    K = rng.integers(-16, 17, (m, n)).astype(np.float64)
    Dm = api.DenseMatrix.from_array(K)
    try:
        for what, xin, nout, call_of, exact_of in (
                ("K.x", n, m, lambda x, y: Dm.matvec(x, y, 0), lambda x: K.astype(np.int64) @ x.astype(np.int64)),
                ("K^T.x", m, n, lambda x, y: Dm.matvec(x, y, 1), lambda x: K.T.astype(np.int64) @ x.astype(np.int64)),
                ("K^T.K.x", n, n, lambda x, y: Dm.ata(x, y), lambda x: K.T.astype(np.int64) @ (K.astype(np.int64) @ x.astype(np.int64)))):
            x = rng.integers(-16, 17, xin).astype(np.float64)
            xs = dev(x); xd = torch.empty_like(xs); y = torch.empty(nout, dtype=torch.float64, device="cuda")
            exact = exact_of(x).astype(np.float64)
            assert np.abs(exact).max() < 2.0 ** 52

            def anchor(r, outs):
                assert Dm.last_kernel, what
                X.assert_exact(outs[0], exact, ("dense", what))
            env.pair([(xd, xs)], lambda: call_of(xd, y), [y], enqueue_only=True, tag=("dense", what), anchor=anchor)
    finally:
        Dm.destroy()


def test_sharded_product_on_one_gpu(env, api, lib, port):
    """lcg_hip_csr_split_for_test: the only single-GPU path through the fork and join with the second stream (comm.hip).  The gather
    buffer and the local slice are both written late."""
    from liblcg_amd import partition
    n, nranks, r = 10007, 4, 1
    g = port.gen_init(n, 16, 50, True, 9, 0.01)
    rp, ci, v = port.gen_rows(g)
    x = np.random.default_rng(4).standard_normal(n)
    glen = partition.gathered_length(n, nranks)
    xpad = np.zeros(glen); xpad[:n] = x
    r0, r1 = partition.shard_range(n, nranks, r)
    A = api.CsrMatrix.generate(n, 16, 50, True, 9, 0.01, r0, r1)
    try:
        assert lib.lcg_hip_csr_split_for_test(A.h, n, nranks, r) == 0
        xfull = torch.as_tensor(st.DevPtr(lib.lcg_hip_csr_xfull(A.h), glen), device="cuda")
        assert xfull.data_ptr() == lib.lcg_hip_csr_xfull(A.h)
        xfs, xls = dev(xpad), dev(x[r0:r1].copy())
        xl, yl = torch.empty_like(xls), torch.empty_like(xls)

        def anchor(res, outs):
            X.assert_rows(outs[0], rp[r0:r1 + 1] - rp[r0], ci[rp[r0]:rp[r1]], v[rp[r0]:rp[r1]], x, ("shard", nranks, r))
            assert lib.lcg_hip_csr_local_nnz(A.h) > 0.9 * A.nnz
        env.pair([(xfull, xfs), (xl, xls)], lambda: A.spmv(xl, yl), [yl], enqueue_only=True, tag="sharded", anchor=anchor)
    finally:
        A.destroy()


# ================================================================================================ level 1, Jacobi
@pytest.mark.parametrize("n", [1001, 524289])
def test_level_one(env, api, lib, n):
    """dot, nrm2, cdot (both forms), axpy, scal, vecmul, vecdiv, set2box -- one workgroup's worth and more than one stride, odd."""
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n), rng.standard_normal(n) + 3.0
    ca, cb = rng.standard_normal(n) + 1j * rng.standard_normal(n), rng.standard_normal(n) + 1j * rng.standard_normal(n)
    As, Bs, CAs, CBs = dev(a), dev(b), dev(ca), dev(cb)
    ad, bd, out = torch.empty_like(As), torch.empty_like(As), torch.empty_like(As)
    cad, cbd = torch.empty_like(CAs), torch.empty_like(CAs)

    def within(r, parts, terms, what):
        """r against sum(sign * p . q) over parts, each in extended precision: exact_ref's dot bound for `terms` products."""
        exact = sum(s * X.hp_dot(p, q)[0] for s, p, q in parts)
        absum = sum(X.hp_dot(p, q)[1] for _, p, q in parts)
        assert abs(r - exact) <= X.dot_bound(absum, terms), (what, r, exact, absum)
    ra, _ = env.pair([(ad, As), (bd, Bs)], lambda: api.dot(ad, bd), [], False, tag="dot", anchor=lambda r, o: within(r, [(1, a, b)], n, "dot"))
    aa = []
    env.pair([(ad, As)], lambda: api.nrm2(ad), [], False, tag="nrm2", anchor=lambda r, o: aa.append((r, api.dot(ad, ad))))
    assert aa[0][0] == float(np.sqrt(aa[0][1])), ("nrm2 is the square root of dot(a, a)", aa)
    within(aa[0][1], [(1, a, a)], n, "dot(a, a)")
    for conj, tag in ((False, "cdot"), (True, "cinner")):
        s = 1.0 if conj else -1.0       # sum a b: (ar br - ai bi) + i (ar bi + ai br); sum conj(a) b: (ar br + ai bi) + i (ar bi - ai br)

        def anchor(r, o):
            within(r.real, [(1, ca.real, cb.real), (s, ca.imag, cb.imag)], 2 * n, tag)
            within(r.imag, [(1, ca.real, cb.imag), (-s, ca.imag, cb.real)], 2 * n, tag)
        env.pair([(cad, CAs), (cbd, CBs)], lambda: api.cdot(cad, cbd, conj=conj), [], False, tag=tag, anchor=anchor)

    def exact_out(f):
        return lambda r, outs: X.assert_exact(outs[0], f(), "level 1")
    P = lib
    env.pair([(ad, As), (out, Bs)], lambda: P.lcg_hip_axpy(n, 0.5, ad.data_ptr(), out.data_ptr()), [out], True, tag="axpy",
             anchor=exact_out(lambda: b + 0.5 * a))     # (0.5 a is exact: one rounding with or without a fused multiply-add)
    env.pair([(out, As)], lambda: P.lcg_hip_scal(n, 0.5, out.data_ptr()), [out], True, tag="scal", anchor=exact_out(lambda: 0.5 * a))
    env.pair([(ad, As), (bd, Bs)], lambda: P.lcg_hip_vecmul(n, ad.data_ptr(), bd.data_ptr(), out.data_ptr()), [out], True, tag="vecmul",
             anchor=exact_out(lambda: a * b))
    env.pair([(ad, As), (bd, Bs)], lambda: P.lcg_hip_vecdiv(n, ad.data_ptr(), bd.data_ptr(), out.data_ptr()), [out], True, tag="vecdiv",
             anchor=exact_out(lambda: a / b))
    low, hig = dev(np.full(n, -0.5)), dev(np.full(n, 0.25))
    lo_d, hi_d = torch.empty_like(low), torch.empty_like(low)
    env.pair([(lo_d, low), (hi_d, hig), (out, As)], lambda: P.lcg_hip_set2box(n, lo_d.data_ptr(), hi_d.data_ptr(), out.data_ptr()), [out], True,
             tag="set2box", anchor=exact_out(lambda: np.clip(a, -0.5, 0.25)))


def test_jacobi(env, api, lib):
    """lcg_hip_csr_build_jacobi on S from adopted arrays written late, then lcg_hip_jacobi_mx."""
    S = sc.system("spd", 513)
    n = S["n"]
    rps, cis, vs = dev(S["rp"]), dev(S["ci"]), dev(S["v"])
    rpd, cid, vd = torch.empty_like(rps), torch.empty_like(cis), torch.empty_like(vs)
    x = np.random.default_rng(5).standard_normal(n)
    xs = dev(x); xd, y, diag = torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs)
    A = api.CsrMatrix.from_csr(rpd, cid, vd, adopt=True)
    try:
        def call():
            A.build_jacobi(diag)
            lib.lcg_hip_jacobi_mx(A.h, xd.data_ptr(), y.data_ptr(), n)
        rows = np.repeat(np.arange(n), np.diff(S["rp"]))
        d = S["v"][S["ci"] == rows]

        def anchor(r, o):
            X.assert_exact(o[1], d, "the diagonal")
            X.assert_exact(o[0], (1.0 / d) * x, "x over the diagonal, as the stored reciprocal times x")
        env.pair([(rpd, rps), (cid, cis), (vd, vs), (xd, xs)], call, [y, diag], True, tag="jacobi", anchor=anchor)
    finally:
        A.destroy()


# ================================================================================================ IC(0) / ILU(0)
@pytest.mark.parametrize("factor", ["ic0", "ilu0", "ic0_c64"])
def test_factor_built_and_applied_on_a_side_stream(env, api, lib, factor):
    """build_ic0 / build_ilu0 / build_ic0_c64 on S from adopted arrays written late (the builds mix stream work with synchronous
    copies), then every `which` of the solve with level schedules and with 3 sweeps.  The factor built on S has the bits of the one
    built on the own stream."""
    base = "ic0" if factor.startswith("ic0") else "ilu0"
    rp, ci, v = tm.system(base, "layered")
    n = len(rp) - 1
    c64 = factor == "ic0_c64"
    if c64:
        v = (v + 0.25j * np.abs(v) * (ci == np.repeat(np.arange(n), np.diff(rp)))).astype(np.complex64)
    rng = np.random.default_rng(seed_of(factor))
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) if c64 else rng.standard_normal(n)
    rps, cis, vs, xs = dev(rp), dev(ci), dev(v), dev(x)
    rpd, cid, vd, xd, y = torch.empty_like(rps), torch.empty_like(cis), torch.empty_like(vs), torch.empty_like(xs), torch.empty_like(xs)
    A = (api.CsrMatrix.from_csr_c64 if c64 else api.CsrMatrix.from_csr)(rpd, cid, vd, adopt=True)
    build = A.build_ic0 if base == "ic0" else A.build_ilu0
    solve = A.ic0_solve if base == "ic0" else A.ilu0_solve
    to_host = A.ic0_factor_to_host if base == "ic0" else (lambda: A.ilu0_factor_to_host(0) + A.ilu0_factor_to_host(1))
    arrays = [(rpd, rps), (cid, cis), (vd, vs)]
    try:
        def built():
            build()
            return tuple(f.tobytes() for f in to_host())

        def anchor(r, o):       # (the factor itself is held to the checkers by tests/test_gpu_ic0*.py and test_gpu_ilu0*.py)
            for f in to_host():
                assert f.size and not np.isnan(f.view(np.float32 if f.dtype == np.complex64 else f.dtype)).any(), factor
        env.pair(arrays, built, [], False, tag=(factor, "build"), anchor=anchor)
        info = A.ic0_info() if base == "ic0" else A.ilu0_info()
        assert info["zero_pivot"] == -1 and info["launches_per_apply"] > 2, info
        for sweeps in (0, 3):
            tm.set_sweeps(A, base, sweeps)
            for which in (0, 1, 2):
                env.pair([(xd, xs)], lambda: solve(xd, y, which), [y], True, tag=(factor, sweeps, which),
                         anchor=lambda r, o: st.no_nan(o, (factor, sweeps, which)))
    finally:
        A.destroy()


@pytest.mark.parametrize("factor", ["ic0", "ilu0"])
def test_batched_triangular_solves(env, api, lib, factor):
    """lcg_hip_ic0_solve_multi / lcg_hip_ilu0_solve_multi at k = 4, level schedules and 3 sweeps: run (a) is the single-vector solve
    of every column bit for bit."""
    arrays = tm.system(factor, "layered")
    n = len(arrays[0]) - 1
    A = tm.build(api, factor, arrays)
    Xh = np.random.default_rng(seed_of("trim", factor)).standard_normal((n, 4))
    Xs = dev(Xh); Xd, Y = torch.empty_like(Xs), torch.empty_like(Xs)
    multi = A.ic0_solve_multi if factor == "ic0" else A.ilu0_solve_multi
    try:
        for sweeps in (0, 3):
            tm.set_sweeps(A, factor, sweeps)
            for which in (0, 1, 2):
                want = tm.single(torch, A, factor, which, Xh)
                env.pair([(Xd, Xs)], lambda: multi(Xd, Y, which), [Y], True, tag=(factor, sweeps, which),
                         anchor=lambda r, o: X.assert_exact(o[0], want, (factor, sweeps, which, "against the single-vector solves")))
    finally:
        A.destroy()


# ================================================================================================ solver loops
import test_gpu_stop_contract as T      # noqa: E402  (Bench, guarded, guards_intact -- unchanged)

SMALL_CASES = [(L, n) for L, n in sc.CASES if n in (65, 513)]
LARGE_CASES = [(sc.BY_NAME[name], sc.SIZES[sc.BY_NAME[name].family][2]) for name in ("cg_auto", "c_bicg_sym", "c64_bicg")]
LOOP_CASES = SMALL_CASES + LARGE_CASES
_systems = {}


@pytest.fixture(scope="module")
def benches(api, lib, port):
    made = {}

    def get(L, n):
        if (L.name, n) not in made:
            if (L.kind, n) not in _systems:
                _systems[(L.kind, n)] = sc.system(L.kind, n)
            made[(L.name, n)] = T.Bench(api, lib, port, L, n, _systems[(L.kind, n)])
        return made[(L.name, n)]
    yield get
    for B in made.values():
        B.A.destroy()
    made.clear(); _systems.clear()


@pytest.mark.parametrize("case", LOOP_CASES, ids=[f"{L.name}-{n}" for L, n in LOOP_CASES])
def test_solver_loops(env, benches, case):
    """Every loop of stop_cases.LOOPS through Bench.solve: free-running, with a progress callback (one synchronisation per
    iteration) and capped at 3, with m, b and a box loop's bounds written late.  Code, count, residual, iterate, the callback's ks
    and caller-owned workspaces: the bits of the run on the own stream.  The large sizes reach the paced enqueue (work >= 2^20)."""
    L, n = case
    B = benches(L, n)
    for variant, kw in (("free", {}), ("callback", {"on_progress": lambda k, mp, res: 0}), ("capped", {"cap": 3})):
        a = st.bench_solve(env, T, B, late=False, **kw)
        if variant == "capped":
            assert (a["ret"], a["iters"]) == (T.CAP, 3), (L.name, n, a["ret"], a["iters"])
        else:
            assert a["ret"] == 0 and sc.ITER_WINDOW[0] <= a["iters"] <= sc.ITER_WINDOW[1], (L.name, n, variant, a["ret"], a["iters"])
            if variant == "callback":
                assert a["ks"] == list(range(a["iters"] + 1))
        b = st.bench_solve(env, T, B, late=True, **kw)
        st.same_solve(a, b, (L.name, n, variant))
        for r in (a, b):
            assert T.guards_intact(r["mbuf"]) and T.guards_intact(r["bbuf"]), (L.name, n, variant)
            assert T.same(r["bbuf"].cpu().numpy()[T.GUARD:-T.GUARD], r["b_in"])


@pytest.mark.parametrize("name", ["cg_auto", "c_bicg_sym", "c64_bicg"])
def test_host_vectors(env, api, lib, benches, name):
    """m and B in host memory (mem = HOST): copied in and out by the library on its stream, entered while the delay runs on S."""
    L = sc.BY_NAME[name]
    B = benches(L, 513)
    cplx = L.family != "real"

    def run():
        m = np.zeros(513, B.dtype); b = np.ascontiguousarray(B.rhs)
        para = (api.clcg_default_parameters if cplx else api.lcg_default_parameters)(epsilon=L.eps, abs_diff=L.abs_diff)
        if L.family == "real":
            info = api.lcg_solver("lcg_hip_csr_ax", None, m, b, 513, para, B.A, L.sid)
        elif L.family == "c128":
            info = api.clcg_solver("clcg_hip_csr_ax", None, m, b, 513, para, B.A, L.sid)
        else:
            info = api.clcg_solver_c64("clcg_hip_csr_ax_c64", None, m, b, 513, para, B.A, L.sid)
        return info.ret, info.iterations, info.residual, m
    ra, _ = env.reference([], run, [])
    assert ra[0] == 0 and sc.ITER_WINDOW[0] <= ra[1] <= sc.ITER_WINDOW[1] and ra[2] <= L.eps, (name, ra[:3])
    rb, _ = env.late([], run, [], enqueue_only=False)
    assert st.same_scalars(ra, rb), (name, ra[:3], rb[:3])


def test_a_callers_own_product(env, api, lib, benches):
    """A Python Afp that forwards to lcg_hip_spmv, and one whose product is a torch op on torch's CURRENT stream -- what an embedding
    application writes after api.use_torch_stream(): classic CG at n = 65."""
    L = sc.BY_NAME["cg_classic"]
    B = benches(L, 65)

    def forward(inst, xp, yp, nn):
        assert lib.lcg_hip_spmv(B.A.h, xp, yp) == 0
    a = st.bench_solve(env, T, B, late=False, afp=forward)
    assert a["ret"] == 0
    st.same_solve(a, st.bench_solve(env, T, B, late=True, afp=forward), "forwarding Afp")
    Kd = dev(sc.dense_of(B.S))

    def torch_product(inst, xp, yp, nn):
        x = torch.as_tensor(st.DevPtr(xp, nn), device="cuda")
        y = torch.as_tensor(st.DevPtr(yp, nn), device="cuda")
        torch.sum(Kd * x, dim=1, out=y)
    a = st.bench_solve(env, T, B, late=False, afp=torch_product)
    assert a["ret"] == 0 and sc.ITER_WINDOW[0] <= a["iters"] <= sc.ITER_WINDOW[1], (a["ret"], a["iters"])
    st.same_solve(a, st.bench_solve(env, T, B, late=True, afp=torch_product), "torch Afp on the current stream")


# ---------------------------------------------------------------------------------------------------------- batched loops
def _batched_cases():
    real = [("spd", 65), ("spd", 32771)]
    nonsym = [("nonsym", 65), ("nonsym", 32771)]
    helm = [("helm", 40), ("helm", 182)]
    out = []
    for key in real:
        out += [("lcg_multi", key, None), ("lpcg_multi", key, None), ("lpcg_multi_m", key, "ic0"), ("lpcg_multi_m", key, "ilu0")]
    for key in nonsym:
        out += [("lbicgstab_multi", key, None), ("lbicgstab_multi", key, "ilu0")]
    for key in helm:
        out += [("clbicg_sym_multi", key, None), ("clpcg_multi", key, None)]
    return out


BATCHED = _batched_cases()


@pytest.mark.parametrize("loop,key,pre", BATCHED, ids=[f"{l}-{k[0]}{k[1]}-{p or 'plain'}" for l, k, p in BATCHED])
def test_batched_loops(env, api, lib, loop, key, pre):
    """Every batched loop at k = 2 and 8, on the smallest system of its case module and the first beyond MM_MG row blocks, capped at 6
    and converged: per column code, count, residual and iterate."""
    cplx = loop.startswith("cl")
    mod = mz if cplx else (mb if loop == "lbicgstab_multi" else mc)
    S = mod.system(*key)
    assert (S["blocks"] > mc.MM_MG) == (key[1] not in (65, 40)), (key, S["blocks"])
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    try:
        if pre == "ic0":
            A.build_ic0()
        elif pre == "ilu0":
            A.build_ilu0()
        else:
            A.build_jacobi()
        fn = {"lcg_multi": lib.lcg_hip_lcg_multi, "lpcg_multi": lib.lcg_hip_lpcg_multi, "lpcg_multi_m": lib.lcg_hip_lpcg_multi_m,
              "lbicgstab_multi": lib.lcg_hip_lbicgstab_multi, "clbicg_sym_multi": lib.clcg_hip_lbicg_sym_multi,
              "clpcg_multi": lib.clcg_hip_lpcg_multi}[loop]
        lead_of = {"lpcg_multi_m": lambda k: (A.h, k, api.PRECONDS[pre]),
                   "lbicgstab_multi": lambda k: (A.h, k, api.M_NONE if pre is None else api.PRECONDS[pre])}.get(loop, lambda k: (A.h, k))
        for k in (2, 8):
            Bh = (mz if cplx else mc).columns(S["n"], S["b"], k)
            M0 = (mz if cplx else mc).guesses(S, k)
            Bs, M0s = dev(Bh), dev(M0)
            Bd, Md = torch.empty_like(Bs), torch.empty_like(M0s)
            for cap in (6, 0):
                para = (api.clcg_default_parameters if cplx else api.lcg_default_parameters)(max_iterations=cap, epsilon=1e-10, abs_diff=int(not cplx))

                def call():
                    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
                    rc = fn(*lead_of(k), Md.data_ptr(), Bd.data_ptr(), C.byref(para), ret, its, res, 1)
                    return rc, list(ret), list(its), list(res)

                def anchor(r, outs):
                    rc, ret, its, res = r
                    assert rc == 0 and 99 not in ret and -1 not in its, (loop, key, k, cap, r)
                    st.no_nan(outs, (loop, key, k, cap))
                    if cap == 0:        # column 0 (b itself from a zero guess) converges
                        assert ret[0] == 0 and its[0] > 0, (loop, key, k, r)
                    elif loop == "lbicgstab_multi" and pre == "ilu0":       # (ILU(0) applied exactly is nearly A^-1 on these bands: 4 iterations)
                        assert 0 < max(its) <= cap, (loop, key, k, r)
                    else:
                        assert max(its) == cap, (loop, key, k, r)
                env.pair([(Md, M0s), (Bd, Bs)], call, [Md], False, tag=(loop, key, pre, k, cap), anchor=anchor)
    finally:
        A.destroy()


# ================================================================================================ the default stream
def test_default_stream_needs_no_synchronisation(env, api, lib):
    """What the rest of the suite assumes without saying so: with the library on its OWN stream (a blocking one), work that torch
    puts on its default stream -- the delay, the late writes, the clones -- is ordered against the library's by the runtime, with no
    synchronisation in between: spmv, a CG solve and a two-sided ic0_solve."""
    A, xs, rp, col, val, x = env.control_system
    xd, y = torch.empty_like(xs), torch.empty_like(xs)
    env.pair([(xd, xs)], lambda: A.spmv(xd, y), [y], True, tag="spmv", on_default=True,
             anchor=lambda r, o: X.assert_exact(o[0], X.exact_int_product(rp, col, val, x), "default stream"))
    S = sc.system("spd", 513)
    H = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    try:
        H.build_ic0()
        bs = dev(np.random.default_rng(6).standard_normal(513)); bd, z = torch.empty_like(bs), torch.empty_like(bs)
        env.pair([(bd, bs)], lambda: H.ic0_solve(bd, z, 2), [z], True, tag="ic0_solve", on_default=True, anchor=lambda r, o: st.no_nan(o))
    finally:
        H.destroy()


def test_default_stream_cg_solve(env, benches):
    """The same for a CG solve: b and the guess written late on the default stream."""
    L = sc.BY_NAME["cg_auto"]
    B = benches(L, 513)
    a = st.bench_solve(env, T, B, late=False)
    assert a["ret"] == 0
    st.same_solve(a, st.bench_solve(env, T, B, late=True, on_default=True), "CG, inputs written late on the default stream")


# ================================================================================================ switches
@pytest.fixture(scope="module")
def second(env, api):
    """A second side stream that does not queue behind the first: a product on it (the library switched to it) while the FIRST runs
    the delay and writes x late sees NaN -- otherwise the switch tests would be blind to a missing wait (stream_cases.pick_second)."""
    return st.pick_second(env)


def test_switch_then_read_the_product_and_reuse_the_plan(env, api, lib, second):
    """On S1: delay, late x, y = A.x with the binned plan.  Then lcg_hip_set_stream(S2), and on S2 an axpy that reads y and a second
    product of the same handle (its expand buffer is shared).  Both have the bits of the own-stream run; the switch drains nothing."""
    S1, S2 = env.need_stream(), second
    rng = np.random.default_rng(77)
    rp, col = _generated(api, 20000, api.GEN_SCRAMBLED, 0, 2)
    n = len(rp) - 1
    val, x = data(rng, rp, n, False, True)
    x2 = X.int_values(rng, n, 8, zeros=0.02); z0 = X.int_values(rng, n, 8)
    A = api.CsrMatrix.from_csr(rp, col, val)
    assert lib.lcg_hip_csr_set_binned(A.h, 1) == 0
    xs, x2d, z0s = dev(x), dev(x2), dev(z0)
    xd, y, y2, z = torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs)
    try:
        # reference, own stream
        A.spmv(xs, y); A.spmv(x2d, y2); z.copy_(z0s)
        assert lib.lcg_hip_axpy(n, 2.0, y.data_ptr(), z.data_ptr()) == 0
        api.synchronize(); torch.cuda.synchronize()
        assert lib.lcg_hip_csr_last_kernel(A.h).decode().startswith("k_bin_expand")
        ref = [t.cpu().numpy().copy() for t in (y, y2, z)]
        X.assert_rows(ref[0], rp, col, val, x, "binned")            # (products rounded before the add: the row bound, not the exact sum)
        X.assert_rows(ref[1], rp, col, val, x2, "binned")
        np.testing.assert_array_equal(ref[2], z0 + 2.0 * ref[0])
        for t in (xd, y, y2):
            st.nan_fill(t)
        z.copy_(z0s)
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(S1):
                api.use_torch_stream()
                E = env.delay.enqueue()
                xd.copy_(xs, non_blocking=True)
                assert not E.query(), st.PREMISE
                A.spmv(xd, y)
            with torch.cuda.stream(S2):
                api.use_torch_stream()          # S1 -> S2
                assert lib.lcg_hip_get_stream() == S2.cuda_stream
                assert lib.lcg_hip_axpy(n, 2.0, y.data_ptr(), z.data_ptr()) == 0
                A.spmv(x2d, y2)
                assert not E.query(), "the switch or the calls behind it drained the first stream"
                got = [t.clone() for t in (y, y2, z)]
                S2.synchronize()
            got = [t.cpu().numpy() for t in got]
        finally:
            api.use_own_stream()
            S1.synchronize()
        for name, a, b in zip(("y = A.x enqueued before the switch", "the second product of the same plan", "the axpy that reads y"), ref, got):
            assert a.tobytes() == b.tobytes(), (name, int(np.isnan(b).sum()), "NaN")
    finally:
        torch.cuda.synchronize()
        A.destroy()


def test_switch_between_two_applies_of_one_factor(env, api, lib, second):
    """On S1 a two-sided ic0_solve (its intermediate lives in the factor's tmp) of a vector written late; switch; the same handle
    applied to another vector on S2.  Both results are the own-stream bits."""
    S1, S2 = env.need_stream(), second
    arrays = tm.system("ic0", "layered")
    n = len(arrays[0]) - 1
    A = tm.build(api, "ic0", arrays)
    rng = np.random.default_rng(78)
    xs, x2 = dev(rng.standard_normal(n)), dev(rng.standard_normal(n))
    xd, y, y2 = torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs)
    try:
        A.ic0_solve(xs, y, 2); A.ic0_solve(x2, y2, 2)
        api.synchronize(); torch.cuda.synchronize()
        ref = [t.cpu().numpy().copy() for t in (y, y2)]
        st.no_nan(ref)
        for t in (xd, y, y2):
            st.nan_fill(t)
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(S1):
                api.use_torch_stream()
                E = env.delay.enqueue()
                xd.copy_(xs, non_blocking=True)
                assert not E.query(), st.PREMISE
                A.ic0_solve(xd, y, 2)
            with torch.cuda.stream(S2):
                api.use_torch_stream()
                A.ic0_solve(x2, y2, 2)
                assert not E.query(), "the switch or the apply behind it drained the first stream"
                got = [t.clone() for t in (y, y2)]
                S2.synchronize()
            got = [t.cpu().numpy() for t in got]
        finally:
            api.use_own_stream()
            S1.synchronize()
        for name, a, b in zip(("the apply enqueued before the switch", "the apply after it"), ref, got):
            assert a.tobytes() == b.tobytes(), (name, int(np.isnan(b).sum()), "NaN")
    finally:
        torch.cuda.synchronize()
        A.destroy()


def test_back_to_the_own_stream_and_synchronize(env, api, lib):
    """After work on S: lcg_hip_set_stream(NULL), lcg_hip_synchronize() -- the outputs are complete (the own stream waited for S)."""
    S = env.need_stream()
    A, xs, rp, col, val, x = env.control_system
    xd, y = torch.empty_like(xs), torch.empty_like(xs)
    st.nan_fill(xd); st.nan_fill(y)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(S):
            api.use_torch_stream()
            assert lib.lcg_hip_get_stream() == S.cuda_stream
            E = env.delay.enqueue()
            xd.copy_(xs, non_blocking=True)
            assert not E.query(), st.PREMISE
            A.spmv(xd, y)
    finally:
        api.use_own_stream()
    api.synchronize()
    assert E.query(), "lcg_hip_synchronize() on the own stream returned before the work enqueued on the previous stream was done"
    own = lib.lcg_hip_get_stream()
    assert own not in (None, 0, S.cuda_stream)
    X.assert_exact(y.cpu().numpy(), X.exact_int_product(rp, col, val, x), "after the switch back")
    S.synchronize()


def test_get_stream_and_setting_the_current_stream_again(env, api, lib):
    """lcg_hip_get_stream returns what was set, the own stream after NULL; setting the current stream again enqueues nothing: the
    delay is still running afterwards and no launch is counted."""
    S = env.need_stream()
    own = lib.lcg_hip_get_stream()
    assert own and own != S.cuda_stream
    try:
        with torch.cuda.stream(S):
            api.use_torch_stream()
            assert lib.lcg_hip_get_stream() == S.cuda_stream
            E = env.delay.enqueue()
            counts = lambda: tuple(c.value for c in _launches(lib))        # noqa: E731
            before = counts()
            for _ in range(3):
                api.use_torch_stream()
                env.set_stream_handle(S.cuda_stream)
            assert counts() == before
            assert lib.lcg_hip_get_stream() == S.cuda_stream
            assert not E.query(), "setting the current stream again waited for it"
            S.synchronize()
    finally:
        api.use_own_stream()
    assert lib.lcg_hip_get_stream() == own
    api.use_own_stream()
    assert lib.lcg_hip_get_stream() == own


def _launches(lib):
    c = [C.c_int(), C.c_int(), C.c_int(), C.c_int()]
    assert lib.lcg_hip_last_launches(*[C.byref(v) for v in c]) == 0
    return c
