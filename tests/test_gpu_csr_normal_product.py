"""-m gpu: the build and the products of include/lcg_hip_staging_csr_normal.h on the systems of tests/csr_normal_cases.py -- K^T itself
against numpy's stable transposition, K^T.x / K^T.K.x and their k-wide forms against exact integer sums and against extended-precision
sums under a two-level rounding bound, the carried dots, the independence of a column from k, its position and its neighbours, the
normal Jacobi, every refusal, and what lcg_hip_spmv_op still answers on such a handle.

The two-level bound.  y_hat = fl(K^T.t_hat), t_hat = fl(K.x).  By tests/exact_ref.py's argument a product of rows of at most L terms
in any order has |t_hat - t| <= gamma(L + 4) |K||x|, and the second product adds gamma(L_c + 4) |K^T||t_hat| (L_c: the row of K^T) and
carries the first one's error through |K^T|:
    |y_hat - y| <= gamma(L_c + 4) |K^T||t_hat| + |K^T| gamma(L + 4) |K||x|       elementwise,
against sums in extended precision whose own error, at most gamma_ld(L + L_c + 2) |K^T||K||x|, is added.
Integer data: with magnitudes <= 2^p, p = floor((52 - ceil(log2(L L_c))) / 3), every partial sum of both products is an integer below
2^52, so the results equal the int64 sums bit for bit (exact_ref's argument one level deeper)."""
import ctypes as C
import math

import numpy as np
import pytest

import csr_normal_cases as X
import exact_ref as er

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ALL = list(X.TABLE) + ["product_only"]
E_ARG = X.E_ARG


def _system(name):
    return X.product_only() if name == "product_only" else X.system(name)


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
            made[name] = X.handle(api, _system(name), jacobi=name != "product_only")
        return made[name]
    yield get
    for A in made.values():
        A.destroy()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a C-ordered copy: the cases' arrays are read-only)


def empty(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


# ================================================================================================ 1. K^T itself
@pytest.mark.parametrize("name", ALL)
def test_transpose_is_the_stable_transposition(api, lib, handles, name):
    S = _system(name)
    A = handles(name)
    assert A.n_cols == S["n"] and A.n == S["m"]
    rpT, ciT, vT = A.normal_to_host()
    assert np.array_equal(rpT, S["rpT"]) and np.array_equal(ciT, S["ciT"])
    assert np.array_equal(X.bits(vT), X.bits(S["vT"]))
    info = A.normal_info()
    assert info["longest_column"] == int(np.diff(S["rpT"]).max())
    assert info["extra_bytes"] >= 12 * len(ciT) + 4 * (S["n"] + 1) + 8 * S["m"] and info["build_ms"] > 0.0
    # idempotent: a second call keeps the arrays where they are
    ptrs = [C.c_void_p() for _ in range(3)]
    lib.lcg_hip_csr_normal_arrays(A.h, *[C.byref(p) for p in ptrs])
    A.build_normal()
    again = [C.c_void_p() for _ in range(3)]
    lib.lcg_hip_csr_normal_arrays(A.h, *[C.byref(p) for p in again])
    assert [p.value for p in ptrs] == [p.value for p in again]
    # two builds agree bit for bit
    B = X.handle(api, S, jacobi=False)
    for a, b in zip(B.normal_to_host(), (rpT, ciT, vT)):
        assert a.tobytes() == b.tobytes()
    B.destroy()


def test_same_values_everywhere_keep_the_entry_order(api):
    """Duplicates that a value rule could not tell apart -- equal values, -0.0 beside 0.0, a NaN: the order is K's own."""
    rp = np.array([0, 4, 4, 7], np.int32)
    ci = np.array([1, 1, 0, 1, 1, 0, 1], np.int32)
    v = np.array([0.0, -0.0, 5.0, np.nan, 2.0, 1.0, 2.0])
    A = api.CsrMatrix.from_csr(rp, ci, v, n_cols=3)
    A.build_normal()
    want = X.transpose_host(rp, ci, v, 3)
    for a, b in zip(A.normal_to_host(), want):
        assert a.tobytes() == np.ascontiguousarray(b).tobytes()
    assert A.normal_info()["longest_column"] == 5
    A.destroy()


# ================================================================================================ 2. integer data
def _int_system(S, seed):
    L, Lc = int(np.diff(S["rp"]).max()), int(np.diff(S["rpT"]).max())
    p = (52 - math.ceil(math.log2(L * Lc))) // 3
    assert p >= 1
    rng = np.random.default_rng(seed)
    v = er.int_values(rng, len(S["ci"]), p)
    return p, rng, v


def _int_ata(S, v, X_int):
    """K^T.(K.X) and K.X in int64 for integer-valued columns."""
    rows = np.repeat(np.arange(S["m"]), np.diff(S["rp"]))
    vi, Xi = v.astype(np.int64), X_int.astype(np.int64)
    T = np.zeros((S["m"], Xi.shape[1]), np.int64)
    np.add.at(T, rows, vi[:, None] * Xi[S["ci"]])
    Y = np.zeros((S["n"], Xi.shape[1]), np.int64)
    np.add.at(Y, S["ci"], vi[:, None] * T[rows])
    bound = np.zeros((S["n"], Xi.shape[1]), np.int64)
    Ta = np.zeros_like(T); np.add.at(Ta, rows, np.abs(vi[:, None] * Xi[S["ci"]]))
    np.add.at(bound, S["ci"], np.abs(vi[:, None]) * Ta[rows])
    assert bound.max() <= 2 ** 52, "the magnitude rule"
    return T, Y


@pytest.mark.parametrize("name", ["product_only", "edge65", "wide513", "dense3000", "tall9000", "tiny3x1"])
def test_integer_data_are_exact(api, name):
    S = _system(name)
    p, rng, v = _int_system(S, 31)
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], v, n_cols=S["n"])
    A.build_normal()
    for k in X.KS:
        Xi = er.int_values(rng, (S["n"], k), p)
        T, Y = _int_ata(S, v, Xi)
        Yd = empty(S["n"], k)
        A.ata_multi(dev(Xi), Yd); api.synchronize()
        er.assert_exact(Yd.cpu().numpy(), Y.astype(np.float64), (name, "ata_multi", k))
        # K^T alone on the exact K.X (an integer block of at most 2^(2p) L)
        Yt = empty(S["n"], k)
        A.spmm_t(dev(T.astype(np.float64)), Yt); api.synchronize()
        er.assert_exact(Yt.cpu().numpy(), Y.astype(np.float64), (name, "spmm_t", k))
    x = er.int_values(rng, S["n"], p)
    T, Y = _int_ata(S, v, x[:, None])
    y = empty(S["n"])
    A.ata(dev(x), y); api.synchronize()
    er.assert_exact(y.cpu().numpy(), Y[:, 0].astype(np.float64), (name, "ata"))
    y2 = empty(S["n"])
    A.spmv_t(dev(T[:, 0].astype(np.float64)), y2); api.synchronize()
    er.assert_exact(y2.cpu().numpy(), Y[:, 0].astype(np.float64), (name, "spmv_t"))
    # in place: x and y the same vector
    xy = dev(x)
    A.ata(xy, xy); api.synchronize()
    er.assert_exact(xy.cpu().numpy(), Y[:, 0].astype(np.float64), (name, "ata in place"))
    A.destroy()


# ================================================================================================ 3. full-mantissa data
def _two_level(S, x, t_hat):
    """(the exact K^T.(K.x) as longdouble, the bound of the module docstring)"""
    assert er.LONGDOUBLE_OK
    LD = np.longdouble
    L, Lc = er.lengths(S["rp"]).astype(np.float64), er.lengths(S["rpT"]).astype(np.float64)
    t = er._row_sum(S["v"].astype(LD) * x.astype(LD)[S["ci"]], S["rp"])
    y = er._row_sum(S["vT"].astype(LD) * t[S["ciT"]], S["rpT"])
    up = 1.0 + 4 * er.U * (L.max() + Lc.max() + 4)                                      # (the bound's own sums, rounded up)
    kx_abs = er._row_sum(np.abs(S["v"]) * np.abs(x)[S["ci"]], S["rp"]) * up
    first = er._row_sum(np.abs(S["vT"]) * (er.gamma(L + 4) * kx_abs)[S["ciT"]], S["rpT"]) * up
    second = er.gamma(Lc + 4) * er._row_sum(np.abs(S["vT"]) * np.abs(t_hat)[S["ciT"]], S["rpT"]) * up
    own = er.gamma(L.max() + Lc + 2, er.ULD) * er._row_sum(np.abs(S["vT"]) * kx_abs[S["ciT"]], S["rpT"]) * up
    return y, first + second + own + 1e-300


@pytest.mark.parametrize("name", ALL)
def test_full_mantissa_data_within_the_two_level_bound(api, handles, name):
    S = _system(name)
    A = handles(name)
    rng = np.random.default_rng(5)
    worst = 0.0
    for k in X.KS:
        Xh = rng.uniform(-1.0, 1.0, (S["n"], k)) * 2.0 ** rng.integers(-8, 9, (S["n"], k))
        Yd, Td = empty(S["n"], k), empty(S["m"], k)
        A.ata_multi(dev(Xh), Yd)
        A.spmm(dev(Xh), Td); api.synchronize()
        Y, T = Yd.cpu().numpy(), Td.cpu().numpy()
        Yt = empty(S["n"], k)
        A.spmm_t(Td, Yt); api.synchronize()
        assert np.array_equal(X.bits(Yt.cpu().numpy()), X.bits(Y)), "K^T.(K.X) is spmm_t of spmm"
        for j in range(k):
            exact, bound = _two_level(S, Xh[:, j], T[:, j])
            err = np.abs((Y[:, j].astype(np.longdouble) - exact).astype(np.float64))
            assert np.all(err <= bound), (name, k, j, int(np.argmax(err / bound)), float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            # K^T alone: exact_ref's one-level bound with the rows of K^T
            er.assert_rows(Y[:, j], S["rpT"], S["ciT"], S["vT"], T[:, j], (name, "spmm_t", k, j))
    x = rng.uniform(-1.0, 1.0, S["n"])
    y, t = empty(S["n"]), empty(S["m"])
    A.ata(dev(x), y)
    A.spmv(dev(x), t); api.synchronize()
    exact, bound = _two_level(S, x, t.cpu().numpy())
    err = np.abs((y.cpu().numpy().astype(np.longdouble) - exact).astype(np.float64))
    assert np.all(err <= bound), (name, "ata", float((err / bound).max()))
    y2 = empty(S["n"])
    A.spmv_t(t, y2); api.synchronize()
    assert np.array_equal(X.bits(y2.cpu().numpy()), X.bits(y.cpu().numpy())), "K^T.(K.x) is spmv_t of spmv"
    er.assert_rows(y2.cpu().numpy(), S["rpT"], S["ciT"], S["vT"], t.cpu().numpy(), (name, "spmv_t"))
    print(f"{name}: worst ratio of an error to the two-level bound {max(worst, float((err / bound).max())):.3g}")


# ================================================================================================ 4. dots, 5. independence
@pytest.mark.parametrize("name", ["edge65", "dense3000", "tall9000", "main", "tiny5x2"])
def test_dots_and_column_independence(api, handles, name):
    S = _system(name)
    A = handles(name)
    n = S["n"]
    rng = np.random.default_rng(9)
    X8, U8 = rng.standard_normal((n, 8)), rng.standard_normal((n, 8))
    Y8 = empty(n, 8)
    d8 = A.ata_multi_dot(dev(X8), Y8, dev(U8)); api.synchronize()
    Y8h = Y8.cpu().numpy()
    plain = empty(n, 8)
    A.ata_multi(dev(X8), plain); api.synchronize()
    assert np.array_equal(X.bits(plain.cpu().numpy()), X.bits(Y8h)), "the carried sum does not change Y"
    for j in range(8):
        er.assert_dot(d8[j], Y8h[:, j], U8[:, j], (name, j))
    # call to call
    Y8b = empty(n, 8)
    d8b = A.ata_multi_dot(dev(X8), Y8b, dev(U8)); api.synchronize()
    assert np.array_equal(X.bits(d8b), X.bits(d8)) and np.array_equal(X.bits(Y8b.cpu().numpy()), X.bits(Y8h))
    # k and position
    for k, picks in ((2, (0, 1)), (2, (5, 2)), (4, (4, 2, 1, 7)), (4, (3, 0, 6, 2)), (8, (7, 6, 5, 4, 3, 2, 1, 0))):
        Yk = empty(n, k)
        dk = A.ata_multi_dot(dev(X8[:, picks]), Yk, dev(U8[:, picks])); api.synchronize()
        Ykh = Yk.cpu().numpy()
        for pos, j in enumerate(picks):
            assert np.array_equal(X.bits(Ykh[:, pos]), X.bits(Y8h[:, j])) and X.bits(dk[pos:pos + 1])[0] == X.bits(d8[j:j + 1])[0], (name, k, pos, j)
        Tk = empty(n, k)
        A.ata_multi(dev(X8[:, picks]), Tk); api.synchronize()
        assert np.array_equal(X.bits(Tk.cpu().numpy()), X.bits(Ykh))
    # neighbours: NaN, Inf, huge
    Xn, Un = X8[:, :4].copy(), U8[:, :4].copy()
    Xn[:, 0] = np.nan; Xn[n // 2, 2] = np.inf; Xn[:, 3] *= 1e200; Un[0, 0] = np.inf
    Yn = empty(n, 4)
    dn = A.ata_multi_dot(dev(Xn), Yn, dev(Un)); api.synchronize()
    assert np.array_equal(X.bits(Yn.cpu().numpy()[:, 1]), X.bits(Y8h[:, 1])) and X.bits(dn[1:2])[0] == X.bits(d8[1:2])[0]
    assert np.isnan(Yn.cpu().numpy()[:, 0]).all()


# ================================================================================================ 6. Jacobi
@pytest.mark.parametrize("name", list(X.TABLE))
def test_normal_jacobi(api, lib, handles, name):
    S = _system(name)
    A = handles(name)
    n = S["n"]
    d = empty(n)
    A.build_jacobi_normal(d); api.synchronize()
    dh = d.cpu().numpy()
    # the column sums of squares: within gamma(L_c + 1) of the exact sum (L_c rounded squares, any order): tests/test_gpu_dense.py:276
    LD = np.longdouble
    exact = er._row_sum(S["vT"].astype(LD) ** 2, S["rpT"])
    Lc = er.lengths(S["rpT"])
    assert np.all(np.abs((dh.astype(LD) - exact).astype(np.float64)) <= er.gamma(Lc + 1) * exact.astype(np.float64)), name
    np.testing.assert_allclose(dh, X.normal_diagonal(S), rtol=float(2 * er.gamma(Lc.max() + 1)))
    x = np.random.default_rng(3).standard_normal(n)
    z = empty(n)
    lib.lcg_hip_csr_jacobi_normal_mx(A.h, dev(x).data_ptr(), z.data_ptr(), n); api.synchronize()
    assert np.array_equal(z.cpu().numpy(), x * (1.0 / dh)), name        # the reciprocal is one division
    d2 = empty(n)
    A.build_jacobi_normal(d2); api.synchronize()
    assert np.array_equal(X.bits(d2.cpu().numpy()), X.bits(dh))


def test_a_column_no_datum_sees_is_named_and_nothing_is_stored(api, lib, handles):
    A = handles("product_only")
    n = X.product_only()["n"]
    d = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    assert lib.lcg_hip_csr_build_jacobi_normal(A.h, d.data_ptr()) == E_ARG
    err = lib.lcg_hip_last_error().decode()
    assert "lcg_hip_csr_build_jacobi_normal" in err and "column 0 " in err, err
    api.synchronize()
    assert (d.cpu().numpy() == 7.0).all()
    B = dev(np.ones((n, 2))); M = torch.zeros_like(B)
    ret = (C.c_int * 2)(); its = (C.c_int * 2)(); res = (C.c_double * 2)()
    p = api.lcg_default_parameters(epsilon=1e-10, max_iterations=3)
    assert lib.lcg_hip_csr_normal_lpcg_multi(A.h, 2, M.data_ptr(), B.data_ptr(), C.byref(p), ret, its, res, 1) == X.NOPRE
    # the square diagonal's reciprocals are another thing: building them does not make the normal ones
    S = X.system("tiny3x1")
    sq = api.CsrMatrix.from_csr(np.arange(4, dtype=np.int32), np.arange(3, dtype=np.int32), np.array([2.0, 4.0, 8.0]))
    sq.build_jacobi(); sq.build_normal()
    B3 = dev(np.ones((3, 2))); M3 = torch.zeros_like(B3)
    assert lib.lcg_hip_csr_normal_lpcg_multi(sq.h, 2, M3.data_ptr(), B3.data_ptr(), C.byref(p), ret, its, res, 1) == X.NOPRE
    sq.build_jacobi_normal()
    z = empty(3)
    lib.lcg_hip_jacobi_mx(sq.h, dev(np.ones(3)).data_ptr(), z.data_ptr(), 3); api.synchronize()
    assert np.array_equal(z.cpu().numpy(), 1.0 / np.array([2.0, 4.0, 8.0]))
    lib.lcg_hip_csr_jacobi_normal_mx(sq.h, dev(np.ones(3)).data_ptr(), z.data_ptr(), 3); api.synchronize()
    assert np.array_equal(z.cpu().numpy(), 1.0 / np.array([4.0, 16.0, 64.0]))
    sq.destroy()
    assert S["n"] == 1


# ================================================================================================ 7. refusals
def _entry_calls(lib, h, n, m, k=4):
    """name -> a call of every entry that needs the normal state, on well-formed device vectors"""
    x, y, t = empty(n * k), empty(n * k), empty(m * k)
    x.zero_(); t.zero_()
    lo = torch.zeros(n, dtype=torch.float64, device="cuda")
    out = (C.c_double * 8)()
    ret = (C.c_int * 8)(*([99] * 8)); its = (C.c_int * 8)(); pr = (C.c_int * 8)(); res = (C.c_double * 8)()
    keep = (x, y, t, lo, out, ret, its, pr, res)
    P = lambda a: a.data_ptr()      # noqa: E731
    return keep, ret, {
        "lcg_hip_csr_normal_info": lambda: lib.lcg_hip_csr_normal_info(h, None, None, None),
        "lcg_hip_csr_normal_arrays": lambda: lib.lcg_hip_csr_normal_arrays(h, None, None, None),
        "lcg_hip_spmv_t": lambda: lib.lcg_hip_spmv_t(h, P(t), P(y)),
        "lcg_hip_csr_ata": lambda: lib.lcg_hip_csr_ata(h, P(x), P(y)),
        "lcg_hip_csr_build_jacobi_normal": lambda: lib.lcg_hip_csr_build_jacobi_normal(h, None),
        "lcg_hip_spmm_t": lambda: lib.lcg_hip_spmm_t(h, k, P(t), P(y)),
        "lcg_hip_csr_ata_multi": lambda: lib.lcg_hip_csr_ata_multi(h, k, P(x), P(y)),
        "lcg_hip_csr_ata_multi_dot": lambda: lib.lcg_hip_csr_ata_multi_dot(h, k, P(x), P(y), P(x), out),
        "lcg_hip_csr_normal_lcg_multi": lambda: lib.lcg_hip_csr_normal_lcg_multi(h, k, P(y), P(x), None, ret, its, res, 1),
        "lcg_hip_csr_normal_lpcg_multi": lambda: lib.lcg_hip_csr_normal_lpcg_multi(h, k, P(y), P(x), None, ret, its, res, 1),
        "lcg_hip_csr_normal_solver_constrained_multi":
            lambda: lib.lcg_hip_csr_normal_solver_constrained_multi(h, k, X.SPG, P(y), P(x), P(lo), P(lo), None, ret, its, pr, res, 1),
    }


def test_refusals(api, lib):
    S = X.system("small")
    n, m = S["n"], S["m"]
    err = lambda: lib.lcg_hip_last_error().decode()     # noqa: E731
    bare = X.handle(api, S, normal=False)
    Dn = api.DenseMatrix.from_array(np.eye(4))
    Zc = api.CsrMatrix.from_csr(np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4) + 0j)
    Z64 = api.CsrMatrix.from_csr_c64(np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4, np.complex64))
    # sharded on one GPU (tests/test_gpu_multi_product.py): rank 0's 4 rows of an 8 x 8 system, split into its local and remote parts --
    # one without a normal state, one whose state was built while it was whole
    shards = []
    for built in (False, True):
        Zs = api.CsrMatrix.from_csr(np.arange(5, dtype=np.int32), np.array([0, 5, 2, 7], np.int32), np.ones(4), n_cols=8)
        if built:
            Zs.build_normal()
            assert lib.lcg_hip_csr_ata(Zs.h, dev(np.ones(8)).data_ptr(), empty(8).data_ptr()) == 0      # served while it is whole
        assert lib.lcg_hip_csr_split_for_test(Zs.h, 8, 2, 0) == 0
        shards.append(Zs)
    try:
        # handles of another kind: before anything else, nothing written
        for H, word in ((Dn, "dense"), (Zc, "complex"), (Z64, "complex64"), (shards[0], "sharded"), (shards[1], "sharded")):
            keep, ret, calls = _entry_calls(lib, H.h, 4, 4)
            calls["lcg_hip_csr_build_normal"] = lambda H=H: lib.lcg_hip_csr_build_normal(H.h)
            for name, call in calls.items():
                assert call() == E_ARG, (word, name)
                assert name in err() and word in err() and "square" not in err(), (word, name, err())
            api.synchronize()
            assert list(ret) == [99] * 8 and torch.isnan(keep[1]).all()
        assert lib.lcg_hip_csr_cols(Dn.h) == E_ARG
        assert [lib.lcg_hip_csr_cols(H.h) for H in (Zc, Z64, *shards)] == [4, 4, 8, 8]        # the query serves every CSR handle
        # no normal state: every entry names the build
        keep, ret, calls = _entry_calls(lib, bare.h, n, m)
        for name, call in calls.items():
            assert call() == E_ARG, name
            assert name + ":" in err() and "lcg_hip_csr_build_normal" in err() and "square" not in err(), (name, err())
        api.synchronize()
        assert list(ret) == [99] * 8 and torch.isnan(keep[1]).all()
        # ... the callbacks park it: the solve ends with the code
        para = api.lcg_default_parameters(epsilon=1e-10, max_iterations=5)
        b = dev(S["b"]); mm = torch.zeros_like(b)
        assert lib.lcg_hip_solver(api.L.fnptr(lib, "lcg_hip_csr_ata_ax"), None, mm.data_ptr(), b.data_ptr(), n, C.byref(para), bare.h, X.CG, 1) == E_ARG
        assert "lcg_hip_csr_ata_ax" in err() and "lcg_hip_csr_build_normal" in err()
        # with the state: the entries' own checks, then the reference's codes in its order, then the missing diagonal
        bare.build_normal()
        assert lib.lcg_hip_solver(api.L.fnptr(lib, "lcg_hip_csr_ata_ax"), None, mm.data_ptr(), b.data_ptr(), n, C.byref(para), bare.h, X.CG, 1) == X.MAXIT
        sq = api.CsrMatrix.from_csr(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))
        sq.build_normal()
        bm = dev(np.ones(n)); m2 = torch.zeros_like(bm)
        for fn in ("lcg_hip_csr_ata_ax",):
            rc = lib.lcg_hip_solver(api.L.fnptr(lib, fn), None, m2.data_ptr(), bm.data_ptr(), n - 1, C.byref(para), sq.h, X.CG, 1)
            assert rc == E_ARG and "n_size" in err() and fn in err(), (rc, err())
        # the Jacobi callback's own refusals, parked like the product's: the reciprocals not built, then n_size
        zj = empty(n)
        rc = lib.lcg_hip_solver_preconditioned(api.L.fnptr(lib, "lcg_hip_csr_ata_ax"), api.L.fnptr(lib, "lcg_hip_csr_jacobi_normal_mx"), None,
                                               m2.data_ptr(), bm.data_ptr(), n, C.byref(para), sq.h, X.PCG, 1)
        assert rc == E_ARG and "lcg_hip_csr_jacobi_normal_mx" in err() and "lcg_hip_csr_build_jacobi_normal was not called" in err(), (rc, err())
        lib.lcg_hip_csr_jacobi_normal_mx(sq.h, bm.data_ptr(), zj.data_ptr(), n); api.synchronize()
        assert "was not called" in err() and torch.isnan(zj).all()
        assert lib.lcg_hip_csr_build_jacobi_normal(sq.h, None) == 0
        lib.lcg_hip_csr_jacobi_normal_mx(sq.h, bm.data_ptr(), zj.data_ptr(), n - 1); api.synchronize()
        assert "lcg_hip_csr_jacobi_normal_mx: n_size" in err() and torch.isnan(zj).all(), err()
        lib.lcg_hip_csr_jacobi_normal_mx(sq.h, bm.data_ptr(), zj.data_ptr(), n); api.synchronize()
        assert (zj.cpu().numpy() == 1.0).all()
        assert lib.lcg_hip_solver_preconditioned(api.L.fnptr(lib, "lcg_hip_csr_ata_ax"), api.L.fnptr(lib, "lcg_hip_csr_jacobi_normal_mx"), None,
                                                 m2.data_ptr(), bm.data_ptr(), n, C.byref(para), sq.h, X.PCG, 1) in (X.CONV, X.ALREADY, X.MAXIT)
        sq.destroy()
        B = dev(X.columns(S, 4)); M = torch.zeros_like(B); lo = dev(np.zeros(n)); hi = dev(np.ones(n))
        ret = (C.c_int * 4)(*([99] * 4)); its = (C.c_int * 4)(); pr = (C.c_int * 4)(); res = (C.c_double * 4)()
        for fn in (lib.lcg_hip_csr_normal_lcg_multi, lib.lcg_hip_csr_normal_lpcg_multi):
            assert fn(bare.h, 4, M.data_ptr(), B.data_ptr(), C.byref(api.lcg_default_parameters(max_iterations=-1, epsilon=0.0)), ret, its, res, 1) == X.BADCAP
            assert fn(bare.h, 4, M.data_ptr(), B.data_ptr(), C.byref(api.lcg_default_parameters(epsilon=0.0)), ret, its, res, 1) == X.BADEPS
            assert fn(bare.h, 4, M.data_ptr(), B.data_ptr(), C.byref(api.lcg_default_parameters(epsilon=1.0)), ret, its, res, 1) == X.BADEPS
            assert fn(bare.h, 4, M.data_ptr(), B.data_ptr(), C.byref(para), ret, its, res, 5) == E_ARG and "mem" in err()
        assert lib.lcg_hip_csr_normal_lpcg_multi(bare.h, 4, M.data_ptr(), B.data_ptr(), C.byref(para), ret, its, res, 1) == X.NOPRE
        assert lib.lcg_hip_csr_normal_lpcg_multi(bare.h, 4, M.data_ptr(), B.data_ptr(), C.byref(api.lcg_default_parameters(epsilon=0.0)), ret, its, res, 1) == X.BADEPS
        box = lib.lcg_hip_csr_normal_solver_constrained_multi
        args = (M.data_ptr(), B.data_ptr(), lo.data_ptr(), hi.data_ptr())
        assert box(bare.h, 4, X.SPG, *args, C.byref(api.lcg_default_parameters(max_iterations=-1)), ret, its, pr, res, 1) == X.BADCAP
        assert box(bare.h, 4, X.SPG, *args, C.byref(api.lcg_default_parameters(epsilon=1e-10, sigma=0.0)), ret, its, pr, res, 1) == -1014   # LCG_INVALID_SIGMA
        assert box(bare.h, 4, X.PG, *args, C.byref(api.lcg_default_parameters(epsilon=1e-10, step=0.0)), ret, its, pr, res, 1) == -1015     # LCG_INVALID_LAMBDA
        assert box(bare.h, 4, X.SPG, *args, C.byref(api.lcg_default_parameters(epsilon=1e-10, maxi_m=65)), ret, its, pr, res, 1) == E_ARG and "maxi_m" in err()
        assert list(ret) == [99] * 4 and not M.any()
        assert lib.lcg_hip_csr_normal_lcg_multi(bare.h, 4, M.data_ptr(), B.data_ptr(), C.byref(para), ret, its, res, 1) == 0 and list(ret) == [X.MAXIT] * 3 + [X.ALREADY]
        # a column index outside [0, n_cols)
        bad = api.CsrMatrix.from_csr(np.array([0, 2, 3], np.int32), np.array([0, 5, 1], np.int32), np.ones(3), n_cols=4)
        assert lib.lcg_hip_csr_build_normal(bad.h) == E_ARG and "outside [0, 4)" in err()
        assert lib.lcg_hip_csr_ata(bad.h, M.data_ptr(), M.data_ptr()) == E_ARG and "lcg_hip_csr_build_normal" in err()
        bad.destroy()
    finally:
        for H in (bare, Dn, Zc, Z64, *shards):
            H.destroy()


# ================================================================================================ 8. existing behaviour
def test_spmv_op_still_refuses_a_rectangular_matrix(api, lib):
    """lcg_hip_spmv_op(layout = 1) on a non-square handle: the same code and text with and without the normal state; layout 0 is
    lcg_hip_spmv."""
    S = X.system("small")
    A = X.handle(api, S, normal=False)
    x, t = dev(S["xt"]), empty(S["m"])
    y = empty(S["n"])
    rc0 = lib.lcg_hip_spmv_op(A.h, t.data_ptr(), y.data_ptr(), 1, 0)
    e0 = lib.lcg_hip_last_error().decode()
    assert rc0 == -2000 and "op(A) needs a square matrix" in e0, (rc0, e0)          # LCG_HIP_E_RUNTIME
    assert lib.lcg_hip_spmv_op(A.h, x.data_ptr(), t.data_ptr(), 0, 0) == 0
    api.synchronize()
    t0 = t.cpu().numpy().copy()
    A.build_normal()
    rc1 = lib.lcg_hip_spmv_op(A.h, t.data_ptr(), y.data_ptr(), 1, 0)
    assert (rc1, lib.lcg_hip_last_error().decode()) == (rc0, e0)
    t2 = empty(S["m"])
    assert lib.lcg_hip_spmv_op(A.h, x.data_ptr(), t2.data_ptr(), 0, 0) == 0
    api.synchronize()
    assert np.array_equal(X.bits(t2.cpu().numpy()), X.bits(t0)) and torch.isnan(y).all()
    A.destroy()
