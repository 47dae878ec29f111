"""-m gpu: the dense products over k = 2, 4, 8 right-hand sides (liblcg_amd/csrc/dense_multi.hip): K.X, K^T.X, K^T.(K.X) and the
operator with its carried sum, against exact integer sums (bit for bit) and per-row rounding bounds (tests/exact_ref.py), every
k-wide kernel family reached; column j's bits the same at k = 2, 4, 8, whatever the other columns hold and from call to call;
nothing read behind X or U (every block handed to the device here sits in a larger buffer with NaN directly behind its last row);
Y fully written; the refusals.

Shapes and the branch each is the smallest to reach (dense.hpp: row_plan, col_plan; NP = ceil(N / 2) packs per row):
  (1, 1) W = 4, one row, odd N      (50, 13) W = 8, odd N        (37, 29) W = 16, odd N, created with ld > N
  (100, 80) W = 64; forced split: two strips, W = 32             (1000, 800) one strip although M < 1024; forced split: nine
  (1, 4097), (3, 5000) the automatic split, odd N / even N       (8191, 1025) 8191 rows x 513 packs, forced split: two strips
  column form: (3, 5000), (1, 4097), (1000, 800), (8191, 1025) one strip of rows (RS = 1); (4097, 1), (5000, 3), (100, 80) folded"""
import ctypes as C
import math

import numpy as np
import pytest

import dense_checker as dc
import exact_ref as er

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = [(1, 1), (1, 4097), (4097, 1), (3, 5000), (5000, 3), (100, 80), (1000, 800), (8191, 1025), (50, 13)]
KS = (2, 4, 8)
E_ARG = -2003


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


def _poisoned(X):
    """X (rows, k) on the device, inside a larger buffer with NaN directly behind its last row."""
    rows, k = X.shape
    buf = torch.full((rows * k + 64,), float("nan"), dtype=torch.float64, device="cuda")
    buf[:rows * k] = torch.from_numpy(np.ascontiguousarray(X).reshape(-1)).cuda()
    v = buf[:rows * k].view(rows, k)
    assert v.data_ptr() % 16 == 0
    return v


def _mm(api, D, X, out_rows, layout=0, ata=False):
    """One k-wide product into a Y pre-filled with NaN; X from a poisoned buffer."""
    Xd = _poisoned(X)
    Y = torch.full((out_rows, X.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
    if ata:
        D.ata_multi(Xd, Y)
    else:
        D.matmat(Xd, Y, layout)
    api.synchronize()
    return Y.cpu().numpy()


def _full(rng, shape):
    return rng.standard_normal(shape) * np.exp2(rng.integers(-6, 7, shape))


def _can_split(m, n):
    """lcg_hip_dense_set_kernel(K, 2) is refused where the columns cannot be cut (tests/test_gpu_dense.py)."""
    return (n + 1) // 2 >= 32 and m < 8192


def _ata_bits(m, n):
    p = (52 - math.ceil(math.log2(m * n))) // 3
    assert p >= 1
    return p


def _exact(Ki, Xi):
    """Ki.Xi for integer-valued float64 data, exactly (int64), with the magnitude rule of exact_ref.exact_int_product."""
    a, x = Ki.astype(np.int64), Xi.astype(np.int64)
    assert np.all(np.abs(a).astype(np.float64) @ np.abs(x).astype(np.float64) <= 2.0 ** 53)
    return (a @ x).astype(np.float64)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_exact_sums_and_every_path(api):
    """Integer data: the device's Y equals the exact sums bit for bit, whatever the summation order, for k = 2, 4, 8, the automatic
    and the forced row forms.  The union of the k-wide kernels that ran must be the library's whole list."""
    lib = api.L.load()
    seen = set()
    names = api.DenseMatrix.multi_kernel_names()
    for (m, n, pad) in [(m, n, 0) for (m, n) in SHAPES] + [(37, 29, 11)]:       # the last one: ld > N
        rng = np.random.default_rng(m * 7919 + n)
        p = er.int_bits(max(m, n))
        K = er.int_values(rng, (m, n), p)
        if pad:
            wide = np.full((m, n + pad), 7.0); wide[:, :n] = K
            D = api.DenseMatrix.from_array(wide[:, :n])
        else:
            D = api.DenseMatrix.from_array(K)
        pa = _ata_bits(m, n)
        Ka = er.int_values(rng, (m, n), pa)
        Da = api.DenseMatrix.from_rows([Ka[i] for i in range(m)])
        assert D.multi_last_kernel == ""
        for k in KS:
            X = er.int_values(rng, (n, k), p); Xt = er.int_values(rng, (m, k), p); Xa = er.int_values(rng, (n, k), pa)
            want, want_t = _exact(K, X), _exact(K.T, Xt)
            want_a = _exact(Ka.T, _exact(Ka, Xa))
            for variant in (0, 1, 2):
                if variant == 2 and not _can_split(m, n):
                    assert lib.lcg_hip_dense_set_kernel(D.h, 2) == E_ARG          # refused: nothing to split
                    continue
                D.set_kernel(variant); Da.set_kernel(variant)
                er.assert_exact(_mm(api, D, X, m), want, (m, n, k, "K.X", variant))
                seen.add(D.multi_last_kernel)
                if variant:
                    assert D.multi_last_kernel == names[variant - 1]
                er.assert_exact(_mm(api, Da, Xa, n, ata=True), want_a, (m, n, k, "ata", variant))
                seen.add(Da.multi_last_kernel)
                assert Da.multi_last_kernel == "k_dnm_ata_two_pass"
            D.set_kernel(0); Da.set_kernel(0)
            er.assert_exact(_mm(api, D, Xt, n, layout=1), want_t, (m, n, k, "K^T.X"))
            seen.add(D.multi_last_kernel)
            assert D.multi_last_kernel == "k_dnm_col"
        # variants 4 - 6 are not looked at by the k-wide products
        for variant in (4, 5, 6):
            if lib.lcg_hip_dense_set_kernel(Da.h, variant) == 0:
                er.assert_exact(_mm(api, Da, Xa, n, ata=True), want_a, (m, n, "ata", variant))
        assert D.last_kernel == ""              # the single-vector name is not touched
        D.destroy(); Da.destroy()
    assert seen == set(names), (sorted(seen), names)


@pytest.mark.parametrize("shape", SHAPES + [(37, 29)])
def test_full_mantissa_rows_within_the_rounding_bound(api, shape):
    """Every column of every product within exact_ref's per-row bound.  K^T.(K.X): the second stage against the device's own first
    stage plus |K^T| dt, as tests/test_gpu_dense.py bounds the single product.  k = 8 (the largest shape: k = 2, for the host's time;
    the columns' bits do not depend on k, which test_columns_do_not_depend_on_k_neighbours_or_the_call pins)."""
    m, n = shape
    k = 8 if m * n <= 1 << 20 else 2
    rng = np.random.default_rng(m * 131 + n)
    K = _full(rng, (m, n))
    KT = np.ascontiguousarray(K.T)
    csr, csr_t = dc.dense_as_csr(K), dc.dense_as_csr(KT)
    D = api.DenseMatrix.from_array(torch.from_numpy(K).cuda())
    X, Xt = _full(rng, (n, k)), _full(rng, (m, k))
    for variant in (0, 1, 2):
        if variant == 2 and not _can_split(m, n):
            continue
        D.set_kernel(variant)
        Y = _mm(api, D, X, m)
        for j in range(k):
            er.assert_rows(Y[:, j], *csr, X[:, j], tag=(shape, k, j, "K.X", variant))
    D.set_kernel(0)
    Yt = _mm(api, D, Xt, n, layout=1)
    for j in range(k):
        er.assert_rows(Yt[:, j], *csr_t, Xt[:, j], tag=(shape, k, j, "K^T.X"))
    T = _mm(api, D, X, m)
    for variant in (0, 1, 2):
        if variant == 2 and not _can_split(m, n):
            continue
        D.set_kernel(variant)
        Tv = T if variant == 0 else _mm(api, D, X, m)
        Ya = _mm(api, D, X, n, ata=True)
        for j in range(k):
            ref = er.hp_product(*csr_t, Tv[:, j])
            err = er.row_errors(Ya[:, j], ref)
            dt = er.bound_f64(np.full(m, n), er.hp_product(*csr, X[:, j])[2])
            bound = er.bound_f64(np.full(n, m), ref[2]) + 2.0 * (np.abs(KT) @ dt)
            assert np.all(err <= bound), (shape, variant, j, float(np.max(err / bound)))
    D.destroy()


@pytest.mark.parametrize("shape", [(1000, 800), (3, 5000), (5000, 3), (37, 29), (257, 257)])
def test_columns_do_not_depend_on_k_neighbours_or_the_call(api, shape, capsys):
    """Column j of K.X, K^T.X, K^T.(K.X) and dots[j] of the operator with its carried sum: the same bits at k = 2, 4 and 8, with the
    neighbours replaced by other data, NaN and +-Inf, at another position of the block, and over five calls.  The sums are held to
    exact_ref.assert_dot's bound.  Whether a column also has the bits of the single-vector product is printed, not asserted."""
    m, n = shape
    rng = np.random.default_rng(m + 17 * n)
    K = _full(rng, (m, n))
    D = api.DenseMatrix.from_array(K)
    square = m == n
    X8, Xt8, U8 = _full(rng, (n, 8)), _full(rng, (m, 8)), _full(rng, (n, 8))

    def products(X, Xt, U):
        """(K.X, K^T.Xt, K^T.K.X, dots of K^T.K.X with U[, K.X through the operator and its dots])"""
        k = X.shape[1]
        out = [_mm(api, D, X, m), _mm(api, D, Xt, n, layout=1), _mm(api, D, X, n, ata=True)]
        for normal in ((True, False) if square else (True,)):
            Y = torch.full((n, k), float("nan"), dtype=torch.float64, device="cuda")
            dots = D.op_multi_dot(_poisoned(X), Y, _poisoned(U), normal=normal)
            out += [Y.cpu().numpy(), dots.reshape(1, k)]
        return out

    base = products(X8, Xt8, U8)
    for r in base:
        assert np.isfinite(r).all()                      # Y fully written: no NaN of the pre-fill is left
    assert _same_bits(base[3], base[2])                  # the operator's Y is the product's
    for j in range(8):
        er.assert_dot(base[4][0, j], base[3][:, j], U8[:, j], (shape, j))
        if square:
            assert _same_bits(base[5][:, j], base[0][:, j])
            er.assert_dot(base[6][0, j], base[5][:, j], U8[:, j], (shape, j, "K"))
    for _ in range(4):                                   # five calls
        again = products(X8, Xt8, U8)
        assert all(_same_bits(a, b) for a, b in zip(again, base)), shape
    # other k, other neighbours, another position: column j of the k = 8 block at position `pos` of a block of `k`
    junk = [np.nan, np.inf, -np.inf]
    for k, pos, j in [(2, 0, 0), (2, 1, 1), (2, 0, 5), (2, 1, 7), (4, 0, 2), (4, 1, 3), (4, 2, 4), (4, 3, 6), (8, 7, 0), (8, 0, 7)]:
        X, Xt, U = _full(rng, (n, k)), _full(rng, (m, k)), _full(rng, (n, k))
        for c in range(k):
            if c != pos and c % 2 == 0:
                X[:, c] = junk[c % 3]; Xt[:, c] = junk[(c + 1) % 3]; U[::3, c] = junk[(c + 2) % 3]
        X[:, pos], Xt[:, pos], U[:, pos] = X8[:, j], Xt8[:, j], U8[:, j]
        got = products(X, Xt, U)
        for a, b in zip(got, base):
            assert _same_bits(a[:, pos], b[:, j]), (shape, k, pos, j)
    # a NaN column stays a NaN column and nothing else
    X = X8[:, :4].copy(); X[:, 2] = np.nan
    Y = _mm(api, D, X, n, ata=True)
    assert np.isnan(Y[:, 2]).all() and np.isfinite(Y[:, [0, 1, 3]]).all()
    # (not promised) the single-vector product's bits
    y1 = torch.empty(m, dtype=torch.float64, device="cuda")
    D.matvec(torch.from_numpy(X8[:, 0].copy()).cuda(), y1); api.synchronize()
    with capsys.disabled():
        print(f"\n{shape}: column 0 of K.X has the single-vector product's bits: {_same_bits(y1.cpu().numpy(), base[0][:, 0])}")
    D.destroy()


def test_work_memory_grows_with_k_and_the_single_products_stay(api):
    """The first call at a larger k re-allocates the handle's block and table; results before and after are the same bits, and the
    single-vector products of the same handle are not disturbed."""
    rng = np.random.default_rng(5)
    m, n = 3, 5000
    K = _full(rng, (m, n)); X = _full(rng, (n, 8)); x = _full(rng, n)
    D = api.DenseMatrix.from_array(K)
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    D.ata(torch.from_numpy(x).cuda(), y); api.synchronize()
    first = y.cpu().numpy()
    a2 = _mm(api, D, X[:, :2], n, ata=True)
    a8 = _mm(api, D, X, n, ata=True)
    a2b = _mm(api, D, X[:, :2], n, ata=True)
    assert _same_bits(a2, a2b) and _same_bits(a2, a8[:, :2])
    D.ata(torch.from_numpy(x).cuda(), y); api.synchronize()
    assert _same_bits(first, y.cpu().numpy()) and D.last_kernel.startswith("k_dn_")
    D.destroy()


def test_refusals_leave_y_untouched(api):
    lib = api.L.load()
    rp = np.arange(5, dtype=np.int32); ci = np.arange(4, dtype=np.int32)
    A = api.CsrMatrix.from_csr(rp, ci, np.ones(4))
    D = api.DenseMatrix.from_array(np.eye(4))
    Dc = api.DenseMatrix.from_array(np.eye(4) + 0j)
    R = api.DenseMatrix.from_array(np.ones((6, 4)))
    X = torch.ones((8, 4), dtype=torch.float64, device="cuda")
    Y = torch.full((8, 4), 5.0, dtype=torch.float64, device="cuda")
    out = (C.c_double * 8)()
    x, y = X.data_ptr(), Y.data_ptr()
    entries = {
        "lcg_hip_dense_matmat": lambda h, xx=x, yy=y, layout=0: lib.lcg_hip_dense_matmat(h, 4, xx, yy, layout),
        "lcg_hip_dense_ata_multi": lambda h, xx=x, yy=y: lib.lcg_hip_dense_ata_multi(h, 4, xx, yy),
        "lcg_hip_dense_op_multi_dot": lambda h, xx=x, yy=y, normal=1: lib.lcg_hip_dense_op_multi_dot(h, 4, normal, xx, yy, xx, out),
    }

    def refused(name, why, *a, **kw):
        assert entries[name](*a, **kw) == E_ARG, name
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and why in err, err
        api.synchronize()
        assert torch.all(Y == 5.0), name

    for name in entries:
        refused(name, "not a dense matrix", A.h)            # a CSR handle
        refused(name, "complex", Dc.h)                      # a complex dense handle
        refused(name, "overlap", D.h, yy=x)                 # X and Y the same block
        refused(name, "overlap", D.h, xx=y + 32)            # ... and overlapping in part
    refused("lcg_hip_dense_matmat", "layout", D.h, layout=2)
    refused("lcg_hip_dense_matmat", "layout", D.h, layout=-1)
    refused("lcg_hip_dense_op_multi_dot", "square", R.h, normal=0)
    refused("lcg_hip_dense_op_multi_dot", "normal", D.h, normal=2)
    assert lib.lcg_hip_dense_multi_last_kernel(A.h) == b""
    # and the handles are unharmed
    assert lib.lcg_hip_dense_matmat(D.h, 4, x, y, 0) == 0
    api.synchronize()
    assert torch.all(Y[:4] == 1.0) and torch.all(Y[4:] == 5.0)
    for h in (A, D, Dc, R):
        h.destroy()
