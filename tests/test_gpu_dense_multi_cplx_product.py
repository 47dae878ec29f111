"""-m gpu: the complex128 dense products over k = 2, 4, 8 right-hand sides (liblcg_amd/csrc/dense_multi_cplx.hip): K.X, conj(K).X,
K^T.X, K^H.X and the loops' operator with its carried unconjugated sum, against exact integer sums (bit for bit) and per-row rounding
bounds (tests/exact_ref.py), every complex k-wide kernel family reached; column j's bits the same at k = 2, 4, 8, at another position,
whatever the other columns hold and from call to call; nothing read behind X or U (every block handed to the device here sits in a
larger buffer with NaN directly behind its last row); Y pre-filled with NaN and fully written; the refusals.

Shapes and the branch each is the smallest to reach (dense.hpp: row_plan, col_plan with NP = N packs per row; restated below and
asserted in test_shapes_reach_their_branches).  Row form, four rows per lane group at every k:
  (1, 1) W = 4, one row             (50, 7) W = 8                  (37, 13) W = 16, created with ld > N
  (100, 80) W = 64; forced split: five strips, W = 16              (3, 2500), (1, 2049) the automatic split: nine and eight strips
  (2051, 513) M >= 1024: one strip; forced split: four strips      row counts 1, 3, 37, 50, 2051 are no multiples of 4
Column form: (3, 2500), (1, 2049) one strip of rows; (2500, 3), (100, 80) folded; (2049, 1) one pack met by 256 row groups."""
import ctypes as C

import numpy as np
import pytest

import dense_checker as dc
import dense_multi_cplx_cases as zc
import exact_ref as er

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = [(1, 1), (50, 7), (37, 13), (100, 80), (3, 2500), (1, 2049), (2051, 513), (2500, 3), (2049, 1)]
KS = (2, 4, 8)
E_ARG = -2003
NAN = complex(np.nan, np.nan)
FORMS = [(0, 0), (0, 1), (1, 0), (1, 1)]        # (layout, conjugate): K.X, conj(K).X, K^T.X, K^H.X


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


# ---- dense.hpp's plans, restated ------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def row_plan(M, NP, split, forced):
    S = 1
    if split:
        cap = max(1, NP // 16 if forced else NP // 256)
        S = min(_cdiv(8192, M), cap)
    pps = _cdiv(NP, S)
    return dict(W=min(64, max(4, _pow2ceil(pps))), S=_cdiv(NP, pps), pps=pps)


def row_auto(M, NP):
    split = M < 1024 and row_plan(M, NP, True, False)["S"] >= 2
    return row_plan(M, NP, split, False)


def col_plan(M, NP):
    CW = min(256, _pow2ceil(NP))
    RG = 256 // CW
    CT = _cdiv(NP, CW)
    RS = max(1, min(_cdiv(1024, CT), _cdiv(M, RG * 16)))
    rps = _cdiv(_cdiv(M, RS), RG) * RG
    return dict(CW=CW, RG=RG, CT=CT, RS=_cdiv(M, rps), rps=rps)


def _can_split(m, n):
    return row_plan(m, n, True, True)["S"] >= 2


def test_shapes_reach_their_branches():
    assert row_auto(1, 1) == dict(W=4, S=1, pps=1)
    assert row_auto(50, 7)["W"] == 8 and row_auto(37, 13)["W"] == 16
    assert row_auto(100, 80) == dict(W=64, S=1, pps=80) and row_plan(100, 80, True, True) == dict(W=16, S=5, pps=16)
    assert row_auto(3, 2500)["S"] == 9 and row_auto(1, 2049)["S"] == 8
    assert row_auto(2051, 513)["S"] == 1 and row_plan(2051, 513, True, True)["S"] == 4
    assert not any(_can_split(m, n) for m, n in [(1, 1), (50, 7), (37, 13), (2500, 3), (2049, 1)])
    assert col_plan(3, 2500)["RS"] == 1 and col_plan(1, 2049)["RS"] == 1
    assert col_plan(2500, 3)["RS"] == 3 and col_plan(100, 80)["RS"] == 4
    assert col_plan(2049, 1) == dict(CW=1, RG=256, CT=1, RS=1, rps=2304)
    assert all(m % 4 for m in (1, 3, 37, 50, 2051))


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _poisoned(X):
    """The complex block X (rows, k) on the device, inside a larger buffer with NaN directly behind its last row."""
    rows, k = X.shape
    buf = torch.full((rows * k + 64,), NAN, dtype=torch.complex128, device="cuda")
    buf[:rows * k] = torch.from_numpy(np.ascontiguousarray(X, np.complex128).reshape(-1)).cuda()
    v = buf[:rows * k].view(rows, k)
    assert v.data_ptr() % 16 == 0
    return v


def _mm(api, D, X, out_rows, layout=0, conjugate=0):
    """One k-wide product into a Y pre-filled with NaN; X from a poisoned buffer."""
    Y = torch.full((out_rows, X.shape[1]), NAN, dtype=torch.complex128, device="cuda")
    D.cmatmat(_poisoned(X), Y, layout, conjugate)
    api.synchronize()
    return Y.cpu().numpy()


def _op(api, D, X, U):
    """(Y, dots) of the loops' operator with its carried sum; X and U from poisoned buffers."""
    n, k = X.shape
    Y = torch.full((n, k), NAN, dtype=torch.complex128, device="cuda")
    dots = D.cop_multi_dot(_poisoned(X), Y, _poisoned(U))
    return Y.cpu().numpy(), dots


def _opk(K, layout, conjugate):
    A = K.conj() if conjugate else K
    return np.ascontiguousarray(A.T if layout else A)


def _full(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp2(rng.integers(-6, 7, shape))


def _col(Y, j):
    return np.ascontiguousarray(Y[:, j])


def _same_bits(a, b):
    return np.array_equal(zc.bits(a), zc.bits(b))


def _exact_int_dot(y, u):
    """sum y_i u_i (unconjugated) of integer-valued complex vectors, exactly; raises if a partial sum could round."""
    yr, yi, ur, ui = (np.asarray(t).astype(np.int64) for t in (y.real, y.imag, u.real, u.imag))
    assert np.array_equal(yr, y.real) and np.array_equal(ui, u.imag)
    assert float(np.abs(yr).astype(np.float64) @ np.abs(ur) + np.abs(yi).astype(np.float64) @ np.abs(ui)) < 2.0 ** 52
    assert float(np.abs(yr).astype(np.float64) @ np.abs(ui) + np.abs(yi).astype(np.float64) @ np.abs(ur)) < 2.0 ** 52
    return complex(float(np.sum(yr * ur - yi * ui)), float(np.sum(yr * ui + yi * ur)))


_SEEN = set()


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(37, 13, 11)], ids=lambda s: "x".join(map(str, s)))
def test_exact_sums_on_integers_every_form_and_path(api, shape):
    """Integer data: the device's Y equals exact_ref.exact_int_product on K, conj(K), K^T, K^H bit for bit, whatever the summation
    order, for k = 2, 4, 8, the automatic and the forced row forms."""
    lib = api.L.load()
    m, n = shape[:2]
    rng = np.random.default_rng(m * 7919 + n)
    p = er.int_bits(max(m, n), "c128")
    K = er.int_values(rng, (m, n), p, cplx=True)
    if len(shape) == 3:                             # ld > N
        wide = np.full((m, n + shape[2]), 7.0 + 3.0j); wide[:, :n] = K
        D = api.DenseMatrix.from_array(wide[:, :n])
    else:
        D = api.DenseMatrix.from_array(K)
    assert D.multi_last_kernel == ""
    names = api.DenseMatrix.cmulti_kernel_names()
    csr = {f: dc.dense_as_csr(_opk(K, *f)) for f in FORMS}
    for k in KS:
        X = {0: er.int_values(rng, (n, k), p, cplx=True, zeros=0.02), 1: er.int_values(rng, (m, k), p, cplx=True, zeros=0.02)}
        want = {f: np.stack([er.exact_int_product(*csr[f], _col(X[f[0]], j)) for j in range(k)], axis=1) for f in FORMS}
        for variant in (0, 1, 2):
            if variant == 2 and not _can_split(m, n):
                assert lib.lcg_hip_dense_set_kernel(D.h, 2) == E_ARG          # refused: nothing to split
                continue
            D.set_kernel(variant)
            for conj in (0, 1):
                er.assert_exact(_mm(api, D, X[0], m, 0, conj), want[(0, conj)], (shape, k, "row", conj, variant))
                _SEEN.add(D.multi_last_kernel)
                if variant:
                    assert D.multi_last_kernel == names[variant - 1]
                else:
                    assert D.multi_last_kernel == names[1 if row_auto(m, n)["S"] > 1 else 0]
        D.set_kernel(0)
        for conj in (0, 1):
            er.assert_exact(_mm(api, D, X[1], n, 1, conj), want[(1, conj)], (shape, k, "col", conj))
            _SEEN.add(D.multi_last_kernel)
            assert D.multi_last_kernel == "k_zdnm_col"
    assert D.last_kernel == ""                  # the single-vector name is not touched
    D.destroy()


def test_every_complex_kernel_family_ran(api):
    """The union of lcg_hip_dense_multi_last_kernel over the run above is the complex name list."""
    names = api.DenseMatrix.cmulti_kernel_names()
    assert names == zc.NAMES
    if len(_SEEN) < len(names):                 # (run alone: reach the three families here)
        rng = np.random.default_rng(1)
        D = api.DenseMatrix.from_array(_full(rng, (100, 80)))
        X = _full(rng, (80, 2)); Xt = _full(rng, (100, 2))
        for variant in (1, 2):
            D.set_kernel(variant); _mm(api, D, X, 100); _SEEN.add(D.multi_last_kernel)
        _mm(api, D, Xt, 80, 1); _SEEN.add(D.multi_last_kernel)
        D.destroy()
    assert _SEEN == set(names), (sorted(_SEEN), names)


@pytest.mark.parametrize("shape", SHAPES + [(37, 13, 11)], ids=lambda s: "x".join(map(str, s)))
def test_full_mantissa_rows_within_the_rounding_bound(api, shape):
    """Every column of all four products within exact_ref.assert_rows' per-row bound (bound_c128).  k = 8 (the largest shape: k = 2,
    for the host's time; the columns' bits do not depend on k, which test_columns_do_not_depend_on_k_neighbours_or_the_call pins)."""
    m, n = shape[:2]
    k = 8 if m * n <= 1 << 18 else 2
    rng = np.random.default_rng(m * 131 + n)
    K = _full(rng, (m, n))
    if len(shape) == 3:
        wide = np.full((m, n + shape[2]), NAN); wide[:, :n] = K
        D = api.DenseMatrix.from_array(wide[:, :n])
    else:
        D = api.DenseMatrix.from_array(torch.from_numpy(K).cuda())
    X = {0: _full(rng, (n, k)), 1: _full(rng, (m, k))}
    for (layout, conj) in FORMS:
        csr = dc.dense_as_csr(_opk(K, layout, conj))
        for variant in ((0, 1, 2) if layout == 0 else (0,)):
            if variant == 2 and not _can_split(m, n):
                continue
            D.set_kernel(variant)
            Y = _mm(api, D, X[layout], n if layout else m, layout, conj)
            for j in range(k):
                er.assert_rows(_col(Y, j), *csr, _col(X[layout], j), tag=(shape, k, j, layout, conj, variant))
        D.set_kernel(0)
    D.destroy()


@pytest.mark.parametrize("shape", [(1, 1), (3, 3), (65, 65), (200, 200), (513, 513), (2049, 2049)], ids=lambda s: f"n{s[0]}")
def test_the_carried_sum(api, shape):
    """Integers: Y and the dot bit for bit against the integer product and sum, k = 2, 4, 8 (n = 2049: 33 workgroups of 64 rows, the
    last of one row; the row form split at n = 2049 is not: M >= 1024).  Random data: each component within exact_ref's dot bound of
    the extended-precision sum of the kernel's own Y (2n real products per component), and the same bits from call to call."""
    n = shape[0]
    rng = np.random.default_rng(n + 3)
    Ki = er.int_values(rng, (n, n), 4, cplx=True)
    D = api.DenseMatrix.from_array(Ki)
    csr = dc.dense_as_csr(Ki)
    for k in (KS if n <= 513 else (8,)):
        Xi = er.int_values(rng, (n, k), 4, cplx=True, zeros=0.02); Ui = er.int_values(rng, (n, k), 8, cplx=True, zeros=0.02)
        Y, dots = _op(api, D, Xi, Ui)
        assert _same_bits(Y, _mm(api, D, Xi, n))                                    # Y itself: the plain product's bits
        for j in range(k):
            ye = er.exact_int_product(*csr, _col(Xi, j))
            er.assert_exact(_col(Y, j), ye, (n, k, j))
            want = _exact_int_dot(ye, Ui[:, j])
            assert dots[j].real == want.real and dots[j].imag == want.imag, (n, k, j, dots[j], want)
    D.destroy()
    if n > 513:
        return
    K = _full(rng, (n, n))
    D = api.DenseMatrix.from_array(K)
    for k in KS:
        X = _full(rng, (n, k)); U = _full(rng, (n, k))
        Y, dots = _op(api, D, X, U)
        for j in range(k):
            y, u = _col(Y, j), _col(U, j)
            er.assert_dot(dots[j].real, np.concatenate([y.real, -y.imag]), np.concatenate([u.real, u.imag]), (n, k, j, "re"))
            er.assert_dot(dots[j].imag, np.concatenate([y.real, y.imag]), np.concatenate([u.imag, u.real]), (n, k, j, "im"))
        Y2, dots2 = _op(api, D, X, U)
        assert _same_bits(Y, Y2) and _same_bits(dots, dots2)
    D.destroy()


@pytest.mark.parametrize("shape", [(100, 80), (3, 2500), (2500, 3), (37, 13), (257, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_columns_do_not_depend_on_k_neighbours_or_the_call(api, shape, capsys):
    """Column j of the four products and, for square K, of the operator with dots[j]: the same bits at k = 2, 4 and 8, with the
    neighbours replaced by other data, NaN and +-Inf, at another position of the block, and over three calls.  Whether a column also
    has the bits of the single-vector product is printed, not asserted (it is not promised)."""
    m, n = shape
    rng = np.random.default_rng(m + 17 * n)
    K = _full(rng, (m, n))
    D = api.DenseMatrix.from_array(K)
    square = m == n
    X8, Xt8, U8 = _full(rng, (n, 8)), _full(rng, (m, 8)), _full(rng, (n, 8))

    def products(X, Xt, U):
        out = [_mm(api, D, X, m, 0, 0), _mm(api, D, X, m, 0, 1), _mm(api, D, Xt, n, 1, 0), _mm(api, D, Xt, n, 1, 1)]
        if square:
            Y, dots = _op(api, D, X, U)
            out += [Y, dots.reshape(1, -1)]
        return out

    base = products(X8, Xt8, U8)
    for r in base:
        assert np.isfinite(r).all()            # Y fully written: no NaN of the pre-fill is left
    if square:
        assert _same_bits(base[4], base[0])                      # the operator's Y is the product's
    for _ in range(2):                                           # three calls
        assert all(_same_bits(a, b) for a, b in zip(products(X8, Xt8, U8), base)), shape
    # other k, other neighbours, another position: column j of the k = 8 block at position `pos` of a block of `k`
    junk = [NAN, complex(np.inf, -np.inf), complex(-np.inf, 1.0)]
    for k, pos, j in [(2, 0, 0), (2, 1, 1), (2, 0, 5), (2, 1, 7), (4, 0, 2), (4, 1, 3), (4, 2, 4), (4, 3, 6), (8, 7, 0), (8, 0, 7)]:
        X, Xt, U = _full(rng, (n, k)), _full(rng, (m, k)), _full(rng, (n, k))
        for c in range(k):
            if c != pos and c % 2 == 0:
                X[:, c] = junk[c % 3]; Xt[:, c] = junk[(c + 1) % 3]; U[::3, c] = junk[(c + 2) % 3]
        X[:, pos], Xt[:, pos], U[:, pos] = X8[:, j], Xt8[:, j], U8[:, j]
        for a, b in zip(products(X, Xt, U), base):
            assert _same_bits(a[:, pos], b[:, j]), (shape, k, pos, j)
    # a NaN column stays a NaN column and nothing else
    X = X8[:, :4].copy(); X[:, 2] = NAN
    Y = _mm(api, D, X, m)
    assert np.isnan(Y[:, 2].real).all() and np.isfinite(Y[:, [0, 1, 3]]).all()
    # the forced forms are their own bits, the same at every k
    if _can_split(m, n):
        for variant in (1, 2):
            D.set_kernel(variant)
            y8 = _mm(api, D, X8, m)
            assert _same_bits(_mm(api, D, X8[:, 2:4].copy(), m), y8[:, 2:4]) and _same_bits(_mm(api, D, X8[:, 4:8].copy(), m), y8[:, 4:8])
        D.set_kernel(0)
    # (not promised) the single-vector product's bits
    y1 = torch.empty(m, dtype=torch.complex128, device="cuda")
    D.matvec(torch.from_numpy(X8[:, 0].copy()).cuda(), y1); api.synchronize()
    with capsys.disabled():
        print(f"\n{shape}: column 0 of K.X has the single-vector product's bits: {_same_bits(y1.cpu().numpy(), base[0][:, 0])}")
    D.destroy()


def test_work_memory_grows_with_k_and_the_single_products_stay(api):
    """The first call at a larger k re-allocates the handle's table (under the split row form and the folded column form); results
    before and after are the same bits, and the single-vector products of the same handle are not disturbed."""
    rng = np.random.default_rng(5)
    for (m, n, layout) in [(3, 2500, 0), (2500, 3, 1)]:
        K = _full(rng, (m, n))
        rows_in, rows_out = (m, n) if layout else (n, m)
        X = _full(rng, (rows_in, 8)); x = _full(rng, rows_in)
        D = api.DenseMatrix.from_array(K)
        y = torch.empty(rows_out, dtype=torch.complex128, device="cuda")
        D.matvec(torch.from_numpy(x).cuda(), y, layout); api.synchronize()
        first = y.cpu().numpy()
        a2 = _mm(api, D, X[:, :2].copy(), rows_out, layout)
        a8 = _mm(api, D, X, rows_out, layout)
        a2b = _mm(api, D, X[:, :2].copy(), rows_out, layout)
        assert _same_bits(a2, a2b) and _same_bits(a2, a8[:, :2])
        D.matvec(torch.from_numpy(x).cuda(), y, layout); api.synchronize()
        assert _same_bits(first, y.cpu().numpy()) and D.last_kernel.startswith("k_dn_")
        D.destroy()


def test_refusals_leave_y_untouched(api):
    lib = api.L.load()
    rp = np.arange(5, dtype=np.int32); ci = np.arange(4, dtype=np.int32)
    A = api.CsrMatrix.from_csr(rp, ci, np.ones(4) + 0j)
    D = api.DenseMatrix.from_array(np.eye(4) + 0j)
    Dr = api.DenseMatrix.from_array(np.eye(4))
    R = api.DenseMatrix.from_array(np.ones((6, 4)) + 0j)
    sentinel = complex(5.0, -2.0)
    X = torch.ones((8, 4), dtype=torch.complex128, device="cuda")
    Y = torch.full((8, 4), sentinel, dtype=torch.complex128, device="cuda")
    out = (C.c_double * 8)()
    x, y = X.data_ptr(), Y.data_ptr()
    entries = {
        "clcg_hip_dense_matmat": lambda h, xx=x, yy=y, layout=0, conj=0: lib.clcg_hip_dense_matmat(h, 4, xx, yy, layout, conj),
        "clcg_hip_dense_op_multi_dot": lambda h, xx=x, yy=y: lib.clcg_hip_dense_op_multi_dot(h, 4, xx, yy, xx, out),
    }

    def refused(name, why, *a, **kw):
        assert entries[name](*a, **kw) == E_ARG, name
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and why in err, err
        api.synchronize()
        assert bool((Y == sentinel).all()), name

    for name in entries:
        refused(name, "not a dense matrix", A.h)            # a CSR handle
        refused(name, "real", Dr.h)                         # a real dense handle
        refused(name, "overlap", D.h, yy=x)                 # X and Y the same block
        refused(name, "overlap", D.h, xx=y + 64)            # ... and overlapping in part
    for layout, conj in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        refused("clcg_hip_dense_matmat", "layout", D.h, layout=layout, conj=conj)
    refused("clcg_hip_dense_op_multi_dot", "square", R.h)
    # bad k, a null or misaligned block: before the handle is looked at
    assert lib.clcg_hip_dense_matmat(D.h, 3, x, y, 0, 0) == E_ARG and "k must be" in lib.lcg_hip_last_error().decode()
    assert lib.clcg_hip_dense_matmat(D.h, 4, x + 8, y, 0, 0) == E_ARG and "aligned" in lib.lcg_hip_last_error().decode()
    assert lib.clcg_hip_dense_matmat(D.h, 4, None, y, 0, 0) == E_ARG and "null" in lib.lcg_hip_last_error().decode()
    api.synchronize()
    assert bool((Y == sentinel).all())
    # the real k-wide entries keep refusing the complex handle
    Xf = torch.ones((8, 4), dtype=torch.float64, device="cuda"); Yf = torch.full((8, 4), 5.0, dtype=torch.float64, device="cuda")
    assert lib.lcg_hip_dense_matmat(D.h, 4, Xf.data_ptr(), Yf.data_ptr(), 0) == E_ARG and "complex" in lib.lcg_hip_last_error().decode()
    assert lib.lcg_hip_dense_multi_last_kernel(A.h) == b""
    # and the handles are unharmed
    assert lib.clcg_hip_dense_matmat(D.h, 4, x, y, 0, 0) == 0
    api.synchronize()
    assert bool((Y[:4] == 1.0).all()) and bool((Y[4:] == sentinel).all())
    for h in (A, D, Dr, R):
        h.destroy()
