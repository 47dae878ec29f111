"""-m gpu: the complex64 dense products (liblcg_amd/csrc/dense_c64.hip): K.x, conj(K).x, K^T.x, K^H.x, and K.X / conj(K).X over k = 2,
4, 8 right-hand sides on the fp32 matrix instruction, with the loops' carried unconjugated sum -- against exact integer sums (bit for
bit) and per-row rounding bounds (tests/exact_ref.py: int_bits / bound_c64 / dot_bound), every kernel name asserted per shape; column
j's bits the same at k = 2, 4, 8, at another position, whatever the other columns hold and from call to call; nothing read behind x,
X or U (every vector handed to the device here sits in a larger buffer with NaN directly behind its last entry); Y pre-filled with NaN
and fully written; the refusals, in both directions.

Shapes: tests/dense_c64_cases.py's SHAPES and the branch each is the smallest to reach (asserted in tests/test_dense_c64_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import dense_c64_cases as X
import dense_checker as dc
import exact_ref as er

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KS = (2, 4, 8)
E_ARG = -2003
NAN = complex(np.nan, np.nan)
FORMS = [(0, 0), (0, 1), (1, 0), (1, 1)]        # (layout, conjugate): K.x, conj(K).x, K^T.x, K^H.x
AUTO, ROW, ROW_SPLIT, COL = 0, 1, 2, 3


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _poisoned(V):
    """The complex64 array V (a vector or a (rows, k) block) on the device, inside a larger buffer with NaN directly behind it."""
    V = np.ascontiguousarray(V, np.complex64)
    buf = torch.full((V.size + 64,), NAN, dtype=torch.complex64, device="cuda")
    buf[:V.size] = torch.from_numpy(V.reshape(-1)).cuda()
    v = buf[:V.size].view(*V.shape)
    assert v.data_ptr() % 16 == 0
    return v


def _mv(api, D, x, out_rows, layout=0, conjugate=0):
    y = torch.full((out_rows,), NAN, dtype=torch.complex64, device="cuda")
    D.matvec_c64(_poisoned(x), y, layout, conjugate)
    api.synchronize()
    return y.cpu().numpy()


def _mm(api, D, Xb, out_rows, conjugate=0):
    Y = torch.full((out_rows, Xb.shape[1]), NAN, dtype=torch.complex64, device="cuda")
    D.cmatmat_c64(_poisoned(Xb), Y, conjugate)
    api.synchronize()
    return Y.cpu().numpy()


def _op(api, D, Xb, U):
    n, k = Xb.shape
    Y = torch.full((n, k), NAN, dtype=torch.complex64, device="cuda")
    dots = D.cop_multi_dot_c64(_poisoned(Xb), Y, _poisoned(U))
    return Y.cpu().numpy(), dots


def _opk(K, layout, conjugate):
    A = K.conj() if conjugate else K
    return np.ascontiguousarray(A.T if layout else A)


def _full(rng, shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp2(rng.integers(-6, 7, shape))).astype(np.complex64)


def _ints(rng, shape, p, zeros=0.1):
    return er.int_values(rng, shape, p, cplx=True, zeros=zeros).astype(np.complex64)


def _col(Y, j):
    return np.ascontiguousarray(Y[:, j])


def _same_bits(a, b):
    return np.array_equal(X.bits(a), X.bits(b))


def _exact_int_dot(y, u):
    yr, yi, ur, ui = (np.asarray(t).astype(np.int64) for t in (y.real, y.imag, u.real, u.imag))
    assert np.array_equal(yr, y.real) and np.array_equal(ui, u.imag)
    assert float(np.abs(yr).astype(np.float64) @ np.abs(ur) + np.abs(yi).astype(np.float64) @ np.abs(ui)) < 2.0 ** 52
    assert float(np.abs(yr).astype(np.float64) @ np.abs(ui) + np.abs(yi).astype(np.float64) @ np.abs(ur)) < 2.0 ** 52
    return complex(float(np.sum(yr * ur - yi * ui)), float(np.sum(yr * ui + yi * ur)))


def _row_name(m, n, variant):
    split = variant == ROW_SPLIT or (variant != ROW and X.row_auto(m, X.packs(n))["S"] > 1)
    return split


def _handles(api, K, extra_ld=0):
    """The same matrix as a host-made handle (numpy, optionally a view with ld > N) and a device-made one (torch)."""
    m, n = K.shape
    if extra_ld:
        wide = np.full((m, n + extra_ld), 7 + 3j, np.complex64); wide[:, :n] = K
        host = api.DenseMatrix.from_array_c64(wide[:, :n])
    else:
        host = api.DenseMatrix.from_array_c64(K)
    wide_d = torch.full((m, n + 3), NAN, dtype=torch.complex64, device="cuda")
    wide_d[:, :n] = torch.from_numpy(K).cuda()
    dev = api.DenseMatrix.from_array_c64(wide_d[:, :n])         # a device view with ld = N + 3
    return host, dev


_SEEN = set()


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", X.SHAPES + [(17, 33, 11)], ids=lambda s: "x".join(map(str, s)))
def test_exact_sums_on_integers_every_form_and_path(api, shape):
    """Integer data within exact_ref.int_bits(L, "c64"): every partial sum of a row of L terms is exact in fp32 whatever the order, so
    the device's results equal exact_ref.exact_int_product on K, conj(K), K^T, K^H bit for bit -- the four single-vector forms, both
    k-wide forms at k = 2, 4, 8, the automatic and the forced variants, host-made and device-made handles."""
    lib = api.L.load()
    m, n = shape[:2]
    rng = np.random.default_rng(m * 7919 + n)
    p = er.int_bits(max(m, n), "c64")
    K = _ints(rng, (m, n), p)
    host, dev = _handles(api, K, shape[2] if len(shape) == 3 else 0)
    names = api.DenseMatrix.kernel_names_c64()
    csr = {f: dc.dense_as_csr(_opk(K.astype(np.complex128), *f)) for f in FORMS}
    x = {0: _ints(rng, n, p, 0.02), 1: _ints(rng, m, p, 0.02)}
    want1 = {f: er.exact_int_product(*csr[f], x[f[0]].astype(np.complex128)) for f in FORMS}
    for D in (host, dev):
        assert D.last_kernel == "" and D.multi_last_kernel == "" and (D.m, D.n) == (m, n)
        assert lib.lcg_hip_dense_rows(D.h) == m and lib.lcg_hip_dense_cols(D.h) == n
        for variant in (AUTO, ROW, ROW_SPLIT, COL):
            if variant == ROW_SPLIT and not X.can_split(m, n):
                assert lib.lcg_hip_dense_set_kernel(D.h, ROW_SPLIT) == E_ARG          # refused: nothing to split
                continue
            D.set_kernel(variant)
            split = _row_name(m, n, variant)
            for (layout, conj) in FORMS:
                y = _mv(api, D, x[layout], n if layout else m, layout, conj)
                er.assert_exact(y, want1[(layout, conj)], (shape, "single", layout, conj, variant))
                assert D.last_kernel == (names[2] if layout else names[1 if split else 0]), (shape, variant, D.last_kernel)
                _SEEN.add(D.last_kernel)
            for k in KS:
                Xb = _ints(rng, (n, k), p, 0.02)
                for conj in (0, 1):
                    Y = _mm(api, D, Xb, m, conj)
                    for j in range(k):
                        er.assert_exact(_col(Y, j), er.exact_int_product(*csr[(0, conj)], _col(Xb, j).astype(np.complex128)),
                                        (shape, "k-wide", k, j, conj, variant))
                    assert D.multi_last_kernel == names[4 if split else 3], (shape, variant, D.multi_last_kernel)
                    _SEEN.add(D.multi_last_kernel)
        for variant in (4, 5, 6, -1, 7):
            assert lib.lcg_hip_dense_set_kernel(D.h, variant) == E_ARG                 # no K^T.K forms here
        D.destroy()


def test_every_kernel_family_ran(api):
    """The union of the reported names over the run above is the complex64 name list."""
    names = api.DenseMatrix.kernel_names_c64()
    assert names == X.NAMES
    if len(_SEEN) < len(names):                 # (run alone: reach the five families here)
        rng = np.random.default_rng(1)
        D = api.DenseMatrix.from_array_c64(_full(rng, (200, 64)))
        x, xt, Xb = _full(rng, 64), _full(rng, 200), _full(rng, (64, 2))
        for variant in (ROW, ROW_SPLIT):
            D.set_kernel(variant)
            _mv(api, D, x, 200); _SEEN.add(D.last_kernel)
            _mm(api, D, Xb, 200); _SEEN.add(D.multi_last_kernel)
        _mv(api, D, xt, 64, 1); _SEEN.add(D.last_kernel)
        D.destroy()
    assert _SEEN == set(names), (sorted(_SEEN), names)


@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_full_mantissa_rows_within_the_rounding_bound(api, shape, capsys):
    """Every output within exact_ref.bound_c64 = 3 (L + 5) 2^-24 (|K||x|)_i, L the terms of that output (N for the row forms, M for
    the column forms), against exact_ref.hp_product on the complex64 inputs.  tests/test_gpu_c64.py's derivation: each real component
    is a chain of two fp32 fused multiply-adds per term plus the adds that join lanes, wavefronts and slots, fewer roundings on any
    term's way to the root than the 2 L + 10 the bound allows (a lane or a wavefront holds a fraction of the row).  The worst ratio
    is printed."""
    m, n = shape
    rng = np.random.default_rng(m * 131 + n)
    K = _full(rng, (m, n))
    D = api.DenseMatrix.from_array_c64(torch.from_numpy(K).cuda())
    x = {0: _full(rng, n), 1: _full(rng, m)}
    k = 8 if m * n <= 1 << 16 else 2
    Xb = _full(rng, (n, k))
    worst = 0.0
    for variant in (AUTO, ROW, ROW_SPLIT):
        if variant == ROW_SPLIT and not X.can_split(m, n):
            continue
        D.set_kernel(variant)
        for (layout, conj) in FORMS:
            if layout and variant:
                continue
            csr = dc.dense_as_csr(_opk(K.astype(np.complex128), layout, conj))
            L = m if layout else n
            ref = er.hp_product(*csr, x[layout].astype(np.complex128))
            err = er.row_errors(_mv(api, D, x[layout], n if layout else m, layout, conj).astype(np.complex128), ref)
            bound = er.bound_c64(np.full(len(err), L), ref[2])
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (shape, "single", layout, conj, variant, float(np.max(err / bound)))
            if layout == 0:
                Y = _mm(api, D, Xb, m, conj)
                for j in range(k):
                    ref = er.hp_product(*csr, _col(Xb, j).astype(np.complex128))
                    err = er.row_errors(_col(Y, j).astype(np.complex128), ref)
                    bound = er.bound_c64(np.full(len(err), L), ref[2])
                    worst = max(worst, float(np.max(err / bound)))
                    assert np.all(err <= bound), (shape, "k-wide", k, j, conj, variant, float(np.max(err / bound)))
    with capsys.disabled():
        print(f"\n{shape}: worst error / bound {worst:.4f}")
    D.destroy()


@pytest.mark.parametrize("n", [1, 3, 65, 200, 513, 2049], ids=lambda n: f"n{n}")
def test_the_carried_sum(api, n):
    """Integers: Y and the dot bit for bit against the integer product and sum, k = 2, 4, 8 (n = 2049: 33 workgroups of 64 rows, the
    last of one row).  Random data: each component within exact_ref.dot_bound of the extended-precision sum of the kernel's own Y (2n
    real products per component, exact in fp64, summed in fp64), and the same bits from call to call."""
    rng = np.random.default_rng(n + 3)
    p = min(4, er.int_bits(n, "c64"))
    Ki = _ints(rng, (n, n), p)
    D = api.DenseMatrix.from_array_c64(Ki)
    csr = dc.dense_as_csr(Ki.astype(np.complex128))
    for k in (KS if n <= 513 else (8,)):
        Xi = _ints(rng, (n, k), p, 0.02); Ui = _ints(rng, (n, k), 8, 0.02)
        Y, dots = _op(api, D, Xi, Ui)
        assert _same_bits(Y, _mm(api, D, Xi, n))                                    # Y itself: the plain product's bits
        for j in range(k):
            ye = er.exact_int_product(*csr, _col(Xi, j).astype(np.complex128))
            er.assert_exact(_col(Y, j), ye, (n, k, j))
            want = _exact_int_dot(ye, Ui[:, j].astype(np.complex128))
            assert dots[j].real == want.real and dots[j].imag == want.imag, (n, k, j, dots[j], want)
    D.destroy()
    if n > 513:
        return
    K = _full(rng, (n, n))
    D = api.DenseMatrix.from_array_c64(K)
    for k in KS:
        Xb = _full(rng, (n, k)); U = _full(rng, (n, k))
        Y, dots = _op(api, D, Xb, U)
        for j in range(k):
            y, u = _col(Y, j).astype(np.complex128), _col(U, j).astype(np.complex128)
            er.assert_dot(dots[j].real, np.concatenate([y.real, -y.imag]), np.concatenate([u.real, u.imag]), (n, k, j, "re"))
            er.assert_dot(dots[j].imag, np.concatenate([y.real, y.imag]), np.concatenate([u.imag, u.real]), (n, k, j, "im"))
        Y2, dots2 = _op(api, D, Xb, U)
        assert _same_bits(Y, Y2) and _same_bits(dots, dots2)
    D.destroy()


@pytest.mark.parametrize("shape", [(200, 64), (33, 2050), (17, 33), (65, 513), (257, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_columns_do_not_depend_on_k_neighbours_or_the_call(api, shape, capsys):
    """Column j of K.X and conj(K).X and, for square K, of the operator with dots[j]: the same bits at k = 2, 4 and 8, with the
    neighbours replaced by other data, zeros, NaN and +-Inf, at another position of the block, and over three calls.  Whether a column
    also has the bits of the single-vector product is printed, not asserted (it is not promised)."""
    m, n = shape
    rng = np.random.default_rng(m + 17 * n)
    K = _full(rng, (m, n))
    D = api.DenseMatrix.from_array_c64(K)
    square = m == n
    X8, U8 = _full(rng, (n, 8)), _full(rng, (n, 8))

    def products(Xb, U):
        out = [_mm(api, D, Xb, m, 0), _mm(api, D, Xb, m, 1)]
        if square:
            Y, dots = _op(api, D, Xb, U)
            out += [Y, dots.reshape(1, -1)]
        return out

    base = products(X8, U8)
    for r in base:
        assert np.isfinite(r).all()            # Y fully written: no NaN of the pre-fill is left
    if square:
        assert _same_bits(base[2], base[0])                      # the operator's Y is the product's
    for _ in range(2):                                           # three calls
        assert all(_same_bits(a, b) for a, b in zip(products(X8, U8), base)), shape
    junk = [NAN, complex(np.inf, -np.inf), complex(-np.inf, 1.0), 0j]
    for k, pos, j in [(2, 0, 0), (2, 1, 1), (2, 0, 5), (2, 1, 7), (4, 0, 2), (4, 1, 3), (4, 2, 4), (4, 3, 6), (8, 7, 0), (8, 0, 7)]:
        Xb, U = _full(rng, (n, k)), _full(rng, (n, k))
        for c in range(k):
            if c != pos and c % 2 == 0:
                Xb[:, c] = junk[c % 4]; U[::3, c] = junk[(c + 2) % 4]
        if pos != k - 1:
            Xb[:, k - 1] = junk[(k + pos) % 4]
        Xb[:, pos], U[:, pos] = X8[:, j], U8[:, j]
        for a, b in zip(products(Xb, U), base):
            assert _same_bits(a[:, pos], b[:, j]), (shape, k, pos, j)
    # a NaN column stays a NaN column and nothing else
    Xb = X8[:, :4].copy(); Xb[:, 2] = NAN
    Y = _mm(api, D, Xb, m)
    assert np.isnan(Y[:, 2].real).all() and np.isfinite(Y[:, [0, 1, 3]]).all()
    # the forced forms are their own bits, the same at every k
    if X.can_split(m, n):
        for variant in (ROW, ROW_SPLIT):
            D.set_kernel(variant)
            y8 = _mm(api, D, X8, m)
            assert _same_bits(_mm(api, D, X8[:, 2:4].copy(), m), y8[:, 2:4]) and _same_bits(_mm(api, D, X8[:, 4:8].copy(), m), y8[:, 4:8])
        D.set_kernel(AUTO)
    # (not promised) the single-vector product's bits
    y1 = _mv(api, D, X8[:, 0].copy(), m)
    with capsys.disabled():
        print(f"\n{shape}: column 0 of K.X has the single-vector product's bits: {_same_bits(y1, base[0][:, 0])}")
    D.destroy()


def test_single_vector_products_repeat_their_bits(api):
    rng = np.random.default_rng(11)
    for (m, n) in [(33, 2050), (4100, 7), (65, 513)]:
        D = api.DenseMatrix.from_array_c64(_full(rng, (m, n)))
        x, xt = _full(rng, n), _full(rng, m)
        for (layout, conj) in FORMS:
            a = _mv(api, D, xt if layout else x, n if layout else m, layout, conj)
            assert np.isfinite(a).all()
            for _ in range(2):
                assert _same_bits(a, _mv(api, D, xt if layout else x, n if layout else m, layout, conj))
        D.destroy()


def test_refusals_leave_the_outputs_untouched(api):
    """The complex64 entries refuse every other kind of handle, the entries of the other kinds refuse the complex64 handle, each with
    LCG_HIP_E_ARG, "complex64" in the text and nothing written."""
    lib = api.L.load()
    rp = np.arange(5, dtype=np.int32); ci = np.arange(4, dtype=np.int32)
    A = api.CsrMatrix.from_csr(rp, ci, np.ones(4) + 0j)
    A64 = api.CsrMatrix.from_csr_c64(rp, ci, np.ones(4, np.complex64))
    Dz = api.DenseMatrix.from_array(np.eye(4) + 0j)
    Dr = api.DenseMatrix.from_array(np.eye(4))
    D = api.DenseMatrix.from_array_c64(np.eye(4, dtype=np.complex64))
    R = api.DenseMatrix.from_array_c64(np.ones((6, 4), np.complex64))
    assert D.is_c64 and not Dz.is_c64
    sentinel = complex(5.0, -2.0)
    Xd = torch.ones((8, 4), dtype=torch.complex64, device="cuda")
    Yd = torch.full((8, 4), sentinel, dtype=torch.complex64, device="cuda")
    out = (C.c_double * 8)(*([7.0] * 8))
    ret = (C.c_int * 4)(*([99] * 4))
    p = api.clcg_default_parameters()
    x, y = Xd.data_ptr(), Yd.data_ptr()
    new = {
        "clcg_hip_dense_matvec_c64": lambda h, xx=x, yy=y: lib.clcg_hip_dense_matvec_c64(h, xx, yy, 0, 0),
        "lcg_hip_dense_build_jacobi_c64": lambda h, xx=x, yy=y: lib.lcg_hip_dense_build_jacobi_c64(h, yy),
        "clcg_hip_dense_matmat_c64": lambda h, xx=x, yy=y: lib.clcg_hip_dense_matmat_c64(h, 4, xx, yy, 0),
        "clcg_hip_dense_op_multi_dot_c64": lambda h, xx=x, yy=y: lib.clcg_hip_dense_op_multi_dot_c64(h, 4, xx, yy, xx, out),
        "clcg_hip_dense_lbicg_sym_multi_c64": lambda h, xx=x, yy=y: lib.clcg_hip_dense_lbicg_sym_multi_c64(h, 4, yy, xx, C.byref(p), ret, None, None, 1),
        "clcg_hip_dense_lpcg_multi_c64": lambda h, xx=x, yy=y: lib.clcg_hip_dense_lpcg_multi_c64(h, 4, yy, xx, C.byref(p), ret, None, None, 1),
    }

    def untouched():
        api.synchronize()
        assert bool((Yd == sentinel).all()) and list(out) == [7.0] * 8 and list(ret) == [99] * 4

    for name, call in new.items():
        for h in (A.h, A64.h, Dz.h, Dr.h):
            assert call(h) == E_ARG, name
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and "complex64" in err, err
            untouched()
    for name in ("clcg_hip_dense_matmat_c64", "clcg_hip_dense_op_multi_dot_c64"):
        assert new[name](D.h, yy=x) == E_ARG and "overlap" in lib.lcg_hip_last_error().decode()
        assert new[name](D.h, xx=y + 64) == E_ARG and "overlap" in lib.lcg_hip_last_error().decode()
    for name in ("clcg_hip_dense_op_multi_dot_c64", "lcg_hip_dense_build_jacobi_c64", "clcg_hip_dense_lbicg_sym_multi_c64",
                 "clcg_hip_dense_lpcg_multi_c64"):
        assert new[name](R.h) == E_ARG and "square" in lib.lcg_hip_last_error().decode(), name
    assert lib.clcg_hip_dense_matmat_c64(D.h, 4, x, y, 2) == E_ARG and "conjugate" in lib.lcg_hip_last_error().decode()
    untouched()
    # the entries of the real and complex128 dense handles, and of CSR handles, refuse the complex64 dense handle
    Xf = torch.ones((8, 4), dtype=torch.float64, device="cuda"); Yf = torch.full((8, 4), 5.0, dtype=torch.float64, device="cuda")
    xf, yf = Xf.data_ptr(), Yf.data_ptr()
    lp = api.lcg_default_parameters()
    old = {
        "lcg_hip_dense_matvec": lambda: lib.lcg_hip_dense_matvec(D.h, xf, yf, 0),
        "clcg_hip_dense_matvec": lambda: lib.clcg_hip_dense_matvec(D.h, xf, yf, 0, 0),
        "lcg_hip_dense_ata": lambda: lib.lcg_hip_dense_ata(D.h, xf, yf),
        "lcg_hip_dense_build_jacobi": lambda: lib.lcg_hip_dense_build_jacobi(D.h, 0, yf),
        "lcg_hip_dense_matmat": lambda: lib.lcg_hip_dense_matmat(D.h, 4, xf, yf, 0),
        "lcg_hip_dense_ata_multi": lambda: lib.lcg_hip_dense_ata_multi(D.h, 4, xf, yf),
        "lcg_hip_dense_op_multi_dot": lambda: lib.lcg_hip_dense_op_multi_dot(D.h, 4, 0, xf, yf, xf, out),
        "clcg_hip_dense_matmat": lambda: lib.clcg_hip_dense_matmat(D.h, 2, xf, yf, 0, 0),
        "clcg_hip_dense_op_multi_dot": lambda: lib.clcg_hip_dense_op_multi_dot(D.h, 2, xf, yf, xf, out),
        "lcg_hip_dense_lcg_multi": lambda: lib.lcg_hip_dense_lcg_multi(D.h, 4, 0, yf, xf, C.byref(lp), ret, None, None, 1),
        "lcg_hip_dense_lpcg_multi": lambda: lib.lcg_hip_dense_lpcg_multi(D.h, 4, 0, yf, xf, C.byref(lp), ret, None, None, 1),
        "clcg_hip_dense_lbicg_sym_multi": lambda: lib.clcg_hip_dense_lbicg_sym_multi(D.h, 2, yf, xf, C.byref(p), ret, None, None, 1),
        "clcg_hip_dense_lpcg_multi": lambda: lib.clcg_hip_dense_lpcg_multi(D.h, 2, yf, xf, C.byref(p), ret, None, None, 1),
        "lcg_hip_dense_solver_constrained_multi": lambda: lib.lcg_hip_dense_solver_constrained_multi(D.h, 4, 0, 0, yf, xf, xf, xf, C.byref(lp), ret, None, None, None, 1),
    }
    for name, call in old.items():
        assert call() == E_ARG, name
        err = lib.lcg_hip_last_error().decode()
        assert name + ":" in err and "complex64" in err, err
        api.synchronize()
        assert bool((Yf == 5.0).all()) and list(out) == [7.0] * 8 and list(ret) == [99] * 4, name
    assert lib.lcg_hip_spmv_c64(D.h, x, y, 0, 0) == E_ARG and "dense" in lib.lcg_hip_last_error().decode()       # a CSR entry
    assert lib.clcg_hip_spmm_c64(D.h, 4, x, y) == E_ARG
    untouched()
    # and the handles are unharmed
    assert lib.clcg_hip_dense_matmat_c64(D.h, 4, x, y, 0) == 0
    api.synchronize()
    assert bool((Yd[:4] == 1.0).all()) and bool((Yd[4:] == sentinel).all())
    for h in (A, A64, Dz, Dr, D, R):
        h.destroy()
