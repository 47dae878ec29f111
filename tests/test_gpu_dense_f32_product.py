"""-m gpu: a real dense matrix stored in fp32 (lcg_hip_dense_create_f32, include/lcg_hip_staging_dense_f32.h) IS the fp64 handle of the
widened matrix: every product, under the automatic choice and under every variant lcg_hip_dense_set_kernel accepts for the shape, has
the twin's bits -- equality of the uint64 views, not closeness -- and reports the twin's kernel names.  The pair is anchored on
tests/exact_ref.py's exact sums, so twin and handle cannot be wrong together.  Special values (fp32 subnormals, signed zeros, FLT_MAX,
Inf, NaN) come through as the twin's; the refusals, the create checks, either memory source and the caller's stream.

Shapes: tests/dense_f32_cases.py says which branch each is the smallest to reach."""
import ctypes as C

import numpy as np
import pytest

import dense_checker as dc
import dense_f32_cases as X
import exact_ref as er

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E_ARG, KS = X.E_ARG, X.KS
NAN = float("nan")


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib(api):
    return api.L.load()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cases' arrays are read-only)


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def matvec(api, H, x, out_len, layout=0):
    y = nans(out_len)
    H.matvec(dev(x), y, layout)
    api.synchronize()
    return y.cpu().numpy()


def ata(api, H, x):
    y = nans(H.n)
    H.ata(dev(x), y)
    api.synchronize()
    return y.cpu().numpy()


def jacobi(api, lib, H, normal):
    """(diag_out, the reciprocals as lcg_hip_dense_jacobi_mx applies them to ones)."""
    d, z = nans(H.n), nans(H.n)
    H.build_jacobi(bool(normal), d)
    lib.lcg_hip_dense_jacobi_mx(H.h, torch.ones(H.n, dtype=torch.float64, device="cuda").data_ptr(), z.data_ptr(), H.n)
    api.synchronize()
    return d.cpu().numpy(), z.cpu().numpy()


def matmat(api, H, Xb, out_rows, layout=0):
    Y = nans(out_rows, Xb.shape[1])
    H.matmat(dev(Xb), Y, layout)
    api.synchronize()
    return Y.cpu().numpy()


def ata_multi(api, H, Xb):
    Y = nans(H.n, Xb.shape[1])
    H.ata_multi(dev(Xb), Y)
    api.synchronize()
    return Y.cpu().numpy()


def op_dot(api, H, Xb, U, normal):
    Y = nans(H.n, Xb.shape[1])
    dots = H.op_multi_dot(dev(Xb), Y, dev(U), normal=bool(normal))
    api.synchronize()
    return Y.cpu().numpy(), dots


def everything(api, lib, H, m, n, seed):
    """Every product of one handle under its current variant, as a dict of name -> array, plus the kernel names reported."""
    out, names = {}, {}
    x, xt = X.vector(seed, n), X.vector(seed + 1, m)
    out["K.x"] = matvec(api, H, x, m); names["K.x"] = H.last_kernel
    out["K^T.x"] = matvec(api, H, xt, n, 1); names["K^T.x"] = H.last_kernel
    out["ata"] = ata(api, H, x); names["ata"] = H.last_kernel
    out["jacobi1 diag"], out["jacobi1 recip"] = jacobi(api, lib, H, 1)
    if m == n:
        out["jacobi0 diag"], out["jacobi0 recip"] = jacobi(api, lib, H, 0)
    for k in KS:
        Xb, Xt, U = X.vector(seed + 10 * k, n, k), X.vector(seed + 10 * k + 1, m, k), X.vector(seed + 10 * k + 2, n, k)
        out[f"K.X k={k}"] = matmat(api, H, Xb, m); names[f"K.X k={k}"] = H.multi_last_kernel
        out[f"K^T.X k={k}"] = matmat(api, H, Xt, n, 1); names[f"K^T.X k={k}"] = H.multi_last_kernel
        out[f"ata_multi k={k}"] = ata_multi(api, H, Xb); names[f"ata_multi k={k}"] = H.multi_last_kernel
        out[f"op1 Y k={k}"], out[f"op1 dots k={k}"] = op_dot(api, H, Xb, U, 1); names[f"op1 k={k}"] = H.multi_last_kernel
        if m == n:
            out[f"op0 Y k={k}"], out[f"op0 dots k={k}"] = op_dot(api, H, Xb, U, 0); names[f"op0 k={k}"] = H.multi_last_kernel
    return out, names


@pytest.mark.parametrize("shape", X.SHAPES + [X.PADDED], ids=lambda s: "x".join(map(str, s)))
def test_same_bits_as_the_fp64_handle_of_the_widened_matrix(api, lib, shape):
    m, n = shape[:2]
    ld = shape[2] if len(shape) > 2 else None
    K = X.matrix(m, n)
    F, D = X.pair(api, K, ld)
    assert (F.value_bytes, D.value_bytes) == (4, 8)
    assert F.last_kernel == "" and F.multi_last_kernel == ""
    ran = []
    for variant in range(7):
        rf, rd = lib.lcg_hip_dense_set_kernel(F.h, variant), lib.lcg_hip_dense_set_kernel(D.h, variant)
        want = 0 if variant in X.accepted(m, n) else E_ARG
        assert rf == rd == want, (shape, variant, rf, rd, want)
        if want:
            continue
        ran.append(variant)
        of, nf = everything(api, lib, F, m, n, 100 * variant + m + n)
        od, nd = everything(api, lib, D, m, n, 100 * variant + m + n)
        assert nf == nd, (shape, variant, nf, nd)
        for key in od:
            assert not np.isnan(od[key]).any(), (shape, variant, key, "the twin left NaN: an output was not written")
            assert X.same_bits(of[key], od[key]), (shape, variant, key, int((X.bits(of[key]) != X.bits(od[key])).sum()), "values differ")
        if variant == X.AUTO:       # two calls give the same bits
            again, _ = everything(api, lib, F, m, n, m + n)
            assert all(X.same_bits(again[key], of[key]) for key in of), (shape, "second call")
    assert ran == X.accepted(m, n)
    F.destroy(); D.destroy()


def test_a_columns_bits_do_not_depend_on_k_or_on_its_position(api):
    """Inherited from the fp64 kernels or not: checked once, on the shape that splits by itself and the one that does not."""
    for m, n in ((1000, 800), (3, 5000)):
        F = api.DenseMatrix.from_array_f32(X.matrix(m, n))
        col, colt = X.vector(5, n), X.vector(6, m)
        want = None
        for k in KS:
            for pos in (0, k - 1):
                Xb, Xt = X.vector(70 + k, n, k), X.vector(80 + k, m, k)
                Xb[:, pos] = col; Xt[:, pos] = colt
                if pos:
                    Xb[:, 0] = NAN; Xt[:, 0] = NAN      # a neighbour's NaN stays in its column
                got = [matmat(api, F, Xb, m)[:, pos], matmat(api, F, Xt, n, 1)[:, pos], ata_multi(api, F, Xb)[:, pos]]
                assert not any(np.isnan(g).any() for g in got), (m, n, k, pos)
                want = got if want is None else want
                assert all(X.same_bits(g, w) for g, w in zip(got, want)), (m, n, k, pos)
        F.destroy()


def _same_bits_or_nan_together(a, b, tag):
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (tag, "NaN in other places than the twin's", int(na.sum()), int(nb.sum()))
    assert np.array_equal(X.bits(a)[~na], X.bits(b)[~nb]), (tag, "bits differ from the twin's")


def test_special_values_come_through_as_the_twins(api, lib):
    """fp32 subnormals (1e-40f, the smallest), +-0, FLT_MAX, an Inf row and a quiet-NaN row: NaN where the twin has NaN, the twin's
    bits everywhere else.  x is chosen so that the subnormal rows give nonzero sums a flushing conversion would turn into zeros."""
    K = X.special_matrix()
    m, n = K.shape
    F, D = X.pair(api, K)
    x = np.full(n, 1.5); x[1::2] = 0.75
    xt = np.full(m, 1.25)
    for variant in X.accepted(m, n):
        F.set_kernel(variant); D.set_kernel(variant)
        yf, yd = matvec(api, F, x, m), matvec(api, D, x, m)
        _same_bits_or_nan_together(yf, yd, (variant, "K.x"))
        assert 0.0 < yd[0] < 1e-37 and 0.0 < yd[2] < 1e-37 and np.isinf(yd[20]) and np.isnan(yd[21]) and np.isnan(yd).sum() == 1
        _same_bits_or_nan_together(matvec(api, F, xt, n, 1), matvec(api, D, xt, n, 1), (variant, "K^T.x"))
        _same_bits_or_nan_together(ata(api, F, x), ata(api, D, x), (variant, "ata"))
        for k in KS:
            Xb, Xt = np.repeat(x[:, None], k, axis=1) * (1.0 + np.arange(k)), np.repeat(xt[:, None], k, axis=1) * (1.0 + np.arange(k))
            _same_bits_or_nan_together(matmat(api, F, Xb, m), matmat(api, D, Xb, m), (variant, k, "K.X"))
            _same_bits_or_nan_together(matmat(api, F, Xt, n, 1), matmat(api, D, Xt, n, 1), (variant, k, "K^T.X"))
            _same_bits_or_nan_together(ata_multi(api, F, Xb), ata_multi(api, D, Xb), (variant, k, "ata_multi"))
    # the column sums of squares of the finite part (a column of zeros would be refused): a subnormal float's square is a normal double
    Kf = K.copy(); Kf[20, 3] = 1.0; Kf[21, 9] = 1.0; Kf[:, 12] = 0.5
    F2, D2 = X.pair(api, Kf)
    for a, b in zip(jacobi(api, lib, F2, 1), jacobi(api, lib, D2, 1)):
        assert X.same_bits(a, b)
    for h in (F, D, F2, D2):
        h.destroy()


def test_independent_anchor_on_the_exact_sums(api):
    """K.x and K^T.x of the fp32 handle lie within tests/exact_ref.py's per-row rounding bound of the exact sums of the widened K,
    as tests/test_gpu_exact_products.py holds the fp64 products to it."""
    m, n = 1000, 800
    K = X.matrix(m, n)
    T = X.twin(K)
    F = api.DenseMatrix.from_array_f32(K)
    x, xt = X.vector(11, n), X.vector(12, m)
    er.assert_rows(matvec(api, F, x, m), *dc.dense_as_csr(T), x, tag=("f32", "K.x"))
    er.assert_rows(matvec(api, F, xt, n, 1), *dc.dense_as_csr(np.ascontiguousarray(T.T)), xt, tag=("f32", "K^T.x"))
    F.destroy()


def test_value_bytes_of_every_kind_of_handle(api, lib):
    K = X.matrix(5, 7)
    hs = [api.DenseMatrix.from_array_f32(K), api.DenseMatrix.from_array(K), api.DenseMatrix.from_array(X.twin(K)),
          api.DenseMatrix.from_array(X.twin(K) + 0j), api.DenseMatrix.from_array_c64(K.astype(np.complex64))]
    assert [h.value_bytes for h in hs] == [4, 8, 8, 16, 8]          # from_array keeps widening a float32 array
    A = api.CsrMatrix.from_csr(np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4))
    assert lib.lcg_hip_dense_value_bytes(A.h) == E_ARG and b"lcg_hip_dense_value_bytes" in lib.lcg_hip_last_error()
    for h in hs + [A]:
        h.destroy()


def test_entries_for_other_kinds_refuse_the_handle(api, lib):
    """The complex entries, a _c64 entry and the CSR entries answer the fp32 handle as they answer a real fp64 one: LCG_HIP_E_ARG,
    outputs untouched."""
    F = api.DenseMatrix.from_array_f32(X.matrix(100, 80)[:80])
    D = api.DenseMatrix.from_array(X.twin(X.matrix(100, 80)[:80]))
    x = torch.ones(160, dtype=torch.float64, device="cuda"); y = torch.full((160,), 5.0, dtype=torch.float64, device="cuda")
    xf = torch.ones(160, dtype=torch.float32, device="cuda"); yf = torch.full((160,), 5.0, dtype=torch.float32, device="cuda")
    Xb = torch.ones((80, 4), dtype=torch.float64, device="cuda"); Yb = torch.full((80, 4), 5.0, dtype=torch.float64, device="cuda")
    px, py, pxf, pyf = x.data_ptr(), y.data_ptr(), xf.data_ptr(), yf.data_ptr()
    calls = {
        "clcg_hip_dense_matvec": lambda h: lib.clcg_hip_dense_matvec(h, px, py, 0, 0),
        "clcg_hip_dense_matmat": lambda h: lib.clcg_hip_dense_matmat(h, 2, Xb.data_ptr(), Yb.data_ptr(), 0, 0),
        "clcg_hip_dense_matvec_c64": lambda h: lib.clcg_hip_dense_matvec_c64(h, pxf, pyf, 0, 0),
        "lcg_hip_dense_build_jacobi_c64": lambda h: lib.lcg_hip_dense_build_jacobi_c64(h, None),
        "clcg_hip_dense_matmat_c64": lambda h: lib.clcg_hip_dense_matmat_c64(h, 2, pxf, pyf, 0),
        "lcg_hip_spmv": lambda h: lib.lcg_hip_spmv(h, px, py),
        "lcg_hip_spmm": lambda h: lib.lcg_hip_spmm(h, 4, Xb.data_ptr(), Yb.data_ptr()),
        "lcg_hip_csr_ata": lambda h: lib.lcg_hip_csr_ata(h, px, py),
        "lcg_hip_csr_build_normal": lambda h: lib.lcg_hip_csr_build_normal(h),
        "lcg_hip_csr_rows": lambda h: lib.lcg_hip_csr_rows(h),
        "lcg_hip_csr_destroy": lambda h: lib.lcg_hip_csr_destroy(h),
    }
    for name, call in calls.items():
        rf = call(F.h); ef = lib.lcg_hip_last_error()
        rd = call(D.h); ed = lib.lcg_hip_last_error()
        assert rf == rd == E_ARG and ef == ed and name.encode() in ef, (name, rf, rd, ef, ed)
    # the complex callbacks park their refusal and write nothing
    lib.clcg_hip_dense_ax(F.h, px, py, 80, 0, 0)
    lib.clcg_hip_dense_ax_c64(F.h, pxf, pyf, 80, 0, 0)
    api.synchronize()
    assert torch.all(y == 5.0) and torch.all(yf == 5.0) and torch.all(Yb == 5.0)
    assert (lib.lcg_hip_dense_rows(F.h), lib.lcg_hip_dense_cols(F.h), F.value_bytes) == (80, 80, 4)      # and the handle is unharmed
    out = matvec(api, F, np.ones(80), 80)
    assert X.same_bits(out, matvec(api, D, np.ones(80), 80))
    F.destroy(); D.destroy()


def test_create_checks_with_a_device(api, lib):
    """ld < N, a NULL val and a bad mem: lcg_hip_dense_create's codes, and no handle."""
    K = X.matrix(5, 7)
    Kd = X.twin(K)
    for args32, args64 in (((5, 7, K.ctypes.data, 6, 0), (5, 7, Kd.ctypes.data, 6, 0, 0)),
                           ((5, 7, None, 7, 0), (5, 7, None, 7, 0, 0)),
                           ((5, 7, K.ctypes.data, 7, 2), (5, 7, Kd.ctypes.data, 7, 0, 2)),
                           ((5, 7, K.ctypes.data, 7, -1), (5, 7, Kd.ctypes.data, 7, 0, -1)),
                           ((0, 7, K.ctypes.data, 7, 0), (0, 7, Kd.ctypes.data, 7, 0, 0))):
        h32, h64 = C.c_void_p(1), C.c_void_p(1)
        r32 = lib.lcg_hip_dense_create_f32(C.byref(h32), *args32); e32 = lib.lcg_hip_last_error().decode()
        r64 = lib.lcg_hip_dense_create(C.byref(h64), *args64); e64 = lib.lcg_hip_last_error().decode()
        assert r32 == r64 == E_ARG and h32.value is None and h64.value is None, (args32, r32, r64)
        assert e32 == e64.replace("lcg_hip_dense_create:", "lcg_hip_dense_create_f32:"), (e32, e64)
    assert lib.lcg_hip_dense_create_f32(None, 5, 7, K.ctypes.data, 7, 0) == E_ARG


def test_host_and_device_sources_give_the_same_handle(api):
    for (m, n, ld) in ((1000, 800, None), (37, 29, 40), (5, 7, None)):
        K = X.matrix(m, n)
        src = K if ld is None else X.padded(K, ld)
        Fh = api.DenseMatrix.from_array_f32(src)
        wide = dev(src.base if ld is not None else src)
        Fd = api.DenseMatrix.from_array_f32(wide[:, :n])
        assert ld is None or wide[:, :n].stride(0) == ld
        x, xt = X.vector(21, n), X.vector(22, m)
        assert X.same_bits(matvec(api, Fh, x, m), matvec(api, Fd, x, m)), (m, n, ld)
        assert X.same_bits(matvec(api, Fh, xt, n, 1), matvec(api, Fd, xt, n, 1)), (m, n, ld)
        Fh.destroy(); Fd.destroy()


def test_callers_stream(api, lib):
    """tests/stream_cases.py's late-input pattern for lcg_hip_dense_create_f32: the handle made on the side stream from device memory
    written behind the delay, and the product taken with it, have the bytes of the run on the library's own stream."""
    import stream_cases as st
    env = st.make_env(torch, api, lib)
    try:
        m, n = 300, 240
        K = X.matrix(m, n)
        Ksrc, x_src = dev(K), dev(X.vector(31, n))
        Kd, x = torch.empty_like(Ksrc), torch.empty_like(x_src)
        y = torch.empty(m, dtype=torch.float64, device="cuda")
        made = []

        def create():
            F = api.DenseMatrix.from_array_f32(Kd)
            made.append(F)
            F.matvec(x, y)
            return F.value_bytes

        want = matvec(api, api.DenseMatrix.from_array(X.twin(K)), x_src.cpu().numpy(), m)

        def anchor(r, outs):
            assert r == 4 and X.same_bits(outs[0], want)
        env.pair([(Kd, Ksrc), (x, x_src)], create, [y], False, tag="create_f32", anchor=anchor)
        for F in made:
            F.destroy()
    finally:
        st.close_env(env)
