"""-m gpu: the multi-vector product Y = A.X (lcg_hip_spmm, lcg_hip_spmm_dot) for k = 2, 4, 8 through the C ABI, column by column
against the exact sums and per-row rounding bounds of tests/exact_ref.py.

Shapes: the smallest at which the mapping can go wrong -- rows around the 64-row block, a second LDS window (one row of 3000
entries among rows of 3), empty rows (the first and the last among them), rectangular matrices, and mean row lengths of 100 and
300 entries, where the kernel gives a row 16 and 64 lanes instead of 4.  Y is filled with NaN before every call (an unwritten row
fails)."""
import ctypes as C
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

import exact_ref as X

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E_ARG = -2003
KS = (2, 4, 8)


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random_rows(rng, n, ncols, lens):
    """CSR pattern with the given row lengths, columns drawn anywhere (sorted, distinct within a row)."""
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(ncols, int(m), replace=False)) for m in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rp, col


def _laplace(nx):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx))
    M = (sp.kron(sp.identity(nx), T) + sp.kron(T, sp.identity(nx))).tocsr()
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32)


def shapes():
    """name -> (n_rows, n_cols, rowptr, col)"""
    rng = np.random.default_rng(20260)
    out = {}
    for n in (1, 63, 64, 65, 255, 257, 1000):
        lens = rng.integers(1, min(n, 9) + 1, n)
        out[f"n{n}"] = (n, n) + _random_rows(rng, n, n, lens)
    rp, col = _laplace(30)
    out["laplace30"] = (900, 900, rp, col)
    lens = rng.integers(0, 7, 300); lens[[0, 1, 63, 64, 128, 298, 299]] = 0
    out["empty_rows"] = (300, 300) + _random_rows(rng, 300, 300, lens)
    lens = np.full(200, 3); lens[77] = 3000
    out["arrow"] = (200, 4000) + _random_rows(rng, 200, 4000, lens)
    out["rect_200x77"] = (200, 77) + _random_rows(rng, 200, 77, rng.integers(0, 12, 200))
    out["rect_77x200"] = (77, 200) + _random_rows(rng, 77, 200, rng.integers(0, 12, 77))
    out["mean100"] = (70, 500) + _random_rows(rng, 70, 500, rng.integers(60, 141, 70))        # 16 lanes per row
    out["mean300"] = (37, 5000) + _random_rows(rng, 37, 5000, rng.integers(1, 600, 37) + 150)  # 64 lanes per row, rows over two windows
    return out


SHAPES = shapes()


def spmm(lib, A, k, Xh, n_rows):
    Xd = dev(Xh)
    Y = torch.full((n_rows, k), np.nan, dtype=torch.float64, device="cuda")
    assert lib.lcg_hip_spmm(A.h, k, Xd.data_ptr(), Y.data_ptr()) == 0, lib.lcg_hip_last_error()
    torch.cuda.synchronize()
    return Y.cpu().numpy()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_columns_exact_and_within_the_row_bound(api, lib, name):
    n, nc, rp, col = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lens = np.diff(rp)
    p = X.int_bits(max(1, int(lens.max(initial=1))))
    nnz = int(rp[-1])
    vi = X.int_values(rng, nnz, p)
    vr = rng.standard_normal(nnz) * np.repeat(2.0 ** rng.uniform(-30, 30, n), lens)
    Ai = api.CsrMatrix.from_csr(rp, col, vi, n_cols=nc)
    Ar = api.CsrMatrix.from_csr(rp, col, vr, n_cols=nc)
    for k in KS:
        Xi = np.stack([X.int_values(rng, nc, p, zeros=0.02) for _ in range(k)], axis=1)
        Y = spmm(lib, Ai, k, Xi, n)
        for j in range(k):
            X.assert_exact(np.ascontiguousarray(Y[:, j]), X.exact_int_product(rp, col, vi, Xi[:, j]), (name, k, j))
        Xr = np.stack([rng.standard_normal(nc) * 2.0 ** rng.uniform(-30, 30, nc) for _ in range(k)], axis=1)
        Y = spmm(lib, Ar, k, Xr, n)
        for j in range(k):
            X.assert_rows(np.ascontiguousarray(Y[:, j]), rp, col, vr, Xr[:, j], (name, k, j))
    Ai.destroy(); Ar.destroy()


@pytest.mark.parametrize("name", ["n257", "arrow", "mean100", "mean300", "laplace30"])
def test_a_column_does_not_depend_on_the_others(api, lib, name):
    n, nc, rp, col = SHAPES[name]
    rng = np.random.default_rng(5)
    val = rng.standard_normal(int(rp[-1]))
    A = api.CsrMatrix.from_csr(rp, col, val, n_cols=nc)
    x = [rng.standard_normal(nc) for _ in range(4)]
    Y1 = spmm(lib, A, 4, np.stack(x, axis=1), n)
    Y2 = spmm(lib, A, 4, np.stack([x[0], np.full(nc, np.nan), np.zeros(nc), x[0]], axis=1), n)
    assert np.array_equal(bits(Y1[:, 0]), bits(Y2[:, 0]))
    assert np.array_equal(bits(Y2[:, 3]), bits(Y2[:, 0]))
    assert np.all(Y2[:, 2] == 0.0)
    assert np.all(np.isnan(Y2[np.diff(rp) > 0, 1]))
    Y3 = spmm(lib, A, 4, np.stack(x, axis=1), n)
    assert np.array_equal(Y1.view(np.uint64), Y3.view(np.uint64))             # a second call: the same bits
    # the same column among 2 and among 8: the order of a column's sum is the matrix's alone
    Y4 = spmm(lib, A, 2, np.stack([x[0], x[1]], axis=1), n)
    Y5 = spmm(lib, A, 8, np.stack(x + x, axis=1), n)
    assert np.array_equal(bits(Y4[:, 0]), bits(Y1[:, 0]))
    assert np.array_equal(bits(Y5[:, 4]), bits(Y1[:, 0]))
    A.destroy()


def _laplace_many_blocks():
    """A 5-point Laplacian with more than 512 row blocks: the dots go through the fold."""
    rp, col = _laplace(190)
    return 190 * 190, 190 * 190, rp, col


@pytest.mark.parametrize("name", ["n1", "n65", "n1000", "empty_rows", "arrow", "mean100", "mean300", "many_blocks"])
def test_the_dot_carrying_form(api, lib, name):
    n, nc, rp, col = _laplace_many_blocks() if name == "many_blocks" else SHAPES[name]
    rng = np.random.default_rng(11)
    val = rng.standard_normal(int(rp[-1]))
    A = api.CsrMatrix.from_csr(rp, col, val, n_cols=nc)
    for k in KS:
        Xh = rng.standard_normal((nc, k)); Uh = rng.standard_normal((n, k)) * 2.0 ** rng.uniform(-10, 10, (n, 1))
        Xd, Ud = dev(Xh), dev(Uh)
        Y = torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")
        dots = (C.c_double * k)()
        assert lib.lcg_hip_spmm_dot(A.h, k, Xd.data_ptr(), Y.data_ptr(), Ud.data_ptr(), dots) == 0, lib.lcg_hip_last_error()
        Yh = Y.cpu().numpy()
        Yp = spmm(lib, A, k, Xh, n)
        assert np.array_equal(Yh.view(np.uint64), Yp.view(np.uint64))         # Y itself: the plain product's bits
        for j in range(k):
            X.assert_rows(np.ascontiguousarray(Yh[:, j]), rp, col, val, Xh[:, j], (name, k, j))
            X.assert_dot(dots[j], np.ascontiguousarray(Yh[:, j]), np.ascontiguousarray(Uh[:, j]), (name, k, j))
        dots2 = (C.c_double * k)()
        assert lib.lcg_hip_spmm_dot(A.h, k, Xd.data_ptr(), Y.data_ptr(), Ud.data_ptr(), dots2) == 0
        assert list(dots) == list(dots2)
    A.destroy()


def test_arrays_the_caller_keeps(api, lib):
    """Adopted device arrays without slack behind them and with an 8-byte-aligned base: read entry by entry, never past the end."""
    n, nc, rp, col = SHAPES["n257"]
    rng = np.random.default_rng(3)
    nnz = int(rp[-1])
    val = rng.standard_normal(nnz)
    rpd = dev(rp)
    cold = dev(np.concatenate([[0], col]).astype(np.int32))[1:]         # base 4 mod 16
    vald = dev(np.concatenate([[0.0], val]))[1:]                        # base 8 mod 16
    h = C.c_void_p()
    assert lib.lcg_hip_csr_create(C.byref(h), n, nc, nnz, rpd.data_ptr(), cold.data_ptr(), vald.data_ptr(), 0, 1, 1) == 0
    for k in KS:
        Xh = rng.standard_normal((nc, k))
        Xd = dev(Xh)
        Y = torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")
        assert lib.lcg_hip_spmm(h, k, Xd.data_ptr(), Y.data_ptr()) == 0
        torch.cuda.synchronize()
        Yh = Y.cpu().numpy()
        for j in range(k):
            X.assert_rows(np.ascontiguousarray(Yh[:, j]), rp, col, val, Xh[:, j], ("adopted", k, j))
    lib.lcg_hip_csr_destroy(h)


def test_handles_this_path_does_not_serve(api, lib):
    n, nc, rp, col = SHAPES["n65"]
    rng = np.random.default_rng(9)
    nnz = int(rp[-1])
    Xd = torch.zeros((n, 4), dtype=torch.float64, device="cuda"); Y = torch.zeros_like(Xd)
    p = api.lcg_default_parameters()

    def refused(h, what):
        dots = (C.c_double * 4)()
        for rc in (lib.lcg_hip_spmm(h, 4, Xd.data_ptr(), Y.data_ptr()),
                   lib.lcg_hip_spmm_dot(h, 4, Xd.data_ptr(), Y.data_ptr(), Xd.data_ptr(), dots),
                   lib.lcg_hip_lcg_multi(h, 4, Y.data_ptr(), Xd.data_ptr(), C.byref(p), None, None, None, 1),
                   lib.lcg_hip_lpcg_multi(h, 4, Y.data_ptr(), Xd.data_ptr(), C.byref(p), None, None, None, 1)):
            assert rc == E_ARG, (what, rc)
            err = lib.lcg_hip_last_error().decode()
            assert err and what in err, (what, err)

    Ac = api.CsrMatrix.from_csr(rp, col, rng.standard_normal(nnz) + 1j * rng.standard_normal(nnz))
    refused(Ac.h, "complex")
    A64 = api.CsrMatrix.from_csr_c64(rp, col, (rng.standard_normal(nnz) + 1j * rng.standard_normal(nnz)).astype(np.complex64))
    refused(A64.h, "complex64")
    D = api.DenseMatrix.from_array(rng.standard_normal((n, n)))
    refused(D.h, "dense")
    As = api.CsrMatrix.from_csr(rp, col, rng.standard_normal(nnz), n_cols=2 * n)      # rank 0's rows of a 2n x 2n system
    Xd = torch.zeros((2 * n, 4), dtype=torch.float64, device="cuda")
    assert lib.lcg_hip_spmm(As.h, 4, Xd.data_ptr(), Y.data_ptr()) == 0     # served while it is whole
    assert lib.lcg_hip_csr_split_for_test(As.h, 2 * n, 2, 0) == 0
    refused(As.h, "sharded")
    for M in (Ac, A64, D, As):
        M.destroy()
