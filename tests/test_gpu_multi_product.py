"""-m gpu: the multi-vector product Y = A.X (lcg_hip_spmm, lcg_hip_spmm_dot) for k = 2, 4, 8 through the C ABI, column by column
against the exact sums and per-row rounding bounds of tests/exact_ref.py.

Shapes: the smallest at which the mapping can go wrong -- rows around the 64-row block, a second LDS window (one row of 3000
entries among rows of 3), empty rows (the first and the last among them), rectangular matrices, and mean row lengths of 100 and
300 entries, where the kernel gives a row 16 and 64 lanes instead of 4.  Y is filled with NaN before every call (an unwritten row
fails).

The edges of the MM_CH = 2304-entry LDS window are pinned by the shapes of window_shapes(): a block slice of exactly 2304 and
2304 +- 1 entries, a slice that starts at rowptr % 4 = 1, 2, 3 with a row ending exactly at the window's end, a row over three
windows at R = 16 and at R = 64, a single-row matrix (R = 4, one row in the block), partial last blocks at R = 16 and R = 4.
NaN and +-Inf in a few rows of X: test_nonfinite_x_stays_in_its_rows_of_every_column; the folded dots at R = 16 and R = 4:
test_the_dot_carrying_form[band30_8197 / band140_2051]; adopted arrays with poison behind them: test_arrays_the_caller_keeps.  The
batched loops' branches are pinned by tests/test_gpu_multi_edges.py."""
import ctypes as C
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

import exact_ref as X
import multi_cases as mc

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
    out.update(window_shapes(rng))
    return out


MM_CH = 2304        # csr_multi.hip: entries per LDS window
# the class of rows_per_block each window shape is there for (the product sets no kernel name: the mean row length is the statement)
WINDOW_CLASS = {"win_exact": 64, "win_plus1": 64, "win_minus1": 64, "win_row_end_1": 64, "win_row_end_2": 64, "win_row_end_3": 64,
                "three_windows": 16, "three_windows_r64": 64, "one_row": 4, "r4_partial": 4, "r16_partial": 16}


def window_shapes(rng):
    """Shapes at the edges of the LDS window (a block's slice of col / val is staged from base = rowptr[row0] & ~3, MM_CH entries at
    a time)."""
    out = {}
    for name, mid in (("win_exact", 36), ("win_plus1", 37), ("win_minus1", 35)):
        lens = np.full(64, 36); lens[31] = mid                  # one block whose slice is MM_CH, MM_CH + 1, MM_CH - 1 entries
        out[name] = (64, 200) + _random_rows(rng, 64, 200, lens)
    for r in (1, 2, 3):
        # block 1 starts at rowptr = 256 + r (base = 256); its row 47 ends exactly at base + MM_CH, sixteen more rows follow
        lens = np.concatenate([[4 + r], np.full(63, 4), np.full(47, 48), [48 - r], np.full(16, 40)])
        rp, col = _random_rows(rng, 128, 300, lens)
        assert rp[64] % 4 == r and rp[64 + 48] == (rp[64] & ~3) + MM_CH and rp[-1] > rp[64 + 48]
        out[f"win_row_end_{r}"] = (128, 300, rp, col)
    lens = np.full(64, 2); lens[21] = 5000                      # mean 80: R = 16, the long row's 16 lanes walk three windows
    out["three_windows"] = (64, 6000) + _random_rows(rng, 64, 6000, lens)
    lens = np.full(128, 2); lens[85] = 5000                     # mean 41: R = 64, T = 4
    out["three_windows_r64"] = (128, 6000) + _random_rows(rng, 128, 6000, lens)
    out["one_row"] = (1, 6000) + _random_rows(rng, 1, 6000, np.array([5000]))       # R = 4, nrows = 1, three windows
    lens = rng.integers(100, 400, 21); lens[8:12] = (700, 650, 720, 690)            # 4 q + 1 rows; one block's slice is 2760 entries
    out["r4_partial"] = (21, 3000) + _random_rows(rng, 21, 3000, lens)
    out["r16_partial"] = (37, 500) + _random_rows(rng, 37, 500, rng.integers(60, 141, 37))     # 16 q + 5 rows
    for name, R in WINDOW_CLASS.items():
        n, _, rp, _ = out[name]
        assert mc.rows_per_block(rp[-1] / n) == R, (name, rp[-1] / n)
    assert any(out["r4_partial"][2][min(21, r0 + 4)] - out["r4_partial"][2][r0] > MM_CH for r0 in range(0, 21, 4))
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


def _band_many_blocks(n, h, R):
    """The dense band of multi_cases at the smallest size with 513 row blocks of R rows: the fold at R = 16 and R = 4."""
    rp, col, _ = mc.band_pattern(n, h)
    assert mc.rows_per_block(rp[-1] / n) == R and -(-n // R) == mc.MM_MG + 1
    return n, n, rp, col


MANY_BLOCKS = {"many_blocks": _laplace_many_blocks, "band30_8197": lambda: _band_many_blocks(8197, 30, 16),
               "band140_2051": lambda: _band_many_blocks(2051, 140, 4)}


@pytest.mark.parametrize("name", ["n1", "n65", "n1000", "empty_rows", "arrow", "mean100", "mean300", "many_blocks", "band30_8197", "band140_2051"])
def test_the_dot_carrying_form(api, lib, name):
    n, nc, rp, col = MANY_BLOCKS[name]() if name in MANY_BLOCKS else SHAPES[name]
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
    """Adopted device arrays with an 8-byte-aligned base: read entry by entry, never past the slice.  The arrays are views into
    longer tensors of the test's own: behind col lie zeros, behind val NaN, so an entry read past a slice and used shows as NaN in Y
    (row 0 of X is finite) while no address outside the allocation is touched.  And Y is the copied matrix's Y bit for bit: the
    order of a sum is the matrix's alone."""
    for name in ("n257", "arrow", "three_windows", "three_windows_r64", "r16_partial", "r4_partial"):
        n, nc, rp, col = SHAPES[name]
        rng = np.random.default_rng(3)
        nnz = int(rp[-1])
        val = rng.standard_normal(nnz)
        tail = 64 if name != "n257" else 0          # (n257: no slack at all behind the arrays, as before)
        rpd = dev(rp)
        cold = dev(np.concatenate([[0], col, np.zeros(tail)]).astype(np.int32))[1:1 + nnz]       # base 4 mod 16
        vald = dev(np.concatenate([[0.0], val, np.full(tail, np.nan)]))[1:1 + nnz]              # base 8 mod 16
        assert cold.data_ptr() % 16 == 4 and vald.data_ptr() % 16 == 8
        h = C.c_void_p()
        assert lib.lcg_hip_csr_create(C.byref(h), n, nc, nnz, rpd.data_ptr(), cold.data_ptr(), vald.data_ptr(), 0, 1, 1) == 0
        A = api.CsrMatrix.from_csr(rp, col, val, n_cols=nc)
        for k in KS:
            Xh = rng.standard_normal((nc, k))
            Xd = dev(Xh)
            Y = torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")
            assert lib.lcg_hip_spmm(h, k, Xd.data_ptr(), Y.data_ptr()) == 0
            torch.cuda.synchronize()
            Yh = Y.cpu().numpy()
            for j in range(k):
                X.assert_rows(np.ascontiguousarray(Yh[:, j]), rp, col, val, Xh[:, j], ("adopted", name, k, j))
            assert np.array_equal(bits(Yh), bits(spmm(lib, A, k, Xh, n))), (name, k)
        lib.lcg_hip_csr_destroy(h)
        A.destroy()


@pytest.mark.parametrize("name", ["n1000", "r16_partial", "r4_partial", "three_windows", "three_windows_r64", "one_row"])
def test_nonfinite_x_stays_in_its_rows_of_every_column(api, lib, name):
    """NaN, +Inf and -Inf in X at row 0, the last row and a few referenced rows (explicitly stored zeros in val), in one column and
    in all of them: a row of Y that references none of them is, bit for bit, the row of the run with those entries 0 -- no lane past
    the window (which re-reads its first unit), no lane past nrows and no reuse of the staging buffer leaks them -- and a row that
    does has the category of an ordered sum.  One shape per R class, the rows over three windows and the single row."""
    from test_gpu_exact_products import _nonfinite_check, _specials
    n, nc, rp, col = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    val = rng.standard_normal(int(rp[-1]))
    val[rng.random(len(val)) < 0.05] = 0.0
    A = api.CsrMatrix.from_csr(rp, col, val, n_cols=nc)
    cs, kinds = _specials(rng, col, nc)
    for k in KS:
        Xh = rng.standard_normal((nc, k))
        X0 = Xh.copy(); X0[cs, :] = 0.0
        Y0 = spmm(lib, A, k, X0, n)
        jc = k - 1
        X1 = X0.copy(); X1[cs, jc] = kinds              # one column
        Xa = X0.copy(); Xa[cs, :] = kinds[:, None]      # all columns
        Y1, Ya = spmm(lib, A, k, X1, n), spmm(lib, A, k, Xa, n)
        for j in range(k):
            _nonfinite_check(np.ascontiguousarray(Ya[:, j]), np.ascontiguousarray(Y0[:, j]), rp, col, val, Xa[:, j], cs, (name, k, j, "all"))
            if j == jc:
                _nonfinite_check(np.ascontiguousarray(Y1[:, j]), np.ascontiguousarray(Y0[:, j]), rp, col, val, X1[:, j], cs, (name, k, j, "one"))
            else:
                assert np.array_equal(bits(Y1[:, j]), bits(Y0[:, j])), (name, k, j)     # the untouched columns: the clean run's bits
    A.destroy()


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
