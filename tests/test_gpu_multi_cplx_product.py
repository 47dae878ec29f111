"""-m gpu: the complex multi-vector product Y = A.X (clcg_hip_spmm, clcg_hip_spmm_dot) for k = 2, 4, 8 through the C ABI, column by
column against the exact sums and per-row rounding bounds of tests/exact_ref.py.

Shapes: the smallest at which the mapping can go wrong -- rows around the 64-row block, empty rows (the first and the last among
them), rectangular matrices, mean row lengths of 100 and 300 entries (16 and 64 lanes per row instead of 4), n = 1.  Y is filled
with NaN before every call (an unwritten row fails).

The edges of the CMM_W = 1536-entry LDS window (multi_cplx.hpp) are pinned by window_shapes(): a block slice
of exactly CMM_W and CMM_W +- 1 entries, a slice that starts at rowptr % 4 = 1, 2, 3 with a row ending exactly at the window's end,
a row over three windows at R = 16 and at R = 64, a single-row matrix (R = 4, one row in the block), partial last blocks at R = 16
and R = 4.  The dots: bit-exact against the integer sum, in the folded cases (more than MM_MG = 512 row blocks) at R = 64, 16, 4 too."""
import ctypes as C
import zlib

import numpy as np
import pytest

import exact_ref as X
import multi_cplx_cases as cc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E_ARG = -2003
KS = (2, 4, 8)
CMM_W = 1536        # multi_cplx.hpp: entries per LDS window of k_cspmm
assert CMM_W == cc.CMM_W


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


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _random_rows(rng, n, ncols, lens):
    """CSR pattern with the given row lengths, columns drawn anywhere (sorted, distinct within a row)."""
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(ncols, int(m), replace=False)) for m in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rp, col


# the class of rows_per_block (csr_multi.hip) each window shape is there for (the product sets no kernel name: the mean row length is the statement)
WINDOW_CLASS = {"win_exact": 64, "win_plus1": 64, "win_minus1": 64, "win_row_end_1": 64, "win_row_end_2": 64, "win_row_end_3": 64,
                "three_windows": 16, "three_windows_r64": 64, "one_row": 4, "r4_partial": 4, "r16_partial": 16}


def window_shapes(rng):
    """Shapes at the edges of the LDS window (a block's slice of col / val is staged from base = rowptr[row0] & ~3, CMM_W entries at
    a time)."""
    out = {}
    for name, mid in (("win_exact", 24), ("win_plus1", 25), ("win_minus1", 23)):
        lens = np.full(64, 24); lens[31] = mid                  # one block whose slice is CMM_W, CMM_W + 1, CMM_W - 1 entries
        out[name] = (64, 200) + _random_rows(rng, 64, 200, lens)
        assert out[name][2][-1] == CMM_W + mid - 24
    for r in (1, 2, 3):
        # block 1 starts at rowptr = 256 + r (base = 256); its row 47 ends exactly at base + CMM_W, sixteen more rows follow
        lens = np.concatenate([[4 + r], np.full(63, 4), np.full(47, 32), [32 - r], np.full(16, 28)])
        rp, col = _random_rows(rng, 128, 300, lens)
        assert rp[64] % 4 == r and rp[64 + 48] == (rp[64] & ~3) + CMM_W and rp[-1] > rp[64 + 48]
        out[f"win_row_end_{r}"] = (128, 300, rp, col)
    lens = np.full(64, 2); lens[21] = 3500                      # mean 57: R = 16, the long row's 16 lanes walk three windows
    out["three_windows"] = (64, 6000) + _random_rows(rng, 64, 6000, lens)
    lens = np.full(128, 2); lens[85] = 3500                     # mean 29: R = 64, T = 4
    out["three_windows_r64"] = (128, 6000) + _random_rows(rng, 128, 6000, lens)
    out["one_row"] = (1, 6000) + _random_rows(rng, 1, 6000, np.array([3500]))       # R = 4, nrows = 1, three windows
    lens = rng.integers(100, 400, 21); lens[8:12] = (700, 650, 720, 690)            # 4 q + 1 rows; one block's slice is 2760 entries
    out["r4_partial"] = (21, 3000) + _random_rows(rng, 21, 3000, lens)
    out["r16_partial"] = (37, 500) + _random_rows(rng, 37, 500, rng.integers(60, 141, 37))     # 16 q + 5 rows
    for name, R in WINDOW_CLASS.items():
        n, _, rp, _ = out[name]
        assert cc.rows_per_block(rp[-1] / n) == R, (name, rp[-1] / n)
    assert 3500 > 2 * CMM_W
    return out


def shapes():
    """name -> (n_rows, n_cols, rowptr, col)"""
    rng = np.random.default_rng(20261)
    out = {}
    for n in (1, 63, 65, 257, 1000):
        lens = rng.integers(1, min(n, 9) + 1, n)
        out[f"n{n}"] = (n, n) + _random_rows(rng, n, n, lens)
    lens = rng.integers(0, 7, 300); lens[[0, 1, 63, 64, 128, 298, 299]] = 0
    out["empty_rows"] = (300, 300) + _random_rows(rng, 300, 300, lens)
    out["rect_200x77"] = (200, 77) + _random_rows(rng, 200, 77, rng.integers(0, 12, 200))
    out["rect_77x200"] = (77, 200) + _random_rows(rng, 77, 200, rng.integers(0, 12, 77))
    out["mean100"] = (70, 500) + _random_rows(rng, 70, 500, rng.integers(60, 141, 70))        # 16 lanes per row
    out["mean300"] = (37, 5000) + _random_rows(rng, 37, 5000, rng.integers(1, 600, 37) + 150)  # 64 lanes per row
    out.update(window_shapes(rng))
    return out


SHAPES = shapes()


def _fold_shape(kind, n, R):
    S = cc.system(kind, n)
    assert S["R"] == R and S["blocks"] > cc.MM_MG
    return S["n"], S["n"], S["rp"], S["ci"]


# more than MM_MG row blocks: the dots go through k_mm_fold, at every class
MANY_BLOCKS = {"fold_r64": lambda: _fold_shape("helm", 182, 64), "fold_r16": lambda: _fold_shape("band30", 8197, 16),
               "fold_r4": lambda: _fold_shape("band140", 2051, 4)}


def shape(name):
    return MANY_BLOCKS[name]() if name in MANY_BLOCKS else SHAPES[name]


def cspmm(lib, A, k, Xh, n_rows):
    Xd = dev(Xh)
    Y = torch.full((n_rows, k), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
    assert lib.clcg_hip_spmm(A.h, k, Xd.data_ptr(), Y.data_ptr()) == 0, lib.lcg_hip_last_error()
    torch.cuda.synchronize()
    return Y.cpu().numpy()


def cspmm_dot(lib, A, k, Xh, Uh, n_rows):
    Xd, Ud = dev(Xh), dev(Uh)
    Y = torch.full((n_rows, k), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
    dots = (C.c_double * (2 * k))()
    assert lib.clcg_hip_spmm_dot(A.h, k, Xd.data_ptr(), Y.data_ptr(), Ud.data_ptr(), dots) == 0, lib.lcg_hip_last_error()
    return Y.cpu().numpy(), np.array(dots[:]).view(np.complex128)


def exact_int_dot(y, u):
    """sum y_i u_i (unconjugated) of integer-valued complex vectors, exactly; raises if a partial sum could round."""
    yr, yi, ur, ui = (np.asarray(t).astype(np.int64) for t in (y.real, y.imag, u.real, u.imag))
    assert np.array_equal(yr, y.real) and np.array_equal(ui, u.imag)
    assert float(np.abs(yr).astype(np.float64) @ np.abs(ur) + np.abs(yi).astype(np.float64) @ np.abs(ui)) < 2.0 ** 52
    assert float(np.abs(yr).astype(np.float64) @ np.abs(ui) + np.abs(yi).astype(np.float64) @ np.abs(ur)) < 2.0 ** 52
    return complex(float(np.sum(yr * ur - yi * ui)), float(np.sum(yr * ui + yi * ur)))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_columns_exact_and_within_the_row_bound(api, lib, name):
    n, nc, rp, col = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lens = np.diff(rp)
    p = X.int_bits(max(1, int(lens.max(initial=1))), "c128")
    nnz = int(rp[-1])
    vi = X.int_values(rng, nnz, p, cplx=True)
    vr = crand(rng, nnz) * np.repeat(2.0 ** rng.uniform(-30, 30, n), lens)
    Ai = api.CsrMatrix.from_csr(rp, col, vi, n_cols=nc)
    Ar = api.CsrMatrix.from_csr(rp, col, vr, n_cols=nc)
    for k in KS:
        Xi = np.stack([X.int_values(rng, nc, p, cplx=True, zeros=0.02) for _ in range(k)], axis=1)
        Y = cspmm(lib, Ai, k, Xi, n)
        for j in range(k):
            X.assert_exact(np.ascontiguousarray(Y[:, j]), X.exact_int_product(rp, col, vi, Xi[:, j]), (name, k, j))
        Xr = np.stack([crand(rng, nc) * 2.0 ** rng.uniform(-30, 30, nc) for _ in range(k)], axis=1)
        Y = cspmm(lib, Ar, k, Xr, n)
        for j in range(k):
            X.assert_rows(np.ascontiguousarray(Y[:, j]), rp, col, vr, Xr[:, j], (name, k, j))
    Ai.destroy(); Ar.destroy()


@pytest.mark.parametrize("name", ["n1", "n65", "n1000", "empty_rows", "mean100", "mean300", "three_windows", "r4_partial",
                                  "fold_r64", "fold_r16", "fold_r4"])
def test_the_dot_carrying_form_is_exact_on_integers(api, lib, name):
    """A, X in [-2^4, 2^4] and U in [-2^8, 2^8] (integers, both components): every product and partial sum of Y and of the dot is an
    exactly representable integer, so Y equals the integer product and the dot the integer sum BIT FOR BIT whatever the order --
    per-block partials, the fold, msum."""
    n, nc, rp, col = shape(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 7)
    nnz = int(rp[-1])
    vi = X.int_values(rng, nnz, 4, cplx=True)
    A = api.CsrMatrix.from_csr(rp, col, vi, n_cols=nc)
    for k in KS:
        Xi = np.stack([X.int_values(rng, nc, 4, cplx=True, zeros=0.02) for _ in range(k)], axis=1)
        Ui = np.stack([X.int_values(rng, n, 8, cplx=True, zeros=0.02) for _ in range(k)], axis=1)
        Y, dots = cspmm_dot(lib, A, k, Xi, Ui, n)
        Yp = cspmm(lib, A, k, Xi, n)
        assert np.array_equal(bits(Y), bits(Yp))                                # Y itself: the plain product's bits
        for j in range(k):
            ye = X.exact_int_product(rp, col, vi, Xi[:, j])
            X.assert_exact(np.ascontiguousarray(Y[:, j]), ye, (name, k, j))
            want = exact_int_dot(ye, Ui[:, j])
            assert dots[j].real == want.real and dots[j].imag == want.imag, (name, k, j, dots[j], want)
    A.destroy()


@pytest.mark.parametrize("name", ["n257", "mean100", "mean300", "fold_r64", "fold_r4"])
def test_the_dot_on_random_values(api, lib, name):
    """Full-mantissa data: each component of the dot within exact_ref's dot bound of the extended-precision sum of the kernel's own
    Y (2n real products per component), and the same bits from call to call."""
    n, nc, rp, col = shape(name)
    rng = np.random.default_rng(11)
    val = crand(rng, int(rp[-1]))
    A = api.CsrMatrix.from_csr(rp, col, val, n_cols=nc)
    for k in KS:
        Xh = crand(rng, nc, k); Uh = crand(rng, n, k) * 2.0 ** rng.uniform(-10, 10, (n, 1))
        Y, dots = cspmm_dot(lib, A, k, Xh, Uh, n)
        for j in range(k):
            y, u = np.ascontiguousarray(Y[:, j]), np.ascontiguousarray(Uh[:, j])
            X.assert_rows(y, rp, col, val, Xh[:, j], (name, k, j))
            X.assert_dot(dots[j].real, np.concatenate([y.real, -y.imag]), np.concatenate([u.real, u.imag]), (name, k, j, "re"))
            X.assert_dot(dots[j].imag, np.concatenate([y.real, y.imag]), np.concatenate([u.imag, u.real]), (name, k, j, "im"))
        Y2, dots2 = cspmm_dot(lib, A, k, Xh, Uh, n)
        assert np.array_equal(bits(dots), bits(dots2)) and np.array_equal(bits(Y), bits(Y2))
    A.destroy()


@pytest.mark.parametrize("name", ["n257", "mean100", "mean300", "three_windows", "fold_r64"])
def test_a_column_does_not_depend_on_the_others(api, lib, name):
    n, nc, rp, col = shape(name)
    rng = np.random.default_rng(5)
    val = crand(rng, int(rp[-1]))
    A = api.CsrMatrix.from_csr(rp, col, val, n_cols=nc)
    x = [crand(rng, nc) for _ in range(4)]
    u = [crand(rng, n) for _ in range(4)]
    Y1, d1 = cspmm_dot(lib, A, 4, np.stack(x, axis=1), np.stack(u, axis=1), n)
    bad = [np.full(nc, complex(np.nan, np.nan)), np.full(nc, complex(np.inf, -np.inf)), np.zeros(nc, np.complex128)]
    Y2, d2 = cspmm_dot(lib, A, 4, np.stack([x[0], bad[0], bad[1], x[0]], axis=1), np.stack([u[0], u[1], u[2], u[0]], axis=1), n)
    assert np.array_equal(bits(Y1[:, 0]), bits(Y2[:, 0])) and bits(d1[0:1]).tolist() == bits(d2[0:1]).tolist()
    assert np.array_equal(bits(Y2[:, 3]), bits(Y2[:, 0])) and bits(d2[3:4]).tolist() == bits(d2[0:1]).tolist()
    assert np.all(np.isnan(Y2[np.diff(rp) > 0, 1].real))
    Y3, d3 = cspmm_dot(lib, A, 4, np.stack(x, axis=1), np.stack(u, axis=1), n)
    assert np.array_equal(bits(Y1), bits(Y3)) and np.array_equal(bits(d1), bits(d3))      # a second call: the same bits
    # the same column among 2 and among 8: the order of a column's sums is the matrix's alone
    Y4, d4 = cspmm_dot(lib, A, 2, np.stack([bad[2], x[0]], axis=1), np.stack([u[1], u[0]], axis=1), n)
    Y5, d5 = cspmm_dot(lib, A, 8, np.stack(x + [x[0]] + bad, axis=1), np.stack(u + u, axis=1), n)
    assert np.array_equal(bits(Y4[:, 1]), bits(Y1[:, 0])) and bits(d4[1:2]).tolist() == bits(d1[0:1]).tolist()
    assert np.array_equal(bits(Y5[:, 4]), bits(Y1[:, 0])) and bits(d5[4:5]).tolist() == bits(d1[0:1]).tolist()
    assert np.all(Y4[:, 0] == 0.0)
    # the plain product: the same bits as the dot-carrying one
    assert np.array_equal(bits(cspmm(lib, A, 4, np.stack(x, axis=1), n)), bits(Y1))
    A.destroy()


def test_arrays_the_caller_keeps(api, lib):
    """Adopted device arrays with an 8-byte-aligned value base and no slack: read entry by entry, never past the slice.  The arrays
    are views into longer tensors of the test's own: behind col lie zeros, behind val NaN, so an entry read past a slice and used
    shows as NaN in Y (row 0 of X is finite) while no address outside the allocation is touched.  And Y is the copied matrix's Y bit
    for bit: the order of a sum is the matrix's alone."""
    for name in ("n257", "three_windows", "three_windows_r64", "r16_partial", "r4_partial", "win_row_end_3"):
        n, nc, rp, col = SHAPES[name]
        rng = np.random.default_rng(3)
        nnz = int(rp[-1])
        val = crand(rng, nnz)
        tail = 64 if name != "n257" else 0          # (n257: nothing at all behind the arrays)
        rpd = dev(rp)
        cold = dev(np.concatenate([[0], col, np.zeros(tail)]).astype(np.int32))[1:1 + nnz]                       # base 4 mod 16
        vald = dev(np.concatenate([[0.0], val.view(np.float64), np.full(2 * tail, np.nan)]))[1:1 + 2 * nnz]     # base 8 mod 16
        assert cold.data_ptr() % 16 == 4 and vald.data_ptr() % 16 == 8
        h = C.c_void_p()
        assert lib.lcg_hip_csr_create(C.byref(h), n, nc, nnz, rpd.data_ptr(), cold.data_ptr(), vald.data_ptr(), 1, 1, 1) == 0
        A = api.CsrMatrix.from_csr(rp, col, val, n_cols=nc)
        for k in KS:
            Xh = crand(rng, nc, k)
            Xd = dev(Xh)
            Y = torch.full((n, k), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
            assert lib.clcg_hip_spmm(h, k, Xd.data_ptr(), Y.data_ptr()) == 0
            torch.cuda.synchronize()
            Yh = Y.cpu().numpy()
            for j in range(k):
                X.assert_rows(np.ascontiguousarray(Yh[:, j]), rp, col, val, Xh[:, j], ("adopted", name, k, j))
            assert np.array_equal(bits(Yh), bits(cspmm(lib, A, k, Xh, n))), (name, k)
        lib.lcg_hip_csr_destroy(h)
        A.destroy()


def test_handles_this_path_does_not_serve(api, lib):
    n, nc, rp, col = SHAPES["n65"]
    rng = np.random.default_rng(9)
    nnz = int(rp[-1])
    Xd = torch.zeros((n, 4), dtype=torch.complex128, device="cuda")
    sentinel = complex(7.0, -3.0)
    p = api.clcg_default_parameters()

    def refused(h, what, rows=n):
        dots = (C.c_double * 8)()
        Xr = torch.zeros((rows, 4), dtype=torch.complex128, device="cuda")
        Y = torch.full((n, 4), sentinel, dtype=torch.complex128, device="cuda")
        for rc in (lib.clcg_hip_spmm(h, 4, Xr.data_ptr(), Y.data_ptr()),
                   lib.clcg_hip_spmm_dot(h, 4, Xr.data_ptr(), Y.data_ptr(), Y.data_ptr(), dots),
                   lib.clcg_hip_lbicg_sym_multi(h, 4, Y.data_ptr(), Xd.data_ptr(), C.byref(p), None, None, None, 1),
                   lib.clcg_hip_lpcg_multi(h, 4, Y.data_ptr(), Xd.data_ptr(), C.byref(p), None, None, None, 1)):
            assert rc == E_ARG, (what, rc)
            err = lib.lcg_hip_last_error().decode()
            assert err and what in err, (what, err)
        torch.cuda.synchronize()
        assert bool((Y == sentinel).all()), what                                # Y untouched

    Ar = api.CsrMatrix.from_csr(rp, col, rng.standard_normal(nnz))
    refused(Ar.h, "real")
    A64 = api.CsrMatrix.from_csr_c64(rp, col, crand(rng, nnz).astype(np.complex64))
    refused(A64.h, "complex64")
    D = api.DenseMatrix.from_array(crand(rng, n, n))
    refused(D.h, "dense")
    As = api.CsrMatrix.from_csr(rp, col, crand(rng, nnz), n_cols=2 * n)        # rank 0's rows of a 2n x 2n system
    X2 = torch.zeros((2 * n, 4), dtype=torch.complex128, device="cuda"); Y2 = torch.zeros((n, 4), dtype=torch.complex128, device="cuda")
    assert lib.clcg_hip_spmm(As.h, 4, X2.data_ptr(), Y2.data_ptr()) == 0       # served while it is whole
    assert lib.lcg_hip_csr_split_for_test(As.h, 2 * n, 2, 0) == 0
    refused(As.h, "sharded", rows=2 * n)
    # and the real product keeps refusing complex handles
    Ac = api.CsrMatrix.from_csr(rp, col, crand(rng, nnz))
    Xf = torch.zeros((n, 4), dtype=torch.float64, device="cuda"); Yf = torch.zeros_like(Xf)
    assert lib.lcg_hip_spmm(Ac.h, 4, Xf.data_ptr(), Yf.data_ptr()) == E_ARG and "complex" in lib.lcg_hip_last_error().decode()
    for M in (Ar, A64, D, As, Ac):
        M.destroy()


def test_python_front(api):
    n, nc, rp, col = SHAPES["n257"]
    rng = np.random.default_rng(2)
    val = crand(rng, int(rp[-1]))
    A = api.CsrMatrix.from_csr(rp, col, val, n_cols=nc)
    Xh, Uh = crand(rng, nc, 4), crand(rng, n, 4)
    Xd, Ud = dev(Xh), dev(Uh)
    Y = torch.full((n, 4), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
    A.cspmm(Xd, Y)
    api.synchronize()
    Yh = Y.cpu().numpy()
    for j in range(4):
        X.assert_rows(np.ascontiguousarray(Yh[:, j]), rp, col, val, Xh[:, j], ("front", j))
    dots = A.cspmm_dot(Xd, Y, Ud)
    assert dots.dtype == np.complex128 and dots.shape == (4,)
    want = np.sum(Yh * Uh, axis=0)
    assert np.all(np.abs(dots - want) <= 1e-12 * np.sum(np.abs(Yh * Uh), axis=0))
    with pytest.raises(ValueError):
        A.cspmm(Xd.real.contiguous(), Y)
    A.destroy()
