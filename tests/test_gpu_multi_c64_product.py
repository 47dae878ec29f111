"""-m gpu: the complex64 multi-vector product Y = A.X (clcg_hip_spmm_c64, clcg_hip_spmm_dot_c64) for k = 2, 4, 8 through the C ABI,
column by column against the exact sums and per-row rounding bounds of tests/exact_ref.py.

Systems (patterns of tests/multi_cplx_cases.py, by the class of rows_per_block: mean row length <= 48 -> R = 64 rows per block and
T = 4 lanes per row, <= 256 -> R = 16, T = 16, more -> R = 4, T = 64): chain n = 1, 2, 3, 65, 513; helm 40; helm 182 (more than 512 row
blocks of 64: the fold); band30 1029 (R = 16, partial last block); band30 8197 (R = 16 folded); band140 2051 (R = 4 folded); band260
261 (R = 4, last block of one row); tests/test_gpu_c64.py's ragged() (empty rows, one row of 5000 entries that spans three LDS windows
of 2304).  Y is filled with NaN before every call (an unwritten row fails)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import exact_ref as X
import multi_cplx_cases as mcc
import multi_c64_cases as cc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E_ARG = -2003
KS = (2, 4, 8)
U32 = 2.0 ** -24

SYSTEMS = [("chain", 1), ("chain", 2), ("chain", 3), ("chain", 65), ("chain", 513), ("helm", 40), ("helm", 182), ("band30", 1029),
           ("band30", 8197), ("band140", 2051), ("band260", 261), ("ragged", 0)]
# key -> (R, folded: more than MM_MG row blocks)
CLASS = dict(mcc.CLASS)
CLASS[("ragged", 0)] = (64, False)
IDS = [f"{k}-{n}" for k, n in SYSTEMS]


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


_PATTERNS = {}


def pattern(key):
    """(n, rowptr, col, R) of a system; its class is asserted against the statement above."""
    if key not in _PATTERNS:
        if key[0] == "ragged":
            from test_gpu_c64 import ragged
            rp, ci, _ = ragged()
            assert np.diff(rp).max() == 5000 > 2 * cc.C64MM_W and (np.diff(rp) == 0).any()
        else:
            S = mcc.system(*key)
            rp, ci = S["rp"], S["ci"]
        n = len(rp) - 1
        R = mcc.rows_per_block(float(rp[-1]) / n)
        assert R == CLASS[key][0] and ((n + R - 1) // R > mcc.MM_MG) == CLASS[key][1], key
        _PATTERNS[key] = (n, np.asarray(rp, np.int32), np.asarray(ci, np.int32), R)
    return _PATTERNS[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def cspmm(lib, A, k, Xh, n_rows):
    Xd = dev(np.asarray(Xh, np.complex64))
    Y = torch.full((n_rows, k), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
    assert lib.clcg_hip_spmm_c64(A.h, k, Xd.data_ptr(), Y.data_ptr()) == 0, lib.lcg_hip_last_error()
    torch.cuda.synchronize()
    return Y.cpu().numpy()


def cspmm_dot(lib, A, k, Xh, Uh, n_rows):
    Xd, Ud = dev(np.asarray(Xh, np.complex64)), dev(np.asarray(Uh, np.complex64))
    Y = torch.full((n_rows, k), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
    dots = (C.c_double * (2 * k))()
    assert lib.clcg_hip_spmm_dot_c64(A.h, k, Xd.data_ptr(), Y.data_ptr(), Ud.data_ptr(), dots) == 0, lib.lcg_hip_last_error()
    return Y.cpu().numpy(), np.array(dots[:]).view(np.complex128)


def exact_int_dot(y, u):
    """sum y_i u_i (unconjugated) of integer-valued complex vectors, exactly; raises if a partial sum could round in fp64."""
    yr, yi, ur, ui = (np.asarray(t).astype(np.int64) for t in (y.real, y.imag, u.real, u.imag))
    assert np.array_equal(yr, y.real) and np.array_equal(ui, u.imag)
    assert float(np.abs(yr).astype(np.float64) @ np.abs(ur) + np.abs(yi).astype(np.float64) @ np.abs(ui)) < 2.0 ** 52
    assert float(np.abs(yr).astype(np.float64) @ np.abs(ui) + np.abs(yi).astype(np.float64) @ np.abs(ur)) < 2.0 ** 52
    return complex(float(np.sum(yr * ur - yi * ui)), float(np.sum(yr * ui + yi * ur)))


@pytest.mark.parametrize("key", SYSTEMS, ids=IDS)
def test_exact_sums_on_integers(api, lib, key):
    """A, X and U integers (both components) of at most exact_ref.int_bits(longest row, "c64") bits: every product and every
    partial sum of a row is an integer of at most 23 bits, which fp32 represents exactly, so Y equals the int64 product BIT FOR BIT
    in every column whatever the order -- a lane's fma chain, the slot adds.  The dot's terms are integers below 2^52 in all
    (n <= 2^19): dots equals the integer sum bit for bit whatever the order -- per-block partials, the fold, msum.  The
    dot-carrying form writes the plain product's Y."""
    n, rp, ci, _ = pattern(key)
    assert n <= 2 ** 19
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    p = X.int_bits(int(np.diff(rp).max()), "c64")
    vi = X.int_values(rng, int(rp[-1]), p, cplx=True)
    A = api.CsrMatrix.from_csr_c64(rp, ci, vi)
    for k in KS:
        Xi = np.stack([X.int_values(rng, n, p, cplx=True, zeros=0.02) for _ in range(k)], axis=1)
        Ui = np.stack([X.int_values(rng, n, p, cplx=True, zeros=0.02) for _ in range(k)], axis=1)
        Yp = cspmm(lib, A, k, Xi, n)
        Y, dots = cspmm_dot(lib, A, k, Xi, Ui, n)
        assert np.array_equal(bits(Y), bits(Yp))
        for j in range(k):
            ye = X.exact_int_product(rp, ci, vi, Xi[:, j])
            X.assert_exact(np.ascontiguousarray(Y[:, j]), ye.astype(np.complex64), (key, k, j))
            want = exact_int_dot(ye, Ui[:, j])
            assert dots[j].real == want.real and dots[j].imag == want.imag, (key, k, j, dots[j], want)
    A.destroy()


@pytest.mark.parametrize("key", [("helm", 40), ("band140", 2051), ("ragged", 0)], ids=lambda k: f"{k[0]}-{k[1]}")
def test_rounding_bound_on_full_mantissa_data(api, lib, key):
    """|y_i - y_ref,i| <= 3 (len_i + 5 + T) 2^-24 (|A||x|)_i, T = 256 / R the lanes of a row.  tests/test_gpu_c64.py's derivation with
    the row-sum exchange in place of the butterfly: each real component of a row's sum is a chain of fp32 roundings -- two fma per
    entry on the way through a lane (at most 2 len_i in all), then the T - 1 slot adds that join the lanes' partial sums, where
    lcg_hip_spmv_c64 has at most 9 butterfly adds.  With m <= 2 len_i + T roundings on any term's way to the root, |error| <=
    gamma_m sum |terms| ~ m u sum |terms| (Higham 3.1 / 4.2), a component's terms sum to at most (|A||x|)_i (Cauchy-Schwarz), and the
    modulus of the two components' errors adds sqrt(2): sqrt(2) (2 len_i + T) = 2.83 (len_i + T / 2) <= 3 (len_i + 5 + T).
    The reference is exact_ref.hp_product on the complex64-rounded inputs (its own error, 2^-64 relative per term, is far below).
    The dot: each component is a sum of 2 n exact fp64 products of the kernel's own Y with U, held to exact_ref.dot_bound with the
    fp64 unit roundoff."""
    n, rp, ci, R = pattern(key)
    T = 256 // R
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()) + 1)
    lens = np.diff(rp)
    v = (crand(rng, int(rp[-1])) * np.repeat(2.0 ** rng.uniform(-8, 8, n), lens)).astype(np.complex64)
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    for k in KS:
        Xr = np.stack([crand(rng, n) * 2.0 ** rng.uniform(-8, 8, n) for _ in range(k)], axis=1).astype(np.complex64)
        Ur = np.stack([crand(rng, n) for _ in range(k)], axis=1).astype(np.complex64)
        Y, dots = cspmm_dot(lib, A, k, Xr, Ur, n)
        for j in range(k):
            ref = X.hp_product(rp, ci, v.astype(np.complex128), Xr[:, j].astype(np.complex128))
            err = X.row_errors(Y[:, j].astype(np.complex128), ref)
            bound = 3.0 * (lens + 5 + T) * U32 * ref[2] + 1e-30
            worst = float(np.max(err / bound))
            print(key, k, j, "worst error / bound", worst)
            assert np.all(err <= bound), (key, k, j, worst)
            y, u = Y[:, j].astype(np.complex128), Ur[:, j].astype(np.complex128)
            X.assert_dot(dots[j].real, np.concatenate([y.real, -y.imag]), np.concatenate([u.real, u.imag]), (key, k, j, "re"))
            X.assert_dot(dots[j].imag, np.concatenate([y.real, y.imag]), np.concatenate([u.imag, u.real]), (key, k, j, "im"))
    A.destroy()


@pytest.mark.parametrize("key", [("helm", 182), ("band30", 1029), ("ragged", 0)], ids=lambda k: f"{k[0]}-{k[1]}")
def test_a_column_does_not_depend_on_its_neighbours_its_place_or_k(api, lib, key):
    """The same column at every position of k = 2, 4 and 8 blocks, the other columns holding NaN, Inf and large values: its bytes of
    Y and its two dots are identical in every case, and two calls give the same bytes."""
    n, rp, ci, _ = pattern(key)
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()) + 2)
    v = crand(rng, int(rp[-1])).astype(np.complex64)
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    x, u = crand(rng, n).astype(np.complex64), crand(rng, n).astype(np.complex64)
    fill = [complex(np.nan, np.nan), complex(np.inf, -np.inf), complex(3e37, -3e37), complex(1.0, np.nan)]
    base = None
    for k in KS:
        for pos in range(k):
            Xh = np.empty((n, k), np.complex64); Uh = np.empty((n, k), np.complex64)
            for j in range(k):
                Xh[:, j] = fill[(j + pos) % 4]; Uh[:, j] = fill[(j + pos + 1) % 4]
            Xh[:, pos], Uh[:, pos] = x, u
            Y, dots = cspmm_dot(lib, A, k, Xh, Uh, n)
            got = (bits(Y[:, pos]).copy(), dots[pos].real.tobytes() + dots[pos].imag.tobytes())
            assert np.isfinite(np.ascontiguousarray(Y[:, pos]).view(np.float32)).all() and np.isfinite(dots[pos])
            if base is None:
                base = got
                Y2, dots2 = cspmm_dot(lib, A, k, Xh, Uh, n)
                assert Y.tobytes() == Y2.tobytes() and dots.tobytes() == dots2.tobytes()
            assert np.array_equal(got[0], base[0]) and got[1] == base[1], (key, k, pos)
    A.destroy()


@pytest.mark.parametrize("key", [("chain", 3), ("helm", 40), ("band30", 1029), ("band260", 261), ("ragged", 0)], ids=lambda k: f"{k[0]}-{k[1]}")
def test_both_load_paths_give_the_same_bytes(api, lib, key):
    """Copied arrays (16-byte aligned with slack behind them: the branch-free 16-byte loads) and device arrays adopted without slack
    (entry by entry, never past the slice)."""
    n, rp, ci, _ = pattern(key)
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()) + 3)
    v = crand(rng, int(rp[-1])).astype(np.complex64)
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)
    B = api.CsrMatrix.from_csr_c64(dev(rp), dev(ci), dev(v), adopt=True)
    for k in KS:
        Xh, Uh = crand(rng, n, k).astype(np.complex64), crand(rng, n, k).astype(np.complex64)
        Ya, da = cspmm_dot(lib, A, k, Xh, Uh, n)
        Yb, db = cspmm_dot(lib, B, k, Xh, Uh, n)
        assert Ya.tobytes() == Yb.tobytes() and da.tobytes() == db.tobytes(), (key, k)
        assert cspmm(lib, B, k, Xh, n).tobytes() == Ya.tobytes()
    A.destroy(); B.destroy()


def test_other_handles_are_refused_and_y_stays_untouched(api, lib):
    S = mcc.system("helm", 40)
    n, rp, ci = S["n"], S["rp"], S["ci"]
    A64 = api.CsrMatrix.from_csr_c64(rp, ci, S["v"])
    A128 = api.CsrMatrix.from_csr(rp, ci, S["v"])
    Areal = api.CsrMatrix.from_csr(rp, ci, S["v"].real.copy())
    D = api.DenseMatrix.from_array(np.eye(n))
    x = torch.ones((n, 4), dtype=torch.complex64, device="cuda")
    dots = (C.c_double * 8)()
    for H, word in ((A128, "complex128"), (Areal, "real"), (D, "dense")):
        for entry in ("spmm", "dot"):
            y = torch.full((n, 4), 7.0 + 0j, dtype=torch.complex64, device="cuda")
            if entry == "spmm":
                rc = lib.clcg_hip_spmm_c64(H.h, 4, x.data_ptr(), y.data_ptr())
            else:
                rc = lib.clcg_hip_spmm_dot_c64(H.h, 4, x.data_ptr(), y.data_ptr(), x.data_ptr(), dots)
            assert rc == E_ARG, (word, entry, rc)
            assert word in lib.lcg_hip_last_error().decode().lower(), lib.lcg_hip_last_error()
            torch.cuda.synchronize()
            assert bool((y == 7.0).all())
    # the complex128 entries still refuse the complex64 handle, with the text they have always had
    xz = torch.ones((n, 4), dtype=torch.complex128, device="cuda")
    yz = torch.full((n, 4), 7.0 + 0j, dtype=torch.complex128, device="cuda")
    assert lib.clcg_hip_spmm(A64.h, 4, xz.data_ptr(), yz.data_ptr()) == E_ARG
    assert lib.lcg_hip_last_error().decode() == ("clcg_hip_spmm: the matrix holds complex64 values; the complex multi-vector path "
                                                 "serves complex128 matrices")
    assert lib.lcg_hip_spmm(A64.h, 4, xz.data_ptr(), yz.data_ptr()) == E_ARG
    assert "complex64" in lib.lcg_hip_last_error().decode()
    torch.cuda.synchronize()
    assert bool((yz == 7.0).all())
    # and the Python front
    Y = torch.full((n, 4), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
    A64.cspmm_c64(x, Y)
    d = A64.cspmm_dot_c64(x, Y, x)
    api.synchronize()
    ref = S["v"].astype(np.complex64).astype(np.complex128)
    want = np.add.reduceat(ref, rp[:-1])
    assert np.allclose(Y.cpu().numpy()[:, 2], want, rtol=1e-5, atol=1e-5) and d.shape == (4,) and np.allclose(d, want.sum(), rtol=1e-5)
    for H in (A64, A128, Areal, D):
        H.destroy()
