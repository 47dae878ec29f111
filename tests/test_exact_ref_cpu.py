"""CPU: the reference and bounds of tests/exact_ref.py have teeth.  Correct products in other orders pass the per-row bound
(and, on integer data, bit equality); products that are subtly wrong -- values kept to 45 mantissa bits, x rounded to fp32, an
entry dropped, doubled or moved to the next row, a row never written -- fail them, on ragged matrices with empty rows and rows of
1 .. 3 entries where a band scaled by the largest row would see nothing."""
import numpy as np
import pytest

import exact_ref as X


def _ragged(seed, n=600, max_len=40, cplx=False, scaled=True):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n)
    lens[rng.integers(0, n, n // 8)] = 0
    lens[rng.integers(0, n, n // 4)] = rng.integers(1, 4, n // 4)          # rows of 1 .. 3 entries
    lens[0] = lens[-1] = 0
    rp = np.zeros(n + 1, np.int64); np.cumsum(lens, out=rp[1:])
    col = rng.integers(0, n, rp[-1])
    val = rng.standard_normal(rp[-1]) + (1j * rng.standard_normal(rp[-1]) if cplx else 0)
    x = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
    if scaled:      # rows and columns over 2^-30 .. 2^30: the scale differs from row to row
        val = val * np.repeat(2.0 ** rng.uniform(-30, 30, n), lens)
        x = x * 2.0 ** rng.uniform(-30, 30, n)
    return rng, rp, col, val, x


def _serial(rp, col, val, x, order=None, fma=False):
    """Row by row, left to right (or in `order` within each row), in fp64 -- vectorised over rows by slot."""
    lens = np.diff(rp)
    y = np.zeros(len(lens), dtype=val.dtype)
    perm = np.arange(len(col)) if order is None else order
    for k in range(int(lens.max())):
        r = np.flatnonzero(lens > k)
        e = perm[rp[r] + k]
        if fma:     # an FMA-like step: the product kept exactly (Dekker's TwoProduct), added to y with one rounding of a
            #         double-double sum (TwoSum, then the rounded sum of the low parts): at most two roundings per step
            p, pe = X._two_prod(val[e], x[col[e]])
            s, se = X._two_sum(y[r], p)
            y[r] = s + (se + pe)
        else:
            y[r] = y[r] + val[e] * x[col[e]]
    return y


def _within_row_shuffle(rng, rp):
    key = np.repeat(np.arange(len(rp) - 1), np.diff(rp)) + rng.random(rp[-1])
    return np.argsort(key, kind="stable")


@pytest.mark.parametrize("cplx", [False, True])
def test_correct_orders_pass(cplx):
    rng, rp, col, val, x = _ragged(1, cplx=cplx)
    ref = X.hp_product(rp, col, val, x)
    M_y = np.zeros(len(rp) - 1, val.dtype)
    for i in range(len(rp) - 1):        # numpy's own product, row by row
        M_y[i] = val[rp[i]:rp[i + 1]] @ x[col[rp[i]:rp[i + 1]]] if rp[i + 1] > rp[i] else 0
    X.assert_rows(M_y, rp, col, val, x, ("numpy", cplx), ref=ref)
    X.assert_rows(_serial(rp, col, val, x), rp, col, val, x, ("serial", cplx), ref=ref)
    X.assert_rows(_serial(rp, col, val, x, _within_row_shuffle(rng, rp)), rp, col, val, x, ("permuted", cplx), ref=ref)
    if not cplx:
        X.assert_rows(_serial(rp, col, val, x, fma=True), rp, col, val, x, ("fma", cplx), ref=ref)


def _round_mantissa(v, bits):
    m, e = np.frexp(v)
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def _wrong_products(rng, rp, col, val, x):
    """name -> y of a subtly wrong kernel."""
    lens = np.diff(rp)
    out = {}
    out["values to 45 bits"] = _serial(rp, col, _round_mantissa(val.real, 45) + (1j * _round_mantissa(val.imag, 45) if np.iscomplexobj(val) else 0), x)
    out["x to fp32"] = _serial(rp, col, val, x.astype(np.complex64 if np.iscomplexobj(x) else np.float32).astype(x.dtype))
    e = rp[np.flatnonzero(lens >= 2)[3]] + 1        # an entry in the middle of a row of >= 2 entries (value nonzero)
    r = int(np.searchsorted(rp, e, side="right") - 1)
    v = val.copy(); v[e] = 0
    out["entry dropped"] = _serial(rp, col, v, x)
    v = val.copy(); v[e] *= 2
    out["entry doubled"] = _serial(rp, col, v, x)
    y = _serial(rp, col, val, x); y[r] -= val[e] * x[col[e]]; y[r + 1] += val[e] * x[col[e]]
    out["entry in the next row"] = y
    y = _serial(rp, col, val, x); y[np.flatnonzero(lens == 0)[1]] = np.nan
    out["row never written"] = y
    return out


@pytest.mark.parametrize("cplx", [False, True])
def test_wrong_products_fail_the_row_bound(cplx):
    rng, rp, col, val, x = _ragged(2, cplx=cplx)
    ref = X.hp_product(rp, col, val, x)
    for name, y in _wrong_products(rng, rp, col, val, x).items():
        assert len(X.bad_rows(y, rp, col, val, x, ref=ref)) > 0, name
    # the former band, 1e-12 max|ref|, passes the 45-bit values: the gap this module closes
    y = _wrong_products(rng, rp, col, val, x)["values to 45 bits"]
    yref = (ref[0].astype(np.float64) + (1j * ref[1].astype(np.float64) if cplx else 0))
    assert np.abs(y - yref).max() <= 1e-12 * np.abs(yref).max()


@pytest.mark.parametrize("cplx", [False, True])
def test_integer_exactness_catches_one_wrong_entry(cplx):
    rng, rp, col, _, _ = _ragged(3, cplx=cplx, scaled=False)
    lens = np.diff(rp)
    p = X.int_bits(lens.max(), "c128" if cplx else "f64")
    val = X.int_values(rng, rp[-1], p, cplx); x = X.int_values(rng, len(rp) - 1, p, cplx, zeros=0)
    ye = X.exact_int_product(rp, col, val, x)
    X.assert_exact(_serial(rp, col, val, x), ye, "serial")
    X.assert_exact(_serial(rp, col, val, x, _within_row_shuffle(rng, rp)), ye, "permuted")
    if not cplx:        # (the FMA emulation is real-valued)
        X.assert_exact(_serial(rp, col, val, x, fma=True), ye, "fma")
    e = int(np.flatnonzero(val != 0)[len(val) // 2])
    for name, (v, c) in {"dropped": (np.where(np.arange(len(val)) == e, 0, val), col),
                         "doubled": (np.where(np.arange(len(val)) == e, 2 * val, val), col),
                         "wrong column": (val, np.where(np.arange(len(col)) == e, (col + 1) % (len(rp) - 1), col))}.items():
        with pytest.raises(AssertionError):
            X.assert_exact(_serial(rp, c, v, x), ye, name)


def test_magnitude_rule_keeps_every_order_exact():
    """At the largest magnitudes the rule admits, sums in two orders and fp64 / fp32 (c64 rule) stay exact."""
    rng = np.random.default_rng(4)
    for L in (1, 2, 3, 64, 65, 1000):
        for kind, dt in (("f64", np.float64), ("c128", np.complex128), ("c64", np.complex64)):
            p = X.int_bits(L, kind)
            rp = np.array([0, L], np.int64); col = rng.integers(0, 4, L)
            hi = 2.0 ** p
            val = np.full(L, hi) * (1 + 1j if kind != "f64" else 1); x = np.full(4, hi) * (1 - 1j if kind != "f64" else 1)
            ye = X.exact_int_product(rp, col, val, x)
            y32 = _serial(rp, col, val.astype(dt), x.astype(dt))
            assert y32.astype(ye.dtype)[0] == ye[0], (L, kind)


def test_double_double_fallback_agrees_with_longdouble():
    for cplx in (False, True):
        _, rp, col, val, x = _ragged(5, cplx=cplx)
        ld = X.hp_product(rp, col, val, x)
        dd = X.hp_product(rp, col, val, x, force_dd=True)
        y = _serial(rp, col, val, x)
        e_ld, e_dd = X.row_errors(y, ld), X.row_errors(y, dd)
        assert np.all(np.abs(e_ld - e_dd) <= 2 * X.gamma(np.diff(rp) + 2, X.ULD) * ld[2] + 1e-300)
        assert len(X.bad_rows(y, rp, col, val, x, ref=dd)) == 0


def test_exact_int_product_refuses_data_beyond_the_rule():
    """Rows whose partial sums could leave 2^53 are refused, not summed."""
    rp = np.array([0, 3], np.int64); col = np.zeros(3, np.int64)
    with pytest.raises(AssertionError):
        X.exact_int_product(rp, col, np.full(3, 2.0 ** 26), np.full(1, 2.0 ** 26))
    assert X.exact_int_product(rp, col, np.full(3, 2.0 ** 25), np.full(1, 2.0 ** 26))[0] == 3 * 2.0 ** 51


def test_dot_bound_is_never_looser_than_the_former_band():
    for n in (1, 10, 1000, 10 ** 6, 10 ** 8):
        assert X.dot_bound(1.0, n) <= 1e-12
