"""Reference products for the A.x kernels that are exact or nearly so, and per-row rounding bounds that any correct
kernel meets -- a helper of the tests (like c64_checker.py), not a conftest.

Two references:

* Integer data (``int_bits`` picks the magnitudes): products in int64, real and imaginary parts apart, summed per row.
  With |a|, |x| <= 2^p and 2p + ceil(log2 L) <= B (L = the longest row, or 2L terms per component for complex values),
  every product and every partial sum, in any order and any tree, is an integer of at most B bits, so fp64 (B = 52;
  c128: the same with 2L terms, one bit fewer) and fp32 (B = 23 for complex64) represent it exactly.  A correct kernel's
  y then equals the exact sum BIT FOR BIT, whatever its summation order, FMA contraction or split.

* Full-mantissa data: products and row sums in extended precision (np.longdouble when it has a 64-bit significand,
  otherwise double-double by Dekker's split and Knuth's TwoSum).  Its own error, at most gamma_ld(L + 1) (|A||x|)_i for
  real rows and gamma_ld(2L + 1) for complex ones (u_ld = 2^-64), is added to every bound.

The bounds (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1 and the summation analysis of
section 4.2).  With u = 2^-53 and gamma(m) = m u / (1 - m u), a sum of L rounded products evaluated in ANY order (any
tree, any split into partial sums that are added later) has |y_hat - y| <= gamma(L) sum |a_k x_k|: every term passes
through at most L roundings (its product, then at most L - 1 additions on its way to the root).  FMA contraction only
removes roundings.  A kernel may add a few more operations on the way: the initial zero it starts from, the `y +=` of
a windowed kernel that adds window partials, the combine of a row range or of a row shard's local and remote parts;
four extra roundings cover them:

    fp64:  |y_hat_i - y_i| <= gamma(L_i + 4) (|A||x|)_i
    c128:  |y_hat_i - y_i| <= sqrt(2) gamma(2 L_i + 4) (|A||x|)_i

(c128: each component is a real sum of 2 L_i products whose magnitudes sum to at most |a||x| by Cauchy-Schwarz, and the
modulus of the two components' errors adds sqrt(2).)  complex64 keeps tests/test_gpu_c64.py's derivation,
3 (L_i + 5) 2^-24 (|A||x|)_i.

Dot epilogues (lcg_hip_spmv_dot: y.u and y.y), checked against the extended-precision dot of the kernel's own y.  Whatever
the reduction's shape, a sum of n rounded products meets at most n + 1 roundings per term, so

    |s_hat - s| <= gamma(n + 1) sum |y_i u_i|

for any order.  No tighter depth is derived from the kernels' reduction trees here, so above about 9,000 terms this is no
tighter than the suite's former band 1e-12 sum |y_i u_i|; ``dot_bound`` takes the smaller of the two, so no check gets
looser.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -53
U32 = 2.0 ** -24
ULD = 2.0 ** -64


def gamma(m, u=U):
    m = np.asarray(m, dtype=np.float64)
    return m * u / (1.0 - m * u)


def lengths(rp):
    return np.diff(np.asarray(rp, np.int64))


# ------------------------------------------------------------------------------------------------ row sums
def _row_sum(terms, rp):
    """Per-row sums of `terms` (entry order) with empty rows 0: np.add.reduceat over the non-empty rows' starts."""
    rp = np.asarray(rp, np.int64)
    n = len(rp) - 1
    out = np.zeros(n, dtype=terms.dtype)
    ne = np.flatnonzero(rp[1:] > rp[:-1])
    if len(ne):
        out[ne] = np.add.reduceat(terms, rp[:-1][ne])
    return out


def int_bits(max_len, kind="f64"):
    """Largest p such that |a|, |x| <= 2^p keeps every partial sum of a row of max_len entries exact (module docstring)."""
    B = {"f64": 52, "c128": 51, "c64": 23}[kind]
    terms = max(1, int(max_len)) * (2 if kind != "f64" else 1)
    p = (B - math.ceil(math.log2(terms))) // 2
    assert p >= 1, (max_len, kind)
    return p


def int_values(rng, size, p, cplx=False, zeros=0.1):
    """Integers in [-2^p, 2^p] as float64 / complex128, with a share of explicit zeros."""
    hi = 2 ** p
    v = rng.integers(-hi, hi + 1, size).astype(np.float64)
    if cplx:
        v = v + 1j * rng.integers(-hi, hi + 1, size).astype(np.float64)
    if zeros:
        v[rng.random(size) < zeros] = 0
    return v


def exact_int_product(rp, col, val, x):
    """y = A.x exactly for integer-valued val / x (float64 or complex128), as float64 / complex128.  Raises if the data break
    the magnitude rule (a sum would not be exactly representable)."""
    col = np.asarray(col, np.int64)
    cplx = np.iscomplexobj(val) or np.iscomplexobj(x)
    val = np.asarray(val); x = np.asarray(x)

    def as_int(a):
        r = np.asarray(a).astype(np.float64)
        assert np.all(r == np.round(r)) and np.all(np.abs(r) < 2.0 ** 62), "exact_int_product needs integer data"
        return r.astype(np.int64)

    # every partial sum, in any order and tree, is at most the row's sum of |terms|: that must stay within 2^53
    lim = "exact_int_product: data beyond the magnitude rule (a partial sum may round)"
    if not cplx:
        a, xx = as_int(val), as_int(x)[col]
        assert np.all(np.abs(a) < 2 ** 31) and np.all(np.abs(xx) < 2 ** 31), lim
        assert np.all(_row_sum(np.abs(a * xx), rp) <= 2 ** 53), lim
        return _row_sum(a * xx, rp).astype(np.float64)
    ar, ai = as_int(np.real(val)), as_int(np.imag(val))
    xr, xi = as_int(np.real(x))[col], as_int(np.imag(x))[col]
    assert all(np.all(np.abs(t) < 2 ** 31) for t in (ar, ai, xr, xi)), lim
    assert np.all(_row_sum(np.abs(ar * xr) + np.abs(ai * xi), rp) <= 2 ** 53), lim
    assert np.all(_row_sum(np.abs(ar * xi) + np.abs(ai * xr), rp) <= 2 ** 53), lim
    yr = _row_sum(ar * xr - ai * xi, rp); yi = _row_sum(ar * xi + ai * xr, rp)
    return yr.astype(np.float64) + 1j * yi.astype(np.float64)


# ------------------------------------------------------------------------------------------------ extended precision
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a          # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a); bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_row_sum(terms_hi, terms_lo, rp):
    """Double-double row sums of (hi, lo) terms, slot by slot across rows (vectorised over rows)."""
    rp = np.asarray(rp, np.int64)
    lens = np.diff(rp)
    s = np.zeros(len(lens)); e = np.zeros(len(lens))
    for k in range(int(lens.max()) if len(lens) else 0):
        r = np.flatnonzero(lens > k)
        idx = rp[r] + k
        t, err = _two_sum(s[r], terms_hi[idx])
        err = err + e[r] + terms_lo[idx]
        s[r], e[r] = _two_sum(t, err)
    return s, e


def _real_terms_dd(a_parts, x_parts, signs):
    """hi / lo parts of sum(sign * a * x) over the given (a, x) pairs, entry by entry."""
    hi = np.zeros(len(a_parts[0])); lo = np.zeros(len(a_parts[0]))
    for a, xx, sg in zip(a_parts, x_parts, signs):
        p, pe = _two_prod(a, xx)
        hi, e = _two_sum(hi, sg * p)
        lo = lo + e + sg * pe
    return hi, lo


def hp_product(rp, col, val, x, force_dd=False):
    """A.x in extended precision: (y as np.longdouble / pair of longdouble for complex, when available; otherwise the double-double
    (hi + lo) rounded to the nearest float64 pair), together with |A||x| as float64 rounded up.  Return (y_re, y_im or None, absax).
    y_re / y_im are float64-convertible arrays whose own error is below gamma_ld(len + 1) (or gamma_ld(2 len + 1)) |A||x|."""
    col = np.asarray(col, np.int64)
    cplx = np.iscomplexobj(val) or np.iscomplexobj(x)
    val = np.asarray(val, np.complex128 if cplx else np.float64); x = np.asarray(x, np.complex128 if cplx else np.float64)
    absax = _row_sum(np.abs(val) * np.abs(x)[col], rp) * (1 + 4 * U * (lengths(rp) + 2))
    if LONGDOUBLE_OK and not force_dd:
        L = np.longdouble
        if not cplx:
            return _row_sum(val.astype(L) * x.astype(L)[col], rp), None, absax
        ar, ai = val.real.astype(L), val.imag.astype(L)
        xr, xi = x.real.astype(L)[col], x.imag.astype(L)[col]
        return _row_sum(ar * xr - ai * xi, rp), _row_sum(ar * xi + ai * xr, rp), absax
    # double-double fallback: never silently fp64
    if not cplx:
        h, lo = _real_terms_dd([val], [x[col]], [1.0])
        s, e = _dd_row_sum(h, lo, rp)
        return _DD(s, e), None, absax
    ar, ai, xr, xi = val.real, val.imag, x.real[col], x.imag[col]
    s1, e1 = _dd_row_sum(*_real_terms_dd([ar, ai], [xr, xi], [1.0, -1.0]), rp)
    s2, e2 = _dd_row_sum(*_real_terms_dd([ar, ai], [xi, xr], [1.0, 1.0]), rp)
    return _DD(s1, e1), _DD(s2, e2), absax


class _DD:
    """A double-double vector: difference against float64 data is computed as (y - hi) - lo."""
    def __init__(self, hi, lo):
        self.hi, self.lo = hi, lo

    def diff(self, y):
        return (np.asarray(y, np.float64) - self.hi) - self.lo


def _diff(ref, y):
    if isinstance(ref, _DD):
        return ref.diff(y)
    return (np.asarray(y).astype(np.longdouble) - ref).astype(np.float64)


def row_errors(y, ref):
    """|y - ref| per row (float64); NaN / Inf in y give NaN / Inf (which fail every bound)."""
    ref_re, ref_im, _ = ref
    y = np.asarray(y)
    if ref_im is None:
        return np.abs(_diff(ref_re, y.real if np.iscomplexobj(y) else y))
    return np.hypot(_diff(ref_re, y.real), _diff(ref_im, y.imag))


# ------------------------------------------------------------------------------------------------ bounds
def bound_f64(lens, absax):
    lens = np.asarray(lens, np.float64)
    return gamma(lens + 4) * absax + gamma(lens + 1, ULD) * absax + 1e-300


def bound_c128(lens, absax):
    lens = np.asarray(lens, np.float64)
    return math.sqrt(2.0) * gamma(2 * lens + 4) * absax + gamma(2 * lens + 1, ULD) * absax + 1e-300


def bound_c64(lens, absax):
    return 3.0 * (np.asarray(lens, np.float64) + 5) * U32 * absax + 1e-30


def select_rows(rp, col, val, rows):
    """The CSR arrays of the rows `rows` alone (in that order; the columns stay what they are): rowptr from 0, col, val."""
    rp = np.asarray(rp, np.int64); rows = np.asarray(rows, np.int64)
    lens = rp[rows + 1] - rp[rows]
    srp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.repeat(rp[rows] - srp[:-1], lens) + np.arange(srp[-1])
    return srp, np.asarray(col)[idx], np.asarray(val)[idx]


def bad_rows(y, rp, col, val, x, ref=None, lens=None, rows=None):
    """Rows of y outside the per-row bound of the value type (fp64 or c128) against the extended-precision reference.
    lens: terms per row when they are not the CSR row lengths (COO duplicates, a transposed product).
    rows: check these rows only (y stays the whole product) -- each against the same reference sum, in the same entry order, and
    the same bound as the full call gives it; a ref / lens passed with it belong to the selection."""
    if rows is not None:
        rows = np.asarray(rows, np.int64)
        srp, scol, sval = select_rows(rp, col, val, rows)
        return rows[bad_rows(np.asarray(y)[rows], srp, scol, sval, x, ref=ref, lens=lens)]
    ref = hp_product(rp, col, val, x) if ref is None else ref
    lens = lengths(rp) if lens is None else lens
    cplx = ref[1] is not None
    b = (bound_c128 if cplx else bound_f64)(lens, ref[2])
    err = row_errors(y, ref)
    return np.flatnonzero(~(err <= b))


def assert_rows(y, rp, col, val, x, tag=(), lens=None, ref=None, rows=None):
    if rows is not None:
        rows = np.asarray(rows, np.int64)
        srp, scol, sval = select_rows(rp, col, val, rows)
        return assert_rows(np.asarray(y)[rows], srp, scol, sval, x, tuple(tag) + ("selected rows",), lens=lens, ref=ref)
    bad = bad_rows(y, rp, col, val, x, ref=ref, lens=lens)
    if len(bad):
        ref = hp_product(rp, col, val, x) if ref is None else ref
        i = bad[:5]
        err = row_errors(np.asarray(y)[i], (ref[0][i], None if ref[1] is None else ref[1][i], ref[2][i])) if not isinstance(ref[0], _DD) else None
        raise AssertionError(f"{tag}: {len(bad)} rows outside the per-row bound, first {i.tolist()} err {err} |A||x| {ref[2][i]}")


def assert_exact(y, y_exact, tag=()):
    """Bit-for-bit equality (NaN never equal)."""
    y = np.asarray(y)
    same = y.view(np.uint8).reshape(len(y), -1) == np.asarray(y_exact, y.dtype).view(np.uint8).reshape(len(y), -1)
    bad = np.flatnonzero(~same.all(axis=1))
    assert not len(bad), f"{tag}: {len(bad)} rows differ from the exact sum, first {bad[:5].tolist()}: {y[bad[:5]]} vs {np.asarray(y_exact)[bad[:5]]}"


def dot_bound(abs_sum, n):
    """Bound of a dot of n products against its exact value (module docstring); never looser than 1e-12 abs_sum."""
    return min(float(gamma(n + 1)), 1e-12) * abs_sum + 1e-300


def assert_dot(s, a, b, tag=()):
    """A device dot s = a.b (a: the kernel's own y) within dot_bound of the extended-precision sum."""
    exact, absum = hp_dot(a, b)
    assert abs(s - exact) <= dot_bound(absum, len(a)), (tag, s, exact, absum)


def check_row_windows(y, x, n, fetch, tag=(), count=50, width=4096):
    """Per-row bound on windows of `width` rows (at least 200k rows in all, or every row): the first and last rows and `count`
    windows spread over the matrix, each starting 2048 rows before a multiple of 2048 -- so each holds the edges of 64-row blocks,
    1024-row tile chunks and 2048-row range chunks.  fetch(a, b) -> (rowptr from 0, col, val) of rows [a, b)."""
    starts = {0, max(0, n - width)}
    starts |= {max(0, min(n - width, (k * n // count) // 2048 * 2048 - 2048)) for k in range(1, count)}
    seen = np.zeros(n, bool)
    for a in sorted(starts):
        b = min(n, a + width)
        rp, col, val = fetch(a, b)
        assert_rows(np.asarray(y[a:b]), rp, col, val, x, tuple(tag) + (a,))
        seen[a:b] = True
    assert seen.sum() >= min(n, 200_000), (tag, int(seen.sum()))


def hp_dot(a, b):
    """sum(a * b) in extended precision (float64 result) and sum |a b|."""
    if LONGDOUBLE_OK:
        s = float(np.sum(np.asarray(a, np.longdouble) * np.asarray(b, np.longdouble)))
    else:
        h, lo = _real_terms_dd([np.asarray(a, np.float64)], [np.asarray(b, np.float64)], [1.0])
        s = float(np.sum(h) + np.sum(lo))
    return s, float(np.abs(a) @ np.abs(b))
