"""The complex64 IC(0) checker: the fp32 incomplete Cholesky factor and its two fp32 triangular solves, restated from the math
 in complex64, not from any implementation.

IC(0) on the pattern of A's lower triangle (diagonal included, upper triangle ignored, duplicates summed), unconjugated:
    L(i,j) = (A(i,j) - sum_{k<j} L(i,k) L(j,k)) / L(j,j)      for j < i in the pattern, the sum in column order
    L(i,i) = sqrt(A(i,i) - sum_{k<i} L(i,k)^2)                 the principal root, the sum in column order
and the solves  y_i = (x_i - sum_k T(i,k) y_k) / T(i,i)  with T = L (forward) or L^T (backward), the sum in column order.

Every operation is one fp32 complex operation, in the order written above:
    product   (a.re b.re - a.im b.im, a.re b.im + a.im b.re), each part a fused multiply-add over one rounded product:
              fma(a.re, b.re, -(a.im b.im)), fma(a.re, b.im, a.im b.re)
    quotient  cuCdivf's formula, both operands scaled by |b.re| + |b.im| (c64_checker.Prec.div)
    root      the principal square root from hypot and sqrt in fp32 (std::sqrt(std::complex<float>)'s branches)
    sum       one fp32 rounding per part
A fused multiply-add is evaluated here as an exact product in fp64 plus the addend, rounded to fp64 and then to fp32: the same
as one fp32 rounding except in rare ties.  A pivot fails when it is 0 or not finite.
"""
import math

import numpy as np
import scipy.sparse as sp

import ic0_checker as IC

F32, F64 = np.float32, np.float64


def _f(x):
    return float(F32(x))


def _q(a, b):
    """a / b in fp32 with IEEE's answers for a zero or non-finite b (inf, nan) rather than Python's exception."""
    with np.errstate(all="ignore"):
        return float(F32(a) / F32(b))


# ------------------------------------------------------------------------------------------ scalars (pairs of fp32 values)
def mul(a, b):
    return (_f(a[0] * b[0] - _f(a[1] * b[1])), _f(a[0] * b[1] + _f(a[1] * b[0])))


def sub(a, b):
    return (_f(a[0] - b[0]), _f(a[1] - b[1]))


def div(a, b):
    s = _f(abs(b[0]) + abs(b[1]))
    oos = _q(1.0, s)
    ars, ais, brs, bis = _f(a[0] * oos), _f(a[1] * oos), _f(b[0] * oos), _f(b[1] * oos)
    s = _f(_f(brs * brs) + _f(bis * bis))
    oos = _q(1.0, s)
    return (_f(_f(_f(ars * brs) + _f(ais * bis)) * oos), _f(_f(_f(ais * brs) - _f(ars * bis)) * oos))


def csqrt(z):
    x, y = z
    if x == 0.0 and y == 0.0:
        return (0.0, y)
    r = float(np.hypot(F32(x), F32(y)))
    if x >= 0.0:
        t = _f(math.sqrt(_f(0.5 * _f(r + x))))
        return (t, _q(y, _f(2.0 * t)))
    t = _f(math.sqrt(_f(0.5 * _f(r - x))))
    return (_q(abs(y), _f(2.0 * t)), math.copysign(t, y))


def pivot_fails(d):
    return (d[0] == 0.0 and d[1] == 0.0) or not (math.isfinite(d[0]) and math.isfinite(d[1]))


# ------------------------------------------------------------------------------------------ factor
def ic0(n, rowptr, col, val):
    """(rowptr, col, val, zero_pivot) of the fp32 L: rows sorted, diagonal last, complex64 values; zero_pivot = smallest failing
    row or -1.  Duplicates are summed in complex64 in the order given."""
    rows = IC.lower_rows(n, np.asarray(rowptr), np.asarray(col), np.asarray(val, np.complex64))
    Lc, Lv = [], []
    zp = -1
    for i in range(n):
        cols = sorted(rows[i])
        vals = [(float(rows[i][c].real), float(rows[i][c].imag)) for c in cols]
        pos = {c: q for q, c in enumerate(cols)}
        for q in range(len(cols) - 1):
            j = cols[q]
            s = vals[q]
            cj, vj = Lc[j], Lv[j]
            for k, ljk in zip(cj[:-1], vj[:-1]):        # k < j, ascending: the sum in column order
                r = pos.get(k)
                if r is not None and r < q:
                    s = sub(s, mul(vals[r], ljk))
            vals[q] = div(s, vj[-1])
        d = vals[-1]
        for q in range(len(cols) - 1):
            d = sub(d, mul(vals[q], vals[q]))
        if pivot_fails(d) and zp < 0:
            zp = i
        vals[-1] = csqrt(d)
        Lc.append(cols)
        Lv.append(vals)
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in Lc])
    cc = np.fromiter((c for r in Lc for c in r), np.int64, int(rp[-1]))
    vv = np.array([complex(*v) for r in Lv for v in r], np.complex64)
    return rp, cc, vv, zp


def dense_cholesky_unconjugated(A):
    """L with A = L L^T (unconjugated, principal roots) of a dense complex matrix, in complex128: the exact factor that IC(0)
    equals where the lower triangle has no fill outside its pattern (tridiagonal, full band)."""
    A = np.array(A, np.complex128)
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


# ------------------------------------------------------------------------------------------ vectorised fp32 parts
def _vmul(ar, ai, br, bi):
    re = (ar.astype(F64) * br - (ai * bi).astype(F64)).astype(F32)
    im = (ar.astype(F64) * bi + (ai * br).astype(F64)).astype(F32)
    return re, im


def _vdiv(ar, ai, br, bi):
    s = np.abs(br) + np.abs(bi)
    oos = F32(1.0) / s
    ars, ais, brs, bis = ar * oos, ai * oos, br * oos, bi * oos
    s = brs * brs + bis * bis
    oos = F32(1.0) / s
    return (ars * brs + ais * bis) * oos, (ais * brs - ars * bis) * oos


class Ic64Apply:
    """y = L^-1 x (which 0), L^-T x (1) or (L.L^T)^-1 x (2) in fp32, every row in column order: rows of one level at a time
    (a level's rows read only earlier levels), all of a level's rows advanced one entry at a time."""

    def __init__(self, n, rowptr, col, val):
        self.n = n
        L = sp.csr_matrix((np.asarray(val, np.complex64), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
        L.sort_indices()
        LT = L.T.tocsr()
        LT.sort_indices()
        fw, bw = IC.levels(n, L.indptr, L.indices)
        self.tri = [self._prep(L, fw, False), self._prep(LT, bw, True)]

    @staticmethod
    def _prep(T, level, up):
        rp = T.indptr.astype(np.int64)
        order = np.argsort(level, kind="stable")
        bounds = np.searchsorted(level[order], np.arange(int(level.max()) + 2))
        return {"rp": rp, "col": T.indices.astype(np.int64), "re": T.data.real.astype(F32), "im": T.data.imag.astype(F32),
                "levels": [order[bounds[l]:bounds[l + 1]] for l in range(len(bounds) - 1)], "up": up}

    @staticmethod
    def _solve(t, x):
        xr, xi = np.real(x).astype(F32), np.imag(x).astype(F32)
        yr, yi = np.zeros_like(xr), np.zeros_like(xi)
        rp, col, vr, vi, up = t["rp"], t["col"], t["re"], t["im"], t["up"]
        for rows in t["levels"]:
            s, e = rp[rows], rp[rows + 1]
            b = s + 1 if up else s                       # off-diagonal entries [b, f), the diagonal at s (L^T) or e - 1 (L)
            f = e if up else e - 1
            dg = s if up else e - 1
            ar, ai = xr[rows].copy(), xi[rows].copy()
            for q in range(int((f - b).max()) if len(rows) else 0):
                m = q < f - b
                p = np.where(m, b + q, dg)
                pr, pi = _vmul(vr[p], vi[p], yr[col[p]], yi[col[p]])
                ar = np.where(m, ar - pr, ar)
                ai = np.where(m, ai - pi, ai)
            yr[rows], yi[rows] = _vdiv(ar, ai, vr[dg], vi[dg])
        return (yr.astype(np.complex64) + 1j * yi.astype(np.complex64)).astype(np.complex64)

    def solve(self, x, which=2):
        with np.errstate(all="ignore"):
            if which == 0:
                return self._solve(self.tri[0], x)
            if which == 1:
                return self._solve(self.tri[1], x)
            return self._solve(self.tri[1], self._solve(self.tri[0], x))

    def mx(self, x):
        """c64_checker.pcg's preconditioner: z = (L.L^T)^-1 r."""
        return self.solve(np.asarray(x, np.complex64), 2)


def c128_apply(n, rowptr, col, val):
    """The same preconditioner in complex128 (ic0_checker's factor of the complex64 values, SciPy's solves): the twin run that
    c64_checker's tolerance rule compares against."""
    rp, cc, vv, _ = IC.ic0(n, rowptr, col, np.asarray(val, np.complex64).astype(np.complex128))
    ap = IC.IcApply(IC.to_sparse(n, rp, cc, vv))
    return lambda x: ap.solve(np.asarray(x, np.complex128), 2)
