"""The IC(0) checker: incomplete Cholesky with zero fill and the PCG loops it preconditions, restated in NumPy / SciPy from
the math, not from any implementation.

IC(0) on the pattern of A's lower triangle (diagonal included, upper triangle ignored, duplicates summed):
    L(i,j) = (A(i,j) - sum_{k<j} L(i,k) L(j,k)) / L(j,j)      for j < i in the pattern, k over both rows' patterns
    L(i,i) = sqrt(A(i,i) - sum_{k<i} L(i,k)^2)
unconjugated for complex A, with the principal square root.
"""
import cmath
import math

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve_triangular


def lower_rows(n, rowptr, col, val):
    """Per row: {column: summed value} of the entries on or below the diagonal; the diagonal always present."""
    rows = []
    zero = val.dtype.type(0)
    for i in range(n):
        d = {i: zero}
        for p in range(rowptr[i], rowptr[i + 1]):
            j = int(col[p])
            if j <= i:
                d[j] = d.get(j, zero) + val[p]
        rows.append(d)
    return rows


def ic0(n, rowptr, col, val):
    """(rowptr, col, val, zero_pivot) of L: rows sorted, diagonal last; zero_pivot = smallest failing row or -1."""
    cplx = np.iscomplexobj(val)
    rows = lower_rows(n, np.asarray(rowptr), np.asarray(col), np.asarray(val))
    Lc, Lv = [], []
    zp = -1
    for i in range(n):
        cols = sorted(rows[i])
        vals = [rows[i][c] for c in cols]
        pos = {c: q for q, c in enumerate(cols)}
        for q in range(len(cols) - 1):
            j = cols[q]
            s = vals[q]
            cj, vj = Lc[j], Lv[j]
            for k, ljk in zip(cj[:-1], vj[:-1]):        # k < j, ascending: the sum in column order
                r = pos.get(k)
                if r is not None and r < q:
                    s = s - vals[r] * ljk
            vals[q] = s / vj[-1]
        d = vals[-1]
        for q in range(len(cols) - 1):
            d = d - vals[q] * vals[q]
        if cplx:
            bad = d == 0 or not (math.isfinite(d.real) and math.isfinite(d.imag))
            vals[-1] = cmath.sqrt(d)
        else:
            bad = not (d > 0) or not math.isfinite(d)
            vals[-1] = math.sqrt(d) if d >= 0 else float("nan")
        if bad and zp < 0:
            zp = i
        Lc.append(cols)
        Lv.append(vals)
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in Lc])
    cc = np.fromiter((c for r in Lc for c in r), np.int64, int(rp[-1]))
    vv = np.array([v for r in Lv for v in r], np.complex128 if cplx else np.float64)
    return rp, cc, vv, zp


def to_sparse(n, rowptr, col, val):
    return sp.csr_matrix((np.asarray(val), np.asarray(col), np.asarray(rowptr)), shape=(n, n))


class IcApply:
    """z = (L.L^T)^-1 x with SciPy's triangular solves (unconjugated transpose)."""

    def __init__(self, L):
        self.L = sp.csr_matrix(L)
        self.LT = sp.csr_matrix(L.T)

    def solve(self, x, which=2):
        if which == 0:
            return spsolve_triangular(self.L, x, lower=True)
        if which == 1:
            return spsolve_triangular(self.LT, x, lower=False)
        return spsolve_triangular(self.LT, spsolve_triangular(self.L, x, lower=True), lower=False)


def lpcg(A, M, b, eps, abs_diff, max_iterations=0, m0=None):
    """lcg's preconditioned CG: residual = sqrt(r.r)/n with abs_diff, else r.r / max(m.m, 1); returns (m, iterations)."""
    n = len(b)
    m = np.zeros(n) if m0 is None else np.array(m0, float)
    r = b - A @ m
    z = M(r)
    d = z.copy()
    m2 = max(m @ m, 1.0)
    r2 = r @ r
    zr = z @ r

    def res():
        return math.sqrt(r2) / n if abs_diff else r2 / m2

    t = 0
    if res() <= eps:
        return m, 0
    while True:
        if res() <= eps or (max_iterations > 0 and t + 1 > max_iterations):
            return m, t
        t += 1
        Ad = A @ d
        ak = zr / (d @ Ad)
        m = m + ak * d
        r = r - ak * Ad
        z = M(r)
        m2 = max(m @ m, 1.0)
        r2 = r @ r
        zrn = z @ r
        bk = zrn / zr
        zr = zrn
        d = z + bk * d


def clpcg(A, M, b, eps, abs_diff, max_iterations=0):
    """clcg's preconditioned CG (complex-symmetric A): unconjugated r.z and d.Ad, residual from <r, r>."""
    n = len(b)
    m = np.zeros(n, np.complex128)
    r = b - A @ m
    d = M(r)
    dn = r @ d
    r2 = np.vdot(r, r).real
    m2 = 1.0

    def res():
        return math.sqrt(r2) / n if abs_diff else r2 / m2

    t = 0
    if res() <= eps:
        return m, 0
    while True:
        if res() <= eps or (max_iterations > 0 and t + 1 > max_iterations):
            return m, t
        t += 1
        Ax = A @ d
        ak = dn / (d @ Ax)
        m = m + ak * d
        r = r - ak * Ax
        if not abs_diff:
            m2 = max(np.vdot(m, m).real, 1.0)
        r2 = np.vdot(r, r).real
        s = M(r)
        dold = dn
        dn = r @ s
        d = (dn / dold) * d + s
