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


def levels(n, rowptr, col):
    """(forward, backward) level of every row of L, L = the lower triangle of the pattern (diagonal excluded as a dependency).
    Forward: row i reads y_j for every j < i in its row, so level(i) = 1 + max level(j), 0 with no such j.  Backward (L^T): row j
    reads y_i for every i > j with L(i,j) in the pattern, so level(j) = 1 + max level(i) over those i."""
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    reads = [sorted({int(c) for c in col[rowptr[i]:rowptr[i + 1]] if c < i}) for i in range(n)]
    read_by = [[] for _ in range(n)]
    for i in range(n):
        for j in reads[i]:
            read_by[j].append(i)
    fw = np.zeros(n, np.int64)
    for i in range(n):                                  # every row read comes first in this order
        fw[i] = 1 + max((fw[j] for j in reads[i]), default=-1)
    bw = np.zeros(n, np.int64)
    for j in range(n - 1, -1, -1):
        bw[j] = 1 + max((bw[i] for i in read_by[j]), default=-1)
    return fw, bw


def widths(level):
    """Rows per level."""
    return np.bincount(np.asarray(level), minlength=int(np.max(level)) + 1 if len(level) else 0)


def segments(widths, max_merged):
    """Launches for one triangle: every level wider than max_merged rows alone, every maximal run of consecutive
    levels of at most max_merged rows together."""
    count, in_run = 0, False
    for w in widths:
        if w > max_merged:
            count += 1
            in_run = False
        elif not in_run:
            count += 1
            in_run = True
    return count


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


def lpcg(A, M, b, eps, abs_diff, max_iterations=0, m0=None, snap=None):
    """lcg's preconditioned CG: residual = sqrt(r.r)/n with abs_diff, else r.r / max(m.m, 1); returns (m, iterations).
    snap: a dict whose keys are iteration counts; the iterate after that many iterations is stored under each."""
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
        if snap is not None and t in snap:
            snap[t] = m.copy()
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


def clpbicg(A, M, b, eps, abs_diff, max_iterations=0):
    """clcg's preconditioned BiCG with a user M (Eigen back-end): a.dot(b) = sum conj(a_i) b_i, stop rule on 4th powers
    (r4 = |<r,r>|^2, m4 = max(|<m,m>|^2, 1); abs_diff: sqrt(r4) / n), the second product conj(A).ps, and the shadow residual
    rebuilt as conj(r_old) - conj(ak) conj(A).ps every iteration.  Returns (m, iterations)."""
    n = len(b)
    Ac = A.conj()
    m = np.zeros(n, np.complex128)
    r = b - A @ m
    z = M(r)
    pk, rs, ps = z.copy(), r.conj(), z.conj()
    rho = np.vdot(rs, z)
    m4 = max(abs(np.vdot(m, m)) ** 2, 1.0)
    r4 = abs(np.vdot(r, r)) ** 2
    if (abs_diff and math.sqrt(r4) / n <= eps) or r4 / m4 <= eps:
        return m, 0
    t = 0
    while True:
        res = math.sqrt(r4) / n if abs_diff else r4 / m4
        if res <= eps or (max_iterations > 0 and t + 1 > max_iterations):
            return m, t
        t += 1
        Ax = A @ pk
        Asx = Ac @ ps
        ak = rho / np.vdot(ps, Ax)
        m = m + ak * pk
        rs = r.conj() - np.conj(ak) * Asx
        r = r - ak * Ax
        m4 = max(abs(np.vdot(m, m)) ** 2, 1.0)
        r4 = abs(np.vdot(r, r)) ** 2
        z = M(r)
        rho2 = np.vdot(rs, z)
        bk = rho2 / rho
        rho = rho2
        pk = z + bk * pk
        ps = z.conj() + np.conj(bk) * ps


# ------------------------------------------------------------------------------------------ test matrices
def laplace3d(k):
    """The 7-point Laplacian on a k^3 grid, rows sorted: forward level of (x, y, z) is x + y + z."""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(k, k))
    I = sp.identity(k)
    A = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def assemble(n, lower, diag, upper=True):
    """CSR (rows sorted) of the symmetric matrix with strictly lower entries lower[i] = {j: value} and diagonal diag; upper=False:
    the lower triangle alone."""
    rows = [dict(lower[i]) for i in range(n)]
    for i in range(n):
        rows[i][i] = diag[i]
    if upper:
        for i in range(n):
            for j, x in lower[i].items():
                rows[j][i] = x
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    cols = [sorted(r) for r in rows]
    ci = np.fromiter((c for cs in cols for c in cs), np.int32, int(rp[-1]))
    v = np.array([rows[i][c] for i in range(n) for c in cols[i]], np.complex128 if np.iscomplexobj(diag) else np.float64)
    return rp, ci, v


def _offdiag(rng, cplx):
    return rng.uniform(-1.0, 1.0) + (1j * rng.uniform(-1.0, 1.0) if cplx else 0.0)


def dominant_diagonal(rng, n, lower, cplx):
    """1 + U(0, 1) + the row's off-diagonal magnitudes (both triangles), complex: plus i U(-0.5, 0.5): strictly diagonally
    dominant, so SPD (real) and every IC(0) pivot usable."""
    s = np.zeros(n)
    for i in range(n):
        for j, x in lower[i].items():
            s[i] += abs(x); s[j] += abs(x)
    d = 1.0 + rng.uniform(0.0, 1.0, n) + s
    return d + 1j * rng.uniform(-0.5, 0.5, n) if cplx else d


def layered_parts(widths, seed, cplx=False):
    """(lower, diag, starts) of a matrix whose forward levels are exactly the layers of the given widths: layer t is rows
    starts[t] .. starts[t+1]-1; each of its rows reads 1-3 rows of layer t-1 and, one time in three, one row of an earlier layer."""
    rng = np.random.default_rng(seed)
    starts = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    n = int(starts[-1])
    lower = [{} for _ in range(n)]
    for t in range(1, len(widths)):
        a, b = int(starts[t - 1]), int(starts[t])
        for i in range(b, int(starts[t + 1])):
            for j in rng.integers(a, b, size=int(rng.integers(1, 4))):
                lower[i][int(j)] = _offdiag(rng, cplx)
            if t >= 2 and rng.uniform() < 1.0 / 3.0:
                lower[i][int(rng.integers(0, a))] = _offdiag(rng, cplx)
    return lower, dominant_diagonal(rng, n, lower, cplx), starts


def layered(widths, seed, cplx=False):
    """(rowptr, col, val) of the layered matrix (layered_parts), both triangles stored, rows sorted."""
    lower, diag, _ = layered_parts(widths, seed, cplx)
    return assemble(len(diag), lower, diag)


def random_spd(n, seed):
    """SPD, strictly diagonally dominant, on a random lower pattern: row i reads 0-3 rows, mostly near it, sometimes far back,
    so its level sets are irregular: wide ones near the top, long runs of narrow ones later."""
    rng = np.random.default_rng(seed)
    lower = [{} for _ in range(n)]
    for i in range(1, n):
        for _ in range(int(rng.integers(0, 4))):
            j = i - 1 - int(rng.geometric(0.002)) if rng.uniform() < 0.7 else int(rng.integers(0, i))
            if j >= 0:
                lower[i][j] = _offdiag(rng, False)
    return assemble(n, lower, dominant_diagonal(rng, n, lower, False))


def shuffle_split(rowptr, col, val, seed, split=0.4):
    """The same matrix with every row's entries in random order and some entries split into two that sum to it."""
    rng = np.random.default_rng(seed)
    nrp, nc, nv = [0], [], []
    for i in range(len(rowptr) - 1):
        c, x = list(col[rowptr[i]:rowptr[i + 1]]), list(val[rowptr[i]:rowptr[i + 1]])
        for q in range(len(c)):
            if rng.uniform() < split:
                c.append(c[q]); x.append(0.25 * x[q]); x[q] = 0.75 * x[q]
        order = rng.permutation(len(c))
        nc += [c[q] for q in order]; nv += [x[q] for q in order]
        nrp.append(len(nc))
    return np.array(nrp, np.int32), np.array(nc, np.int32), np.array(nv, np.asarray(val).dtype)
