"""The ILU(0) checker: incomplete LU with zero fill, its two triangular solves, the sweep apply and the right-preconditioned
BiCGStab run, restated in NumPy / SciPy from the math, not from any implementation.

ILU(0) on the pattern of A (every entry, duplicates summed, one explicit zero on every diagonal), unconjugated for complex A:
    w(i,j) = A(i,j) - sum_{k < min(i,j)} L(i,k) U(k,j)     k ascending over the columns of row i that rows k hold column j for,
                                                           one accumulator, one product subtracted at a time
    U(i,j) = w(i,j)             j >= i
    L(i,j) = w(i,j) / U(j,j)    j < i,     L(i,i) = 1 (not stored)
A pivot fails when U(i,i) is 0 or not finite (a negative real pivot is fine).

The defining property and its rounding bound (`residual_check`).  Every entry is c - sum of t products, for L followed by one
division: by Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 8.4 (the analysis behind Theorem 9.3, LU
factorisation), evaluated in any order,
    | A(i,j) - sum_{k <= min(i,j)} L(i,k) U(k,j) |  <=  gamma(t + 1) (|L| |U|)(i,j),      gamma(m) = m u / (1 - m u)
with t the number of products with k < min(i,j) and L(i,i) = 1 (t = 0 and j >= i: U(i,j) = A(i,j), exactly).  Where the
input holds an entry d times, the build's sum of them adds gamma(d - 1) sum |a_p| (Higham, section 4.2).  Real: u = 2^-53.  Complex: every real rounding error delta
becomes a complex one of a larger modulus; the model fl(x op y) = (x op y)(1 + delta) and with it the lemma carry over with u
replaced by the largest such modulus (Higham, section 3.6):
    addition, subtraction:  |delta| <= u
    multiplication:         |delta| <= sqrt(2) gamma(2)                                   (Higham, Lemma 3.5)
    division a / b by the scaled formula (r = b.y / b.x, d = b.x + b.y r, ((a.x + a.y r) / d, (a.y - a.x r) / d) for
    |b.x| >= |b.y|, mirrored otherwise): r has one rounding; d adds two terms of one sign, relative error gamma(3), and
    |d| = |b|^2 / |b.x| >= |b|; a numerator has absolute error gamma(3) (|a.x| + |a.y|) <= sqrt(2) gamma(3) |a|; the quotient
    adds d's gamma(3) and one rounding: each component is off by at most sqrt(2) gamma(7) |a| / |b|, the pair's modulus by
    at most 2 gamma(7) |a / b|.
So u_c = 2 gamma(7) = 14 u / (1 - 7 u) covers all three.  Fused multiply-adds only remove roundings.  The product L.U is
evaluated here in rational arithmetic (fractions.Fraction: exact), so the reference adds nothing to the bound.
"""
import math
from fractions import Fraction

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve_triangular

import ic0_checker as IC
import ic0_sweeps_checker as S
from ic0_checker import clpbicg, clpcg, lpcg        # noqa: F401  (the loops ILU(0) preconditions: imported, not copied)

U64 = 2.0 ** -53
UC = 14.0 * U64 / (1.0 - 7.0 * U64)


def gamma(m, u):
    m = np.asarray(m, np.float64)
    return m * u / (1.0 - m * u)


# ------------------------------------------------------------------------------------------ the factor
def full_rows(n, rowptr, col, val):
    """Per row: {column: summed value} of every entry; the diagonal always present."""
    rows = []
    zero = np.asarray(val).dtype.type(0)
    for i in range(n):
        d = {i: zero}
        for p in range(rowptr[i], rowptr[i + 1]):
            j = int(col[p])
            d[j] = d.get(j, zero) + val[p]
        rows.append(d)
    return rows


def _csr(rows_c, rows_v, cplx):
    n = len(rows_c)
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in rows_c])
    cc = np.fromiter((c for r in rows_c for c in r), np.int64, int(rp[-1]))
    vv = np.array([v for r in rows_v for v in r], np.complex128 if cplx else np.float64)
    return rp, cc, vv


def ilu0(n, rowptr, col, val):
    """((rowptr, col, val) of L, (rowptr, col, val) of U, zero_pivot): L's rows sorted, no diagonal; U's rows sorted, diagonal
    first; zero_pivot = smallest failing row or -1."""
    val = np.asarray(val)
    cplx = np.iscomplexobj(val)
    rows = full_rows(n, np.asarray(rowptr), np.asarray(col), val)
    Lc, Lv, Uc, Uv = [], [], [], []
    zp = -1
    with np.errstate(all="ignore"):
        for i in range(n):
            w = rows[i]
            cols = sorted(w)
            for k in cols:
                if k >= i:
                    break
                l = w[k] / Uv[k][0]                          # every earlier product with a smaller k is already subtracted
                w[k] = l
                for j, ukj in zip(Uc[k][1:], Uv[k][1:]):     # row k's upper part: L(i,k) U(k,j) leaves every (i,j) of the pattern
                    if j in w:
                        w[j] = w[j] - l * ukj
            d = w[i]
            bad = d == 0 or not (math.isfinite(d.real) and math.isfinite(d.imag))
            if bad and zp < 0:
                zp = i
            Lc.append([c for c in cols if c < i]); Lv.append([w[c] for c in cols if c < i])
            Uc.append([c for c in cols if c >= i]); Uv.append([w[c] for c in cols if c >= i])
    return _csr(Lc, Lv, cplx), _csr(Uc, Uv, cplx), zp


def to_sparse(n, tri):
    return sp.csr_matrix((np.asarray(tri[2]), np.asarray(tri[1]), np.asarray(tri[0])), shape=(n, n))


def levels(n, L, U):
    """(forward level of every row from L's pattern, backward level from U's): row i of L reads y_k for every k in its row;
    row i of U reads y_j for every j > i in its row."""
    fw = np.zeros(n, np.int64)
    for i in range(n):
        fw[i] = 1 + max((fw[k] for k in L[1][L[0][i]:L[0][i + 1]]), default=-1)
    bw = np.zeros(n, np.int64)
    for i in range(n - 1, -1, -1):
        bw[i] = 1 + max((bw[j] for j in U[1][U[0][i] + 1:U[0][i + 1]]), default=-1)
    return fw, bw


def launches(n, L, U, max_merged=1024):
    """Launches of one exact apply by DESIGN 11's grouping rule over both triangles."""
    fw, bw = levels(n, L, U)
    return IC.segments(IC.widths(fw), max_merged) + IC.segments(IC.widths(bw), max_merged)


def sweep_launches(k):
    """Launches of a k-sweep apply: U scales once and sweeps k - 1 times; L's first sweep is y = x, read by its second in place
    of a vector of its own (one copy when k = 1)."""
    return max(k - 1, 1) + k


class IluApply:
    """z = U^-1 L^-1 x with SciPy's triangular solves."""

    def __init__(self, n, L, U):
        self.L = (to_sparse(n, L) + sp.identity(n, dtype=np.asarray(L[2]).dtype)).tocsr()
        self.U = to_sparse(n, U)

    def solve(self, x, which=2):
        if which == 0:
            return spsolve_triangular(self.L, x, lower=True, unit_diagonal=True)
        if which == 1:
            return spsolve_triangular(self.U, x, lower=False)
        return spsolve_triangular(self.U, spsolve_triangular(self.L, x, lower=True, unit_diagonal=True), lower=False)


# ------------------------------------------------------------------------------------------ the defining property
def _frac(v):
    return (Fraction(float(v.real)), Fraction(float(v.imag))) if isinstance(v, complex) or np.iscomplexobj(v) else (Fraction(float(v)), Fraction(0))


def residual_check(n, rowptr, col, val, L, U):
    """max over the pattern of |(L.U - A)(i,j)| / (gamma(t + 1) (|L| |U|)(i,j)) (module docstring): <= 1 for a correct factor.
    Entries whose bound is 0 (nothing was computed: U(i,j) = A(i,j)) must match exactly; a violation there returns inf.
    Returns (worst ratio, its (i, j), largest t)."""
    cplx = np.iscomplexobj(L[2]) or np.iscomplexobj(U[2])
    u = UC if cplx else U64
    rowptr, col, val = np.asarray(rowptr), np.asarray(col), np.asarray(val)
    A = []                                              # per row {column: [the entries given for it]} (duplicates: summed by the build)
    for i in range(n):
        d = {i: []}
        for p in range(rowptr[i], rowptr[i + 1]):
            d.setdefault(int(col[p]), []).append(val[p])
        A.append(d)
    Lrow = [dict(zip(map(int, L[1][L[0][i]:L[0][i + 1]]), L[2][L[0][i]:L[0][i + 1]])) for i in range(n)]
    Ucol = [{} for _ in range(n)]
    for k in range(n):
        for p in range(U[0][k], U[0][k + 1]):
            Ucol[int(U[1][p])][k] = U[2][p]
    worst, where, tmax = 0.0, None, 0
    for i in range(n):
        Li = Lrow[i]
        for j, parts in A[i].items():
            Uj = Ucol[j]
            m = min(i, j)
            small, big = (Li, Uj) if len(Li) <= len(Uj) else (Uj, Li)
            ks = [k for k in small if k < m and k in big]
            t = len(ks)
            sr, si = Fraction(0), Fraction(0)
            for a in parts:                             # -A(i,j), exactly
                ar, ai = _frac(a)
                sr -= ar; si -= ai
            # the build's own sum of d duplicates: gamma(d - 1) sum |a_p| (Higham, section 4.2), carried into w(i,j) as it is
            dup = float(gamma(len(parts) - 1, u)) * float(sum(abs(a) for a in parts)) if len(parts) > 1 else 0.0
            mag = 0.0
            for k in ks:
                (lr, li), (ur, ui) = _frac(Li[k]), _frac(Uj[k])
                sr += lr * ur - li * ui
                si += lr * ui + li * ur
                mag += abs(Li[k]) * abs(Uj[k])
            if j >= i:                                  # L(i,i) = 1 times U(i,j)
                lr, li, (ur, ui) = Fraction(1), Fraction(0), _frac(Uj[i])
                mag += abs(Uj[i])
            else:
                (lr, li), (ur, ui) = _frac(Li[j]), _frac(Uj[j])
                mag += abs(Li[j]) * abs(Uj[j])
            sr += lr * ur - li * ui
            si += lr * ui + li * ur
            err = math.hypot(float(sr), float(si))
            bound = (float(gamma(t + 1, u)) * mag if (t or j < i) else 0.0) + dup
            ratio = 0.0 if err == 0.0 else (err / bound if bound > 0.0 else math.inf)
            if ratio > worst:
                worst, where = ratio, (i, j)
            tmax = max(tmax, t)
    return worst, where, tmax


# ------------------------------------------------------------------------------------------ sweeps
class Tri(S.Tri):
    """One triangle of the factor for ic0_sweeps_checker's `sweeps` / `exact` / `sweep_bound`: U as stored (diagonal first), or
    L with its unit diagonal made explicit and stored last -- dividing by 1 is exact in real arithmetic and in the scaled
    complex quotient (s = 1, a.re * 1 + a.im * 0 and a denominator of 1), so the row's result has the bits of not dividing."""

    def __init__(self, n, tri, up, level):
        T = to_sparse(n, tri)
        if not up:
            T = (T + sp.identity(n, dtype=T.dtype)).tocsr()
        T.sort_indices()
        self.n, self.up = n, up
        self.rp, self.col, self.val = T.indptr.astype(np.int64), T.indices.astype(np.int64), T.data
        s, e = self.rp[:-1], self.rp[1:]
        self.b, self.f, self.dg = (s + 1, e, s) if up else (s, e - 1, e - 1)
        assert np.array_equal(self.col[self.dg], np.arange(n))
        self.level = np.asarray(level)
        self.levels = int(self.level.max()) + 1 if n else 0
        self.longest = int((e - s).max()) if n else 0


def triangles(n, L, U):
    fw, bw = levels(n, L, U)
    return Tri(n, L, False, fw), Tri(n, U, True, bw)


class SweepApply:
    """The k-sweep operator of a factor (which 0: L, 1: U, 2: both, L's result the input of U's); k = 0: the exact row-ordered
    solves with the same row arithmetic."""

    def __init__(self, n, L, U, k):
        self.L, self.U = triangles(n, L, U)
        self.k = k
        self.kind = S.kind_of(self.U.val)

    def _one(self, T, x):
        return S.sweeps(T, x, self.k, self.kind) if self.k else S.exact(T, x, self.kind)

    def solve(self, x, which=2):
        if which == 0:
            return self._one(self.L, x)
        if which == 1:
            return self._one(self.U, x)
        return self._one(self.U, self._one(self.L, x))


def apply_bound(TL, TU, x, k, which):
    """Componentwise E of a k-sweep apply, so that two evaluations differ by at most 2 E (ic0_sweeps_checker.apply_bound with U in
    L^T's place)."""
    return S.apply_bound(TL, TU, x, k, which)


# ------------------------------------------------------------------------------------------ BiCGStab
def lbicgstab(A, b, eps, max_iterations=0):
    """liblcg's BiCGStab (lcg.cpp) from m = 0 with the relative stop rule r.r / max(m.m, 1) <= eps; A is a function.  Returns
    (m, iterations)."""
    n = len(b)
    m = np.zeros(n)
    r = b - A(m)
    r0 = r.copy()
    p = r.copy()
    rr0 = r @ r0
    m2 = max(m @ m, 1.0)
    r2 = r @ r
    t = 0
    if r2 / m2 <= eps:
        return m, 0
    while True:
        if r2 / m2 <= eps or (max_iterations > 0 and t + 1 > max_iterations):
            return m, t
        t += 1
        Ap = A(p)
        ak = rr0 / (Ap @ r0)
        s = r - ak * Ap
        As = A(s)
        wk = (As @ s) / (As @ As)
        m = m + (ak * p + wk * s)
        r = s - wk * As
        m2 = max(m @ m, 1.0)
        r2 = r @ r
        rr1 = r @ r0
        bk = (ak / wk) * rr1 / rr0
        rr0 = rr1
        p = r + bk * (p - wk * Ap)


def right_bicgstab(As, apply, b, eps):
    """Right-preconditioned run: A M^-1 u = b from u = 0 by lbicgstab, then x = M^-1 u.  Returns (x, iterations, |b - A x| / |b|)."""
    u, t = lbicgstab(lambda v: As @ apply(v), b, eps)
    x = apply(u)
    return x, t, float(np.linalg.norm(b - As @ x) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------ test matrices
def _arrays(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def convdiff(k, pe):
    """2-D convection-diffusion with first-order upwinding on a k x k grid: kron(I, T1) + kron(T2, I), T1 = tridiag(-1 - pe,
    2 + pe, -1), T2 = tridiag(-1 - pe/2, 2 + pe/2, -1) (sub-, main, super-diagonal).  Non-symmetric for pe > 0, an M-matrix."""
    T1 = sp.diags([-1.0 - pe, 2.0 + pe, -1.0], [-1, 0, 1], shape=(k, k))
    T2 = sp.diags([-1.0 - pe / 2, 2.0 + pe / 2, -1.0], [-1, 0, 1], shape=(k, k))
    I = sp.identity(k)
    return _arrays(sp.kron(I, T1) + sp.kron(T2, I))


def shifted(k, s):
    """The 5-point Laplacian of a k x k grid minus s I: symmetric, indefinite for s inside the spectrum."""
    rp, ci, v = S.laplace2d(k)
    return _arrays(sp.csr_matrix((v, ci, rp), shape=(k * k, k * k)) - s * sp.identity(k * k))


def drop_upper(rowptr, col, val, every=3):
    """The same matrix without every `every`-th strictly upper entry: a non-symmetric pattern."""
    keep = np.ones(len(col), bool)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    up = np.flatnonzero(np.asarray(col) > rows)
    keep[up[::every]] = False
    A = sp.csr_matrix((np.asarray(val)[keep], (rows[keep], np.asarray(col)[keep])), shape=(len(rowptr) - 1,) * 2)
    return _arrays(A)


def chain(n, seed=5):
    """A non-symmetric tridiagonal, diagonally dominant matrix: n levels of one row each in L and in U."""
    rng = np.random.default_rng(seed)
    return _arrays(sp.diags([rng.uniform(-1.0, 1.0, n - 1), 2.5 + rng.uniform(0.0, 1.0, n), rng.uniform(-1.0, 1.0, n - 1)], [-1, 0, 1]))


def rhs(As, seed=3):
    """b = A x* with x* uniform in [1, 2]."""
    xs = np.random.default_rng(seed).uniform(1.0, 2.0, As.shape[0])
    return As @ xs, xs


def convdiff3d(k, pe):
    """3-D convection-diffusion with first-order upwinding on a k^3 grid, 7 points: convdiff's two directions and a third,
    T3 = tridiag(-1 - pe/4, 2 + pe/4, -1), slowest.  Non-symmetric values on a symmetric pattern, an M-matrix; the forward level
    of grid point (z, y, x) is x + y + z."""
    T1 = sp.diags([-1.0 - pe, 2.0 + pe, -1.0], [-1, 0, 1], shape=(k, k))
    T2 = sp.diags([-1.0 - pe / 2, 2.0 + pe / 2, -1.0], [-1, 0, 1], shape=(k, k))
    T3 = sp.diags([-1.0 - pe / 4, 2.0 + pe / 4, -1.0], [-1, 0, 1], shape=(k, k))
    I = sp.identity(k)
    return _arrays(sp.kron(I, sp.kron(I, T1)) + sp.kron(I, sp.kron(T2, I)) + sp.kron(T3, sp.kron(I, I)))


def mirror(n, lower):
    """Strictly lower rows {j: value} turned about the anti-diagonal: entry (i, j), j < i, goes to (n-1-i, n-1-j), strictly
    upper.  A forward level of `lower` becomes the same backward level of the result."""
    upper = [{} for _ in range(n)]
    for i in range(n):
        for j, x in lower[i].items():
            upper[n - 1 - i][n - 1 - j] = x
    return upper


def dominant_diagonal(rng, n, lower, upper, cplx):
    """ic0_checker.dominant_diagonal for two independent triangles: 1 + U(0, 1) + every off-diagonal magnitude of the entry's
    row and of its column (complex: plus i U(-0.5, 0.5)).  Strictly dominant by rows and by columns: every ILU(0) pivot usable."""
    s = np.zeros(n)
    for part in (lower, upper):
        for i in range(n):
            for j, x in part[i].items():
                s[i] += abs(x); s[j] += abs(x)
    d = 1.0 + rng.uniform(0.0, 1.0, n) + s
    return d + 1j * rng.uniform(-0.5, 0.5, n) if cplx else d


def assemble(n, lower, upper, diag):
    """CSR (rows sorted) of strictly lower rows, strictly upper rows and a diagonal; nothing is mirrored."""
    rows = [{**lower[i], **upper[i], i: diag[i]} for i in range(n)]
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    cols = [sorted(r) for r in rows]
    ci = np.fromiter((c for cs in cols for c in cs), np.int32, int(rp[-1]))
    v = np.array([rows[i][c] for i in range(n) for c in cols[i]], np.complex128 if np.iscomplexobj(diag) else np.float64)
    return rp, ci, v


def layered_nonsym_parts(widths_L, widths_U, seed, cplx=False):
    """(lower, upper, diag, starts_L, starts_U): the strictly lower pattern is ic0_checker.layered_parts(widths_L), so L's forward
    level t is rows starts_L[t] .. starts_L[t+1]-1; the strictly upper pattern is a second, independent layered_parts(widths_U)
    turned about the anti-diagonal (`mirror`), so U's backward level t is rows n-starts_U[t+1] .. n-starts_U[t]-1.  Every value
    is a draw of its own; the diagonal is strictly dominant."""
    assert sum(widths_L) == sum(widths_U)
    lower, _, stL = IC.layered_parts(widths_L, seed, cplx)
    low2, _, stU = IC.layered_parts(widths_U, seed + 7919, cplx)
    n = int(stL[-1])
    upper = mirror(n, low2)
    diag = dominant_diagonal(np.random.default_rng(seed + 104729), n, lower, upper, cplx)
    return lower, upper, diag, stL, stU


def layered_nonsym(widths_L, widths_U, seed, cplx=False):
    """(rowptr, col, val), rows sorted, of layered_nonsym_parts: forward levels of exactly widths_L rows, backward levels of
    exactly widths_U rows (in backward level order), non-symmetric pattern and values."""
    lower, upper, diag, _, _ = layered_nonsym_parts(widths_L, widths_U, seed, cplx)
    return assemble(len(diag), lower, upper, diag)


def _strict_lower(rp, ci, v):
    n = len(rp) - 1
    return [{int(ci[p]): v[p] for p in range(rp[i], rp[i + 1]) if ci[p] < i} for i in range(n)]


def random_nonsym(n, seed):
    """ic0_checker.random_spd's strictly lower pattern and values; the strictly upper part is a second, independent draw of it
    turned about the anti-diagonal: irregular level sets in both triangles, no symmetry of pattern or values; strictly dominant."""
    lower = _strict_lower(*IC.random_spd(n, seed))
    upper = mirror(n, _strict_lower(*IC.random_spd(n, seed + 7919)))
    diag = dominant_diagonal(np.random.default_rng(seed + 104729), n, lower, upper, False)
    return assemble(n, lower, upper, diag)


# the sweep kernel's staging window (k_ic_sweep): SWEEP_ROWS consecutive rows per workgroup; their slice of the
# triangle, counted from the 4-entry unit that holds its first entry, is staged when it is at most SWEEP_WINDOW entries long
SWEEP_ROWS, SWEEP_WINDOW = 256, 2048
# entries of L / of U (diagonals included) in each 256-row workgroup of window_edges, and its short last workgroup's rows
WINDOW_L = (0, 2048, 2049, 2048, 2047, 301)
WINDOW_U = (2048, 2049, 2048, 2047, 1025, 100)
WINDOW_TAIL = 100


def sweep_windows(n, rowptr):
    """Per workgroup of a sweep over the triangle with this rowptr: (own entries, cnt, rowptr[row0] & 3), with
    cnt = rowptr[row0 + nrows] - (rowptr[row0] & ~3), the length the kernel compares with its window."""
    rowptr = np.asarray(rowptr)
    out = []
    for row0 in range(0, n, SWEEP_ROWS):
        s, e = int(rowptr[row0]), int(rowptr[min(row0 + SWEEP_ROWS, n)])
        out.append((e - s, e - (s & ~3), s & 3))
    return out


def window_cases(n, rowptr):
    """The window-edge situations a triangle's sweep meets, by name."""
    wins = sweep_windows(n, rowptr)
    found = set()
    for own, cnt, off in wins:
        if cnt == SWEEP_WINDOW and off == 0:
            found.add("full_aligned")               # cnt = 2048, rowptr[row0] & 3 = 0: the largest staged slice
        if cnt == SWEEP_WINDOW and off != 0:
            found.add("full_by_offset")             # cnt = 2048 of which the first `off` entries are the neighbour's
        if own == cnt == SWEEP_WINDOW + 1:
            found.add("over_by_one")                # cnt = 2049 of its own: global memory
        if own <= SWEEP_WINDOW < cnt:
            found.add("over_by_offset")             # at most 2048 of its own, over only through rowptr[row0] & 3 != 0
        if own == 0:
            found.add("all_rows_empty")
    own, cnt, off = wins[-1]
    if n % SWEEP_ROWS and cnt <= SWEEP_WINDOW and int(rowptr[n]) % 4:
        found.add("last_unit_in_slack")             # staged, and its last 16-byte unit of col ends past nnz
    return found


WINDOW_SET = {"full_aligned", "over_by_one", "over_by_offset", "last_unit_in_slack"}       # both triangles; L: + "all_rows_empty"


def window_edges(seed, cplx=False):
    """A matrix of 5 x 256 + WINDOW_TAIL rows whose ILU(0) triangles hold WINDOW_L / WINDOW_U entries in the sweep kernel's
    successive workgroups, which puts them on both sides of its window edge (window_cases).  Every workgroup is a layer: a row's
    strictly lower columns are drawn from the layers before it, its strictly upper ones from the layers after it, so L and U have
    at most 6 levels each.  A workgroup's entries are spread evenly over its rows, the first rows taking the remainder."""
    rng = np.random.default_rng(seed)
    n = SWEEP_ROWS * (len(WINDOW_L) - 1) + WINDOW_TAIL
    lower, upper = [{} for _ in range(n)], [{} for _ in range(n)]
    for w in range(len(WINDOW_L)):
        a, b = w * SWEEP_ROWS, min((w + 1) * SWEEP_ROWS, n)
        for part, total, lo, hi in ((lower, WINDOW_L[w], 0, a), (upper, WINDOW_U[w] - (b - a), b, n)):
            q, r = divmod(total, b - a)
            for i in range(a, b):
                k = q + (i - a < r)
                if k:
                    for j in rng.choice(hi - lo, size=k, replace=False) + lo:
                        part[i][int(j)] = IC._offdiag(rng, cplx)
    return assemble(n, lower, upper, dominant_diagonal(rng, n, lower, upper, cplx))


# ------------------------------------------------------------------------------------------ scheduled systems, pivot failures
# rows per forward level of L, rows per backward level of U (in backward level order): wide levels (> 1024 rows, a launch each)
# next to each other, after and before runs of narrow ones, at the widths 1023 / 1024 / 1025 around the rule's edge
LAYERS_L = [1024, 1025, 1, 1023, 3000, 1024, 5, 2048]
LAYERS_U = [2048, 7, 1024, 1500, 1, 1025, 1023, 2522]
PIVOT_CASES = ["two_in_wide_level", "larger_row_first_in_time", "narrow_run", "empty_row", "nan_upper", "complex_zero"]


def _zero_pivot(rp, ci, v, r):
    """Makes w(r,r) an exact zero whatever the rounding: A(r,r) = 0 and A(k,r) = 0 (still stored) for every k < r of row r, so
    the pivot is 0 - sum L(r,k).0."""
    for p in range(rp[r], rp[r + 1]):
        k = int(ci[p])
        if k == r:
            v[p] = 0.0
        elif k < r:
            q = rp[k] + np.flatnonzero(ci[rp[k]:rp[k + 1]] == r)
            v[q] = 0.0


def pivot_case(case, seed):
    """((rowptr, col, val) whose ILU(0) fails, the smallest failing row, (rowptr, col, val) repaired).  Ordinary bad matrices:
    every one has a defined error return."""
    if case == "larger_row_first_in_time":
        # convdiff3d(40, 2): row 1600 = (1, 0, 0) is on forward level 1, in the narrow run of levels 0-45 (one launch); row 439 =
        # (0, 10, 39) is on level 49, the fourth wide level after it: four launches later
        rp, ci, good = convdiff3d(40, 2)
        bad = good.copy()
        for r in (1600, 439):
            _zero_pivot(rp, ci, bad, r)
        return (rp, ci, bad), 439, (rp, ci, good)
    cplx = case == "complex_zero"
    lower, upper, diag, st, _ = layered_nonsym_parts(LAYERS_L, LAYERS_U, seed, cplx)
    n = len(diag)
    if case == "nan_upper":                         # U(k,i) = NaN, k in row i of L: the merge of row k carries it into w(i,i)
        want = int(st[4]) + 7
        k = min(lower[want])
        upper[k][want] = 0.5
        rp, ci, good = assemble(n, lower, upper, diag)
        bad = good.copy()
        bad[rp[k] + np.flatnonzero(ci[rp[k]:rp[k + 1]] == want)] = np.nan
        return (rp, ci, bad), want, (rp, ci, good)
    if case == "complex_zero":                      # L(i,j) = 2 / 4, w(i,i) = 1 - 0.5 * 2: (0, 0) exactly; row j is on level 0
        want, j = int(st[1]) + 3, int(st[0]) + 5
        lower[want] = {j: 2.0 + 0j}
        upper[j][want] = 2.0 + 0j
        diag[j] = 4.0 + 0j
        good = assemble(n, lower, upper, diag)
        diag[want] = 1.0 + 0j
        return assemble(n, lower, upper, diag), want, good
    rp, ci, good = assemble(n, lower, upper, diag)
    bad = good.copy()
    if case == "two_in_wide_level":                 # level 4: 3000 rows, 12 workgroups of 256; the first and the last
        want = int(st[4]) + 100
        _zero_pivot(rp, ci, bad, int(st[4]) + 2950)
        _zero_pivot(rp, ci, bad, want)
    elif case == "narrow_run":                      # level 3 (1023 rows), in the narrow run of levels 2-3
        want = int(st[3]) + 500
        _zero_pivot(rp, ci, bad, want)
    elif case == "empty_row":                       # nothing stored: its diagonal is the explicit zero the build puts there
        want = int(st[5]) + 10
        keep = np.ones(len(ci), bool)
        keep[rp[want]:rp[want + 1]] = False
        rpb = np.concatenate([rp[:want + 1], rp[want + 1:] - (rp[want + 1] - rp[want])]).astype(np.int32)
        return (rpb, ci[keep], good[keep]), want, (rp, ci, good)
    else:
        raise KeyError(case)
    return (rp, ci, bad), want, (rp, ci, good)
