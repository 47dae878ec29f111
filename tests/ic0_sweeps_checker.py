"""The IC(0) sweep checker: a triangular solve replaced by k Jacobi sweeps, restated in NumPy from the math, not
from any implementation.

For a triangle T = D + N (D its diagonal, N its strict part) applied to x:
    y(1)_i   = x_i / T(i,i)
    y(j+1)_i = (x_i - sum_p T(i,c_p) y(j)_{c_p}) / T(i,i)        p over the row's off-diagonal entries in column order
    result   = y(k)
Every sweep reads y(j) and writes y(j+1) into another vector.  A row is summed by one accumulator: start from x_i, subtract the
products in column order, divide once by the diagonal.  N is nilpotent, so k >= levels(T) sweeps give the exact solve, and --
the row's arithmetic being the exact row-ordered solve's -- the same bits (`exact` below is that solve).

Arithmetic kinds: "f64" (real), "c128", "c64", and "f80" / "c80" (np.longdouble: the wider recurrence that `sweep_bound` is
checked against).  Complex values are carried as (re, im) pairs of real arrays, so that every real operation is one IEEE
rounding whatever the array length: product (ar br - ai bi, ar bi + ai br), quotient by ic0_c64_checker's rule (both operands
scaled by |b.re| + |b.im|).  "c64" uses ic0_c64_checker's own fp32 product (fused multiply-adds) and quotient.

`sweep_bound(T, x, k)` is the componentwise rounding bound E(k) of k sweeps:
    E(1)   = g |x| / |D|
    E(j+1) = |D|^-1 ( |N| E(j) + g (|x| + |N| |y(j)|) )
    g      = (longest row + 3) u c,   u = 2^-53 (f64, c128) or 2^-24 (c64),   c = 1 (real) or 4 (complex: the constants of
             complex multiplication and scaled division)
Two evaluations in the same precision differ by at most 2 E(k): both round.  With `e_in`, a componentwise bound on a difference
between the two evaluations' inputs x, the same recurrence carries it along (E(1) = (g |x| + e_in) / |D|, and e_in beside
g (...) afterwards): that is how the full apply (L's sweeps feeding L^T's) is bounded -- first order in g, like the rest.
"""
import numpy as np
import scipy.sparse as sp

import ic0_c64_checker as Q
import ic0_checker as IC

KINDS = {"f64": (np.float64, False, 2.0 ** -53), "c128": (np.float64, True, 2.0 ** -53), "c64": (np.float32, True, 2.0 ** -24),
         "f80": (np.longdouble, False, None), "c80": (np.longdouble, True, None)}


def kind_of(val):
    dt = np.asarray(val).dtype
    return "c64" if dt == np.complex64 else "c128" if dt.kind == "c" else "f64"


class Tri:
    """One triangle in CSR, rows sorted: L (diagonal last) or, up=True, L^T (diagonal first), from L's arrays."""

    def __init__(self, n, rowptr, col, val, up):
        L = sp.csr_matrix((np.asarray(val), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
        T = L.T.tocsr() if up else L
        T.sort_indices()
        self.n, self.up = n, up
        self.rp, self.col, self.val = T.indptr.astype(np.int64), T.indices.astype(np.int64), T.data
        s, e = self.rp[:-1], self.rp[1:]
        self.b, self.f, self.dg = (s + 1, e, s) if up else (s, e - 1, e - 1)
        assert np.array_equal(self.col[self.dg], np.arange(n)), "every row has its diagonal, first (L^T) or last (L)"
        fw, bw = IC.levels(n, L.indptr, L.indices)
        self.level = bw if up else fw
        self.levels = int(self.level.max()) + 1 if n else 0
        self.longest = int((e - s).max()) if n else 0

    def abs_parts(self):
        """(|D| as a vector, |N| as a sparse matrix) in float64."""
        A = sp.csr_matrix((np.abs(self.val).astype(np.float64), self.col, self.rp), shape=(self.n, self.n))
        d = A.diagonal()
        return d, (A - sp.diags(d)).tocsr()


def triangles(n, rowptr, col, val):
    """(L, L^T) of a factor given as L's CSR arrays (rows sorted, diagonal last)."""
    return Tri(n, rowptr, col, val, False), Tri(n, rowptr, col, val, True)


# ------------------------------------------------------------------------------------------ arithmetic on (re, im) pairs
def _parts(v, kind):
    R, cplx, _ = KINDS[kind]
    v = np.asarray(v)
    return (v.real.astype(R), v.imag.astype(R)) if cplx else (v.astype(R), None)


def _whole(p, kind):
    R, cplx, _ = KINDS[kind]
    if not cplx:
        return p[0]
    C = {np.float32: np.complex64, np.float64: np.complex128, np.longdouble: np.clongdouble}[R]
    out = np.empty(len(p[0]), C)
    out.real, out.imag = p[0], p[1]
    return out


def _mul(a, b, kind):
    if kind == "c64":
        return Q._vmul(a[0], a[1], b[0], b[1])
    if a[1] is None:
        return a[0] * b[0], None
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _div(a, b, kind):
    with np.errstate(all="ignore"):
        if a[1] is None:
            return a[0] / b[0], None
        return Q._vdiv(a[0], a[1], b[0], b[1])         # (dtype-generic: 1 / s in the operands' own type)


def _take(p, idx):
    return p[0][idx], None if p[1] is None else p[1][idx]


def _put(p, idx, v):
    p[0][idx] = v[0]
    if p[1] is not None:
        p[1][idx] = v[1]


def _rows(T, tv, rows, x, y, kind):
    """The new values of `rows`: one accumulator per row from x_i, the row's products T(i,c) y_c subtracted in column order (all rows
    advanced one entry at a time, a row dropping out when it has no more), one division by the diagonal."""
    b, f, dg = T.b[rows], T.f[rows], T.dg[rows]
    acc = _take(x, rows)
    acc = (acc[0].copy(), None if acc[1] is None else acc[1].copy())
    ln = f - b
    for q in range(int(ln.max()) if len(rows) else 0):
        act = np.nonzero(ln > q)[0]
        p = b[act] + q
        pr = _mul(_take(tv, p), _take(y, T.col[p]), kind)
        acc[0][act] = acc[0][act] - pr[0]
        if acc[1] is not None:
            acc[1][act] = acc[1][act] - pr[1]
    return _div(acc, _take(tv, dg), kind)


def sweeps(T, x, k, kind=None, history=None):
    """y(k): k sweeps on triangle T from y = 0, row by row in column order, between two vectors.  history: a list that receives
    y(1) .. y(k)."""
    assert k >= 1
    kind = kind or kind_of(T.val)
    tv, xp = _parts(T.val, kind), _parts(x, kind)
    allrows = np.arange(T.n)
    y = _div(xp, _take(tv, T.dg), kind)
    if history is not None:
        history.append(_whole(y, kind))
    for _ in range(k - 1):
        y = _rows(T, tv, allrows, xp, y, kind)          # reads the old vector, returns a new one
        if history is not None:
            history.append(_whole(y, kind))
    return _whole(y, kind)


def exact(T, x, kind=None):
    """T^-1 x by the row-ordered solve, level by level (a level's rows read earlier levels only), with the rows' arithmetic of
    `sweeps`."""
    kind = kind or kind_of(T.val)
    R, cplx, _ = KINDS[kind]
    tv, xp = _parts(T.val, kind), _parts(x, kind)
    y = (np.zeros(T.n, R), np.zeros(T.n, R) if cplx else None)
    order = np.argsort(T.level, kind="stable")
    bounds = np.searchsorted(T.level[order], np.arange(T.levels + 1))
    for l in range(T.levels):
        rows = order[bounds[l]:bounds[l + 1]]
        _put(y, rows, _rows(T, tv, rows, xp, y, kind))
    return _whole(y, kind)


class SweepApply:
    """The k-sweep operator of a factor: which 0: k sweeps on L, 1: on L^T, 2: both, L's result the input of L^T's.  k = 0: the
    exact row-ordered solves."""

    def __init__(self, n, rowptr, col, val, k, kind=None):
        self.L, self.LT = triangles(n, rowptr, col, val)
        self.k, self.kind = k, kind or kind_of(val)

    def _one(self, T, x):
        return sweeps(T, x, self.k, self.kind) if self.k else exact(T, x, self.kind)

    def solve(self, x, which=2):
        if which == 0:
            return self._one(self.L, x)
        if which == 1:
            return self._one(self.LT, x)
        return self._one(self.LT, self._one(self.L, x))

    def mx(self, x):
        return self.solve(x, 2)


# ------------------------------------------------------------------------------------------ the rounding bound
def gamma(T, kind):
    _, cplx, u = KINDS[kind]
    return (T.longest + 3) * u * (4.0 if cplx else 1.0)


def sweep_bound(T, x, k, kind=None, e_in=None):
    """E(k), componentwise (float64): the rounding bound of k sweeps on T applied to x (module docstring).  e_in: a componentwise
    bound on a difference in the input x between the two evaluations compared."""
    kind = kind or kind_of(T.val)
    g = gamma(T, kind)
    d, N = T.abs_parts()
    ax = np.abs(np.asarray(x)).astype(np.float64)
    e0 = np.zeros(T.n) if e_in is None else np.asarray(e_in, np.float64)
    ys = []
    sweeps(T, x, k, kind, history=ys)
    E = (g * ax + e0) / d
    for j in range(1, k):
        E = (N @ E + e0 + g * (ax + N @ np.abs(ys[j - 1]).astype(np.float64))) / d
    return E


def apply_bound(L, LT, x, k, which, kind=None):
    """The componentwise bound E of a k-sweep apply (which 0, 1, 2), so that two evaluations differ by at most 2 E.  which = 2:
    L^T's sweeps on the checker's L result, with L's bound as the difference of their inputs."""
    kind = kind or kind_of(L.val)
    if which == 0:
        return sweep_bound(L, x, k, kind)
    if which == 1:
        return sweep_bound(LT, x, k, kind)
    return sweep_bound(LT, sweeps(L, x, k, kind), k, kind, e_in=sweep_bound(L, x, k, kind))


# ------------------------------------------------------------------------------------------ test matrices
def arrow(n, cplx=False):
    """A dense last row and column on a diagonal (symmetric, dominant): row n-1 of L is dense, every row of L^T but the last
    has two entries."""
    lower = [{} for _ in range(n)]
    for j in range(n - 1):
        lower[n - 1][j] = 1.0 / (1 + j % 5) + (0.25j * ((j % 3) - 1) if cplx else 0.0)
    diag = np.array([4.0 + (i % 7) for i in range(n - 1)] + [float(n)]) + (0.5j if cplx else 0.0)
    return IC.assemble(n, lower, diag)


def chain(n, seed=5):
    """A tridiagonal SPD matrix: n levels of one row each, both ways."""
    rng = np.random.default_rng(seed)
    lower = [{} if i == 0 else {i - 1: rng.uniform(-1.0, 1.0)} for i in range(n)]
    return IC.assemble(n, lower, 2.5 + rng.uniform(0.0, 1.0, n))


def laplace2d(k):
    """The 5-point Laplacian on a k x k grid, rows sorted."""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(k, k))
    A = (sp.kron(T, sp.identity(k)) + sp.kron(sp.identity(k), T)).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


UNEVEN_WIDTHS = [3, 40, 1, 1, 700, 5, 2, 1500, 30, 1, 1, 200, 9]


def uneven(name):
    """(rowptr, col, val) of a matrix with rows of uneven length: real ("spd": a random pattern, "arrow700", "arrow4096") or
    complex symmetric ("layered": a random pattern, "carrow700", "carrow4096")."""
    if name == "spd":
        return IC.random_spd(3000, 21)
    if name == "layered":
        return IC.layered(UNEVEN_WIDTHS, seed=6, cplx=True)
    return arrow(int(name.lstrip("carrow")), name.startswith("c"))


def factor(rowptr, col, val):
    """The checker's IC(0) factor of a test matrix in the precision of val: (n, rowptr, col, val of L)."""
    n = len(rowptr) - 1
    f = Q.ic0 if np.asarray(val).dtype == np.complex64 else IC.ic0
    rp, cc, vv, zp = f(n, rowptr, col, val)
    assert zp == -1
    return n, rp, cc, vv


def random_vector(n, kind, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, n)
    if KINDS[kind][1]:
        x = x + 1j * rng.uniform(-1.0, 1.0, n)
    return x.astype({"f64": np.float64, "c128": np.complex128, "c64": np.complex64}[kind])
