"""numpy restatement of liblcg's dense products in the reference's own order -- a helper of the tests (like c64_checker.py),
not a conftest.

lcg_matvec (algebra.cpp:165-193) and clcg_matvec (lcg_complex.cpp:169-234) keep ONE accumulator per output and add the terms
for j (layout 0) or i (layout 1) ascending; the complex forms add, per term, exactly the two expressions of
lcg_complex.cpp:184-185, 198-199, 214-215, 228-229 (each a sum or difference of two rounded products, then added to the
accumulator).  The loops below walk the summation index and are vectorised over the outputs, so every output sees the
reference's sequence of roundings (numpy does not contract a * b + c).  tests/test_dense_cpu.py holds them to the real
liblcg bit for bit.
"""
from __future__ import annotations

import numpy as np


def matvec(K, x, layout=0):
    """lcg_matvec: layout 0 y = K.x, layout 1 y = K^T.x."""
    K = np.asarray(K, np.float64); x = np.asarray(x, np.float64)
    m, n = K.shape
    if layout == 0:
        y = np.zeros(m)
        for j in range(n):
            y += K[:, j] * x[j]
        return y
    y = np.zeros(n)
    for i in range(m):
        y += K[i, :] * x[i]
    return y


def cmatvec(K, x, layout=0, conjugate=0):
    """clcg_matvec's four forms.  conjugate = 1 conjugates the ENTRIES of K only (lcg_complex.cpp:184-185): conj(K).x / K^H.x."""
    K = np.asarray(K, np.complex128); x = np.asarray(x, np.complex128)
    m, n = K.shape
    kr, ki, xr, xi = K.real, K.imag, x.real, x.imag
    cols = layout == 0
    re = np.zeros(m if cols else n); im = np.zeros(m if cols else n)
    for k in range(n if cols else m):
        ar, ai = (kr[:, k], ki[:, k]) if cols else (kr[k, :], ki[k, :])
        if conjugate:
            re += ar * xr[k] + ai * xi[k]
            im += ar * xi[k] - ai * xr[k]
        else:
            re += ar * xr[k] - ai * xi[k]
            im += ar * xi[k] + ai * xr[k]
    return re + 1j * im


def ata(K, x):
    """sample1.cpp:48-53 (CalAx): tmp = K.x, then y = K^T.tmp."""
    return matvec(K, matvec(K, x, 0), 1)


def normal_diagonal(K):
    """sample1.cpp:98-107: d_i = sum_j K(j,i)^2, j ascending, one accumulator per column (the preconditioner is 1 / d_i)."""
    K = np.asarray(K, np.float64)
    d = np.zeros(K.shape[1])
    for j in range(K.shape[0]):
        d += K[j, :] * K[j, :]
    return d


def dense_as_csr(K):
    """K with every entry present as (rowptr, col, val): what tests/exact_ref.py's references take."""
    m, n = K.shape
    return np.arange(m + 1, dtype=np.int64) * n, np.tile(np.arange(n, dtype=np.int64), m), np.ascontiguousarray(K).reshape(-1)
