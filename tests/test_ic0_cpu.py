"""The IC(0) checker itself (tests/ic0_checker.py), without a GPU: it is the exact Cholesky factor wherever the pattern has no
fill, and on case_10K_A its preconditioned CG takes the iteration counts DESIGN 11 quotes."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import ic0_checker as K


def _dense_to_csr(A):
    n = A.shape[0]
    rp, ci, v = [0], [], []
    for i in range(n):
        nz = np.nonzero(A[i])[0]
        ci.extend(nz); v.extend(A[i, nz]); rp.append(len(ci))
    return np.array(rp), np.array(ci), np.array(v, A.dtype)


def _factor_dense(A):
    n = A.shape[0]
    rp, ci, v, zp = K.ic0(n, *_dense_to_csr(A))
    assert zp == -1
    return K.to_sparse(n, rp, ci, v).toarray()


def test_tridiagonal_is_exact_cholesky():
    n = 200
    rng = np.random.default_rng(3)
    off = rng.uniform(-1, 1, n - 1)
    A = np.diag(np.abs(off).sum() / n + 2.5 + rng.uniform(0, 1, n)) + np.diag(off, 1) + np.diag(off, -1)
    np.testing.assert_allclose(_factor_dense(A), np.linalg.cholesky(A), rtol=0, atol=1e-13)


def test_full_band_is_exact_cholesky():
    n, bw = 120, 5
    rng = np.random.default_rng(4)
    A = np.zeros((n, n))
    for k in range(1, bw + 1):
        o = rng.uniform(-1, 1, n - k)
        A += np.diag(o, k) + np.diag(o, -k)
    A += np.diag(2 * bw + 1 + rng.uniform(0, 1, n))
    np.testing.assert_allclose(_factor_dense(A), np.linalg.cholesky(A), rtol=0, atol=1e-12)


def test_upper_triangle_is_ignored_and_duplicates_sum():
    A = np.array([[4.0, 1.0, 0.0], [1.0, 5.0, 2.0], [0.0, 2.0, 6.0]])
    rp = np.array([0, 3, 7, 10]); ci = np.array([2, 0, 1, 1, 0, 2, 1, 2, 1, 2])
    v = np.array([99.0, 4.0, 7.0, 2.0, 1.0, 55.0, 3.0, 6.0, 2.0, 0.0])     # row 1's diagonal comes as 2 + 3
    Lr, Lc, Lv, zp = K.ic0(3, rp, ci, v)
    np.testing.assert_allclose(K.to_sparse(3, Lr, Lc, Lv).toarray(), np.linalg.cholesky(A), atol=1e-15)


def test_complex_is_unconjugated_with_principal_root():
    A = np.array([[2 + 1j, 0.5j], [0.5j, 3 - 2j]])
    L = _factor_dense(A)
    np.testing.assert_allclose(L @ L.T, A, atol=1e-14)
    assert L[0, 0].real > 0 and L[1, 1].real > 0


def test_failed_pivot_is_the_smallest_row():
    A = np.diag([1.0, 2.0, -1.0, 3.0, -2.0])
    assert K.ic0(5, *_dense_to_csr(A))[3] == 2


@pytest.fixture(scope="module")
def sys10k():
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    n, row, col, val, b = read_coo_system(os.path.join(GOLDEN, "case_10K_A"))
    rp, ci, v = coo_to_csr_host(n, row, col, val)
    return n, rp, ci, v, b


@pytest.mark.parametrize("eps,abs_diff,want_ic,want_jacobi", [(1e-10, 1, 54, 181), (1e-6, 0, 18, 57)])
def test_case10k_iteration_counts(sys10k, eps, abs_diff, want_ic, want_jacobi):
    n, rp, ci, v, b = sys10k
    Lr, Lc, Lv, zp = K.ic0(n, rp, ci, v)
    assert zp == -1
    assert Lv[Lr[1:] - 1].min() ** 2 > 1.1                  # every pivot positive (smallest 1.12)
    A = K.to_sparse(n, rp, ci, v)
    M = K.IcApply(K.to_sparse(n, Lr, Lc, Lv))
    assert K.lpcg(A, M.solve, b, eps, abs_diff)[1] == want_ic
    dinv = 1.0 / A.diagonal()
    assert K.lpcg(A, lambda r: r * dinv, b, eps, abs_diff)[1] == want_jacobi
