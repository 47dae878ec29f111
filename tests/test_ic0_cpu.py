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


# ------------------------------------------------------------------------------------------ level sets and launches
def _longest_paths(n, edges):
    """Longest path ending at every node of a DAG by n rounds of relaxation over all edges (u -> v: v after u)."""
    lev = np.zeros(n, np.int64)
    for _ in range(n):
        changed = False
        for u, v in edges:
            if lev[v] < lev[u] + 1:
                lev[v] = lev[u] + 1; changed = True
        if not changed:
            break
    return lev


@pytest.mark.parametrize("seed", range(6))
def test_levels_are_longest_paths(seed):
    from conftest import FUZZ_SEED_OFFSET
    rng = np.random.default_rng(500 + seed + FUZZ_SEED_OFFSET)
    n = int(rng.integers(1, 40))
    A = (rng.uniform(size=(n, n)) < rng.uniform(0.02, 0.3)).astype(float)
    A[rng.uniform(size=n) < 0.2] = 0.0                          # some empty rows
    rp, ci, _ = _dense_to_csr(A)
    # both triangles may hold entries: only the strictly lower ones are dependencies (row i reads row j < i)
    deps = {(int(j), i) for i in range(n) for j in ci[rp[i]:rp[i + 1]] if j < i}
    fw, bw = K.levels(n, rp, ci)
    np.testing.assert_array_equal(fw, _longest_paths(n, sorted(deps)))
    np.testing.assert_array_equal(bw, _longest_paths(n, sorted((i, j) for j, i in deps)))


def test_levels_follow_rows_not_storage_order():
    # row 2 reads row 1 (and stores an upper entry); row 3 reads rows 2 and 0, unsorted, row 0 twice
    rp = np.array([0, 1, 2, 5, 9]); ci = np.array([0, 1, 2, 1, 3, 3, 0, 2, 0])
    fw, bw = K.levels(4, rp, ci)
    np.testing.assert_array_equal(fw, [0, 0, 1, 2])
    np.testing.assert_array_equal(bw, [1, 2, 1, 0])     # L^T: row 1 waits for 2, which waits for 3; row 0 for 3 only


@pytest.mark.parametrize("widths,max_merged,want", [
    ([1024, 1025, 1024], 1024, 3),          # narrow, wide, narrow
    ([1024, 1024, 1024], 1024, 1),          # a level of exactly max_merged rows is narrow
    ([1025, 1025], 1024, 2),                # all wide
    ([3, 1, 700, 1024, 5], 1024, 1),        # all narrow: one run
    ([1, 2, 1, 3], 0, 4),                   # max_merged = 0: one launch per level
    ([1, 1, 2, 1, 1], 1, 3),                # 1: runs of single-row levels
    ([1023, 1024, 1023, 1], 1023, 3),       # 1023: the 1024-row level is wide
    ([2048, 1, 1, 2048, 7, 2048], 1024, 5),
    ([], 1024, 0),
])
def test_segments_rule(widths, max_merged, want):
    assert K.segments(widths, max_merged) == want


def test_laplace3d_40_levels_and_launches():
    rp, ci, _ = K.laplace3d(40)
    fw, bw = K.levels(len(rp) - 1, rp, ci)
    wf, wb = K.widths(fw), K.widths(bw)
    assert len(wf) == len(wb) == 118
    assert (wf > 1024).sum() == (wb > 1024).sum() == 26
    assert K.segments(wf, 1024) + K.segments(wb, 1024) == 56


@pytest.mark.parametrize("cplx", [False, True])
def test_layered_generator_gives_the_widths_asked(cplx):
    widths = [1024, 1025, 1, 1023, 3000, 1024, 5, 2048]
    rp, ci, v = K.layered(widths, 41, cplx)
    n = len(rp) - 1
    assert n == sum(widths) and np.iscomplexobj(v) == cplx
    fw, _ = K.levels(n, rp, ci)
    assert list(K.widths(fw)) == widths
    srp, sci, sv = K.shuffle_split(rp, ci, v, 42)
    assert list(K.widths(K.levels(n, srp, sci)[0])) == widths
    As, Ass = K.to_sparse(n, rp, ci, v), K.to_sparse(n, srp, sci, sv)
    assert abs(As - As.T).max() == 0 and abs(As - Ass).max() < 1e-15
    assert K.ic0(n, rp, ci, v)[3] == -1


def test_checker_pbicg_converges_on_complex_case():
    from conftest import _ccase
    n, rp, ci, v, b, xs = _ccase("1K")
    Lr, Lc, Lv, zp = K.ic0(n, rp, ci, v)
    assert zp == -1
    A = K.to_sparse(n, rp, ci, v)
    M = K.IcApply(K.to_sparse(n, Lr, Lc, Lv))
    m, t = K.clpbicg(A, M.solve, b, 1e-10, 1)
    assert t == 17 and np.linalg.norm(m - xs) < 1e-8
    # A complex-symmetric and M = M^T: the shadow recurrence walks conj of the primal one, so PBiCG meets PCG
    mp, tp = K.clpcg(A, M.solve, b, 1e-10, 1)
    assert tp == t and np.linalg.norm(m - mp) <= 1e-10 * np.linalg.norm(mp)
