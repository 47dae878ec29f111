"""-m gpu: every A.x form against the exact sums and per-row rounding bounds of tests/exact_ref.py.

Each form runs (a) on integer data, where any correct summation order gives the exact sum and y must match it bit for bit, and
(b) on full-mantissa data whose rows and columns are scaled by 2^U(-30, 30), against the per-row bound gamma(L_i + 4) (|A||x|)_i
(c128: sqrt(2) gamma(2 L_i + 4)).  y is filled with NaN before every call (an unwritten row fails), and every case asserts the
kernel family it reached (lcg_hip_csr_last_kernel, packed runs / templates).  Then: non-finite entries of x stay in the rows
that reference them, and products follow a rewrite of an adopted matrix's values and columns (include/lcg_hip.h)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import exact_ref as X
from test_gpu_kernels import _ragged, _stencil
from test_gpu_ranges import mixed_system

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_out(n, dtype):
    return torch.full((n,), complex(np.nan, np.nan) if dtype.is_complex else np.nan, dtype=dtype, device="cuda")


def data(rng, rp, ncols, cplx, integer, kind=None, max_len=None):
    """(val, x): integers within the exactness rule (a) or full-mantissa values, rows and columns scaled by 2^U(-30, 30) (b)."""
    nnz = int(rp[-1]); lens = np.diff(rp)
    if integer:
        p = X.int_bits(max(1, int(max_len if max_len is not None else lens.max(initial=1))), kind or ("c128" if cplx else "f64"))
        return X.int_values(rng, nnz, p, cplx), X.int_values(rng, ncols, p, cplx, zeros=0.02)
    val = rng.standard_normal(nnz) + (1j * rng.standard_normal(nnz) if cplx else 0)
    x = rng.standard_normal(ncols) + (1j * rng.standard_normal(ncols) if cplx else 0)
    return val * np.repeat(2.0 ** rng.uniform(-30, 30, len(lens)), lens), x * 2.0 ** rng.uniform(-30, 30, ncols)


def check(y, rp, col, val, x, integer, tag, lens=None):
    y = y.cpu().numpy() if isinstance(y, torch.Tensor) else y
    if integer:
        X.assert_exact(y, X.exact_int_product(rp, col, val, x), tag)
    else:
        X.assert_rows(y, rp, col, val, x, tag, lens=lens)


def max_line(rp, col, ncols):
    """Longest row or column: the terms per sum of A.x and A^T.x."""
    return int(max(np.diff(rp).max(initial=1), np.bincount(col, minlength=ncols).max(initial=1)))


def product(api, lib, A, xd, ydt, n, form="A"):
    """y = op(A).x into a NaN-filled vector; form 'A' / 'AT' / 'conj' / 'AH'.  Returns (y, kernel name)."""
    y = nan_out(n, ydt)
    if form == "A":
        A.spmv(xd, y)
    else:
        layout, conj = {"AT": (1, 0), "conj": (0, 1), "AH": (1, 1)}[form]
        assert lib.lcg_hip_spmv_op(A.h, xd.data_ptr(), y.data_ptr(), layout, conj) == 0
    api.synchronize()
    return y, lib.lcg_hip_csr_last_kernel(A.h).decode()


def op_csr(rp, col, val, n, form):
    """CSR of op(A) (any entry order within a row: the checks do not depend on it)."""
    if form == "A":
        return rp, col, val
    M = sp.csr_matrix((val, col, rp), shape=(n, n))
    M = M.T.tocsr() if form in ("AT", "AH") else M
    v = np.conj(M.data) if form in ("conj", "AH") else M.data
    if form == "conj":
        return rp, col, np.conj(val)
    return M.indptr, M.indices, v


def dot_check(lib, A, xd, ud, rp, col, val, x, integer, tag, expect):
    """lcg_hip_spmv_dot (the automatic choice: a forced variant never carries the dot): y exact (a) or within the row bound (b) like
    the plain product, y.u and y.y exact (a) or within the dot bound (b)."""
    n = xd.numel()
    A.set_kernel(0)
    y = nan_out(n, xd.dtype)
    sums = (C.c_double * 2)()
    assert lib.lcg_hip_spmv_dot(A.h, xd.data_ptr(), y.data_ptr(), ud.data_ptr(), sums) == 0
    kern = lib.lcg_hip_csr_last_kernel(A.h).decode()
    assert expect in kern, (tag, kern)
    check(y, rp, col, val, x, integer, tag + ("dot", kern))
    yh, uh = y.cpu().numpy(), ud.cpu().numpy()
    for s, (exact, absum) in zip(sums, (X.hp_dot(yh, uh), X.hp_dot(yh, yh))):
        if integer:
            assert s == exact, (tag, kern, s, exact)
        else:
            assert abs(s - exact) <= X.dot_bound(absum, n), (tag, kern, s, exact, absum)
    return kern


def dot_u(rng, n, integer, rp):
    """u for the dot: integers small enough that y.u and y.y are exact sums (a), or full-mantissa values (b)."""
    if not integer:
        return rng.standard_normal(n) * 2.0 ** rng.uniform(-20, 20, n)
    return X.int_values(rng, n, 4, zeros=0)


def dot_data(rng, rp, ncols, integer):
    """(val, x) for products whose dot must be exact on integer data: |y| <= 2^q, |u| <= 2^4, n terms of y.y within 52 bits."""
    if not integer:
        return data(rng, rp, ncols, False, False)
    n = len(rp) - 1
    q = (52 - int(np.ceil(np.log2(max(2, n)))) ) // 2
    lb = int(np.ceil(np.log2(max(2, np.diff(rp).max(initial=1)))))
    p = max(1, (q - lb) // 2)
    return X.int_values(rng, int(rp[-1]), p), X.int_values(rng, ncols, p, zeros=0.02)


# ------------------------------------------------------------------------------------------------ 3. the sweep
VARIANTS = (0, -1, -16, -32, -64, -128, -256, 1, 2, 4, 8, 16, 32, 64)


@pytest.mark.parametrize("integer", [True, False], ids=["exact", "bound"])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_set_kernel_variants(api, lib, cplx, integer):
    """Lanes per row (k_spmv_wave), LDS-staged one window (k_spmv_lds1) and windowed (k_spmv_ldsw), the automatic choice; sizes at the
    block edges, empty first and last rows, rows that fill an LDS window exactly and one entry more."""
    rng = np.random.default_rng(101 + 2 * cplx + integer)
    win = 2240 if not cplx else 1344
    seen = set()
    for n, max_len, long_rows in ((1, 9, ()), (63, 9, ()), (64, 12, ()), (65, 30, ()), (255, 40, ()), (256, 3, ()), (257, 60, ()),
                                  (3001, 40, ((5, 5000), (2999, 2500), (3000, 7))), (4000, 8, ((70, win), (1000, win + 1)))):
        lens = rng.integers(0, max_len + 1, n)
        lens[rng.integers(0, n, n // 10)] = 0
        for r, ln in long_rows:
            lens[r] = ln
        if n > 2:
            lens[0] = lens[-1] = 0          # empty first and last rows
        lens[0] += lens.sum() == 0
        rp = np.zeros(n + 1, np.int32); np.cumsum(lens, out=rp[1:])
        col = rng.integers(0, n, rp[-1]).astype(np.int32)
        val, x = data(rng, rp, n, cplx, integer)
        A = api.CsrMatrix.from_csr(rp, col, val)
        xd = dev(x)
        for var in VARIANTS:
            A.set_kernel(var)
            y, kern = product(api, lib, A, xd, xd.dtype, n)
            if var > 0:
                assert kern.startswith("k_spmv_wave"), (n, var, kern)
            elif var < -1:
                assert kern.startswith(("k_spmv_lds1 ", "k_spmv_ldsw ")), (n, var, kern)
            elif var == -1:     # (the automatic LDS choice takes k_spmv_run1 where the blocks are runs: a single row is one)
                assert kern.startswith(("k_spmv_lds1 ", "k_spmv_ldsw ", "k_spmv_run1 ")), (n, var, kern)
            else:               # (automatic: the row-block families at these sizes; c128 has no packed forms)
                assert kern.startswith(("k_spmv_lds1 ", "k_spmv_ldsw ", "k_spmv_run1 ", "k_spmv_wave")), (n, var, kern)
            seen.add(kern.split(" ")[0])
            check(y, rp, col, val, x, integer, (n, var, kern))
        A.destroy()
    assert {"k_spmv_wave", "k_spmv_lds1", "k_spmv_ldsw"} <= seen, seen


def _packed_cases(rng):
    """(name, rp, col, ncols, set_kernel, packed mode, expected substrings of the kernel name, run / template expectation)."""
    out = []
    n = 3001
    rp, col = _ragged(rng, n, n, 30)
    out.append(("ragged, 18-bit", rp, col, n, -64, 1, ("k_spmv_ldsp", "18-bit")))
    nc = 1 << 20
    lens = rng.integers(0, 30, 2049); lens[0] = lens[-1] = 0
    rp2 = np.zeros(2050, np.int32); np.cumsum(lens, out=rp2[1:])
    out.append(("wide blocks, 21-bit", rp2, rng.integers(0, nc - 1, rp2[-1]).astype(np.int32), nc, -64, 1, ("k_spmv_ldsp", "21-bit")))
    L, n = 5, 6400 + 13
    offs = np.sort(rng.choice(3000, L, replace=False))
    out.append(("run blocks", (np.arange(n + 1) * L).astype(np.int32), (np.arange(n)[:, None] + offs).ravel().astype(np.int32), n + 3000,
                -64, 1, ("k_spmv_ldsp", "run blocks")))
    for dims in ((9, 7, 5), (20, 33, 64)):
        nn, rps, cis = _stencil(dims, 1)
        out.append((f"templates <= 32 diagonals {dims}", rps, cis, nn, -64, 1, ("k_spmv_ldsp", "template blocks")))
    for dims, faces, dof in (((12, 11, 20), True, 4), ((40, 70), False, 3)):
        n0, rp0, ci0 = _stencil(dims, 1, faces)
        B = sp.kron(sp.csr_matrix((np.ones(len(ci0)), ci0, rp0), shape=(n0, n0)), np.ones((dof, dof)), format="csr"); B.sort_indices()
        out.append((f"templates 33..64 diagonals {dims} x {dof}", B.indptr.astype(np.int32), B.indices.astype(np.int32), n0 * dof, -64, 1,
                    ("k_spmv_ldsp", "template blocks")))
    for dims, dof, want in (((14, 15, 16), 2, "long rows"), ((12, 13, 14), 3, "per group of consecutive columns")):
        n0, rp0, ci0 = _stencil(dims, 1, False)
        B = sp.kron(sp.csr_matrix((np.ones(len(ci0)), ci0, rp0), shape=(n0, n0)), np.ones((dof, dof)), format="csr"); B.sort_indices()
        out.append((f"long rows 27-point x {dof}", B.indptr.astype(np.int32), B.indices.astype(np.int32), n0 * dof, 0, 1, ("long rows", want)))
    lens = rng.integers(40, 69, 9001); lens[rng.integers(0, 9001, 20)] = 0
    rp3 = np.zeros(9002, np.int64); rp3[1:] = np.cumsum(lens)
    ci3 = np.concatenate([np.sort(rng.choice(np.arange(max(0, i - 3000), min(9001, i + 3000)), lens[i], replace=False)) for i in range(9001)])
    out.append(("long rows ragged", rp3.astype(np.int32), ci3.astype(np.int32), 9001, 0, 1, ("long rows",)))
    for dims, faces in (((6, 9, 16), True), ((33, 64), False), ((9, 8, 30), True)):
        nn, rps, cis = _stencil(dims, 2 if dims == (9, 8, 30) else 1, faces)
        out.append((f"k_spmv_run1 {dims}", rps, cis, nn, 0, -1, ("k_spmv_run1 ",)))
    return out


@pytest.mark.parametrize("integer", [True, False], ids=["exact", "bound"])
def test_packed_run_template_long_and_run1(api, lib, integer):
    """Packed columns (18 / 21 bits), run blocks, template blocks (<= 32 and 33 .. 64 diagonals, several unknowns per point), long
    rows in blocks of 32 / 16 (pk_R, pk_dof) and k_spmv_run1: y against the exact sum or the bound; the product carrying the dot where
    the family carries it (k_spmv_ldsp, k_spmv_run1d), its y bit-identical and its sums exact / within the dot bound."""
    rng = np.random.default_rng(202 + integer)
    for name, rp, col, ncols, var, mode, want in _packed_cases(rng):
        n = len(rp) - 1
        val, x = dot_data(rng, rp, ncols, integer)
        A = api.CsrMatrix.from_csr(rp, col, val, n_cols=ncols)
        A.set_kernel(var)
        assert lib.lcg_hip_csr_set_packed(A.h, mode) == 0
        xd = dev(x)
        y, kern = product(api, lib, A, xd, xd.dtype, n)
        assert all(w in kern for w in want), (name, kern)
        if "run blocks" in want:
            assert lib.lcg_hip_csr_packed_runs(A.h, None) > 0, name
        if "template blocks" in want:
            assert lib.lcg_hip_csr_packed_templates(A.h) > 0, name
        check(y, rp, col, val, x, integer, name)
        if n == ncols:
            ud = dev(dot_u(rng, n, integer, rp))
            expect = "k_spmv_run1d" if "run1" in name else ("long rows" if "long rows" in name else "carrying the dot")
            dot_check(lib, A, xd, ud, rp, col, val, x, integer, (name,), expect)
        A.destroy()


def _generated(api, n, pattern, band, seed):
    G = api.CsrMatrix.generate(n, 16, band, True, seed, 0.01, pattern=pattern)
    rp, ci, _ = G.arrays_to_host()
    G.destroy()
    return rp, ci


@pytest.mark.parametrize("integer", [True, False], ids=["exact", "bound"])
def test_tiled_binned_and_dot_families(api, lib, integer):
    """k_tile_spmv (row-random bands; one row past a 1024-row chunk), k_bin_expand (scrambled columns), k_spmv_lds1d (small ragged
    systems at block edges), each with y checked, and the dot each carries."""
    rng = np.random.default_rng(303 + integer)
    for n, pattern, setter, want in ((20000, api.GEN_ROW_RANDOM_BAND, lib.lcg_hip_csr_set_tiled, "k_tile_spmv"),
                                     (8 * 1024 + 1, api.GEN_ROW_RANDOM_BAND, lib.lcg_hip_csr_set_tiled, "k_tile_spmv"),
                                     (20000, api.GEN_SCRAMBLED, lib.lcg_hip_csr_set_binned, "k_bin_expand")):
        rp, ci = _generated(api, n, pattern, 3000 if pattern else 0, 2)
        val, x = dot_data(rng, rp, n, integer)
        A = api.CsrMatrix.from_csr(rp, ci, val)
        assert setter(A.h, 1) == 0
        xd = dev(x)
        y, kern = product(api, lib, A, xd, xd.dtype, n)
        assert kern.startswith(want), (n, kern)
        check(y, rp, ci, val, x, integer, (n, kern))
        if want == "k_tile_spmv":
            dot_check(lib, A, xd, dev(dot_u(rng, n, integer, rp)), rp, ci, val, x, integer, (n, "tiled"), "k_tile_spmv")
        A.destroy()
    seen = set()
    for n, max_len in ((1, 3), (63, 12), (64, 30), (65, 3), (257, 12), (5000, 30), (2049, 6)):
        rp, col = _ragged(rng, n, n, max_len)
        if rp[-1] == 0:
            continue
        val, x = dot_data(rng, rp, n, integer)
        A = api.CsrMatrix.from_csr(rp, col, val)
        xd = dev(x)
        y, kern = product(api, lib, A, xd, xd.dtype, n)
        check(y, rp, col, val, x, integer, (n, kern))
        dot_check(lib, A, xd, dev(dot_u(rng, n, integer, rp)), rp, col, val, x, integer, (n, max_len),
                         "k_spmv_lds1d" if n >= 256 else "carrying the dot")
        seen.add(lib.lcg_hip_csr_last_kernel(A.h).decode().split(" ")[0])
        # (below 256 rows a short last block -- one row -- can make the blocks mostly runs: k_spmv_run1d carries the dot then)
        A.destroy()
    assert "k_spmv_lds1d" in seen, seen


def _arrow(rng, n=300_000):
    offs = np.unique(np.concatenate([[0], rng.integers(1, 3000, 8)]))
    B = sp.diags([np.ones(n - o) for o in offs], offs, shape=(n, n), format="coo")
    rows = [B.row, B.col[B.row != B.col]]; cols = [B.col, B.row[B.row != B.col]]
    for r, cnt in {n - 1: n - 1, n // 2 + 17: 120_000, 70_001: 60_000}.items():
        c = rng.choice(np.setdiff1d(np.arange(n), [r], assume_unique=True), cnt, replace=False) if cnt < n - 1 else np.delete(np.arange(n), r)
        rows += [np.full(len(c), r), c]; cols += [c, np.full(len(c), r)]
    M = sp.coo_matrix((np.ones(sum(len(r) for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    M.sum_duplicates(); M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32)


@pytest.mark.parametrize("integer", [True, False], ids=["exact", "bound"])
def test_row_ranges(api, lib, integer):
    """Row ranges: half constant diagonals, half scattered columns (8192 + 8192 rows and a cut one row past a 2048-row chunk), the
    stencil + coupled rows of test_gpu_ranges, and the arrow matrix whose dense rows get a range of their own (automatic choice)."""
    rng = np.random.default_rng(404 + integer)
    cases = []
    for nh in (8192, 2049 + 2048):
        r1, c1 = _generated(api, nh, api.GEN_DIAGONALS, 300, 4)
        r2, c2 = _generated(api, nh, api.GEN_SCRAMBLED, 0, 6)
        cases.append((f"two classes {nh}", np.concatenate([r1, r2[1:] + r1[-1]]).astype(np.int32), np.concatenate([c1, c2 + nh]).astype(np.int32), 1))
    n, _, (rpm, cim, _) = mixed_system(rng, False, dims=(24, 26, 20))
    cases.append(("mixed stencil + couplings", rpm, cim, 1))
    cases.append(("arrow", *_arrow(rng), -1))
    for name, rp, ci, mode in cases:
        n = len(rp) - 1
        val, x = data(rng, rp, n, False, integer)
        A = api.CsrMatrix.from_csr(rp, ci, val)
        assert lib.lcg_hip_csr_set_ranges(A.h, mode) == 0
        xd = dev(x)
        y, kern = product(api, lib, A, xd, xd.dtype, n)
        assert lib.lcg_hip_csr_ranges(A.h, 0, None) >= 2 and kern.startswith("rows [0, "), (name, kern)
        if name == "arrow":
            assert "k_lr_" in kern, kern
        check(y, rp, ci, val, x, integer, name)
        A.destroy()


@pytest.mark.parametrize("integer", [True, False], ids=["exact", "bound"])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_spmv_op_all_forms(api, lib, cplx, integer):
    """lcg_hip_spmv_op: A, A^T, conj(A), A^H (the built copies), twice each; a row and a column longer than any window."""
    rng = np.random.default_rng(505 + 2 * cplx + integer)
    for n in (65, 2500):
        rp, col = _ragged(rng, n, n, 30, long_rows=[(7, 2400)] if n > 2400 else ())
        if n > 2400:
            col[rp[100]:rp[100] + 10] = 3          # a column of more entries than most
        val, x = data(rng, rp, n, cplx, integer, max_len=max_line(rp, col, n))
        A = api.CsrMatrix.from_csr(rp, col, val)
        xd = dev(x)
        for form in ("A", "AT", "conj", "AH"):
            orp, oci, ov = op_csr(rp, col, val, n, form)
            for rep in range(2):
                y, kern = product(api, lib, A, xd, xd.dtype, n, form)
                assert kern.startswith(("k_spmv_lds1 ", "k_spmv_ldsw ", "k_spmv_run1 ", "k_spmv_wave")), (n, form, kern)
                check(y, orp, oci, ov, x, integer, (n, form, rep, kern))
        A.destroy()


@pytest.mark.parametrize("integer", [True, False], ids=["exact", "bound"])
def test_coo_ingest_with_duplicates(api, lib, integer):
    """lcg_hip_csr_from_coo, row-sorted (device path) and shuffled (host sort), with repeated (row, column) pairs kept as terms:
    L_i counts the COO terms of row i."""
    rng = np.random.default_rng(606 + integer)
    n = 3000
    nnz = 40000
    row = rng.integers(0, n - 1, nnz).astype(np.int32)       # the last row stays empty
    col = rng.integers(0, n, nnz).astype(np.int32)
    dup = rng.integers(0, nnz, 3000)
    row = np.concatenate([row, row[dup]]); col = np.concatenate([col, col[dup]])
    order = np.argsort(row, kind="stable")
    rp = np.zeros(n + 1, np.int64); np.add.at(rp, row + 1, 1); rp = np.cumsum(rp).astype(np.int32)
    val, x = data(rng, rp, n, False, integer)
    v_in = np.empty_like(val); v_in[order] = val                 # val is in row-sorted order; v_in in input order
    for name, perm in (("sorted", order), ("shuffled", rng.permutation(len(row)))):
        A = api.CsrMatrix.from_coo(n, row[perm], col[perm], v_in[perm])
        xd = dev(x)
        y, kern = product(api, lib, A, xd, xd.dtype, n)
        assert kern.startswith(("k_spmv_lds1 ", "k_spmv_ldsw ")), (name, kern)
        check(y, rp, col[order], val, x, integer, (name, kern))
        A.destroy()


def _c64_case(rng, n, mean, long_min):
    lens = rng.poisson(mean, n).astype(np.int64)
    lens[rng.integers(0, n, n // 10)] = 0
    lens[0] = lens[-1] = 0
    lens[n // 3] = long_min; lens[n // 2] = long_min + 1
    rp = np.zeros(n + 1, np.int64); rp[1:] = np.cumsum(lens)
    return rp.astype(np.int32), rng.integers(0, n, rp[-1]).astype(np.int32)


def test_c64_all_forms_and_lane_counts(api, lib):
    """lcg_hip_spmv_c64 in all four forms on integer data (exact in fp32): W = 1 .. 64 lanes per row reached by the mean row length,
    entry pairs (copied) and single entries (adopted, odd nnz, not padded), rows of exactly long_min and long_min + 1 entries."""
    rng = np.random.default_rng(707)
    for W, mean in ((1, 0.6), (2, 2.5), (4, 6.0), (8, 12.0), (16, 24.0), (32, 48.0), (64, 100.0)):
        long_min = max(256, 64 * W)
        n = 4001
        rp, col = _c64_case(rng, n, mean, long_min)
        if rp[-1] % 2 == 0:         # odd nnz: the adopted copy must take single entries
            rp[-1] += 1; col = np.append(col, np.int32(5))
        p = X.int_bits(max_line(rp, col, n), "c64")
        val = X.int_values(rng, int(rp[-1]), p, True).astype(np.complex64)
        x = X.int_values(rng, n, p, True, zeros=0).astype(np.complex64)
        rpd, cid, vd = dev(rp), dev(col), dev(val)
        for adopt in (0, 1):
            A = api.CsrMatrix.from_csr_c64(rpd, cid, vd, adopt=bool(adopt)) if adopt else api.CsrMatrix.from_csr_c64(rp, col, val)
            xd = dev(x)
            for form, (layout, conj) in (("A", (0, 0)), ("AT", (1, 0)), ("conj", (0, 1)), ("AH", (1, 1))):
                y = nan_out(n, torch.complex64)
                assert lib.lcg_hip_spmv_c64(A.h, xd.data_ptr(), y.data_ptr(), layout, conj) == 0
                torch.cuda.synchronize()
                kern = lib.lcg_hip_csr_last_kernel(A.h).decode()
                assert kern.startswith("k_c64_rows<"), kern
                if form == "A":
                    assert kern.startswith(f"k_c64_rows<{W}>"), (W, mean, kern)
                    assert ("(single entries)" if adopt else "(entry pairs)") in kern, (adopt, kern)
                    assert (f"k_c64_long (1 long rows)" in kern), kern          # long_min + 1 only
                orp, oci, ov = op_csr(rp, col, val.astype(np.complex128), n, form)
                ye = X.exact_int_product(orp, oci, ov, x.astype(np.complex128))
                X.assert_exact(y.cpu().numpy().astype(np.complex128), ye, (W, adopt, form, kern))
            A.destroy()


# ------------------------------------------------------------------------------------------------ 4. non-finite x
def _family_matrices(api, lib, rng):
    """(name, handle maker, rp, col, ncols, expected kernel prefix): one matrix per real family."""
    out = []
    rp, col = _ragged(rng, 3001, 3001, 40, long_rows=[(5, 5000)])
    out.append(("wave", rp, col, 3001, lambda A: A.set_kernel(8), "k_spmv_wave"))
    out.append(("ldsw", rp, col, 3001, lambda A: A.set_kernel(-64), "k_spmv_ldsw"))
    rp1, col1 = _ragged(rng, 3001, 3001, 30)
    out.append(("lds1", rp1, col1, 3001, lambda A: A.set_kernel(-64), "k_spmv_lds1 "))
    out.append(("ldsp", rp1, col1, 3001, lambda A: (A.set_kernel(-64), lib.lcg_hip_csr_set_packed(A.h, 1)), "k_spmv_ldsp"))
    nn, rps, cis = _stencil((9, 7, 5), 1)
    out.append(("templates", rps, cis, nn, lambda A: (A.set_kernel(-64), lib.lcg_hip_csr_set_packed(A.h, 1)), "k_spmv_ldsp"))
    nn2, rps2, cis2 = _stencil((6, 9, 16), 1, True)
    out.append(("run1", rps2, cis2, nn2, lambda A: None, "k_spmv_run1 "))
    rpt, cit = _generated(api, 20000, api.GEN_ROW_RANDOM_BAND, 3000, 2)
    out.append(("tiled", rpt, cit, 20000, lambda A: lib.lcg_hip_csr_set_tiled(A.h, 1), "k_tile_spmv"))
    rpb, cib = _generated(api, 20000, api.GEN_SCRAMBLED, 0, 2)
    out.append(("binned", rpb, cib, 20000, lambda A: lib.lcg_hip_csr_set_binned(A.h, 1), "k_bin_expand"))
    L, nr = 5, 6400 + 13
    offs = np.sort(rng.choice(3000, L, replace=False))
    out.append(("run blocks", (np.arange(nr + 1) * L).astype(np.int32), (np.arange(nr)[:, None] + offs).ravel().astype(np.int32), nr + 3000,
                lambda A: (A.set_kernel(-64), lib.lcg_hip_csr_set_packed(A.h, 1)), "k_spmv_ldsp (LDS-staged, run blocks"))
    n0, rp0, ci0 = _stencil((14, 15, 16), 1, False)
    B = sp.kron(sp.csr_matrix((np.ones(len(ci0)), ci0, rp0), shape=(n0, n0)), np.ones((2, 2)), format="csr"); B.sort_indices()
    out.append(("long rows", B.indptr.astype(np.int32), B.indices.astype(np.int32), 2 * n0, lambda A: lib.lcg_hip_csr_set_packed(A.h, 1),
                "k_spmv_ldsp (LDS-staged, long rows"))
    r1, c1 = _generated(api, 8192, api.GEN_DIAGONALS, 300, 4)
    r2, c2 = _generated(api, 8192, api.GEN_SCRAMBLED, 0, 6)
    out.append(("ranges", np.concatenate([r1, r2[1:] + r1[-1]]).astype(np.int32), np.concatenate([c1, c2 + 8192]).astype(np.int32), 16384,
                lambda A: lib.lcg_hip_csr_set_ranges(A.h, 1), "rows [0, "))
    return out


def _specials(rng, col, ncols, count=6):
    """Columns that get NaN / +Inf / -Inf: column 0 and the last column (what masked lanes would read) and a few referenced ones."""
    cs = np.unique(np.concatenate([[0, ncols - 1], rng.choice(np.unique(col), count, replace=False)]))
    kinds = np.array([np.nan, np.inf, -np.inf])[np.arange(len(cs)) % 3]
    return cs, kinds


def _category(got, terms, rowid, ne, nrows, tag):
    """The category a real sum of `terms` (row ids `rowid`) has in any order: NaN if a term is NaN or +Inf meets -Inf, else +Inf /
    -Inf if such a term is there -- for the rows ne (got = the kernel's sums of those rows)."""
    has_nan = np.zeros(nrows, bool); np.logical_or.at(has_nan, rowid, np.isnan(terms))
    pos = np.zeros(nrows, bool); np.logical_or.at(pos, rowid, terms == np.inf)
    neg = np.zeros(nrows, bool); np.logical_or.at(neg, rowid, terms == -np.inf)
    want_nan = has_nan | (pos & neg)
    assert np.array_equal(np.isnan(got), want_nan[ne]), (tag, "NaN rows")
    assert np.array_equal(got == np.inf, (pos & ~want_nan)[ne]), (tag, "+Inf rows")
    assert np.array_equal(got == -np.inf, (neg & ~want_nan)[ne]), (tag, "-Inf rows")


def _nonfinite_check(yb, y0, rp, col, val, x_special, cs, tag, real=True):
    """Rows that do not reference the special columns: bitwise equal to the run with those x = 0; rows that do: the category of an
    ordered CSR sum -- for complex values per component, each a real sum of the products re(a) re(x), -im(a) im(x) (real part) and
    re(a) im(x), im(a) re(x) (imaginary part)."""
    lens = np.diff(rp)
    n = len(lens)
    rowid = np.repeat(np.arange(n), lens)
    hit = np.zeros(n, bool); hit[rowid[np.isin(col, cs)]] = True
    assert np.array_equal(yb[~hit].view(np.uint8), y0[~hit].view(np.uint8)), (tag, np.flatnonzero(~hit & ~(yb == y0))[:5])
    ne = np.flatnonzero(hit)
    with np.errstate(invalid="ignore", over="ignore"):
        if real:
            _category(yb[ne], val * x_special[col], rowid, ne, n, tag)
            return
        a = np.asarray(val, np.complex128); xc = np.asarray(x_special, np.complex128)[col]
        r2 = np.concatenate([rowid, rowid])
        _category(yb[ne].real, np.concatenate([a.real * xc.real, -(a.imag * xc.imag)]), r2, ne, n, tag + ("re",))
        _category(yb[ne].imag, np.concatenate([a.real * xc.imag, a.imag * xc.real]), r2, ne, n, tag + ("im",))


def test_nonfinite_x_stays_in_its_rows(api, lib):
    """NaN, +Inf and -Inf in x (column 0, the last column, referenced columns; explicitly stored zeros in the matrix) in every real
    family, c128 (row-block kernels and op forms) and c64: no masked or padding lane leaks them into another row."""
    rng = np.random.default_rng(808)
    for name, rp, col, ncols, force, want in _family_matrices(api, lib, rng):
        n = len(rp) - 1
        val, x = data(rng, rp, ncols, False, False)
        val[rng.random(len(val)) < 0.05] = 0.0
        cs, kinds = _specials(rng, col, ncols)
        xs = x.copy(); xs[cs] = kinds
        x0 = x.copy(); x0[cs] = 0.0
        A = api.CsrMatrix.from_csr(rp, col, val, n_cols=ncols)
        force(A)
        y0, k0 = product(api, lib, A, dev(x0), torch.float64, n)
        yb, kb = product(api, lib, A, dev(xs), torch.float64, n)
        assert kb.startswith(want) and k0 == kb, (name, kb)
        _nonfinite_check(yb.cpu().numpy(), y0.cpu().numpy(), rp, col, val, xs, cs, name)
        if name == "lds1":      # the product carrying its dot (k_spmv_lds1d): its y part
            A.set_kernel(0)
            ud = dev(np.ones(n))
            ys = []
            for xv in (x0, xs):
                y = nan_out(n, torch.float64); sums = (C.c_double * 2)()
                assert lib.lcg_hip_spmv_dot(A.h, dev(xv).data_ptr(), y.data_ptr(), ud.data_ptr(), sums) == 0
                ys.append(y.cpu().numpy())
            kd = lib.lcg_hip_csr_last_kernel(A.h).decode()
            assert kd.startswith("k_spmv_lds1d"), kd
            _nonfinite_check(ys[1], ys[0], rp, col, val, xs, cs, ("lds1d", kd))
        A.destroy()
    # c128: the row-block kernels and the built op copies
    rp, col = _ragged(rng, 2500, 2500, 30, long_rows=[(7, 2400)])
    val, x = data(rng, rp, 2500, True, False)
    val[rng.random(len(val)) < 0.05] = 0
    cs, kinds = _specials(rng, col, 2500)
    xs = x.copy(); xs[cs] = kinds
    x0 = x.copy(); x0[cs] = 0
    A = api.CsrMatrix.from_csr(rp, col, val)
    for var in (8, -64, 0):
        A.set_kernel(var)
        for form in ("A", "AT", "conj", "AH"):
            orp, oci, ov = op_csr(rp, col, val, 2500, form)
            y0, _ = product(api, lib, A, dev(x0), torch.complex128, 2500, form)
            yb, kb = product(api, lib, A, dev(xs), torch.complex128, 2500, form)
            _nonfinite_check(yb.cpu().numpy(), y0.cpu().numpy(), orp, oci, ov, xs, cs, ("c128", var, form, kb), real=False)
    A.destroy()
    # c64: pairs and single entries
    for mean in (2.5, 24.0):
        rp, col = _c64_case(rng, 3001, mean, 256 if mean < 5 else 1024)
        if rp[-1] % 2 == 0:
            rp[-1] += 1; col = np.append(col, np.int32(5))
        val = (rng.standard_normal(rp[-1]) + 1j * rng.standard_normal(rp[-1])).astype(np.complex64)
        val[rng.random(len(val)) < 0.05] = 0
        x = (rng.standard_normal(3001) + 1j * rng.standard_normal(3001)).astype(np.complex64)
        cs, kinds = _specials(rng, col, 3001)
        xs = x.copy(); xs[cs] = kinds
        x0 = x.copy(); x0[cs] = 0
        rpd, cid, vd = dev(rp), dev(col), dev(val)
        for adopt in (False, True):
            A = api.CsrMatrix.from_csr_c64(rpd, cid, vd, adopt=True) if adopt else api.CsrMatrix.from_csr_c64(rp, col, val)
            for form, (layout, conj) in (("A", (0, 0)), ("AT", (1, 0)), ("conj", (0, 1)), ("AH", (1, 1))):
                ys = []
                for xv in (x0, xs):
                    y = nan_out(3001, torch.complex64)
                    assert lib.lcg_hip_spmv_c64(A.h, dev(xv).data_ptr(), y.data_ptr(), layout, conj) == 0
                    torch.cuda.synchronize()
                    ys.append(y.cpu().numpy())
                kern = lib.lcg_hip_csr_last_kernel(A.h).decode()
                orp, oci, ov = op_csr(rp, col, val, 3001, form)
                _nonfinite_check(ys[1], ys[0], orp, oci, ov, xs, cs, ("c64", mean, adopt, form, kern), real=False)
            A.destroy()


# ------------------------------------------------------------------------------------------------ 5. rewriting an adopted matrix
def _adopted(api, rp, col, val, adopt):
    """Device arrays the handle adopts (adopt 2: views of longer tensors, >= 64 readable bytes behind col and val)."""
    pad = 32 if adopt == 2 else 0
    rpd = dev(rp)
    colb = torch.zeros(len(col) + pad, dtype=torch.int32, device="cuda"); colb[:len(col)] = dev(col)
    valb = torch.zeros(len(val) + pad, dtype=torch.complex128 if np.iscomplexobj(val) else torch.float64, device="cuda")
    valb[:len(val)] = dev(val)
    cold, vald = colb[:len(col)], valb[:len(val)]
    return api.CsrMatrix.from_csr(rpd, cold, vald, adopt=adopt), cold, vald


def _all_forms(api, lib, A, rp, col, val, x, cplx, tag, want):
    n = len(rp) - 1
    xd = dev(x)
    for form in ("A", "AT", "conj", "AH"):
        y, kern = product(api, lib, A, xd, xd.dtype, n, form)
        if form == "A":
            assert want in kern, (tag, kern)
        orp, oci, ov = op_csr(rp, col, val, n, form)
        check(y, orp, oci, ov, x, True, tag + (form, kern))
    if not cplx:
        ye = X.exact_int_product(rp, col, val, x)
        y = nan_out(n, torch.float64)
        sums = (C.c_double * 2)()
        assert lib.lcg_hip_spmv_dot(A.h, xd.data_ptr(), y.data_ptr(), xd.data_ptr(), sums) == 0
        X.assert_exact(y.cpu().numpy(), ye, tag + ("dot",))


@pytest.mark.parametrize("adopt", [1, 2])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_rewriting_an_adopted_matrix(api, lib, cplx, adopt):
    """The protocol of include/lcg_hip.h: rewrite the values, then the columns (same row pointers) of an adopted matrix, call
    set_packed / set_tiled / set_binned / set_ranges (A, 0) and then (A, -1) -- or (A, 1) to force the family again -- and every form
    (A, A^T, conj(A), A^H, the product carrying the dot) follows the new arrays exactly.  The op(A) copies built before the rewrite
    must not answer after it; on the small matrix (no plans of its own) each rewrite calls only ONE of the four setters -- each of
    them in one of the four parametrisations -- since any one of them frees the op(A) copies."""
    rng = np.random.default_rng(909 + 2 * cplx + adopt)
    setters = (lib.lcg_hip_csr_set_packed, lib.lcg_hip_csr_set_tiled, lib.lcg_hip_csr_set_binned, lib.lcg_hip_csr_set_ranges)
    rp0, col0 = _ragged(rng, 3001, 3001, 30)
    cases = [("small", rp0, col0, None, "k_spmv_")]
    if not cplx and adopt == 2:     # (adopt 1 promises no slack behind the arrays: the one-window kernels and their copies stay out)
        nn, rps, cis = _stencil((20, 33, 64), 1)
        cases.append(("packed", rps, cis, lib.lcg_hip_csr_set_packed, "k_spmv_ldsp"))
        cases.append(("tiled", *_generated(api, 20000, api.GEN_ROW_RANDOM_BAND, 3000, 3), lib.lcg_hip_csr_set_tiled, "k_tile_spmv"))
        cases.append(("binned", *_generated(api, 20000, api.GEN_SCRAMBLED, 0, 3), lib.lcg_hip_csr_set_binned, "k_bin_expand"))
        r1, c1 = _generated(api, 8192, api.GEN_DIAGONALS, 300, 4)
        r2, c2 = _generated(api, 8192, api.GEN_SCRAMBLED, 0, 6)
        cases.append(("ranges", np.concatenate([r1, r2[1:] + r1[-1]]).astype(np.int32), np.concatenate([c1, c2 + 8192]).astype(np.int32),
                      lib.lcg_hip_csr_set_ranges, "rows [0, "))
    for name, rp, col, force, want in cases:
        n = len(rp) - 1
        p = X.int_bits(max_line(rp, col, n) + 2, "c128" if cplx else "f64")
        val = X.int_values(rng, len(col), p, cplx); x = X.int_values(rng, n, p, cplx, zeros=0)
        A, cold, vald = _adopted(api, rp, col, val, adopt)
        if force is not None:
            assert force(A.h, 1) == 0
        _all_forms(api, lib, A, rp, col, val, x, cplx, (name, adopt, "before"), want)
        # 1. new values
        val2 = X.int_values(rng, len(col), p, cplx)
        vald.copy_(dev(val2)); torch.cuda.synchronize()
        step = setters if force is not None else (setters[(adopt + cplx) % 4],)
        for s in step:
            assert s(A.h, 0) == 0
        for s in step:
            assert s(A.h, -1) == 0
        if force is not None:
            assert force(A.h, 1) == 0
        _all_forms(api, lib, A, rp, col, val2, x, cplx, (name, adopt, "new values"), want)
        # 2. new columns (same row pointers, in range; the family's column pattern kept: shifted by one or jittered by a few)
        if name in ("packed", "ranges"):
            col2 = np.minimum(col.astype(np.int64) + 1, n - 1).astype(np.int32)
        else:
            col2 = np.clip(col.astype(np.int64) + rng.integers(-2, 3, len(col)), 0, n - 1).astype(np.int32)
        cold.copy_(dev(col2)); torch.cuda.synchronize()
        step = setters if force is not None else (setters[(adopt + cplx + 2) % 4],)
        for s in step:
            assert s(A.h, 0) == 0
        for s in step:
            assert s(A.h, -1) == 0
        if force is not None:
            assert force(A.h, 1) == 0
        _all_forms(api, lib, A, rp, col2, val2, x, cplx, (name, adopt, "new columns"), want)
        A.destroy()
