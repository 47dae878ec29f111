"""-m gpu: stretches of run blocks (csr_packed.hip: k_pk_stretch_flags / the stretch path of k_spmv_ldsp).  Consecutive full run blocks with the
same row length, the same offsets column - row and their entries one behind the other form a stretch; the blocks of the four longest
stretches derive their plan from their number instead of loading it.  Nothing of the result may change by a bit: every product here is
compared with the same kernel's product with the stretches switched off, with the plain row-block kernel's, and with exact row sums,
and the stretches found are those numpy finds in the CSR arrays."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
from sym_cases import expected_stretches

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WINDOW = 2240       # entries of the largest LDS window: a block of 64 rows beyond it does not take the packed kernel


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    return _lib.load()


def _regions(regs, tail=0):
    """CSR pattern of consecutive regions (blocks of 64 rows, offsets): row r of a region holds the columns r + offsets.  `tail` rows
    more continue the last region (a partial last block).  Returns n, rowptr, columns (one array per row)."""
    rows = []
    r = 0
    for i, (nblocks, offs) in enumerate(regs):
        m = 64 * nblocks + (tail if i == len(regs) - 1 else 0)
        offs = np.asarray(offs, np.int64)
        rows.extend(list((np.arange(r, r + m)[:, None] + offs[None, :]).astype(np.int32)))
        r += m
    rp = np.zeros(r + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in rows])
    return r, rp.astype(np.int32), rows


def _break(rows, r):
    """One entry of row r moved by one column (still sorted, still in range): the row's block is no run block any more."""
    c = rows[r].copy()
    k = len(c) // 2
    c[k] = c[k - 1] + 1 if c[k - 1] + 1 < c[k] else c[k] - 1
    assert not np.array_equal(c, rows[r]) and np.all(np.diff(c) > 0)
    rows[r] = c


def _count(top):
    return len(top), int(sum(top))


def _products(api, lib, A, n, ncols, x, forced=True):
    """y with the stretches on, off, and of the plain kernel (set_packed 0); the kernel's name and the stretches in use while on."""
    xd = torch.from_numpy(x).cuda()
    ys = [torch.full((n,), 5.0 + i, dtype=torch.float64, device="cuda") for i in range(3)]
    if forced:
        A.set_kernel(-64)
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    assert lib.lcg_hip_csr_set_run_stretches(A.h, 1) == 0
    A.spmv(xd, ys[0]); api.synchronize()
    kern = lib.lcg_hip_csr_last_kernel(A.h).decode()
    blocks = C.c_int64(-1)
    count = lib.lcg_hip_csr_run_stretches(A.h, C.byref(blocks))
    model_on = lib.lcg_hip_csr_last_traffic_model(A.h)
    assert lib.lcg_hip_csr_set_run_stretches(A.h, 0) == 0
    A.spmv(xd, ys[1]); api.synchronize()
    assert lib.lcg_hip_csr_run_stretches(A.h, None) == 0
    model_off = lib.lcg_hip_csr_last_traffic_model(A.h)
    assert lib.lcg_hip_csr_set_run_stretches(A.h, 1) == 0
    assert lib.lcg_hip_csr_set_packed(A.h, 0) == 0
    A.spmv(xd, ys[2]); api.synchronize()
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    return ys, kern, (count, blocks.value), (model_on, model_off)


def _check(api, lib, name, n, rp, rows, rng, dot=False):
    col = np.concatenate(rows).astype(np.int32)
    ncols = int(col.max()) + 1
    val = rng.standard_normal(len(col)); x = rng.standard_normal(ncols)
    A = api.CsrMatrix.from_csr(rp, col, val, n_cols=ncols)
    ys, kern, got, (model_on, model_off) = _products(api, lib, A, n, ncols, x)
    first = np.arange(0, n, 64)
    fits = int((rp[np.minimum(first + 64, n)].astype(np.int64) - rp[first]).max()) <= WINDOW
    want = _count(expected_stretches(rp, col, n)) if fits else (0, 0)    # (a block beyond the window: the windowed kernel answers, no packed form)
    print(f"{name}: {kern}; stretches (count, blocks) {got}, numpy {want}; traffic model on/off {model_on}/{model_off}")
    if fits:
        assert "run blocks" in kern, (name, kern)
    assert got == want, (name, got, want)
    if want[0]:     # per block of a stretch: 64 row pointers, two words, the groups of its columns; per stretch its table back
        assert model_off - model_on > (4 * 64 + 8) * want[1] and model_on > 8 * len(col), (name, model_on, model_off)
    else:
        assert model_on == model_off, name
    assert torch.equal(ys[0], ys[1]), (name, "stretches on / off")
    assert torch.equal(ys[0], ys[2]), (name, "stretches on / plain kernel")
    X.assert_rows(ys[0].cpu().numpy(), rp, col, val, x, (name,))
    if dot:
        # the kernel carrying the dot (automatic choice: rows long enough for 64-row blocks): y and both sums, u == x (the block's
        # own gathers where it holds its diagonal) and u elsewhere, the same bits with the stretches on and off
        A.set_kernel(0)
        xfull = torch.from_numpy(x).cuda()
        u = torch.from_numpy(rng.standard_normal(n)).cuda()
        out = {}
        for mode in (1, 0):
            assert lib.lcg_hip_csr_set_run_stretches(A.h, mode) == 0
            for uname, uu in (("u=x", xfull), ("u", u)):
                y = torch.empty(n, dtype=torch.float64, device="cuda")
                res = (C.c_double * 2)()
                assert lib.lcg_hip_spmv_dot(A.h, xfull.data_ptr(), y.data_ptr(), uu.data_ptr(), res) == 0
                k = lib.lcg_hip_csr_last_kernel(A.h).decode()
                assert "k_spmv_ldsp" in k and "carrying the dot" in k, (name, k)
                out[mode, uname] = (y, res[0], res[1])
        for uname in ("u=x", "u"):
            a, b = out[1, uname], out[0, uname]
            assert torch.equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], (name, uname, a[1:], b[1:])
            assert torch.equal(a[0], ys[0]), (name, uname)
    A.destroy()


@pytest.mark.parametrize("L", [1, 9, 33, 35, 40])
def test_one_stretch(api, lib, L):
    """A pure shifted-offset matrix of 37 full blocks and 5 rows more: one stretch of 37 blocks, the partial last block outside it.
    L = 1: one slot per wavefront at most; 9: the smallest window; 33 / 35: the headline's window and the largest; 40: the block of 64
    rows exceeds the LDS window, so the packed kernel (and with it the stretches) does not answer -- the three products still agree."""
    rng = np.random.default_rng(700 + L)
    offs = np.sort(rng.choice(np.arange(1, 5000), L, replace=False))
    if L >= 33:
        offs[0] = 0         # (with the diagonal among the offsets: the dot takes u from the block's gathers)
    n, rp, rows = _regions([(37, offs)], tail=5)
    assert n == 64 * 37 + 5
    if 64 * L <= WINDOW:
        assert _count(expected_stretches(rp, np.concatenate(rows), n)) == (1, 37)
    _check(api, lib, ("one stretch", L), n, rp, rows, rng, dot=L == 33)     # (35: the automatic choice takes 32-row blocks)


@pytest.mark.parametrize("same_L", [False, True], ids=["L 9 and 33", "L 33 twice"])
def test_two_stretches(api, lib, same_L):
    """Rows [0, 640) with one set of offsets, rows [640, 1600) with another -- of another length, or of the same length."""
    rng = np.random.default_rng(720 + same_L)
    o1 = np.sort(rng.choice(5000, 33 if same_L else 9, replace=False))
    o2 = np.sort(rng.choice(5000, 33, replace=False))
    assert not np.array_equal(o1, o2)
    n, rp, rows = _regions([(10, o1), (15, o2)])
    assert n == 1600 and _count(expected_stretches(rp, np.concatenate(rows), n)) == (2, 25)
    _check(api, lib, ("two stretches", same_L), n, rp, rows, rng, dot=same_L)


def test_one_broken_entry(api, lib):
    """One entry of block 7 of 40 off its diagonal: that block keeps columns of its own, blocks [0, 7) and [8, 40) are two stretches."""
    rng = np.random.default_rng(730)
    n, rp, rows = _regions([(40, np.sort(rng.choice(5000, 33, replace=False)))])
    _break(rows, 7 * 64 + 6)
    assert _count(expected_stretches(rp, np.concatenate(rows), n)) == (2, 39)
    _check(api, lib, "one broken entry", n, rp, rows, rng, dot=True)


def test_more_stretches_than_descriptors(api, lib):
    """Six regions of 3, 20, 5, 30, 4 and 12 blocks, their offsets alternating between two sets: six stretches, of which the four
    longest (30, 20, 12, 5 blocks) are taken; the blocks of the other two load their plan like any run block."""
    rng = np.random.default_rng(740)
    oa = np.sort(rng.choice(5000, 9, replace=False)); ob = np.sort(rng.choice(5000, 12, replace=False))
    n, rp, rows = _regions([(3, oa), (20, ob), (5, oa), (30, ob), (4, oa), (12, ob)], tail=17)
    assert _count(expected_stretches(rp, np.concatenate(rows), n)) == (4, 67)
    _check(api, lib, "six stretches", n, rp, rows, rng)


def test_a_single_run_block_is_no_stretch(api, lib):
    """5 run blocks, a broken block, ONE run block, a broken block, 6 run blocks: the single block is not taken (two blocks at least)."""
    rng = np.random.default_rng(750)
    n, rp, rows = _regions([(14, np.sort(rng.choice(5000, 33, replace=False)))])
    _break(rows, 5 * 64 + 63)
    _break(rows, 7 * 64)
    assert _count(expected_stretches(rp, np.concatenate(rows), n)) == (2, 11)
    _check(api, lib, "single run block", n, rp, rows, rng)


def test_generated_constant_diagonals(api, lib):
    """The generated constant-diagonal system (400,000 rows, 16 pairs, band 3000): one stretch covers the interior, the kernel is the
    run-block one, and a CG solve capped at 10 iterations, the dot carried in the product, walks the same bits with the stretches on
    and off."""
    nn, band = 400000, 3000
    B = api.CsrMatrix.generate(nn, 16, band, True, 5, 0.01)
    rp, col, val = B.arrays_to_host()
    rng = np.random.default_rng(760)
    x = rng.standard_normal(nn)
    ys, kern, got, _ = _products(api, lib, B, nn, nn, x)
    top = expected_stretches(rp, col, nn)
    want = _count(top)
    nblk = (nn + 63) // 64
    print(f"generated: {kern}; stretches (count, blocks) {got}, numpy {want}, blocks {nblk}")
    assert "run blocks" in kern, kern
    assert got == want, (got, want)
    # ONE stretch covers everything but the clipped bands at both ends (34 blocks allowed for the stretches of other L found there);
    # the library's count and blocks are numpy's (above), so its largest stretch is numpy's
    assert top[0] >= nblk - 2 * (band // 64 + 2) - 34, (top, nblk)
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    X.assert_rows(ys[0].cpu().numpy(), rp, col, val, x, ("generated",))
    # the capped solve (automatic kernel choice, so that the loop takes the product that carries the dot)
    B.set_kernel(0)
    b = torch.from_numpy(rng.standard_normal(nn)).cuda()
    runs = {}
    for mode in (1, 0):
        assert lib.lcg_hip_csr_set_run_stretches(B.h, mode) == 0
        m = torch.zeros(nn, dtype=torch.float64, device="cuda")
        info = api.lcg("lcg_hip_csr_ax", None, m, b, nn, api.lcg_default_parameters(epsilon=1e-300, abs_diff=1, max_iterations=10), B)
        k = lib.lcg_hip_csr_last_kernel(B.h).decode()
        assert "run blocks" in k and "carrying the dot" in k, k
        assert (lib.lcg_hip_csr_run_stretches(B.h, None) > 0) == (mode == 1)
        runs[mode] = (m, info)
    assert torch.equal(runs[1][0], runs[0][0])
    a, c = runs[1][1], runs[0][1]
    assert (a.ret, a.iterations, a.residual) == (c.ret, c.iterations, c.residual) and a.iterations == 10, (a, c)
    B.destroy()
