"""-m gpu: the batched triangular applies (lcg_hip_ic0_solve_multi, lcg_hip_ilu0_solve_multi; csr_tri_multi.hip), without a
tolerance: column j of a batched apply has the bits of the single-vector solve of column j -- for k = 2, 4, 8, both factors,
which = 0, 1, 2, the exact level-scheduled solves (narrow groups, a 3000-level chain, a level wider than 1024 rows, every level
forced into a wide launch) and s = 1, 2, 3, `levels` sweeps (rows at the edges of a workgroup, slices at the edges of the LDS
window, a dense row) -- whatever the other columns hold, whatever k is, from call to call.  Then the work vectors that grow, and
the error returns.  The systems and what each is there for: tests/tri_multi_cases.py, shown by tests/test_tri_multi_cases_cpu.py."""
import numpy as np
import pytest

import tri_multi_cases as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
E_ARG = T.E_ARG


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


def block(n, k, seed=3):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, k)))


def check_columns(A, factor, X, tag):
    """Every which: the batched apply of X against the single-vector solve of each column, bit for bit.  Returns the batched
    results by which."""
    out = {}
    for which in (0, 1, 2):
        got = T.batched(torch, A, factor, which, X)
        want = T.single(torch, A, factor, which, X)
        bad = [j for j in range(X.shape[1]) if not T.same_bits(got[:, j], want[:, j])]
        assert not bad, (tag, "which", which, "columns", bad, float(np.nanmax(np.abs(got - want))))
        out[which] = got
    return out


# ------------------------------------------------------------------------------------------ 1. exact solves
@pytest.mark.parametrize("name", ["laplace64", "chain3000", "layered"])
@pytest.mark.parametrize("factor", T.FACTORS)
def test_exact_solves_have_the_single_solves_bits(api, factor, name):
    rp, ci, v = T.system(factor, name)
    n = len(rp) - 1
    A = T.build(api, factor, (rp, ci, v))
    try:
        inf = T.info(A, factor)
        if name == "chain3000":
            assert inf["lo"] == inf["up"] == 3000 and inf["launches"] == 2         # one narrow launch per triangle
        if name == "layered":
            assert inf["launches"] == (5 if factor == "ic0" else 6)                 # narrow run, the wide level, narrow run (L^T: wide first)
        for k in T.KS:
            check_columns(A, factor, block(n, k), (factor, name, k))
    finally:
        A.destroy()


@pytest.mark.parametrize("factor", T.FACTORS)
def test_exact_solves_with_every_level_a_wide_launch(api, lib, factor):
    rp, ci, v = T.system(factor, "laplace64")
    n = len(rp) - 1
    A = T.build(api, factor, (rp, ci, v))
    try:
        X = block(n, 8)
        merged = T.batched(torch, A, factor, 2, X)
        T.schedule_for_test(lib, A, factor, 0)
        inf = T.info(A, factor)
        assert inf["launches"] == inf["lo"] + inf["up"] == 2 * 127
        for k in T.KS:
            got = check_columns(A, factor, X[:, :k].copy(), (factor, "wide", k))
            assert T.same_bits(got[2], merged[:, :k])                               # and the grouping changes no bit
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 2. sweeps
@pytest.mark.parametrize("name", T.SWEEP_SYSTEMS)
@pytest.mark.parametrize("factor", T.FACTORS)
def test_sweeps_have_the_single_sweeps_bits(api, factor, name):
    """s = 1, 2, 3: against the single-vector sweeps.  s = levels: the exact batched solve's bits (which the tests above hold to
    the single exact solves)."""
    rp, ci, v = T.system(factor, name)
    n = len(rp) - 1
    A = T.build(api, factor, (rp, ci, v))
    try:
        inf = T.info(A, factor)
        ks = (int(name[6:]),) if name.startswith("window") else T.KS                # a window matrix is made for one k
        X = block(n, 8, seed=9)
        exact = {k: {w: T.batched(torch, A, factor, w, X[:, :k].copy()) for w in (0, 1, 2)} for k in ks}
        for s in (1, 2, 3):
            T.set_sweeps(A, factor, s)
            for k in ks:
                check_columns(A, factor, X[:, :k].copy(), (factor, name, "s", s, "k", k))
        levels = {0: inf["lo"], 1: inf["up"], 2: max(inf["lo"], inf["up"])}
        for which in (0, 1, 2):
            T.set_sweeps(A, factor, max(levels[which], 1))
            for k in ks:
                got = T.batched(torch, A, factor, which, X[:, :k].copy())
                assert T.same_bits(got, exact[k][which]), (factor, name, which, k, levels[which])
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("sweeps", [0, 3])
@pytest.mark.parametrize("factor", T.FACTORS)
def test_a_column_does_not_depend_on_its_neighbours(api, factor, sweeps):
    rp, ci, v = T.system(factor, "laplace64")
    n = len(rp) - 1
    A = T.build(api, factor, (rp, ci, v))
    try:
        T.set_sweeps(A, factor, sweeps)
        X = block(n, 8, seed=21)
        for which in (0, 1, 2):
            ref = T.batched(torch, A, factor, which, X)
            assert T.same_bits(T.batched(torch, A, factor, which, X), ref)          # two calls
            # column 0 at k = 2, 4, 8
            for k in (2, 4):
                assert T.same_bits(T.batched(torch, A, factor, which, X[:, :k].copy())[:, 0], ref[:, 0]), (which, k)
            # neighbours of NaN, of +-Inf in a few rows, and of zeros
            P = X.copy()
            P[:, 1] = np.nan
            P[5, 2] = np.inf; P[n // 2, 2] = -np.inf; P[n - 1, 2] = np.inf
            P[:, 3] = 0.0
            got = T.batched(torch, A, factor, which, P)
            for j in (0, 4, 5, 6, 7):
                assert T.same_bits(got[:, j], ref[:, j]), (which, j)
            assert np.isnan(got[:, 1]).all() and not np.isfinite(got[:, 2]).all()
            assert T.same_bits(got[:, 3], np.zeros(n)) or not got[:, 3].any()       # zeros in, zeros out (their sign aside)
            for k in (2, 4):                                                        # the poisoned columns beside column 0 at every k
                assert T.same_bits(T.batched(torch, A, factor, which, P[:, :k].copy())[:, 0], ref[:, 0]), (which, k)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 4. the work vectors
@pytest.mark.parametrize("factor", T.FACTORS)
def test_sweep_count_changes_and_growing_k(api, factor):
    """The k-wide work vectors are made at the first batched apply that needs them, grow with k, survive a change of the sweep
    count, and are counted by the info entry."""
    rp, ci, v = T.system(factor, "laplace64")
    n = len(rp) - 1
    A = T.build(api, factor, (rp, ci, v))
    try:
        X = block(n, 8, seed=33)
        b0 = T.info(A, factor)["bytes"]
        check_columns(A, factor, X[:, :2].copy(), (factor, "exact k=2"))            # lo's result for which = 2, 2 wide
        b1 = T.info(A, factor)["bytes"]
        assert b1 - b0 == 8 * n * 2, (b0, b1)
        T.set_sweeps(A, factor, 2)
        b1s = T.info(A, factor)["bytes"]                                            # (the single path's own two sweep vectors)
        check_columns(A, factor, X[:, :2].copy(), (factor, "s=2 k=2"))              # + the two sweep vectors, 2 wide
        assert T.info(A, factor)["bytes"] - b1s == 2 * 8 * n * 2
        T.set_sweeps(A, factor, 5)                                                  # a larger count after a smaller one
        check_columns(A, factor, X[:, :4].copy(), (factor, "s=5 k=4"))              # regrown to 4 wide
        check_columns(A, factor, X, (factor, "s=5 k=8"))                            # and to 8
        b8 = T.info(A, factor)["bytes"]
        check_columns(A, factor, X[:, :2].copy(), (factor, "s=5 k=2 again"))        # a smaller k afterwards: nothing changes
        assert T.info(A, factor)["bytes"] == b8 and b8 - b1s == 3 * 8 * n * 8 - 8 * n * 2
        T.set_sweeps(A, factor, 0)                                                  # exact again after sweeps
        check_columns(A, factor, X, (factor, "exact k=8"))
        T.set_sweeps(A, factor, 1)
        check_columns(A, factor, X[:, :4].copy(), (factor, "s=1 k=4"))
        (A.build_ic0 if factor == "ic0" else A.build_ilu0)()                        # a rebuild frees them with the factor
        assert T.info(A, factor)["bytes"] == b0
        check_columns(A, factor, X[:, :4].copy(), (factor, "rebuilt k=4"))
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 5. error returns
@pytest.mark.parametrize("factor", T.FACTORS)
def test_error_returns_leave_y_untouched_and_the_library_usable(api, lib, factor, case1kc):
    rp, ci, v = T.system(factor, "spd129")
    n = len(rp) - 1
    fn = lib.lcg_hip_ic0_solve_multi if factor == "ic0" else lib.lcg_hip_ilu0_solve_multi
    name = "lcg_hip_ic0_solve_multi" if factor == "ic0" else "lcg_hip_ilu0_solve_multi"
    A = T.build(api, factor, (rp, ci, v))
    bare = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        k = 4
        X = block(n, k)
        good = T.batched(torch, A, factor, 2, X)
        Xd = torch.from_numpy(X).cuda()
        big = torch.full((2 * n * k + 2,), 7.0, dtype=torch.float64, device="cuda")
        Yd = big[:n * k]
        assert Xd.data_ptr() % 16 == 0 and Yd.data_ptr() % 16 == 0

        def refused(rc, *words):
            assert rc == E_ARG, rc
            err = lib.lcg_hip_last_error().decode()
            assert name + ":" in err and all(w in err for w in words), err
            torch.cuda.synchronize()
            assert bool((big == 7.0).all())                                         # Y untouched
            assert T.same_bits(T.batched(torch, A, factor, 2, X), good)             # and the library still serves

        for bad_k in (0, 1, 3, 5, 16, -2):
            refused(fn(A.h, bad_k, 2, Xd.data_ptr(), Yd.data_ptr()), "k must be 2, 4 or 8")
        refused(fn(A.h, k, 2, None, Yd.data_ptr()), "null")
        refused(fn(A.h, k, 2, Xd.data_ptr(), None), "null")
        refused(fn(A.h, k, 2, Xd.data_ptr() + 8, Yd.data_ptr()), "16-byte aligned")
        refused(fn(A.h, k, 2, Xd.data_ptr(), Yd.data_ptr() + 8), "16-byte aligned")
        refused(fn(None, k, 2, Xd.data_ptr(), Yd.data_ptr()), "handle is null")
        for which in (3, -1):
            refused(fn(A.h, k, which, Xd.data_ptr(), Yd.data_ptr()), "which")
        # X and Y overlapping: the same block, and blocks that share their last / first 16 bytes
        refused(fn(A.h, k, 2, Yd.data_ptr(), Yd.data_ptr()), "overlap")
        refused(fn(A.h, k, 2, big.data_ptr() + 8 * (n * k - 2), Yd.data_ptr()), "overlap")
        refused(fn(A.h, k, 2, Yd.data_ptr(), big.data_ptr() + 8 * (n * k - 2)), "overlap")
        refused(fn(bare.h, k, 2, Xd.data_ptr(), Yd.data_ptr()), "no factor")
        # other kinds of handle
        nc, rpc, cic, vc = case1kc[:4]
        Ac = api.CsrMatrix.from_csr(rpc, cic, vc)
        Ac.build_ic0() if factor == "ic0" else Ac.build_ilu0()
        refused(fn(Ac.h, k, 2, Xd.data_ptr(), Yd.data_ptr()), "complex")
        Ac.destroy()
        A64 = api.CsrMatrix.from_csr_c64(rpc, cic, vc.astype(np.complex64))
        refused(fn(A64.h, k, 2, Xd.data_ptr(), Yd.data_ptr()), "complex64")
        A64.destroy()
        D = api.DenseMatrix.from_array(np.eye(8))
        rc = fn(D.h, k, 2, Xd.data_ptr(), Yd.data_ptr())
        assert rc == E_ARG and "dense" in lib.lcg_hip_last_error().decode().lower()
        D.destroy()
        assert T.same_bits(T.batched(torch, A, factor, 2, X), good)
        # adjacent blocks do not overlap
        assert fn(A.h, k, 2, Yd.data_ptr(), big.data_ptr() + 8 * n * k) == 0
        torch.cuda.synchronize()
    finally:
        bare.destroy()
        A.destroy()


def test_python_front_refuses_malformed_blocks(api):
    rp, ci, v = T.system("ic0", "spd129")
    A = T.build(api, "ic0", (rp, ci, v))
    try:
        X = torch.zeros((129, 4), dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            A.ic0_solve_multi(X, torch.zeros((129, 2), dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            A.ic0_solve_multi(X.float(), X.float())
        with pytest.raises(api.LcgHipError):
            A.ilu0_solve_multi(X, torch.zeros_like(X))                              # no ILU(0) factor on this handle
    finally:
        A.destroy()
