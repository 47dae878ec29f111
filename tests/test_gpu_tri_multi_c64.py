"""-m gpu: the batched complex64 IC(0) apply (clcg_hip_ic0_solve_multi_c64; csr_tri_multi.hip's IcmC64 instantiations), without a
tolerance: column j of a batched apply has the bits of lcg_hip_ic0_solve_c64 on column j alone (the arrays compared as uint64) -- for
k = 2, 4, 8, which = 0, 1, 2, the exact level-scheduled solves (narrow groups, a 3000-level chain, a level wider than 1024 rows,
every level forced into a wide launch) and s = 1, 2, 3, 5 sweeps (rows at the edges of a workgroup, slices at the edges of the LDS
window, a dense row) -- whatever the other columns hold, wherever the column stands, whatever k is, from call to call.  Then the
work vectors that grow, and the refusals.  The systems: tests/tri_multi_c64_cases.py, shown by tests/test_tri_multi_c64_cases_cpu.py."""
import numpy as np
import pytest

import tri_multi_c64_cases as Z
import tri_multi_cases as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
E_ARG = Z.E_ARG
NAME = "clcg_hip_ic0_solve_multi_c64"


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


def check_columns(lib, A, X, tag, whiches=(0, 1, 2)):
    """The batched apply of X against the single-vector solve of each column, bit for bit.  Returns the batched results by which."""
    out = {}
    for which in whiches:
        got = Z.batched(torch, lib, A, which, X)
        want = Z.single(torch, lib, A, which, X)
        bad = [j for j in range(X.shape[1]) if not Z.same_bits(got[:, j], want[:, j])]
        assert not bad, (tag, "which", which, "columns", bad, float(np.nanmax(np.abs(got - want))))
        out[which] = got
    return out


# ------------------------------------------------------------------------------------------ 1. exact solves
@pytest.mark.parametrize("name", Z.EXACT_SYSTEMS)
def test_exact_solves_have_the_single_solves_bits(api, lib, name):
    rp, ci, v = Z.system(name)
    n = len(rp) - 1
    A = Z.build(api, (rp, ci, v))
    try:
        inf = A.ic0_info()
        if name == "chain3000":
            assert inf["levels_lower"] == inf["levels_upper"] == 3000 and inf["launches_per_apply"] == 2
        if name == "layered":
            assert inf["launches_per_apply"] == 5           # narrow run, the wide level, narrow run (L^T: wide first)
        for k in Z.KS:
            check_columns(lib, A, Z.cblock(n, k), (name, k))
    finally:
        A.destroy()


@pytest.mark.parametrize("name", Z.EXACT_SYSTEMS)
def test_exact_solves_with_every_level_a_wide_launch(api, lib, name):
    rp, ci, v = Z.system(name)
    n = len(rp) - 1
    A = Z.build(api, (rp, ci, v))
    try:
        X = Z.cblock(n, 8)
        merged = {w: Z.batched(torch, lib, A, w, X) for w in (0, 1, 2)}
        assert lib.lcg_hip_csr_ic0_schedule_for_test(A.h, 0) == 0
        inf = A.ic0_info()
        assert inf["launches_per_apply"] == inf["levels_lower"] + inf["levels_upper"]
        if name == "chain3000":                             # 6000 launches per apply: one k, which = 2 alone
            assert Z.same_bits(check_columns(lib, A, X[:, :4].copy(), (name, "wide", 4), whiches=(2,))[2], merged[2][:, :4])
            return
        for k in Z.KS:
            got = check_columns(lib, A, X[:, :k].copy(), (name, "wide", k))
            for w in (0, 1, 2):
                assert Z.same_bits(got[w], merged[w][:, :k])                        # and the grouping changes no bit
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 2. sweeps
@pytest.mark.parametrize("name", Z.SWEEP_SYSTEMS)
def test_sweeps_have_the_single_sweeps_bits(api, lib, name):
    """s = 1, 2, 3, 5 (five: both sweep buffers, twice) against the single-vector sweeps, at every k, every which."""
    rp, ci, v = Z.system(name)
    n = len(rp) - 1
    A = Z.build(api, (rp, ci, v))
    try:
        X = Z.cblock(n, 8, seed=9)
        for s in (1, 2, 3, 5):
            A.ic0_set_sweeps(s)
            for k in Z.KS:
                check_columns(lib, A, X[:, :k].copy(), (name, "s", s, "k", k))
    finally:
        A.destroy()


def test_levels_sweeps_give_the_exact_solves_bits(api, lib):
    rp, ci, v = Z.system("layered")
    n = len(rp) - 1
    A = Z.build(api, (rp, ci, v))
    try:
        inf = A.ic0_info()
        X = Z.cblock(n, 8, seed=10)
        exact = {w: Z.batched(torch, lib, A, w, X) for w in (0, 1, 2)}
        levels = {0: inf["levels_lower"], 1: inf["levels_upper"], 2: max(inf["levels_lower"], inf["levels_upper"])}
        for which in (0, 1, 2):
            A.ic0_set_sweeps(levels[which])
            assert Z.same_bits(Z.batched(torch, lib, A, which, X), exact[which]), (which, levels[which])
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 3. independence
FILLS = {"nan": complex(np.nan, np.nan), "inf": complex(np.inf, -np.inf), "1e30": complex(1e30, -1e30), "zero": 0.0}


@pytest.mark.parametrize("sweeps", [0, 3])
def test_a_column_does_not_depend_on_its_neighbours_or_its_place(api, lib, sweeps):
    rp, ci, v = Z.system("laplace64")
    n = len(rp) - 1
    A = Z.build(api, (rp, ci, v))
    try:
        A.ic0_set_sweeps(sweeps)
        x = Z.cblock(n, 1, seed=21)[:, 0]
        for which in (0, 1, 2):
            want = Z.single(torch, lib, A, which, x[:, None].copy())[:, 0]
            for k in Z.KS:
                for pos in range(k):
                    for fill in (("nan", "inf") if (pos + k) % 2 else ("1e30", "zero")):       # every fill at every k, half the places each
                        P = np.full((n, k), FILLS[fill], np.complex64)
                        P[:, pos] = x
                        got = Z.batched(torch, lib, A, which, P)
                        assert Z.same_bits(got[:, pos], want), (which, k, pos, fill)
                        if fill == "nan":
                            assert np.isnan(np.delete(got, pos, axis=1).view(np.float32)).all()
                        if fill == "zero":
                            assert not np.delete(got, pos, axis=1).any()
            # mixed neighbours in one block, twice
            P = Z.cblock(n, 8, seed=22)
            P[:, 0] = x
            P[:, 1] = FILLS["nan"]; P[5, 2] = FILLS["inf"]; P[n - 1, 2] = FILLS["inf"]; P[:, 3] = 0.0; P[:, 5] = FILLS["1e30"]
            a, b = Z.batched(torch, lib, A, which, P), Z.batched(torch, lib, A, which, P)
            assert Z.same_bits(a, b) and Z.same_bits(a[:, 0], want), which
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 4. the work vectors
def test_growing_k_and_sweep_count_changes(api, lib):
    """k = 2 -> 8 -> 4 on one factor with the sweep count changed in between, then exact again: the same bits as the single solves
    throughout, and the info entry's bytes grow once per work vector and once with k (8 bytes per element and column)."""
    rp, ci, v = Z.system("laplace64")
    n = len(rp) - 1
    A = Z.build(api, (rp, ci, v))
    try:
        X = Z.cblock(n, 8, seed=33)
        b0 = A.ic0_info()["bytes"]
        check_columns(lib, A, X[:, :2].copy(), "exact k=2")                         # lo's result for which = 2, 2 wide
        b1 = A.ic0_info()["bytes"]
        assert b1 - b0 == 8 * n * 2, (b0, b1)
        A.ic0_set_sweeps(2)
        b1s = A.ic0_info()["bytes"]                                                 # (the single path's own two sweep vectors)
        check_columns(lib, A, X[:, :2].copy(), "s=2 k=2")                           # + the two sweep vectors, 2 wide
        assert A.ic0_info()["bytes"] - b1s == 2 * 8 * n * 2
        A.ic0_set_sweeps(5)
        check_columns(lib, A, X, "s=5 k=8")                                         # regrown to 8 wide
        b8 = A.ic0_info()["bytes"]
        assert b8 - b1s == 3 * 8 * n * 8 - 8 * n * 2
        A.ic0_set_sweeps(3)
        check_columns(lib, A, X[:, :4].copy(), "s=3 k=4")                           # a smaller k afterwards: nothing changes
        assert A.ic0_info()["bytes"] == b8
        A.ic0_set_sweeps(0)                                                         # exact again after sweeps
        check_columns(lib, A, X, "exact k=8")
        check_columns(lib, A, X[:, :2].copy(), "exact k=2 again")
        assert A.ic0_info()["bytes"] == b8 - (b1s - b1)                             # (set_sweeps(0) frees the single path's two)
        A.build_ic0()                                                               # a rebuild frees them with the factor
        assert A.ic0_info()["bytes"] == b0
        check_columns(lib, A, X[:, :4].copy(), "rebuilt k=4")
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_y_untouched_and_the_library_usable(api, lib, case1kc):
    rp, ci, v = Z.system("spd129")
    n = len(rp) - 1
    fn = lib.clcg_hip_ic0_solve_multi_c64
    A = Z.build(api, (rp, ci, v))
    bare = api.CsrMatrix.from_csr_c64(rp, ci, v)
    try:
        k = 4
        X = Z.cblock(n, k)
        good = Z.batched(torch, lib, A, 2, X)
        Xd = torch.from_numpy(X).cuda()
        big = torch.full((2 * n * k + 2,), complex(7.0, 7.0), dtype=torch.complex64, device="cuda")
        Yd = big[:n * k]
        assert Xd.data_ptr() % 16 == 0 and Yd.data_ptr() % 16 == 0

        def refused(rc, *words, name=NAME):
            assert rc == E_ARG, rc
            err = lib.lcg_hip_last_error().decode()
            assert name in err and all(w in err for w in words), err
            torch.cuda.synchronize()
            assert bool((big == complex(7.0, 7.0)).all())                           # Y untouched
            assert Z.same_bits(Z.batched(torch, lib, A, 2, X), good)                # and the next good call works

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
        Areal = api.CsrMatrix.from_csr(rp, ci, v.real.astype(np.float64))
        Areal.build_ic0()
        refused(fn(Areal.h, k, 2, Xd.data_ptr(), Yd.data_ptr()), "real")
        Areal.destroy()
        nc, rpc, cic, vc = case1kc[:4]
        A128 = api.CsrMatrix.from_csr(rpc, cic, vc)
        A128.build_ic0()
        refused(fn(A128.h, k, 2, Xd.data_ptr(), Yd.data_ptr()), "complex128")
        A128.destroy()
        D = api.DenseMatrix.from_array(np.eye(8))
        rc = fn(D.h, k, 2, Xd.data_ptr(), Yd.data_ptr())
        assert rc == E_ARG and "dense" in lib.lcg_hip_last_error().decode().lower()
        D.destroy()
        torch.cuda.synchronize()
        assert bool((big == complex(7.0, 7.0)).all())
        # the real entry on the complex64 handle refuses as before
        refused(lib.lcg_hip_ic0_solve_multi(A.h, k, 2, Xd.data_ptr(), Yd.data_ptr()), "complex64", name="lcg_hip_ic0_solve_multi")
        # adjacent blocks do not overlap
        assert fn(A.h, k, 2, Yd.data_ptr(), big.data_ptr() + 8 * n * k) == 0
        torch.cuda.synchronize()
    finally:
        bare.destroy()
        A.destroy()


def test_python_front(api, lib):
    rp, ci, v = Z.system("spd129")
    A = Z.build(api, (rp, ci, v))
    try:
        Xh = Z.cblock(129, 4, seed=4)
        X = torch.from_numpy(Xh).cuda()
        Y = torch.zeros_like(X)
        A.ic0_solve_multi_c64(X, Y)
        api.synchronize()
        assert Z.same_bits(Y.cpu().numpy(), Z.single(torch, lib, A, 2, Xh))
        with pytest.raises(ValueError):
            A.ic0_solve_multi_c64(X, torch.zeros((129, 2), dtype=torch.complex64, device="cuda"))
        with pytest.raises(ValueError):
            A.ic0_solve_multi_c64(X.to(torch.complex128), Y.to(torch.complex128))
        with pytest.raises(api.LcgHipError):
            A.ic0_solve_multi_c64(X, Y, which=5)
    finally:
        A.destroy()
