"""IC(0) on the MI355X (csr_ic0.hip): the device factor against the checker (tests/ic0_checker.py), the level-scheduled
triangular solves against SciPy, the PCG loops preconditioned by it against the checker's restatements, the error paths, and
the C++ sample of sample8's IC(0) leg."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import ic0_checker as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
E_ARG = -2003


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


# ------------------------------------------------------------------------------------------ fixtures
def tridiag(n, seed=5):
    rng = np.random.default_rng(seed)
    off = rng.uniform(-1.0, 1.0, n - 1)
    dia = 2.5 + rng.uniform(0.0, 1.0, n)
    rp = np.zeros(n + 1, np.int32)
    cols, vals = [], []
    for i in range(n):
        if i: cols.append(i - 1); vals.append(off[i - 1])
        cols.append(i); vals.append(dia[i])
        if i + 1 < n: cols.append(i + 1); vals.append(off[i])
        rp[i + 1] = len(cols)
    return rp, np.array(cols, np.int32), np.array(vals)


def arrow(n):
    """A dense last row and column on a diagonal: SPD, row n-1 of L is dense."""
    rp = np.zeros(n + 1, np.int32)
    cols, vals = [], []
    for i in range(n - 1):
        cols += [i, n - 1]; vals += [4.0 + (i % 7), 1.0 / (1 + i % 5)]
        rp[i + 1] = len(cols)
    cols += list(range(n)); vals += [1.0 / (1 + i % 5) for i in range(n - 1)] + [float(n)]
    rp[n] = len(cols)
    return rp, np.array(cols, np.int32), np.array(vals)


def laplace3d(k):
    import scipy.sparse as sp
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(k, k))
    I = sp.identity(k)
    A = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def shuffled_with_duplicates(rp, ci, v, seed=11):
    """The same matrix with every row's entries in random order and some entries split in two."""
    rng = np.random.default_rng(seed)
    nrp, nc, nv = [0], [], []
    for i in range(len(rp) - 1):
        c, x = list(ci[rp[i]:rp[i + 1]]), list(v[rp[i]:rp[i + 1]])
        for q in range(len(c)):
            if rng.uniform() < 0.4:
                c.append(c[q]); x.append(0.25 * x[q]); x[q] = 0.75 * x[q]
        order = rng.permutation(len(c))
        nc += [c[q] for q in order]; nv += [x[q] for q in order]
        nrp.append(len(nc))
    return np.array(nrp, np.int32), np.array(nc, np.int32), np.array(nv)


def _matrix(api, name, case10k, case1kc, case10kc):
    """(CsrMatrix, rowptr, col, val) on the host."""
    if name == "case10k":
        n, rp, ci, v, b, xs = case10k
    elif name in ("case1kc", "case10kc"):
        n, rp, ci, v, b, xs = case1kc if name == "case1kc" else case10kc
    elif name.startswith("lap2d"):
        nx, ny = map(int, name[5:].split("x"))
        A = api.CsrMatrix.laplace2d(nx, ny)
        rp, ci, v = A.arrays_to_host()
        return A, rp, ci, v
    elif name == "generated":
        A = api.CsrMatrix.generate(3000, 4, 30, True, 7, 0.5, pattern=api.GEN_DIAGONALS)
        rp, ci, v = A.arrays_to_host()
        return A, rp, ci, v
    elif name == "tridiag50k":
        rp, ci, v = tridiag(50000)
    elif name == "arrow4096":
        rp, ci, v = arrow(4096)
    elif name == "diagonal":
        n = 5000
        rp, ci, v = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), 1.0 + np.arange(n) % 13
    elif name == "shuffled_dups":
        A0 = api.CsrMatrix.laplace2d(40, 30)
        rp, ci, v = shuffled_with_duplicates(*A0.arrays_to_host())
        A0.destroy()
    return api.CsrMatrix.from_csr(rp, ci, v), rp, ci, v


FACTOR_CASES = ["case10k", "lap2d64x64", "lap2d300x200", "tridiag50k", "generated", "arrow4096", "diagonal", "shuffled_dups",
                "case1kc", "case10kc"]


# ------------------------------------------------------------------------------------------ 1. factor
@pytest.mark.parametrize("name", FACTOR_CASES)
def test_factor_matches_checker(api, case10k, case1kc, case10kc, name):
    A, rp, ci, v = _matrix(api, name, case10k, case1kc, case10kc)
    n = len(rp) - 1
    A.build_ic0()
    info = A.ic0_info()
    assert info["zero_pivot"] == -1 and info["bytes"] > 0 and info["build_ms"] > 0
    Lr, Lc, Lv = A.ic0_factor_to_host()
    Kr, Kc, Kv, zp = K.ic0(n, rp, ci, v)
    assert zp == -1
    np.testing.assert_array_equal(Lr, Kr)
    np.testing.assert_array_equal(Lc, Kc)
    assert np.abs(Lv - Kv).max() <= 1e-12 * np.abs(Kv).max()
    A.destroy()


# ------------------------------------------------------------------------------------------ 2. solves
@pytest.mark.parametrize("name", ["case10k", "tridiag50k", "lap2d300x200", "case10kc"])
def test_solves_match_scipy_and_repeat_bitwise(api, case10k, case1kc, case10kc, name):
    A, rp, ci, v = _matrix(api, name, case10k, case1kc, case10kc)
    n = len(rp) - 1
    A.build_ic0()
    Lr, Lc, Lv = A.ic0_factor_to_host()
    M = K.IcApply(K.to_sparse(n, Lr, Lc, Lv))
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, n) + (1j * rng.uniform(-1, 1, n) if A.is_complex else 0)
    xd = torch.from_numpy(x).cuda()
    for which in (0, 1, 2):
        ys = [torch.zeros_like(xd) for _ in range(3)]
        for y in ys:
            A.ic0_solve(xd, y, which)
        torch.cuda.synchronize()
        ref = M.solve(x, which)
        got = ys[0].cpu().numpy()
        assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref)
        assert all(torch.equal(ys[0], y) for y in ys[1:])                  # the same bits on every call
        # one launch per level against the production grouping: the same bits again
        from liblcg_amd import _lib
        lib = _lib.load()
        assert lib.lcg_hip_csr_ic0_schedule_for_test(A.h, 0) == 0
        per_level = A.ic0_info()["launches_per_apply"]
        y0 = torch.zeros_like(xd)
        A.ic0_solve(xd, y0, which)
        assert lib.lcg_hip_csr_ic0_schedule_for_test(A.h, -1) == 0
        torch.cuda.synchronize()
        assert torch.equal(y0, ys[0])
        info = A.ic0_info()
        assert per_level == info["levels_lower"] + info["levels_upper"]
    A.destroy()


def _launches_rule(rp, ci, groupings=(1024,)):
    """Launches per apply by DESIGN 11's rule over the checker's level sets of both triangles, for each max_merged given."""
    fw, bw = K.levels(len(rp) - 1, rp, ci)
    wf, wb = K.widths(fw), K.widths(bw)
    return [K.segments(wf, mm) + K.segments(wb, mm) for mm in groupings]


def test_launch_counts(api, case10k, case1kc, case10kc):
    from liblcg_amd import _lib
    lib = _lib.load()
    for name, want in (("case10k", 2), ("tridiag50k", 2)):
        A, rp, ci, _ = _matrix(api, name, case10k, case1kc, case10kc)
        A.build_ic0()
        info = A.ic0_info()
        assert [info["launches_per_apply"]] == [want] == _launches_rule(rp, ci), (name, info)
        if name == "tridiag50k":
            assert info["levels_lower"] == info["levels_upper"] == 50000
        A.destroy()
    rp, ci, v = laplace3d(64)
    A = api.CsrMatrix.from_csr(rp, ci, v)
    A.build_ic0()
    info = A.ic0_info()
    assert info["levels_lower"] == info["levels_upper"] == 3 * 63 + 1
    # the middle planes are wider than a workgroup: exactly the launches the rule gives, under every grouping
    groupings = (0, 1, 2, 63, 64, 1023, 1024)
    rule = _launches_rule(rp, ci, groupings)
    assert info["launches_per_apply"] == rule[-1] > 2
    try:
        for mm, want in zip(groupings, rule):
            assert lib.lcg_hip_csr_ic0_schedule_for_test(A.h, mm) == 0
            assert A.ic0_info()["launches_per_apply"] == want, mm
    finally:
        assert lib.lcg_hip_csr_ic0_schedule_for_test(A.h, -1) == 0
    assert A.ic0_info()["launches_per_apply"] == info["launches_per_apply"]
    A.destroy()


# ------------------------------------------------------------------------------------------ 3. PCG
def test_pcg_case10k(api, case10k):
    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    A.build_ic0()
    A.build_jacobi()
    bd = torch.from_numpy(b).cuda()
    para = api.lcg_default_parameters(epsilon=1e-10, abs_diff=1)
    m = torch.zeros(n, dtype=torch.float64, device="cuda")
    info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", None, m, bd, n, para, A)
    Lr, Lc, Lv, _ = K.ic0(n, rp, ci, v)
    As = K.to_sparse(n, rp, ci, v)
    M = K.IcApply(K.to_sparse(n, Lr, Lc, Lv))
    mref, iref = K.lpcg(As, M.solve, b, 1e-10, 1)
    assert iref == 54
    assert info.ret == 0 and abs(info.iterations - iref) <= 2
    assert np.abs(m.cpu().numpy() - xs).mean() < 1e-6
    mj = torch.zeros_like(m)
    jac = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_jacobi_mx", None, mj, bd, n, para, A)
    assert jac.ret == 0 and 3 * info.iterations <= jac.iterations
    for k in (1, 2, 3, 4):
        mk = torch.zeros_like(m)
        ik = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", None, mk, bd, n,
                                           api.lcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=k), A)
        want, _ = K.lpcg(As, M.solve, b, 1e-10, 1, max_iterations=k)
        assert ik.iterations == k
        assert np.linalg.norm(mk.cpu().numpy() - want) <= 1e-12 * np.linalg.norm(want)
    seen = []

    def progress(inst, mp, res, para_p, nn, k):
        seen.append(k)
        return 0
    mp = torch.zeros_like(m)
    ip = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", progress, mp, bd, n, para, A)
    assert ip.ret == 0 and ip.iterations == info.iterations and max(seen) == info.iterations
    A.destroy()


# ------------------------------------------------------------------------------------------ 4. complex
@pytest.mark.parametrize("case", ["1K", "10K"])
def test_complex_pcg(api, case1kc, case10kc, case):
    n, rp, ci, v, b, xs = case1kc if case == "1K" else case10kc
    A = api.CsrMatrix.from_csr(rp, ci, v)
    A.build_ic0()
    A.build_jacobi()
    bd = torch.from_numpy(b).cuda()
    para = api.clcg_default_parameters(epsilon=1e-10, abs_diff=1)
    m = torch.zeros(n, dtype=torch.complex128, device="cuda")
    info = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ic0_mx", None, m, bd, n, para, A, api.CLCG_PCG)
    assert info.ret == 0
    assert np.linalg.norm(m.cpu().numpy() - xs) <= 1e-5
    mj = torch.zeros_like(m)
    jac = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_jacobi_mx", None, mj, bd, n, para, A, api.CLCG_PCG)
    assert jac.ret == 0 and info.iterations <= jac.iterations
    Lr, Lc, Lv, _ = K.ic0(n, rp, ci, v)
    As = K.to_sparse(n, rp, ci, v)
    M = K.IcApply(K.to_sparse(n, Lr, Lc, Lv))
    for k in (1, 2, 3, 4):
        mk = torch.zeros_like(m)
        ik = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ic0_mx", None, mk, bd, n,
                                            api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=k), A, api.CLCG_PCG)
        want, t = K.clpcg(As, M.solve, b, 1e-10, 1, max_iterations=k)
        assert ik.iterations == t                            # (case_10K_cA converges in 3)
        assert np.linalg.norm(mk.cpu().numpy() - want) <= 1e-12 * np.linalg.norm(want)
    A.destroy()


# ------------------------------------------------------------------------------------------ 5. errors
def test_errors(api, case10k):
    from liblcg_amd import _lib
    lib = _lib.load()
    rp, ci, v = tridiag(100)
    v = v.copy()
    v[rp[17] + 1] = -3.0                                     # row 17's diagonal
    A = api.CsrMatrix.from_csr(rp, ci, v)
    assert lib.lcg_hip_csr_build_ic0(A.h) == E_ARG
    assert "17" in lib.lcg_hip_last_error().decode()
    assert A.ic0_info()["zero_pivot"] == 17
    x = torch.ones(100, dtype=torch.float64, device="cuda"); y = torch.zeros_like(x)
    assert lib.lcg_hip_ic0_solve(A.h, 2, x.data_ptr(), y.data_ptr()) == E_ARG
    A.destroy()

    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    bd = torch.from_numpy(b).cuda()
    m = torch.zeros(n, dtype=torch.float64, device="cuda")
    para = api.lcg_default_parameters(epsilon=1e-10, abs_diff=1)
    assert lib.lcg_hip_solver_preconditioned(_lib.fnptr(lib, "lcg_hip_csr_ax"), _lib.fnptr(lib, "lcg_hip_ic0_mx"), None,
                                             m.data_ptr(), bd.data_ptr(), n, para, A.h, api.LCG_PCG, api.MEM_DEVICE) == E_ARG
    A.build_ic0()
    mc = torch.zeros(n, dtype=torch.complex128, device="cuda"); bc = bd.to(torch.complex128)
    cpara = api.clcg_default_parameters(epsilon=1e-10, abs_diff=1)
    assert lib.clcg_hip_solver_preconditioned(_lib.fnptr(lib, "clcg_hip_csr_ax"), _lib.fnptr(lib, "clcg_hip_ic0_mx"), None,
                                              mc.data_ptr(), bc.data_ptr(), n, cpara, A.h, api.CLCG_PCG, api.MEM_DEVICE) == E_ARG
    x = torch.ones(n, dtype=torch.float64, device="cuda")
    assert lib.lcg_hip_ic0_solve(A.h, 2, x.data_ptr(), x.data_ptr()) == E_ARG        # x and y alias
    assert lib.lcg_hip_ic0_solve(A.h, 3, x.data_ptr(), m.data_ptr()) == E_ARG
    A.destroy()
    torch.cuda.synchronize()

    # create -> build_ic0 -> destroy gives its memory back
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        A = api.CsrMatrix.from_csr(rp, ci, v)
        A.build_ic0()
        A.build_ic0()                                        # rebuild on repeat
        A.destroy()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)


# ------------------------------------------------------------------------------------------ 6. C++
def test_cpp_sample():
    from liblcg_amd import _lib
    _lib.build()
    bindir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "sample_csr_ic0")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sample_csr_ic0.cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", exe])
    p = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    it = int(re.search(r"iterations:\s*(\d+)", p.stdout).group(1))
    err = float(re.search(r"mean error:\s*(\S+)", p.stdout).group(1))
    assert abs(it - 54) <= 2 and err < 1e-6, p.stdout
