"""IC(0) applied by Jacobi sweeps on the MI355X (csr_tri.hip: k_ic_scale, k_ic_sweep): `levels` sweeps return the exact solves'
bits; k sweeps lie within the rounding bound of the sweep checker (tests/ic0_sweeps_checker.py) run on the device's own factor;
PCG with the k-sweep operator walks the checker's loops; the setting, its errors, the done flag, and the C++ sample."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import c64_checker as K64
import ic0_checker as IC
import ic0_c64_checker as Q
import ic0_sweeps_checker as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
E_ARG = -2003
U32 = 2.0 ** -24
SAMPLE14 = {"epsilon": 1e-6, "abs_diff": 0, "max_iterations": 5000}


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------ systems
def _arrays(name, case10k, case1kc, case10kc):
    """(rowptr, col, val) on the host; a name ending in "64" is the complex64 copy of a complex system."""
    c64 = name.endswith("64")
    base = name[:-2] if c64 else name
    if base == "case10k":
        rp, ci, v = case10k[1:4]
    elif base in ("case1kc", "case10kc"):
        rp, ci, v = (case1kc if base == "case1kc" else case10kc)[1:4]
    elif base == "laplace":
        rp, ci, v = S.laplace2d(64)                # 64 x 64
    elif base == "chain3000":
        rp, ci, v = S.chain(3000)
    else:
        rp, ci, v = S.uneven(base)
    return rp, ci, (v.astype(np.complex64) if c64 else v)


def _matrix(api, name, case10k, case1kc, case10kc):
    rp, ci, v = _arrays(name, case10k, case1kc, case10kc)
    A = api.CsrMatrix.from_csr_c64(rp, ci, v) if v.dtype == np.complex64 else api.CsrMatrix.from_csr(rp, ci, v)
    A.build_ic0()
    return A, rp, ci, v


def _solve(A, which, xd):
    y = torch.zeros_like(xd)
    A.ic0_solve(xd, y, which)
    torch.cuda.synchronize()
    return y.cpu().numpy()


THREE_TYPES = ["case10k", "case1kc", "case10kc", "case1kc64", "case10kc64"]


# ------------------------------------------------------------------------------------------ 1. the bit contract
@pytest.mark.parametrize("name", THREE_TYPES + ["laplace", "chain3000"])
def test_levels_sweeps_return_the_exact_solves_bits(api, case10k, case1kc, case10kc, name):
    A, rp, ci, v = _matrix(api, name, case10k, case1kc, case10kc)
    try:
        n = len(rp) - 1
        info = A.ic0_info()
        levels = {0: info["levels_lower"], 1: info["levels_upper"], 2: max(info["levels_lower"], info["levels_upper"])}
        if name == "chain3000":
            assert levels[0] == levels[1] == 3000
        xd = torch.from_numpy(S.random_vector(n, S.kind_of(v), 2)).cuda()
        exact = {which: _solve(A, which, xd) for which in (0, 1, 2)}
        for which in (0, 1, 2):
            A.ic0_set_sweeps(levels[which])
            got = _solve(A, which, xd)
            assert got.tobytes() == exact[which].tobytes(), (name, which, levels[which], float(np.abs(got - exact[which]).max()))
            assert _solve(A, which, xd).tobytes() == got.tobytes(), (name, which)
        A.ic0_set_sweeps(3)                                             # and a short run repeats its bits as well
        for which in (0, 1, 2):
            assert _solve(A, which, xd).tobytes() == _solve(A, which, xd).tobytes(), (name, which)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 2. k sweeps against the checker
UNEVEN = ["spd", "arrow700", "arrow4096", "layered", "carrow700", "carrow4096", "layered64", "carrow70064", "carrow409664"]


@pytest.mark.parametrize("name", THREE_TYPES + UNEVEN)
def test_k_sweeps_within_the_rounding_bound(api, case10k, case1kc, case10kc, name):
    """|device - checker| <= 2 E(k) per component (ic0_sweeps_checker.sweep_bound: nothing in it is measured; tests/test_ic0_sweeps_cpu.py
    shows the checker alone inside E(k)), the checker run on the factor downloaded from the device."""
    A, rp, ci, v = _matrix(api, name, case10k, case1kc, case10kc)
    try:
        n = len(rp) - 1
        lrp, lc, lv = A.ic0_factor_to_host()
        kind = S.kind_of(lv)
        assert kind == S.kind_of(v)
        L, LT = S.triangles(n, lrp, lc, lv)
        x = S.random_vector(n, kind, 8)
        xd = torch.from_numpy(x).cuda()
        worst = 0.0
        for k in (1, 2, 3, 4, 7):
            A.ic0_set_sweeps(k)
            M = S.SweepApply(n, lrp, lc, lv, k)
            for which in (0, 1, 2):
                got, ref = _solve(A, which, xd), M.solve(x, which)
                E = S.apply_bound(L, LT, x, k, which)
                err = np.abs(got.astype(np.complex128) - ref.astype(np.complex128))
                ratio = float(np.max(err / np.maximum(2.0 * E, 1e-300)))
                worst = max(worst, ratio)
                print(f"{name} k={k} which={which}: max |device - checker| / (2 E) = {ratio:.3f}")
                assert np.all(np.isfinite(got)) and np.all(err <= 2.0 * E), (name, k, which, ratio)
        print(f"{name}: worst ratio {worst:.3f}")
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 3. PCG
def test_pcg_case10k(api, case10k):
    """lcg_hip_ic0_mx with k = 2, 4 against ic0_checker.lpcg with the checker's k-sweep operator: capped runs at 1e-12, converged
    runs by return code, count (+- 2) and mean error against case_10K_B (tests/test_gpu_ic0.py's limits for the exact apply)."""
    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ic0()
        bd = torch.from_numpy(b).cuda()
        Lr, Lc, Lv, _ = IC.ic0(n, rp, ci, v)
        As = IC.to_sparse(n, rp, ci, v)
        for k in (2, 4):
            A.ic0_set_sweeps(k)
            M = S.SweepApply(n, Lr, Lc, Lv, k)
            for cap in (1, 2, 5):
                mk = torch.zeros(n, dtype=torch.float64, device="cuda")
                ik = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", None, mk, bd, n,
                                                   api.lcg_default_parameters(epsilon=1e-10, abs_diff=1, max_iterations=cap), A)
                want, _ = IC.lpcg(As, M.mx, b, 1e-10, 1, max_iterations=cap)
                rel = np.linalg.norm(mk.cpu().numpy() - want) / np.linalg.norm(want)
                print(f"case10k k={k} cap={cap}: rel {rel:.2e}")
                assert ik.iterations == cap and rel <= 1e-12, (k, cap, rel)
            m = torch.zeros(n, dtype=torch.float64, device="cuda")
            info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", None, m, bd, n,
                                                 api.lcg_default_parameters(epsilon=1e-10, abs_diff=1), A)
            _, iref = IC.lpcg(As, M.mx, b, 1e-10, 1)
            err = float(np.abs(m.cpu().numpy() - xs).mean())
            print(f"case10k k={k}: iterations {info.iterations} (checker {iref}), mean error {err:.2e}")
            assert info.ret == 0 and abs(info.iterations - iref) <= 2, (k, info, iref)
            assert err < 1e-6, (k, err)
    finally:
        A.destroy()


def _clpcg(api, A, bd, n, **para):
    m = torch.zeros(n, dtype=torch.complex128, device="cuda")
    para = {k: x for k, x in para.items() if x}                         # (max_iterations = 0: the default, to convergence)
    info = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ic0_mx", None, m, bd, n,
                                          api.clcg_default_parameters(epsilon=1e-10, abs_diff=1, **para), A, api.CLCG_PCG)
    return info, m.cpu().numpy()


@pytest.mark.parametrize("case", ["1K", "10K"])
def test_complex_pcg(api, case1kc, case10kc, case):
    """clcg_hip_ic0_mx with k = 2, 4 against ic0_checker.clpcg with the k-sweep operator (tests/test_gpu_ic0.py's limits).
    case_10K_cA's triangles have 2 levels: with k = 2 every iterate is the exact apply's, bit for bit."""
    n, rp, ci, v, b, xs = case1kc if case == "1K" else case10kc
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ic0()
        bd = torch.from_numpy(b).cuda()
        Lr, Lc, Lv, _ = IC.ic0(n, rp, ci, v)
        As = IC.to_sparse(n, rp, ci, v)
        exact = {cap: _clpcg(api, A, bd, n, max_iterations=cap) for cap in (1, 2, 5, 0)}
        for k in (2, 4):
            A.ic0_set_sweeps(k)
            M = S.SweepApply(n, Lr, Lc, Lv, k)
            for cap in (1, 2, 5):
                ik, mk = _clpcg(api, A, bd, n, max_iterations=cap)
                want, t = IC.clpcg(As, M.mx, b, 1e-10, 1, max_iterations=cap)
                rel = np.linalg.norm(mk - want) / np.linalg.norm(want)
                print(f"case_{case}_cA k={k} cap={cap}: iterations {ik.iterations} (checker {t}), rel {rel:.2e}")
                assert ik.iterations == t and rel <= 1e-12, (case, k, cap, rel)
            info, m = _clpcg(api, A, bd, n)
            _, iref = IC.clpcg(As, M.mx, b, 1e-10, 1)
            err = float(np.linalg.norm(m - xs))
            print(f"case_{case}_cA k={k}: iterations {info.iterations} (checker {iref}), distance {err:.2e}")
            assert info.ret == 0 and abs(info.iterations - iref) <= 2, (case, k, info, iref)
            assert err <= 1e-5, (case, k, err)
            if case == "10K" and k == 2:
                assert A.ic0_info()["levels_lower"] == A.ic0_info()["levels_upper"] == 2
                for cap in (1, 2, 5, 0):
                    ik, mk = _clpcg(api, A, bd, n, max_iterations=cap)
                    assert ik.iterations == exact[cap][0].iterations and mk.tobytes() == exact[cap][1].tobytes(), cap
    finally:
        A.destroy()


def _tol64(run, k):
    """tests/test_gpu_c64.py's tolerance for capped complex64 runs: 4 x the checker's own fp32-vs-complex128 gap, at least 64 u."""
    a, e = run(np.complex64, k), run(np.complex128, k)
    d = np.linalg.norm(a["x"].astype(np.complex128) - e["x"]) / max(np.linalg.norm(e["x"]), 1e-30)
    return a, max(4.0 * d, 64 * U32)


@pytest.mark.parametrize("case", ["1K", "10K"])
def test_c64_pcg(api, case1kc, case10kc, case):
    """clcg_hip_ic0_mx_c64 with k = 2, 4 against c64_checker.pcg with the fp32 k-sweep operator on the checker's fp32 factor:
    capped runs at tests/test_gpu_c64.py's tolerance (the complex128 twin: the same sweeps in complex128 on ic0_checker's
    factor of the complex64 values), converged runs at sample14's settings by return code, count (+- 2) and averaged error
    (tests/test_gpu_ic0_c64.py: 3x the checker's + 1e-7)."""
    n, rp, ci, v, b, xs = case1kc if case == "1K" else case10kc
    v, b = v.astype(np.complex64), b.astype(np.complex64)
    ops = K64.csr_ops(rp, ci, v, np.complex64)
    lrp, lc, lv, _ = Q.ic0(n, rp, ci, v)
    wrp, wc, wv, _ = IC.ic0(n, rp, ci, v.astype(np.complex128))
    m0 = np.zeros(n, np.complex64)
    bd = torch.from_numpy(b).cuda()
    A = api.CsrMatrix.from_csr_c64(rp, ci, v)

    def gpu(para):
        m = torch.zeros(n, dtype=torch.complex64, device="cuda")
        info = api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_ic0_mx_c64", None, m, bd, n, para, A)
        return info, m.cpu().numpy()
    try:
        A.build_ic0()
        exact = {cap: gpu(api.clcg_default_parameters(epsilon=1e-30, max_iterations=cap)) for cap in (1, 2, 5)}
        for k in (2, 4):
            A.ic0_set_sweeps(k)
            m32 = S.SweepApply(n, lrp, lc, lv, k)
            m64 = S.SweepApply(n, wrp, wc, wv, k)
            mx = {np.complex64: lambda x: m32.mx(np.asarray(x, np.complex64)),
                  np.complex128: lambda x: m64.mx(np.asarray(x, np.complex128))}
            for cap in (1, 2, 5):
                para = {"epsilon": 1e-30, "max_iterations": cap}
                ref, tol = _tol64(lambda dt, c: K64.pcg(ops["A"], mx[dt], b, m0, para, dt), cap)
                info, x = gpu(api.clcg_default_parameters(epsilon=1e-30, max_iterations=cap))
                rel = np.linalg.norm(x.astype(np.complex128) - ref["x"]) / np.linalg.norm(ref["x"])
                print(f"case_{case}_cA c64 k={k} cap={cap}: rel {rel:.2e} (tolerance {tol:.2e})")
                assert info.ret == ref["ret"] and info.iterations == ref["iters"], (case, k, cap, info, ref["ret"], ref["iters"])
                assert rel <= tol, (case, k, cap, rel, tol)
                if case == "10K" and k == 2:                   # 2 levels: the exact apply's bits
                    assert x.tobytes() == exact[cap][1].tobytes() and info.iterations == exact[cap][0].iterations, cap
            info, x = gpu(api.clcg_default_parameters(**SAMPLE14))
            ref = K64.pcg(ops["A"], mx[np.complex64], b, m0, SAMPLE14)
            xs64 = xs.astype(np.complex64)
            e_ref = float(np.linalg.norm((ref["x"] - xs64).astype(np.complex128)) / n)
            e = float(np.linalg.norm((x - xs64).astype(np.complex128)) / n)
            print(f"case_{case}_cA c64 k={k}: iterations {info.iterations} (checker {ref['iters']}), error {e:.2e} (checker {e_ref:.2e})")
            assert info.ret == ref["ret"] == K64.CLCG_CONVERGENCE, (case, k, info, ref["ret"])
            assert abs(info.iterations - ref["iters"]) <= 2, (case, k, info.iterations, ref["iters"])
            assert e <= 3 * e_ref + 1e-7, (case, k, e, e_ref)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 4. the setting and its errors
def test_setting_and_errors(api, lib, case10k):
    import ctypes as C
    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    k = C.c_int(-7)
    try:
        # no factor yet, NULL, a negative count
        assert lib.lcg_hip_csr_ic0_set_sweeps(A.h, 2) == E_ARG and "no factor" in lib.lcg_hip_last_error().decode()
        assert lib.lcg_hip_csr_ic0_get_sweeps(A.h, C.byref(k)) == E_ARG and "no factor" in lib.lcg_hip_last_error().decode()
        assert lib.lcg_hip_csr_ic0_set_sweeps(None, 2) == E_ARG and "NULL" in lib.lcg_hip_last_error().decode()
        assert lib.lcg_hip_csr_ic0_get_sweeps(None, C.byref(k)) == E_ARG
        A.build_ic0()
        assert lib.lcg_hip_csr_ic0_get_sweeps(A.h, C.byref(k)) == 0 and k.value == 0
        assert lib.lcg_hip_csr_ic0_set_sweeps(A.h, -1) == E_ARG and "-1" in lib.lcg_hip_last_error().decode()
        assert lib.lcg_hip_csr_ic0_get_sweeps(A.h, C.byref(k)) == 0 and k.value == 0
        before = A.ic0_info()
        assert before["sweeps"] == 0
        xd = torch.from_numpy(S.random_vector(n, "f64", 1)).cuda()
        y0 = _solve(A, 2, xd)
        # a round trip; launches and bytes follow the setting
        for kk in (1, 3, 8):
            assert lib.lcg_hip_csr_ic0_set_sweeps(A.h, kk) == 0
            assert lib.lcg_hip_csr_ic0_get_sweeps(A.h, C.byref(k)) == 0 and k.value == kk
            info = A.ic0_info()
            assert info["sweeps"] == kk and info["launches_per_apply"] == 2 * kk
            assert info["bytes"] == before["bytes"] + 2 * 8 * n
        assert _solve(A, 2, xd).tobytes() != y0.tobytes()               # 8 sweeps of 201 levels: another operator
        # back to the exact apply: the old bits, the old counts
        A.ic0_set_sweeps(0)
        assert A.ic0_info() == before
        assert _solve(A, 2, xd).tobytes() == y0.tobytes()
        # a rebuild resets the setting
        A.ic0_set_sweeps(5)
        A.build_ic0()
        info = A.ic0_info()
        assert info["sweeps"] == 0 and info["launches_per_apply"] == before["launches_per_apply"] and info["bytes"] == before["bytes"]
        assert _solve(A, 2, xd).tobytes() == y0.tobytes()
        # the Python view raises on the same error
        with pytest.raises(api.LcgHipError):
            A.ic0_set_sweeps(-3)
    finally:
        A.destroy()

    # type mixing: set_sweeps serves every handle; the solve entries still refuse the other type
    rp, ci, v = S.uneven("layered")
    nn = len(rp) - 1
    A64 = api.CsrMatrix.from_csr_c64(rp, ci, v.astype(np.complex64))
    A128 = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        for H in (A64, A128):
            H.build_ic0()
            H.ic0_set_sweeps(3)
            assert H.ic0_info()["sweeps"] == 3 and H.ic0_info()["launches_per_apply"] == 6
        x64 = torch.ones(nn, dtype=torch.complex64, device="cuda"); y64 = torch.zeros_like(x64)
        x128 = torch.ones(nn, dtype=torch.complex128, device="cuda"); y128 = torch.zeros_like(x128)
        assert lib.lcg_hip_ic0_solve(A64.h, 2, x128.data_ptr(), y128.data_ptr()) == E_ARG
        assert "complex64" in lib.lcg_hip_last_error().decode()
        assert lib.lcg_hip_ic0_solve_c64(A128.h, 2, x64.data_ptr(), y64.data_ptr()) == E_ARG
        assert lib.lcg_hip_ic0_solve_c64(A64.h, 2, x64.data_ptr(), y64.data_ptr()) == 0
        assert lib.lcg_hip_ic0_solve(A128.h, 2, x128.data_ptr(), y128.data_ptr()) == 0
        assert lib.lcg_hip_ic0_solve_c64(A64.h, 2, x64.data_ptr(), x64.data_ptr()) == E_ARG      # x and y alias, as before
        torch.cuda.synchronize()
        assert A128.ic0_info()["bytes"] - A64.ic0_info()["bytes"] == 8 * (2 * len(A64.ic0_factor_to_host()[1]) + 3 * nn)
    finally:
        A64.destroy()
        A128.destroy()

    # set -> destroy and set -> 0 give the memory back
    n, rp, ci, v, b, xs = case10k
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        A = api.CsrMatrix.from_csr(rp, ci, v)
        A.build_ic0()
        A.ic0_set_sweeps(4)
        A.ic0_set_sweeps(0)
        A.ic0_set_sweeps(2)
        A.destroy()
    assert lib.lcg_hip_trim() == 0
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)


# ------------------------------------------------------------------------------------------ 5. the done flag
def test_early_convergence_with_and_without_progress_callback(api, case10k):
    """A solve that converges with sweeps set leaves the same iterate and count whether or not a progress callback forces a
    synchronisation in every iteration: the sweeps launched after the stop see the done flag and write nothing."""
    n, rp, ci, v, b, xs = case10k
    A = api.CsrMatrix.from_csr(rp, ci, v)
    try:
        A.build_ic0()
        A.ic0_set_sweeps(4)
        bd = torch.from_numpy(b).cuda()
        para = api.lcg_default_parameters(epsilon=1e-10, abs_diff=1)
        m = torch.zeros(n, dtype=torch.float64, device="cuda")
        info = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", None, m, bd, n, para, A)
        seen = []

        def progress(inst, mp, res, para_p, nn, k):
            seen.append(k)
            return 0
        mp = torch.zeros_like(m)
        ip = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", progress, mp, bd, n, para, A)
        assert info.ret == ip.ret == 0 and ip.iterations == info.iterations == max(seen), (info, ip)
        assert torch.equal(m, mp)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 6. C++
def _sample(name):
    from liblcg_amd import _lib
    _lib.build()
    bindir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, name)
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", name + ".cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", exe])
    p = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_cpp_sample():
    out = _sample("sample_csr_ic0_sweeps")
    exact = re.search(r"PCG-IC0 exact \(sweeps 0, (\d+) launches per apply\): ret=0 .*iterations:\s*(\d+) mean error:\s*(\S+)", out)
    sweeps = re.search(r"PCG-IC0 sweeps \(sweeps 4, (\d+) launches per apply\): ret=0 .*iterations:\s*(\d+) mean error:\s*(\S+)", out)
    assert exact and sweeps, out
    jacobi = int(re.search(r"^PCG: ret=0 .*iterations=(\d+)", _sample("sample_csr"), flags=re.M).group(1))
    assert int(sweeps.group(1)) == 8, out
    assert abs(int(exact.group(2)) - 54) <= 2, out
    assert int(exact.group(2)) <= int(sweeps.group(2)) <= jacobi, (out, jacobi)
    assert float(exact.group(3)) < 1e-6 and float(sweeps.group(3)) < 1e-6, out
