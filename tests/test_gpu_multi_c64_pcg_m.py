"""-m gpu: batched complex64 PCG with the handle's fp32 IC(0) factor as M (clcg_hip_lpcg_multi_m_c64) for k = 2, 4, 8 on
helmholtz(40) and case_10K_cA cast to complex64, exact applies and 2 / 4 sweeps: every column against c64_checker.pcg run on that
column alone with the matching checker apply (ic0_c64_checker.Ic64Apply, tri_multi_c64_cases.Sweep64); then what makes a batch a
batch, the Jacobi forwarding, n.k = 2^20, the refusals, device memory, the Python front and the example program.

Bands: a run capped at 25 (epsilon 1e-30) -- code and count equal the checker's, distance within tri_multi_c64_cases.tol_column (4 x
the checker's complex64 run's distance to its complex128 twin, never below 64 x 2^-24).  With this preconditioner |r|^2 falls by
several orders per iteration, so some runs end before the cap: the recursive residual r -= ak Ad, a difference of nearly equal fp32
vectors, passes 1e-30 as rounding noise, many orders below the 2^-48 |b|^2 that fp32 resolves.  Where the checker's complex64 run
and its complex128 twin themselves disagree on the code or the count, the verdict is decided by the last bit and is not required
(the rule of tests/test_gpu_multi_c64_solvers.py::test_sizes_capped_at_4); the iterate is held to the band in every case.
Converged at sample14's settings -- the rules of tests/test_gpu_multi_c64_solvers.py::test_converged_runs (code 0, the count within
10 % + 2 of the checker's, the distance to the complex128 direct solve within 10 x the checker's own, the reported residual within
epsilon).

Launches: by construction the set-up and every body enqueue one product, three k-wide passes (set-up: r = B - A.m | d = z and the sums
| the verdict; body: the update | the sums | the direction) and the apply's L launches, so a run that reaches the cap of 25 reports
26 products and 26 (3 + L) vector passes -- one pass per body more than the Jacobi form's two, plus the apply."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import multi_c64_cases as cc
import tri_multi_c64_cases as Z
from multi_c64_cases import ALREADY, BADEPS, BADMAXIT, CONV, E_ARG, KS, MAXIT, NANV, NOPRE, PCG, bits, cmulti64
from test_gpu_multi_c64_solvers import NAMES, direct

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SWEEPS = (0, 2, 4)
SYSTEMS = ("helmholtz40", "case10k")
ENTRY = "clcg_hip_lpcg_multi_m_c64"


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def systems(api):
    """name -> (S, handle holding the Jacobi diagonal and a complex64 IC(0) factor)"""
    out = {}
    for name in SYSTEMS:
        S = Z.solver_system(name)
        out[name] = (S, Z.build(api, (S["rp"], S["ci"], S["v"]), jacobi=True))
    yield out
    for _, A in out.values():
        A.destroy()


def zeros(n, k):
    M0 = np.zeros((n, k), np.complex64)
    if k >= 4:
        M0[:, 3] = -0.0 - 0.0j      # a guess of zeros that shows a write
    return M0


def run(lib, api, sweeps, A, M0, B, mem="device", **para):
    A.ic0_set_sweeps(sweeps)
    return Z.multi_m(lib, api, Z.M_IC0, A, M0, B, mem=mem, **para)


def launches(lib):
    vec, prod = C.c_int(), C.c_int()
    lib.lcg_hip_last_launches(C.byref(vec), None, None, C.byref(prod))
    return prod.value, vec.value


# ------------------------------------------------------------------------------------------ 1. every column against the checker
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sweeps", SWEEPS)
@pytest.mark.parametrize("name", SYSTEMS)
def test_capped_at_25_iterations(lib, api, systems, name, sweeps, k):
    S, A = systems[name]
    n = S["n"]
    B, M0 = cc.columns(S, k), zeros(n, k)
    para = dict(epsilon=1e-30, max_iterations=25)
    rc, ret, its, res, M = run(lib, api, sweeps, A, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    prod, vec = launches(lib)
    for j in range(k):
        if not B[:, j].any():
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j])), (j, ret[j], its[j])
            continue
        ref, tol = Z.tol_column(S, sweeps, B[:, j], ("col", NAMES[j]), **para)
        twin = Z.checker_column(S, sweeps, B[:, j], ("col", NAMES[j]), np.complex128, **para)
        strict = (ref["ret"], ref["iters"]) == (twin["ret"], twin["iters"])
        rel = np.linalg.norm(M[:, j].astype(np.complex128) - ref["x"]) / np.linalg.norm(ref["x"])
        print(name, sweeps, k, j, "ret", ret[j], ref["ret"], twin["ret"], "its", its[j], ref["iters"], twin["iters"], "distance", rel,
              "tol", tol, "residual", res[j], ref["residual"])
        if strict:
            assert ret[j] == ref["ret"] and its[j] == ref["iters"], (j, ret[j], ref["ret"], its[j], ref["iters"])
        else:
            assert ret[j] in (CONV, MAXIT) and 0 < its[j] <= 25, (j, ret[j], its[j])
        assert rel <= tol, (j, rel, tol)
    if name == "helmholtz40" and sweeps == 2:           # (the checker's runs are still going at the cap there: the CPU test shows it)
        assert max(its) == 25
    L = A.ic0_info()["launches_per_apply"]
    if sweeps:
        assert L == 2 * sweeps
    if max(its) == 25:                                  # what a run that reaches the cap enqueued
        assert lib.lcg_hip_last_iterations() == 25
        assert (prod, vec) == (26, 26 * (3 + L)), (prod, vec, L)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sweeps", SWEEPS)
@pytest.mark.parametrize("name", SYSTEMS)
def test_converged_at_sample14s_settings(lib, api, systems, name, sweeps, k):
    S, A = systems[name]
    n = S["n"]
    B, M0 = cc.columns(S, k), zeros(n, k)
    para = dict(Z.SAMPLE14)
    rc, ret, its, res, M = run(lib, api, sweeps, A, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        if not B[:, j].any():
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            continue
        ref = Z.checker_column(S, sweeps, B[:, j], ("col", NAMES[j]), **para)
        xd = direct(S, B[:, j])
        err_ref = np.linalg.norm(ref["x"] - xd) / np.linalg.norm(xd)
        err = np.linalg.norm(M[:, j] - xd) / np.linalg.norm(xd)
        print(name, sweeps, k, j, "ret", ret[j], "its", its[j], ref["iters"], "error", err, "checker's", err_ref, "residual", res[j])
        assert ret[j] == ref["ret"] == CONV
        assert abs(its[j] - ref["iters"]) <= 0.1 * ref["iters"] + 2, (j, its[j], ref["iters"])
        assert err <= 10 * err_ref, (j, err, err_ref)
        assert res[j] <= para["epsilon"]
    longest = int(np.argmax(its))
    assert lib.lcg_hip_last_iterations() == its[longest] and lib.lcg_hip_last_residual() == res[longest]
    if name == "case10k":                               # the factor is worth its launches: fewer iterations than the diagonal
        jac = cmulti64(lib, api, PCG, A, M0, B, **para)
        print("case10k column 0: IC(0) count", its[0], "Jacobi count", jac[2][0])
        assert jac[0] == 0 and jac[1][0] == CONV and its[0] < jac[2][0], (its[0], jac[2][0])


# ------------------------------------------------------------------------------------------ 2. Jacobi forwarding
@pytest.mark.parametrize("k", KS)
def test_jacobi_is_lpcg_multi_c64_itself(lib, api, systems, k):
    S, A = systems["helmholtz40"]
    B, M0 = cc.columns(S, k), zeros(S["n"], k)
    for para in (dict(epsilon=1e-8, max_iterations=3000), dict(epsilon=1e-30, max_iterations=25)):
        old = cmulti64(lib, api, PCG, A, M0, B, **para)
        new = Z.multi_m(lib, api, Z.M_JACOBI, A, M0, B, **para)
        assert old[0] == new[0] == 0 and old[1:4] == new[1:4], (old[1:4], new[1:4])
        assert np.array_equal(bits(old[4]), bits(new[4]))


# ------------------------------------------------------------------------------------------ 3. in a batch
def fast_and_slow(S, k):
    """cc.columns with the second column 1e-4 b: judged against max(|m|, 1) = 1, it stops several iterations before b."""
    B = cc.columns(S, k).copy()
    B[:, 1] = np.float32(1e-4) * S["b"]
    return np.ascontiguousarray(B)


@pytest.mark.parametrize("sweeps", [0, 2])
def test_verdicts_differ_and_stopped_columns_are_final(lib, api, systems, sweeps):
    S, A = systems["helmholtz40"]
    n, k = S["n"], 4
    B, M0 = fast_and_slow(S, k), np.zeros((n, k), np.complex64)
    para = dict(epsilon=1e-8)
    rc, ret, its, res, M = run(lib, api, sweeps, A, M0, B, max_iterations=3000, **para)
    assert rc == 0 and ret == [CONV, CONV, CONV, ALREADY], ret
    t_fast, t_slow = its[1], its[0]
    print(sweeps, "counts", its)
    assert 0 < t_fast < t_slow, its
    # a cap at the fast column's count: both verdicts in one call, and frozen means final -- the column that converged at t_fast
    # while the others went on has the bits of the same batch capped at t_fast
    rc, ret_c, its_c, res_c, M_c = run(lib, api, sweeps, A, M0, B, max_iterations=t_fast, **para)
    assert rc == 0
    assert ret_c[1] == CONV and its_c[1] == t_fast and ret_c[0] == MAXIT and its_c[0] == t_fast
    assert ret_c[3] == ALREADY and its_c[3] == 0
    assert np.array_equal(bits(M_c[:, 1]), bits(M[:, 1])) and res_c[1] == res[1]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sweeps", [0, 2])
def test_a_nan_stays_in_its_column(lib, api, systems, sweeps, k):
    S, A = systems["helmholtz40"]
    n = S["n"]
    B, M0 = fast_and_slow(S, k), np.zeros((n, k), np.complex64)
    para = dict(epsilon=1e-8, max_iterations=40)
    rc, ret, its, res, M = run(lib, api, sweeps, A, M0, B, **para)
    Bn = B.copy(); Bn[n // 2, 1] = complex(np.nan, 1.0)
    rc_n, ret_n, its_n, res_n, M_n = run(lib, api, sweeps, A, M0, Bn, **para)
    assert rc == 0 and rc_n == 0
    assert ret_n[1] == NANV and its_n[1] == 1, (ret_n, its_n)
    for j in range(k):
        if j == 1:
            continue
        assert ret_n[j] == ret[j] and its_n[j] == its[j] and res_n[j] == res[j], j
        assert np.array_equal(bits(M_n[:, j]), bits(M[:, j])), j
        assert np.isfinite(M_n[:, j].real).all() and np.isfinite(M_n[:, j].imag).all()


@pytest.mark.parametrize("sweeps", [0, 2])
@pytest.mark.parametrize("name", SYSTEMS)
def test_independence_and_repeatability(lib, api, systems, name, sweeps):
    S, A = systems[name]
    n, k = S["n"], 4
    B, M0 = cc.columns(S, k), np.zeros((n, k), np.complex64)
    para = dict(epsilon=1e-8, max_iterations=30)
    r1 = run(lib, api, sweeps, A, M0, B, **para)
    r2 = run(lib, api, sweeps, A, M0, B, **para)
    r3 = run(lib, api, sweeps, A, M0, B, mem="host", **para)
    for r in (r2, r3):
        assert r[0] == r1[0] == 0 and r[1:4] == r1[1:4]
        assert r[4].tobytes() == r1[4].tobytes()
    # other neighbours
    B2 = B.copy()
    rng = np.random.default_rng(8)
    B2[:, 1] = (rng.standard_normal(n) * 1e3).astype(np.complex64); B2[:, 2] = 0.0; B2[:, 3] = np.float32(1e-6) * S["b"]
    M2 = M0.copy(); M2[:, 1] = rng.standard_normal(n).astype(np.complex64)
    r4 = run(lib, api, sweeps, A, M2, B2, **para)
    assert r4[0] == 0 and (r4[1][0], r4[2][0], r4[3][0]) == (r1[1][0], r1[2][0], r1[3][0])
    assert np.array_equal(bits(r4[4][:, 0]), bits(r1[4][:, 0]))
    # the same columns in another order at the same k
    perm = [2, 0, 3, 1]
    r5 = run(lib, api, sweeps, A, M0, np.ascontiguousarray(B[:, perm]), **para)
    assert r5[0] == 0
    for jn, jo in enumerate(perm):
        assert (r5[1][jn], r5[2][jn], r5[3][jn]) == (r1[1][jo], r1[2][jo], r1[3][jo]), (jn, jo)
        assert np.array_equal(bits(r5[4][:, jn]), bits(r1[4][:, jo])), (jn, jo)
    # and at another k (the sums are one tree over leaves that depend on n alone)
    r8 = run(lib, api, sweeps, A, np.zeros((n, 8), np.complex64), cc.columns(S, 8), **para)
    assert r8[0] == 0
    for j in range(4):
        assert (r8[1][j], r8[2][j], r8[3][j]) == (r1[1][j], r1[2][j], r1[3][j]), j
        assert np.array_equal(bits(r8[4][:, j]), bits(r1[4][:, j])), j


# ------------------------------------------------------------------------------------------ 4. n.k = 2^20
def test_work_of_two_to_the_twenty(lib, api):
    """n = 131,072 at k = 8: n.k = 2^20, so six bodies are in flight and the mapped mirror is refreshed every iteration; 2048
    workgroups of the 8-wide sweep.  Column 0 against the single-vector solver with the single-vector apply at the same cap -- the same
    recurrence with other sums -- within column 0's band on the chain's first 4096 rows (the checker's factor of 131,072 rows takes
    too long for a test; the chain's coefficients and the band do not depend on its length)."""
    n, k, sweeps = 131072, 8, 2
    S, Scut = Z.chain_system(n), Z.chain_system(4096)
    assert np.array_equal(S["v"][:3 * 4000], Scut["v"][:3 * 4000]) and np.array_equal(S["b"][:4000], Scut["b"][:4000])
    B = cc.columns(S, k)
    para = dict(epsilon=1e-30, max_iterations=10)
    A = Z.build(api, (S["rp"], S["ci"], S["v"]))
    try:
        M0 = np.zeros((n, k), np.complex64)
        r1 = run(lib, api, sweeps, A, M0, B, **para)
        r2 = run(lib, api, sweeps, A, M0, B, **para)
        assert r1[0] == r2[0] == 0 and r1[1:4] == r2[1:4] and r1[4].tobytes() == r2[4].tobytes()
        assert r1[1] == [MAXIT, MAXIT, MAXIT, ALREADY, MAXIT, MAXIT, MAXIT, MAXIT] and r1[2] == [10, 10, 10, 0, 10, 10, 10, 10]
        m = torch.zeros(n, dtype=torch.complex64, device="cuda")
        b = torch.from_numpy(np.ascontiguousarray(B[:, 0])).cuda()
        info = api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_ic0_mx_c64", None, m, b, n,
                                                  api.clcg_default_parameters(**para), A)
        assert info.ret == MAXIT and info.iterations == 10
        x1 = m.cpu().numpy().astype(np.complex128)
        _, tol = Z.tol_column(Scut, sweeps, cc.columns(Scut, k)[:, 0], ("col", "b"), **para)
        d = np.linalg.norm(r1[4][:, 0] - x1) / np.linalg.norm(x1)
        print("2^20 column 0: distance to the single solve", d, "tol", tol)
        assert d <= tol, (d, tol)
    finally:
        A.destroy()


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_release_the_solver(lib, api, systems):
    S, A = systems["helmholtz40"]
    n, k = S["n"], 4
    B, Zr = cc.columns(S, k), np.zeros((n, k), np.complex64)
    good = dict(epsilon=1e-8, max_iterations=10)
    ref = run(lib, api, 2, A, Zr, B, **good)
    assert ref[0] == 0

    def still_works():
        r = run(lib, api, 2, A, Zr, B, **good)
        assert r[0] == 0 and r[1:4] == ref[1:4] and np.array_equal(bits(r[4]), bits(ref[4]))

    for precond in (Z.M_ILU0, Z.M_NONE, 99):
        r = Z.multi_m(lib, api, precond, A, Zr, B, **good)
        err = lib.lcg_hip_last_error().decode()
        assert r[0] == E_ARG and r[1] == [99] * k and ENTRY in err and "precond" in err, (precond, r[0], err)
        assert np.array_equal(bits(r[4]), bits(Zr))
        still_works()
    bare = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"])         # no factor, no Jacobi diagonal
    for precond in (Z.M_JACOBI, Z.M_IC0):
        r = Z.multi_m(lib, api, precond, bare, Zr, B, **good)
        assert r[0] == NOPRE and r[1] == [99] * k and np.array_equal(bits(r[4]), bits(Zr))      # nothing ran, nothing was reported
        assert Z.multi_m(lib, api, precond, bare, Zr, B, epsilon=0.0)[0] == BADEPS              # the parameters come first
    bare.build_jacobi()                                                 # the factor is still missing
    assert Z.multi_m(lib, api, Z.M_IC0, bare, Zr, B, **good)[0] == NOPRE
    assert Z.multi_m(lib, api, Z.M_JACOBI, bare, Zr, B, **good)[0] == 0
    bare.build_ic0()
    assert Z.multi_m(lib, api, Z.M_IC0, bare, Zr, B, **good)[0] == 0
    bare.destroy()
    still_works()
    for precond in (Z.M_JACOBI, Z.M_IC0):
        assert Z.multi_m(lib, api, precond, A, Zr, B, epsilon=0.0)[0] == BADEPS
        still_works()
        assert Z.multi_m(lib, api, precond, A, Zr, B, epsilon=1.0)[0] == BADEPS
        assert Z.multi_m(lib, api, precond, A, Zr, B, max_iterations=-1)[0] == BADMAXIT
        still_works()
    # handles of another type
    A128 = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"].astype(np.complex128))
    A128.build_ic0()
    Areal = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"].real.astype(np.float64))
    Areal.build_ic0()
    for H, word in ((A128, "complex128"), (Areal, "real")):
        r = Z.multi_m(lib, api, Z.M_IC0, H, Zr, B, **good)
        assert r[0] == E_ARG and r[1] == [99] * k and np.array_equal(bits(r[4]), bits(Zr)) and word in lib.lcg_hip_last_error().decode()
        H.destroy()
    Zd = torch.zeros((n, k), dtype=torch.complex64, device="cuda")
    assert lib.clcg_hip_lpcg_multi_m_c64(A.h, k, Z.M_IC0, Zd.data_ptr(), Zd.data_ptr(), None, None, None, None, 7) == E_ARG
    assert "mem" in lib.lcg_hip_last_error().decode()
    still_works()
    # the single-vector path beside it: column 0 is b, the same recurrence with other sums
    A.ic0_set_sweeps(2)
    m = torch.zeros(n, dtype=torch.complex64, device="cuda")
    info = api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_ic0_mx_c64", None, m, torch.from_numpy(S["b"]).cuda(), n,
                                              api.clcg_default_parameters(**good), A)
    assert info.ret == ref[1][0] and info.iterations == ref[2][0]
    _, tol = Z.tol_column(S, 2, S["b"], ("col", "b"), **good)
    x1 = m.cpu().numpy()
    assert np.linalg.norm(x1 - ref[4][:, 0]) <= tol * np.linalg.norm(x1)


# ------------------------------------------------------------------------------------------ 6. device memory
def test_repeated_solves_do_not_grow_device_memory(api, lib):
    """The pattern of tests/test_gpu_multi_c64_solvers.py's test of the same name (n = 90000: the factor's k-wide work vectors are
    5.8 MB each at k = 8): after the first solve at the widest k and the largest sweep count, 20 more solves at every k take no more
    device memory; after destroy and trim the device has its memory back."""
    S = cc.system("helmholtz", 300)
    torch.cuda.empty_cache()
    assert lib.lcg_hip_trim() == 0
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    A = Z.build(api, (S["rp"], S["ci"], S["v"]))
    A.ic0_set_sweeps(2)
    Bs = {k: torch.from_numpy(cc.columns(S, k)).cuda() for k in KS}
    Ms = {k: torch.zeros_like(Bs[k]) for k in KS}
    p = api.clcg_default_parameters(epsilon=1e-30, max_iterations=5)

    def solve(k):
        Ms[k].zero_()
        infos = api.clpcg_multi_c64(A, Ms[k], Bs[k], p, precond="ic0")
        assert infos[0].ret == MAXIT and infos[0].iterations == 5

    solve(8)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    for i in range(20):
        solve(KS[i % 3])
    torch.cuda.synchronize()
    free2 = torch.cuda.mem_get_info()[0]
    assert free1 < free0 and free2 >= free1 - (1 << 20), (free0, free1, free2)
    A.destroy()
    del Bs, Ms
    torch.cuda.empty_cache()
    assert lib.lcg_hip_trim() == 0
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)


# ------------------------------------------------------------------------------------------ 7. front ends
def test_python_front(api, systems):
    S, A = systems["helmholtz40"]
    n = S["n"]
    Bh = cc.columns(S, 4)
    B = torch.from_numpy(Bh).cuda()
    p = api.clcg_default_parameters(epsilon=1e-8)
    A.ic0_set_sweeps(0)
    counts = {}
    for precond in ("jacobi", "ic0"):
        M = torch.zeros((n, 4), dtype=torch.complex64, device="cuda")
        infos = api.clpcg_multi_c64(A, M, B, p, precond=precond)
        assert [i.ret for i in infos] == [CONV, CONV, CONV, ALREADY] and infos[3].iterations == 0
        Y = torch.full((n, 4), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
        A.cspmm_c64(M, Y)
        api.synchronize()
        r = (Y - B).cpu().numpy()
        assert np.linalg.norm(r[:, 0]) <= 1e-3 * np.linalg.norm(Bh[:, 0]), precond
        counts[precond] = infos[0].iterations
    print("iterations of column 0:", counts)
    assert counts["ic0"] < counts["jacobi"]
    M = torch.zeros((n, 4), dtype=torch.complex64, device="cuda")
    assert api.clpcg_multi_c64(A, M, B, p)[0].iterations == counts["jacobi"]           # the old call signature
    for bad in ("ssor", "ilu0"):
        with pytest.raises(ValueError):
            api.clpcg_multi_c64(A, M, B, p, precond=bad)
    Mh = cc.aligned_block(np.zeros((n, 4), np.complex64))
    infos_h = api.clpcg_multi_c64(A, Mh, cc.aligned_block(Bh), p, precond="ic0")
    assert [i.ret for i in infos_h] == [CONV, CONV, CONV, ALREADY]


def test_sample_program_solves_four_sources(api, lib, systems):
    """examples/sample_csr_multi_c64_ic0.cpp: columns 0..2 converge, the zero column is already optimised, and a column's true
    residual |b - A.x|^2 / max(|x|, 1)^2 (recomputed in double from the iterate) exceeds the residual the loop reported by no more
    than 10 x the largest such ratio that single clcg_hip_solver_preconditioned_c64 solves of the same columns show here."""
    from conftest import GOLDEN
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_c64_ic0")
    p = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = re.findall(r"^column (\d): ret=(-?\d+) iterations=(\d+) residual=(\S+) true_residual=(\S+)", p.stdout, flags=re.M)
    assert [(int(j), int(r)) for j, r, _, _, _ in got] == [(0, CONV), (1, CONV), (2, CONV), (3, ALREADY)], p.stdout
    assert int(got[3][2]) == 0
    S, A = systems["case10k"]
    n = S["n"]
    A.ic0_set_sweeps(0)
    e0 = np.zeros(n, np.complex64); e0[0] = 1.0
    ratios = []
    for bcol in (S["b"], np.float32(2.0) * S["b"], e0):
        m = torch.zeros(n, dtype=torch.complex64, device="cuda")
        info = api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_ic0_mx_c64", None, m,
                                                  torch.from_numpy(np.ascontiguousarray(bcol)).cuda(), n,
                                                  api.clcg_default_parameters(epsilon=1e-6, max_iterations=1000), A)
        assert info.ret == CONV
        x = m.cpu().numpy().astype(np.complex128)
        r = bcol.astype(np.complex128) - S["ops"]["A"](x)
        true = float(np.vdot(r, r).real / max(np.vdot(x, x).real, 1.0))
        ratios.append(true / info.residual)
    bound = 10.0 * max(ratios)
    print("single solves' true / reported:", ratios, "bound", bound, "sample:", got)
    for j, _, its, res, true in got[:3]:
        assert float(res) <= 1e-6 and float(true) <= bound * float(res), (j, res, true, bound)
