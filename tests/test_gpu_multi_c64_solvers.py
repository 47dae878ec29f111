"""-m gpu: the batched complex64 loops (clcg_hip_lbicg_sym_multi_c64, clcg_hip_lpcg_multi_c64) for k = 2, 4, 8, every column
against the checker's complex64 run of that column alone (tests/c64_checker.py); then what makes a batch a batch: columns that stop
at different iterations and stay final, a NaN that stays in its column, columns that do not depend on their neighbours or on k, and
the error returns.  Systems, columns and the driver: tests/multi_c64_cases.py (tests/test_multi_c64_cases_cpu.py shows with the
checker alone that the cases are what they claim).

The band of a capped run is tests/test_gpu_c64.py's _tol rule: two fp32 evaluations of the same recurrence lie about as far from
each other as the checker's complex64 run lies from its complex128 twin -- 4 x that distance, never below 64 x 2^-24."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import c64_checker as K
import multi_c64_cases as cc
from multi_c64_cases import ALREADY, BADEPS, BADMAXIT, BICG_SYM, CONV, E_ARG, KS, MAXIT, NANV, NOPRE, PCG, SIDS, bits, cmulti64

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAMES = ["b", "small", "rand", "zero", "minus", "rand3", "half", "twice"]


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


_HANDLES = {}


@pytest.fixture(scope="module")
def handle(api):
    """handle(kind, n) -> (S, CsrMatrix with its Jacobi diagonal), kept for the module."""
    def get(kind, n=0):
        if (kind, n) not in _HANDLES:
            S = cc.system(kind, n)
            A = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"])
            A.build_jacobi()
            _HANDLES[(kind, n)] = (S, A)
        return _HANDLES[(kind, n)]
    yield get
    for _, A in _HANDLES.values():
        A.destroy()
    _HANDLES.clear()


def zeros(S, k):
    M0 = np.zeros((S["n"], k), np.complex64)
    if k >= 4:
        M0[:, 3] = -0.0 - 0.0j      # a guess of zeros that shows a write
    return M0


def check_capped(lib, api, S, A, sid, k, cap, strict=True):
    """One batch capped at `cap` against the checker, column by column.  strict: the checker's run is still going at the cap, so code
    -1019, the count and the residual are required too."""
    B, M0 = cc.columns(S, k), zeros(S, k)
    para = dict(epsilon=1e-30, max_iterations=cap)
    rc, ret, its, res, M = cmulti64(lib, api, sid, A, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        if not B[:, j].any():
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j])), (j, ret[j], its[j])
            continue
        ref, tol = cc.tol_column(S, sid, B[:, j], ("col", NAMES[j]), **para)
        rel = np.linalg.norm(M[:, j].astype(np.complex128) - ref["x"]) / np.linalg.norm(ref["x"])
        print(S["key"], sid, k, cap, j, "ret", ret[j], ref["ret"], "its", its[j], ref["iters"], "distance", rel, "tol", tol,
              "residual", res[j], ref["residual"])
        assert rel <= tol, (sid, k, cap, j, rel, tol)
        if strict:
            assert ret[j] == ref["ret"] == MAXIT and its[j] == ref["iters"] == cap, (j, ret[j], its[j], ref["ret"], ref["iters"])
            assert abs(res[j] - ref["residual"]) <= max(8 * tol, 1e-5) * ref["residual"], (j, res[j], ref["residual"])
    return ret, its


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", SIDS)
def test_capped_runs_against_the_checker(lib, api, handle, sid, k):
    S, A = handle("helmholtz", 100)
    for cap in range(1, 7):
        check_capped(lib, api, S, A, sid, k, cap)
        assert lib.lcg_hip_last_iterations() == cap
    vec, prod = C.c_int(), C.c_int()
    lib.lcg_hip_last_launches(C.byref(vec), None, None, C.byref(prod))
    assert (prod.value, vec.value) == (1 + 6, 2 + 2 * 6)        # three launches per iteration, three for the setup


_DIRECT = {}


def direct(S, b):
    """The complex128 direct solve of one column (the factor shared)."""
    if S["key"] not in _DIRECT:
        import scipy.sparse.linalg as spl
        _DIRECT[S["key"]] = spl.splu(S["ops"]["matrix"].tocsc())
    return _DIRECT[S["key"]].solve(b.astype(np.complex128))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", SIDS)
def test_converged_runs(lib, api, handle, sid, k):
    """tests/test_gpu_c64.py's test_converged_runs rules per column, to eps = 1e-10 on |r|^2 / max(|m|, 1)^2: code 0, the count within
    10 % + 2 of the checker's, the distance to the complex128 direct solve of that column within 10 x the checker's own."""
    S, A = handle("helmholtz", 100)
    B, M0 = cc.columns(S, k), zeros(S, k)
    para = dict(epsilon=1e-10, max_iterations=3000)
    rc, ret, its, res, M = cmulti64(lib, api, sid, A, M0, B, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    for j in range(k):
        if not B[:, j].any():
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            continue
        ref = cc.checker_column(S, sid, B[:, j], ("col", NAMES[j]), **para)
        xd = direct(S, B[:, j])
        err_ref = np.linalg.norm(ref["x"] - xd) / np.linalg.norm(xd)
        err = np.linalg.norm(M[:, j] - xd) / np.linalg.norm(xd)
        print(sid, k, j, "ret", ret[j], "its", its[j], ref["iters"], "error", err, "checker's", err_ref, "residual", res[j])
        assert ret[j] == ref["ret"] == CONV
        assert abs(its[j] - ref["iters"]) <= 0.1 * ref["iters"] + 2, (j, its[j], ref["iters"])
        assert err <= 10 * err_ref, (j, err, err_ref)
        assert res[j] <= 1e-10
    longest = int(np.argmax(its))
    assert lib.lcg_hip_last_iterations() == its[longest] and lib.lcg_hip_last_residual() == res[longest]


@pytest.mark.parametrize("sid", SIDS)
def test_independence_and_freezing(lib, api, handle, sid):
    """helmholtz(40), eps = 1e-8: 1e-2 b stops at least two iterations before b and the random column.  Every column's M bytes, count,
    residual and code are identical in a k = 4 batch, a k = 2 batch (1e-2 b with the zero column), a k = 8 batch and a k = 4 batch
    whose random column holds a NaN in B -- that one ends with CLCG_NAN_VALUE at count 1 and touches nobody."""
    S, A = handle("helmholtz", 40)
    n = S["n"]
    para = dict(epsilon=1e-8, max_iterations=3000)

    def run(B, names):
        M0 = np.zeros(B.shape, np.complex64)
        rc, ret, its, res, M = cmulti64(lib, api, sid, A, M0, B, **para)
        assert rc == 0, lib.lcg_hip_last_error()
        return {nm: (ret[j], its[j], res[j], bits(M[:, j]).copy()) for j, nm in enumerate(names)}

    base = run(cc.columns(S, 4), NAMES[:4])
    print(sid, {nm: v[:3] for nm, v in base.items()})
    assert [base[nm][0] for nm in NAMES[:4]] == [CONV, CONV, CONV, ALREADY] and base["zero"][1] == 0
    assert base["small"][1] + 2 <= min(base["b"][1], base["rand"][1]), {nm: v[1] for nm, v in base.items()}
    Bnan = cc.columns(S, 4)
    Bnan[n // 2, 2] = complex(np.nan, 1.0)
    batches = {"k2": run(cc.pair_small_zero(S), ["small", "zero"]), "k8": run(cc.columns(S, 8), NAMES),
               "again": run(cc.columns(S, 4), NAMES[:4]), "nan": run(Bnan, ["b", "small", "nan", "zero"])}
    assert batches["nan"]["nan"][:2] == (NANV, 1)
    for tag, got in batches.items():
        for nm, v in got.items():
            if nm in base:
                assert v[:3] == base[nm][:3] and np.array_equal(v[3], base[nm][3]), (tag, nm, v[:3], base[nm][:3])
    # frozen means final: the column that converged early = the same batch capped at its count
    t = base["small"][1]
    M0 = np.zeros((n, 4), np.complex64)
    rc, ret, its, res, M = cmulti64(lib, api, sid, A, M0, cc.columns(S, 4), epsilon=1e-8, max_iterations=t)
    assert rc == 0 and (ret[1], its[1], res[1]) == base["small"][:3] and ret[0] == MAXIT and its[0] == t
    assert np.array_equal(bits(M[:, 1]), base["small"][3])


@pytest.mark.parametrize("key", [("chain", 1), ("chain", 2), ("chain", 3), ("chain", 65), ("chain", 513), ("helm", 182)],
                         ids=lambda k: f"{k[0]}-{k[1]}")
@pytest.mark.parametrize("sid", SIDS)
def test_sizes_capped_at_4(lib, api, handle, sid, key):
    """n = 1, 2, 3 (fewer rows than lanes of a piece group), 65, 513, and helm 182 (n = 33124: the folded d.Ad and a thread's second
    stride in the TREE pass), every k.  Where n < 4 the Krylov space is used up before the cap: what is left of r is rounding, and
    whether a column then counts on, converges or breaks down is decided by the last bit -- the iterate is held to the band, the
    verdict is not."""
    S, A = handle(*key)
    for k in KS:
        check_capped(lib, api, S, A, sid, k, 4, strict=S["n"] >= 4)


@pytest.mark.parametrize("sid", SIDS)
def test_host_and_device_memory_give_the_same_bytes(lib, api, handle, sid):
    S, A = handle("helmholtz", 40)
    B, M0 = cc.columns(S, 4), zeros(S, 4)
    a = cmulti64(lib, api, sid, A, M0, B, mem="device", epsilon=1e-8)
    b = cmulti64(lib, api, sid, A, M0, B, mem="host", epsilon=1e-8)
    assert a[0] == b[0] == 0 and a[1:4] == b[1:4] and a[4].tobytes() == b[4].tobytes()
    assert a[1] == [CONV, CONV, CONV, ALREADY]


def test_parameter_and_handle_refusals(lib, api, handle):
    S, A = handle("helmholtz", 40)
    n, k = S["n"], 4
    B, Z = cc.columns(S, k), np.zeros((S["n"], k), np.complex64)
    good = dict(epsilon=1e-8, max_iterations=10)
    ref = cmulti64(lib, api, BICG_SYM, A, Z, B, **good)
    assert ref[0] == 0

    def still_works():
        r = cmulti64(lib, api, BICG_SYM, A, Z, B, **good)
        assert r[0] == 0 and r[1:4] == ref[1:4] and np.array_equal(bits(r[4]), bits(ref[4]))

    bare = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"])         # no Jacobi diagonal
    r = cmulti64(lib, api, PCG, bare, Z, B, **good)
    assert r[0] == NOPRE and r[1] == [99] * k                           # nothing ran, nothing was reported
    assert cmulti64(lib, api, PCG, bare, Z, B, epsilon=0.0)[0] == BADEPS    # the parameters come first
    still_works()
    assert cmulti64(lib, api, BICG_SYM, bare, Z, B, **good)[0] == 0     # BiCG-sym needs no diagonal
    bare.destroy()
    A128 = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"].astype(np.complex128))
    A128.build_jacobi()
    Areal = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"].real.astype(np.float64))
    rect = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"], n_cols=n + 5)
    for sid in SIDS:
        assert cmulti64(lib, api, sid, A, Z, B, epsilon=0.0)[0] == BADEPS
        assert cmulti64(lib, api, sid, A, Z, B, epsilon=1.0)[0] == BADEPS
        assert cmulti64(lib, api, sid, A, Z, B, max_iterations=-1)[0] == BADMAXIT
        still_works()
        for H, word in ((A128, "complex128"), (Areal, "real")):
            r = cmulti64(lib, api, sid, H, Z, B, **good)
            assert r[0] == E_ARG and r[1] == [99] * k and np.array_equal(bits(r[4]), bits(Z)), (sid, word, r[0])
            assert word in lib.lcg_hip_last_error().decode()
        assert cmulti64(lib, api, sid, rect, Z, B, **good)[0] == E_ARG and "square" in lib.lcg_hip_last_error().decode()
        fn = lib.clcg_hip_lpcg_multi_c64 if sid == PCG else lib.clcg_hip_lbicg_sym_multi_c64
        Zd = torch.zeros((n, k), dtype=torch.complex64, device="cuda")
        assert fn(A.h, k, Zd.data_ptr(), Zd.data_ptr(), None, None, None, None, 7) == E_ARG and "mem" in lib.lcg_hip_last_error().decode()
        still_works()
    # the complex128 batch still refuses the complex64 handle
    Zz = torch.zeros((n, k), dtype=torch.complex128, device="cuda")
    assert lib.clcg_hip_lbicg_sym_multi(A.h, k, Zz.data_ptr(), Zz.data_ptr(), None, None, None, None, 1) == E_ARG
    assert "complex64" in lib.lcg_hip_last_error().decode()
    for H in (A128, Areal, rect):
        H.destroy()


def test_repeated_solves_do_not_grow_device_memory(api, lib):
    """Modelled on tests/test_gpu_c64.py's test of the same name: handles, Jacobi diagonals and batched solves of both loops at every
    k, three rounds; after destroy and trim the device has its memory back.  (n = 90000: a matrix of 5 MB and work vectors of 6 MB at
    k = 8 show in the device's free memory, which is first cleared of what earlier tests left in the library's pool and torch's cache.)"""
    S = cc.system("helmholtz", 300)
    torch.cuda.empty_cache()
    assert lib.lcg_hip_trim() == 0
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for rnd in range(3):
        A = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"])
        A.build_jacobi()
        for sid in SIDS:
            for k in KS:
                B = torch.from_numpy(cc.columns(S, k)).cuda()
                for _ in range(3):
                    M = torch.zeros_like(B)
                    f = api.clpcg_multi_c64 if sid == PCG else api.clbicg_sym_multi_c64
                    infos = f(A, M, B, api.clcg_default_parameters(epsilon=1e-30, max_iterations=5))
                    assert infos[0].ret == MAXIT and infos[0].iterations == 5
                del B, M
        if rnd == 0:
            torch.cuda.synchronize()
            free1 = torch.cuda.mem_get_info()[0]
        A.destroy()
        torch.cuda.empty_cache()
        assert lib.lcg_hip_trim() == 0
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)
    assert free1 < free0


def test_python_front(api, handle):
    S, A = handle("helmholtz", 40)
    n = S["n"]
    Bh = cc.columns(S, 4)
    B = torch.from_numpy(Bh).cuda()
    p = api.clcg_default_parameters(epsilon=1e-8)
    for f in (api.clbicg_sym_multi_c64, api.clpcg_multi_c64):
        M = torch.zeros((n, 4), dtype=torch.complex64, device="cuda")
        infos = f(A, M, B, p)
        assert [i.ret for i in infos] == [CONV, CONV, CONV, ALREADY] and infos[3].iterations == 0
        Y = torch.full((n, 4), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
        A.cspmm_c64(M, Y)
        api.synchronize()
        r = (Y - B).cpu().numpy()
        assert np.linalg.norm(r[:, 0]) <= 1e-3 * np.linalg.norm(Bh[:, 0])
        Mh = cc.aligned_block(np.zeros((n, 4), np.complex64))
        infos_h = f(A, Mh, cc.aligned_block(Bh), p)
        assert [i.ret for i in infos_h] == [CONV, CONV, CONV, ALREADY]
        assert np.array_equal(bits(Mh), bits(M.cpu().numpy()))


def test_sample_program_one_batch_against_eight_single_solves():
    """examples/sample_csr_multi_c64.cpp compiles with plain g++ against the header and runs sample14's system against eight scaled
    sources: every column's averaged error, in the batch and alone, within 3 x (+ 1e-7) of the checker's run of that column with
    the same cap (tests/test_gpu_c64.py's test_cpp_sample rule)."""
    from conftest import GOLDEN
    from test_dropin_cpp import _build
    from test_gpu_c64 import case
    exe = _build("sample_csr_multi_c64")
    p = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = re.findall(r"^column (\d): batch ret=(-?\d+) iterations=(\d+) error=(\S+) \| single ret=(-?\d+) iterations=(\d+) error=(\S+)",
                      p.stdout, flags=re.M)
    assert [int(r[0]) for r in rows] == list(range(8)) * 2, p.stdout
    assert "clcg_hip_lbicg_sym_multi_c64" in p.stdout and "clcg_hip_lpcg_multi_c64" in p.stdout
    rp, ci, v, b, xs = case("10K")
    ops = K.csr_ops(rp, ci, v, np.complex64)
    jac = K.jacobi(rp, ci, v)
    n = len(b)
    cfg = {"epsilon": 1e-6, "max_iterations": 200}
    scale = [1.0, 0.5, -1.0, 2.0, 0.25, -0.5, 4.0, -2.0]
    for i, r in enumerate(rows):
        s = np.float32(scale[i % 8])
        bj, m0 = (s * b).astype(np.complex64), np.zeros(n, np.complex64)
        ref = K.bicg_sym(ops["A"], bj, m0, cfg) if i < 8 else K.pcg(ops["A"], jac, bj, m0, cfg)
        e_ref = float(np.linalg.norm((ref["x"] - (s * xs).astype(np.complex64)).astype(np.complex128)) / n)
        print(r, "checker", ref["ret"], ref["iters"], e_ref)
        assert int(r[1]) in (CONV, MAXIT) and int(r[4]) in (CONV, MAXIT)
        assert float(r[3]) <= 3 * e_ref + 1e-7 and float(r[6]) <= 3 * e_ref + 1e-7, (r, e_ref)
