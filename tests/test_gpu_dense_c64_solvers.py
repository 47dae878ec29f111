"""-m gpu: the complex64 loops on a dense complex64 handle.  Single-vector: clcg_hip_solver_c64 (BiCG, BiCG-sym) and
clcg_hip_solver_preconditioned_c64 (PCG) through the callbacks clcg_hip_dense_ax_c64 / clcg_hip_dense_jacobi_mx_c64; batched:
clcg_hip_dense_lbicg_sym_multi_c64 and clcg_hip_dense_lpcg_multi_c64 over k = 2, 4, 8 right-hand sides -- every run held to
tests/c64_checker.py's run of the same column alone (tests/dense_c64_cases.py: systems, columns, and the tolerance max(4 d, 64 u) with
d measured on the checker alone and printed by tests/test_dense_c64_cpu.py).

n in {1, 2, 3, 65, 200, 513}.  Capped runs use epsilon = 1e-30 at n >= 65 (never reached in six iterations: code and count are the
cap's) and epsilon = 1e-10 at n <= 3, where a Krylov loop ends after n iterations: past that point a run at epsilon = 1e-30 is
rounding noise (the checker's own residuals there are 1e-14 .. 1e-45, and whether one of them is below 1e-30 depends on the last bit
of a product), while at 1e-10 every residual of the checker's runs is more than three orders of magnitude away from the threshold on
either side, so code and count are the loop's and not the noise's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dense_c64_cases as X
import stream_cases as st
from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BICG, BICG_SYM, PCG, KS = X.BICG, X.BICG_SYM, X.PCG, X.KS
CONV, ALREADY, MAXIT, NANV, NOPRE, E_ARG = X.CONV, X.ALREADY, X.MAXIT, X.NANV, X.NOPRE, X.E_ARG
AX, MX = "clcg_hip_dense_ax_c64", "clcg_hip_dense_jacobi_mx_c64"


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib(api):
    return api.L.load()


@pytest.fixture(scope="module")
def handle(api):
    made = {}

    def get(n):
        if n not in made:
            made[n] = api.DenseMatrix.from_array_c64(X.system(n)["K"])
            made[n].build_jacobi_c64()
        return made[n]
    yield get
    for D in made.values():
        D.destroy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eps(n):
    return 1e-30 if n >= 65 else 1e-10


def _rel(x, ref):
    return float(np.linalg.norm(x.astype(np.complex128) - ref.astype(np.complex128)) / max(np.linalg.norm(ref.astype(np.complex128)), 1e-30))


def _solve(api, kind, D, b, para, Afp=AX, Mfp=MX, mem_host=False):
    n = len(b)
    if mem_host:
        m = np.zeros(n, np.complex64); bb = np.ascontiguousarray(b, np.complex64)
    else:
        m = torch.zeros(n, dtype=torch.complex64, device="cuda"); bb = dev(b)
    if kind == PCG:
        info = api.clcg_solver_preconditioned_c64(Afp, Mfp, None, m, bb, n, para, D)
    else:
        info = api.clcg_solver_c64(Afp, None, m, bb, n, para, D, api.CLCG_BICG if kind == BICG else api.CLCG_BICG_SYM)
    return info, (m if mem_host else m.cpu().numpy())


# ================================================================================================ single-vector loops
@pytest.mark.parametrize("n", X.SIZES)
@pytest.mark.parametrize("kind", [BICG, BICG_SYM, PCG])
def test_capped_runs_against_the_checker(api, lib, handle, kind, n):
    """1 .. 6 iterations: code and count equal the checker's, the iterate within the checker's own tolerance, and BiCG asks its
    callback for K^H once per iteration (the recorded (layout, conjugate) pairs)."""
    S, D = X.system(n), handle(n)
    asked = []
    lib_ax = lib.clcg_hip_dense_ax_c64

    def user_ax(inst, x, y, nn, layout, conj):
        asked.append((layout, conj))
        lib_ax(inst, x, y, nn, layout, conj)

    for k in range(1, 7):
        cap = dict(epsilon=_eps(n), max_iterations=k)
        ref, tol, agree = X.tol_run(S, kind, S["b"], "b", **cap)
        asked.clear()
        info, x = _solve(api, kind, D, S["b"], api.clcg_default_parameters(**cap), Afp=user_ax if kind == BICG else AX)
        assert agree
        assert (info.ret, info.iterations) == (ref["ret"], ref["iters"]), (kind, n, k, info, ref["ret"], ref["iters"])
        rel = _rel(x, ref["x"])
        print(kind, n, k, "rel", rel, "tol", tol)
        assert rel <= tol, (kind, n, k, rel, tol)
        if kind == BICG:
            # K^H once per body: exactly k where the cap ended the run; a run that converged before the cap had its next bodies
            # enqueued before the verdict reached the host (they fall through on the device)
            assert set(asked) == {(0, 0), (1, 1)} and asked[0] == (0, 0), asked
            assert asked.count((1, 1)) == k if info.ret == MAXIT else info.iterations <= asked.count((1, 1)) <= k, (asked, info)
        else:
            assert D.last_kernel == "k_cdn_row"


@pytest.mark.parametrize("n", [65, 200, 513])
@pytest.mark.parametrize("kind", [BICG, BICG_SYM, PCG])
def test_converged_runs(api, handle, kind, n):
    """tests/test_gpu_c64.py::test_converged_runs' rule at epsilon = 1e-10: the distance to the generating x within 10 x the checker's
    own converged error, the count within 10 % (+ 2) of the checker's; host and device memory give the same bits."""
    S, D = X.system(n), handle(n)
    cfg = dict(epsilon=1e-10, max_iterations=3000)
    ref = X.checker_run(S, kind, S["b"], "b", np.complex64, "exact", **cfg)
    assert ref["ret"] == CONV
    info, x = _solve(api, kind, D, S["b"], api.clcg_default_parameters(**cfg))
    assert info.ret == CONV
    err_ref, err = _rel(ref["x"], S["xt"]), _rel(x, S["xt"])
    assert err <= 10 * err_ref, (kind, n, err, err_ref)
    assert abs(info.iterations - ref["iters"]) <= 0.1 * ref["iters"] + 2, (kind, n, info.iterations, ref["iters"])
    info_h, xh = _solve(api, kind, D, S["b"], api.clcg_default_parameters(**cfg), mem_host=True)
    assert (info_h.ret, info_h.iterations) == (info.ret, info.iterations) and xh.tobytes() == x.tobytes()


def test_callbacks_park_their_failures(api, lib):
    """A non-square K, a wrong n_size, PCG without the reciprocals, a handle of another kind: the solve ends with LCG_HIP_E_ARG and m
    untouched."""
    S = X.system(65)
    R = api.DenseMatrix.from_array_c64(np.ascontiguousarray(S["K"][:, :64]))
    D = api.DenseMatrix.from_array_c64(S["K"])
    Dz = api.DenseMatrix.from_array(S["K128"])
    para = api.clcg_default_parameters(epsilon=1e-10, max_iterations=5)
    b = dev(S["b"])

    def refused(call, why):
        m = torch.full((65,), 3 - 1j, dtype=torch.complex64, device="cuda")
        with pytest.raises(api.LcgHipError) as e:
            call(m)
        assert why in str(e.value), str(e.value)
        api.synchronize()
        assert bool((m == 3 - 1j).all())

    refused(lambda m: api.clcg_solver_c64(AX, None, m, b, 65, para, R, api.CLCG_BICG_SYM), "not square")
    refused(lambda m: api.clcg_solver_c64(AX, None, m[:64], b[:64], 64, para, D, api.CLCG_BICG_SYM), "n_size")
    refused(lambda m: api.clcg_solver_preconditioned_c64(AX, MX, None, m, b, 65, para, D), "lcg_hip_dense_build_jacobi_c64")
    refused(lambda m: api.clcg_solver_c64(AX, None, m, b, 65, para, Dz, api.CLCG_BICG_SYM), "complex64")
    refused(lambda m: api.clcg_solver_c64("clcg_hip_dense_ax", None, m, b, 65, para, D, api.CLCG_BICG_SYM), "complex64")
    # a zero on the diagonal: no reciprocals are kept
    Kz = S["K"].copy(); Kz[7, 7] = 0
    Z = api.DenseMatrix.from_array_c64(Kz)
    assert lib.lcg_hip_dense_build_jacobi_c64(Z.h, None) == E_ARG and "diagonal entry 7" in lib.lcg_hip_last_error().decode()
    refused(lambda m: api.clcg_solver_preconditioned_c64(AX, MX, None, m, b, 65, para, Z), "lcg_hip_dense_build_jacobi_c64")
    # the diagonal itself, and the reciprocals applied: c64_checker's formula bit for bit
    d = torch.empty(65, dtype=torch.complex64, device="cuda")
    D.build_jacobi_c64(d)
    api.synchronize()
    assert np.array_equal(d.cpu().numpy(), np.diag(S["K"]))
    r = np.random.default_rng(3)
    x = (r.standard_normal(65) + 1j * r.standard_normal(65)).astype(np.complex64)
    z = torch.empty(65, dtype=torch.complex64, device="cuda")
    lib.clcg_hip_dense_jacobi_mx_c64(D.h, dev(x).data_ptr(), z.data_ptr(), 65, 0, 0)
    api.synchronize()
    want = X.jacobi(S)(x)
    got = z.cpu().numpy()
    # (the device's complex product is c64_mul's fused form; numpy's is not: two fp32 roundings of difference at most)
    assert np.all(np.abs(got - want) <= 4 * X.U32 * np.abs(want)), float(np.max(np.abs(got - want) / np.abs(want)))
    for h in (R, D, Dz, Z):
        h.destroy()


# ================================================================================================ batched loops
def _columns_against_the_checker(S, sid, B, run, para, tag):
    rc, ret, its, res, M = run
    assert rc == 0, (tag, rc)
    for j in range(B.shape[1]):
        bcol = np.ascontiguousarray(B[:, j])
        ref, tol, agree = X.tol_run(S, sid, bcol, ("col", B.shape[1], j), **para)
        if agree:
            assert (ret[j], its[j]) == (ref["ret"], ref["iters"]), (tag, j, ret[j], its[j], ref["ret"], ref["iters"])
        if not ref["x"].any():
            assert not M[:, j].any(), (tag, j)              # (the zero column: already optimised, never stored to)
        else:
            rel = _rel(M[:, j], ref["x"])
            assert rel <= tol, (tag, j, rel, tol)


@pytest.mark.parametrize("n", X.SIZES)
@pytest.mark.parametrize("sid", X.SIDS)
def test_batched_capped_runs_hold_every_column_to_the_checker(api, lib, handle, sid, n):
    """Three iterations (n <= 3: up to six at epsilon = 1e-10), k = 2, 4, 8: every column against the checker's run of that column
    alone -- code and count equal where the checker's summation orders agree, the iterate within the checker's tolerance; the zero
    column is already optimised with no iteration."""
    S, D = X.system(n), handle(n)
    for k in KS:
        B = X.columns(S, k)
        para = dict(epsilon=_eps(n), max_iterations=3 if n >= 65 else 6)
        run = X.cmulti64_dense(lib, api, sid, D, np.zeros_like(B), B, **para)
        _columns_against_the_checker(S, sid, B, run, para, (sid, n, k))
        if k >= 4:
            assert run[1][3] == ALREADY and run[2][3] == 0 and not run[4][:, 3].any()
        assert D.multi_last_kernel == "k_cdnm_mfma"


@pytest.mark.parametrize("n", [65, 200, 513])
@pytest.mark.parametrize("sid", X.SIDS)
def test_batched_converged_runs(api, lib, handle, sid, n):
    """epsilon = 1e-10, k = 8: every column's code is the checker's, its error against the column's solution within 10 x the checker's
    own and its count within 10 % (+ 2)."""
    S, D = X.system(n), handle(n)
    B = X.columns(S, 8)
    para = dict(epsilon=1e-10, max_iterations=3000)
    rc, ret, its, res, M = X.cmulti64_dense(lib, api, sid, D, np.zeros_like(B), B, **para)
    assert rc == 0
    for j in range(8):
        bcol = np.ascontiguousarray(B[:, j])
        ref = X.checker_run(S, sid, bcol, ("col", 8, j), np.complex64, "exact", **para)
        assert ret[j] == ref["ret"], (sid, n, j, ret[j], ref["ret"])
        if ref["ret"] == ALREADY:
            assert its[j] == 0
            continue
        xs = np.linalg.solve(S["K128"], bcol.astype(np.complex128))
        err_ref, err = _rel(ref["x"], xs), _rel(M[:, j], xs)
        assert err <= 10 * err_ref, (sid, n, j, err, err_ref)
        assert abs(its[j] - ref["iters"]) <= 0.1 * ref["iters"] + 2, (sid, n, j, its[j], ref["iters"])


@pytest.mark.parametrize("sid", X.SIDS)
def test_verdict_mix_and_frozen_columns(api, lib, handle, sid):
    """One batch of four: b (runs into the cap), 1e-2 b (|m| stays below 1: converges well before b does), a zero column whose guess is
    all -0.0 (already optimised) and a column of B with a NaN (CLCG_NAN_VALUE at its first iteration).  Each code and count is the
    checker's for that column alone; the already-optimised column's bytes of M are never stored to (still -0.0); the converged
    column's bytes are those of a batch that was capped at its own count (a stopped column is final)."""
    n = 200
    S, D = X.system(n), handle(n)
    B = X.columns(S, 4)
    B[:, 2] = 0
    B[:, 3] = S["b"]; B[5, 3] = complex(np.nan, 0.0)
    full = dict(epsilon=1e-10, max_iterations=3000)
    c_small = X.checker_run(S, sid, np.ascontiguousarray(B[:, 1]), "small", np.complex64, "exact", **full)
    c_b = X.checker_run(S, sid, np.ascontiguousarray(B[:, 0]), "b", np.complex64, "exact", **full)
    assert c_small["ret"] == c_b["ret"] == CONV and c_small["iters"] + 4 <= c_b["iters"]
    cap = c_small["iters"] + 3
    M0 = np.zeros_like(B); M0[:, 2] = complex(-0.0, -0.0)
    para = dict(epsilon=1e-10, max_iterations=cap)
    rc, ret, its, res, M = X.cmulti64_dense(lib, api, sid, D, M0, B, **para)
    assert rc == 0
    assert (ret[0], its[0]) == (MAXIT, cap)
    assert ret[1] == CONV and abs(its[1] - c_small["iters"]) <= 2
    assert (ret[2], its[2]) == (ALREADY, 0) and np.array_equal(X.bits(M[:, 2]), X.bits(M0[:, 2]))
    assert (ret[3], its[3]) == (NANV, 1)
    assert np.isfinite(M[:, :2]).all() and np.isfinite(res[0]) and np.isfinite(res[1])
    # a stopped column is final: capped at its own count, the same bytes
    rc2, ret2, its2, _, M2 = X.cmulti64_dense(lib, api, sid, D, M0, B, epsilon=1e-10, max_iterations=its[1])
    assert rc2 == 0 and (ret2[1], its2[1]) == (CONV, its[1]) and np.array_equal(X.bits(M2[:, 1]), X.bits(M[:, 1]))


@pytest.mark.parametrize("sid", X.SIDS)
def test_a_column_does_not_depend_on_k_place_neighbours_call_or_memory(api, lib, handle, sid):
    """Column j's iterate, count, residual and code: the same bits at k = 2, 4, 8, at every position, beside NaN / Inf / zero columns,
    on a second call, and from host memory."""
    n = 65
    S, D = X.system(n), handle(n)
    B8 = X.columns(S, 8)
    para = dict(epsilon=1e-10, max_iterations=12)
    rc, ret8, its8, res8, M8 = X.cmulti64_dense(lib, api, sid, D, np.zeros_like(B8), B8, **para)
    assert rc == 0
    again = X.cmulti64_dense(lib, api, sid, D, np.zeros_like(B8), B8, **para)
    host = X.cmulti64_dense(lib, api, sid, D, np.zeros_like(B8), B8, mem="host", **para)
    for other in (again, host):
        assert other[:4] == (rc, ret8, its8, res8) and np.array_equal(X.bits(other[4]), X.bits(M8))
    junk = [complex(np.nan, np.nan), complex(np.inf, -np.inf), 0j, complex(1.0, np.nan)]
    for k, pos, j in [(2, 0, 0), (2, 1, 2), (2, 0, 5), (4, 3, 1), (4, 1, 4), (4, 2, 7), (8, 7, 0), (8, 0, 6)]:
        B = np.zeros((n, k), np.complex64)
        for c in range(k):
            B[:, c] = junk[c % 4] if c % 2 == 0 else B8[:, (c + 3) % 8]
        B[:, pos] = B8[:, j]
        rcb, ret, its, res, M = X.cmulti64_dense(lib, api, sid, D, np.zeros_like(B), B, **para)
        assert rcb == 0
        assert (ret[pos], its[pos]) == (ret8[j], its8[j]) and np.float64(res[pos]).tobytes() == np.float64(res8[j]).tobytes(), (k, pos, j)
        assert np.array_equal(X.bits(M[:, pos]), X.bits(M8[:, j])), (k, pos, j)


def test_pcg_without_the_diagonal_and_a_non_square_handle(api, lib):
    S = X.system(65)
    D = api.DenseMatrix.from_array_c64(S["K"])
    R = api.DenseMatrix.from_array_c64(np.ascontiguousarray(S["K"][:, :64]))
    B = X.columns(S, 2)
    M0 = np.full_like(B, 2 + 1j)
    rc, ret, its, res, M = X.cmulti64_dense(lib, api, PCG, D, M0, B, epsilon=1e-10)
    assert rc == NOPRE and ret == [99, 99] and np.array_equal(M, M0)
    rc, ret, its, res, M = X.cmulti64_dense(lib, api, BICG_SYM, D, np.zeros_like(B), B, epsilon=1e-10, max_iterations=2)
    assert rc == 0 and ret == [MAXIT, MAXIT]            # BiCG-sym needs no diagonal
    for sid in X.SIDS:
        rc, ret, its, res, M = X.cmulti64_dense(lib, api, sid, R, M0, B, epsilon=1e-10)
        assert rc == E_ARG and ret == [99, 99] and np.array_equal(M, M0) and "square" in lib.lcg_hip_last_error().decode()
    # the parameter codes of the CSR batch
    D.build_jacobi_c64()
    for sid in X.SIDS:
        assert X.cmulti64_dense(lib, api, sid, D, M0, B, epsilon=2.0)[0] == X.BADEPS
        assert X.cmulti64_dense(lib, api, sid, D, M0, B, epsilon=1e-6, max_iterations=-1)[0] == X.BADMAXIT
    D.destroy(); R.destroy()


# ================================================================================================ a caller's stream
@pytest.fixture(scope="module")
def env(api, lib):
    e = st.make_env(torch, api, lib)
    yield e
    st.close_env(e)


def test_callers_stream(env, api, lib):
    """tests/stream_cases.py's late-input pattern for every complex64 dense entry: run (b) on the side stream, entered while the delay
    runs on it with the inputs written behind the delay, has run (a)'s returned values and bytes."""
    n = 200
    S = X.system(n)
    Ksrc = dev(S["K"])
    Kd = torch.empty_like(Ksrc)
    x_src, X_src, U_src, B_src = dev(S["xt"]), dev(X.columns(S, 4)), dev(X.columns(S, 4)[::-1].copy()), dev(X.columns(S, 4))
    x, Xb, U, Bd = (torch.empty_like(t) for t in (x_src, X_src, U_src, B_src))
    y = torch.empty_like(x); Y = torch.empty_like(Xb); Md = torch.empty_like(Bd); diag = torch.empty_like(x); z = torch.empty_like(x)
    para = api.clcg_default_parameters(epsilon=1e-30, max_iterations=4)
    made = []

    def create():
        D = api.DenseMatrix.from_array_c64(Kd)
        made.append(D)
        D.matvec_c64(x, y)
        return 0

    # a handle made from device memory that is written late, then a product with it
    env.pair([(Kd, Ksrc), (x, x_src)], create, [y], False, tag="create", anchor=lambda r, o: st.no_nan(o, "create"))
    D = api.DenseMatrix.from_array_c64(S["K"])
    for layout, conj in ((0, 0), (0, 1), (1, 0), (1, 1)):
        env.pair([(x, x_src)], lambda: D.matvec_c64(x, y, layout, conj), [y], True, tag=("matvec", layout, conj),
                 anchor=lambda r, o: st.no_nan(o, "matvec"))
    env.pair([(x, x_src)], lambda: lib.clcg_hip_dense_ax_c64(D.h, x.data_ptr(), y.data_ptr(), n, 0, 0), [y], True, tag="ax",
             anchor=lambda r, o: st.no_nan(o, "ax"))
    D.build_jacobi_c64()
    env.pair([(x, x_src)], lambda: lib.clcg_hip_dense_jacobi_mx_c64(D.h, x.data_ptr(), z.data_ptr(), n, 0, 0), [z], True, tag="mx",
             anchor=lambda r, o: st.no_nan(o, "mx"))
    D2 = api.DenseMatrix.from_array_c64(S["K"])
    env.pair([], lambda: D2.build_jacobi_c64(diag), [diag], False, tag="build_jacobi", anchor=lambda r, o: st.no_nan(o, "diag"))
    env.pair([(Xb, X_src)], lambda: D.cmatmat_c64(Xb, Y), [Y], True, tag="matmat", anchor=lambda r, o: st.no_nan(o, "matmat"))
    env.pair([(Xb, X_src), (U, U_src)], lambda: list(D.cop_multi_dot_c64(Xb, Y, U).view(np.float64)), [Y], False, tag="op_multi_dot",
             anchor=lambda r, o: st.no_nan(o, "op"))
    for sid in X.SIDS:
        def call():
            ret = (C.c_int * 4)(*([99] * 4)); its = (C.c_int * 4)(*([-1] * 4)); res = (C.c_double * 4)()
            fn = lib.clcg_hip_dense_lpcg_multi_c64 if sid == PCG else lib.clcg_hip_dense_lbicg_sym_multi_c64
            rc = fn(D.h, 4, Md.data_ptr(), Bd.data_ptr(), C.byref(para), ret, its, res, 1)
            return rc, list(ret), list(its), list(res)

        def anchor(r, outs):
            assert r[0] == 0 and r[1][:3] == [MAXIT] * 3 and r[1][3] == ALREADY and r[2][:3] == [4, 4, 4], r
            st.no_nan(outs, sid)
        env.pair([(Md, torch.zeros_like(Md)), (Bd, B_src)], call, [Md], False, tag=sid, anchor=anchor)
    # the single-vector loops through the callbacks
    m = torch.empty_like(x); b_src = dev(S["b"]); b = torch.empty_like(b_src)
    for kind in (BICG, BICG_SYM, PCG):
        def solve():
            if kind == PCG:
                info = api.clcg_solver_preconditioned_c64(AX, MX, None, m, b, n, para, D)
            else:
                info = api.clcg_solver_c64(AX, None, m, b, n, para, D, api.CLCG_BICG if kind == BICG else api.CLCG_BICG_SYM)
            return info.ret, info.iterations, info.residual

        def anchor1(r, outs):
            assert r[:2] == (MAXIT, 4), (kind, r)
            st.no_nan(outs, kind)
        env.pair([(m, torch.zeros_like(m)), (b, b_src)], solve, [m], False, tag=kind, anchor=anchor1)
    for h in made + [D, D2]:
        h.destroy()


# ================================================================================================ the Python front, the example
def test_python_front(api, lib, handle):
    n = 65
    S, D = X.system(n), handle(n)
    B = X.columns(S, 4)
    para = api.clcg_default_parameters(epsilon=1e-10, max_iterations=3000)
    for sid, fn in ((BICG_SYM, api.dense_clbicg_sym_multi_c64), (PCG, api.dense_clpcg_multi_c64)):
        want = X.cmulti64_dense(lib, api, sid, D, np.zeros_like(B), B, epsilon=1e-10, max_iterations=3000)
        M = torch.zeros((n, 4), dtype=torch.complex64, device="cuda")
        infos = fn(D, M, dev(B), para)
        api.synchronize()
        assert [(i.ret, i.iterations, i.residual) for i in infos] == list(zip(want[1], want[2], want[3]))
        assert np.array_equal(X.bits(M.cpu().numpy()), X.bits(want[4]))
        Mh = X.aligned_block(np.zeros((n, 4), np.complex64))
        infos = fn(D, Mh, X.aligned_block(B), para)
        assert [i.ret for i in infos] == want[1] and np.array_equal(X.bits(Mh), X.bits(want[4]))
    # from_array_c64 widens nothing; from_array keeps widening
    assert D.is_c64 and D.is_complex and (D.m, D.n) == (n, n)
    W = api.DenseMatrix.from_array(S["K"])
    assert not W.is_c64 and W.is_complex
    y = torch.empty(n, dtype=torch.complex128, device="cuda")
    W.matvec(dev(S["xt"].astype(np.complex128)), y)
    api.synchronize()
    assert _rel(y.cpu().numpy(), S["K128"] @ S["xt"].astype(np.complex128)) < 1e-14
    W.destroy()


def test_sample_program_solves_one_and_four_right_hand_sides():
    bindir = os.path.join(ROOT, "examples", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "sample_dense_c64")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sample_dense_c64.cpp"),
                           "-L" + os.path.join(ROOT, "liblcg_amd", "lib"), "-llcg_hip",
                           "-Wl,-rpath,$ORIGIN/../../liblcg_amd/lib", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "BICG_SYM: ret=0" in p.stdout and p.stdout.count("ret=0") == 9 and "k_cdnm_mfma" in p.stdout and "k_cdn_row" in p.stdout, p.stdout
