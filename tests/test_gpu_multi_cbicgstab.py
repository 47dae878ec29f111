"""-m gpu: the batched complex BiCGStab (clcg_hip_lbicgstab_multi) and the two product modes it takes its sums from
(clcg_hip_spmm_inner, clcg_hip_spmm_dot2) on the systems of tests/multi_cbicg_cases.py, every column against the oracle's
orc_clbicgstab on that column alone (plain) or against the helper's numpy restatement of the x-space loop (Jacobi).  Every comparison
hands both sides a shadow vector with non-zero imaginary parts (the default draw is real and cannot tell conj(rb) from rb); one
case uses the seed's own draw.

Bands.  Capped at 3 iterations, the chains and helms also at 6 (epsilon = 1e-20; tests/test_multi_cbicg_cases_cpu.py shows that every
plain case ends at its cap): tests/test_gpu_multi_bicgstab.py's band -- code and count equal; |m_j - x| <= max(1e-9, 50 x the reference
run's own response to 1-ulp changes of b at that count) |x|; the reported residual within 1e-9 relative.  Converged, both rules:
conftest.check_converged_run's rules 1 and 2 as tests/test_gpu_multi_cplx_solvers.py states them for a complex column, with the
band that function keeps for BiCGStab (`wide`: the count within max(3, 4 x the reference's own spread under 1-ulp changes of b, 30 %),
the distance to x_true within 100 x the reference's).

Tiny systems (n = 1, 2, 3): only kernel edges are asserted.  BiCGStab finishes such systems by an exact half step, and whether the
0 / 0 that follows ends as CLCG_NAN_VALUE or as a converged step is decided by one rounding of s = r - ak v."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import multi_cbicg_cases as zb
from multi_cbicg_cases import ALREADY, BADEPS, BADMAXIT, CONV, E_ARG, KS, MAXIT, M_IC0, M_ILU0, M_JACOBI, M_NONE, NANV, NOPRE, bits, cbicg

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


_HANDLES = {}


@pytest.fixture(scope="module")
def handle(api):
    """handle(key) -> (S, CsrMatrix with its Jacobi diagonal), kept for the module."""
    def get(key):
        if key not in _HANDLES:
            S = zb.system(*key)
            A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
            A.build_jacobi()
            _HANDLES[key] = (S, A)
        return _HANDLES[key]
    yield get
    for _, A in _HANDLES.values():
        A.destroy()
    _HANDLES.clear()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def parts(a, b):
    """(re, im) of sum conj(a_i) b_i as two real dots for exact_ref.assert_dot: (x, y) pairs with sum x.y = the part."""
    return ((np.concatenate([a.real, a.imag]), np.concatenate([b.real, b.imag])),
            (np.concatenate([a.real, -a.imag]), np.concatenate([b.imag, b.real])))


# ------------------------------------------------------------------------------------------------------------ 1. the product modes
def _product(lib, A, mode, k, Xd, Ud, n):
    """(Y, sums): mode "inner" -> k complex sums; "dot2" -> (k complex sums, k real sums)."""
    Y = torch.full((n, k), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
    out = (C.c_double * (3 * k))()
    fn = lib.clcg_hip_spmm_inner if mode == "inner" else lib.clcg_hip_spmm_dot2
    assert fn(A.h, k, Xd.data_ptr(), Y.data_ptr(), Ud.data_ptr(), out) == 0, lib.lcg_hip_last_error()
    o = np.array(out[:])
    if mode == "inner":
        return Y.cpu().numpy(), (o[:2 * k].view(np.complex128).copy(),)
    return Y.cpu().numpy(), (o[:2 * k].view(np.complex128).copy(), o[2 * k:].copy())


@pytest.mark.parametrize("mode", ["inner", "dot2"])
@pytest.mark.parametrize("key", [("chain", 3), ("chain", 513), ("helm", 182), ("band30", 1029), ("band140", 2051), ("band260", 261)], ids=zb.sys_id)
def test_product_modes(lib, handle, key, mode):
    """Y has clcg_hip_spmm's bits; the sums are within exact_ref's bound of the extended-precision sums of what the kernel wrote;
    column 0's sums are the same bits at k = 2, 4, 8, with NaN and Inf in the other columns, from call to call."""
    S, A = handle(key)
    n = S["n"]
    rng = np.random.default_rng(11)
    scale = 2.0 ** rng.uniform(-10, 10, (n, 1))
    x0, u0 = crand(rng, n), crand(rng, n) * scale[:, 0]
    ush = crand(rng, n) * scale[:, 0]                  # inner: the ONE vector all columns share
    first = None
    for k in KS:
        Xh, Uh = crand(rng, n, k), crand(rng, n, k) * scale
        Xh[:, 0], Uh[:, 0] = x0, u0
        Xd = dev(Xh)
        Ud = dev(ush) if mode == "inner" else dev(Uh)
        Yh, sums = _product(lib, A, mode, k, Xd, Ud, n)
        Yp = torch.full((n, k), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
        assert lib.clcg_hip_spmm(A.h, k, Xd.data_ptr(), Yp.data_ptr()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(bits(Yh), bits(Yp.cpu().numpy()))                  # Y: the plain product's bits
        for j in range(k):
            y = np.ascontiguousarray(Yh[:, j])
            a, b = (ush, y) if mode == "inner" else (y, np.ascontiguousarray(Uh[:, j]))
            (re_x, re_y), (im_x, im_y) = parts(a, b)
            X.assert_dot(sums[0][j].real, re_x, re_y, (key, mode, k, j, "re"))
            X.assert_dot(sums[0][j].imag, im_x, im_y, (key, mode, k, j, "im"))
            if mode == "dot2":
                X.assert_dot(sums[1][j], *parts(y, y)[0], (key, mode, k, j, "|y|^2"))
        # column 0: the same whatever the others hold (NaN and Inf included), from call to call, whatever k is
        X2, U2 = Xh.copy(), Uh.copy()
        X2[:, 1:] = crand(rng, n, k - 1) * 1e3; U2[:, 1:] = 0.0
        X2[n // 2, 1] = complex(np.nan, 1.0); X2[n - 1, k - 1] = complex(-np.inf, 0.0); U2[0, k - 1] = complex(0.0, np.inf)
        _, other = _product(lib, A, mode, k, dev(X2), Ud if mode == "inner" else dev(U2), n)
        _, again = _product(lib, A, mode, k, Xd, Ud, n)
        col0 = lambda t: [bits(np.asarray(s[0])).tolist() for s in t]
        assert col0(other) == col0(sums), (key, mode, k, "neighbours")
        assert not np.isfinite(other[0][1]), (key, mode, k)                         # (the NaN did reach its own column's sum)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again, sums)), (key, mode, k, "again")
        first = first or col0(sums)
        assert col0(sums) == first, (key, mode, k, sums, first)


def test_product_error_returns_leave_y_alone(api, lib, handle):
    S, A = handle(("chain", 513))
    n = S["n"]
    rng = np.random.default_rng(9)
    Xd = dev(crand(rng, n, 4)); ud = dev(crand(rng, n + 1))
    Y = torch.full((n, 4), 7.0 + 0j, dtype=torch.complex128, device="cuda")
    out = (C.c_double * 12)()
    Ar = api.CsrMatrix.from_csr(S["rp"], S["ci"], np.ascontiguousarray(S["v"].real))
    Ac = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"].astype(np.complex64))
    D = api.DenseMatrix.from_array(crand(rng, 8, 8))
    for name, fn, third in (("clcg_hip_spmm_inner", lib.clcg_hip_spmm_inner, ud), ("clcg_hip_spmm_dot2", lib.clcg_hip_spmm_dot2, Xd)):
        p = third.data_ptr()
        calls = [("k must be", lambda: fn(A.h, 3, Xd.data_ptr(), Y.data_ptr(), p, out)),
                 ("null pointer", lambda: fn(A.h, 4, Xd.data_ptr(), Y.data_ptr(), None, out)),
                 ("null pointer", lambda: fn(A.h, 4, None, Y.data_ptr(), p, out)),
                 ("aligned", lambda: fn(A.h, 4, Xd.data_ptr() + 8, Y.data_ptr(), p, out)),
                 ("aligned", lambda: fn(A.h, 4, Xd.data_ptr(), Y.data_ptr(), p + 8, out)),
                 ("result array", lambda: fn(A.h, 4, Xd.data_ptr(), Y.data_ptr(), p, None)),
                 ("real", lambda: fn(Ar.h, 4, Xd.data_ptr(), Y.data_ptr(), p, out)),
                 ("complex64", lambda: fn(Ac.h, 4, Xd.data_ptr(), Y.data_ptr(), p, out)),
                 ("dense", lambda: fn(D.h, 4, Xd.data_ptr(), Y.data_ptr(), p, out)),
                 ("handle is null", lambda: fn(None, 4, Xd.data_ptr(), Y.data_ptr(), p, out))]
        for what, call in calls:
            assert call() == E_ARG, (name, what)
            err = lib.lcg_hip_last_error().decode()
            assert what in err and name in err, (name, what, err)
            torch.cuda.synchronize()
            assert bool((Y == 7.0).all()), (name, what)
    for M in (Ar, Ac, D):
        M.destroy()


# ------------------------------------------------------------------------------------------------------------ 2. capped
def _compare_capped(ref, sens, ret, its, res, mj, j, tag):
    print("  ", tag, j, "ret", ret, ref["ret"], "its", its, ref["iters"], "residual", res, ref["residual"])
    assert ret == ref["ret"] and its == ref["iters"], (tag, j, ret, ref["ret"], its, ref["iters"])
    nx = np.linalg.norm(ref["x"])
    d = np.linalg.norm(mj - ref["x"]) / nx
    print("      distance", d, "reference run's response", sens)
    assert d <= max(1e-9, 50.0 * sens), (tag, j, d, sens)
    assert abs(res - ref["residual"]) <= 1e-9 * ref["residual"], (tag, j, res, ref["residual"])


def _capped(lib, api, port, handle, key, cap, k, pre):
    S, A = handle(key)
    n = S["n"]
    rb = zb.shadow(port, n)
    B = zb.columns(n, S["b"], k)
    M0 = np.zeros((n, k), np.complex128)
    zero = [j for j in range(k) if not B[:, j].any()]
    for j in zero:
        M0[:, j] = -0.0 - 0.0j          # a guess of zeros that shows a write
    para = dict(epsilon=zb.CAP_EPS, max_iterations=cap)
    rc, ret, its, res, M = cbicg(lib, api, M_NONE if pre is None else M_JACOBI, A, M0, B, rb=rb, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    if pre is None:
        run = lambda b, tag: zb.oracle_column(port, S, b, tag, rb, **para)
    else:
        run = lambda b, tag: zb.restated_column(S, pre, b, tag, rb, **para)
    for j in range(k):
        if j in zero:
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))      # the sign bits too
            continue
        ref = run(B[:, j], ("col", j))
        _compare_capped(ref, zb.response(run, B[:, j], (j,)), ret[j], its[j], res[j], M[:, j], j, (key, k, pre, cap))
    return ret, its


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", zb.CAPPED, ids=lambda c: f"{c[0][0]}-{c[0][1]}-cap{c[1]}")
def test_capped_plain_against_the_oracle(lib, api, port, handle, case, k):
    key, cap = case
    ret, its = _capped(lib, api, port, handle, key, cap, k, None)
    assert ret[0] == MAXIT and its[0] == cap and lib.lcg_hip_last_iterations() == cap
    v, p = C.c_int(), C.c_int()
    lib.lcg_hip_last_launches(C.byref(v), None, None, C.byref(p))
    assert (p.value, v.value) == (1 + 2 * cap, 2 + 3 * cap), (p.value, v.value)     # per iteration: 2 products, 3 passes


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", zb.CAPPED, ids=lambda c: f"{c[0][0]}-{c[0][1]}-cap{c[1]}")
def test_capped_jacobi_against_the_restatement(lib, api, port, handle, case, k):
    key, cap = case
    _capped(lib, api, port, handle, key, cap, k, "jacobi")


def test_capped_from_a_block_of_guesses_and_with_the_seeds_own_draw(lib, api, port, handle):
    """Non-zero guesses (the zero column then has a residual and runs); and the one case whose shadow vector is the library's own draw
    from lcg_hip_set_shadow_seed, which the oracle's vecrnd(n, seed) restates."""
    key, cap, k = ("helm", 40), 6, 4
    S, A = handle(key)
    n = S["n"]
    B, M0 = zb.columns(n, S["b"], k), zb.guesses(S, k)
    para = dict(epsilon=zb.CAP_EPS, max_iterations=cap)
    for name, kw, rb in (("explicit", dict(rb=zb.shadow(port, n)), zb.shadow(port, n)), ("seed", dict(seed=77), port.vecrnd(n, 77))):
        rc, ret, its, res, M = cbicg(lib, api, M_NONE, A, M0, B, **kw, **para)
        assert rc == 0, lib.lcg_hip_last_error()
        for j in range(k):
            run = lambda b, tag: zb.oracle_column(port, S, b, (name,) + tag, rb, m0=M0[:, j].copy(), **para)
            ref = run(B[:, j], ("guess", j))
            if B[:, j].any():
                sens = zb.response(run, B[:, j], ("guess", j))
            else:       # a zero column has no b to move by an ulp: its only input, the guess, is moved instead
                moved = [zb.oracle_column(port, S, B[:, j], (name, "guess-pert", j, s), rb, m0=zb.ulp_changes(M0[:, j], s), **para) for s in range(2)]
                sens = max(np.linalg.norm(m["x"] - ref["x"]) for m in moved) / np.linalg.norm(ref["x"])
            _compare_capped(ref, sens, ret[j], its[j], res[j], M[:, j], j, (key, name, "guess"))
    lib.lcg_hip_set_shadow_seed(1)


# ------------------------------------------------------------------------------------------------------------ 3. converged
_SPREAD = {}


def _converged_column(run, b, tag, got, xt, eps):
    ref = run(b, ("conv",) + tag)
    if tag not in _SPREAD:
        _SPREAD[tag] = max(abs(run(zb.ulp_changes(b, s), ("convpert", s) + tag)["iters"] - ref["iters"]) for s in range(2))
    dit = _SPREAD[tag]
    ret, its, res, x = got
    print("  ", tag, "ret", ret, ref["ret"], "its", its, ref["iters"], "spread", dit, "residual", res)
    assert ret == ref["ret"] == CONV, (tag, ret, ref["ret"])
    assert abs(its - ref["iters"]) <= max(3, 4 * dit, 0.3 * ref["iters"]), (tag, its, ref["iters"], dit)
    assert res <= eps, (tag, res)
    if xt is not None:
        e_gpu, e_ref = np.linalg.norm(x - xt), np.linalg.norm(ref["x"] - xt)
        print("      distance to x_true", e_gpu, "reference's", e_ref)
        assert e_gpu <= 100.0 * max(e_ref, 1e-14 * np.linalg.norm(xt)), (tag, e_gpu, e_ref)


@pytest.mark.parametrize("pre", [None, "jacobi"], ids=["plain", "jacobi"])
@pytest.mark.parametrize("rule", sorted(zb.RULES))
@pytest.mark.parametrize("key,k", [(("helm", 40), 2), (("helm", 40), 8), (("helm", 182), 4), (("band30", 1029), 4), (("band140", 2051), 8)],
                         ids=lambda v: zb.sys_id(v) if isinstance(v, tuple) else f"k{v}")
def test_converged_columns(lib, api, port, handle, key, k, rule, pre):
    S, A = handle(key)
    n, xt = S["n"], S["xt"]
    rb = zb.shadow(port, n)
    B = zb.columns(n, S["b"], k)
    para = zb.RULES[rule]
    M0 = np.zeros((n, k), np.complex128)
    zero = [j for j in range(k) if not B[:, j].any()]
    for j in zero:
        M0[:, j] = -0.0 - 0.0j
    rc, ret, its, res, M = cbicg(lib, api, M_NONE if pre is None else M_JACOBI, A, M0, B, rb=rb, **para)
    assert rc == 0, lib.lcg_hip_last_error()
    print(key, k, rule, pre, "ret", ret, "its", its)
    if pre is None:
        run = lambda b, tag: zb.oracle_column(port, S, b, tag, rb, **para)
    else:
        run = lambda b, tag: zb.restated_column(S, pre, b, tag, rb, **para)
    sols = [xt, zb.cc.SMALL * xt, None, None, -xt, None, 0.5 * xt, 2.0 * xt]
    for j in range(k):
        if j in zero:
            assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j]))
            continue
        _converged_column(run, B[:, j], (key, rule, pre, j), (ret[j], its[j], res[j], M[:, j]), sols[j], para["epsilon"])
    longest = int(np.argmax(its))
    assert lib.lcg_hip_last_iterations() == its[longest] and lib.lcg_hip_last_residual() == res[longest]


# ------------------------------------------------------------------------------------------------------------ 4. a batch is a batch
@pytest.mark.parametrize("pre", [None, "jacobi"], ids=["plain", "jacobi"])
@pytest.mark.parametrize("key", [("helm", 40), ("helm", 182), ("band30", 1029), ("band140", 2051)], ids=zb.sys_id)
def test_independence_of_neighbours_k_place_and_calls(lib, api, port, handle, key, pre):
    """Column j's iterate, count, residual and code: the same bits at k = 2, 4 and 8 in every place, with its neighbours replaced by
    NaN, zero or other data, from call to call, from host memory."""
    S, A = handle(key)
    n = S["n"]
    rb = zb.shadow(port, n)
    precond = M_NONE if pre is None else M_JACOBI
    para = dict(epsilon=1e-10, abs_diff=1, max_iterations=5)
    rng = np.random.default_rng(8)
    b0, m0 = S["b"], 0.1 * crand(rng, n)

    def run(k, pos, others, mem="device"):
        B = np.zeros((n, k), np.complex128); M0 = np.zeros((n, k), np.complex128)
        for j in range(k):
            B[:, j], M0[:, j] = (b0, m0) if j == pos else others(j)
        rc, ret, its, res, M = cbicg(lib, api, precond, A, M0, B, rb=rb, mem=mem, **para)
        assert rc == 0
        return ret[pos], its[pos], res[pos], bits(M[:, pos]).copy()

    def same(a, b, what):
        assert a[:3] == b[:3] and np.array_equal(a[3], b[3]), (what, a[:3], b[:3])

    other = lambda j: (3.0 * np.roll(b0, j + 1), np.zeros(n, np.complex128))
    base = run(4, 0, other)
    assert base[0] in (CONV, MAXIT) and base[1] >= 2, base[:3]
    same(run(4, 0, other), base, "again")
    same(run(4, 0, other, mem="host"), base, "host")
    same(run(4, 0, lambda j: (np.full(n, complex(np.nan, np.nan)), np.zeros(n, np.complex128))), base, "NaN neighbours")
    same(run(4, 0, lambda j: (np.zeros(n, np.complex128), np.zeros(n, np.complex128))), base, "zero neighbours")
    for k in KS:
        for pos in range(k):
            same(run(k, pos, lambda j: (1e3 * np.roll(b0, 7 * j + 1), np.roll(m0, j + 1))), base, ("k", k, "place", pos))


@pytest.mark.parametrize("pre", [None, "jacobi"], ids=["plain", "jacobi"])
def test_verdicts_differ_a_nan_stays_in_its_column_and_stopped_columns_are_final(lib, api, port, handle, pre):
    """Four columns under abs_diff = 1: 0 late (b), 1 early (1e-2 b), 2 a NaN in B, 3 zero -- all four verdicts in one call, which
    returns at max_iterations = 0 although the NaN column never converges."""
    S, A = handle(("helm", 40))
    n, k = S["n"], 4
    rb = zb.shadow(port, n)
    precond = M_NONE if pre is None else M_JACOBI
    B = zb.columns(n, S["b"], k)
    Bn = B.copy(); Bn[n // 2, 2] = complex(np.nan, 1.0)
    M0 = np.zeros((n, k), np.complex128); M0[:, 3] = -0.0 - 0.0j
    para = dict(epsilon=1e-10, abs_diff=1)
    rc, ret, its, res, M = cbicg(lib, api, precond, A, M0, Bn, rb=rb, **para)
    assert rc == 0
    print(pre, ret, its, res)
    assert [ret[0], ret[1], ret[3]] == [CONV, CONV, ALREADY] and ret[2] == NANV and its[2] == 1 and its[3] == 0, (ret, its)
    assert np.array_equal(bits(M[:, 3]), bits(M0[:, 3])) and np.isfinite(M[:, :2].view(np.float64)).all()
    t_fast, t_slow = its[1], its[0]
    assert 0 < t_fast and t_fast + 2 <= t_slow, its
    assert lib.lcg_hip_last_iterations() == t_slow
    # the clean batch: columns 0 and 1 do not see the NaN of column 2
    rc, ret_c, its_c, res_c, M_c = cbicg(lib, api, precond, A, M0, B, rb=rb, **para)
    assert rc == 0 and ret_c[2] == CONV
    for j in (0, 1):
        assert (ret_c[j], its_c[j], res_c[j]) == (ret[j], its[j], res[j]) and np.array_equal(bits(M_c[:, j]), bits(M[:, j])), j
    # frozen means final: the column that converged at t_fast while the others went on = the same batch capped at t_fast
    rc, ret_f, its_f, res_f, M_f = cbicg(lib, api, precond, A, M0, Bn, rb=rb, max_iterations=t_fast, **para)
    assert rc == 0 and ret_f[1] == CONV and its_f[1] == t_fast and ret_f[0] == MAXIT and its_f[0] == t_fast
    assert np.array_equal(bits(M_f[:, 1]), bits(M[:, 1])) and res_f[1] == res[1]
    # ... and a cap between the two counts
    cap = (t_fast + t_slow) // 2
    rc, ret_m, its_m, res_m, M_m = cbicg(lib, api, precond, A, M0, Bn, rb=rb, max_iterations=cap, **para)
    assert rc == 0 and (ret_m[1], its_m[1]) == (CONV, t_fast) and (ret_m[0], its_m[0]) == (MAXIT, cap) and (ret_m[2], its_m[2]) == (NANV, 1)
    assert np.array_equal(bits(M_m[:, 1]), bits(M[:, 1])) and res_m[1] == res[1]


def test_a_batch_column_and_a_single_solve_see_the_same_shadow_vector(lib, api, handle):
    """At the same seed the single-vector clcg_hip_solver(CLCG_BICGSTAB) on clcg_hip_csr_ax and column j of a batch draw the same
    rbar0: the same recurrence, so the capped iterates agree to rounding (they add their sums in different orders)."""
    S, A = handle(("helm", 40))
    n, k, cap = S["n"], 4, 6
    B = zb.columns(n, S["b"], k)
    para = dict(epsilon=zb.CAP_EPS, max_iterations=cap)
    rc, ret, its, res, M = cbicg(lib, api, M_NONE, A, np.zeros((n, k), np.complex128), B, seed=5, **para)
    assert rc == 0
    for j in (0, 2):
        m = torch.zeros(n, dtype=torch.complex128, device="cuda")
        info = api.clcg_solver("clcg_hip_csr_ax", None, m, dev(B[:, j]), n, api.clcg_default_parameters(**para), A, api.CLCG_BICGSTAB, shadow_seed=5)
        torch.cuda.synchronize()
        assert (info.ret, info.iterations) == (ret[j], its[j]) == (MAXIT, cap)
        x = m.cpu().numpy()
        assert np.linalg.norm(M[:, j] - x) <= 1e-9 * np.linalg.norm(x), j
        assert abs(info.residual - res[j]) <= 1e-6 * res[j], j
    lib.lcg_hip_set_shadow_seed(1)


# ------------------------------------------------------------------------------------------------------------ 5. tiny systems
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", (1, 2, 3))
def test_tiny_systems(lib, api, port, n, k):
    S = zb.system("chain", n)
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    A.build_jacobi()
    rb = zb.shadow(port, n)
    B = zb.columns(n, S["b"], k)
    for rule, para in zb.RULES.items():
        for precond in (M_NONE, M_JACOBI):
            M0 = np.zeros((n, k), np.complex128)
            for j in range(k):
                if not B[:, j].any():
                    M0[:, j] = -0.0 - 0.0j
            rc, ret, its, res, M = cbicg(lib, api, precond, A, M0, B, rb=rb, **para)
            assert rc == 0, lib.lcg_hip_last_error()
            print(n, k, rule, precond, "ret", ret, "its", its)
            for j in range(k):
                if not B[:, j].any():
                    assert ret[j] == ALREADY and its[j] == 0 and np.array_equal(bits(M[:, j]), bits(M0[:, j])), (j, ret[j], its[j])
                    continue
                assert ret[j] in (CONV, NANV) and 1 <= its[j] <= n + 1, (j, ret[j], its[j])      # (CONV = 0; NANV = the cap's -1019)
                if np.isfinite(M[:, j]).all() and ret[j] == CONV:      # the host's own value of the stop rule
                    r2 = np.linalg.norm(B[:, j] - S["A"] @ M[:, j]) ** 2
                    host = r2 / n if para["abs_diff"] else r2 * r2 / max(np.linalg.norm(M[:, j]) ** 4, 1.0)
                    assert host <= 2.0 * para["epsilon"] + 1e-28, (j, host)
            again = cbicg(lib, api, precond, A, M0, B, rb=rb, **para)
            assert again[0] == 0 and list(again[1:3]) == [ret, its]
            assert np.array_equal(bits(np.array(again[3])), bits(np.array(res))) and np.array_equal(bits(again[4]), bits(M))
    A.destroy()


# ------------------------------------------------------------------------------------------------------------ 6. error returns
def test_error_returns_release_the_solver(lib, api, port, handle):
    S, A = handle(("helm", 40))
    n, k = S["n"], 4
    rb = zb.shadow(port, n)
    B = zb.columns(n, S["b"], k)
    Z = np.zeros((n, k), np.complex128)
    good = dict(epsilon=1e-10, abs_diff=1, max_iterations=5)
    ref = cbicg(lib, api, M_NONE, A, Z, B, rb=rb, **good)
    assert ref[0] == 0

    def still_works():
        r = cbicg(lib, api, M_NONE, A, Z, B, rb=rb, **good)
        assert r[0] == 0 and r[1:4] == ref[1:4] and np.array_equal(bits(r[4]), bits(ref[4]))
        m = torch.zeros(n, dtype=torch.complex128, device="cuda")
        info = api.clcg_solver("clcg_hip_csr_ax", None, m, dev(S["b"]), n, api.clcg_default_parameters(**good), A, api.CLCG_BICGSTAB)
        assert info.ret == MAXIT and info.iterations == 5

    p = api.clcg_default_parameters(**good)
    Md, Bd = dev(Z), dev(B)
    rng = np.random.default_rng(2)
    Ar = api.CsrMatrix.from_csr(S["rp"], S["ci"], np.ascontiguousarray(S["v"].real))
    Ac = api.CsrMatrix.from_csr_c64(S["rp"], S["ci"], S["v"].astype(np.complex64))
    D = api.DenseMatrix.from_array(crand(rng, 64, 64))
    R = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"], n_cols=n + 5)
    bare = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])            # no Jacobi diagonal

    def raw(h, kk, precond, mptr, mem=1):
        return lib.clcg_hip_lbicgstab_multi(h, kk, precond, mptr, Bd.data_ptr(), C.byref(p), None, None, None, mem)

    for what, call in (("k must be", lambda: raw(A.h, 3, M_NONE, Md.data_ptr())),
                       ("aligned", lambda: raw(A.h, k, M_NONE, Md.data_ptr() + 8)),
                       ("null pointer", lambda: raw(A.h, k, M_NONE, None)),
                       ("real", lambda: raw(Ar.h, k, M_NONE, Md.data_ptr())),
                       ("complex64", lambda: raw(Ac.h, k, M_NONE, Md.data_ptr())),
                       ("dense", lambda: raw(D.h, k, M_NONE, Md.data_ptr())),
                       ("square", lambda: raw(R.h, k, M_NONE, Md.data_ptr())),
                       ("mem", lambda: raw(A.h, k, M_NONE, Md.data_ptr(), 7)),
                       ("precond", lambda: raw(A.h, k, M_IC0, Md.data_ptr())),
                       ("precond", lambda: raw(A.h, k, M_ILU0, Md.data_ptr())),
                       ("precond", lambda: raw(A.h, k, 7, Md.data_ptr()))):
        assert call() == E_ARG, what
        err = lib.lcg_hip_last_error().decode()
        assert what in err and "clcg_hip_lbicgstab_multi" in err, (what, err)
        still_works()
    torch.cuda.synchronize()
    assert not Md.cpu().numpy().any()
    for para, code in ((dict(epsilon=0.0), BADEPS), (dict(epsilon=1.0), BADEPS), (dict(max_iterations=-1), BADMAXIT)):
        for precond in (M_NONE, M_JACOBI):
            r = cbicg(lib, api, precond, A, Z, B, rb=rb, **para)
            assert r[0] == code and r[1] == [99] * k and not r[4].any(), (para, precond, r[0])
        still_works()
    r = cbicg(lib, api, M_JACOBI, bare, Z, B, rb=rb, **good)
    assert r[0] == NOPRE and r[1] == [99] * k and r[2] == [-1] * k and not r[4].any()       # nothing ran, nothing was reported
    assert cbicg(lib, api, M_NONE, bare, Z, B, rb=rb, **good)[1:4] == ref[1:4]              # the plain loop needs no diagonal
    still_works()
    for M in (Ar, Ac, D, R, bare):
        M.destroy()


# ------------------------------------------------------------------------------------------------------------ 7. front and sample
def test_python_front(api, lib, port, handle):
    S, A = handle(("helm", 40))
    n = S["n"]
    Bh = zb.columns(n, S["b"], 4)
    B = dev(Bh)
    p = api.clcg_default_parameters(epsilon=1e-10, abs_diff=1)
    M = torch.zeros((n, 4), dtype=torch.complex128, device="cuda")
    infos = api.clbicgstab_multi(A, M, B, p)
    assert [i.ret for i in infos] == [CONV, CONV, CONV, ALREADY] and infos[3].iterations == 0
    Mj = np.zeros((n, 4), np.complex128)
    infos_j = api.clbicgstab_multi(A, Mj, Bh, p, precond="jacobi")
    assert [i.ret for i in infos_j] == [CONV, CONV, CONV, ALREADY]
    assert np.linalg.norm(Mj[:, 0] - M[:, 0].cpu().numpy()) <= 1e-4 * np.linalg.norm(Mj[:, 0])
    Y = torch.full((n, 4), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
    u = dev(zb.shadow(port, n))
    s1 = A.cspmm_inner(M, Y, u)
    Yh, uh = Y.cpu().numpy(), u.cpu().numpy()
    assert np.linalg.norm((Yh - Bh)[:, 0]) ** 2 / n <= 2e-10            # (the abs rule is sum |r|^2 / n <= 1e-10)
    assert np.allclose(s1, np.conj(uh) @ Yh, rtol=1e-12, atol=1e-12 * np.linalg.norm(uh) * np.linalg.norm(Yh))
    s2, q2 = A.cspmm_dot2(M, Y, B)
    assert np.allclose(s2, np.einsum("ij,ij->j", np.conj(Yh), Bh), rtol=1e-12) and np.allclose(q2, np.einsum("ij,ij->j", np.conj(Yh), Yh).real, rtol=1e-12)
    with pytest.raises(ValueError):
        api.clbicgstab_multi(A, Mj, Bh, p, precond="ic0")


def test_sample_program_solves_four_sources_plain_and_with_jacobi():
    import re
    import subprocess
    from test_dropin_cpp import _build
    exe = _build("sample_csr_multi_c128_bicgstab")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = re.findall(r"^(plain|jacobi) column (\d): ret=(-?\d+) iterations=(\d+)", p.stdout, flags=re.M)
    assert [(w, int(j), int(r)) for w, j, r, _ in got] == [(w, j, ALREADY if j == 3 else CONV) for w in ("plain", "jacobi") for j in range(4)]
    assert all(int(t) > 0 for _, j, _, t in got if int(j) != 3)
