"""-m gpu: the three staged entries (clcg_hip_spmm_inner, clcg_hip_spmm_dot2, clcg_hip_lbicgstab_multi) on a caller's stream, under
the late-input pattern of tests/stream_cases.py (make_env, env.pair): run (a) on the library's own stream with the inputs ready, run
(b) on a non-blocking side stream entered while the delay is still running and the inputs are written behind it; (b) must give (a)'s
bits in every output and returned scalar.  k = 2 and 8 on helm 40 and helm 182 (more than MM_MG row blocks: the folded sums) of
tests/multi_cbicg_cases.py; the loop capped at 6 and converged, plain and with Jacobi.  The shadow residual is host-side state that
the solve uploads on its stream: it is handed over before every call."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import multi_cbicg_cases as zb
import stream_cases as st

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KEYS = [("helm", 40), ("helm", 182)]


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available(), "GPU tests need the MI355X; there is no CPU fallback"
    return a


@pytest.fixture(scope="module")
def lib(api):
    from liblcg_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def env(api, lib):
    e = st.make_env(torch, api, lib)
    yield e
    st.close_env(e)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("key", KEYS, ids=zb.sys_id)
def test_complex_block_products_with_conjugated_sums(env, api, lib, key):
    """clcg_hip_spmm_inner (u, one vector, written late too) and clcg_hip_spmm_dot2 at k = 2 and 8: Y and the returned sums."""
    S = zb.system(*key)
    n = S["n"]
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    try:
        for k in (2, 8):
            rng = np.random.default_rng(500 + k + n)
            Xh, Uh, uh = crand(rng, n, k), crand(rng, n, k), crand(rng, n)
            Xs, Us, us = dev(Xh), dev(Uh), dev(uh)
            Xd, Ud, ud, Y = torch.empty_like(Xs), torch.empty_like(Xs), torch.empty_like(us), torch.empty_like(Xs)

            def rows(outs):
                for j in range(k):
                    X.assert_rows(np.ascontiguousarray(outs[0][:, j]), S["rp"], S["ci"], S["v"], Xh[:, j], (key, k, j))

            def inner():
                out = (C.c_double * (2 * k))()
                assert lib.clcg_hip_spmm_inner(A.h, k, Xd.data_ptr(), Y.data_ptr(), ud.data_ptr(), out) == 0, lib.lcg_hip_last_error()
                return list(out)

            def anchor_inner(r, outs):
                rows(outs)
                for j in range(k):
                    y = np.ascontiguousarray(outs[0][:, j])
                    X.assert_dot(r[2 * j], np.concatenate([uh.real, uh.imag]), np.concatenate([y.real, y.imag]), (key, k, j, "re"))
                    X.assert_dot(r[2 * j + 1], np.concatenate([uh.real, -uh.imag]), np.concatenate([y.imag, y.real]), (key, k, j, "im"))
            env.pair([(Xd, Xs), (ud, us)], inner, [Y], enqueue_only=False, tag=("inner", key, k), anchor=anchor_inner)

            def dot2():
                out = (C.c_double * (3 * k))()
                assert lib.clcg_hip_spmm_dot2(A.h, k, Xd.data_ptr(), Y.data_ptr(), Ud.data_ptr(), out) == 0, lib.lcg_hip_last_error()
                return list(out)

            def anchor_dot2(r, outs):
                rows(outs)
                for j in range(k):
                    y, u = np.ascontiguousarray(outs[0][:, j]), np.ascontiguousarray(Uh[:, j])
                    X.assert_dot(r[2 * j], np.concatenate([y.real, y.imag]), np.concatenate([u.real, u.imag]), (key, k, j, "re"))
                    X.assert_dot(r[2 * j + 1], np.concatenate([y.real, -y.imag]), np.concatenate([u.imag, u.real]), (key, k, j, "im"))
                    X.assert_dot(r[2 * k + j], np.concatenate([y.real, y.imag]), np.concatenate([y.real, y.imag]), (key, k, j, "|y|^2"))
            env.pair([(Xd, Xs), (Ud, Us)], dot2, [Y], enqueue_only=False, tag=("dot2", key, k), anchor=anchor_dot2)
    finally:
        A.destroy()


@pytest.mark.parametrize("pre", [None, "jacobi"], ids=["plain", "jacobi"])
@pytest.mark.parametrize("key", KEYS, ids=zb.sys_id)
def test_batched_complex_bicgstab(env, api, lib, port, key, pre):
    """clcg_hip_lbicgstab_multi at k = 2 and 8, capped at 6 and converged: per column code, count, residual and iterate."""
    S = zb.system(*key)
    n = S["n"]
    rb = zb.shadow(port, n)
    A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
    try:
        A.build_jacobi()
        precond = zb.M_NONE if pre is None else zb.M_JACOBI
        for k in (2, 8):
            Bs, M0s = dev(zb.columns(n, S["b"], k)), dev(zb.guesses(S, k))
            Bd, Md = torch.empty_like(Bs), torch.empty_like(M0s)
            for cap in (6, 0):
                para = api.clcg_default_parameters(max_iterations=cap, epsilon=1e-10, abs_diff=1)

                def call():
                    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
                    assert lib.lcg_hip_set_shadow_vector(rb.ctypes.data, n) == 0
                    rc = lib.clcg_hip_lbicgstab_multi(A.h, k, precond, Md.data_ptr(), Bd.data_ptr(), C.byref(para), ret, its, res, 1)
                    return rc, list(ret), list(its), list(res)

                def anchor(r, outs):
                    rc, ret, its, res = r
                    assert rc == 0 and 99 not in ret and -1 not in its, (key, pre, k, cap, r)
                    st.no_nan(outs, (key, pre, k, cap))
                    if cap == 0:        # column 0 (b itself from a zero guess) converges
                        assert ret[0] == zb.CONV and its[0] > 0, (key, pre, k, r)
                    else:
                        assert max(its) == cap, (key, pre, k, r)
                env.pair([(Md, M0s), (Bd, Bs)], call, [Md], False, tag=(key, pre, k, cap), anchor=anchor)
    finally:
        A.destroy()
