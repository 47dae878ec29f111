"""Restatement vs the compiled reference.

Every case is held to the reference's own outputs stored in tests/golden/ref_pins.npz
(tests/golden/make_ref_pins.py wrote them from oracle/_ref/liblcg_ref.so; each solution
vector as the SHA-256 of its bytes), so the checks run on every machine.  Where
oracle/_ref/liblcg_ref.so is present (built by build() where the reference sources exist;
on the GPU box the prebuilt .so travels with the snapshot) the compiled reference is ALSO
run live beside the pins.  Nothing here reads the reference's
sources at run time.
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from oracle import pyoracle as po

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pins.npz")

RHS_SIDS = [(0, 0), (1, 1), (2, 0), (3, 0)]
RHS_TOLS = [(1e-6, 0), (1e-10, 1)]
GEN_SYSTEMS = [
    ("diagonals", 4000, 300, True, 1, (0, 1, 2, 3)),
    ("scrambled", 2500, 0, True, 0, (0, 1)),
    ("row-random band", 3000, 200, True, 2, (0, 1, 3)),
    ("non-symmetric", 3000, 250, False, 1, (2, 3)),
]
GEN_TOLS = ((1e-6, 0), (1e-11, 1))
X_HEAD = 4             # leading entries of each solution kept beside its digest
SEED_REPLAY_SIDS = [po.CLCG_BICG_SYM, po.CLCG_CGS, po.CLCG_TFQMR]
OTHER_TWO_SIDS = [po.CLCG_BICG, po.CLCG_BICGSTAB]


# ---- inputs and pin keys (shared with tests/golden/make_ref_pins.py) ----------------------------------------------------------
def rhs_inputs(n, sid):
    rng = np.random.default_rng(100 + sid)
    b = rng.standard_normal(n); m0 = rng.standard_normal(n) * 0.1
    return b, m0


def gen_inputs(port, tag, n, band, sym, pattern):
    g = port.gen_init(n, 16, band, sym, seed=7, diag_shift=0.01, pattern=pattern)
    rp, ci, v = port.gen_rows(g)
    rng = np.random.default_rng(sum(map(ord, tag)))
    b = rng.standard_normal(n); m0 = rng.standard_normal(n) * 0.1
    return rp, ci, v, b, m0


def dot_inputs():
    rng = np.random.default_rng(5)
    return rng.standard_normal(4097), rng.standard_normal(4097)


def rhs_para(eps, ad):
    return po.default_para(epsilon=eps, abs_diff=ad)


def gen_para(eps, ad):
    return po.default_para(epsilon=eps, abs_diff=ad, max_iterations=400)


def seed_replay_para():
    return po.default_cpara(epsilon=1e-8, abs_diff=1)


def other_two_para():
    return po.default_cpara(epsilon=1e-8, abs_diff=1, max_iterations=150)


def rhs_key(sid, eps, ad):
    return f"rhs/{sid}/{eps:g}/{ad}"


def gen_key(tag, sid, eps):
    return f"gen/{tag}/{sid}/{eps:g}"


def cplx_key(kind, sid):
    return f"{kind}/{sid}"


def x_digest(x):
    """SHA-256 of the solution vector's bytes (float64 / complex128, little-endian): equal digests = equal vectors, bit for bit."""
    x = np.ascontiguousarray(x, "<c16" if np.iscomplexobj(x) else "<f8")
    return np.frombuffer(hashlib.sha256(x.tobytes()).digest(), np.uint8)


def record(r):
    """A solve's outputs as pin arrays: return code, count, the seed the reference drew its shadow residual from (where it drew one),
    residual, and the solution vector as its digest plus its first entries (these only make a failure readable)."""
    return {"meta": np.array([r["ret"], r["iters"], r.get("seed_before", -1)], np.int64),
            "residual": np.array([r["residual"]], np.float64), "x_sha256": x_digest(r["x"]), "x_head": np.array(r["x"][:X_HEAD])}


# ---- fixtures and comparisons -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref():
    """The compiled reference where oracle/_ref was built, else None (the pins stand in for it)."""
    return po.Oracle("reference") if po.have_ref() else None


@pytest.fixture(scope="module")
def pins():
    return np.load(PINS)


def pinned(pins, key):
    meta = pins[f"{key}/meta"]
    return {"ret": int(meta[0]), "iters": int(meta[1]), "seed_before": int(meta[2]),
            "residual": float(pins[f"{key}/residual"][0]), "x_sha256": pins[f"{key}/x_sha256"], "x_head": pins[f"{key}/x_head"]}


def assert_same(a, c, *tag):
    assert (a["ret"], a["iters"], a["residual"]) == (c["ret"], c["iters"], c["residual"]), tag
    if "x_sha256" in a:         # a pin: the restatement's x must hash to the reference's, byte for byte
        assert np.array_equal(c["x"][:X_HEAD], a["x_head"]) and np.array_equal(x_digest(c["x"]), a["x_sha256"]), \
            (tag, "x differs from the reference's", c["x"][:X_HEAD], a["x_head"])
    else:
        assert np.array_equal(a["x"], c["x"]), tag


def live_seeded(ref, sid, rp, ci, v, b, para):
    """A live complex solve of the reference whose shadow-residual draw fell inside one clock second (seed known)."""
    for _ in range(5):
        a = ref.csolve(sid, rp, ci, v, b, para=para)
        if a.get("seed_before") == a.get("seed_after"):
            break
    return a


# ---- the checks ---------------------------------------------------------------------------------------------------------------
def test_struct_sizes(ref, pins):
    """64-byte lcg_para, 24-byte clcg_para."""
    assert tuple(pins["sizes"]) == (ctypes.sizeof(po.Para), ctypes.sizeof(po.CPara)) == (64, 24)
    if ref is not None:
        assert ref.lib.ref_sizeof_lcg_para() == ctypes.sizeof(po.Para) == 64
        assert ref.lib.ref_sizeof_clcg_para() == ctypes.sizeof(po.CPara) == 24


@pytest.mark.parametrize("sid,jac", RHS_SIDS)
@pytest.mark.parametrize("eps,ad", RHS_TOLS)
def test_real_bit_exact_random_rhs(ref, pins, port, case10k, sid, jac, eps, ad):
    n, rp, ci, v, _, _ = case10k
    b, m0 = rhs_inputs(n, sid)
    para = rhs_para(eps, ad)
    c = port.solve(sid, rp, ci, v, b, m0=m0, para=para, jacobi=bool(jac))
    assert_same(pinned(pins, rhs_key(sid, eps, ad)), c, "pinned")
    if ref is not None:
        assert_same(ref.solve(sid, rp, ci, v, b, m0=m0, para=para, jacobi=bool(jac)), c, "live")


@pytest.mark.parametrize("sid", SEED_REPLAY_SIDS)
def test_complex_bit_exact_seed_replay(ref, pins, port, case1kc, sid):
    n, rp, ci, v, b, _ = case1kc
    para = seed_replay_para()
    p = pinned(pins, cplx_key("seed_replay", sid))
    assert_same(p, port.csolve(sid, rp, ci, v, b, para=para, rbar0=port.vecrnd(n, p["seed_before"])), "pinned")
    if ref is not None:
        a = live_seeded(ref, sid, rp, ci, v, b, para)
        assert_same(a, port.csolve(sid, rp, ci, v, b, para=para, rbar0=port.vecrnd(n, a["seed_before"])), "live")


def test_dot_and_coo_matvec(ref, pins, port):
    a, b = dot_inputs()
    assert float(pins["dot"][0]) == port.dot(a, b)
    if ref is not None:
        assert ref.dot(a, b) == port.dot(a, b)


@pytest.mark.parametrize("tag,n,band,sym,pattern,sids", GEN_SYSTEMS)
def test_real_bit_exact_on_generated_systems(ref, pins, port, tag, n, band, sym, pattern, sids):
    """The pin on MORE than the one bundled matrix: systems of the synthetic family (BASELINE configs 2-5 in small) with a random
    right-hand side and a random initial guess -- return code, count, residual and every component of x of the restatement equal
    those of the compiled liblcg, at a loose and at a tight tolerance."""
    rp, ci, v, b, m0 = gen_inputs(port, tag, n, band, sym, pattern)
    for sid in sids:
        for eps, ad in GEN_TOLS:
            para = gen_para(eps, ad)
            c = port.solve(sid, rp, ci, v, b, m0=m0, para=para, jacobi=(sid == 1))
            assert_same(pinned(pins, gen_key(tag, sid, eps)), c, "pinned", tag, sid, eps)
            if ref is not None:
                assert_same(ref.solve(sid, rp, ci, v, b, m0=m0, para=para, jacobi=(sid == 1)), c, "live", tag, sid, eps)


@pytest.mark.parametrize("sid", OTHER_TWO_SIDS)
def test_complex_bit_exact_the_other_two(ref, pins, port, case1kc, sid):
    """clbicg (adjoint product, no shadow residual) and clbicgstab (which does not converge on the bundled systems: both sides stop at
    the same cap with the same numbers), beside the three of test_complex_bit_exact_seed_replay."""
    n, rp, ci, v, b, _ = case1kc
    para = other_two_para()

    def port_run(seed):
        if sid == po.CLCG_BICG:
            return port.csolve(sid, rp, ci, v, b, para=para)
        return port.csolve(sid, rp, ci, v, b, para=para, rbar0=port.vecrnd(n, seed))

    p = pinned(pins, cplx_key("other_two", sid))
    assert_same(p, port_run(p["seed_before"]), "pinned")
    if ref is not None:
        a = live_seeded(ref, sid, rp, ci, v, b, para)
        assert_same(a, port_run(a.get("seed_before")), "live")
