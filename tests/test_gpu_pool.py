"""-m gpu: the work-vector pool (pool.hpp: Pool) and the placement's state (pool.hpp: PlaceState, placement.hip) as the solvers
see them, at sizes where nothing but the bookkeeping is at stake: which pool vector a solve receives, what is evicted, what an arena
adds, and when the placement's memory answers and when it has been told to forget.  Sizes follow from the code: Workspace::get
allocates exactly 8 * n bytes per real vector, classic CG holds 3 of them and BiCGStab 6.  Iterates are compared by SHA-256."""
import ctypes as C
import hashlib

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 8192
CAP = 4


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    return _lib.load()


def _system(api, n, seed=3):
    A = api.CsrMatrix.generate(n, 6, 300, True, seed, 0.01, pattern=api.GEN_DIAGONALS)
    xt = torch.empty(n, dtype=torch.float64, device="cuda"); api.gen_xtrue(n, seed, 0, n, xt)
    b = torch.empty_like(xt); A.spmv(xt, b); api.synchronize()
    return A, b


@pytest.fixture(scope="module")
def systems(api):
    """n / 2, n and 2 n rows: made once, left unchanged"""
    s = {n: _system(api, n) for n in (N // 2, N, 2 * N)}
    yield s
    for A, _ in s.values():
        A.destroy()


@pytest.fixture()
def classic(api, lib):
    """classic CG, placement off, an empty pool -- and everything back as it was afterwards"""
    api.set_cg_schedule(1)
    assert lib.lcg_hip_set_placement(0) == 0 and lib.lcg_hip_trim() == 0
    assert _pool(lib) == (0, 0, 0)
    yield
    lib.lcg_hip_set_placement(-1)
    api.set_cg_schedule(0)
    lib.lcg_hip_trim()


def _pool(lib):
    v, b, a = C.c_int(-1), C.c_int64(-1), C.c_int(-1)
    assert lib.lcg_hip_pool_info(C.byref(v), C.byref(b), C.byref(a)) == 0
    return v.value, b.value, a.value


def _last(lib):
    t, mv = C.c_int(-1), C.c_int(-1)
    assert lib.lcg_hip_last_placement(C.byref(t), C.byref(mv), None, None) == 0
    return t.value, mv.value


def _walk(lib):
    ch, ms, held, found, why = C.c_int(-1), C.c_double(-1.0), C.c_int64(-1), C.c_int(-1), C.c_char_p()
    made = lib.lcg_hip_last_placement_walk(C.byref(ch), C.byref(ms), C.byref(held), C.byref(found), C.byref(why))
    return made, ch.value, ms.value, held.value, found.value, (why.value or b"").decode()


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _solve(api, system, n, solver=None, ws=()):
    A, b = system
    para = api.lcg_default_parameters(epsilon=1e-20, abs_diff=1, max_iterations=CAP)
    m = torch.zeros(n, dtype=torch.float64, device="cuda")
    if ws:
        info = api.lcg("lcg_hip_csr_ax", None, m, b, n, para, A, *ws)
    else:
        info = api.lcg_solver("lcg_hip_csr_ax", None, m, b, n, para, A, api.LCG_CG if solver is None else solver)
    assert info.iterations == CAP
    return _sha(m)


def test_pool_reuse_and_eviction(api, lib, systems, classic):
    n = N
    ref = _solve(api, systems[n], n)
    assert _pool(lib) == (3, 24 * n, 0)                 # g, d, A.d: 8 n bytes each
    # a smaller solve takes the vectors that are there (best fit: any of them)
    half = _solve(api, systems[n // 2], n // 2)
    assert _pool(lib) == (3, 24 * n, 0)
    # a larger one finds nothing that fits: every request gives one idle vector back and allocates
    _solve(api, systems[2 * n], 2 * n)
    assert _pool(lib) == (3, 48 * n, 0)
    # BiCGStab holds six
    _solve(api, systems[2 * n], 2 * n, api.LCG_BICGSTAB)
    assert _pool(lib) == (6, 96 * n, 0)
    # the bits do not depend on which vectors a solve was handed
    assert _solve(api, systems[n], n) == ref and _solve(api, systems[n // 2], n // 2) == half
    assert _pool(lib) == (6, 96 * n, 0)
    assert lib.lcg_hip_trim() == 0 and _pool(lib) == (0, 0, 0)


def test_arena_beside_own_vectors(api, lib, systems, classic):
    n = N
    ref = _solve(api, systems[n], n)
    assert lib.lcg_hip_trim() == 0 and _pool(lib) == (0, 0, 0)
    assert lib.lcg_hip_pool_add_arena_for_test(8 * n, 2) == 0
    assert _pool(lib) == (2, 16 * n, 2)
    # two of CG's vectors are slots of the arena, the third is allocated beside it
    assert _solve(api, systems[n], n) == ref
    assert _pool(lib) == (3, 24 * n, 2)
    # 2 n rows fit no slot: the arena stays (its slots are never evicted one by one), the first request gives the own vector back,
    # and three vectors of 16 n bytes are allocated
    _solve(api, systems[2 * n], 2 * n)
    assert _pool(lib) == (5, 16 * n + 48 * n, 2)
    assert lib.lcg_hip_trim() == 0 and _pool(lib) == (0, 0, 0)


def test_forced_placement_remembers_and_forgets(api, lib, systems, classic):
    """Mode 1 at 8192 rows (placement.hip: wanted needs 4096): every candidate is timed, nothing is walked (the stream is far below
    PlaceState::Tune::stream_min), the bits are those of mode 0; the memo answers the second solve and is emptied by lcg_hip_trim, by
    lcg_hip_csr_set_ranges (csr.hip -> csr_choice.hip: ranges_free, "another kernel family may stream another copy of the matrix")
    and by lcg_hip_csr_destroy."""
    n = N
    ref = _solve(api, systems[n], n)
    assert _last(lib) == (0, 0)
    walk0 = _walk(lib)
    assert lib.lcg_hip_set_placement(1) == 0 and lib.lcg_hip_trim() == 0
    assert _solve(api, systems[n], n) == ref and _last(lib)[0] >= 3         # g, d, A.d at least
    assert _solve(api, systems[n], n) == ref and _last(lib)[0] == 0         # the same vectors against the same matrix: from memory
    assert lib.lcg_hip_trim() == 0
    assert _solve(api, systems[n], n) == ref and _last(lib)[0] >= 3
    assert _solve(api, systems[n], n) == ref and _last(lib)[0] == 0
    assert lib.lcg_hip_csr_set_ranges(systems[n][0].h, -1) == 0             # (-1: the mode the matrix has anyway)
    assert _solve(api, systems[n], n) == ref and _last(lib)[0] >= 3
    assert _solve(api, systems[n], n) == ref and _last(lib)[0] == 0
    # a matrix of its own, destroyed and made again (the same seed: the same system)
    own = _system(api, n)
    try:
        assert _solve(api, own, n) == ref and _last(lib)[0] >= 3
        assert _solve(api, own, n) == ref and _last(lib)[0] == 0
        own[0].destroy()
        own = _system(api, n)
        assert _solve(api, own, n) == ref and _last(lib)[0] >= 3
    finally:
        own[0].destroy()
    assert _walk(lib) == walk0                                               # no walk below stream_min


def test_callers_vectors_are_left_alone(api, lib, systems, classic):
    n = N
    ref = _solve(api, systems[n], n)
    assert lib.lcg_hip_set_placement(1) == 0
    before = _pool(lib)
    ws = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3)]
    assert _solve(api, systems[n], n, ws=ws) == ref
    assert _last(lib) == (0, 0) and _pool(lib) == before
