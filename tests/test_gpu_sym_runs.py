"""-m gpu: symmetric run stretches (csr_sym.hip; lcg_hip_csr_set_sym_runs).  A run stretch with an antisymmetric offset table whose
values mirror each other bit for bit multiplies the blocks of its sliced range from a half store, a lower entry read as its partner
row's upper entry.  Nothing of the result may change by a bit: every product here is compared, as 64-bit integers, with the same
handle's product with the mode off, and that product is held to exact row sums (exact_ref).  Forced mode throughout: the automatic
mode looks only at products of >= 512 MB (tests/test_gpu_sym_mixed.py runs it, and the stretch inside mixed matrices, with the
systems and helpers of this file)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import exact_ref as X

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SLICES = {1: "one slice", 2: "two slices", 4: "four slices", 8: "eight slices"}
P1_64, P1_37 = [64], [37]                                      # one pair: a multiple of 64 (one partner tile) / an offset < 64 (the same or the neighbouring block)
P7 = [1, 5, 63, 64, 100, 128, 190]
P16 = [1, 2, 3, 7, 20, 33, 63, 64, 65, 96, 127, 128, 129, 160, 192, 200]


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    return _lib.load()


def plan(n, offs, nx):
    """What the library must find in a constant-diagonal system of n rows: the stretch [b0, b1) of full run blocks, the apron Q, the
    first block of the sliced range (the next multiple of 8 behind b0 + Q) and the blocks per slice."""
    m = max(offs)
    b0, b1 = -(-m // 64), (n - m) // 64
    Q = -(-m // 64) + 1
    inner0 = -(-(b0 + Q) // 8) * 8
    return b0, b1, Q, inner0, (b1 - inner0) // nx


def rows_for(offs, S, tail=37):
    """n so that eight slices get S blocks each (and one slice 8 S + 2), two blocks stay behind them and the last block is partial."""
    m = max(offs)
    inner0 = plan(10 ** 6, offs, 8)[3]
    n = 64 * (inner0 + 8 * S + 2) + m + tail
    assert plan(n, offs, 8)[4] == S and n % 64 != 0
    return n


def system(n, offs, rng, upper=None):
    """CSR of the matrix with diagonals 0, +-offs (clipped at the edges): A[i, i + o] = A[i + o, i], the diagonal dominant (SPD).
    upper: the offsets above the diagonal when they differ from those below it (then no symmetric pattern)."""
    lo = np.sort(np.asarray(offs))
    up = lo if upper is None else np.sort(np.asarray(upper))
    D = np.concatenate([-lo[::-1], [0], up])
    p = len(lo)
    cols = np.arange(n)[:, None] + D[None, :]
    ok = (cols >= 0) & (cols < n)
    vals = np.zeros(cols.shape)
    for t in range(len(up)):
        v = rng.standard_normal(n)
        vals[:, p + 1 + t] = v                          # A[i, i + o] = v[i]
        if upper is None:
            vals[:, p - 1 - t] = np.roll(v, up[t])      # A[i, i - o] = v[i - o]
    if upper is not None:
        vals[:, :p] = rng.standard_normal((n, p))
    vals[:, p] = 1.0 + (np.abs(vals) * ok).sum(1)
    rp = np.concatenate([[0], np.cumsum(ok.sum(1))]).astype(np.int32)
    return rp, cols[ok].astype(np.int32), vals[ok]


def bits_equal(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def kernel(lib, A):
    return lib.lcg_hip_csr_last_kernel(A.h).decode()


def on_off(api, lib, A, n, x, nx, forced_kernel=True):
    """y with the mode forced and off, the kernel names, and what the plan took while on."""
    xd = torch.from_numpy(x).cuda()
    ys = [torch.full((n,), 5.0 + i, dtype=torch.float64, device="cuda") for i in range(2)]
    if forced_kernel:
        A.set_kernel(-64)
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    A.set_sym_runs(1, nx)
    A.spmv(xd, ys[0]); api.synchronize()
    k_on, took = kernel(lib, A), A.sym_runs()
    model_on = lib.lcg_hip_csr_last_traffic_model(A.h)
    extra_on = C.c_int64(0); assert lib.lcg_hip_csr_plan_info(A.h, None, C.byref(extra_on)) == 0
    A.set_sym_runs(0, nx)
    A.spmv(xd, ys[1]); api.synchronize()
    k_off = kernel(lib, A)
    model_off = lib.lcg_hip_csr_last_traffic_model(A.h)
    extra_off = C.c_int64(0); assert lib.lcg_hip_csr_plan_info(A.h, None, C.byref(extra_off)) == 0
    assert A.sym_runs()[0] == 0 and "k_spmv_ldsp_sym" not in k_off and k_off.startswith("k_spmv_ldsp"), k_off
    return ys, k_on, took, (model_on, model_off), (extra_on.value, extra_off.value)


@pytest.mark.parametrize("nx", [1, 2, 4, 8])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name,offs", [("1 pair, 64", P1_64), ("1 pair, 37", P1_37), ("7 pairs", P7), ("16 pairs", P16)])
def test_products(api, lib, name, offs, S, nx):
    """L = 3, 15, 33; offsets that are multiples of 64 and not, below 64, across slice fronts (every partner at S = 1) and into the
    apron; one, two, four and eight slices; n no multiple of 64 and a head that is no multiple of 8 blocks."""
    rng = np.random.default_rng(900 + 10 * len(offs) + S)
    n = rows_for(offs, S)
    rp, col, val = system(n, offs, rng)
    x = rng.standard_normal(n)
    b0, b1, Q, inner0, Sx = plan(n, offs, nx)
    assert (b0 + Q) % 8 != 0 and Sx >= 1
    A = api.CsrMatrix.from_csr(rp, col, val)
    ys, k_on, took, (model_on, model_off), (extra_on, extra_off) = on_off(api, lib, A, n, x, nx)
    print(f"{name}, S {S}, NX {nx}: n {n}, stretch [{b0}, {b1}), apron {Q}, sliced from {inner0}; {took}; {k_on}")
    assert took == (nx, nx * Sx, "taken"), (took, nx, Sx)
    assert k_on.startswith("k_spmv_ldsp (") and "k_spmv_ldsp_sym" in k_on and SLICES[nx] in k_on, k_on
    p = len(offs)
    # one tile per apron and sliced block (and, where the plan without the mode is built without them, the stretches' tables: < 1 KB)
    assert 0 <= extra_on - extra_off - 512 * (p + 1) * (Q + nx * Sx) < 1024, (extra_on, extra_off)
    # (what enters the L2s: the partner reads are counted, so only the per-block plan of the sliced blocks goes -- 64 row pointers, two words)
    assert (4 * 64 + 8) * nx * Sx - 16 * 12 <= model_off - model_on < 512 * nx * Sx, (model_on, model_off)      # (one table of 12 slots per wavefront comes back)
    assert bits_equal(ys[0], ys[1]), (name, S, nx)
    X.assert_rows(ys[1].cpu().numpy(), rp, col, val, x, (name, S, nx))
    A.destroy()


def _refused(api, lib, rp, col, val, x, n, why, nan=False):
    A = api.CsrMatrix.from_csr(rp, col, val)
    ys, k_on, took, models, extras = on_off(api, lib, A, n, x, 8)
    print(f"refusal: {took}; {k_on}")
    assert took[0] == 0 and took[1] == 0 and took[2].startswith("refused") and why in took[2], took
    assert k_on.startswith("k_spmv_ldsp") and "k_spmv_ldsp_sym" not in k_on, k_on
    assert models[0] == models[1] and abs(extras[0] - extras[1]) < 1024, (models, extras)      # (no half store; the stretches' tables at most)
    assert bits_equal(ys[0], ys[1])
    if not nan:
        X.assert_rows(ys[1].cpu().numpy(), rp, col, val, x, (why,))
    A.destroy()


@pytest.mark.parametrize("what", ["one ulp", "minus zero", "nan payload"])
def test_refused_values(api, lib, what):
    """One lower entry of one row of the sliced range against its partner's upper entry: one ulp apart, -0.0 against +0.0, two NaNs
    with different payloads.  The stretch is refused and the old kernel answers with the same bits."""
    rng = np.random.default_rng(930)
    offs = P7
    n = rows_for(offs, 1)
    rp, col, val = system(n, offs, rng)
    b0, b1, Q, inner0, S = plan(n, offs, 8)
    i, k, p = 64 * (inner0 + 5) + 17, 2, len(offs)          # row i, lower slot k: the partner is row i - offs[p - 1 - k], its slot 2p - k
    ip = i - sorted(offs)[p - 1 - k]
    lo, up = int(rp[i]) + k, int(rp[ip]) + 2 * p - k
    assert col[lo] == ip and col[up] == i and val[lo] == val[up]
    bitsv = val.view(np.uint64)
    if what == "one ulp":
        bitsv[lo] += 1
    elif what == "minus zero":
        val[lo], val[up] = -0.0, 0.0
    else:
        bitsv[lo], bitsv[up] = 0x7FF8000000000001, 0x7FF8000000000002
    assert bitsv[lo] != bitsv[up]
    _refused(api, lib, rp, col, val, rng.standard_normal(n), n, "bit for bit", nan=what == "nan payload")


def test_refused_offsets(api, lib):
    """Three entries per row with the diagonal in the middle, but offsets -70 and +50: not antisymmetric."""
    rng = np.random.default_rng(940)
    n = rows_for([70], 1)
    rp, col, val = system(n, [70], rng, upper=[50])
    _refused(api, lib, rp, col, val, rng.standard_normal(n), n, "antisymmetric")


def test_refused_handles(api, lib):
    """A complex128, a complex64 and a sharded handle keep their paths whatever the mode says."""
    rng = np.random.default_rng(950)
    offs = P7
    n = rows_for(offs, 1)
    rp, col, val = system(n, offs, rng)
    x = rng.standard_normal(n)
    # complex128
    Ac = api.CsrMatrix.from_csr(rp, col, val.astype(np.complex128))
    Ac.set_kernel(-64)
    assert lib.lcg_hip_csr_set_sym_runs(Ac.h, 1) == 0
    xc = torch.from_numpy(x.astype(np.complex128)).cuda(); yc = torch.empty_like(xc)
    Ac.spmv(xc, yc); api.synchronize()
    assert "k_spmv_ldsp_sym" not in kernel(lib, Ac) and Ac.sym_runs()[0] == 0, kernel(lib, Ac)
    X.assert_rows(yc.cpu().numpy(), rp, col, val.astype(np.complex128), x.astype(np.complex128), ("complex128",))
    Ac.destroy()
    # complex64: the switch itself refuses the handle
    A32 = api.CsrMatrix.from_csr_c64(rp, col, val.astype(np.complex64))
    assert lib.lcg_hip_csr_set_sym_runs(A32.h, 1) != 0 and lib.lcg_hip_csr_set_sym_slices(A32.h, 8) != 0
    x32 = torch.from_numpy(x.astype(np.complex64)).cuda(); y32 = torch.empty_like(x32)
    A32.spmv_c64(x32, y32); api.synchronize()
    assert torch.isfinite(torch.view_as_real(y32)).all()
    A32.destroy()
    # sharded (one rank: the all-gather is a copy)
    A = api.CsrMatrix.from_csr(rp, col, val)
    ys, k_on, took, *_ = on_off(api, lib, A, n, x, 8)
    assert took == (8, 8, "taken")
    A.distribute(n, 0)
    xd = torch.from_numpy(x).cuda()
    out = []
    for mode in (1, 0):
        assert lib.lcg_hip_csr_set_sym_runs(A.h, mode) == 0
        y = torch.empty_like(xd)
        A.spmv(xd, y); api.synchronize()
        assert "k_spmv_ldsp_sym" not in kernel(lib, A) and A.sym_runs()[0] == 0, kernel(lib, A)
        out.append(y)
    assert bits_equal(out[0], out[1])
    X.assert_rows(out[0].cpu().numpy(), rp, col, val, x, ("sharded",))
    A.destroy()


@pytest.fixture(scope="module")
def solve_system(api, lib):
    """16 pairs (33 entries per row: the automatic choice takes blocks of 64 rows, and the loops the product that carries the dot)."""
    rng = np.random.default_rng(960)
    n = rows_for(P16, 3)
    rp, col, val = system(n, P16, rng)
    A = api.CsrMatrix.from_csr(rp, col, val)
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    yield A, n, rp, col, val, rng
    A.destroy()


@pytest.mark.parametrize("nx", [1, 8])
def test_carried_dot(api, lib, solve_system, nx):
    """lcg_hip_spmv_dot: y, y.u and y.y with u = x (taken from the gather of the diagonal's slot) and another u, the bits of the mode off."""
    A, n, rp, col, val, rng = solve_system
    x = torch.from_numpy(rng.standard_normal(n)).cuda()
    u = torch.from_numpy(rng.standard_normal(n)).cuda()
    A.set_kernel(0)
    out = {}
    for mode in (1, 0):
        A.set_sym_runs(mode, nx)
        for uname, uu in (("u=x", x), ("u", u)):
            y = torch.empty(n, dtype=torch.float64, device="cuda")
            res = (C.c_double * 2)()
            assert lib.lcg_hip_spmv_dot(A.h, x.data_ptr(), y.data_ptr(), uu.data_ptr(), res) == 0
            k = kernel(lib, A)
            assert "carrying the dot" in k and k.startswith("k_spmv_ldsp (") and ("k_spmv_ldsp_sym" in k) == bool(mode), k
            out[mode, uname] = (y, res[0], res[1])
    for uname in ("u=x", "u"):
        a, b = out[1, uname], out[0, uname]
        assert bits_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], (uname, a[1:], b[1:])
    X.assert_rows(out[0, "u"][0].cpu().numpy(), rp, col, val, x.cpu().numpy(), ("carried dot",))


def _solve(api, lib, A, n, b, eps, cap, mode, nx=8):
    A.set_kernel(0)
    A.set_sym_runs(mode, nx)
    m = torch.zeros(n, dtype=torch.float64, device="cuda")
    info = api.lcg("lcg_hip_csr_ax", None, m, b, n, api.lcg_default_parameters(epsilon=eps, abs_diff=1, max_iterations=cap), A)
    k = kernel(lib, A)
    assert "carrying the dot" in k and k.startswith("k_spmv_ldsp (") and ("k_spmv_ldsp_sym" in k) == bool(mode), k
    api.synchronize()
    return hashlib.sha256(m.cpu().numpy().tobytes()).hexdigest(), (info.ret, info.iterations, info.residual)


def test_solves(api, lib, solve_system):
    """CG capped at 30 iterations, CG stopped by epsilon in the middle, and one solve on a caller's stream: the SHA-256 of the
    iterate and the solver's answer are those of the mode off."""
    A, n, rp, col, val, rng = solve_system
    b = torch.from_numpy(rng.standard_normal(n)).cuda()
    off = _solve(api, lib, A, n, b, 1e-300, 30, 0)
    assert off[1][1] == 30, off
    for nx in (1, 2, 4, 8):
        assert _solve(api, lib, A, n, b, 1e-300, 30, 1, nx) == off, nx
    off = _solve(api, lib, A, n, b, 1e-12, 200, 0)
    assert 3 < off[1][1] < 200, off                     # stopped by epsilon, in the middle
    on = _solve(api, lib, A, n, b, 1e-12, 200, 1)
    assert on == off, (on, off)
    S = torch.cuda.Stream()
    try:
        with torch.cuda.stream(S):
            b2 = b.clone()
            api.use_torch_stream()
            mine = _solve(api, lib, A, n, b2, 1e-12, 200, 1)
            S.synchronize()
    finally:
        api.use_own_stream()
    assert mine == off, (mine, off)


def test_switching_between_products(api, lib):
    """set_sym_runs between products on one handle: the half store is freed and built again, y keeps its bits."""
    rng = np.random.default_rng(970)
    offs = P7
    n = rows_for(offs, 1)
    rp, col, val = system(n, offs, rng)
    A = api.CsrMatrix.from_csr(rp, col, val)
    A.set_kernel(-64)
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    x = torch.from_numpy(rng.standard_normal(n)).cuda()
    first = None
    for mode, nx in ((0, 0), (1, 8), (1, 8), (0, 0), (1, 1), (-1, 0), (1, 0), (1, 4), (0, 8)):
        A.set_sym_runs(mode, nx)
        y = torch.full((n,), 3.0, dtype=torch.float64, device="cuda")
        A.spmv(x, y); api.synchronize()
        took, k = A.sym_runs(), kernel(lib, A)
        want = 0 if mode != 1 else (nx or 1)            # (automatic: a product of a few hundred KB is not looked at)
        assert took[0] == want and k.startswith("k_spmv_ldsp (") and ("k_spmv_ldsp_sym" in k) == bool(want), (mode, nx, took, k)
        extra = C.c_int64(0); assert lib.lcg_hip_csr_plan_info(A.h, None, C.byref(extra)) == 0
        if first is None:
            first, extra0 = y, extra.value
        assert bits_equal(y, first), (mode, nx)
        assert (extra.value - extra0 >= 512 * (len(offs) + 1)) == bool(want), (mode, nx, extra.value, extra0)    # (the stretches' tables stay: < 1 KB)
    for bad in (-2, 2):
        assert lib.lcg_hip_csr_set_sym_runs(A.h, bad) != 0
    assert lib.lcg_hip_csr_set_sym_slices(A.h, 3) != 0
    A.destroy()


def test_generated_constant_diagonals(api, lib):
    """The benchmark's generator (symmetric constant diagonals): its values mirror each other bit for bit, so its interior is taken."""
    n = 64 * 40 + 11
    A = api.CsrMatrix.generate(n, 16, 200, True, 3, 0.01, pattern=api.GEN_DIAGONALS)
    rp, col, val = A.arrays_to_host()
    x = np.random.default_rng(980).standard_normal(n)
    ys, k_on, took, *_ = on_off(api, lib, A, n, x, 8)
    print(f"generated: {took}; {k_on}")
    assert took[0] == 8 and took[1] >= 8 and took[2] == "taken" and "k_spmv_ldsp_sym" in k_on, (took, k_on)
    assert bits_equal(ys[0], ys[1])
    X.assert_rows(ys[1].cpu().numpy(), rp, col, val, x, ("generated",))
    A.destroy()


def test_fresh_handle_solved_with_placement(api, lib):
    """A handle whose FIRST product is the solver's own -- made by the placement of the work vectors (lcg_hip_set_placement(1): forced,
    the system is far below its automatic size; n >= 4096), not by spmv or spmv_dot -- takes the symmetric stretch all the same: the
    plan that first product builds holds the half store, the loop's products run from it, and iterate and answer are those of a fresh
    handle with the mode off."""
    rng = np.random.default_rng(990)
    n = rows_for(P16, 6)
    assert n >= 4096
    rp, col, val = system(n, P16, rng)
    b = torch.from_numpy(rng.standard_normal(n)).cuda()
    got = {}
    try:
        assert lib.lcg_hip_set_placement(1) == 0
        for mode in (1, 0):
            A = api.CsrMatrix.from_csr(rp, col, val)
            assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
            A.set_sym_runs(mode)
            assert kernel(lib, A) == ""                     # nothing multiplied yet
            got[mode] = _solve(api, lib, A, n, b, 1e-300, 12, mode, 0)      # (asserts the kernel's name)
            took = A.sym_runs()
            assert (took[0], took[2]) == ((1, "taken") if mode else (0, "not tried")), (mode, took)
            A.destroy()
    finally:
        lib.lcg_hip_set_placement(-1)
    assert got[1] == got[0] and got[0][1][1] == 12, got


def test_rewritten_values_of_an_adopted_matrix(api, lib):
    """The half store is a copy of values.  The rewrite protocol of include/lcg_hip.h -- new values in the adopted arrays, then ANY one
    of set_packed / set_tiled / set_binned / set_ranges (A, 0) and (A, -1) -- drops it with the op(A) copies: the next product follows
    the new values, from a new half store where they mirror each other again and from the old kernel where they do not."""
    rng = np.random.default_rng(995)
    offs = P7
    n = rows_for(offs, 1)
    rp, col, val = system(n, offs, rng)
    pad = 32
    colb = torch.zeros(len(col) + pad, dtype=torch.int32, device="cuda"); colb[:len(col)] = torch.from_numpy(col).cuda()
    valb = torch.zeros(len(val) + pad, dtype=torch.float64, device="cuda"); valb[:len(val)] = torch.from_numpy(val).cuda()
    A = api.CsrMatrix.from_csr(torch.from_numpy(rp).cuda(), colb[:len(col)], valb[:len(val)], adopt=2)
    A.set_kernel(-64)
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    A.set_sym_runs(1, 8)
    x = rng.standard_normal(n)
    xd = torch.from_numpy(x).cuda()

    def product(v, want):
        y = torch.full((n,), 9.0, dtype=torch.float64, device="cuda")
        A.spmv(xd, y); api.synchronize()
        assert (A.sym_runs()[0], "k_spmv_ldsp_sym" in kernel(lib, A)) == (want, bool(want)), (A.sym_runs(), kernel(lib, A))
        X.assert_rows(y.cpu().numpy(), rp, col, v, x, ("rewritten", want))
        return y

    product(val, 8)
    setters = (lib.lcg_hip_csr_set_binned, lib.lcg_hip_csr_set_tiled, lib.lcg_hip_csr_set_ranges, lib.lcg_hip_csr_set_packed)
    for step, setter in enumerate(setters):
        if step % 2 == 0:       # other symmetric values / values that do not mirror each other
            _, _, v2 = system(n, offs, np.random.default_rng(996 + step))
        else:
            v2 = np.random.default_rng(996 + step).standard_normal(len(val))
        valb[:len(val)].copy_(torch.from_numpy(v2).cuda()); torch.cuda.synchronize()
        assert setter(A.h, 0) == 0 and setter(A.h, -1) == 0
        if setter is lib.lcg_hip_csr_set_packed:
            assert setter(A.h, 1) == 0              # (a system this small takes the packed form only when forced)
        product(v2, 8 if step % 2 == 0 else 0)
    A.destroy()


def test_refused_unsorted_rows(api, lib):
    """CSR rows may be stored in any order and a run block does not care.  A symmetric band stored in mirror order -- west, south,
    centre, north, east: offsets -1, -500, 0, 500, 1 -- has an antisymmetric table with the diagonal in the middle, but its last offset
    is not its largest, which the apron is sized from: such a stretch is refused, and the old kernel answers with the same bits."""
    rng = np.random.default_rng(985)
    offs = [1, 500]
    n = rows_for(offs, 1)
    rp, col, val = system(n, offs, rng)
    full = np.flatnonzero(np.diff(rp) == 5)
    at = rp[full].astype(np.int64)[:, None] + np.array([1, 0, 2, 4, 3])[None, :]       # sorted -500, -1, 0, 1, 500 -> mirror order
    col[rp[full].astype(np.int64)[:, None] + np.arange(5)[None, :]] = col[at]
    val[rp[full].astype(np.int64)[:, None] + np.arange(5)[None, :]] = val[at]
    i = int(full[len(full) // 2])
    assert (col[rp[i]:rp[i] + 5] - i).tolist() == [-1, -500, 0, 500, 1]
    _refused(api, lib, rp, col, val, rng.standard_normal(n), n, "ascending")
