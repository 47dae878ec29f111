"""-m gpu: symmetric run stretches (csr_sym.hip) inside mixed matrices and at their limits.  tests/test_gpu_sym_runs.py and
tests/test_gpu_sym_groups.py run one kind of matrix, a pure constant-diagonal system with the stretches' switch off and the mode
forced; here the stretch lies between irregular rows, is not the longest, meets the run stretches' own switch, the limits on its
row length, offsets of thousands of rows and the automatic mode.  The matrices and what the library must find in them come from
tests/sym_cases.py (expected_plan reads the CSR arrays alone; tests/test_sym_cases_cpu.py holds it to the closed forms).

Every product is compared as 64-bit integers with the same handle's product with the mode off, and that product is held to exact
row sums (exact_ref.assert_rows): no tolerance beyond exact_ref's own.  Every case also asserts what CsrMatrix.sym_runs() says, the
kernel string, the bytes the plan gained (one tile of 512 (p + 1) bytes per apron and sliced block) and the traffic model.

The count of consecutive blocks per XCD is the process's (LCG_HIP_SYM_GROUP is read once): everything runs with the default, and
test_one_block_per_xcd runs the one-slice cases of test_irregular_head_and_tail and test_wide_offsets once more in ONE child with a
count of 1 -- this file as a program -- and compares hashes."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import exact_ref as X
import sym_cases as SC
import test_gpu_sym_groups as GR
import test_gpu_sym_runs as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_asked = os.environ.get("LCG_HIP_SYM_GROUP", "")
G_NOW = int(_asked) if _asked in ("1", "2", "4", "8") else GR.DEFAULT        # consecutive blocks per XCD this process runs with


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    return _lib.load()


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def state(lib, A):
    """What a handle says after a product: kernel, symmetric stretch, run stretches in use, traffic model, the plan's bytes."""
    extra, blocks = C.c_int64(0), C.c_int64(-1)
    assert lib.lcg_hip_csr_plan_info(A.h, None, C.byref(extra)) == 0
    count = lib.lcg_hip_csr_run_stretches(A.h, C.byref(blocks))
    return SimpleNamespace(kernel=R.kernel(lib, A), took=A.sym_runs(), stretches=(count, blocks.value),
                           model=lib.lcg_hip_csr_last_traffic_model(A.h), extra=extra.value)


def check_states(want, on, off, nx, s, tag):
    """The mode on against the mode off, stretches' switch s: what expected_plan (want) says must be taken, and what follows from it."""
    assert off.took[0] == 0 and off.took[1] == 0 and "k_spmv_ldsp_sym" not in off.kernel and off.kernel.startswith("k_spmv_ldsp"), (tag, off)
    assert on.took == want.sym_runs, (tag, on.took, want.sym_runs)
    kept = (len(want.kept), sum(t[1] - t[0] for t in want.kept)) if s else (0, 0)
    assert on.stretches == kept and off.stretches == kept, (tag, on.stretches, off.stretches, kept)    # a symmetric stretch stays a stretch
    c = want.taken
    if c is None:
        assert on.kernel.startswith("k_spmv_ldsp") and "k_spmv_ldsp_sym" not in on.kernel, (tag, on.kernel)
        assert on.model == off.model and abs(on.extra - off.extra) < 1024, (tag, on, off)      # (no half store; the stretches' tables at most)
        return
    p, sb = c.L // 2, nx * c.S
    assert on.kernel.startswith("k_spmv_ldsp (") and "k_spmv_ldsp_sym" in on.kernel and R.SLICES[nx] in on.kernel, (tag, on.kernel)
    assert GR.named(on.kernel, G_NOW) if nx == 1 else "blocks per XCD" not in on.kernel, (tag, on.kernel)
    # one tile per apron and sliced block (and, where the plan without the mode was built without them, the stretches' tables: < 1 KB)
    assert 0 <= on.extra - off.extra - 512 * (p + 1) * (c.Q + sb) < 1024, (tag, on.extra, off.extra)
    if s:       # part_traffic_model: with the stretches in use the sliced range is part of one, taken off with and without the mode
        assert on.model == off.model, (tag, on.model, off.model)
    else:       # else the sliced blocks' plan goes (64 row pointers, two words, the groups of row 0's columns) and one table comes back
        assert off.model - on.model == (4 * 64 + 8 + 16 * ((c.L + 1 + 3) // 4)) * sb - 16 * max(SC.RS_QMIN, (c.L + 3) // 4), (tag, on.model, off.model)


def on_off(api, lib, A, want, xd, nx, s, tag):
    """Two products of a handle whose kernel is forced, the mode on and off, under the stretches' switch s; checked, same bits."""
    n = A.n
    assert lib.lcg_hip_csr_set_run_stretches(A.h, s) == 0
    ys, st = [], []
    for mode in (1, 0):
        A.set_sym_runs(mode, nx)
        y = torch.full((n,), 5.0 + mode, dtype=torch.float64, device="cuda")
        A.spmv(xd, y); api.synchronize()
        ys.append(y); st.append(state(lib, A))
    check_states(want, st[0], st[1], nx, s, tag)
    assert R.bits_equal(ys[0], ys[1]), tag
    return ys


def open_case(api, lib, rp, col, val, x, nx, s=0, tag=()):
    """A handle on the matrix with the packed kernel forced, its products with the mode on and off checked against the expected
    plan, each other and (the mode off) exact row sums.  Returns the handle, y (mode off) and the expected plan."""
    want = SC.expected_plan(rp, col, val, nx)
    A = api.CsrMatrix.from_csr(rp, col, val)
    A.set_kernel(-64)
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    xd = torch.from_numpy(x).cuda()
    ys = on_off(api, lib, A, want, xd, nx, s, tag)
    X.assert_rows(ys[1].cpu().numpy(), rp, col, val, x, tag)
    return A, ys[1], want


def geometry(want, n):
    """What the sizes are chosen for: the apron does not end on a multiple of eight blocks, the last block is partial."""
    c = want.taken
    assert c is not None and (c.b0 + c.Q) % 8 != 0 and n % 64 != 0, (want.status, n)
    return c


# ------------------------------------------------------------------------------------------------ 1. both switches
def _both_switches_system(name):
    if name == "mixed":
        rng = np.random.default_rng(2100)
        rp, col, val = SC.block_system(SC.head_tail_regions(R.P16, 1), rng)
    else:
        offs, S = {"7 pairs, S 1": (R.P7, 1), "7 pairs, S 3": (R.P7, 3), "16 pairs, S 1": (R.P16, 1), "16 pairs, S 3": (R.P16, 3)}[name]
        rng = np.random.default_rng(2100 + 10 * len(offs) + S)
        rp, col, val = R.system(R.rows_for(offs, S), offs, rng)
    return rp, col, val, rng.standard_normal(len(rp) - 1)


@pytest.fixture(scope="module")
def both_switches_systems():
    return {name: _both_switches_system(name) for name in ("7 pairs, S 1", "7 pairs, S 3", "16 pairs, S 1", "16 pairs, S 3", "mixed")}


@pytest.mark.parametrize("nx", [1, 2, 4, 8])
@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("name", ["7 pairs, S 1", "7 pairs, S 3", "16 pairs, S 1", "16 pairs, S 3", "mixed"])
def test_both_switches(api, lib, both_switches_systems, name, s, nx):
    """lcg_hip_csr_set_run_stretches and the symmetric mode together: with the stretches on, the apron and the blocks behind the
    sliced range are STRETCH blocks of the launch that leaves the range out, their numbers shifted by the range's length.  Four
    products -- (mode 1, s), (mode 0, s), (mode 1, 1 - s), (mode 0, 1 - s) -- with the same bits; with the stretches on the handle
    still reports the stretch, and the traffic model is that of the mode off (the range is part of a stretch either way)."""
    rp, col, val, x = both_switches_systems[name]
    n = len(rp) - 1
    A, y, want = open_case(api, lib, rp, col, val, x, nx, s, (name, s, nx))
    c = geometry(want, n)
    assert c.S >= 1 and (nx != 8 or c.b1 - (c.inner0 + nx * c.S) == 2)            # eight slices: two blocks of the stretch behind them
    ys = on_off(api, lib, A, want, torch.from_numpy(x).cuda(), nx, 1 - s, (name, 1 - s, nx, "switched"))
    assert R.bits_equal(ys[0], y) and R.bits_equal(ys[1], y), (name, s, nx)
    A.destroy()


# ------------------------------------------------------------------------------------------------ 2. irregular head and tail
def head_tail_system(offs):
    rng = np.random.default_rng(2200 + len(offs))
    regions = SC.head_tail_regions(offs, 1)
    rp, col, val = SC.block_system(regions, rng)
    return rp, col, val, regions, rng


def head_tail_case(api, lib, offs, nx):
    """ragged (5 blocks + 17 rows) | symmetric stretch | ragged (4 blocks + 29 rows): the longest row has 48 entries, so the launch
    around the range gathers 12 per lane while the symmetric kernel runs 6 or 9, and the blocks behind the range -- two of the
    stretch, then rows of every length -- take their numbers, and the carried dot's slots, shifted by the range's length.
    Plain products, the carried dot with u = x and another u, a CG capped at 30 iterations; returns their hashes."""
    rp, col, val, regions, rng = head_tail_system(offs)
    n = len(rp) - 1
    assert int(np.diff(rp).max()) == 48 and 17 < len(col) / n <= 34       # (the automatic choice: blocks of 64 rows)
    x = rng.standard_normal(n)
    tag = ("head and tail", len(offs), nx)
    A, y, want = open_case(api, lib, rp, col, val, x, nx, 0, tag)
    c = geometry(want, n)
    assert c.b0 > SC.HEAD // 64 and c.b1 + 4 <= n // 64 and c.b1 - (c.inner0 + nx * c.S) == (2 if nx == 8 else 0)
    out = {"product": sha(y)}
    xd, u, b = torch.from_numpy(x).cuda(), torch.from_numpy(rng.standard_normal(n)).cuda(), torch.from_numpy(rng.standard_normal(n)).cuda()
    A.set_kernel(0)
    got = {}
    for mode in (1, 0):
        A.set_sym_runs(mode, nx)
        for uname, uu in (("u=x", xd), ("u", u)):
            yd = torch.full((n,), 2.0, dtype=torch.float64, device="cuda")
            res = (C.c_double * 2)()
            assert lib.lcg_hip_spmv_dot(A.h, xd.data_ptr(), yd.data_ptr(), uu.data_ptr(), res) == 0
            k = R.kernel(lib, A)
            assert "carrying the dot" in k and k.startswith("k_spmv_ldsp (") and ("k_spmv_ldsp_sym" in k) == bool(mode), (tag, k)
            assert not mode or (R.SLICES[nx] in k and (nx != 1 or GR.named(k, G_NOW))), (tag, k)
            got[mode, uname] = (yd, res[0], res[1])
        assert A.sym_runs() == (want.sym_runs if mode else (0, 0, "not tried")), (tag, mode, A.sym_runs())
    for uname in ("u=x", "u"):
        a, o = got[1, uname], got[0, uname]
        assert R.bits_equal(a[0], o[0]) and a[1] == o[1] and a[2] == o[2], (tag, uname, a[1:], o[1:])
        assert R.bits_equal(a[0], y), (tag, uname)                       # (the forced kernel's product, held to exact rows above)
        X.assert_dot(a[1], a[0].cpu().numpy(), (xd if uname == "u=x" else u).cpu().numpy(), tag + (uname, "y.u"))
        X.assert_dot(a[2], a[0].cpu().numpy(), a[0].cpu().numpy(), tag + (uname, "y.y"))
        out["dot " + uname] = [sha(a[0]), float(a[1]).hex(), float(a[2]).hex()]
    off = R._solve(api, lib, A, n, b, 1e-300, 30, 0, nx)
    assert off[1][1] == 30 and np.isfinite(off[1][2]), off
    on = R._solve(api, lib, A, n, b, 1e-300, 30, 1, nx)
    assert on == off, (tag, on, off)
    out["solve"] = [on[0], on[1][0], on[1][1], float(on[1][2]).hex()]
    A.destroy()
    return out


# ------------------------------------------------------------------------------------------------ 6. wide offsets
def wide_case(api, lib, nx):
    """Offsets 1, 63, 64, 65, 2047, 2048 and 5000: an apron of 80 blocks, partner tiles up to 79 blocks back.  One slice: an inner
    range of 70 blocks, more than two windows of 8 G blocks at the default G, every far partner in the apron or windows back.
    Eight slices of 3 blocks: every partner but the nearest crosses several slice fronts."""
    offs = SC.WIDE
    rng = np.random.default_rng(2600 + nx)
    n = GR.rows_for_inner(offs, 70) if nx == 1 else R.rows_for(offs, 3)
    rp, col, val = R.system(n, offs, rng)
    x = rng.standard_normal(n)
    A, y, want = open_case(api, lib, rp, col, val, x, nx, 0, ("wide", nx))
    c = geometry(want, n)
    assert c.Q == 80 and (c.nx, c.S) == ((1, 70) if nx == 1 else (8, 3))
    assert nx == 8 or c.S > 2 * 8 * GR.DEFAULT                           # more than two windows at the default count
    A.destroy()
    return {"product": sha(y)}


ONE_SLICE_CASES = {"head and tail, 16 pairs": lambda api, lib: head_tail_case(api, lib, R.P16, 1),
                   "head and tail, 7 pairs": lambda api, lib: head_tail_case(api, lib, R.P7, 1),
                   "wide offsets": lambda api, lib: wide_case(api, lib, 1)}
_done = {}


def one_slice_case(api, lib, key):
    """(once per process: test_one_block_per_xcd compares what the tests of the cases themselves computed)"""
    if key not in _done:
        _done[key] = ONE_SLICE_CASES[key](api, lib)
    return _done[key]


@pytest.mark.parametrize("nx", [1, 8])
@pytest.mark.parametrize("pairs", [16, 7])
def test_irregular_head_and_tail(api, lib, pairs, nx):
    """head_tail_case with 16 and 7 pairs, one slice and eight: dot partials, the iterate's SHA-256 and the solver's answer are those
    of the mode off."""
    if nx == 1:
        out = one_slice_case(api, lib, f"head and tail, {pairs} pairs")
    else:
        out = head_tail_case(api, lib, R.P16 if pairs == 16 else R.P7, nx)
    assert set(out) == {"product", "dot u=x", "dot u", "solve"}


@pytest.mark.parametrize("nx", [1, 8])
def test_wide_offsets(api, lib, nx):
    out = one_slice_case(api, lib, "wide offsets") if nx == 1 else wide_case(api, lib, nx)
    assert set(out) == {"product"}


def test_one_block_per_xcd(api, lib):
    """The one-slice cases of test_irregular_head_and_tail and test_wide_offsets once more in a child with LCG_HIP_SYM_GROUP=1: the
    same cases pass there under that count's kernel string, and the hashes of y, the carried sums, the iterate's SHA-256, the
    count and the residual are those of the default."""
    assert "LCG_HIP_SYM_GROUP" not in os.environ, "the suite runs with the default count"
    mine = {key: one_slice_case(api, lib, key) for key in ONE_SLICE_CASES}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    kid = subprocess.Popen(cmd, env=dict(os.environ, LCG_HIP_SYM_GROUP="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        so, se = kid.communicate(timeout=120)
        assert kid.returncode == 0, (so[-500:], se[-3000:])
        got = json.loads(so.strip().splitlines()[-1])
        assert got["G"] == 1 and got["cases"] == json.loads(json.dumps(mine)), {k: (w, mine.get(k)) for k, w in got["cases"].items() if w != mine.get(k)}
    finally:        # whatever happened, no child stays behind with the GPU open
        if kid.poll() is None:
            kid.kill()
        kid.wait()


# ------------------------------------------------------------------------------------------------ 3. not the longest
@pytest.fixture(scope="module")
def not_longest_systems():
    out = {}
    for key, spec in SC.not_longest_specs(R.P7, R.P16).items():
        rng = np.random.default_rng(2300)
        rp, col, val = SC.block_system(SC.chain_regions(spec), rng)
        out[key] = (rp, col, val, rng.standard_normal(len(rp) - 1))
    return out


@pytest.mark.parametrize("nx", [1, 8])
@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("key", ["3a", "3b", "3c", "3d third", "3d fifth"])
def test_not_the_longest(api, lib, not_longest_systems, key, s, nx):
    """sym_runs_build walks the stretches by length and goes on past a refused one.
    3a  asymmetric values, 40 blocks | symmetric, 20 blocks: the shorter is taken, the status says "taken".
    3b  other offsets above the diagonal than below it, 40 blocks | symmetric, 20 blocks: the same.
    3c  symmetric 16 pairs, 30 blocks | symmetric 7 pairs, 20 blocks: the longest is taken; with the stretches on the other stays
        a plain stretch (two stretches, 50 blocks).
    3d  six regions of 6, 26, 14, 36, 12 and 20 blocks, five of them with values that do not mirror: the symmetric one the third
        longest -- taken after two refusals --, then the fifth longest -- it has no descriptor, so nothing is taken and the
        status is what the longest was refused for.
    What is taken, with how many blocks, and the status are expected_plan's (check_states)."""
    rp, col, val, x = not_longest_systems[key]
    n = len(rp) - 1
    A, y, want = open_case(api, lib, rp, col, val, x, nx, s, (key, s, nx))
    lengths = sorted((t[1] - t[0] for t in want.kept), reverse=True)
    took = A.sym_runs()         # (the mode is off again: nothing)
    assert took[0] == 0 and n % 64 != 0
    if key == "3d fifth":
        assert want.taken is None and len(want.kept) == 4 and want.status.startswith("refused") and lengths == [36, 26, 20, 14]
    else:
        c = want.taken
        assert c is not None and want.status == "taken"
        assert c.b1 - c.b0 == {"3a": 20, "3b": 20, "3c": 30, "3d third": 20}[key] and (key == "3c") == (c is want.cands[0])
        assert key == "3c" or (c.b0 > 40 and c.s0 > 0 and c.b1 - c.b0 < lengths[0])       # b0 and s0 deep inside the matrix
    A.destroy()


# ------------------------------------------------------------------------------------------------ 4. what the check covers
@pytest.fixture(scope="module")
def covered_system():
    rp, col, val, regions, rng = head_tail_system(R.P16)
    plan = SC.expected_plan(rp, col, val, 8)
    assert plan.taken is not None
    return rp, col, val, regions, plan, SC.checked_words(rp, col, plan), rng.standard_normal(len(rp) - 1)


@pytest.mark.parametrize("where", ["apron lower", "apron upper within the apron", "behind the range", "ragged", "all"])
def test_values_the_check_must_not_see(api, lib, covered_system, where):
    """k_sym_check compares the lower entries of the rows of the sliced range with their partners' upper entries, nothing else.
    One ulp on the apron rows' own lower entries, on the apron's upper entries whose partner is an apron row, on every entry of
    the stretch's blocks behind the sliced range, on the ragged regions, and on all of them at once: the stretch is still taken,
    with the same blocks, the bits of the mode off, exact rows."""
    rp, col, val, regions, plan, pairs, x = covered_system
    sets = SC.outside_sets(rp, col, plan, regions)
    at = np.concatenate(list(sets.values())) if where == "all" else sets[where]
    v2 = SC.perturb_outside(val, pairs, at)
    A, y, want = open_case(api, lib, rp, col, v2, x, 8, 0, ("outside", where))
    assert want.sym_runs == plan.sym_runs and want.status == "taken" and vars(want.taken) == vars(plan.taken)
    A.destroy()


@pytest.mark.parametrize("where", ["first checked word", "last checked word", "last apron row's upper entry into the range"])
def test_values_the_check_must_see(api, lib, covered_system, where):
    """One ulp on the FIRST word k_sym_check compares (first row of the range's first block, slot 0), on the LAST (last row of the
    range, slot p - 1), and on the upper entry of the last apron row that points into the range: refused, "bit for bit", and the
    old kernel answers with the same bits."""
    rp, col, val, regions, plan, pairs, x = covered_system
    v2 = SC.perturb_inside(val, pairs, [SC.inside_words(rp, col, plan)[where]])
    A, y, want = open_case(api, lib, rp, col, v2, x, 8, 0, ("inside", where))
    assert want.sym_runs == (0, 0, SC.WHY_VALUES) and "bit for bit" in want.sym_runs[2]
    A.destroy()


# ------------------------------------------------------------------------------------------------ 5. the limits on L
@pytest.mark.parametrize("nx", [1, 8])
@pytest.mark.parametrize("p", [0, 11, 12, 17])
def test_row_length_limits(api, lib, p, nx):
    """L = 1 (no lower slot, an apron of one block), 23 and 25 (either side of the switch between the kernel's two instances) and
    35 (the largest): taken, with 3 blocks per slice of eight.  The offsets of 11, 12 and 17 pairs include 1, 63, 64 and 65."""
    offs = {0: [], 11: SC.P11, 12: SC.P12, 17: SC.P17}[p]
    assert len(offs) == p and (p == 0 or {1, 63, 64, 65} <= set(offs))
    rng = np.random.default_rng(2500 + p)
    n = SC.sym_region_rows(0, offs, 3)
    rp, col, val = R.system(n, np.asarray(offs, np.int64), rng)
    x = rng.standard_normal(n)
    A, y, want = open_case(api, lib, rp, col, val, x, nx, 0, ("L", 2 * p + 1, nx))
    c = geometry(want, n)
    assert c.L == 2 * p + 1 and c.Q == SC.apron(max(offs, default=0)) and c.nx * c.S == (26 if nx == 1 else 24)
    A.destroy()


def test_row_length_beyond_the_limit(api, lib):
    """18 pairs, 37 entries per row: beyond SYM_MAXL, and a block of 64 rows beyond the LDS window, so the packed kernel does not
    answer at all.  Not the symmetric kernel, the bits of the mode off, exact rows, a status that says refused or not tried."""
    rng = np.random.default_rng(2518)
    n = SC.sym_region_rows(0, SC.P18, 3)
    rp, col, val = R.system(n, SC.P18, rng)
    x = rng.standard_normal(n)
    xd = torch.from_numpy(x).cuda()
    A = api.CsrMatrix.from_csr(rp, col, val)
    A.set_kernel(-64)
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    ys = []
    for mode in (1, 0):
        A.set_sym_runs(mode, 1)
        y = torch.full((n,), 5.0 + mode, dtype=torch.float64, device="cuda")
        A.spmv(xd, y); api.synchronize()
        took, k = A.sym_runs(), R.kernel(lib, A)
        assert "k_spmv_ldsp_sym" not in k and took[0] == 0 and took[1] == 0, (mode, took, k)
        assert took[2].startswith("refused") or took[2] == "not tried", took
        ys.append(y)
    assert R.bits_equal(ys[0], ys[1])
    X.assert_rows(ys[1].cpu().numpy(), rp, col, val, x, ("L 37",))
    A.destroy()


@pytest.mark.parametrize("shape", ["even", "diagonal first"])
def test_row_shapes_refused(api, lib, shape):
    """Offsets -3, 0, 5, 70 (an even row length) and 0, 3, 70 (odd, the diagonal not in the middle): refused, "no odd row length"."""
    lo, up = ([3], [5, 70]) if shape == "even" else ([], [3, 70])
    rng = np.random.default_rng(2540)
    rp, col, val = SC.block_system([(64 * 30 + 9, (lo, up), "skew")], rng)
    x = rng.standard_normal(len(rp) - 1)
    A, y, want = open_case(api, lib, rp, col, val, x, 1, 0, (shape,))
    assert want.sym_runs == (0, 0, SC.WHY_SHAPE) and "no odd row length" in want.sym_runs[2] and len(want.kept) == 1
    A.destroy()


# ------------------------------------------------------------------------------------------------ 7. the automatic mode
def test_automatic_mode(api, lib):
    """Nothing set -- the mode every user gets: a symmetric stretch is looked for from nnz . 12 >= 512 MiB.  The generated
    constant-diagonal system (16 pairs, band 3000) just below that size is not looked at; just above it the stretch is taken,
    in one slice, the default group in the kernel string, and y has the bits of the mode off.  That y is held to exact rows on a
    sample: the first and last 128 rows, the blocks around the first and the last block of the sliced range, 4096 random rows.
    Both handles, 1.36 million rows and 44.7 million entries each: 0.9 s on an MI355X, most of it the copy to the host and the
    expected plan there."""
    t0 = time.time()
    limit = 512 << 20
    need = -(-limit // 12)                      # entries from which the rule holds
    n_lo = need // 33
    lo = api.CsrMatrix.generate(n_lo, 16, 3000, True, 7, 0.01, pattern=api.GEN_DIAGONALS)
    clipped = 33 * n_lo - lo.nnz                # entries the band's ends lose: the same for every n
    n_hi = -(-(need + clipped) // 33)
    hi = api.CsrMatrix.generate(n_hi, 16, 3000, True, 7, 0.01, pattern=api.GEN_DIAGONALS)
    assert lo.nnz * 12 < limit <= hi.nnz * 12 and 0 < n_hi - n_lo < 3000, (n_lo, lo.nnz, n_hi, hi.nnz)
    x = np.random.default_rng(2700).standard_normal(n_hi)
    xd = torch.from_numpy(x).cuda()
    y = torch.full((n_lo,), 3.0, dtype=torch.float64, device="cuda")
    lo.spmv(xd[:n_lo], y); api.synchronize()
    took, k = lo.sym_runs(), R.kernel(lib, lo)
    assert took[0] == 0 and took[1] == 0 and k.startswith("k_spmv_ldsp (") and "k_spmv_ldsp_sym" not in k, (took, k)
    lo.destroy()
    ys = []
    for mode in (-1, 0):
        if mode == 0:
            hi.set_sym_runs(0)
        yy = torch.full((n_hi,), 4.0 + mode, dtype=torch.float64, device="cuda")
        hi.spmv(xd, yy); api.synchronize()
        ys.append((yy, hi.sym_runs(), R.kernel(lib, hi)))
    t1 = time.time()
    rp, col, val = hi.arrays_to_host()
    want = SC.expected_plan(rp, col, val, 1)
    c = want.taken
    assert c is not None and c.L == 33 and c.S > n_hi // 64 - 160, want.status         # (all but the band's ends, their apron and the alignment)
    (y_on, took_on, k_on), (y_off, took_off, k_off) = ys
    assert took_on == want.sym_runs == (1, c.S, "taken"), (took_on, want.sym_runs)
    assert k_on.startswith("k_spmv_ldsp (") and GR.named(k_on, G_NOW), k_on
    assert took_off[0] == 0 and k_off.startswith("k_spmv_ldsp (") and "k_spmv_ldsp_sym" not in k_off, (took_off, k_off)
    assert R.bits_equal(y_on, y_off)
    last = c.inner0 + c.S - 1
    blocks = [b for b in (c.inner0 - 1, c.inner0, c.inner0 + 1, last - 1, last, last + 1) if 0 <= 64 * b < n_hi]
    rows = np.concatenate([np.arange(128), np.arange(n_hi - 128, n_hi)] + [np.arange(64 * b, min(64 * b + 64, n_hi)) for b in blocks]
                          + [np.random.default_rng(2701).integers(0, n_hi, 4096)])
    X.assert_rows(y_off.cpu().numpy(), rp, col, val, x, ("automatic",), rows=np.unique(rows))
    hi.destroy()
    print(f"automatic mode: n {n_lo} / {n_hi}, {len(col)} entries above; device part {t1 - t0:.2f} s, host checks {time.time() - t1:.2f} s")


if __name__ == "__main__":
    from liblcg_amd import _lib, api as _api
    _l = _lib.load()
    print(json.dumps({"G": G_NOW, "cases": {key: run(_api, _l) for key, run in ONE_SLICE_CASES.items()}}))
