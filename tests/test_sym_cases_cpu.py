"""No GPU: the builders and the expected plan of tests/sym_cases.py, which tests/test_gpu_sym_mixed.py holds the library to.  On the
pure constant-diagonal systems the expected plan (found in the CSR arrays) is the closed form of test_gpu_sym_runs.plan; the
builders give what they claim; the perturbations land where they say; csr_sym.hpp, compiled alone as tests/test_sym_map.py does,
agrees on apron, first block and blocks per slice of every stretch of the mixed matrices; and exact_ref's row selection checks what
the full call checks on those rows."""
import subprocess

import numpy as np
import pytest

import exact_ref as X
import sym_cases as SC
import test_gpu_sym_groups as GR
import test_gpu_sym_runs as R
import test_sym_map as M


def mixed():
    """name -> (rowptr, col, val, regions) of the mixed matrices test_gpu_sym_mixed.py runs (the same seeds)."""
    out = {}
    for name, offs, S in (("16 pairs", R.P16, 1), ("7 pairs", R.P7, 1)):
        regions = SC.head_tail_regions(offs, S)
        out["head and tail, " + name] = SC.block_system(regions, np.random.default_rng(2200 + len(offs))) + (regions,)
    for name, spec in SC.not_longest_specs(R.P7, R.P16).items():
        regions = SC.chain_regions(spec)
        out[name] = SC.block_system(regions, np.random.default_rng(2300)) + (regions,)
    return out


@pytest.fixture(scope="module")
def mixed_cases():
    return mixed()


def test_expected_plan_on_pure_systems():
    """Every (offsets, S, nx) of test_gpu_sym_runs.test_products and every (offsets, range) of test_gpu_sym_groups: one stretch,
    taken, with the closed form's b0, b1, Q, inner0 and S."""
    cases = [(offs, R.rows_for(offs, S), (1, 2, 4, 8)) for offs in (R.P1_64, R.P1_37, R.P7, R.P16) for S in (1, 3)]
    cases += [(offs, GR.rows_for_inner(offs, S), (1,)) for _, offs in GR.OFFSETS for S in GR.RANGES]
    cases += [(R.P16, R.rows_for(R.P16, 6), (1,)), (R.P16, GR.rows_for_inner(R.P16, 90), (1,))]
    for offs, n, slices in cases:
        rp, col, val = R.system(n, offs, np.random.default_rng(n))
        for nx in slices:
            want = R.plan(n, offs, nx)
            got = SC.expected_plan(rp, col, val, nx)
            c = got.taken
            assert c is not None and len(got.kept) == 1 and got.cands == [c], (offs, n, nx, got.status)
            assert (c.b0, c.b1, c.Q, c.inner0, c.S) == want, (offs, n, nx, want)
            assert c.L == 2 * len(offs) + 1 and c.kd == len(offs) and list(c.off[len(offs) + 1:]) == sorted(offs)
            assert got.sym_runs == (nx, nx * want[4], "taken")


def test_expected_plan_refusals():
    """The refusals test_gpu_sym_runs.py provokes, as the expected plan words them."""
    n = R.rows_for(R.P7, 1)
    rp, col, val = R.system(n, R.P7, np.random.default_rng(1))
    pairs = SC.checked_words(rp, col, SC.expected_plan(rp, col, val, 8))
    assert SC.expected_plan(rp, col, SC.perturb_inside(val, pairs, pairs[0][[5]]), 8).sym_runs == (0, 0, SC.WHY_VALUES)
    rp, col, val = R.system(R.rows_for([70], 1), [70], np.random.default_rng(2), upper=[50])
    assert SC.expected_plan(rp, col, val, 8).sym_runs == (0, 0, SC.WHY_OFFSETS)
    rp, col, val = R.system(64 * 6, [70], np.random.default_rng(3))             # a stretch of two blocks
    assert SC.expected_plan(rp, col, val, 1).sym_runs == (0, 0, SC.WHY_RANGE)
    rp, col, val = R.system(100, [70], np.random.default_rng(4))
    assert SC.expected_plan(rp, col, val, 1).sym_runs == (0, 0, "no run stretch")
    for lo, up in (([3], [5, 70]), ([], [3, 70])):                              # an even row length; the diagonal first
        rp, col, val = SC.block_system([(64 * 20 + 9, (lo, up), "skew")], np.random.default_rng(5))
        assert SC.expected_plan(rp, col, val, 1).sym_runs == (0, 0, SC.WHY_SHAPE)
    rp, col, val = R.system(SC.sym_region_rows(0, SC.P18, 1), SC.P18, np.random.default_rng(6))
    assert SC.expected_plan(rp, col, val, 1).sym_runs == (0, 0, SC.WHY_SHAPE)  # (37 entries per row)


def test_builders(mixed_cases):
    """Sorted rows, block-diagonal, every diagonal present, symmetric pattern and values where they are claimed, the partial last block."""
    for name, (rp, col, val, regions) in mixed_cases.items():
        rp64 = rp.astype(np.int64)
        n = len(rp) - 1
        starts = SC.region_starts(regions)
        assert n == starts[-1] and n % 64 != 0, (name, n)                       # the partial last block
        assert any(s % 64 for s in starts[1:-1]), (name, starts)                # region starts that are no multiples of 64
        lens = np.diff(rp64)
        row = np.repeat(np.arange(n), lens)
        inner = np.ones(len(col), bool); inner[rp64[:-1][lens > 0]] = False     # not the first entry of its row
        assert np.all(np.diff(col.astype(np.int64))[inner[1:]] > 0), name      # sorted rows, no duplicates
        first = np.arange(0, n, 64)
        assert int((rp64[np.minimum(first + 64, n)] - rp64[first]).max()) <= SC.WINDOW, name
        dense = {}
        for (rows, offs, kind), r0 in zip(regions, starts):
            a, e = rp64[r0], rp64[r0 + rows]
            assert col[a:e].min() >= r0 and col[a:e].max() < r0 + rows, (name, kind)      # block-diagonal
            assert np.all(np.isin(np.arange(r0, r0 + rows), col[a:e][col[a:e] == row[a:e]])), (name, kind)   # every row holds its diagonal
            if kind == "ragged":
                assert lens[r0:r0 + rows].min() >= 1 and lens[r0:r0 + rows].max() <= 48 and len(set(lens[r0:r0 + rows])) > 8
                continue
            D = np.zeros((rows, rows))
            D[row[a:e] - r0, col[a:e] - r0] = val[a:e]
            P = D != 0
            if kind == "sym":
                assert np.array_equal(D, D.T), name                             # bit for bit (no NaN here)
            elif kind == "asym":
                assert np.array_equal(P, P.T) and not np.array_equal(D, D.T), name
            else:
                assert not np.array_equal(P, P.T), name
            lo, up = (offs, offs) if kind != "skew" else offs
            i = rows // 2
            assert (col[rp64[r0 + i]:rp64[r0 + i + 1]] - (r0 + i)).tolist() == sorted([-o for o in lo] + [0] + list(up)), name
    rp, col, val, regions = mixed_cases["head and tail, 16 pairs"]
    assert int(np.diff(rp).max()) == 48


def test_ragged_cap(monkeypatch):
    """Drawn freely, 64 rows of 1 .. 48 entries stay far below the window of 2240; with the window set to 1200 the same draw is
    cut: every block of the matrix, those shared with a constant-diagonal region included, keeps to it."""
    regions = [(64 * 3 + 17, None, "ragged"), (64 * 4 + 5, [1, 2, 3, 4, 5, 6, 7, 8], "sym"), (64 * 2 + 30, None, "ragged")]
    for window in (SC.WINDOW, 1200):
        monkeypatch.setattr(SC, "WINDOW", window)
        rp, col, val = SC.block_system(regions, np.random.default_rng(9))
        n = len(rp) - 1
        first = np.arange(0, n, 64)
        per_block = rp[np.minimum(first + 64, n)].astype(np.int64) - rp[first]
        assert per_block.max() <= window and (per_block.max() > 1200) == (window != 1200), (window, per_block)
        assert window == 2240 or per_block.max() > window // 2         # (cut to an equal share per row, not emptied)


def test_mixed_plans(mixed_cases):
    """What the mixed matrices are built for: which stretch is the longest, which is taken, and that the geometry the GPU tests
    want holds -- the apron does not end on a multiple of eight blocks, and with eight slices two blocks stay behind the range."""
    for name in ("head and tail, 16 pairs", "head and tail, 7 pairs"):
        rp, col, val, regions = mixed_cases[name]
        for nx in (1, 8):
            plan = SC.expected_plan(rp, col, val, nx)
            c = plan.taken
            assert c is not None and len(plan.kept) == 1, (name, plan.status)
            assert (c.b0 + c.Q) % 8 != 0 and c.b0 > SC.HEAD // 64 and c.b1 - c.inner0 == 8 * 1 + 2
            assert c.b1 - (c.inner0 + nx * c.S) == (2 if nx == 8 else 0)
    want = {"3a": ([40, 20], 1, "taken"), "3b": ([40, 20], 1, "taken"), "3c": ([30, 20], 0, "taken"),
            "3d third": ([36, 26, 20, 14], 2, "taken"), "3d fifth": ([36, 26, 20, 14], None, SC.WHY_VALUES)}
    for key, (lengths, which, status) in want.items():
        rp, col, val, regions = mixed_cases[key]
        for nx in (1, 8):
            plan = SC.expected_plan(rp, col, val, nx)
            assert sorted((t[1] - t[0] for t in plan.kept), reverse=True) == lengths, (key, plan.kept)
            assert plan.status == status, (key, nx, plan.status)
            if which is None:
                assert plan.taken is None and len(plan.cands) == 4
                continue
            assert plan.taken is plan.cands[which] and len(plan.cands) == which + 1
            assert plan.taken.b1 - plan.taken.b0 == lengths[which] and (which == 0 or plan.taken.b0 > 40)     # deep inside the matrix
            assert [c.why for c in plan.cands[:which]] == [SC.WHY_OFFSETS if key == "3b" else SC.WHY_VALUES] * which
    # "3d fifth": the symmetric region would be taken had it a descriptor -- alone it is
    rp, col, val, regions = mixed_cases["3d fifth"]
    assert regions[4][2] == "sym"
    alone = SC.block_system([regions[4]], np.random.default_rng(7))
    assert SC.expected_plan(*alone, 1).status == "taken"


def test_perturbations(mixed_cases):
    rp, col, val, regions = mixed_cases["head and tail, 16 pairs"]
    plan = SC.expected_plan(rp, col, val, 8)
    c = plan.taken
    lo, up = pairs = SC.checked_words(rp, col, plan)
    p = c.L // 2
    assert len(lo) == 64 * 8 * c.S * p and len(set(lo.tolist()) | set(up.tolist())) == 2 * len(lo)
    assert lo[0] == rp[64 * c.inner0] and lo[-1] == rp[64 * (c.inner0 + 8 * c.S) - 1] + p - 1
    assert col[lo[0]] == 64 * c.inner0 - max(R.P16) and up[0] == rp[col[lo[0]]] + 2 * p
    assert up.min() >= rp[64 * (c.inner0 - c.Q)] and lo.max() < rp[64 * (c.inner0 + 8 * c.S)]
    sets = SC.outside_sets(rp, col, plan, regions)
    assert set(sets) == {"apron lower", "apron upper within the apron", "behind the range", "ragged"} and all(len(v) for v in sets.values())
    everything = np.concatenate(list(sets.values()))
    for name, at in list(sets.items()) + [("all", everything)]:
        v2 = SC.perturb_outside(val, pairs, at)
        changed = np.flatnonzero(v2.view(np.uint64) != val.view(np.uint64))
        assert np.array_equal(changed, np.unique(at)), name
        assert np.all(np.abs(v2[changed] - val[changed]) <= np.spacing(np.abs(val[changed]))), name      # one ulp
        again = SC.expected_plan(rp, col, v2, 8)
        assert again.sym_runs == plan.sym_runs and vars(again.taken) == vars(c), name
    with pytest.raises(AssertionError):
        SC.perturb_outside(val, pairs, lo[[0]])
    inside = SC.inside_words(rp, col, plan)
    assert set(inside) == {"first checked word", "last checked word", "last apron row's upper entry into the range"}
    assert inside["first checked word"] == lo[0] and inside["last checked word"] == lo[-1]
    w = inside["last apron row's upper entry into the range"]
    assert rp[64 * c.inner0 - 1] <= w < rp[64 * c.inner0] and col[w] >= 64 * c.inner0 and w in set(up.tolist())
    for name, w in inside.items():
        v2 = SC.perturb_inside(val, pairs, [w])
        assert np.count_nonzero(v2.view(np.uint64) != val.view(np.uint64)) == 1
        assert SC.expected_plan(rp, col, v2, 8).sym_runs == (0, 0, SC.WHY_VALUES), name
    with pytest.raises(AssertionError):
        SC.perturb_inside(val, pairs, sets["ragged"][:1])


def test_header_agrees_on_the_mixed_cases(mixed_cases, tmp_path_factory):
    """csr_sym.hpp's sym_offsets_ok, sym_apron and sym_range on every kept stretch of the mixed matrices, for 1, 2, 4 and 8 slices."""
    exe = M._exe(tmp_path_factory)
    seen = 0
    for name, (rp, col, val, regions) in mixed_cases.items():
        for b0, b1, L, off, s0 in SC.kept_stretches(rp, col, len(rp) - 1):
            ok = int(subprocess.check_output([exe, "o", str(L)] + [str(o) for o in off], text=True))
            assert bool(ok) == SC.offsets_ok(off), (name, off)
            if not ok:
                continue
            for nx in (1, 2, 4, 8):
                out = subprocess.check_output([exe, "r", str(b0), str(b1), str(off[-1]), str(nx)], text=True).splitlines()[0].split()
                Q = SC.apron(off[-1])
                rg = SC.sliced_range(b0, b1, Q, nx)
                assert out == (["none", str(Q)] if rg is None else [str(Q), str(rg[0]), str(rg[1])]), (name, b0, b1, nx, out)
                seen += 1
    assert seen >= 4 * 12


def test_row_selection():
    """exact_ref.assert_rows / bad_rows with rows=: the rows it names are judged as the full call judges them."""
    rng = np.random.default_rng(8)
    rp, col, val = SC.block_system([(300, None, "ragged"), (200, [1, 70], "sym")], rng)
    n = len(rp) - 1
    x = rng.standard_normal(n)
    y = np.array([val[rp[i]:rp[i + 1]] @ x[col[rp[i]:rp[i + 1]]] for i in range(n)])
    X.assert_rows(y, rp, col, val, x)
    wrong = [3, 250, 299, 300, 499]
    y[wrong] *= 1 + 1e-12
    full = X.bad_rows(y, rp, col, val, x)
    assert full.tolist() == wrong
    for rows in (np.arange(n), np.array([499, 3, 4, 250, 7]), np.array([5, 6, 301]), np.arange(250, 301)):
        got = X.bad_rows(y, rp, col, val, x, rows=rows)
        assert sorted(got.tolist()) == sorted(set(rows.tolist()) & set(wrong)), rows
        if len(got):
            with pytest.raises(AssertionError):
                X.assert_rows(y, rp, col, val, x, rows=rows)
        else:
            X.assert_rows(y, rp, col, val, x, rows=rows)
    srp, scol, sval = X.select_rows(rp, col, val, np.array([7, 2]))
    assert scol.tolist() == col[rp[7]:rp[8]].tolist() + col[rp[2]:rp[3]].tolist() and srp.tolist() == [0, rp[8] - rp[7], rp[8] - rp[7] + rp[3] - rp[2]]
