"""Matrices and the expected plan for the tests of symmetric run stretches (csr_sym.hip, csr_sym.hpp) -- a helper of the tests, plain
NumPy, no GPU.  block_system builds block-diagonal CSR matrices whose regions are constant-diagonal systems (symmetric or not) or
random rows; expected_plan restates, from the CSR arrays alone, what the library must find in them: the run stretches, which of them
qualifies as a symmetric one, its apron and sliced range, and the words k_sym_check compares; perturb_outside / perturb_inside
change values off and on that set of words."""
from types import SimpleNamespace

import numpy as np

WINDOW = 2240       # entries of the largest LDS window (LdsCfg<double>::CH): a block of 64 rows beyond it does not take the packed kernel
RS_MAX = 4          # stretches a plan keeps (internal.hpp)
RS_QMIN = 12        # slots per wavefront a stretch's table holds at least (internal.hpp)
SYM_MAXL = 36       # csr_sym.hip

WHY_SHAPE = "refused: no odd row length with the diagonal in the middle"
WHY_OFFSETS = "refused: the offsets are not antisymmetric and ascending"
WHY_RANGE = "refused: the inner range is shorter than the slices"
WHY_VALUES = "refused: the values do not mirror each other bit for bit"


# ------------------------------------------------------------------------------------------------ run stretches
def stretches(rp, col, n):
    """Every maximal sequence of >= 2 consecutive full run blocks with the same L, the same offsets of row 0 from the block's first
    row and entries that follow each other, in block order: (b0, b1, L, offsets, first entry)."""
    rp = np.asarray(rp, np.int64); col = np.asarray(col, np.int64)
    lens = np.diff(rp)
    key = []            # per full block: None (no run block) or (L, offsets, first entry)
    for b in range(n // 64):
        r0 = 64 * b
        L = int(lens[r0])
        s = int(rp[r0])
        run = L > 0 and bool(np.all(lens[r0:r0 + 64] == L))
        if run:
            blk = col[s:s + 64 * L].reshape(64, L)
            run = bool(np.array_equal(blk, blk[0][None, :] + np.arange(64)[:, None]))
        key.append((L, tuple((blk[0] - r0).tolist()), s) if run else None)
    found = []
    b = 0
    while b < len(key):
        if key[b] is None:
            b += 1
            continue
        e = b + 1
        while e < len(key) and key[e] is not None and key[e][:2] == key[b][:2] and key[e][2] == key[b][2] + (e - b) * 64 * key[b][0]:
            e += 1
        if e - b >= 2:
            found.append((b, e, key[b][0], key[b][1], key[b][2]))
        b = e
    return found


def kept_stretches(rp, col, n):
    """The stretches a plan keeps: the RS_MAX longest (of equal lengths the first), in block order."""
    top = sorted(stretches(rp, col, n), key=lambda t: -(t[1] - t[0]))[:RS_MAX]       # (sorted is stable, as std::stable_sort)
    return sorted(top, key=lambda t: t[0])


def expected_stretches(rp, col, n):
    """Lengths (in blocks) of the stretches in use, from the CSR arrays: the four longest maximal sequences of >= 2 consecutive full
    run blocks with the same L, the same offsets of row 0 from the block's first row and entries that follow each other."""
    return sorted((t[1] - t[0] for t in kept_stretches(rp, col, n)), reverse=True)


# ------------------------------------------------------------------------------------------------ the symmetric stretch
def offsets_ok(off):
    """csr_sym.hpp: sym_offsets_ok."""
    L = len(off)
    if L < 1 or L % 2 == 0:
        return False
    p = L // 2
    return off[p] == 0 and all(off[k] > off[k - 1] for k in range(1, L)) and all(off[2 * p - k] == -off[k] for k in range(p))


def apron(maxoff):
    """csr_sym.hpp: sym_apron."""
    return (maxoff + 63) // 64 + 1


def sliced_range(b0, b1, Q, nx):
    """csr_sym.hpp: sym_range -- (inner0, S), or None where fewer than nx blocks are left."""
    first = (b0 + Q + 7) // 8 * 8
    if nx < 1 or first + nx > b1:
        return None
    return first, (b1 - first) // nx


def checked_words(rp, col, plan):
    """The index pairs (lower, upper) into the value array that k_sym_check compares for the stretch `plan` (an expected_plan's, its
    `taken`, or one of its candidates): for every row of the sliced range and every lower slot k < p the row's k-th entry and, in
    the row that entry's column names, entry 2p - k.  Row by row, slot by slot: pair 0 is (first row of inner0, slot 0), the last
    pair (last row of the range, slot p - 1)."""
    c = getattr(plan, "taken", plan)
    rp = np.asarray(rp, np.int64); col = np.asarray(col, np.int64)
    p = c.L // 2
    rows = np.arange(64 * c.inner0, 64 * (c.inner0 + c.nx * c.S), dtype=np.int64)
    k = np.arange(p, dtype=np.int64)
    lower = rp[rows][:, None] + k[None, :]
    upper = rp[col[lower]] + (2 * p - k)[None, :]
    assert np.array_equal(col[upper], np.broadcast_to(rows[:, None], upper.shape))       # (the partner's entry points back)
    return lower.ravel(), upper.ravel()


def expected_plan(rp, col, val, nx):
    """What sym_runs_build must make of the CSR arrays with nx slices.  The kept stretches are walked by length (of equal lengths
    the first); one qualifies when its row length is odd, at most SYM_MAXL, with the diagonal in the middle, its offsets pass
    offsets_ok, its sliced range holds nx blocks at least and the checked words mirror each other as 64-bit integers.  The first
    that qualifies is taken; where none does, the status is the refusal of the LONGEST.
    .kept: the kept stretches; .cands: one record per kept stretch in the order walked (b0, b1, L, s0, off, kd, why and, as far as
    the walk got, Q, inner0, S, nx, mirrors); .taken: the record taken or None; .sym_runs: what CsrMatrix.sym_runs() must say."""
    n = len(rp) - 1
    bits = np.ascontiguousarray(val, np.float64).view(np.uint64)
    kept = kept_stretches(rp, col, n)
    cands, taken = [], None
    for b0, b1, L, off, s0 in sorted(kept, key=lambda t: -(t[1] - t[0])):
        zero = [k for k in range(L) if off[k] == 0]
        c = SimpleNamespace(b0=b0, b1=b1, L=L, s0=s0, off=off, kd=zero[-1] if zero else -1, nx=nx, why="taken")
        cands.append(c)
        if L % 2 == 0 or c.kd != L // 2 or L > SYM_MAXL:
            c.why = WHY_SHAPE
            continue
        if not offsets_ok(off):
            c.why = WHY_OFFSETS
            continue
        c.Q = apron(off[-1])
        rg = sliced_range(b0, b1, c.Q, nx)
        if rg is None:
            c.why = WHY_RANGE
            continue
        c.inner0, c.S = rg
        lo, up = checked_words(rp, col, c)
        c.mirrors = bool(np.array_equal(bits[lo], bits[up]))
        if not c.mirrors:
            c.why = WHY_VALUES
            continue
        taken = c
        break
    status = "taken" if taken else (cands[0].why if cands else "no run stretch")
    return SimpleNamespace(kept=kept, cands=cands, taken=taken, status=status,
                           sym_runs=(nx, nx * taken.S, "taken") if taken else (0, 0, status))


def _flip(val, at):
    out = np.array(val, np.float64)
    b = out.view(np.uint64)
    at = np.unique(np.asarray(at, np.int64))
    assert len(at) and np.all(np.isfinite(out[at])) and np.all(out[at] != 0.0)
    b[at] ^= np.uint64(1)           # the last bit of the mantissa: one ulp up or down, never a zero, an infinity or a NaN
    return out


def perturb_outside(val, pairs, at):
    """A copy of val with the entries `at` moved by one ulp; none of them may be a word k_sym_check compares (pairs: checked_words)."""
    assert not np.isin(at, np.concatenate(pairs)).any(), "an entry of the checked set"
    return _flip(val, at)


def perturb_inside(val, pairs, at):
    """A copy of val with the entries `at` moved by one ulp; every one of them must be a word k_sym_check compares, and no pair may
    be moved on both sides."""
    at = np.unique(np.asarray(at, np.int64))
    assert np.isin(at, np.concatenate(pairs)).all(), "an entry off the checked set"
    assert not (np.isin(pairs[0], at) & np.isin(pairs[1], at)).any()
    return _flip(val, at)


# ------------------------------------------------------------------------------------------------ matrices
def region_starts(regions):
    return np.concatenate([[0], np.cumsum([r[0] for r in regions])]).astype(np.int64)


def _ragged(lens, rng):
    """Random sorted rows of the given lengths, the diagonal always among them, columns within the region.  The diagonal is 1 + the
    sums of its row's and its column's other magnitudes: the symmetric part is positive definite, so a CG run neither breaks down
    nor overflows."""
    rows = len(lens)
    assert rows >= 48 and lens.min() >= 1 and lens.max() <= 48
    cols, vals = [], []
    for i in range(rows):
        others = rng.choice(rows - 1, int(lens[i]) - 1, replace=False)
        others = others + (others >= i)
        c = np.sort(np.concatenate([others, [i]]))
        v = rng.standard_normal(len(c))
        v[c == i] = 0.0
        cols.append(c); vals.append(v)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate(cols); val = np.concatenate(vals)
    rowsum = np.add.reduceat(np.abs(val), rp[:-1])
    colsum = np.bincount(col, np.abs(val), rows)
    val[col == np.repeat(np.arange(rows), lens)] = 1.0 + rowsum + colsum
    return rp, col, val


def block_system(regions, rng):
    """Block-diagonal CSR matrix of consecutive regions (rows, offs, kind); a region's columns stay within its own rows, its
    diagonals are clipped at its own edges, and its first row need not be a multiple of 64.  kind:
      "sym"    diagonals 0, +-offs with A[i, i + o] = A[i + o, i] (test_gpu_sym_runs.system);
      "asym"   the same pattern, the values below the diagonal independent of those above it;
      "skew"   offs = (lower, upper): other offsets above the diagonal than below it (their counts may differ too);
      "ragged" random sorted rows of 1 .. 48 entries (offs is ignored); every block of 64 rows of the MATRIX keeps at most WINDOW
               entries, so that the forced packed kernel still answers.
    Returns rowptr, columns (int32) and values."""
    from test_gpu_sym_runs import system        # (not copied; imported here: that module may import this one)

    starts = region_starts(regions)
    n = int(starts[-1])
    # entries per row of the regions that are not ragged, so that the ragged rows know how much room their blocks have left
    lens = np.zeros(n, np.int64)
    ragged = np.zeros(n, bool)
    for (rows, offs, kind), r0 in zip(regions, starts):
        if kind == "ragged":
            ragged[r0:r0 + rows] = True
            continue
        lo, up = (offs, offs) if kind != "skew" else offs
        i = np.arange(rows)
        lens[r0:r0 + rows] = 1 + sum(((i - o >= 0).astype(np.int64) for o in lo), np.zeros(rows, np.int64)) \
                               + sum(((i + o < rows).astype(np.int64) for o in up), np.zeros(rows, np.int64))
    # ragged rows: the longer of two draws from 1 .. 48 (mean 32: a block of 64 such rows comes close to the window, and the mean row
    # of a mixed matrix stays above the 17 entries from which the automatic choice takes blocks of 64 rows), then the longest rows
    # of a block that exceeds the window lose entries one by one
    lens[ragged] = np.maximum(rng.integers(1, 49, int(ragged.sum())), rng.integers(1, 49, int(ragged.sum())))
    for a in range(0, n, 64):
        e = min(a + 64, n)
        while lens[a:e].sum() > WINDOW:
            j = a + int(np.argmax(np.where(ragged[a:e], lens[a:e], 0)))
            assert ragged[j] and lens[j] > 1
            lens[j] -= 1
    parts = []
    for (rows, offs, kind), r0 in zip(regions, starts):
        if kind == "ragged":
            rp, col, val = _ragged(lens[r0:r0 + rows], rng)
        elif kind == "sym":
            rp, col, val = system(rows, np.asarray(offs, np.int64), rng)
        elif kind == "asym":
            rp, col, val = system(rows, np.asarray(offs, np.int64), rng, upper=np.asarray(offs, np.int64))
        elif kind == "skew":
            rp, col, val = system(rows, np.asarray(offs[0], np.int64), rng, upper=np.asarray(offs[1], np.int64))
        else:
            raise ValueError(kind)
        parts.append((np.asarray(rp, np.int64), np.asarray(col, np.int64) + r0, np.asarray(val, np.float64)))
    first = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])])
    rp = np.concatenate([[0]] + [p[0][1:] + first[i] for i, p in enumerate(parts)])
    return rp.astype(np.int32), np.concatenate([p[1] for p in parts]).astype(np.int32), np.concatenate([p[2] for p in parts])


def sym_region_rows(start, offs, S, behind=2, tail=37):
    """Rows of a constant-diagonal region that begins at row `start` so that its stretch gives eight slices S blocks each, `behind`
    blocks (< 8) of the stretch stay behind them and `tail` (< 64) full rows follow the stretch's last block."""
    m = max(offs, default=0)
    b0 = -(-(start + m) // 64)
    inner0 = -(-(b0 + apron(m)) // 8) * 8
    assert 0 <= behind < 8 and 0 <= tail < 64
    return 64 * (inner0 + 8 * S + behind) + m + tail - start


def sym_region_rows_inner(start, offs, S, tail=37):
    """The same for ONE slice with an inner range of exactly S blocks."""
    m = max(offs, default=0)
    b0 = -(-(start + m) // 64)
    inner0 = -(-(b0 + apron(m)) // 8) * 8
    return 64 * (inner0 + S) + m + tail - start


def region_rows_for_blocks(start, maxoff, nblocks, tail=37):
    """Rows of a constant-diagonal region that begins at row `start` so that its stretch has exactly nblocks blocks."""
    assert 0 <= tail < 64
    b0 = -(-(start + maxoff) // 64)
    return 64 * (b0 + nblocks) + maxoff + tail - start


# ------------------------------------------------------------------------------------------------ the mixed cases
P11 = [1, 5, 20, 33, 63, 64, 65, 90, 100, 127, 128]                                            # L = 23: the largest of the NS = 6 instance
P12 = P11 + [130]                                                                               # L = 25: the smallest of the NS = 9 instance
P17 = [1, 2, 3, 7, 20, 33, 63, 64, 65, 96, 127, 128, 129, 160, 192, 200, 210]                   # L = 35: the largest
P18 = P17 + [230]                                                                               # L = 37: beyond SYM_MAXL and the LDS window
WIDE = [1, 63, 64, 65, 2047, 2048, 5000]                                                        # Q = 80
HEAD, TAIL = 5 * 64 + 17, 4 * 64 + 29


def head_tail_regions(offs, S):
    """ragged (5 blocks + 17 rows) | sym | ragged (4 blocks + 29 rows): eight slices of S blocks, two blocks of the stretch behind them."""
    rows = sym_region_rows(HEAD, offs, S)
    if (HEAD + rows + TAIL) % 64 == 0:          # (the last block stays partial)
        rows = sym_region_rows(HEAD, offs, S, tail=38)
    return [(HEAD, None, "ragged"), (rows, offs, "sym"), (TAIL, None, "ragged")]


def chain_regions(spec, tail=29):
    """Regions (kind, offs, blocks of the stretch) one behind the other, the first at row 0; a skew region's offs are (lower, upper)."""
    regions, start = [], 0
    for kind, offs, nblocks in spec:
        m = max(max(offs[0], default=0), max(offs[1], default=0)) if kind == "skew" else max(offs, default=0)
        rows = region_rows_for_blocks(start, m, nblocks, tail)
        regions.append((rows, offs, kind))
        start += rows
    return regions


D3 = [1, 5, 37]


def not_longest_specs(P7, P16):
    """The matrices whose symmetric stretch is not the longest (chain_regions' specs).  "3d": six regions as in
    test_gpu_run_stretches.py's test_more_stretches_than_descriptors, of 6, 26, 14, 36, 12 and 20 blocks -- the symmetric one the
    third longest, then the fifth longest, which gets no descriptor."""
    sizes = (6, 26, 14, 36, 12, 20)
    return {"3a": [("asym", P7, 40), ("sym", P7, 20)],
            "3b": [("skew", ([1, 5, 70], [2, 9, 50]), 40), ("sym", P7, 20)],
            "3c": [("sym", P16, 30), ("sym", P7, 20)],
            "3d third": [("sym" if i == 5 else "asym", D3, b) for i, b in enumerate(sizes)],
            "3d fifth": [("sym" if i == 4 else "asym", D3, b) for i, b in enumerate(sizes)]}


def outside_sets(rp, col, plan, regions):
    """Entries of the matrix that k_sym_check must not look at, by name (plan: an expected_plan with a stretch taken)."""
    c = plan.taken
    rp = np.asarray(rp, np.int64); col = np.asarray(col, np.int64)
    p = c.L // 2
    rows = np.arange(64 * (c.inner0 - c.Q), 64 * c.inner0)
    upper = rp[rows][:, None] + (p + 1 + np.arange(p))[None, :]
    out = {"apron lower": (rp[rows][:, None] + np.arange(p)[None, :]).ravel(),
           "apron upper within the apron": upper[col[upper] < 64 * c.inner0],
           "behind the range": np.arange(rp[64 * (c.inner0 + c.nx * c.S)], rp[64 * c.b1])}
    starts = region_starts(regions)
    out["ragged"] = np.concatenate([np.arange(rp[r0], rp[r0 + rows]) for (rows, offs, kind), r0 in zip(regions, starts) if kind == "ragged"])
    return out


def inside_words(rp, col, plan):
    """Three words k_sym_check does compare: the first and the last lower word, and the first upper entry of the last apron row
    (all of that row's upper entries point into the range)."""
    lo, up = checked_words(rp, col, plan)
    c = plan.taken
    return {"first checked word": int(lo[0]), "last checked word": int(lo[-1]),
            "last apron row's upper entry into the range": int(rp[64 * c.inner0 - 1]) + c.L // 2 + 1}
