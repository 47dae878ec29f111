"""Systems, window-edge matrices and drivers shared by the tests of the batched triangular applies and of batched PCG with a factor:
tests/test_gpu_tri_multi.py, tests/test_gpu_multi_pcg_m.py and tests/test_tri_multi_cases_cpu.py, which shows with the checkers
alone that the cases reach the branches they name.  Modelled on tests/multi_cases.py; a helper of the tests, not a conftest.

The batched sweep (csr_tri_multi.hip: k_ic_sweep_multi<K, DG>): a workgroup of IC_MT = 256 lanes owns mrows(k) = 512 / k consecutive
rows (k / 2 lanes per row) and stages their slice of the triangle -- counted from the 4-entry unit that holds its first entry -- in an
LDS window of IC_MCH = 2048 entries; a longer slice is walked out of global memory.  `window_matrix(factor, k, seed)` puts
successive workgroups of L (and, for ILU(0), of U) on both sides of that edge; `window_cases` names what a triangle's rowptr meets.

The exact batched solve runs on the factor's own level schedule: a level wider than 1024 rows is a launch of its own
(k_lvl_wide), a run of narrower ones is one launch of one workgroup (k_lvl_narrow).
"""
import ctypes as C

import numpy as np

import ic0_checker as IC
import ic0_sweeps_checker as S
import ilu0_checker as K

KS = (2, 4, 8)
IC_MT, IC_MCH = 256, 2048           # csr_tri.hpp
IC_WG = 1024                        # csr_tri.hpp: the widest level a narrow launch takes
FACTORS = ("ic0", "ilu0")
M_JACOBI, M_IC0, M_ILU0 = 0, 1, 2   # lcg_hip.h: LCG_HIP_M_*
PRECOND = {"ic0": M_IC0, "ilu0": M_ILU0}
E_ARG = -2003


def mrows(k):
    """csr_tri.hpp: ic_mrows."""
    return IC_MT * 2 // k


# ------------------------------------------------------------------------------------------ patterns of the triangles
def tri_rowptrs(factor, rowptr, col):
    """(rowptr of lo, rowptr of up) of the zero-fill factor of a matrix with sorted, duplicate-free rows, from its pattern alone.
    IC(0): lo = L, the entries on or below the diagonal; up = L^T.  ILU(0): lo = L strictly below (unit diagonal not stored),
    up = U on or above."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    assert np.all(np.bincount(row[col == row], minlength=n) == 1), "every row stores its diagonal once"

    def rp(cnt):
        return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)

    below = np.bincount(row[col < row], minlength=n)
    if factor == "ilu0":
        return rp(below), rp(np.bincount(row[col >= row], minlength=n))
    # column j of L = row j of L^T: entries (i, j) with i >= j
    return rp(below + 1), rp(np.bincount(col[col <= row], minlength=n))


def sweep_windows(n, rowptr, k):
    """Per workgroup of a k-wide sweep over the triangle with this rowptr: (own entries, cnt, rowptr[row0] & 3, rows), with
    cnt = rowptr[row0 + nrows] - (rowptr[row0] & ~3), the length the kernel compares with its window."""
    R = mrows(k)
    out = []
    for row0 in range(0, n, R):
        nrows = min(R, n - row0)
        s, e = int(rowptr[row0]), int(rowptr[row0 + nrows])
        out.append((e - s, e - (s & ~3), s & 3, nrows))
    return out


def window_cases(n, rowptr, k):
    """The window-edge situations a triangle's k-wide sweep meets, by name."""
    found = set()
    wins = sweep_windows(n, rowptr, k)
    for own, cnt, off, nrows in wins:
        if cnt == IC_MCH and off == 0:
            found.add("full_aligned")               # the largest staged slice
        if cnt == IC_MCH and off != 0:
            found.add("full_by_offset")             # staged: cnt = 2048 of which the first `off` entries are the neighbour's
        if own == cnt == IC_MCH + 1:
            found.add("over_by_one")                # 2049 of its own: global memory
        if own <= IC_MCH < cnt:
            found.add("over_by_offset")             # at most 2048 of its own, over only through rowptr[row0] & 3 != 0
        if cnt > IC_MCH:
            found.add("global_walk")
        if nrows < mrows(k):
            found.add("partial_last_workgroup")
    return found


# entries of lo (IC(0): its diagonals included) in successive workgroups after the first, and the rows of the short last one.  From
# an aligned start: 2048 (full, aligned), 2049 (over by one; the next starts at 1 mod 4), 2048 (over through the offset), 2047
# (full through the offset), then the tail.
WINDOW_LO = (2048, 2049, 2048, 2047)
WINDOW_UP = (2048, 2049, 2048, 2047, 1025)      # ILU(0)'s U (diagonals included), from its first workgroup on
WINDOW_TAIL = 40


def window_matrix(factor, k, seed=5):
    """(rowptr, col, val) of a matrix of 5 mrows(k) + WINDOW_TAIL rows whose factor's lo holds WINDOW_LO entries in workgroups
    1 .. 4 of the k-wide sweep (workgroup 0: the first layer, which has nothing below it but IC(0)'s diagonals -- a multiple of 4).
    ILU(0): not symmetric, and U holds WINDOW_UP entries in workgroups 0 .. 4.  Every workgroup is a layer: a row's strictly lower
    columns come from the layers before it (its strictly upper ones, ILU(0), from the layers after it), so each triangle has at
    most 6 levels.  A workgroup's entries are spread evenly over its rows, the first rows taking the remainder."""
    rng = np.random.default_rng(seed + 100 * k)
    R = mrows(k)
    groups = len(WINDOW_LO) + 1
    n = R * groups + WINDOW_TAIL
    lower, upper = [{} for _ in range(n)], [{} for _ in range(n)]

    def fill(part, a, b, total, lo, hi):
        q, r = divmod(total, b - a)
        for i in range(a, b):
            m = q + (i - a < r)
            if m:
                for j in rng.choice(hi - lo, size=m, replace=False) + lo:
                    part[i][int(j)] = IC._offdiag(rng, False)

    own = R if factor == "ic0" else 0                   # diagonals stored in lo
    for w in range(1, groups):
        fill(lower, w * R, (w + 1) * R, WINDOW_LO[w - 1] - own, 0, w * R)
    fill(lower, groups * R, n, 3 * WINDOW_TAIL + 1, 0, groups * R)      # the tail: a few entries per row, a length that is 1 mod 4
    if factor == "ic0":
        return IC.assemble(n, lower, IC.dominant_diagonal(rng, n, lower, False))
    for w in range(groups):
        fill(upper, w * R, (w + 1) * R, WINDOW_UP[w] - R, (w + 1) * R, n)
    return K.assemble(n, lower, upper, K.dominant_diagonal(rng, n, lower, upper, False))


# ------------------------------------------------------------------------------------------ systems of the apply tests
LAYERS = [3, 40, 1, 1500, 5, 2, 30, 1, 9]           # a 1500-row level (one wide launch) among narrow ones
LAYERS_U = [9, 1, 30, 1500, 2, 5, 1, 40, 3]

_SYSTEMS = {}


def system(factor, name):
    """(rowptr, col, val), rows sorted: "laplace64" (64 x 64 grid), "chain<n>" (tridiagonal: n levels of one row), "layered",
    "arrow700" (a dense row), "spd<n>" (a random pattern of n rows), "window<k>" (window_matrix)."""
    key = (factor, name)
    if key not in _SYSTEMS:
        if name == "laplace64":
            A = S.laplace2d(64)
        elif name.startswith("chain"):
            A = S.chain(int(name[5:]))
        elif name == "layered":
            A = IC.layered(LAYERS, seed=11) if factor == "ic0" else K.layered_nonsym(LAYERS, LAYERS_U, seed=11)
        elif name == "arrow700":
            A = S.arrow(700)
        elif name.startswith("spd"):
            A = IC.random_spd(int(name[3:]), 31) if factor == "ic0" else K.random_nonsym(int(name[3:]), 31)
        elif name.startswith("window"):
            A = window_matrix(factor, int(name[6:]))
        else:
            raise KeyError(name)
        _SYSTEMS[key] = tuple(np.ascontiguousarray(a) for a in A)
    return _SYSTEMS[key]


# rows at the edges of a workgroup of the k-wide sweep: one less, equal, one more (a partial last workgroup of one row)
EDGE_ROWS = sorted({mrows(k) + d for k in KS for d in (-1, 0, 1)})
SWEEP_SYSTEMS = (["laplace64", "chain3000", "layered", "arrow700", "chain1", "chain2", "chain3"]
                 + [f"spd{n}" for n in EDGE_ROWS] + [f"window{k}" for k in KS])


def level_widths(factor, rowptr, col, val):
    """(rows per forward level of lo, rows per backward level of up) from the checkers."""
    n = len(rowptr) - 1
    if factor == "ic0":
        fw, bw = IC.levels(n, rowptr, col)
    else:
        rows = [sorted(int(c) for c in col[rowptr[i]:rowptr[i + 1]]) for i in range(n)]
        Lc = [[c for c in r if c < i] for i, r in enumerate(rows)]
        Uc = [[c for c in r if c >= i] for i, r in enumerate(rows)]
        L = K._csr(Lc, [[0.0] * len(c) for c in Lc], False)
        U = K._csr(Uc, [[0.0] * len(c) for c in Uc], False)
        fw, bw = K.levels(n, L, U)
    return IC.widths(fw), IC.widths(bw)


# ------------------------------------------------------------------------------------------ drivers (GPU)
def build(api, factor, arrays):
    A = api.CsrMatrix.from_csr(*arrays)
    (A.build_ic0 if factor == "ic0" else A.build_ilu0)()
    return A


def set_sweeps(A, factor, s):
    (A.ic0_set_sweeps if factor == "ic0" else A.ilu0_set_sweeps)(s)


def info(A, factor):
    d = A.ic0_info() if factor == "ic0" else A.ilu0_info()
    return {"lo": d.get("levels_lower", d.get("levels_L")), "up": d.get("levels_upper", d.get("levels_U")), "bytes": d["bytes"],
            "launches": d["launches_per_apply"]}


def schedule_for_test(lib, A, factor, max_merged):
    fn = lib.lcg_hip_csr_ic0_schedule_for_test if factor == "ic0" else lib.lcg_hip_csr_ilu0_schedule_for_test
    assert fn(A.h, max_merged) == 0


def single(torch, A, factor, which, X):
    """The single-vector solve of every column of the (n, k) host block X: an (n, k) host block."""
    out = np.empty_like(X)
    solve = A.ic0_solve if factor == "ic0" else A.ilu0_solve
    for j in range(X.shape[1]):
        x = torch.from_numpy(np.ascontiguousarray(X[:, j])).cuda()
        y = torch.full_like(x, 7.0)
        solve(x, y, which)
        torch.cuda.synchronize()
        out[:, j] = y.cpu().numpy()
    return out


def batched(torch, A, factor, which, X):
    """The batched solve of the (n, k) host block X: an (n, k) host block."""
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    Yd = torch.full_like(Xd, 7.0)
    (A.ic0_solve_multi if factor == "ic0" else A.ilu0_solve_multi)(Xd, Yd, which)
    torch.cuda.synchronize()
    return Yd.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def multi_m(lib, api, precond, A, M, B, mem="device", **para):
    """One lcg_hip_lpcg_multi_m solve: (rc, ret[k], iterations[k], residual[k], M afterwards); M, B (n, k) numpy arrays."""
    import torch
    k = B.shape[1]
    p = api.lcg_default_parameters(**para)
    ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
    if mem == "device":
        Md, Bd = torch.from_numpy(M.copy()).cuda(), torch.from_numpy(np.ascontiguousarray(B)).cuda()
        rc = lib.lcg_hip_lpcg_multi_m(A.h, k, precond, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
        torch.cuda.synchronize()
        out = Md.cpu().numpy()
    else:
        raw = np.zeros(M.size + 2); off = 0 if raw.ctypes.data % 16 == 0 else 1
        out = raw[off:off + M.size].reshape(M.shape); out[:] = M
        rawb = np.zeros(B.size + 2); offb = 0 if rawb.ctypes.data % 16 == 0 else 1
        Bh = rawb[offb:offb + B.size].reshape(B.shape); Bh[:] = B
        rc = lib.lcg_hip_lpcg_multi_m(A.h, k, precond, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
    return rc, list(ret), list(its), list(res), out


# ------------------------------------------------------------------------------------------ the yardstick of the loop
_FACTOR = {}


def checker_apply(factor, key, n, rowptr, col, val, sweeps):
    """z = M^-1 r of the checkers for a system (cached under `key`): ic0_checker.IcApply / ic0_sweeps_checker.SweepApply on the
    checker's own IC(0) factor, ilu0_checker.IluApply / SweepApply on its ILU(0) factor."""
    if (factor, key) not in _FACTOR:
        if factor == "ic0":
            rp, cc, vv, zp = IC.ic0(n, rowptr, col, val)
            assert zp == -1
            _FACTOR[(factor, key)] = (rp, cc, vv)
        else:
            L, U, zp = K.ilu0(n, rowptr, col, val)
            assert zp == -1
            _FACTOR[(factor, key)] = (L, U)
    f = _FACTOR[(factor, key)]
    if factor == "ic0":
        if sweeps == 0:
            return IC.IcApply(IC.to_sparse(n, *f)).solve
        return S.SweepApply(n, f[0], f[1], f[2], sweeps).mx
    if sweeps == 0:
        return K.IluApply(n, *f).solve
    return K.SweepApply(n, f[0], f[1], sweeps).solve


_RUNS = {}


def checker_column(factor, key, system, sweeps, bcol, tag, eps, abs_diff, max_iterations=0):
    """ic0_checker.lpcg on one column alone with the matching apply: dict(x, iters, residual, ret).  Cached per system, factor,
    sweeps, `tag` (the caller's name of the column) and parameters."""
    ck = (factor, key, sweeps, tag, eps, abs_diff, max_iterations)
    if ck not in _RUNS:
        n, rp, ci, v = system
        As = IC.to_sparse(n, rp, ci, v)
        M = checker_apply(factor, key, n, rp, ci, v, sweeps)
        bcol = np.asarray(bcol, float)
        if not bcol.any():
            _RUNS[ck] = {"x": np.zeros(n), "iters": 0, "residual": 0.0, "ret": 2}
        else:
            last = {}

            def Mr(r):                                  # (the argument of the last apply IS the recurrence's residual vector)
                last["r"] = r
                return M(r)

            x, t = IC.lpcg(As, Mr, bcol, eps, abs_diff, max_iterations=max_iterations)
            r = last["r"]
            res = float(np.sqrt(r @ r) / n) if abs_diff else float((r @ r) / max(x @ x, 1.0))
            ret = (2 if t == 0 else 0) if res <= eps else -1019
            _RUNS[ck] = {"x": x, "iters": t, "residual": res, "ret": ret}
    return _RUNS[ck]
