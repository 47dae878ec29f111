"""Systems, loops and oracle drivers shared by tests/test_gpu_stop_contract.py and tests/test_stop_contract_cpu.py.

The stop contract of a solver loop (lcg.cpp:206-230, clcg.cpp's twins): the progress callback is handed the live iterate with
k = 0 ... t before every iteration; the iterate it sees at k = K is the iterate a run capped at K returns; a non-zero return at K
ends the solve with that iterate.  The device loops enqueue ahead of the stop test, so the same must hold there bit for bit,
whichever way the loop is driven (tests/test_gpu_stop_contract.py); the CPU module shows that the contract is the reference's.

Systems: banded, diagonally dominant, offsets +-1 and +-37, a diagonal that varies by a factor of about three along the rows:
an SPD one, a non-symmetric twin (the same diagonal, other off-diagonal weights) and a complex symmetric one, S + i D with D a
positive diagonal -- x^H A x has a positive imaginary part for every x, so every eigenvalue lies off the real axis.

Sizes: 65 (one wavefront + 1) and 513 (odd, two workgroups of pairs) for every loop; the large ones lie just beyond ONE stride
of a vector pass, odd, so that a pass walks a second stride and the scalar tail of the two-wide passes runs:
  * fp64: k_vec<Op, true> takes two reals per lane, VB = 256 lanes, at most 512 workgroups: 2 * 256 * 512 = 262144 -> 262147;
  * complex128: one 16-byte element per lane: 256 * 512 = 131072 -> 131075;
  * complex64 (solvers_c64.hip): its Driver is built with cplx = true, so its passes are k_vec<Op, false> as well -- ONE float2
    element per lane and grid_for(n) workgroups: the stride is again 256 * 512 = 131072 elements (of 8 bytes) -> 131075.

CG schedules: CG_AUTO takes the one-reduction arrangement below 2^20 rows (solvers_real.hip: CG1_AUTO_ROWS), so at all three
sizes the AUTO cases walk the one-reduction loop through the automatic choice; the classic loop is reached by CG_CLASSIC, which
is why CG, PCG + Jacobi and lcg() with caller workspaces are each run under both.
"""
import ctypes as C

import numpy as np

from oracle import pyoracle as po

SIZES = {"real": (65, 513, 262147), "c128": (65, 513, 131075), "c64": (65, 513, 131075)}
OFFSETS = (1, 37)
ITER_WINDOW = (8, 200)

# ---------------------------------------------------------------------------------------------------------------- systems
def _diag_profile(n):
    i = np.arange(n, dtype=np.float64)
    return 1.0 + 1.0 * (1.0 + np.sin(0.37 * i + 0.2))        # 1 ... 3 along the rows


def system(kind, n):
    """kind: 'spd', 'nonsym', 'csym' (complex128) or 'csym64' (the complex one rounded to complex64).
    Returns dict(n, rp, ci, v, xt, b) with b = A.xt (row by row, in the working precision's exact sums)."""
    cplx = kind.startswith("csym")
    w = {"spd": ((-1.0, -1.0), (-0.5, -0.5)), "nonsym": ((-0.7, -1.3), (-0.8, -0.2))}.get(kind, ((-1.0, -1.0), (-0.5, -0.5)))
    idx = np.arange(n, dtype=np.int64)
    rows, cols, vals = [], [], []
    for (lo, up), off in zip(w, OFFSETS):
        ok = idx >= off
        rows.append(idx[ok]); cols.append(idx[ok] - off); vals.append(np.full(int(ok.sum()), lo))
        ok = idx + off < n
        rows.append(idx[ok]); cols.append(idx[ok] + off); vals.append(np.full(int(ok.sum()), up))
    diag = 3.3 * _diag_profile(n)                               # sum |off-diagonal| = 3 in every full row
    if cplx:
        diag = diag + 1j * (0.6 + 0.3 * np.cos(0.11 * idx))
    rows.append(idx); cols.append(idx); vals.append(diag)
    row = np.concatenate(rows); col = np.concatenate(cols)
    val = np.concatenate([np.asarray(x, np.complex128 if cplx else np.float64) for x in vals])
    order = np.lexsort((col, row))
    row, col, val = row[order], col[order].astype(np.int32), val[order]
    rp = np.zeros(n + 1, np.int64); np.add.at(rp, row + 1, 1); rp = np.cumsum(rp).astype(np.int32)
    xt = np.sin(0.7 * idx) + 0.3 * np.cos(0.013 * idx)
    if cplx:
        xt = xt + 1j * np.cos(0.45 * idx + 0.1)
    if kind == "csym64":
        val = val.astype(np.complex64); xt = xt.astype(np.complex64)
    b = _matvec(rp, col, val, xt)
    if kind == "csym64":
        b = b.astype(np.complex64)
    return {"kind": kind, "n": n, "rp": rp, "ci": col, "v": val, "xt": xt, "b": b}


def _matvec(rp, ci, v, x):
    n = len(rp) - 1
    y = np.zeros(n, np.complex128 if np.iscomplexobj(v) else np.float64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    np.add.at(y, rows, v.astype(y.dtype) * x.astype(y.dtype)[ci])
    return y


def box(S):
    """Bounds that are active for some components and let the loops meet their stop rule all the same (the rule looks at the
    WHOLE gradient, lcg.cpp:1098-1110, which does not vanish at a bound that cuts the solution off): every fifth component's
    upper bound is the solution's own value there, so the iterate is clamped to it whenever it arrives from above; all other
    bounds lie outside the solution's range."""
    n, xt = S["n"], S["xt"]
    low = np.full(n, -4.0)
    hig = np.full(n, 4.0)
    hig[::5] = xt[::5]
    return low, hig


# ------------------------------------------------------------------------------------------------------------------ loops
class Loop:
    """name; family 'real' | 'c128' | 'c64'; system kind; the oracle's loop (`oracle`); how the device is asked (`entry`,
    `sid`, `schedule`, `mfp`, ...); eps / abs_diff; wide: CGS / BiCGStab-type recurrences (conftest.check_converged_run);
    late: the recurrence IS the oracle's (classic CG / PCG); small: smallest size only."""
    def __init__(self, name, family, kind, oracle, entry, sid=None, schedule=None, mfp=None, eps=1e-10, abs_diff=1, wide=False, late=False,
                 small=False, factor=None, sweeps=0, afp=None, shadow=False):
        self.name, self.family, self.kind, self.oracle, self.entry = name, family, kind, oracle, entry
        self.sid, self.schedule, self.mfp, self.afp = sid, schedule, mfp, afp
        self.eps, self.abs_diff, self.wide, self.late, self.small = eps, abs_diff, wide, late, small
        self.factor, self.sweeps, self.shadow = factor, sweeps, shadow

    def sizes(self):
        return SIZES[self.family][:1] if self.small else SIZES[self.family]

    def __repr__(self):
        return self.name


CG_AUTO, CG_CLASSIC, CG_ONE_REDUCTION = 0, 1, 2
LOOPS = [
    Loop("cg_auto", "real", "spd", "cg", "solver", sid=0, schedule=CG_AUTO),
    Loop("cg_classic", "real", "spd", "cg", "solver", sid=0, schedule=CG_CLASSIC, late=True),
    Loop("cg_one_reduction", "real", "spd", "cg", "solver", sid=0, schedule=CG_ONE_REDUCTION),
    Loop("pcg_jacobi_auto", "real", "spd", "pcg", "pre", mfp="lcg_hip_jacobi_mx", schedule=CG_AUTO),
    Loop("pcg_jacobi_classic", "real", "spd", "pcg", "pre", mfp="lcg_hip_jacobi_mx", schedule=CG_CLASSIC, late=True),
    Loop("cgs", "real", "nonsym", "cgs", "solver", sid=2, wide=True),
    Loop("bicgstab", "real", "nonsym", "bicgstab", "solver", sid=3, wide=True),
    Loop("bicgstab2", "real", "nonsym", "bicgstab2", "solver", sid=4, wide=True),
    Loop("pg", "real", "spd", "pg", "box", sid=5, wide=True),
    Loop("spg", "real", "spd", "spg", "box", sid=6, wide=True),
    Loop("lcg_workspaces", "real", "spd", "cg", "lcg", schedule=CG_AUTO),
    Loop("lcg_workspaces_classic", "real", "spd", "cg", "lcg", schedule=CG_CLASSIC, late=True),
    Loop("lcgs_workspaces", "real", "nonsym", "cgs", "lcgs", wide=True),
    # the triangular factors and the dense callback: the smallest size only.  eps = 1e-13 for PCG: at 1e-10 the exact factors end
    # the oracle's run after 7 iterations, short of the window.  On these bands ILU(0) applied exactly is nearly A^-1 (BiCGStab on
    # the right-preconditioned operator: 4 iterations at 1e-10, 5-6 on harder twins with weaker diagonals and heavier +-37 bands),
    # so that loop runs with the factor applied by ONE sweep per triangle: 12 iterations.
    Loop("pcg_ic0_exact", "real", "spd", "pcg_factor", "pre", mfp="lcg_hip_ic0_mx", factor="ic0", sweeps=0, eps=1e-13, small=True),
    Loop("pcg_ic0_sweeps2", "real", "spd", "pcg_factor", "pre", mfp="lcg_hip_ic0_mx", factor="ic0", sweeps=2, eps=1e-13, small=True),
    Loop("pcg_ilu0_exact", "real", "spd", "pcg_factor", "pre", mfp="lcg_hip_ilu0_mx", factor="ilu0", sweeps=0, eps=1e-13, small=True),
    Loop("pcg_ilu0_sweeps2", "real", "spd", "pcg_factor", "pre", mfp="lcg_hip_ilu0_mx", factor="ilu0", sweeps=2, eps=1e-13, small=True),
    Loop("bicgstab_right_ilu0_sweeps1", "real", "nonsym", "bicgstab_right", "solver", sid=3, afp="lcg_hip_csr_ax_ilu0", factor="ilu0", sweeps=1,
         wide=True, small=True),
    Loop("cg_dense_ata", "real", "spd", "cg_dense", "dense", sid=0, schedule=CG_AUTO, small=True),
    Loop("c_bicg", "c128", "csym", "c_bicg", "csolver", sid=0, wide=True),
    Loop("c_bicg_sym", "c128", "csym", "c_bicg_sym", "csolver", sid=1, wide=True),
    Loop("c_cgs", "c128", "csym", "c_cgs", "csolver", sid=2, wide=True, shadow=True),
    Loop("c_bicgstab", "c128", "csym", "c_bicgstab", "csolver", sid=3, wide=True, shadow=True),
    Loop("c_tfqmr", "c128", "csym", "c_tfqmr", "csolver", sid=4, wide=True, shadow=True),
    Loop("c_pcg_jacobi", "c128", "csym", "c_pcg", "cpre", sid=5, mfp="clcg_hip_jacobi_mx", wide=True),
    Loop("c_pbicg_jacobi", "c128", "csym", "c_pbicg", "cpre", sid=6, mfp="clcg_hip_jacobi_mx", wide=True),
    Loop("c64_bicg", "c64", "csym64", "c64_bicg", "c64solver", sid=0, eps=1e-10, abs_diff=0, wide=True),
    Loop("c64_bicg_sym", "c64", "csym64", "c64_bicg_sym", "c64solver", sid=1, eps=1e-10, abs_diff=0, wide=True),
    Loop("c64_pcg_jacobi", "c64", "csym64", "c64_pcg", "c64pre", sid=5, mfp="clcg_hip_jacobi_mx_c64", eps=1e-10, abs_diff=0, wide=True),
]
BY_NAME = {L.name: L for L in LOOPS}
CASES = [(L, n) for L in LOOPS for n in L.sizes()]
CASE_IDS = [f"{L.name}-{n}" for L, n in CASES]
SHADOW_SEED = 7


def rhs_with_nan(S, where, L=None):
    b = (S["b"] if L is None else rhs_of(L, S)).copy()
    n = S["n"]
    b[{"first": 0, "last": n - 1, "mid": n // 2}[where]] = np.nan
    return b


# ------------------------------------------------------------------------------------------------------------ the oracle
_VP = C.c_void_p
_PROG = C.CFUNCTYPE(C.c_int, _VP, _VP, C.c_double, _VP, C.c_int, C.c_int)
_CAX = C.CFUNCTYPE(None, _VP, _VP, _VP, C.c_int, C.c_int, C.c_int)
_NAN_CODES = (-1017, -1019)


def _p(a):
    return a.ctypes.data_as(_VP)


def oracle_run(port, L, S, b=None, cap=0, on_progress=None):
    """One run of the oracle's loop for L on system S.  on_progress(k, m_copy, residual) -> non-zero stops (None: never).
    Returns dict(ret, iters, x, residual, ks, clamped): ks the k of every callback call; iters the loop's own t -- the last k
    handed over, + 1 where the loop left through its NaN scan (the iteration that found it: no callback call follows)."""
    if L.family == "c64":
        return _c64_oracle(L, S, b, cap, on_progress)
    cplx = L.family == "c128"
    n = S["n"]
    b = np.ascontiguousarray(rhs_of(L, S) if b is None else b)
    m = np.zeros(n, np.complex128 if cplx else np.float64)
    ks, last = [], [0.0]

    def cb(inst, mp, res, para, nn, k):
        ks.append(k); last[0] = res
        if on_progress is None:
            return 0
        x = np.ctypeslib.as_array((C.c_double * ((2 if cplx else 1) * n)).from_address(mp)).copy()
        return int(on_progress(k, x.view(np.complex128) if cplx else x, res))
    prog = _PROG(cb)
    lib = port.lib
    invdiag = None
    if L.oracle in ("pcg", "c_pcg", "c_pbicg"):
        invdiag = 1.0 / port.csr_diag(S["rp"], S["ci"], S["v"])
    inst, keep = port._inst(S["rp"], S["ci"], np.asarray(S["v"], np.complex128 if cplx else np.float64), None if cplx else invdiag, 1)
    if cplx:
        para = po.default_cpara(epsilon=L.eps, abs_diff=L.abs_diff, max_iterations=cap)
        args = (_p(m), _p(b), C.c_int(n), C.byref(para), C.byref(inst))
        ax = lib.orc_csr_cax
        if L.oracle in ("c_pcg", "c_pbicg"):
            inv = np.ascontiguousarray(invdiag, np.complex128)

            def mx(i_, xp, yp, nn, lay, cj):        # the complex Jacobi of orc_csolve_csr_pcg (csr_oracle.c: orc_cjacobi_mx)
                x = np.ctypeslib.as_array((C.c_double * (2 * n)).from_address(xp)).view(np.complex128)
                y = np.ctypeslib.as_array((C.c_double * (2 * n)).from_address(yp)).view(np.complex128)
                y[:] = inv * x
            mxc = _CAX(mx)
            f = lib.orc_clpcg if L.oracle == "c_pcg" else lib.orc_clpbicg
            f.restype = C.c_int
            ret = f(ax, mxc, prog, *args)
        elif L.oracle in ("c_bicg", "c_bicg_sym"):
            f = lib.orc_clbicg if L.oracle == "c_bicg" else lib.orc_clbicg_symmetric
            f.restype = C.c_int
            ret = f(ax, prog, *args)
        else:
            rb = np.ascontiguousarray(port.vecrnd(n, SHADOW_SEED))
            f = {"c_cgs": lib.orc_clcgs, "c_bicgstab": lib.orc_clbicgstab, "c_tfqmr": lib.orc_cltfqmr}[L.oracle]
            f.restype = C.c_int
            ret = f(ax, prog, *args, _p(rb))
    else:
        para = po.default_para(epsilon=L.eps, abs_diff=L.abs_diff, max_iterations=cap)
        args = (_p(m), _p(b), C.c_int(n), C.byref(para), C.byref(inst))
        if L.oracle == "pcg":
            lib.orc_lpcg.restype = C.c_int
            ret = lib.orc_lpcg(lib.orc_csr_ax, lib.orc_jacobi_mx, prog, *args)
        elif L.oracle == "pcg_factor":
            mx = _as_callback(factor_apply(L, S), n)
            lib.orc_lpcg.restype = C.c_int
            ret = lib.orc_lpcg(lib.orc_csr_ax, mx, prog, *args)
        elif L.oracle == "bicgstab_right":      # A.M^-1 u = b for u (the loop's iterate), lcg_hip_csr_ax_ilu0's operator
            apply = factor_apply(L, S)
            ax = _as_callback(lambda x: port.csr_matvec(S["rp"], S["ci"], S["v"], apply(x)), n)
            lib.orc_lbicgstab.restype = C.c_int
            ret = lib.orc_lbicgstab(ax, prog, *args)
        elif L.oracle == "cg_dense":
            import dense_checker as D
            K = dense_of(S)
            ax = _as_callback(lambda x: D.ata(K, x), n)
            lib.orc_lcg.restype = C.c_int
            ret = lib.orc_lcg(ax, prog, *args)
        elif L.oracle in ("pg", "spg"):
            low, hig = box(S)
            lib.orc_lcg_solver_constrained.restype = C.c_int
            ret = lib.orc_lcg_solver_constrained(lib.orc_csr_ax, prog, _p(m), _p(b), _p(low), _p(hig), C.c_int(n), C.byref(para), C.byref(inst),
                                                 C.c_int(6 if L.oracle == "spg" else 5))
        else:
            lib.orc_lcg_solver.restype = C.c_int
            ret = lib.orc_lcg_solver(lib.orc_csr_ax, prog, *args, C.c_int({"cg": 0, "cgs": 2, "bicgstab": 3, "bicgstab2": 4}[L.oracle]))
    iters = (ks[-1] if ks else 0) + (1 if ret in _NAN_CODES and ks and not _ended_at_head(ret, cplx, cap, ks) else 0)
    return {"ret": ret, "iters": iters, "x": m, "residual": last[0], "ks": ks}


def _ended_at_head(ret, cplx, cap, ks):
    """-1019 is the complex enum's NaN code AND the cap code the complex loops hand back (clcg.cpp:126,164): a run that left at
    the loop's head, through the cap, made its last callback call with k = cap."""
    return ret == -1019 and cap > 0 and ks[-1] == cap


def _c64_oracle(L, S, b, cap, on_progress):
    import c64_checker as K
    n = S["n"]
    b = S["b"] if b is None else b
    ops = K.csr_ops(S["rp"], S["ci"], S["v"], np.complex64)
    para = {"epsilon": L.eps, "abs_diff": L.abs_diff, "max_iterations": cap}
    ks, last = [], [0.0]

    def prog(m, res, k):
        ks.append(k); last[0] = float(res)
        return 0 if on_progress is None else int(on_progress(k, np.array(m, np.complex64), float(res)))
    m0 = np.zeros(n, np.complex64)
    if L.oracle == "c64_bicg":
        r = K.bicg(ops["A"], ops["AH"], b, m0, para, progress=prog)
    elif L.oracle == "c64_bicg_sym":
        r = K.bicg_sym(ops["A"], b, m0, para, progress=prog)
    else:
        r = K.pcg(ops["A"], _c64_jacobi(S), b, m0, para, progress=prog)
    return {"ret": r["ret"], "iters": r["iters"], "x": r["x"], "residual": r["residual"], "ks": ks}


def _c64_jacobi(S, dtype=np.complex64):
    """c64_checker.jacobi without its Python loop over the rows (the diagonal of these systems is each row's entry col == row)."""
    import c64_checker as K
    P = K.Prec(dtype)
    rows = np.repeat(np.arange(S["n"]), np.diff(S["rp"]))
    d = np.asarray(S["v"], dtype)[S["ci"] == rows]
    inv = np.array([P.div(P.C(1.0), P.C(x)) for x in d], dtype)
    return lambda x: (inv * np.asarray(x, dtype)).astype(dtype)


_AX = C.CFUNCTYPE(None, _VP, _VP, _VP, C.c_int)


def _as_callback(f, n):
    """A numpy function x -> y as the oracle's lcg_axfunc_ptr."""
    def cb(inst, xp, yp, nn):
        x = np.ctypeslib.as_array((C.c_double * n).from_address(xp))
        np.ctypeslib.as_array((C.c_double * n).from_address(yp))[:] = f(x.copy())
    return _AX(cb)


def factor_apply(L, S):
    """z = M^-1 x as the tests' checkers apply the factor L asks for: exactly (row-ordered solves) or by L.sweeps Jacobi sweeps
    per triangle (ic0_sweeps_checker.SweepApply / ilu0_checker.SweepApply)."""
    if "apply" not in S or S["apply"][0] != (L.factor, L.sweeps):
        n = S["n"]
        if L.factor == "ic0":
            import ic0_sweeps_checker as SW
            _, rp, cc, vv = SW.factor(S["rp"], S["ci"], S["v"])
            f = SW.SweepApply(n, rp, cc, vv, L.sweeps).mx
        else:
            import ilu0_checker as I
            Lf, Uf, zp = I.ilu0(n, S["rp"], S["ci"], S["v"])
            assert zp == -1
            f = I.SweepApply(n, Lf, Uf, L.sweeps).solve
        S["apply"] = ((L.factor, L.sweeps), f)
    return S["apply"][1]


def dense_of(S):
    K = np.zeros((S["n"], S["n"]))
    rows = np.repeat(np.arange(S["n"]), np.diff(S["rp"]))
    K[rows, S["ci"]] = S["v"]
    return K


def rhs_of(L, S):
    """The right-hand side L's solve takes: A.xt -- of the operator the loop really inverts (K^T.K for the dense callback)."""
    if L.oracle == "cg_dense":
        import dense_checker as D
        return D.ata(dense_of(S), S["xt"])
    return S["b"]


class AsPort:
    """What conftest.check_converged_run asks of `port` -- solve(sid, rp, ci, v, b, para=, jacobi=) -> dict(ret, iters, x) -- answered
    by the oracle's loop for L, whichever entry it lives behind: the function serves every loop unchanged."""
    def __init__(self, port, L, S):
        self.port, self.L, self.S = port, L, S

    def solve(self, sid, rp, ci, v, b, para=None, jacobi=False):
        b = np.asarray(b)
        if self.L.family == "c64":
            b = b.astype(np.complex64)
        return oracle_run(self.port, self.L, self.S, b=b, cap=para.max_iterations)


def pick_ks(last):
    """K = 1, 3, the last iteration but one, the last -- in a loop that takes `last` iterations."""
    return sorted({k for k in (1, 3, last - 1, last) if 1 <= k <= last})
