"""ILU(0) beside IC(0) on one handle per system, in one process: what the factor costs to build and hold, what one
apply costs exact and by k = 2, 4, 8 sweeps, and whether right-preconditioned BiCGStab gains time on a non-symmetric system.

Systems: case_10K_A, the 5-point Laplacian 1000^2, the 7-point Laplacian 100^3, convdiff(1000, 2) (2-D convection-diffusion,
first-order upwinding: non-symmetric, no IC(0)), case_10K_cA (complex128).  Per system: levels, launches, build ms, bytes, and
the device time of one full apply (mean of 20 event-timed applies after a warm-up; an exact apply of more than 1500 levels: 5)
for ILU(0) and, where it exists, IC(0).  Three rounds, each round every leg of both factors in turn; medians.

The yardstick of the sweep kernels is IC(0)'s sweep apply on the same handle in the same run (code that was there before):
ILU(0)'s k-sweep apply moves no more bytes (U has L^T's entries on a symmetric pattern, L one entry per row fewer and no
division) and launches 2k - 1 kernels where IC(0) launches 2k, so it should not be slower than IC(0)'s by more than IC(0)'s own
spread over the rounds, (max - min) / median.  Both medians, the spread and the ratio are printed.

BiCGStab on convdiff(1000, 2) to eps = 1e-10 on r.r / max(m.m, 1) from m = 0, b = A x* (x* uniform in [1, 2]): plain, right
ILU(0) exact, k = 2, 4, 8; iterations and wall-clock ms around the solve (the final apply x = U^-1 L^-1 u included), medians of
the rounds after one untimed solve per leg.

    python scripts/ilu0_lab.py [--out profiles/ilu0_lab.txt] [--rounds 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KS = (2, 4, 8)


def convdiff(k, pe):
    import scipy.sparse as sp
    T1 = sp.diags([-1.0 - pe, 2.0 + pe, -1.0], [-1, 0, 1], shape=(k, k))
    T2 = sp.diags([-1.0 - pe / 2, 2.0 + pe / 2, -1.0], [-1, 0, 1], shape=(k, k))
    A = (sp.kron(sp.identity(k), T1) + sp.kron(T2, sp.identity(k))).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="a substring of the systems to run")
    ap.add_argument("--grid", type=int, default=1000, help="side of the 2-D grids (smaller: a rehearsal)")
    args = ap.parse_args()
    import torch
    from liblcg_amd import _lib, api
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    import ic0_lab as R
    lib = _lib.load()
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    api.use_torch_stream()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    g = args.grid
    g3 = max(4, round(g ** (2.0 / 3.0)))

    def systems():
        n, row, col, val, _ = read_coo_system(os.path.join(ROOT, "tests", "golden", "case_10K_A"))
        yield "case_10K_A", True, lambda: api.CsrMatrix.from_csr(*coo_to_csr_host(n, row, col, val))
        yield f"laplace2d {g}x{g}", True, lambda: api.CsrMatrix.laplace2d(g, g)
        yield f"laplace3d {g3}^3", True, lambda: api.CsrMatrix.from_csr(*R.laplace3d(g3))
        yield f"convdiff({g}, 2)", False, lambda: api.CsrMatrix.from_csr(*convdiff(g, 2))
        nc, rowc, colc, valc, _ = read_coo_system(os.path.join(ROOT, "tests", "golden", "case_10K_cA"), True)
        yield "case_10K_cA", True, lambda: api.CsrMatrix.from_csr(*coo_to_csr_host(nc, rowc, colc, valc))

    say(f"ilu0_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    say(f"apply: mean of 20 full applies between events after one warm-up (exact apply of more than 1500 levels: 5); medians of "
        f"{args.rounds} rounds; spread = (max - min) / median over the rounds")
    say()
    for name, has_ic, make in systems():
        if args.only and args.only not in name:
            continue
        A = make()
        n = A.n
        A.build_ilu0()
        facs = [("ILU(0)", A.ilu0_info, A.ilu0_set_sweeps, A.ilu0_solve, "levels_L", "levels_U")]
        if has_ic:
            A.build_ic0()
            facs.append(("IC(0)", A.ic0_info, A.ic0_set_sweeps, A.ic0_solve, "levels_lower", "levels_upper"))
        dt = torch.complex128 if A.is_complex else torch.float64
        x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n)).to(dt).cuda()
        y = torch.empty_like(x)
        legs = [("exact", 0)] + [(f"k={k}", k) for k in KS]
        res = {(f[0], leg): {"us": [], "launches": 0} for f in facs for leg, _ in legs}
        infos = {f[0]: f[1]() for f in facs}
        for _ in range(args.rounds):
            for leg, k in legs:
                for fname, info, set_sweeps, solve, ll, lu in facs:
                    set_sweeps(k)
                    i = info()
                    res[(fname, leg)]["launches"] = i["launches_per_apply"]
                    reps = 5 if k == 0 and max(i[ll], i[lu]) > 1500 else 20
                    solve(x, y)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(reps):
                        solve(x, y)
                    e1.record()
                    torch.cuda.synchronize()
                    res[(fname, leg)]["us"].append(e0.elapsed_time(e1) * 1e3 / reps)
        for f in facs:
            f[2](0)
        say(f"{name} ({'c128' if A.is_complex else 'f64'}): {n} rows, {A.nnz} entries")
        for fname, _, _, _, ll, lu in facs:
            i = infos[fname]
            say(f"  {fname:<7} levels {i[ll]} / {i[lu]}, build {i['build_ms']:.1f} ms, {i['bytes'] / 2 ** 20:.2f} MiB")
        say(f"  {'factor':<7} {'apply':<6} {'launch':>6} {'apply us':>11} {'spread':>7}   apply us by round")
        med = {}
        for fname, *_ in facs:
            for leg, _ in legs:
                r = res[(fname, leg)]
                m = float(np.median(r["us"]))
                med[(fname, leg)] = (m, (max(r["us"]) - min(r["us"])) / m)
                say(f"  {fname:<7} {leg:<6} {r['launches']:>6} {m:>11.1f} {med[(fname, leg)][1]:>7.3f}   {' '.join(f'{q:.1f}' for q in r['us'])}")
        if has_ic:
            for leg, k in legs:
                if not k:
                    continue
                (mi, _), (mc, sc) = med[("ILU(0)", leg)], med[("IC(0)", leg)]
                ratio = mi / mc
                say(f"  sweeps {leg}: ILU(0) {mi:.1f} us, IC(0) {mc:.1f} us, ratio {ratio:.3f}, IC(0)'s spread {sc:.3f}: "
                    f"{'within' if ratio <= 1.0 + sc else 'OUTSIDE'} the margin")
        if not has_ic:
            import scipy.sparse as sp
            rp, ci, v = A.arrays_to_host()
            As = sp.csr_matrix((v, ci, rp), shape=(n, n))
            xs = np.random.default_rng(3).uniform(1.0, 2.0, n)
            bh = As @ xs
            b = torch.from_numpy(bh).cuda()
            para = api.lcg_default_parameters(epsilon=1e-10, max_iterations=20000)
            runs = [("plain", None)] + legs
            out = {leg: {"its": [], "ms": [], "res": 0.0} for leg, _ in runs}

            def solve(k):
                u = torch.zeros_like(b)
                xx = u
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if k is None:
                    r = api.lcg_solver("lcg_hip_csr_ax", None, u, b, n, para, A, api.LCG_BICGSTAB)
                else:
                    r = api.lcg_solver("lcg_hip_csr_ax_ilu0", None, u, b, n, para, A, api.LCG_BICGSTAB)
                    xx = torch.empty_like(u)
                    A.ilu0_solve(u, xx, 2)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                return (r.iterations if r.ret == 0 else -r.iterations), ms, float(np.linalg.norm(bh - As @ xx.cpu().numpy()) / np.linalg.norm(bh))

            for rnd in range(args.rounds):
                for leg, k in runs:
                    if k is not None:
                        A.ilu0_set_sweeps(k)
                    if rnd == 0:
                        solve(k)                        # the first solve of a leg: pool vectors, code objects
                    its, ms, rr = solve(k)
                    out[leg]["its"].append(its); out[leg]["ms"].append(ms); out[leg]["res"] = rr
            A.ilu0_set_sweeps(0)
            say(f"  BiCGStab to eps = 1e-10 from m = 0 ({'right ILU(0): Afp = lcg_hip_csr_ax_ilu0, then x = U^-1 L^-1 u'}):")
            say(f"  {'apply':<6} {'its':>6} {'ms':>10} {'ms / it':>9} {'|b-Ax|/|b|':>11}   ms by round")
            best = None
            for leg, _ in runs:
                o = out[leg]
                its, ms = int(np.median(o["its"])), float(np.median(o["ms"]))
                say(f"  {leg:<6} {its:>6} {ms:>10.2f} {ms / max(abs(its), 1):>9.4f} {o['res']:>11.2e}   {' '.join(f'{q:.2f}' for q in o['ms'])}")
                if its > 0 and (best is None or ms < best[1]):
                    best = (leg, ms)
            plain_ms = float(np.median(out["plain"]["ms"]))
            say(f"  fastest: {best[0]} ({best[1]:.2f} ms; plain {plain_ms:.2f} ms)" + ("" if best[0] != "plain" else ": no ILU(0) setting gains time here"))
        say()
        A.destroy()
        lib.lcg_hip_trim()
    say("(an iteration count shown negative stopped at the cap without converging)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
