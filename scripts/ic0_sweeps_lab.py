"""IC(0) applied by Jacobi sweeps against the exact level-scheduled apply and against Jacobi, in one process on one
handle per system: the four real systems of scripts/ic0_lab.py (PCG to eps = 1e-8 on r.r / max(m.m, 1)) and the three complex
ones of scripts/ic0_c64_lab.py in complex128 and complex64 (eps = 1e-6, sample14's rule), all from m = 0.

Per system and per apply -- exact, k = 1, 2, 3, 4, 6, 8 sweeps per triangle -- the device time of one full apply (mean of 20
event-timed applies after a warm-up), PCG iterations and wall-clock milliseconds around the solve; Jacobi beside them.  Three
rounds, every round exact, then the sweeps, then Jacobi; medians.

The sweep kernel's rate: one more sweep per triangle adds one k_ic_sweep launch on L and one on L^T, so the time of such a
pair is the slope (apply(k = 8) - apply(k = 2)) / 6, launch gaps included.  Its bytes are the algorithm's: both triangles'
entries (4-byte column + value), both row pointer arrays, and three vectors per launch (x read, y(j) gathered, y(j+1) written).
The box's own copy rate is taken as bench.py --full takes it (1 GiB read + 1 GiB written, 10 copies after 3).  A system whose
factor and vectors fit the 256 MiB Infinity Cache is served from it: its rate is not a fraction of HBM bandwidth.

    python scripts/ic0_sweeps_lab.py [--out profiles/ic0_sweeps_lab.txt] [--rounds 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KS = (1, 2, 3, 4, 6, 8)
CAP = {"f64": 20000, "c128": 5000, "c64": 5000}
EPS = {"f64": 1e-8, "c128": 1e-6, "c64": 1e-6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="a substring of the systems to run")
    args = ap.parse_args()
    import torch
    from liblcg_amd import _lib, api
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    import ic0_c64_lab as C64
    import ic0_lab as R
    lib = _lib.load()
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    api.use_torch_stream()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def real_systems():
        n, row, col, val, b = read_coo_system(os.path.join(ROOT, "tests", "golden", "case_10K_A"))
        yield "case_10K_A", lambda: api.CsrMatrix.from_csr(*coo_to_csr_host(n, row, col, val)), b
        yield "laplace2d 1000x1000", lambda: api.CsrMatrix.laplace2d(1000, 1000), np.ones(1000000)
        yield "laplace3d 100^3", lambda: api.CsrMatrix.from_csr(*R.laplace3d(100)), np.ones(1000000)
        yield "tridiagonal 1e6", lambda: api.CsrMatrix.from_csr(*R.tridiag(1000000)), np.ones(1000000)

    def systems():
        for name, make, b in real_systems():
            yield name, "f64", make, b
        for name, get in (("case_1K_cA", lambda: C64.case("1K")), ("case_10K_cA", lambda: C64.case("10K")),
                          ("helmholtz 600^2", lambda: C64.helmholtz(600))):
            rp, ci, v, b = get()
            yield name, "c128", lambda: api.CsrMatrix.from_csr(rp, ci, v.astype(np.complex128)), b
            yield name, "c64", lambda: api.CsrMatrix.from_csr_c64(rp, ci, v.astype(np.complex64)), b

    # the box's own copy rate, as bench.py --full takes it
    src = torch.empty(1 << 27, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        dst.copy_(src)
    torch.cuda.synchronize()
    copy_gbs = 10 * 2 * src.numel() * 8 / (time.perf_counter() - t0) / 1e9
    del src, dst
    torch.cuda.empty_cache()

    say(f"ic0_sweeps_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    say(f"apply: mean of 20 full applies between events after one warm-up (exact apply of more than 100000 levels: 3); PCG from m = 0, "
        f"abs_diff 0, eps 1e-8 (f64, cap {CAP['f64']}) or 1e-6 (complex, cap {CAP['c128']}), wall clock around the solve; medians of "
        f"{args.rounds} rounds, each round exact, k = {', '.join(map(str, KS))}, Jacobi")
    say(f"device copy rate of this box (1 GiB read + 1 GiB written): {copy_gbs:.0f} GB/s")
    say()
    dt = {"f64": torch.float64, "c128": torch.complex128, "c64": torch.complex64}
    vw = {"f64": 8, "c128": 16, "c64": 8}
    summary = []
    for name, kind, make, bh in systems():
        if args.only and args.only not in name:
            continue
        A = make()
        n = A.n
        A.build_ic0()
        A.build_jacobi()
        info0 = A.ic0_info()
        nnzL = len(A.ic0_factor_to_host()[1])
        b = torch.from_numpy(np.ascontiguousarray(bh)).to(dt[kind]).cuda()
        x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n)).to(dt[kind]).cuda()
        y = torch.empty_like(x)
        legs = [("exact", 0)] + [(f"k={k}", k) for k in KS] + [("Jacobi", None)]
        res = {leg: {"apply": [], "its": [], "ms": [], "launches": 0, "mib": 0.0} for leg, _ in legs}

        def solve(ic):
            m = torch.zeros_like(b)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "f64":
                para = api.lcg_default_parameters(epsilon=EPS[kind], abs_diff=0, max_iterations=CAP[kind])
                r = api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx" if ic else "lcg_hip_jacobi_mx", None, m, b, n, para, A)
            else:
                para = api.clcg_default_parameters(epsilon=EPS[kind], abs_diff=0, max_iterations=CAP[kind])
                if kind == "c128":
                    r = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ic0_mx" if ic else "clcg_hip_jacobi_mx", None, m, b, n,
                                                       para, A)
                else:
                    r = api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_ic0_mx_c64" if ic else
                                                           "clcg_hip_jacobi_mx_c64", None, m, b, n, para, A)
            torch.cuda.synchronize()
            return (r.iterations if r.ret == 0 else -r.iterations), (time.perf_counter() - t0) * 1e3

        for rnd in range(args.rounds):
            for leg, k in legs:
                if k is not None:
                    A.ic0_set_sweeps(k)
                    info = A.ic0_info()
                    res[leg]["launches"], res[leg]["mib"] = info["launches_per_apply"], info["bytes"] / 2 ** 20
                    reps = 3 if k == 0 and info0["levels_lower"] > 100000 else 20
                    A.ic0_solve(x, y)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(reps):
                        A.ic0_solve(x, y)
                    e1.record()
                    torch.cuda.synchronize()
                    res[leg]["apply"].append(e0.elapsed_time(e1) * 1e3 / reps)
                if rnd == 0:
                    solve(k is not None)                 # the first solve of a leg: pool vectors, code objects
                its, ms = solve(k is not None)
                res[leg]["its"].append(its)
                res[leg]["ms"].append(ms)
        A.ic0_set_sweeps(0)
        say(f"{name} ({kind}): {n} rows, L {nnzL} entries, levels {info0['levels_lower']} / {info0['levels_upper']}, "
            f"build {info0['build_ms']:.1f} ms")
        say(f"  {'apply':<7} {'launch':>6} {'MiB':>8} {'apply us':>11} {'PCG its':>8} {'PCG ms':>10} {'ms / it':>9}   apply us by round | PCG ms by round")
        med = {}
        for leg, k in legs:
            r = res[leg]
            med[leg] = (float(np.median(r["apply"])) if r["apply"] else float("nan"), int(np.median(r["its"])), float(np.median(r["ms"])))
            a, its, ms = med[leg]
            say(f"  {leg:<7} {r['launches'] if k is not None else 0:>6} {r['mib']:>8.2f} {a:>11.1f} {its:>8} {ms:>10.2f} "
                f"{ms / max(abs(its), 1):>9.4f}   {' '.join(f'{q:.1f}' for q in r['apply'])} | {' '.join(f'{q:.2f}' for q in r['ms'])}")
        # the sweep kernel's rate from the slope between k = 2 and k = 8
        pair_us = (med["k=8"][0] - med["k=2"][0]) / 6.0
        pair_bytes = 2 * (nnzL * (4 + vw[kind]) + 4 * (n + 1) + 3 * vw[kind] * n)
        foot = pair_bytes / 2 ** 20
        say(f"  one sweep on L + one on L^T: {pair_us:.2f} us (slope k = 2 .. 8), {pair_bytes / 1e6:.1f} MB by the algorithm's count: "
            f"{pair_bytes / max(pair_us, 1e-9) / 1e3:.0f} GB/s, {pair_bytes / max(pair_us, 1e-9) / 1e3 / copy_gbs:.2f} of the copy rate "
            f"({'fits' if foot + info0['bytes'] / 2 ** 20 < 256 else 'exceeds'} the Infinity Cache)")
        best = min((leg for leg, k in legs if k), key=lambda l: med[l][2] if med[l][1] > 0 else float("inf"))
        say(f"  k = 4 apply against exact: {med['exact'][0] / med['k=4'][0]:.1f}x faster; the two scalings alone (k = 1): {med['k=1'][0]:.1f} us; "
            f"fastest sweep PCG: {best} {med[best][2]:.2f} ms against exact {med['exact'][2]:.2f} ms and Jacobi {med['Jacobi'][2]:.2f} ms "
            f"({'beats' if med[best][2] < med['Jacobi'][2] else 'loses to'} Jacobi)")
        say()
        summary.append((name, kind, med, best))
        A.destroy()
        lib.lcg_hip_trim()
    say("summary: PCG ms to convergence (iterations)")
    say(f"  {'system':<22} {'type':>5} {'Jacobi':>16} {'exact':>18} {'k=2':>16} {'k=4':>16} {'k=8':>16}  {'best sweeps vs Jacobi':>22}")
    for name, kind, med, best in summary:
        def c(leg):
            return f"{med[leg][2]:.2f} ({med[leg][1]})"
        say(f"  {name:<22} {kind:>5} {c('Jacobi'):>16} {c('exact'):>18} {c('k=2'):>16} {c('k=4'):>16} {c('k=8'):>16}  "
            f"{best + ': ' + format(med['Jacobi'][2] / med[best][2], '.2f') + 'x':>22}")
    say()
    say("(an iteration count shown negative stopped at the cap without converging; 'x' in the last column: Jacobi's time over the sweeps')")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
