"""Complex64 IC(0) against complex128 IC(0) on the same systems, in one process, alternating (c128, c64 per round): the build
time, the device time of one full apply M^-1 x = L^-T (L^-1 x) from events, and PCG to sample14's stop rule (eps = 1e-6 on
|r|^2 / max(|m|, 1)^2, from m = 0) with IC(0) and with Jacobi: iterations and wall-clock milliseconds around the solve (vectors on
the device).  Medians of the rounds.  DESIGN 11 / 12 quote the table this prints.

    python scripts/ic0_c64_lab.py [--out profiles/ic0_c64_lab.txt] [--rounds 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP = 5000      # sample14 runs uncapped; the cap only bounds a run that would not converge in fp32


def helmholtz(nx):
    """5-point Laplacian + (0.3 + 0.8i) I on an nx x nx grid (tests/test_gpu_solvers.py), rows sorted by column."""
    n = nx * nx
    idx = np.arange(n, dtype=np.int64)
    ix, iy = idx % nx, idx // nx
    lens = 1 + (ix > 0) + (ix < nx - 1) + (iy > 0) + (iy < nx - 1)
    rp = np.zeros(n + 1, np.int64); rp[1:] = np.cumsum(lens)
    col = np.empty(rp[-1], np.int32); val = np.empty(rp[-1], np.complex128)
    pos = rp[:-1].copy()
    for ok, off, v in ((iy > 0, -nx, -1.0), (ix > 0, -1, -1.0), (np.ones(n, bool), 0, 4.3 + 0.8j), (ix < nx - 1, 1, -1.0), (iy < nx - 1, nx, -1.0)):
        p = pos[ok]
        col[p] = (idx[ok] + off).astype(np.int32); val[p] = v
        pos[ok] += 1
    rp = rp.astype(np.int32)
    import scipy.sparse as sp
    b = sp.csr_matrix((val, col, rp), shape=(n, n)) @ np.ones(n, np.complex128)
    return rp, col, val, b


def case(tag):
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    n, row, col, val, b = read_coo_system(os.path.join(ROOT, "tests", "golden", f"case_{tag}_cA"), True)
    rp, ci, v = coo_to_csr_host(n, row, col, val)
    return rp, ci, v, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    from liblcg_amd import _lib, api
    lib = _lib.load()
    assert torch.cuda.is_available()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"ic0_c64_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    say(f"build: host ms of lcg_hip_csr_build_ic0(_c64) (lcg_hip_csr_ic0_info); apply: mean of 20 full applies between events after "
        f"one warm-up; PCG: eps 1e-6, abs_diff 0, m = 0, cap {CAP}, wall clock around the solve; medians of {args.rounds} rounds, "
        "each round c128 then c64")
    say()
    systems = (("case_1K_cA", lambda: case("1K")), ("case_10K_cA", lambda: case("10K")), ("helmholtz 600^2", lambda: helmholtz(600)))
    say(f"{'system':<16} {'rows':>7} {'type':>5} {'lev L':>6} {'launch':>6} {'MiB':>7} {'build ms':>9} {'apply us':>9} "
        f"{'IC its':>6} {'IC ms':>8} {'Jac its':>7} {'Jac ms':>8}")
    for name, make in systems:
        rp, ci, v, bh = make()
        n = len(rp) - 1
        mats = {"c128": lambda: api.CsrMatrix.from_csr(rp, ci, v.astype(np.complex128)),
                "c64": lambda: api.CsrMatrix.from_csr_c64(rp, ci, v.astype(np.complex64))}
        dt = {"c128": torch.complex128, "c64": torch.complex64}
        res = {k: {"build": [], "apply": [], "ic_it": [], "ic_ms": [], "jac_it": [], "jac_ms": []} for k in mats}
        info = {}

        def one(kind):
            M = mats[kind]()
            try:
                M.build_ic0()
                info[kind] = M.ic0_info()
                res[kind]["build"].append(info[kind]["build_ms"])
                assert lib.lcg_hip_csr_build_jacobi(M.h, None) == 0
                b = torch.from_numpy(bh).to(dt[kind]).cuda()
                y = torch.empty_like(b)
                M.ic0_solve(b, y)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(20):
                    M.ic0_solve(b, y)
                e1.record(); torch.cuda.synchronize()
                res[kind]["apply"].append(e0.elapsed_time(e1) * 1e3 / 20)
                para = api.clcg_default_parameters(epsilon=1e-6, abs_diff=0, max_iterations=CAP)
                for leg in ("ic", "jac"):
                    m = torch.zeros_like(b)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if kind == "c128":
                        r = api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_ic0_mx" if leg == "ic" else "clcg_hip_jacobi_mx",
                                                           None, m, b, n, para, M)
                    else:
                        r = api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_ic0_mx_c64" if leg == "ic" else
                                                               "clcg_hip_jacobi_mx_c64", None, m, b, n, para, M)
                    torch.cuda.synchronize()
                    res[kind][f"{leg}_ms"].append((time.perf_counter() - t0) * 1e3)
                    res[kind][f"{leg}_it"].append(r.iterations if r.ret == 0 else -r.iterations)     # negative: stopped at the cap
            finally:
                M.destroy()
                lib.lcg_hip_trim()

        for _ in range(args.rounds):
            for kind in ("c128", "c64"):
                one(kind)
        for kind in ("c128", "c64"):
            med = {q: float(np.median(x)) for q, x in res[kind].items()}
            f = info[kind]
            say(f"{name:<16} {n:>7} {kind:>5} {f['levels_lower']:>6} {f['launches_per_apply']:>6} {f['bytes'] / 2**20:>7.2f} "
                f"{med['build']:>9.2f} {med['apply']:>9.1f} {int(med['ic_it']):>6} {med['ic_ms']:>8.2f} {int(med['jac_it']):>7} "
                f"{med['jac_ms']:>8.2f}")
        for q in ("build", "apply", "ic_ms", "jac_ms"):
            say(f"{'':<16} {q} by round: c128 {' '.join(f'{x:.2f}' for x in res['c128'][q])} | c64 {' '.join(f'{x:.2f}' for x in res['c64'][q])}")
    say()
    say("(an iteration count shown negative stopped at the cap without converging)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
