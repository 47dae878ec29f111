"""Complex64 against complex128 on the same systems, in one process, alternating (c128, c64, c64, c128 per round): the A.x
time from events with its bytes / time against 8 TB/s, and the iteration rates of BiCG-sym and PCG + Jacobi (capped runs, wall
clock around the solve, vectors on the device).  DESIGN 12 quotes the table this prints.

    python scripts/c64_lab.py [--out profiles/c64_lab.txt] [--rounds 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12       # bytes / s, the MI355X's HBM
CACHE = 256 << 20   # the Infinity Cache: a product that streams less is served from it after the first of the 50 timed calls


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
    return rp.astype(np.int32), col, val


def case10k():
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    n, row, col, val, b = read_coo_system(os.path.join(ROOT, "tests", "golden", "case_10K_cA"), True)
    return coo_to_csr_host(n, row, col, val)


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

    say(f"c64_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    say("A.x: mean of 50 products between events after 5 warm-up; bytes = values + columns + row pointers + x + y once "
        "(c128 20 B / entry, c64 12 B); it/s: capped solves (eps 1e-30), wall clock around the call, median of the rounds")
    say("rounds alternate c128, c64, c64, c128; a product that streams less than the 256 MiB Infinity Cache is timed from the cache")
    say()
    systems = (("helmholtz 600^2", lambda: helmholtz(600), 400),
               ("helmholtz 2048^2", lambda: helmholtz(2048), 100),
               ("case_10K_cA", case10k, 400))
    hdr = f"{'system':<18} {'rows':>9} {'nnz':>10} {'type':>5} {'A.x us':>9} {'TB/s':>6} {'of 8':>6} {'BiCG-sym it/s':>14} {'PCG+J it/s':>11}"
    say(hdr)
    ratios = []
    for name, make, iters in systems:
        rp, ci, v = make()
        n = len(rp) - 1
        nnz = len(ci)
        A = {"c128": api.CsrMatrix.from_csr(rp, ci, v.astype(np.complex128)), "c64": api.CsrMatrix.from_csr_c64(rp, ci, v.astype(np.complex64))}
        for M in A.values():
            assert lib.lcg_hip_csr_build_jacobi(M.h, None) == 0
        dt = {"c128": torch.complex128, "c64": torch.complex64}
        rng = np.random.default_rng(1)
        xh = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        res = {k: {"ax": [], "sym": [], "pcg": []} for k in A}

        def one(kind):
            M = A[kind]
            x = torch.from_numpy(xh).to(dt[kind]).cuda(); y = torch.empty_like(x)
            mul = (lambda: M.spmv(x, y)) if kind == "c128" else (lambda: M.spmv_c64(x, y))
            for _ in range(5):
                mul()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(50):
                mul()
            e1.record(); torch.cuda.synchronize()
            res[kind]["ax"].append(e0.elapsed_time(e1) * 1e3 / 50)
            b = y.clone()
            para = api.clcg_default_parameters(epsilon=1e-30, max_iterations=iters)
            for leg in ("sym", "pcg"):
                m = torch.zeros_like(b)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if kind == "c128":
                    info = (api.clcg_solver("clcg_hip_csr_ax", None, m, b, n, para, M, api.CLCG_BICG_SYM) if leg == "sym" else
                            api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_jacobi_mx", None, m, b, n, para, M))
                else:
                    info = (api.clcg_solver_c64("clcg_hip_csr_ax_c64", None, m, b, n, para, M, api.CLCG_BICG_SYM) if leg == "sym" else
                            api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_jacobi_mx_c64", None, m, b, n, para, M))
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                res[kind][leg].append(info.iterations / el)
            return lib.lcg_hip_csr_last_kernel(M.h).decode()

        kern = {}
        for _ in range(args.rounds):
            for kind in ("c128", "c64", "c64", "c128"):
                kern[kind] = one(kind)
        med = {k: {q: float(np.median(v)) for q, v in r.items()} for k, r in res.items()}
        for kind in ("c128", "c64"):
            vb = 20 if kind == "c128" else 12
            ew = 16 if kind == "c128" else 8
            by = vb * nnz + 4 * (n + 1) + 2 * ew * n
            us = med[kind]["ax"]
            tbs = by / (us * 1e-6) / 1e12
            say(f"{name:<18} {n:>9} {nnz:>10} {kind:>5} {us:>9.2f} {tbs:>6.2f} {tbs * 1e12 / PEAK:>6.1%} {med[kind]['sym']:>14.0f} {med[kind]['pcg']:>11.0f}"
                + ("  (cache-resident: not an HBM fraction)" if by < CACHE else ""))
        r = (med["c128"]["ax"] / med["c64"]["ax"], med["c64"]["sym"] / med["c128"]["sym"], med["c64"]["pcg"] / med["c128"]["pcg"])
        ratios.append((name, r))
        say(f"{'':<18} c64 / c128: A.x {r[0]:.2f}x faster, BiCG-sym {r[1]:.2f}x, PCG+J {r[2]:.2f}x the iterations per second "
            f"(byte ratio of A.x {(20 * nnz + 4 * (n + 1) + 32 * n) / (12 * nnz + 4 * (n + 1) + 16 * n):.2f}x)")
        say(f"{'':<18} kernels: c128 {kern['c128']} | c64 {kern['c64']}")
        for q in ("ax", "sym", "pcg"):
            say(f"{'':<18} {q} by round: c128 {' '.join(f'{x:.1f}' for x in res['c128'][q])} | c64 {' '.join(f'{x:.1f}' for x in res['c64'][q])}")
        for M in A.values():
            M.destroy()
        lib.lcg_hip_trim()
    say()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
