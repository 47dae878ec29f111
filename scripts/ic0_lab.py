"""IC(0) lab: per system, the factor's levels, launches per apply, build time, device time of one apply
M^-1 x = L^-T (L^-1 x) from events, and PCG time-to-solution with IC(0) against Jacobi at eps = 1e-8 (r.r / max(m.m, 1)).

    python scripts/ic0_lab.py [--out profiles/ic0_lab.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def laplace3d(k):
    import scipy.sparse as sp
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(k, k))
    I = sp.identity(k)
    A = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def tridiag(n, seed=5):
    """diagonally dominant: off-diagonal uniform in [-1, 1], diagonal in [2.5, 3.5]"""
    rng = np.random.default_rng(seed)
    off = rng.uniform(-1.0, 1.0, n - 1)
    dia = 2.5 + rng.uniform(0.0, 1.0, n)
    cnt = np.full(n, 3, np.int64); cnt[0] = cnt[-1] = 2
    rp = np.zeros(n + 1, np.int64); rp[1:] = np.cumsum(cnt)
    col = np.empty(rp[-1], np.int32); val = np.empty(rp[-1])
    i = np.arange(n)
    lo = rp[:-1]
    has_l = i > 0
    col[lo[has_l]] = i[has_l] - 1; val[lo[has_l]] = off
    dpos = lo + has_l
    col[dpos] = i; val[dpos] = dia
    has_u = i < n - 1
    col[dpos[has_u] + 1] = i[has_u] + 1; val[dpos[has_u] + 1] = off
    return rp.astype(np.int32), col, val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from liblcg_amd import api
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    torch.cuda.set_device(0)
    api.use_torch_stream()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def systems():
        n, row, col, val, b = read_coo_system(os.path.join(ROOT, "tests", "golden", "case_10K_A"))
        yield "case_10K_A", api.CsrMatrix.from_csr(*coo_to_csr_host(n, row, col, val)), b
        A = api.CsrMatrix.laplace2d(1000, 1000)
        yield "laplace2d 1000x1000", A, np.ones(A.n)
        A = api.CsrMatrix.from_csr(*laplace3d(100))
        yield "laplace3d 100^3 (7-point)", A, np.ones(A.n)
        A = api.CsrMatrix.from_csr(*tridiag(1000000))
        yield "tridiagonal 1e6", A, np.ones(A.n)

    say(f"# scripts/ic0_lab.py on {torch.cuda.get_device_name(0)}; PCG eps=1e-8 abs_diff=0 from m=0; apply = mean of {args.reps} "
        f"events-timed applies after one warm-up")
    say(f"{'system':28s} {'rows':>8s} {'lev L':>7s} {'lev LT':>7s} {'launch':>6s} {'build ms':>9s} {'apply us':>10s} "
        f"{'IC its':>7s} {'IC ms':>9s} {'Jac its':>8s} {'Jac ms':>9s}")
    for name, A, b in systems():
        n = A.n
        A.build_ic0()
        A.build_jacobi()
        info = A.ic0_info()
        x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n)).cuda()
        y = torch.empty_like(x)
        A.ic0_solve(x, y)
        torch.cuda.synchronize()
        reps = args.reps if n <= 2000000 and info["levels_lower"] < 100000 else 3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            A.ic0_solve(x, y)
        e1.record()
        torch.cuda.synchronize()
        apply_us = e0.elapsed_time(e1) * 1e3 / reps
        bd = torch.from_numpy(np.ascontiguousarray(b)).cuda()
        res = {}
        for tag, mfp in (("ic", "lcg_hip_ic0_mx"), ("jac", "lcg_hip_jacobi_mx")):
            para = api.lcg_default_parameters(epsilon=1e-8, abs_diff=0, max_iterations=20000)
            best = None
            for _ in range(2):                   # the second solve: pool vectors warm
                m = torch.zeros(n, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                info_s = api.lcg_solver_preconditioned("lcg_hip_csr_ax", mfp, None, m, bd, n, para, A)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                best = (info_s.iterations, ms, info_s.ret) if best is None or ms < best[1] else best
            res[tag] = best
        say(f"{name:28s} {n:8d} {info['levels_lower']:7d} {info['levels_upper']:7d} {info['launches_per_apply']:6d} "
            f"{info['build_ms']:9.1f} {apply_us:10.1f} {res['ic'][0]:7d} {res['ic'][1]:9.2f} {res['jac'][0]:8d} {res['jac'][1]:9.2f}"
            + ("" if res["ic"][2] == 0 and res["jac"][2] == 0 else f"  (ret ic={res['ic'][2]} jac={res['jac'][2]})"))
        A.destroy()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
