"""Batched box-constrained solves (lcg_hip_solver_constrained_multi, lcg_hip_dense_solver_constrained_multi) at k = 2, 4, 8
against k single lcg_hip_solver_constrained solves of the same handle, in one process.  The single-vector side is code this change
leaves untouched: PG device resident, SPG with the host reading two sums after every trial step.

Systems: case_10K_A between -5 and 8 (launch-bound); the 5-point Laplacian on a 1000 x 1000 grid (+ 0.05 I) with a solution in
[-1.3, 1.3] between -0.5 and 0.8; a dense 1000 x 800 K as K^T.K (sample1's shape) with a solution in [1, 2] between 0.5 and 1.6; a
dense SPD 8192 x 8192 K (512 MiB) as K, the same bounds.  Columns: b scaled by 1, 0.8, 1.2, 0.7, 1.3, 0.9, 1.1, 0.6, so that
every column has its own active set and its own line searches and none lies outside the box altogether (such a column breaks down at
once: the batch ends it, the single solve runs on to the cap with NaN, and the two sides would not have done the same work).

Per system, solver and k: `rounds` + 1 rounds (the first is a warm-up), each the batch and then the k single solves, all capped at
`cap` accepted steps from M = 0 with epsilon far below reach; wall clock around each side between device synchronisations.
Reported: medians of column-iterations per second (accepted steps of all columns / time), the time to the cap, the spread
(max - min) / median of the batch's rounds, products per accepted step, and ratio = batch / singles in column-iterations per second
(> 1: the batch is faster; losses are marked).

    python scripts/multi_box_lab.py [--out profiles/multi_box_lab.txt] [--rounds 3] [--only SUBSTRING]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (2, 4, 8)
SCALES = [1.0, 0.8, 1.2, 0.7, 1.3, 0.9, 1.1, 0.6]


def laplacian(g):
    n = g * g
    idx = np.arange(n, dtype=np.int64)
    i, j = idx // g, idx % g
    rows, cols, vals = [idx], [idx], [np.full(n, 4.05)]
    for ok, off in ((j > 0, -1), (j < g - 1, 1), (i > 0, -g), (i < g - 1, g)):
        rows.append(idx[ok]); cols.append(idx[ok] + off); vals.append(np.full(int(ok.sum()), -1.0))
    row, col, val = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((col, row))
    rp = np.zeros(n + 1, np.int64); np.add.at(rp, row + 1, 1)
    return np.cumsum(rp).astype(np.int32), col[order].astype(np.int32), val[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="a substring of a system's name")
    args = ap.parse_args()
    import torch
    from liblcg_amd import api
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def systems():
        n, row, col, val, b = read_coo_system(os.path.join(ROOT, "tests", "golden", "case_10K_A"))
        rp, ci, v = coo_to_csr_host(n, row, col, val)
        yield "case_10K_A", "csr", api.CsrMatrix.from_csr(rp, ci, v), "lcg_hip_csr_ax", None, dev(b), -5.0, 8.0, 100
        g = 1000
        rp, ci, v = laplacian(g)
        A = api.CsrMatrix.from_csr(rp, ci, v)
        i = np.arange(g * g, dtype=np.float64)
        xt = dev(np.sin(0.7 * i) + 0.3 * np.cos(0.013 * i)); b = torch.empty_like(xt)
        A.spmv(xt, b); api.synchronize()
        yield "laplacian_1000x1000", "csr", A, "lcg_hip_csr_ax", None, b, -0.5, 0.8, 60
        gen = torch.Generator(device="cuda"); gen.manual_seed(1000 * 31 + 800)
        K = torch.rand((1000, 800), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        xt = torch.rand(800, dtype=torch.float64, device="cuda", generator=gen) + 1
        yield "dense_1000x800_KtK", "dense", api.DenseMatrix.from_array(K), "lcg_hip_dense_ata_ax", 1, K.T @ (K @ xt), 0.5, 1.6, 60
        G = torch.rand((8192, 8192), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        K = G.T @ G / 8192.0 + torch.eye(8192, dtype=torch.float64, device="cuda")
        del G
        xt = torch.rand(8192, dtype=torch.float64, device="cuda", generator=gen) + 1
        yield "dense_8192x8192_K", "dense", api.DenseMatrix.from_array(K), "lcg_hip_dense_ax", 0, K @ xt, 0.5, 1.6, 40

    say(f"multi_box_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    say(f"medians of {args.rounds} rounds after a warm-up round; spread = (max - min) / median of the batch; ratio = batch / k single solves in "
        f"column-iterations per second (> 1: the batch is faster)")
    say()
    for name, kind, H, afp, normal, b, lo, hi, cap in systems():
        if args.only and args.only not in name:
            H.destroy()
            continue
        n = int(b.shape[0])
        low, hig = torch.full((n,), lo, dtype=torch.float64, device="cuda"), torch.full((n,), hi, dtype=torch.float64, device="cuda")
        para = api.lcg_default_parameters(epsilon=1e-300, abs_diff=0, max_iterations=cap)
        say(f"{name}: n = {n}, bounds {lo} / {hi}, cap {cap}")
        for sid, sname in ((api.LCG_PG, "PG"), (api.LCG_SPG, "SPG")):
            for k in KS:
                scale = torch.tensor(SCALES[:k], dtype=torch.float64, device="cuda")
                B = (b[:, None] * scale[None, :]).contiguous()
                cols = [B[:, j].contiguous() for j in range(k)]
                tb, ts, ib, isg, pb = [], [], 0, 0, 0
                for r in range(args.rounds + 1):
                    M = torch.zeros_like(B)
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    if kind == "csr":
                        infos = api.lcg_solver_constrained_multi(H, M, B, low, hig, para, sid)
                    else:
                        infos = api.dense_solver_constrained_multi(H, M, B, low, hig, para, sid, normal=bool(normal))
                    torch.cuda.synchronize(); t1 = time.perf_counter()
                    singles = []
                    for j in range(k):
                        m = torch.zeros(n, dtype=torch.float64, device="cuda")
                        singles.append(api.lcg_solver_constrained(afp, None, m, cols[j], low, hig, n, para, H, sid))
                    torch.cuda.synchronize(); t2 = time.perf_counter()
                    if r:
                        tb.append(t1 - t0); ts.append(t2 - t1)
                    ib, isg, pb = sum(i.iterations for i in infos), sum(i.iterations for i in singles), sum(i.products for i in infos)
                mb, ms = statistics.median(tb), statistics.median(ts)
                rate_b, rate_s = ib / mb, isg / ms
                ratio = rate_b / rate_s
                mark = "" if ratio >= 1.0 else "  ** LOSS **"
                say(f"  {sname:3s} k={k}: batch {rate_b:10.0f} column-iterations/s, {mb * 1e3:9.2f} ms to the cap (spread {(max(tb) - min(tb)) / mb:5.1%}; "
                    f"{ib} accepted steps, {pb / max(ib, 1):.2f} products per step)  {k} single solves {rate_s:10.0f}, {ms * 1e3:9.2f} ms ({isg} steps)  "
                    f"ratio {ratio:5.2f}{mark}")
        say()
        H.destroy()
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
