"""Several right-hand sides at once against k single-vector calls: writes profiles/multi_lab.txt.

One MI355X.  Three patterns: the constant-diagonal pattern and the scrambled pattern of bench.py (33 entries per row) and the
1000 x 1000 five-point Laplacian.  For k = 2, 4, 8:
  * one lcg_hip_spmm beside k x lcg_hip_spmv (automatic kernel choice), timed with events on the library's stream, the two
    alternating in one loop, medians over --reps rounds of --inner products after a warm-up round;
  * lcg_hip_lcg_multi beside k sequential lcg_hip_lcg solves of the same columns, --steps iterations each (epsilon tiny, so nothing
    stops early), host clock around work that ends in a synchronise, medians over --reps: column-iterations per second.
The single-vector path is the library's own in the same process on the same device: its numbers are the yardstick.

--rows 0 (default) takes the largest row count at which the k = 8 blocks fit beside the matrix, its single-vector plan and the
single-vector work vectors: bounded by the int32 entry count (34 entries per row) and by 80 % of the free memory at 1400 bytes per
row; the row count used is printed with the results.

    python scripts/multi_lab.py [--rows N] [--steps 50] [--reps 7] [--inner 10] [--out profiles/multi_lab.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from liblcg_amd import _lib, api  # noqa: E402

KS = (2, 4, 8)


def bytes_per_row_and_column(k, per_row=33.0):
    """By construction: one pass over col / val (12 B per entry) shared by k columns, the gathered rows of X counted once per entry
    that misses (not modelled: 0), and the 11 vector words per row and column of the classic CG schedule."""
    return (per_row * 12.0 + 4.0) / k + 11 * 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "multi_lab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multi_lab.py measures on the GPU: there is no other way to get these numbers"
    lib = _lib.load()
    assert lib.lcg_hip_init(0) == 0
    api.use_torch_stream()
    free, total = torch.cuda.mem_get_info()
    rows = args.rows or min((2 ** 31 - 1) // 34, int(0.8 * free / 1400)) // 1_000_000 * 1_000_000
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"multi_lab: {torch.cuda.get_device_name(0)}, {free / 2**30:.0f} GiB free of {total / 2**30:.0f}; generated patterns at {rows} rows"
        f"{' (the largest at which k = 8 fits beside the matrix)' if not args.rows else ' (--rows)'}; "
        f"{args.reps} rounds, {args.inner} products per round, {args.steps} iterations per solve")
    say("bytes per row and column by construction (33 entries per row, 11 vector words): "
        + ", ".join(f"k = {k}: {bytes_per_row_and_column(k):.0f}" for k in (1,) + KS))

    def ev():
        return torch.cuda.Event(enable_timing=True)

    systems = (("constant diagonals", lambda: api.CsrMatrix.generate(rows, 16, 131072, True, 1, 0.01, pattern=api.GEN_DIAGONALS)),
               ("scrambled", lambda: api.CsrMatrix.generate(rows, 16, 0, True, 1, 0.01, pattern=api.GEN_SCRAMBLED)),
               ("laplace 1000^2", lambda: api.CsrMatrix.laplace2d(1000, 1000)))
    for name, make in systems:
        A = make()
        n, nnz = A.n, A.nnz
        say()
        say(f"== {name}: {n} rows, {nnz} entries ({nnz / n:.1f} per row)")
        g = torch.Generator(device="cuda"); g.manual_seed(1)
        x1 = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
        y1 = torch.empty_like(x1)
        A.spmv(x1, y1); api.synchronize()        # the single-vector plan is built by the first product: not on the clock
        say(f"   single-vector kernel: {lib.lcg_hip_csr_last_kernel(A.h).decode()}")
        for k in KS:
            X = torch.rand((n, k), dtype=torch.float64, device="cuda", generator=g)
            Y = torch.empty_like(X)
            t_mm, t_mv = [], []
            for r in range(args.reps + 1):
                e = [ev() for _ in range(3)]
                e[0].record()
                for _ in range(args.inner):
                    A.spmm(X, Y)
                e[1].record()
                for _ in range(args.inner * k):
                    A.spmv(x1, y1)
                e[2].record()
                torch.cuda.synchronize()
                if r:       # round 0 warms up
                    t_mm.append(e[0].elapsed_time(e[1]) * 1e3 / args.inner)
                    t_mv.append(e[1].elapsed_time(e[2]) * 1e3 / args.inner)
            mm, mv = statistics.median(t_mm), statistics.median(t_mv)
            moved = nnz * 12.0 + 4.0 * n + 16.0 * n * k        # col / val once, rowptr, X read once and Y written once
            say(f"   k = {k}: spmm {mm:9.1f} us (min {min(t_mm):.1f}, max {max(t_mm):.1f}; {moved / mm / 1e6:.2f} TB/s of must-move bytes)   "
                f"{k} x spmv {mv:9.1f} us (min {min(t_mv):.1f}, max {max(t_mv):.1f})   spmm / (k x spmv) = {mm / mv:.3f}")
            del X, Y
        # the loops: b = A.x_true per column
        for k in KS:
            XT = torch.rand((n, k), dtype=torch.float64, device="cuda", generator=g)
            B = torch.empty_like(XT)
            A.spmm(XT, B); api.synchronize()
            cols = [B[:, j].contiguous() for j in range(k)]
            para = api.lcg_default_parameters(epsilon=1e-300, max_iterations=args.steps)
            t_multi, t_seq = [], []
            for r in range(args.reps + 1):
                M = torch.zeros_like(B)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                infos = api.lcg_multi(A, M, B, para)
                api.synchronize()
                t1 = time.perf_counter()
                assert all(i.iterations == args.steps for i in infos), [(i.ret, i.iterations) for i in infos]
                ms = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(k)]
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                for j in range(k):
                    info = api.lcg_solver("lcg_hip_csr_ax", None, ms[j], cols[j], n, para, A, api.LCG_CG)
                    assert info.iterations == args.steps
                api.synchronize()
                t3 = time.perf_counter()
                if r:
                    t_multi.append(t1 - t0); t_seq.append(t3 - t2)
                if r == 1:      # same columns, same iterates (the single loop may run another schedule: to rounding, not to the bit)
                    d = max(float((M[:, j] - ms[j]).norm() / ms[j].norm()) for j in range(k))
                    say(f"   k = {k}: batched iterate against the single solves' after {args.steps} iterations: largest relative distance {d:.1e}")
                del M, ms
            a, b = statistics.median(t_multi), statistics.median(t_seq)
            say(f"   k = {k}: lcg_multi {k * args.steps / a:10.0f} column-iterations/s ({a / args.steps * 1e6:8.1f} us per batched iteration)   "
                f"{k} x lcg {k * args.steps / b:10.0f} column-iterations/s   ratio {b / a:.2f}x")
            del XT, B, cols
        A.destroy()
        lib.lcg_hip_trim()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
