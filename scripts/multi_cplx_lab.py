"""Several complex right-hand sides at once against k single-vector calls: writes profiles/multi_cplx_lab.txt.

One MI355X.  Two complex-symmetric systems: the 1000 x 1000 five-point Laplacian with a complex shift on its diagonal (5 entries per
row) and bench.py's constant-diagonal pattern (33 entries per row) with the same kind of shift.  For k = 2, 4, 8:
  * one clcg_hip_spmm beside k x lcg_hip_spmv on the complex handle (automatic kernel choice), timed with events on the library's
    stream, the two alternating in one loop, medians over --reps rounds of --inner products after a warm-up round;
  * clcg_hip_lbicg_sym_multi beside k sequential clcg_hip_solver(CLCG_BICG_SYM) solves, and clcg_hip_lpcg_multi beside k sequential
    clcg_hip_solver_preconditioned(CLCG_PCG, clcg_hip_jacobi_mx) solves of the same columns, --steps iterations each (epsilon tiny,
    so nothing stops early), host clock around work that ends in a synchronise, the two sides alternating, medians over --reps:
    column-iterations per second, and the ratio beside its cap by construction.
The single-vector path is the library's own in the same process on the same device: its numbers are the yardstick.

    python scripts/multi_cplx_lab.py [--rows 1000000] [--steps 50] [--reps 7] [--inner 10] [--out profiles/multi_cplx_lab.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from liblcg_amd import _lib, api  # noqa: E402

KS = (2, 4, 8)


def bytes_per_row_and_column(loop, k, per_row):
    """By construction, from the passes as written (solvers_multi_cplx.hip, solvers_cplx.hip), the gathers of x not counted.
    Batched: the product writes A.d (16) and its finishing lanes read d again for d.Ad (16); update: reads d, m, Ad, r, writes m, r
    (96; PCG: + s written, + the diagonal's 16 B per row shared by k columns); direction: reads d and r (s), writes d (48).
    Single: the product writes A.d (16); d.Ad is a pass of its own (32); update 96 (PCG: + diagonal read and s written, 128);
    direction 48.  Matrix: 20 B per entry, shared by k columns in a batch."""
    if k == 0:      # the single-vector loop
        return (192.0 if loop == "bicg_sym" else 224.0) + 20.0 * per_row
    vec = 176.0 if loop == "bicg_sym" else 192.0 + 16.0 / k
    return vec + 20.0 * per_row / k


def cap(loop, k, per_row):
    return bytes_per_row_and_column(loop, 0, per_row) / bytes_per_row_and_column(loop, k, per_row)


def complex_shifted(A, seed):
    """A real symmetric handle -> a complex-symmetric one: the same pattern and values, i 0.3 (0.2 + u) |a_ii| added on the diagonal."""
    rp, ci, v = A.arrays_to_host()
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    vc = v.astype(np.complex128)
    dg = np.flatnonzero(rows == ci)
    u = np.random.default_rng(seed).uniform(size=len(dg))
    vc[dg] += 0.05 + 0.3j * (0.2 + u) * np.maximum(np.abs(v[dg]), 1.0)
    del rows
    return api.CsrMatrix.from_csr(rp, ci, vc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "multi_cplx_lab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multi_cplx_lab.py measures on the GPU: there is no other way to get these numbers"
    lib = _lib.load()
    assert lib.lcg_hip_init(0) == 0
    api.use_torch_stream()
    free, total = torch.cuda.mem_get_info()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"multi_cplx_lab: {torch.cuda.get_device_name(0)}, {free / 2**30:.0f} GiB free of {total / 2**30:.0f}; "
        f"{args.reps} rounds, {args.inner} products per round, {args.steps} iterations per solve")
    for per_row in (5, 33):
        say(f"caps by construction at {per_row} entries per row (single / batched bytes per row and column): "
            + "; ".join(f"{loop} " + ", ".join(f"k = {k}: {cap(loop, k, per_row):.2f}x" for k in KS) for loop in ("bicg_sym", "pcg")))

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def real_laplace():
        return api.CsrMatrix.laplace2d(1000, 1000)

    def real_diagonals():
        return api.CsrMatrix.generate(args.rows, 16, 131072, True, 1, 0.01, pattern=api.GEN_DIAGONALS)

    for name, make in (("complex-shifted laplace 1000^2", real_laplace), ("complex-shifted constant diagonals", real_diagonals)):
        Ar = make()
        A = complex_shifted(Ar, 7)
        Ar.destroy()
        A.build_jacobi()
        n, nnz = A.n, A.nnz
        per_row = nnz / n
        say()
        say(f"== {name}: {n} rows, {nnz} entries ({per_row:.1f} per row)")
        g = torch.Generator(device="cuda"); g.manual_seed(1)

        def crand(*shape):
            return torch.complex(torch.rand(shape, dtype=torch.float64, device="cuda", generator=g),
                                 torch.rand(shape, dtype=torch.float64, device="cuda", generator=g))

        x1 = crand(n)
        y1 = torch.empty_like(x1)
        A.spmv(x1, y1); api.synchronize()        # the single-vector plan is built by the first product: not on the clock
        say(f"   single-vector kernel: {lib.lcg_hip_csr_last_kernel(A.h).decode()}")
        for k in KS:
            X = crand(n, k)
            Y = torch.empty_like(X)
            t_mm, t_mv = [], []
            for r in range(args.reps + 1):
                e = [ev() for _ in range(3)]
                e[0].record()
                for _ in range(args.inner):
                    A.cspmm(X, Y)
                e[1].record()
                for _ in range(args.inner * k):
                    A.spmv(x1, y1)
                e[2].record()
                torch.cuda.synchronize()
                if r:       # round 0 warms up
                    t_mm.append(e[0].elapsed_time(e[1]) * 1e3 / args.inner)
                    t_mv.append(e[1].elapsed_time(e[2]) * 1e3 / args.inner)
            mm, mv = statistics.median(t_mm), statistics.median(t_mv)
            moved = nnz * 20.0 + 4.0 * n + 32.0 * n * k        # col / val once, rowptr, X read once and Y written once
            say(f"   k = {k}: cspmm {mm:9.1f} us (min {min(t_mm):.1f}, max {max(t_mm):.1f}; {moved / mm / 1e6:.2f} TB/s of must-move bytes)   "
                f"{k} x spmv {mv:9.1f} us (min {min(t_mv):.1f}, max {max(t_mv):.1f})   k x spmv / cspmm = {mv / mm:.2f}x "
                f"(cap {(20.0 * per_row + 32.0) / (20.0 * per_row / k + 32.0):.2f}x)")
            del X, Y
        # the loops: b = A.x_true per column
        para = api.clcg_default_parameters(epsilon=1e-300, max_iterations=args.steps)
        loops = (("bicg_sym", api.clbicg_sym_multi,
                  lambda m, b: api.clcg_solver("clcg_hip_csr_ax", None, m, b, n, para, A, api.CLCG_BICG_SYM)),
                 ("pcg", api.clpcg_multi,
                  lambda m, b: api.clcg_solver_preconditioned("clcg_hip_csr_ax", "clcg_hip_jacobi_mx", None, m, b, n, para, A, api.CLCG_PCG)))
        for loop, multi, single in loops:
            for k in KS:
                XT = crand(n, k)
                B = torch.empty_like(XT)
                A.cspmm(XT, B); api.synchronize()
                cols = [B[:, j].contiguous() for j in range(k)]
                t_multi, t_seq = [], []
                for r in range(args.reps + 1):
                    M = torch.zeros_like(B)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    infos = multi(A, M, B, para)
                    api.synchronize()
                    t1 = time.perf_counter()
                    assert all(i.iterations == args.steps for i in infos), [(i.ret, i.iterations) for i in infos]
                    ms = [torch.zeros(n, dtype=torch.complex128, device="cuda") for _ in range(k)]
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    for j in range(k):
                        info = single(ms[j], cols[j])
                        assert info.iterations == args.steps, (info.ret, info.iterations)
                    api.synchronize()
                    t3 = time.perf_counter()
                    if r:
                        t_multi.append(t1 - t0); t_seq.append(t3 - t2)
                    if r == 1:      # same columns, same iterates (other summation orders: to rounding, not to the bit)
                        d = max(float((M[:, j] - ms[j]).norm() / ms[j].norm()) for j in range(k))
                        say(f"   {loop} k = {k}: batched iterate against the single solves' after {args.steps} iterations: largest relative distance {d:.1e}")
                    del M, ms
                a, b = statistics.median(t_multi), statistics.median(t_seq)
                say(f"   {loop} k = {k}: batched {k * args.steps / a:10.0f} column-iterations/s ({a / args.steps * 1e6:8.1f} us per batched iteration)   "
                    f"{k} x single {k * args.steps / b:10.0f} column-iterations/s   ratio {b / a:.2f}x (cap {cap(loop, k, per_row):.2f}x)")
                del XT, B, cols
        A.destroy()
        lib.lcg_hip_trim()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
