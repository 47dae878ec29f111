"""Several complex64 right-hand sides at once against k single-vector calls: writes profiles/multi_c64_lab.txt.

One MI355X, one process.  The two complex-symmetric systems of profiles/multi_cplx_lab.txt -- the 1000 x 1000 five-point Laplacian
with a complex shift on its diagonal (5 entries per row) and bench.py's constant-diagonal pattern (31 entries per row) with the same
kind of shift -- cast to complex64.  For k = 2, 4, 8:
  * one clcg_hip_spmm_c64 beside k x lcg_hip_spmv_c64 on the same handle, timed with events on the library's stream, the two
    alternating in one loop, medians over --reps rounds of --inner products after a warm-up round;
  * clcg_hip_lbicg_sym_multi_c64 beside k sequential clcg_hip_solver_c64(CLCG_BICG_SYM) solves, and clcg_hip_lpcg_multi_c64 beside k
    sequential clcg_hip_solver_preconditioned_c64(CLCG_PCG, clcg_hip_jacobi_mx_c64) solves of the same columns, --steps iterations
    each (epsilon tiny, so nothing stops early), host clock around work that ends in a synchronise, the two sides alternating,
    medians over --reps: column-iterations per second, and the ratio beside its cap by construction;
  * the complex128 batch (clcg_hip_spmm, clcg_hip_lbicg_sym_multi, clcg_hip_lpcg_multi) on the same system in complex128, in the same
    process, for comparison.
The single-vector path is the library's own in the same process on the same device: its numbers are the yardstick.

    python scripts/multi_c64_lab.py [--rows 1000000] [--steps 50] [--reps 5] [--inner 10] [--out profiles/multi_c64_lab.txt]
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
    """By construction, from the passes as written (solvers_multi_c64.hip, solvers_c64.hip), 8 B per element, the gathers of x not
    counted.  Batched: the product writes A.d (8) and its finishing lanes read d again for d.Ad (8); update: reads d, m, Ad, r, writes
    m, r (48; PCG: + s written, + the diagonal's 8 B per row shared by k columns); direction: reads d and r (s), writes d (24).
    Single: the product writes A.d (8); d.Ad is a pass of its own (16); update 48 (PCG: + diagonal read and s written, 64);
    direction 24.  Matrix: 12 B per entry, shared by k columns in a batch."""
    if k == 0:      # the single-vector loop
        return (96.0 if loop == "bicg_sym" else 112.0) + 12.0 * per_row
    vec = 88.0 if loop == "bicg_sym" else 96.0 + 8.0 / k
    return vec + 12.0 * per_row / k


def cap(loop, k, per_row):
    return bytes_per_row_and_column(loop, 0, per_row) / bytes_per_row_and_column(loop, k, per_row)


def complex_shifted(A, seed):
    """A real symmetric handle -> the arrays of a complex-symmetric one: the same pattern and values, i 0.3 (0.2 + u) |a_ii| added
    on the diagonal (scripts/multi_cplx_lab.py's systems)."""
    rp, ci, v = A.arrays_to_host()
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    vc = v.astype(np.complex128)
    dg = np.flatnonzero(rows == ci)
    u = np.random.default_rng(seed).uniform(size=len(dg))
    vc[dg] += 0.05 + 0.3j * (0.2 + u) * np.maximum(np.abs(v[dg]), 1.0)
    del rows
    return rp, ci, vc


def mark(ratio):
    """A loss in bold, as the README marks them."""
    return f"**{ratio:.2f}x**" if ratio < 1.0 else f"{ratio:.2f}x"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "multi_c64_lab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multi_c64_lab.py measures on the GPU: there is no other way to get these numbers"
    lib = _lib.load()
    assert lib.lcg_hip_init(0) == 0
    api.use_torch_stream()
    free, total = torch.cuda.mem_get_info()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"multi_c64_lab: {torch.cuda.get_device_name(0)}, {free / 2**30:.0f} GiB free of {total / 2**30:.0f}; "
        f"{args.reps} rounds, {args.inner} products per round, {args.steps} iterations per solve; losses in bold")
    for per_row in (5, 31.4):
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
        rp, ci, vc = complex_shifted(Ar, 7)
        Ar.destroy()
        A = api.CsrMatrix.from_csr_c64(rp, ci, vc.astype(np.complex64))
        Z = api.CsrMatrix.from_csr(rp, ci, vc)
        A.build_jacobi(); Z.build_jacobi()
        n, nnz = A.n, len(ci)
        per_row = nnz / n
        del rp, ci, vc
        say()
        say(f"== {name}, complex64: {n} rows, {nnz} entries ({per_row:.1f} per row)")
        g = torch.Generator(device="cuda"); g.manual_seed(1)

        def crand(dtype, *shape):
            real = torch.float32 if dtype == torch.complex64 else torch.float64
            return torch.complex(torch.rand(shape, dtype=real, device="cuda", generator=g),
                                 torch.rand(shape, dtype=real, device="cuda", generator=g))

        x1 = crand(torch.complex64, n)
        y1 = torch.empty_like(x1)
        A.spmv_c64(x1, y1); api.synchronize()        # the single-vector plan is built by the first product: not on the clock
        say(f"   single-vector kernel: {lib.lcg_hip_csr_last_kernel(A.h).decode()}")
        for k in KS:
            X = crand(torch.complex64, n, k)
            Y = torch.empty_like(X)
            XZ = crand(torch.complex128, n, k)
            YZ = torch.empty_like(XZ)
            t_mm, t_mv, t_zz = [], [], []
            for r in range(args.reps + 1):
                e = [ev() for _ in range(4)]
                e[0].record()
                for _ in range(args.inner):
                    A.cspmm_c64(X, Y)
                e[1].record()
                for _ in range(args.inner * k):
                    A.spmv_c64(x1, y1)
                e[2].record()
                for _ in range(args.inner):
                    Z.cspmm(XZ, YZ)
                e[3].record()
                torch.cuda.synchronize()
                if r:       # round 0 warms up
                    t_mm.append(e[0].elapsed_time(e[1]) * 1e3 / args.inner)
                    t_mv.append(e[1].elapsed_time(e[2]) * 1e3 / args.inner)
                    t_zz.append(e[2].elapsed_time(e[3]) * 1e3 / args.inner)
            mm, mv, zz = statistics.median(t_mm), statistics.median(t_mv), statistics.median(t_zz)
            moved = nnz * 12.0 + 4.0 * n + 16.0 * n * k        # col / val once, rowptr, X read once and Y written once
            say(f"   k = {k}: cspmm_c64 {mm:9.1f} us (min {min(t_mm):.1f}, max {max(t_mm):.1f}; {moved / mm / 1e6:.2f} TB/s of must-move bytes)   "
                f"{k} x spmv_c64 {mv:9.1f} us (min {min(t_mv):.1f}, max {max(t_mv):.1f})   k x spmv_c64 / cspmm_c64 = {mark(mv / mm)} "
                f"(cap {(12.0 * per_row + 16.0) / (12.0 * per_row / k + 16.0):.2f}x)   complex128 cspmm {zz:9.1f} us = {zz / mm:.2f} x cspmm_c64")
            del X, Y, XZ, YZ
        # the loops: b = A.x_true per column
        para = api.clcg_default_parameters(epsilon=1e-300, max_iterations=args.steps)
        loops = (("bicg_sym", api.clbicg_sym_multi_c64, api.clbicg_sym_multi,
                  lambda m, b: api.clcg_solver_c64("clcg_hip_csr_ax_c64", None, m, b, n, para, A, api.CLCG_BICG_SYM)),
                 ("pcg", api.clpcg_multi_c64, api.clpcg_multi,
                  lambda m, b: api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_jacobi_mx_c64", None, m, b, n, para, A,
                                                                  api.CLCG_PCG)))
        for loop, multi, multi_z, single in loops:
            for k in KS:
                XT = crand(torch.complex64, n, k)
                B = torch.empty_like(XT)
                A.cspmm_c64(XT, B); api.synchronize()
                BZ = B.to(torch.complex128)
                cols = [B[:, j].contiguous() for j in range(k)]
                t_multi, t_seq, t_z = [], [], []
                for r in range(args.reps + 1):
                    M = torch.zeros_like(B)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    infos = multi(A, M, B, para)
                    api.synchronize()
                    t1 = time.perf_counter()
                    assert all(i.iterations == args.steps for i in infos), [(i.ret, i.iterations) for i in infos]
                    ms = [torch.zeros(n, dtype=torch.complex64, device="cuda") for _ in range(k)]
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    for j in range(k):
                        info = single(ms[j], cols[j])
                        assert info.iterations == args.steps, (info.ret, info.iterations)
                    api.synchronize()
                    t3 = time.perf_counter()
                    MZ = torch.zeros_like(BZ)
                    torch.cuda.synchronize()
                    t4 = time.perf_counter()
                    multi_z(Z, MZ, BZ, para)
                    api.synchronize()
                    t5 = time.perf_counter()
                    if r:
                        t_multi.append(t1 - t0); t_seq.append(t3 - t2); t_z.append(t5 - t4)
                    if r == 1:      # same columns, same iterates (other summation orders: to fp32 rounding, not to the bit)
                        d = max(float((M[:, j] - ms[j]).norm() / ms[j].norm()) for j in range(k))
                        say(f"   {loop} k = {k}: batched iterate against the single solves' after {args.steps} iterations: largest relative distance {d:.1e}")
                    del M, ms, MZ
                a, b, z = statistics.median(t_multi), statistics.median(t_seq), statistics.median(t_z)
                say(f"   {loop} k = {k}: batched {k * args.steps / a:10.0f} column-iterations/s ({a / args.steps * 1e6:8.1f} us per batched iteration)   "
                    f"{k} x single {k * args.steps / b:10.0f} column-iterations/s   ratio {mark(b / a)} (cap {cap(loop, k, per_row):.2f}x)   "
                    f"complex128 batch {k * args.steps / z:10.0f} column-iterations/s")
                del XT, B, BZ, cols
        A.destroy(); Z.destroy()
        lib.lcg_hip_trim()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
