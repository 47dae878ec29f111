"""Several complex right-hand sides against one NON-symmetric matrix: the batched BiCGStab and its two product modes against the
single-vector path: writes profiles/multi_cbicgstab_lab.txt.

One MI355X.  The two systems of scripts/multi_cplx_lab.py -- the 1000 x 1000 five-point Laplacian with a complex shift on its diagonal
(5 entries per row) and bench.py's constant-diagonal pattern (33 entries per row) with the same kind of shift -- made non-symmetric by
halving every strictly upper entry.  For k = 2, 4, 8:
  * one clcg_hip_spmm_inner and one clcg_hip_spmm_dot2 beside one clcg_hip_spmm (what the carried sums cost; the entries read their
    sums back to the host, a synchronise per call that the plain product does not pay), host clock around --inner calls that end in
    a synchronise, the three alternating in one loop, medians over --reps rounds after a warm-up round;
  * clcg_hip_lbicgstab_multi, plain and with Jacobi, beside k sequential clcg_hip_solver(CLCG_BICGSTAB) solves on clcg_hip_csr_ax of
    the same columns at the same shadow seed, --steps iterations each (epsilon tiny, so nothing stops early), host clock around
    work that ends in a synchronise, the sides alternating, medians over --reps: column-iterations per second and their ratio.
    Every solve is also timed at ONE iteration; the difference is what the iterations cost without the set-up (the guess's product
    and the draw and upload of the shadow vector, once per batch and once per single solve), and that ratio stands beside its cap
    by construction.  The single-vector family has no right-preconditioned complex BiCGStab: the Jacobi batch is set beside the
    same plain single solves.
The single-vector path is the library's own in the same process on the same device: its numbers are the yardstick.

    python scripts/multi_cbicgstab_lab.py [--rows 1000000] [--steps 50] [--reps 7] [--inner 10] [--out profiles/multi_cbicgstab_lab.txt]
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
    """By construction, from the passes as written (solvers_multi_cbicg.hip, solvers_cplx.hip: solve_cbicgstab), 16 B per complex
    element, each product's gather of x counted once (16).
    Single: A.p reads p, writes Ap (32); <rb,Ap> (32); s = r - ak Ap (48); A.s (32); <As,s>, <As,As> (32); update reads s, p, m, As, rb,
    writes m, r (112); direction reads p, Ap, r, writes p (64): 352.
    Batched, plain: A.p reads p, writes v, rb once per row (32 + 16 / k); s = r - ak v (48); A.s reads s, writes t, its finishing
    lanes read s again (48); update reads m, p, s, t, writes m, r, rb once per row (96 + 16 / k); direction (64): 288 + 32 / k.
    Batched, Jacobi: the passes that write p and s also write ph and sh and read the diagonal once per row (+ 32 + 32 / k), the
    update reads ph, sh and s (+ 16): 336 + 64 / k.
    Matrix: 20 B per entry, twice per iteration, shared by k columns in a batch."""
    if k == 0:
        return 352.0 + 40.0 * per_row
    vec = 288.0 + 32.0 / k if loop == "plain" else 336.0 + 64.0 / k
    return vec + 40.0 * per_row / k


def cap(loop, k, per_row):
    return bytes_per_row_and_column(loop, 0, per_row) / bytes_per_row_and_column(loop, k, per_row)


def complex_nonsymmetric(A, seed):
    """A real symmetric handle -> a complex non-symmetric one: the same pattern, i 0.3 (0.2 + u) |a_ii| added on the diagonal
    (scripts/multi_cplx_lab.py: complex_shifted) and every strictly upper entry halved."""
    rp, ci, v = A.arrays_to_host()
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    vc = v.astype(np.complex128)
    dg = np.flatnonzero(rows == ci)
    u = np.random.default_rng(seed).uniform(size=len(dg))
    vc[dg] += 0.05 + 0.3j * (0.2 + u) * np.maximum(np.abs(v[dg]), 1.0)
    vc[ci > rows] *= 0.5
    del rows
    return api.CsrMatrix.from_csr(rp, ci, vc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "multi_cbicgstab_lab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multi_cbicgstab_lab.py measures on the GPU: there is no other way to get these numbers"
    lib = _lib.load()
    assert lib.lcg_hip_init(0) == 0
    api.use_torch_stream()
    free, total = torch.cuda.mem_get_info()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"multi_cbicgstab_lab: {torch.cuda.get_device_name(0)}, {free / 2**30:.0f} GiB free of {total / 2**30:.0f}; "
        f"{args.reps} rounds, {args.inner} products per round, {args.steps} iterations per solve")
    for per_row in (5, 31, 33):
        say(f"caps by construction at {per_row} entries per row (single / batched bytes per row and column): "
            + "; ".join(f"{loop} " + ", ".join(f"k = {k}: {cap(loop, k, per_row):.2f}x" for k in KS) for loop in ("plain", "jacobi")))

    def real_laplace():
        return api.CsrMatrix.laplace2d(1000, 1000)

    def real_diagonals():
        return api.CsrMatrix.generate(args.rows, 16, 131072, True, 1, 0.01, pattern=api.GEN_DIAGONALS)

    for name, make in (("non-symmetric complex laplace 1000^2", real_laplace), ("non-symmetric complex constant diagonals", real_diagonals)):
        Ar = make()
        A = complex_nonsymmetric(Ar, 7)
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

        u1 = crand(n)
        for k in KS:
            X, U = crand(n, k), crand(n, k)
            Y = torch.empty_like(X)
            t = {"spmm": [], "inner": [], "dot2": []}
            calls = {"spmm": lambda: A.cspmm(X, Y), "inner": lambda: A.cspmm_inner(X, Y, u1), "dot2": lambda: A.cspmm_dot2(X, Y, U)}
            for r in range(args.reps + 1):
                for what, call in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.inner):
                        call()
                    api.synchronize()
                    if r:       # round 0 warms up
                        t[what].append((time.perf_counter() - t0) * 1e6 / args.inner)
            med = {w: statistics.median(v) for w, v in t.items()}
            moved = nnz * 20.0 + 4.0 * n + 32.0 * n * k        # col / val once, rowptr, X read once and Y written once
            say(f"   k = {k}: cspmm {med['spmm']:9.1f} us ({moved / med['spmm'] / 1e6:.2f} TB/s of must-move bytes)   "
                f"inner {med['inner']:9.1f} us ({med['inner'] / med['spmm']:.2f}x, min {min(t['inner']):.1f})   "
                f"dot2 {med['dot2']:9.1f} us ({med['dot2'] / med['spmm']:.2f}x, min {min(t['dot2']):.1f})   (the two read their sums back: one synchronise per call)")
            del X, U, Y
        # the loops: b = A.x_true per column.  Every solve is timed at --steps iterations and at ONE: the difference is what the
        # iterations cost, without the set-up (the guess's product and, on both sides, the draw and upload of the shadow vector --
        # once per batch, once per single solve)
        seed = 3
        paras = {"full": api.clcg_default_parameters(epsilon=1e-300, max_iterations=args.steps),
                 "one": api.clcg_default_parameters(epsilon=1e-300, max_iterations=1)}

        def batch(B, loop, which):
            M = torch.zeros_like(B)
            lib.lcg_hip_set_shadow_seed(seed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            infos = api.clbicgstab_multi(A, M, B, paras[which], precond=None if loop == "plain" else "jacobi")
            api.synchronize()
            return time.perf_counter() - t0, sum(i.iterations for i in infos), M

        def singles(cols, which):
            ms = [torch.zeros(n, dtype=torch.complex128, device="cuda") for _ in cols]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            its = 0
            for m, b in zip(ms, cols):
                its += api.clcg_solver("clcg_hip_csr_ax", None, m, b, n, paras[which], A, api.CLCG_BICGSTAB, shadow_seed=seed).iterations
            api.synchronize()
            return time.perf_counter() - t0, its, ms

        for k in KS:
            XT = crand(n, k)
            B = torch.empty_like(XT)
            A.cspmm(XT, B); api.synchronize()
            cols = [B[:, j].contiguous() for j in range(k)]
            T = {(side, which): [] for side in ("plain", "jacobi", "single") for which in ("full", "one")}
            its = {}
            for r in range(args.reps + 1):
                got = {}
                for which in ("full", "one"):
                    for loop in ("plain", "jacobi"):
                        got[(loop, which)] = batch(B, loop, which)
                    got[("single", which)] = singles(cols, which)
                for key, (sec, n_it, _) in got.items():
                    its[key] = n_it
                    if r:       # round 0 warms up
                        T[key].append(sec)
                if r == 1:      # same columns, same shadow vector, same recurrence (other summation orders: to rounding, not to the bit)
                    Mp, Mj, ms = got[("plain", "full")][2], got[("jacobi", "full")][2], got[("single", "full")][2]
                    d = max(float((Mp[:, j] - ms[j]).norm() / ms[j].norm()) for j in range(k))
                    e = max(float((Mj[:, j] - XT[:, j]).norm() / XT[:, j].norm()) for j in range(k))
                    say(f"   k = {k}: plain batched iterate against the single solves' after {args.steps} iterations: largest relative distance {d:.1e}; "
                        f"Jacobi batched iterate against x_true: {e:.1e}")
                del got
            med = {key: statistics.median(v) for key, v in T.items()}
            for loop in ("plain", "jacobi"):
                if its[(loop, "full")] != k * args.steps or its[("single", "full")] != k * args.steps:
                    say(f"   {loop} k = {k}: NOT every column ran {args.steps} iterations: batched {its[(loop, 'full')]}, single {its[('single', 'full')]} column-iterations")
                a, b = med[(loop, "full")], med[("single", "full")]
                da, db = a - med[(loop, "one")], b - med[("single", "one")]
                ia, ib = its[(loop, "full")] - its[(loop, "one")], its[("single", "full")] - its[("single", "one")]
                say(f"   {loop} k = {k}: batched {its[(loop, 'full')] / a:10.0f} column-iterations/s   {k} x single {its[('single', 'full')] / b:10.0f}   "
                    f"ratio {b / a:.2f}x;   without set-up: {da / (ia / k) * 1e6:8.1f} us per batched iteration, batched {ia / da:10.0f}   "
                    f"{k} x single {ib / db:10.0f}   ratio {(ia / da) / (ib / db):.2f}x (cap {cap(loop, k, per_row):.2f}x)")
            del XT, B, cols
        A.destroy()
        lib.lcg_hip_trim()
        torch.cuda.empty_cache()
    lib.lcg_hip_set_shadow_seed(1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
