"""Batched BiCGStab against k single-vector solves, and batched ILU(0) against batched plain: writes
profiles/multi_bicgstab_lab.txt.

One MI355X, one process.  The yardsticks are the library's own paths in the same process on the same handle.
  * iteration rate: lcg_hip_lbicgstab_multi (plain) beside k sequential lcg_hip_solver(LCG_BICGSTAB) solves of the same columns,
    --steps iterations each (epsilon tiny, so nothing stops early), host clock around work that ends in a synchronise, the two legs
    alternating, medians over --reps rounds after a warm-up round: column-iterations per second, k = 2, 4, 8.  Systems: the
    1000 x 1000 convection-diffusion system (first-order upwinding, pe = 2: 5 entries per row) and lcg_hip_csr_generate_ex with
    symmetric = 0, constant diagonals and scrambled (33 entries per row), at --rows rows (0: the largest at which the k = 8 blocks
    fit beside the matrix, its single-vector plan and the single-vector work vectors -- multi_lab.py's bound at 1800 bytes per row);
  * time to the same residual on the convection-diffusion system, k = 8, columns b_j = A.x_j with x_j uniform in [-1, 1), from m = 0,
    r.r / max(m.m, 1) <= eps: plain beside ILU(0) applied exactly and by 2, 4, 8 sweeps.  Both forms iterate on x itself, so the stop
    rule is the same statement; |b - A.x| / |b| of the worst column is recomputed with lcg_hip_spmm and printed.

    python scripts/multi_bicgstab_lab.py [--rows N] [--steps 50] [--reps 5] [--out profiles/multi_bicgstab_lab.txt] [--skip-exact]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (2, 4, 8)
EPS, CAP = 1e-10, 20000
# vector words per row, column and iteration of the plain schedule: A.p (p, r0 read, v written) 3; s = r - ak v 3; A.s (s read as X
# and as U, t written) 3; the update (m, p, s, t, r0 read, m, r written) 7; the direction (r, p, v read, p written) 4
VECTOR_WORDS = 20


def bytes_per_row(k, per_row):
    """By construction, per row, column and iteration: two passes over col / val (12 B per entry) and the row pointer shared by k
    columns, the gathered rows of X counted once, and the 20 vector words of the plain schedule."""
    return 2.0 * (12.0 * per_row + 4.0) / k + 8.0 * VECTOR_WORDS


def convdiff(g, pe):
    import numpy as np
    import scipy.sparse as sp
    T1 = sp.diags([-1.0 - pe, 2.0 + pe, -1.0], [-1, 0, 1], shape=(g, g))
    T2 = sp.diags([-1.0 - pe / 2, 2.0 + pe / 2, -1.0], [-1, 0, 1], shape=(g, g))
    A = sp.csr_matrix(sp.kron(sp.identity(g), T1) + sp.kron(T2, sp.identity(g)))
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "multi_bicgstab_lab.txt"))
    ap.add_argument("--skip-exact", action="store_true", help="leave out the exact ILU(0) leg (its level chain takes seconds per solve)")
    args = ap.parse_args()
    import torch
    from liblcg_amd import _lib, api
    assert torch.cuda.is_available(), "multi_bicgstab_lab.py measures on the GPU: there is no other way to get these numbers"
    lib = _lib.load()
    assert lib.lcg_hip_init(0) == 0
    api.use_torch_stream()
    free, total = torch.cuda.mem_get_info()
    rows = args.rows or min((2 ** 31 - 1) // 34, int(0.8 * free / 1800)) // 1_000_000 * 1_000_000
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"multi_bicgstab_lab: {torch.cuda.get_device_name(0)}, {free / 2**30:.0f} GiB free of {total / 2**30:.0f}; {time.strftime('%Y-%m-%d %H:%M:%S')}; "
        f"generated patterns at {rows} rows{' (the largest at which k = 8 fits)' if not args.rows else ' (--rows)'}; medians of {args.reps} "
        f"rounds after a warm-up round, {args.steps} iterations per solve")
    losses = []
    cd = convdiff(1000, 2.0)
    systems = (("convection-diffusion 1000^2", lambda: api.CsrMatrix.from_csr(*cd)),
               ("constant diagonals, non-symmetric", lambda: api.CsrMatrix.generate(rows, 16, 131072, False, 1, 0.01, pattern=api.GEN_DIAGONALS)),
               ("scrambled, non-symmetric", lambda: api.CsrMatrix.generate(rows, 16, 0, False, 1, 0.01, pattern=api.GEN_SCRAMBLED)))
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    for name, make in systems:
        A = make()
        n = A.n
        per_row = A.nnz / n
        say()
        say(f"== {name}: {n} rows, {A.nnz} entries ({per_row:.2f} per row)")
        say("   bytes per row, column and iteration by construction: " + ", ".join(f"k = {k}: {bytes_per_row(k, per_row):.0f}" for k in (1,) + KS)
            + "; cap of the gain over k = 1: " + ", ".join(f"k = {k}: {bytes_per_row(1, per_row) / bytes_per_row(k, per_row):.2f}x" for k in KS))
        para = api.lcg_default_parameters(epsilon=1e-300, abs_diff=0, max_iterations=args.steps)
        for k in KS:
            XT = torch.rand((n, k), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
            B = torch.empty_like(XT)
            A.spmm(XT, B); api.synchronize()
            cols = [B[:, j].contiguous() for j in range(k)]
            tb, ts = [], []
            for r in range(args.reps + 1):
                M = torch.zeros_like(B)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                ib = api.lbicgstab_multi(A, M, B, para)
                api.synchronize(); t1 = time.perf_counter()
                ms = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(k)]
                torch.cuda.synchronize(); t2 = time.perf_counter()
                iq = [api.lcg_solver("lcg_hip_csr_ax", None, ms[j], cols[j], n, para, A, api.LCG_BICGSTAB) for j in range(k)]
                api.synchronize(); t3 = time.perf_counter()
                if r:
                    tb.append(t1 - t0); ts.append(t3 - t2)
                if r == 1:
                    short = [i.iterations for i in list(ib) + iq if i.iterations != args.steps]
                    d = max(float((M[:, j] - ms[j]).norm() / ms[j].norm()) for j in range(k))
                del M, ms
            b, q = statistics.median(tb), statistics.median(ts)
            rate_b, rate_q = k * args.steps / b, k * args.steps / q
            cap = bytes_per_row(1, per_row) / bytes_per_row(k, per_row)
            say(f"   k = {k}: batched {b * 1e3:9.2f} ms (min {min(tb) * 1e3:.2f}, max {max(tb) * 1e3:.2f}), {rate_b:10.1f} column-iterations/s, "
                f"{bytes_per_row(k, per_row) * n * rate_b / 1e12:.2f} TB/s by construction   {k} x single {q * 1e3:9.2f} ms (min {min(ts) * 1e3:.2f}, "
                f"max {max(ts) * 1e3:.2f}), {rate_q:10.1f} column-iterations/s   batch / singles {q / b:.2f}x of a cap of {cap:.2f}x"
                f"{'  LOSES' if b > q else ''}   iterates against the singles': {d:.1e}"
                + (f"   (!) solves that did not run {args.steps} iterations: {short}" if short else ""))
            if b > q:
                losses.append(f"{name}: k = {k}: {q / b:.2f}x the singles' column-iterations per second")
            del XT, B, cols
        if name.startswith("convection"):
            k = 8
            A.build_ilu0()
            XT = torch.rand((n, k), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
            B = torch.empty_like(XT)
            A.spmm(XT, B); api.synchronize()
            bn = B.norm(dim=0)
            para = api.lcg_default_parameters(epsilon=EPS, abs_diff=0, max_iterations=CAP)
            base = None
            for leg, sweeps in (("plain", None), ("s=2", 2), ("s=4", 4), ("s=8", 8), ("exact", 0)):
                if leg == "exact" and args.skip_exact:
                    continue
                if sweeps is not None:
                    A.ilu0_set_sweeps(sweeps)
                reps = 1 if leg == "exact" else args.reps
                tt = []
                for r in range(reps + (0 if leg == "exact" else 1)):
                    M = torch.zeros_like(B)
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    infos = api.lbicgstab_multi(A, M, B, para, precond=None if sweeps is None else "ilu0")
                    api.synchronize(); t1 = time.perf_counter()
                    if r or leg == "exact":
                        tt.append(t1 - t0)
                    Y = torch.empty_like(B)
                    A.spmm(M, Y); api.synchronize()
                    true = float(((B - Y).norm(dim=0) / bn).max())
                    del M, Y
                t = statistics.median(tt)
                its = [i.iterations for i in infos]
                ok = all(i.ret == 0 for i in infos)
                if leg == "plain":
                    base = t
                mark = "" if leg == "plain" else f"   plain / this {base / t:.2f}x{'  LOSES to plain' if t > base else ''}"
                say(f"   to eps {EPS:g}, k = 8, {leg:<5}: {t * 1e3:10.2f} ms ({len(tt)} round(s)), iterations {max(its)} longest / {min(its)} shortest, "
                    f"{'all converged' if ok else 'codes ' + str([i.ret for i in infos])}, worst |b - A.x| / |b| = {true:.2e}{mark}")
                if leg != "plain" and t > base:
                    losses.append(f"{name}: ILU(0) {leg} k = 8: {base / t:.2f}x batched plain's speed to eps {EPS:g}")
            del XT, B
        A.destroy()
        lib.lcg_hip_trim()
        torch.cuda.empty_cache()
    say()
    say("where the batch, or the factor, loses:")
    for l in losses or ["(nowhere)"]:
        say("   " + l)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
