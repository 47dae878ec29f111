"""Batched IC(0) / ILU(0): the k-wide apply against k single applies, and batched PCG with the factor as M against k single
preconditioned solves and against batched Jacobi: writes profiles/multi_precond_lab.txt.

One MI355X, one process.  Systems: case_10K_A, the 1000 x 1000 five-point Laplacian, the 100^3 seven-point Laplacian, the 10^6
tridiagonal (scripts/ic0_lab.py's).  The yardsticks are the library's own earlier paths run in the same process on the same handle:
lcg_hip_ic0_solve, lcg_hip_solver_preconditioned with lcg_hip_ic0_mx, lcg_hip_lpcg_multi (Jacobi).

  * apply: for the exact solves and s = 2, 4, 8 sweeps, k = 2, 4, 8 -- one lcg_hip_ic0_solve_multi beside k x lcg_hip_ic0_solve, the
    two alternating in one loop between events on the library's stream, medians over --reps rounds after a warm-up round;
  * PCG to eps = 1e-8 on r.r / max(m.m, 1) from m = 0, columns b_j = A.x_j with x_j uniform in [-1, 1): lcg_hip_lpcg_multi_m (IC(0),
    exact and s = 2, 4) beside k sequential lcg_hip_solver_preconditioned(lcg_hip_ic0_mx) solves of the same columns at the same
    setting and beside lcg_hip_lpcg_multi on the same batch; host clock around work that ends in a synchronise; rounds alternate
    batch / singles / Jacobi; medians.  Column-solves per second = k / time.
  * one ILU(0) row per system (s = 2, k = 8).
An exact apply is bound by its level chain: where it takes more than 10 ms (the 1000^2 Laplacian: 17.5 ms; the tridiagonal: 1.1 s)
the exact legs are cut to what fits a short run -- k = 2 only, fewer rounds -- and the line says so.

    python scripts/multi_precond_lab.py [--out profiles/multi_precond_lab.txt] [--reps 5] [--only SUBSTRING]
"""
import argparse
import os
import statistics
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KS = (2, 4, 8)
APPLY_SWEEPS = (0, 2, 4, 8)
PCG_SWEEPS = (0, 2, 4)
EPS, CAP = 1e-8, 20000


def sweep_bytes(per_row, k):
    """A sweep's bytes per row and column by construction: the triangle's col / val (12 B per entry) and row pointer read once for
    all k columns; X read, Y(j) gathered (counted as one read of the vector) and Y(j+1) written per column."""
    return (12.0 * per_row + 4.0) / k + 24.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="a substring of the systems to run")
    args = ap.parse_args()
    import torch
    from liblcg_amd import _lib, api
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    import ic0_lab as R
    lib = _lib.load()
    assert torch.cuda.is_available(), "multi_precond_lab.py measures on the GPU: there is no other way to get these numbers"
    torch.cuda.set_device(0)
    api.use_torch_stream()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    n10, row, col, val, _ = read_coo_system(os.path.join(ROOT, "tests", "golden", "case_10K_A"))
    systems = (("case_10K_A", lambda: api.CsrMatrix.from_csr(*coo_to_csr_host(n10, row, col, val))),
               ("laplace2d 1000x1000", lambda: api.CsrMatrix.laplace2d(1000, 1000)),
               ("laplace3d 100^3", lambda: api.CsrMatrix.from_csr(*R.laplace3d(100))),
               ("tridiagonal 1e6", lambda: api.CsrMatrix.from_csr(*R.tridiag(1000000))))
    say(f"multi_precond_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}; medians of {args.reps} rounds after a "
        f"warm-up round, the legs of a round alternating; PCG from m = 0, abs_diff 0, eps {EPS:g}, cap {CAP}")
    losses = []
    for name, make in systems:
        if args.only and args.only not in name:
            continue
        A = make()
        n = A.n
        A.build_ic0(); A.build_jacobi()
        info0 = A.ic0_info()
        nnzL = len(A.ic0_factor_to_host()[1])
        per_row = nnzL / n
        say()
        say(f"== {name}: {n} rows, {A.nnz} entries, L {nnzL} entries ({per_row:.2f} per row), levels {info0['levels_lower']} / {info0['levels_upper']}")
        say("   a sweep's bytes per row and column by construction: " + ", ".join(f"k = {k}: {sweep_bytes(per_row, k):.1f}" for k in (1,) + KS)
            + "; ratio to k = 1: " + ", ".join(f"{sweep_bytes(per_row, k) / sweep_bytes(per_row, 1):.2f}" for k in KS))
        g = torch.Generator(device="cuda"); g.manual_seed(1)
        # ---- the apply
        x1 = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1
        y1 = torch.empty_like(x1)
        A.ic0_set_sweeps(0)
        A.ic0_solve(x1, y1); torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record(); A.ic0_solve(x1, y1); e1.record(); torch.cuda.synchronize()
        exact_ms = e0.elapsed_time(e1)
        slow_exact = exact_ms > 10.0
        for s in APPLY_SWEEPS:
            A.ic0_set_sweeps(s)
            exact_cut = s == 0 and slow_exact
            for k in ((2,) if exact_cut else KS):
                X = torch.rand((n, k), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
                Y = torch.empty_like(X)
                # a cut exact leg: one apply per round, two rounds after the warm-up round -- or, above half a second an apply, one
                # round and no warm-up round (the call below has loaded the code and made the work vectors)
                reps = (1 if exact_ms > 500.0 else 2) if exact_cut else args.reps
                warm = 0 if exact_cut and exact_ms > 500.0 else 1
                inner = 1 if exact_cut else 10
                A.ic0_solve_multi(X, Y); torch.cuda.synchronize()          # (the work vectors: not on the clock)
                tb, ts = [], []
                for r in range(warm + reps):
                    e = [ev() for _ in range(3)]
                    e[0].record()
                    for _ in range(inner):
                        A.ic0_solve_multi(X, Y)
                    e[1].record()
                    for _ in range(inner * k):
                        A.ic0_solve(x1, y1)
                    e[2].record()
                    torch.cuda.synchronize()
                    if r >= warm:
                        tb.append(e[0].elapsed_time(e[1]) * 1e3 / inner); ts.append(e[1].elapsed_time(e[2]) * 1e3 / inner)
                b, q = statistics.median(tb), statistics.median(ts)
                leg = "exact" if s == 0 else f"s={s}"
                note = f"  (exact apply of {exact_ms:.0f} ms: k = 2 only, {len(tb)} round(s))" if exact_cut else ""
                mark = "  LOSES" if b > q else ""
                say(f"   apply {leg:<5} k = {k}: batched {b:10.1f} us (min {min(tb):.1f}, max {max(tb):.1f})   {k} x single {q:10.1f} us "
                    f"(min {min(ts):.1f}, max {max(ts):.1f})   batched / singles = {b / q:.3f}{mark}{note}")
                if b > q:
                    losses.append(f"{name}: apply {leg} k = {k}: {b / q:.2f} of the singles' time")
                del X, Y
        # ---- PCG
        para = api.lcg_default_parameters(epsilon=EPS, abs_diff=0, max_iterations=CAP)
        for k in KS:
            XT = torch.rand((n, k), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
            B = torch.empty_like(XT)
            A.spmm(XT, B); api.synchronize()
            cols = [B[:, j].contiguous() for j in range(k)]
            for s in PCG_SWEEPS:
                if s == 0 and (exact_ms > 500.0 or (slow_exact and k > 2)):
                    continue
                A.ic0_set_sweeps(s)
                reps = 2 if s == 0 and slow_exact else args.reps
                tm, tq, tj = [], [], []
                for r in range(reps + 1):
                    M = torch.zeros_like(B)
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    im = api.lpcg_multi(A, M, B, para, precond="ic0")
                    api.synchronize(); t1 = time.perf_counter()
                    ms = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(k)]
                    torch.cuda.synchronize(); t2 = time.perf_counter()
                    iq = [api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ic0_mx", None, ms[j], cols[j], n, para, A) for j in range(k)]
                    api.synchronize(); t3 = time.perf_counter()
                    Mj = torch.zeros_like(B)
                    torch.cuda.synchronize(); t4 = time.perf_counter()
                    ij = api.lpcg_multi(A, Mj, B, para)
                    api.synchronize(); t5 = time.perf_counter()
                    if r:
                        tm.append(t1 - t0); tq.append(t3 - t2); tj.append(t5 - t4)
                    if r == 1:
                        assert all(i.ret == 0 for i in im) and all(i.ret == 0 for i in iq) and all(i.ret == 0 for i in ij), (im, iq, ij)
                        d = max(float((M[:, j] - ms[j]).norm() / ms[j].norm()) for j in range(k))
                    del M, ms, Mj
                a, q, jt = statistics.median(tm), statistics.median(tq), statistics.median(tj)
                leg = "exact" if s == 0 else f"s={s}"
                cut = f"  ({reps} rounds)" if reps != args.reps else ""
                say(f"   PCG {leg:<5} k = {k}: batched IC(0) {a * 1e3:9.2f} ms, {k / a:9.1f} column-solves/s (iterations {max(i.iterations for i in im)} longest, "
                    f"{min(i.iterations for i in im)} shortest)   {k} x single {q * 1e3:9.2f} ms, {k / q:9.1f} column-solves/s (iterations "
                    f"{max(i.iterations for i in iq)} / {min(i.iterations for i in iq)})   batch / singles {q / a:.2f}x{'  LOSES' if a > q else ''}   "
                    f"batched Jacobi {jt * 1e3:9.2f} ms ({max(i.iterations for i in ij)} iterations)   Jacobi / IC(0) time {jt / a:.2f}x"
                    f"{'  LOSES to Jacobi' if a > jt else ''}   iterates against the singles': {d:.1e}{cut}")
                if a > q:
                    losses.append(f"{name}: PCG {leg} k = {k}: {q / a:.2f}x the singles' column-solves per second")
                if a > jt:
                    losses.append(f"{name}: PCG {leg} k = {k}: {jt / a:.2f}x batched Jacobi's speed to convergence")
            if k == 8:      # one ILU(0) row
                A.build_ilu0(); A.ilu0_set_sweeps(2)
                tm, tq = [], []
                for r in range(args.reps + 1):
                    M = torch.zeros_like(B)
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    im = api.lpcg_multi(A, M, B, para, precond="ilu0")
                    api.synchronize(); t1 = time.perf_counter()
                    ms = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(k)]
                    torch.cuda.synchronize(); t2 = time.perf_counter()
                    iq = [api.lcg_solver_preconditioned("lcg_hip_csr_ax", "lcg_hip_ilu0_mx", None, ms[j], cols[j], n, para, A) for j in range(k)]
                    api.synchronize(); t3 = time.perf_counter()
                    if r:
                        tm.append(t1 - t0); tq.append(t3 - t2)
                    del M, ms
                a, q = statistics.median(tm), statistics.median(tq)
                say(f"   PCG ILU(0) s=2 k = 8: batched {a * 1e3:9.2f} ms, {k / a:9.1f} column-solves/s (iterations {max(i.iterations for i in im)})   "
                    f"8 x single {q * 1e3:9.2f} ms, {k / q:9.1f} column-solves/s   batch / singles {q / a:.2f}x{'  LOSES' if a > q else ''}")
                if a > q:
                    losses.append(f"{name}: PCG ILU(0) s=2 k = 8: {q / a:.2f}x the singles' column-solves per second")
            del XT, B, cols
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
