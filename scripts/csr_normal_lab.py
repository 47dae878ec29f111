"""Sparse least squares on a rectangular CSR matrix (include/lcg_hip_staging_csr_normal.h) measured on one MI355X, in one
process, the two sides of every comparison alternating, medians of `rounds` rounds after a warm-up round.

Systems (every row of K draws t columns uniformly; duplicates inside a row are kept): a tall K (M = 8 N) at N = 10^6 model parameters and,
small enough for K^T.K to be formed, at N = 125,000; a square and a wide K at N = 10^6, each stacked on 0.1 I (the damping rows of
K' = [K; sqrt(lambda) I], which also leave no column empty); the 578 x 513 system of the tests (65 data rows of 12 entries stacked on
0.5 I) as the launch-bound one; and a K of 10^6 rows whose column 0 is dense, for the build.

  1. one application of K^T.K by lcg_hip_csr_ata (two products) against lcg_hip_spmv with the explicitly formed CSR K^T.K -- the route
     a user has without this feature; its entries per row and its host build time (scipy) stand beside it.  Where K^T.K would hold
     more than --form-max entries it is not formed and the line says so.
  2. lcg_hip_csr_ata_multi at k = 2, 4, 8 against k single applications.
  3. column-iterations per second of the batched CG / PCG / SPG against k single solves through the callbacks, capped, from zeros.
  4. build_ms and extra_bytes of the normal state, and the dense-column build against the first lcg_hip_spmv_op(layout = 1) of a
     square matrix of the same entry count (the transposition that exists without this feature, its first product included).

Bytes by construction of one application: K and K^T once each (12 B per entry, 4 B per row pointer), x read, t written and read, y
written: 24 nnz + 4 (M + N) + 8 k (2 M + 2 N).  "of 6.3 TB/s" is that count over the measured time over the copy rate of the
microarchitecture notes: a whole-call figure, launches included, not a kernel's share of peak.

    python scripts/csr_normal_lab.py [--out profiles/csr_normal_lab.txt] [--rounds 3] [--only SUBSTRING] [--form-max 100000000]
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
COPY_RATE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="a substring of a system's name")
    ap.add_argument("--form-max", type=float, default=1e8, help="K^T.K is formed on the host up to this many entries")
    ap.add_argument("--cap", type=int, default=30)
    args = ap.parse_args()
    import torch
    import scipy.sparse as sp
    from liblcg_amd import api
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    def draw(M, N, t, seed, dense_col=False, stack=None):
        """(rowptr, col, val) on the device: t sorted columns per row, values uniform(-1, 1)."""
        gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
        col = torch.randint(0, N, (M, t), device="cuda", generator=gen, dtype=torch.int32)
        if dense_col:
            col[:, 0] = 0
        col = torch.sort(col, dim=1).values
        val = torch.rand((M, t), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        rp = torch.arange(0, (M + 1) * t, t, dtype=torch.int32, device="cuda")
        col, val = col.reshape(-1), val.reshape(-1)
        if stack is not None:
            rp = torch.cat([rp, rp[-1] + torch.arange(1, N + 1, dtype=torch.int32, device="cuda")])
            col = torch.cat([col, torch.arange(N, dtype=torch.int32, device="cuda")])
            val = torch.cat([val, torch.full((N,), stack, dtype=torch.float64, device="cuda")])
        return rp.contiguous(), col.contiguous(), val.contiguous()

    SYSTEMS = [("tall_8Mx1M_t8", 8_000_000, 1_000_000, 8, None), ("tall_1Mx125K_t8", 1_000_000, 125_000, 8, None),
               ("square_1Mx1M_t8_on_0.1I", 1_000_000, 1_000_000, 8, 0.1), ("wide_250Kx1M_t16_on_0.1I", 250_000, 1_000_000, 16, 0.1),
               ("launch_bound_578x513", 65, 513, 12, 0.5)]

    say(f"csr_normal_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    say(f"medians of {args.rounds} rounds after a warm-up round, the sides alternating; ratio > 1: the new path is faster; losses are marked")
    say()
    for name, M0, N, t, stack in SYSTEMS:
        if args.only and args.only not in name:
            continue
        rp, ci, v = draw(M0, N, t, 7 * N + M0, stack=stack)
        M = int(rp.shape[0]) - 1
        nnz = int(ci.shape[0])
        K = api.CsrMatrix.from_csr(rp, ci, v, n_cols=N)
        K.build_normal()
        info = K.normal_info()
        say(f"{name}: K {M} x {N}, {nnz} entries ({nnz / M:.1f} per row, {nnz / N:.1f} per column, longest column {info['longest_column']}); normal state: "
            f"build {info['build_ms']:.2f} ms, {info['extra_bytes'] / 2**20:.1f} MiB beside the matrix's {12 * nnz / 2**20:.1f} MiB")
        gen = torch.Generator(device="cuda"); gen.manual_seed(5)
        xt = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen) + 1
        x = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen)
        y = torch.empty_like(x)
        reps = 200 if nnz < 1_000_000 else 20
        model1 = 24 * nnz + 4 * (M + N) + 8 * (2 * M + 2 * N)

        # 1. against the formed K^T.K
        est = min(M0 * t * t + (N if stack is not None else 0), N * N)
        formed = None
        if est <= args.form_max:
            t0 = time.perf_counter()
            Kh = sp.csr_matrix((v.cpu().numpy(), ci.cpu().numpy(), rp.cpu().numpy()), shape=(M, N))
            G = (Kh.T @ Kh).tocsr(); G.sort_indices()
            host_s = time.perf_counter() - t0
            formed = api.CsrMatrix.from_csr(G.indptr.astype(np.int32), G.indices.astype(np.int32), G.data)
            gnnz = G.nnz
            del G, Kh
        ta, tf = [], []
        for r in range(args.rounds + 1):
            a = timed(lambda: K.ata(x, y), reps)
            f = timed(lambda: formed.spmv(x, y), reps) if formed is not None else None
            if r:
                ta.append(a); tf.append(f)
        ma = statistics.median(ta)
        line = (f"  1. one application: lcg_hip_csr_ata {ma * 1e6:9.1f} us (spread {(max(ta) - min(ta)) / ma:5.1%}; {model1 / 1e6:.1f} MB by construction, "
                f"{model1 / ma / 1e12:.2f} TB/s = {model1 / ma / COPY_RATE:.0%} of 6.3 TB/s)")
        if formed is not None:
            mf = statistics.median(tf)
            line += (f"; the formed K^T.K ({gnnz / N:.1f} entries per row, {12 * gnnz / 2**20:.1f} MiB, built on the host in {host_s:.2f} s) {mf * 1e6:9.1f} us; "
                     f"ratio {mf / ma:5.2f}{'' if mf >= ma else '  ** LOSS **'}")
            formed.destroy(); formed = None
        else:
            line += f"; K^T.K not formed (about {est / N:.0f} entries per row, {12 * est / 2**30:.1f} GiB)"
        say(line)

        # 2. k wide against k single applications
        for k in KS:
            Xk = torch.rand((N, k), dtype=torch.float64, device="cuda", generator=gen)
            Yk = torch.empty_like(Xk)
            tm, ts = [], []
            for r in range(args.rounds + 1):
                a = timed(lambda: K.ata_multi(Xk, Yk), reps)
                s = timed(lambda: [K.ata(x, y) for _ in range(k)], max(1, reps // k))
                if r:
                    tm.append(a); ts.append(s)
            mm, ms = statistics.median(tm), statistics.median(ts)
            modelk = 24 * nnz + 4 * (M + N) + 8 * k * (2 * M + 2 * N)
            say(f"  2. k={k}: lcg_hip_csr_ata_multi {mm * 1e6:9.1f} us (spread {(max(tm) - min(tm)) / mm:5.1%}; {modelk / 1e6:.1f} MB by construction, "
                f"{modelk / mm / 1e12:.2f} TB/s = {modelk / mm / COPY_RATE:.0%} of 6.3 TB/s)  {k} single applications {ms * 1e6:9.1f} us  "
                f"ratio {ms / mm:5.2f}{'' if ms >= mm else '  ** LOSS **'}")
        # the two halves of the k = 8 product apart: K.X, then K^T over its long rows
        X8 = torch.rand((N, 8), dtype=torch.float64, device="cuda", generator=gen)
        T8 = torch.empty((M, 8), dtype=torch.float64, device="cuda"); Y8 = torch.empty_like(X8)
        K.spmm(X8, T8)
        th = [(timed(lambda: K.spmm(X8, T8), reps), timed(lambda: K.spmm_t(T8, Y8), reps)) for _ in range(args.rounds + 1)][1:]
        h0, h1 = statistics.median([a for a, _ in th]), statistics.median([b for _, b in th])
        b0, b1 = 12 * nnz + 4 * M + 64 * (M + N), 12 * nnz + 4 * N + 64 * (M + N)
        say(f"     k=8 halves: K.X {h0 * 1e6:9.1f} us ({b0 / h0 / 1e12:.2f} TB/s by construction, rows of {nnz / M:.1f}); K^T.T {h1 * 1e6:9.1f} us "
            f"({b1 / h1 / 1e12:.2f} TB/s, rows of {nnz / N:.1f})")
        del X8, T8, Y8

        # 3. the loops
        b = torch.empty(N, dtype=torch.float64, device="cuda")
        K.ata(xt, b); api.synchronize()
        try:
            K.build_jacobi_normal()
            solvers = (("CG", 0), ("PCG", 1), ("SPG", 6))
        except api.LcgHipError:
            say("  3. (a column of K is empty: no Jacobi, no PCG)")
            solvers = (("CG", 0), ("SPG", 6))
        low, hig = torch.full((N,), 0.5, dtype=torch.float64, device="cuda"), torch.full((N,), 1.6, dtype=torch.float64, device="cuda")
        para = api.lcg_default_parameters(epsilon=1e-300, abs_diff=0, max_iterations=args.cap)
        scales = [1.0, 0.8, 1.2, 0.7, 1.3, 0.9, 1.1, 0.6]
        for sname, sid in solvers:
            for k in KS:
                B = (b[:, None] * torch.tensor(scales[:k], dtype=torch.float64, device="cuda")[None, :]).contiguous()
                cols = [B[:, j].contiguous() for j in range(k)]
                tb, ts, ib, isg = [], [], 0, 0
                for r in range(args.rounds + 1):
                    Mk = torch.zeros_like(B)
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    if sid == 0:
                        infos = api.csr_normal_lcg_multi(K, Mk, B, para)
                    elif sid == 1:
                        infos = api.csr_normal_lpcg_multi(K, Mk, B, para)
                    else:
                        infos = api.csr_normal_solver_constrained_multi(K, Mk, B, low, hig, para, api.LCG_SPG)
                    torch.cuda.synchronize(); t1 = time.perf_counter()
                    singles = []
                    for j in range(k):
                        m = torch.zeros(N, dtype=torch.float64, device="cuda")
                        if sid == 0:
                            singles.append(api.lcg_solver("lcg_hip_csr_ata_ax", None, m, cols[j], N, para, K, api.LCG_CG))
                        elif sid == 1:
                            singles.append(api.lcg_solver_preconditioned("lcg_hip_csr_ata_ax", "lcg_hip_csr_jacobi_normal_mx", None, m, cols[j], N, para, K))
                        else:
                            singles.append(api.lcg_solver_constrained("lcg_hip_csr_ata_ax", None, m, cols[j], low, hig, N, para, K, api.LCG_SPG))
                    torch.cuda.synchronize(); t2 = time.perf_counter()
                    if r:
                        tb.append(t1 - t0); ts.append(t2 - t1)
                    ib, isg = sum(i.iterations for i in infos), sum(i.iterations for i in singles)
                mb, msg = statistics.median(tb), statistics.median(ts)
                ratio = (ib / mb) / (isg / msg)
                say(f"  3. {sname:3s} k={k}: batch {ib / mb:10.0f} column-iterations/s, {mb * 1e3:9.2f} ms to the cap of {args.cap} (spread {(max(tb) - min(tb)) / mb:5.1%}; {ib} steps)  "
                    f"{k} single solves {isg / msg:10.0f}, {msg * 1e3:9.2f} ms ({isg} steps)  ratio {ratio:5.2f}{'' if ratio >= 1.0 else '  ** LOSS **'}")
        info = K.normal_info()
        say(f"  4. normal state after the loops: {info['extra_bytes'] / 2**20:.1f} MiB (K^T {12 * nnz / 2**20:.1f} MiB, the M x 8 block {64 * M / 2**20:.1f} MiB)")
        say()
        K.destroy()
        del rp, ci, v
        torch.cuda.empty_cache()

    # 4. the build with a dense column, against the transposition the library has had
    if not args.only or "dense_column" in args.only:
        M, N, t = 1_000_000, 125_000, 8
        say(f"dense_column: K {M} x {N}, {t} per row, column 0 in every row ({M} entries in one row of K^T); against the first lcg_hip_spmv_op(layout = 1) "
            f"of a square {M} x {M} matrix with {t} per row (k_row_sort: one thread per row)")
        bs, os_ = [], []
        for r in range(args.rounds + 1):
            rp, ci, v = draw(M, N, t, 99 + r, dense_col=True)
            K = api.CsrMatrix.from_csr(rp, ci, v, n_cols=N)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            K.build_normal()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            info = K.normal_info()
            K.destroy()
            rp, ci, v = draw(M, M, t, 199 + r)
            A = api.CsrMatrix.from_csr(rp, ci, v)
            xs = torch.ones(M, dtype=torch.float64, device="cuda"); ys = torch.empty_like(xs)
            A.spmv(xs, ys)
            torch.cuda.synchronize(); t2 = time.perf_counter()
            api._chk(api.L.load().lcg_hip_spmv_op(A.h, xs.data_ptr(), ys.data_ptr(), 1, 0), "spmv_op")
            torch.cuda.synchronize(); t3 = time.perf_counter()
            A.destroy()
            if r:
                bs.append((t1 - t0, info["build_ms"])); os_.append(t3 - t2)
        mb, mo = statistics.median([a for a, _ in bs]), statistics.median(os_)
        say(f"  4. lcg_hip_csr_build_normal {mb * 1e3:8.2f} ms (build_ms {statistics.median([b for _, b in bs]):.2f}, longest column {info['longest_column']}, "
            f"{info['extra_bytes'] / 2**20:.1f} MiB)  first A^T.x of the square matrix {mo * 1e3:8.2f} ms  ratio {mo / mb:5.2f}{'' if mo >= mb else '  ** LOSS **'}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
