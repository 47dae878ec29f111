"""Complex128 dense operators over k = 2, 4, 8 right-hand sides against k single products and solves of the same handle, in one
process: clcg_hip_dense_matmat (K.X, K^T.X) against k calls of clcg_hip_dense_matvec, and
clcg_hip_dense_lbicg_sym_multi / clcg_hip_dense_lpcg_multi against k CLCG_BICG_SYM / CLCG_PCG solves on clcg_hip_dense_ax (and
clcg_hip_dense_jacobi_mx).  The single-vector side is code this change leaves untouched.

Shapes: 100^2 and 1000^2 (sample3's own sizes: launch-bound), 8192^2 (1.07 GB), 16384^2 (4.3 GB).  K is the tests' family, made on
the device: G^T.G / n + 0.02 I + 0.1i (H^T.H / n + 0.2 I), symmetrised -- complex-symmetric, not Hermitian, condition number about 30.

The method of scripts/dense_lab.py: per leg the mean device time of `reps` back-to-back calls between two events on the library's
stream after a warm-up; three rounds, each round every leg of a shape in turn (batched and single alternate); medians, and the
spread (max - min) / median of the rounds.  Fraction of the read rate: K's 16 N^2 bytes, read once by the batched product, over the
median, against the box's own read rate taken in the same run (the sum of 4 GiB).  ratio = k single / batched (> 1: the batch is
faster).

Loops: column-iterations per second (k x iterations / wall clock) of the batched loop over `--its` iterations from M = 0 against k
single solves of as many iterations, with the launches per iteration of both sides (lcg_hip_last_launches).

    python scripts/dense_multi_cplx_lab.py [--out profiles/dense_multi_cplx_lab.txt] [--rounds 3] [--only SUBSTRING] [--no-loops]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [100, 1000, 8192, 16384]
KS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--its", type=int, default=30)
    ap.add_argument("--only", default=None, help="a substring of 'NxN' to run")
    ap.add_argument("--no-loops", action="store_true")
    args = ap.parse_args()
    import torch
    from liblcg_amd import _lib, api
    lib = _lib.load()
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    api.use_torch_stream()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(call, reps):
        call(); call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record(); b.synchronize()
        return a.elapsed_time(b) * 1e3 / reps          # microseconds

    def read_rate():
        big = torch.ones(1 << 29, dtype=torch.float64, device="cuda")      # a pure read: the sum of 4 GiB
        for _ in range(2):
            big.sum()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            big.sum()
        torch.cuda.synchronize()
        return 5 * big.numel() * 8 / (time.perf_counter() - t0) / 1e9

    def launches():
        vec, scal, prod = C.c_int(), C.c_int(), C.c_int()
        lib.lcg_hip_last_launches(C.byref(vec), C.byref(scal), None, C.byref(prod))
        return vec.value, scal.value, prod.value

    say(f"dense_multi_cplx_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    rate = read_rate()
    say(f"this box's read rate in this run (sum of 4 GiB, as bench.py --full): {rate:.0f} GB/s")
    say(f"medians of {args.rounds} rounds; spread = (max - min) / median; ratio = k single products (solves) / one batched (> 1: the batch is faster)")
    say()
    for N in SIZES:
        tag = f"{N}x{N}"
        if args.only and args.only not in tag:
            continue
        g = torch.Generator(device="cuda"); g.manual_seed(5000 + N)
        eye = torch.eye(N, dtype=torch.float64, device="cuda")
        G = torch.rand((N, N), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
        Kr = G.T @ G / N + 0.02 * eye
        G = torch.rand((N, N), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
        Ki = 0.1 * (G.T @ G / N + 0.2 * eye)
        del G, eye
        K = torch.complex((Kr + Kr.T) / 2, (Ki + Ki.T) / 2).contiguous()
        del Kr, Ki
        D = api.DenseMatrix.from_array(K)
        del K
        torch.cuda.empty_cache()
        D.build_jacobi(False)
        mat = 16 * N * N
        reps = int(min(200, max(10, 2e9 / mat)))
        x = torch.ones(N, dtype=torch.complex128, device="cuda"); y = torch.empty(N, dtype=torch.complex128, device="cuda")
        h = D.h
        say(f"{tag}: K = {mat / 2**20:.1f} MiB, {reps} calls per timing")
        for k in KS:
            X = torch.ones((N, k), dtype=torch.complex128, device="cuda"); Y = torch.empty((N, k), dtype=torch.complex128, device="cuda")
            px, py, pX, pY = x.data_ptr(), y.data_ptr(), X.data_ptr(), Y.data_ptr()

            def single(f):
                def call():
                    rc = 0
                    for _ in range(k):
                        rc |= f()
                    return rc
                return call
            legs = [("K.X", lambda: lib.clcg_hip_dense_matmat(h, k, pX, pY, 0, 0), single(lambda: lib.clcg_hip_dense_matvec(h, px, py, 0, 0))),
                    ("K^T.X", lambda: lib.clcg_hip_dense_matmat(h, k, pX, pY, 1, 0), single(lambda: lib.clcg_hip_dense_matvec(h, px, py, 1, 0)))]
            res = {i: ([], []) for i in range(len(legs))}
            kern = {}
            for _ in range(args.rounds):
                for i, (label, batched, singles) in enumerate(legs):
                    assert batched() == 0 and singles() == 0
                    res[i][0].append(timed(batched, reps))
                    res[i][1].append(timed(singles, max(2, reps // k)))
                    kern[i] = (D.multi_last_kernel, D.last_kernel)
            for i, (label, _, _) in enumerate(legs):
                mb, ms = statistics.median(res[i][0]), statistics.median(res[i][1])
                sb = (max(res[i][0]) - min(res[i][0])) / mb
                ratio = ms / mb
                mark = "" if ratio >= 1.0 else "  ** LOSS **"
                say(f"  k={k} {label:6s} batched {mb:10.1f} us (spread {sb:5.1%}, K = {mat / mb / 1e3:6.0f} GB/s = "
                    f"{mat / mb / 1e3 / rate:5.1%} of the read rate)  {k} single {ms:10.1f} us  ratio {ratio:5.2f}"
                    f"  (round by round: {', '.join(f'{s / b:.2f}' for b, s in zip(*res[i]))}){mark}  [{kern[i][0]} | {kern[i][1]}]")
            del X, Y
        if not args.no_loops:
            xt = torch.complex(torch.rand(N, dtype=torch.float64, device="cuda", generator=g) + 1,
                               torch.rand(N, dtype=torch.float64, device="cuda", generator=g) + 1)
            b = torch.empty_like(xt)
            D.matvec(xt, b)
            para = api.clcg_default_parameters(epsilon=1e-300, abs_diff=0, max_iterations=args.its)
            loops = [("BiCG-sym", api.dense_clbicg_sym_multi,
                      lambda m, bj: api.clcg_solver("clcg_hip_dense_ax", None, m, bj, N, para, D, api.CLCG_BICG_SYM)),
                     ("PCG", api.dense_clpcg_multi,
                      lambda m, bj: api.clcg_solver_preconditioned("clcg_hip_dense_ax", "clcg_hip_dense_jacobi_mx", None, m, bj, N, para, D))]
            for name, multi, one in loops:
                for k in KS:
                    B = (b[:, None] * torch.arange(1, k + 1, dtype=torch.float64, device="cuda")[None, :]).contiguous()
                    rb, rs = [], []
                    lb = ls = None
                    for r in range(args.rounds + 1):
                        Mb = torch.zeros_like(B)
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        infos = multi(D, Mb, B, para)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        lb = launches()
                        its = 0
                        t2 = time.perf_counter()
                        for j in range(k):
                            m = torch.zeros_like(xt)
                            bj = B[:, j].contiguous()
                            its += one(m, bj).iterations
                        torch.cuda.synchronize()
                        t3 = time.perf_counter()
                        ls = launches()
                        if r:
                            rb.append(sum(i.iterations for i in infos) / (t1 - t0)); rs.append(its / (t3 - t2))
                    mb, ms = statistics.median(rb), statistics.median(rs)
                    ratio = mb / ms
                    mark = "" if ratio >= 1.0 else "  ** LOSS **"
                    say(f"  {name} k={k}: batched {mb:9.0f} column-iterations/s (spread {(max(rb) - min(rb)) / mb:5.1%}; K = "
                        f"{mb / k * mat / 1e9:5.0f} GB/s = {mb / k * mat / 1e9 / rate:5.1%} of the read rate; per iteration "
                        f"{lb[2] / args.its:.1f} operator kernels + {lb[0] / args.its:.1f} passes)  {k} single solves {ms:9.0f} (per iteration "
                        f"{ls[2] / args.its:.1f} products + {(ls[0] + ls[1]) / args.its:.1f} passes and steps)  ratio {ratio:5.2f}{mark}"
                        f"  [{D.multi_last_kernel} | {D.last_kernel}]")
        say()
        D.destroy()
        del D
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
