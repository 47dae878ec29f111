"""Dense operators over k = 2, 4, 8 right-hand sides against k single products of the same handle, in one process:
lcg_hip_dense_matmat (K.X, K^T.X) and lcg_hip_dense_ata_multi against k calls of lcg_hip_dense_matvec / lcg_hip_dense_ata on the
automatic path, and lcg_hip_dense_lcg_multi against k LCG_CG solves on lcg_hip_dense_ata_ax.  The single-vector side is code this
change leaves untouched.

Shapes: 1000 x 800 (sample1: launch-bound), 16384 x 2048 (the widest rows of the single one-pass K^T.K.x), 200000 x 200, 8192^2
(512 MiB: beyond the Infinity Cache), 20000 x 16000 (2.56 GB).

The method of scripts/dense_lab.py: per leg the mean device time of `reps` back-to-back calls between two events on the library's
stream after a warm-up; three rounds, each round every leg of a shape in turn (batched and single alternate); medians, and the
spread (max - min) / median of the rounds.  Fraction of the read rate: K's bytes as the batched product reads them (8 M N once;
K^T.K.X twice) over the median, against the box's own read rate taken in the same run (the sum of 4 GiB).  ratio = k single / batched
(> 1: the batch is faster).

CG: column-iterations per second (k x iterations / wall clock) of lcg_hip_dense_lcg_multi over 200 iterations from M = 0 against k
LCG_CG solves of 200 iterations on lcg_hip_dense_ata_ax, with the launches per iteration of both sides (lcg_hip_last_launches).

    python scripts/dense_multi_lab.py [--out profiles/dense_multi_lab.txt] [--rounds 3] [--only SUBSTRING] [--no-cg]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1000, 800), (16384, 2048), (200000, 200), (8192, 8192), (20000, 16000)]
KS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="a substring of 'MxN' to run")
    ap.add_argument("--no-cg", action="store_true")
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

    say(f"dense_multi_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    rate = read_rate()
    say(f"this box's read rate in this run (sum of 4 GiB, as bench.py --full): {rate:.0f} GB/s")
    say(f"medians of {args.rounds} rounds; spread = (max - min) / median; ratio = k single products (solves) / one batched (> 1: the batch is faster)")
    say()
    for (M, N) in SHAPES:
        tag = f"{M}x{N}"
        if args.only and args.only not in tag:
            continue
        g = torch.Generator(device="cuda"); g.manual_seed(M * 31 + N)
        K = torch.rand((M, N), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
        D = api.DenseMatrix.from_array(K)
        del K
        mat = 8 * M * N
        reps = int(min(200, max(10, 2e9 / mat)))
        xN = torch.ones(N, dtype=torch.float64, device="cuda"); xM = torch.ones(M, dtype=torch.float64, device="cuda")
        yN = torch.empty(N, dtype=torch.float64, device="cuda"); yM = torch.empty(M, dtype=torch.float64, device="cuda")
        h = D.h
        say(f"{tag}: K = {mat / 2**20:.1f} MiB, {reps} calls per timing")
        for k in KS:
            XN = torch.ones((N, k), dtype=torch.float64, device="cuda"); XM = torch.ones((M, k), dtype=torch.float64, device="cuda")
            YN = torch.empty((N, k), dtype=torch.float64, device="cuda"); YM = torch.empty((M, k), dtype=torch.float64, device="cuda")
            pxN, pxM, pyN, pyM = xN.data_ptr(), xM.data_ptr(), yN.data_ptr(), yM.data_ptr()
            pXN, pXM, pYN, pYM = XN.data_ptr(), XM.data_ptr(), YN.data_ptr(), YM.data_ptr()

            def single(f):
                def call():
                    rc = 0
                    for _ in range(k):
                        rc |= f()
                    return rc
                return call
            legs = [("K.X", 1, lambda: lib.lcg_hip_dense_matmat(h, k, pXN, pYM, 0), single(lambda: lib.lcg_hip_dense_matvec(h, pxN, pyM, 0))),
                    ("K^T.X", 1, lambda: lib.lcg_hip_dense_matmat(h, k, pXM, pYN, 1), single(lambda: lib.lcg_hip_dense_matvec(h, pxM, pyN, 1))),
                    ("K^T.K.X", 2, lambda: lib.lcg_hip_dense_ata_multi(h, k, pXN, pYN), single(lambda: lib.lcg_hip_dense_ata(h, pxN, pyN)))]
            res = {i: ([], []) for i in range(len(legs))}
            kern = {}
            for _ in range(args.rounds):
                for i, (label, passes, batched, singles) in enumerate(legs):
                    assert batched() == 0 and singles() == 0
                    res[i][0].append(timed(batched, reps))
                    res[i][1].append(timed(singles, max(2, reps // k)))
                    kern[i] = (D.multi_last_kernel, D.last_kernel)
            for i, (label, passes, _, _) in enumerate(legs):
                mb, ms = statistics.median(res[i][0]), statistics.median(res[i][1])
                sb = (max(res[i][0]) - min(res[i][0])) / mb
                ratio = ms / mb
                mark = "" if ratio >= 1.0 else "  ** LOSS **"
                say(f"  k={k} {label:8s} batched {mb:10.1f} us (spread {sb:5.1%}, K x {passes} = {passes * mat / mb / 1e3:6.0f} GB/s = "
                    f"{passes * mat / mb / 1e3 / rate:5.1%} of the read rate)  {k} single {ms:10.1f} us  ratio {ratio:5.2f}"
                    f"  (round by round: {', '.join(f'{s / b:.2f}' for b, s in zip(*res[i]))}){mark}  [{kern[i][0]} | {kern[i][1]}]")
            del XN, XM, YN, YM
        if not args.no_cg:
            xt = torch.rand(N, dtype=torch.float64, device="cuda", generator=g) + 1
            b = torch.empty_like(xt)
            D.ata(xt, b)
            para = api.lcg_default_parameters(epsilon=1e-300, abs_diff=0, max_iterations=200)
            for k in KS:
                B = (b[:, None] * torch.arange(1, k + 1, dtype=torch.float64, device="cuda")[None, :]).contiguous()
                rb, rs = [], []
                lb = ls = None
                for r in range(args.rounds + 1):
                    Mb = torch.zeros_like(B)
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    infos = api.dense_lcg_multi(D, Mb, B, para)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    lb = launches()
                    its = 0
                    t2 = time.perf_counter()
                    for j in range(k):
                        m = torch.zeros_like(xt)
                        bj = B[:, j].contiguous()
                        info = api.lcg_solver("lcg_hip_dense_ata_ax", None, m, bj, N, para, D, api.LCG_CG)
                        its += info.iterations
                    torch.cuda.synchronize()
                    t3 = time.perf_counter()
                    ls = launches()
                    if r:
                        rb.append(sum(i.iterations for i in infos) / (t1 - t0)); rs.append(its / (t3 - t2))
                mb, ms = statistics.median(rb), statistics.median(rs)
                ratio = mb / ms
                mark = "" if ratio >= 1.0 else "  ** LOSS **"
                say(f"  CG k={k}: batched {mb:9.0f} column-iterations/s (spread {(max(rb) - min(rb)) / mb:5.1%}; per iteration "
                    f"{lb[2] / 200:.1f} operator kernels + {lb[0] / 200:.1f} passes)  {k} single solves {ms:9.0f} (per iteration "
                    f"{ls[2] / 200:.1f} products + {(ls[0] + ls[1]) / 200:.1f} passes and steps)  ratio {ratio:5.2f}{mark}  [{D.multi_last_kernel} | {D.last_kernel}]")
        say()
        D.destroy()
        del D
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
