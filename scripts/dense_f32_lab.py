"""Real dense operators stored in fp32 (lcg_hip_dense_create_f32) against the fp64 handle of the SAME widened matrix, in one process
(DESIGN 27).  The two handles give the same bits by contract (tests/test_gpu_dense_f32_product.py), so the one thing to measure is time:

  * products  K.x, K^T.x, K^T.K.x and their k = 2, 4, 8 forms (lcg_hip_dense_matvec / _ata / _matmat / _ata_multi);
  * solvers   LCG_CG through lcg_hip_dense_ata_ax, lcg_hip_dense_lcg_multi and SPG through lcg_hip_dense_solver_constrained_multi,
              `--its` iterations each, on K^T.K.

By construction the ceiling is 2 x where K's bytes dominate and 1 x where launches do.  Shapes: DESIGN 19's -- 1000 x 800, 2048^2,
8192^2, 20000 x 16000 -- uniform(-1, 1) made on the device as float32 and widened for the fp64 side.

Method (scripts/dense_lab.py's): per leg the mean device time of `reps` back-to-back calls between two events on the library's stream
after a warm-up; `--rounds` rounds, each round every leg of a shape in turn with the two sides alternating; medians, and the spread
(max - min) / median of the fp32 side.  Fraction of the read rate: the bytes of K a call streams (4 M N per pass over the fp32 matrix,
8 M N over the fp64 one) over the median, against the box's own read rate taken in the same run (the sum of 4 GiB, scripts/read_probe.py's
first line).  ratio = fp64 time / fp32 time; a ratio below 1 is a LOSS and is marked, not tuned away.

    python scripts/dense_f32_lab.py [--out profiles/dense_f32_lab.txt] [--rounds 3] [--its 30] [--only SUBSTRING] [--no-solvers]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1000, 800), (2048, 2048), (8192, 8192), (20000, 16000)]
KS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--its", type=int, default=30)
    ap.add_argument("--only", default=None, help="a substring of 'MxN' to run")
    ap.add_argument("--no-solvers", action="store_true")
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

    def mark(ratio):
        return "  ** LOSS **" if ratio < 1.0 else ""

    say(f"dense_f32_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    rate = read_rate()
    say(f"this box's read rate in this run (sum of 4 GiB, scripts/read_probe.py): {rate:.0f} GB/s")
    say(f"medians of {args.rounds} rounds; spread = (max - min) / median of the fp32 side; ratio = fp64 handle / fp32 handle (> 1: the fp32 handle is faster; "
        "the bytes say <= 2)")
    say()
    for (M, N) in SHAPES:
        tag = f"{M}x{N}"
        if args.only and args.only not in tag:
            continue
        g = torch.Generator(device="cuda"); g.manual_seed(7000 + N)
        K32 = (torch.rand((M, N), dtype=torch.float32, device="cuda", generator=g) * 2 - 1).contiguous()
        F = api.DenseMatrix.from_array_f32(K32)
        K64 = K32.double()
        D = api.DenseMatrix.from_array(K64)
        del K32, K64
        torch.cuda.empty_cache()
        assert (F.value_bytes, D.value_bytes) == (4, 8)
        mat = 4 * M * N
        reps = int(min(200, max(10, 2e9 / mat)))
        hf, hd = F.h, D.h
        say(f"{tag}: fp32 K = {mat / 2**20:.1f} MiB (fp64: {2 * mat / 2**20:.1f} MiB), {reps} calls per timing")

        def leg(label, new, old, passes, names):
            tn, to = [], []
            for _ in range(args.rounds):
                assert new() == 0 and old() == 0
                tn.append(timed(new, reps)); to.append(timed(old, reps))
            mn, mo = statistics.median(tn), statistics.median(to)
            say(f"  {label:16s} fp32 {mn:10.1f} us (spread {(max(tn) - min(tn)) / mn:5.1%}, K = {passes * mat / mn / 1e3:6.0f} GB/s = "
                f"{passes * mat / mn / 1e3 / rate:5.1%} of the read rate)  fp64 {mo:10.1f} us (K = {2 * passes * mat / mo / 1e3:6.0f} GB/s = "
                f"{2 * passes * mat / mo / 1e3 / rate:5.1%})  ratio {mo / mn:5.2f}{mark(mo / mn)}  [{names()}]")

        # ---- single-vector products
        x = torch.ones(N, dtype=torch.float64, device="cuda"); xt = torch.ones(M, dtype=torch.float64, device="cuda")
        y = torch.empty(M, dtype=torch.float64, device="cuda"); yt = torch.empty(N, dtype=torch.float64, device="cuda")
        leg("K.x", lambda: lib.lcg_hip_dense_matvec(hf, x.data_ptr(), y.data_ptr(), 0), lambda: lib.lcg_hip_dense_matvec(hd, x.data_ptr(), y.data_ptr(), 0),
            1, lambda: f"{F.last_kernel} | {D.last_kernel}")
        leg("K^T.x", lambda: lib.lcg_hip_dense_matvec(hf, xt.data_ptr(), yt.data_ptr(), 1), lambda: lib.lcg_hip_dense_matvec(hd, xt.data_ptr(), yt.data_ptr(), 1),
            1, lambda: f"{F.last_kernel} | {D.last_kernel}")
        one_pass = N <= 2048
        leg("K^T.K.x", lambda: lib.lcg_hip_dense_ata(hf, x.data_ptr(), yt.data_ptr()), lambda: lib.lcg_hip_dense_ata(hd, x.data_ptr(), yt.data_ptr()),
            1 if one_pass else 2, lambda: f"{F.last_kernel} | {D.last_kernel}")
        # ---- k-wide products
        for k in KS:
            Xb = torch.ones((N, k), dtype=torch.float64, device="cuda"); Xt = torch.ones((M, k), dtype=torch.float64, device="cuda")
            Yb = torch.empty((M, k), dtype=torch.float64, device="cuda"); Yt = torch.empty((N, k), dtype=torch.float64, device="cuda")
            px, pxt, py, pyt = Xb.data_ptr(), Xt.data_ptr(), Yb.data_ptr(), Yt.data_ptr()
            leg(f"k={k} K.X", lambda: lib.lcg_hip_dense_matmat(hf, k, px, py, 0), lambda: lib.lcg_hip_dense_matmat(hd, k, px, py, 0),
                1, lambda: f"{F.multi_last_kernel} | {D.multi_last_kernel}")
            leg(f"k={k} K^T.X", lambda: lib.lcg_hip_dense_matmat(hf, k, pxt, pyt, 1), lambda: lib.lcg_hip_dense_matmat(hd, k, pxt, pyt, 1),
                1, lambda: f"{F.multi_last_kernel} | {D.multi_last_kernel}")
            leg(f"k={k} K^T.K.X", lambda: lib.lcg_hip_dense_ata_multi(hf, k, px, pyt), lambda: lib.lcg_hip_dense_ata_multi(hd, k, px, pyt),
                2, lambda: f"{F.multi_last_kernel} | {D.multi_last_kernel}")
            del Xb, Xt, Yb, Yt
        # ---- solvers on K^T.K, capped at --its iterations
        if not args.no_solvers:
            sol = torch.rand(N, dtype=torch.float64, device="cuda", generator=g) + 1
            b = torch.empty_like(sol)
            D.ata(sol, b)
            para = api.lcg_default_parameters(epsilon=1e-300, abs_diff=0, max_iterations=args.its)
            low, hig = torch.full((N,), 1.0, dtype=torch.float64, device="cuda"), torch.full((N,), 2.0, dtype=torch.float64, device="cuda")

            def solve_leg(label, run):
                """run(H) -> column-iterations done; both sides per round, the first round dropped."""
                rn, ro, same = [], [], True
                for r in range(args.rounds + 1):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    cn, xn = run(F)
                    torch.cuda.synchronize(); t1 = time.perf_counter()
                    co, xo = run(D)
                    torch.cuda.synchronize(); t2 = time.perf_counter()
                    same = same and cn == co and torch.equal(xn, xo)
                    if r:
                        rn.append((t1 - t0) * 1e3); ro.append((t2 - t1) * 1e3)
                mn, mo = statistics.median(rn), statistics.median(ro)
                say(f"  {label:16s} fp32 {mn:10.2f} ms (spread {(max(rn) - min(rn)) / mn:5.1%})  fp64 {mo:10.2f} ms  ratio {mo / mn:5.2f}{mark(mo / mn)}"
                    f"  [{cn} column-iterations; iterates {'identical' if same else 'DIFFER'}]")

            def cg(H):
                m = torch.zeros(N, dtype=torch.float64, device="cuda")
                info = api.lcg_solver("lcg_hip_dense_ata_ax", None, m, b, N, para, H, api.LCG_CG)
                return info.iterations, m
            solve_leg("CG (ata_ax)", cg)
            for k in KS:
                B = (b[:, None] * torch.arange(1, k + 1, dtype=torch.float64, device="cuda")[None, :]).contiguous()

                def cgm(H):
                    Mb = torch.zeros_like(B)
                    return sum(i.iterations for i in api.dense_lcg_multi(H, Mb, B, para, normal=True)), Mb

                def spg(H):
                    Mb = torch.zeros_like(B)
                    return sum(i.iterations for i in api.dense_solver_constrained_multi(H, Mb, B, low, hig, para, api.LCG_SPG, normal=True)), Mb
                solve_leg(f"CG multi k={k}", cgm)
                solve_leg(f"SPG multi k={k}", spg)
        say()
        F.destroy(); D.destroy()
        del F, D
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
