"""Complex64 dense operators against the complex128 dense handle of the SAME matrix and against their own single-vector form, in one
process.  Never the code under test against itself:

  * single   clcg_hip_dense_matvec_c64 (K.x, K^T.x) against clcg_hip_dense_matvec on the complex128 handle: the byte count says <= 2 x;
  * k-wide   clcg_hip_dense_matmat_c64 (k_cdnm_mfma) against k calls of clcg_hip_dense_matvec_c64 (<= k x) and against
             clcg_hip_dense_matmat on the complex128 handle at the same k (<= 2 x);
  * loops    clcg_hip_dense_lbicg_sym_multi_c64 / clcg_hip_dense_lpcg_multi_c64 against clcg_hip_dense_lbicg_sym_multi /
             clcg_hip_dense_lpcg_multi on the complex128 handle (<= 2 x), in column-iterations per second over `--its` iterations.

Matrices: 1000^2, 8192^2, 16384^2 and 20000 x 16000 (products only), scripts/dense_multi_cplx_lab.py's family made on the device and
cast to complex64 for the new handle.

Method (scripts/dense_lab.py's): per leg the mean device time of `reps` back-to-back calls between two events on the library's stream
after a warm-up; three rounds, each round every leg of a shape in turn, so the two sides of a comparison alternate; medians, and the
spread (max - min) / median.  Fraction of the read rate: the complex64 matrix's 8 M N bytes over the median, against the box's own
read rate taken in the same run (the sum of 4 GiB).  A ratio below 1 is a LOSS; one well short of its byte count is marked SHORT.

    python scripts/dense_c64_lab.py [--out profiles/dense_c64_lab.txt] [--rounds 3] [--only SUBSTRING] [--no-loops]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1000, 1000), (8192, 8192), (16384, 16384), (20000, 16000)]
KS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--its", type=int, default=30)
    ap.add_argument("--only", default=None, help="a substring of 'MxN' to run")
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

    def mark(ratio, says):
        if ratio < 1.0:
            return "  ** LOSS **"
        return "  ** SHORT of its byte count **" if ratio < 0.6 * says else ""

    say(f"dense_c64_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    rate = read_rate()
    say(f"this box's read rate in this run (sum of 4 GiB, as bench.py --full): {rate:.0f} GB/s")
    say(f"medians of {args.rounds} rounds; spread = (max - min) / median of the complex64 side; ratio = other side / complex64 side (> 1: the new code is faster)")
    say()
    for (M, N) in SHAPES:
        tag = f"{M}x{N}"
        if args.only and args.only not in tag:
            continue
        g = torch.Generator(device="cuda"); g.manual_seed(5000 + N)
        if M == N:
            eye = torch.eye(N, dtype=torch.float64, device="cuda")
            G = torch.rand((N, N), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
            Kr = G.T @ G / N + 0.02 * eye
            G = torch.rand((N, N), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
            Ki = 0.1 * (G.T @ G / N + 0.2 * eye)
            del G, eye
            K = torch.complex((Kr + Kr.T) / 2, (Ki + Ki.T) / 2).contiguous()
            del Kr, Ki
        else:
            K = torch.complex(torch.rand((M, N), dtype=torch.float64, device="cuda", generator=g) * 2 - 1,
                              torch.rand((M, N), dtype=torch.float64, device="cuda", generator=g) * 2 - 1).contiguous()
        Dz = api.DenseMatrix.from_array(K)
        K32 = K.to(torch.complex64).contiguous()
        del K
        Dc = api.DenseMatrix.from_array_c64(K32)
        del K32
        torch.cuda.empty_cache()
        mat = 8 * M * N
        reps = int(min(200, max(10, 2e9 / mat)))
        hz, hc = Dz.h, Dc.h
        say(f"{tag}: complex64 K = {mat / 2**20:.1f} MiB (complex128: {2 * mat / 2**20:.1f} MiB), {reps} calls per timing")
        # ---- single-vector products
        for layout, label in ((0, "K.x"), (1, "K^T.x")):
            nin, nout = (M, N) if layout else (N, M)
            xc = torch.ones(nin, dtype=torch.complex64, device="cuda"); yc = torch.empty(nout, dtype=torch.complex64, device="cuda")
            xz = torch.ones(nin, dtype=torch.complex128, device="cuda"); yz = torch.empty(nout, dtype=torch.complex128, device="cuda")
            new = lambda: lib.clcg_hip_dense_matvec_c64(hc, xc.data_ptr(), yc.data_ptr(), layout, 0)       # noqa: E731
            old = lambda: lib.clcg_hip_dense_matvec(hz, xz.data_ptr(), yz.data_ptr(), layout, 0)          # noqa: E731
            tn, to = [], []
            for _ in range(args.rounds):
                assert new() == 0 and old() == 0
                tn.append(timed(new, reps)); to.append(timed(old, reps))
            mn, mo = statistics.median(tn), statistics.median(to)
            say(f"  single {label:6s} complex64 {mn:10.1f} us (spread {(max(tn) - min(tn)) / mn:5.1%}, K = {mat / mn / 1e3:6.0f} GB/s = "
                f"{mat / mn / 1e3 / rate:5.1%} of the read rate)  complex128 {mo:10.1f} us  ratio {mo / mn:5.2f} (bytes say <= 2)"
                f"{mark(mo / mn, 2)}  [{Dc.last_kernel} | {Dz.last_kernel}]")
        # ---- k-wide products
        xc = torch.ones(N, dtype=torch.complex64, device="cuda"); yc = torch.empty(M, dtype=torch.complex64, device="cuda")
        for k in KS:
            Xc = torch.ones((N, k), dtype=torch.complex64, device="cuda"); Yc = torch.empty((M, k), dtype=torch.complex64, device="cuda")
            Xz = torch.ones((N, k), dtype=torch.complex128, device="cuda"); Yz = torch.empty((M, k), dtype=torch.complex128, device="cuda")
            wide = lambda: lib.clcg_hip_dense_matmat_c64(hc, k, Xc.data_ptr(), Yc.data_ptr(), 0)          # noqa: E731
            wide_z = lambda: lib.clcg_hip_dense_matmat(hz, k, Xz.data_ptr(), Yz.data_ptr(), 0, 0)        # noqa: E731

            def singles():
                rc = 0
                for _ in range(k):
                    rc |= lib.clcg_hip_dense_matvec_c64(hc, xc.data_ptr(), yc.data_ptr(), 0, 0)
                return rc
            tw, ts, tz = [], [], []
            for _ in range(args.rounds):
                assert wide() == 0 and singles() == 0 and wide_z() == 0
                tw.append(timed(wide, reps)); ts.append(timed(singles, max(2, reps // k))); tz.append(timed(wide_z, reps))
            mw, ms, mz = statistics.median(tw), statistics.median(ts), statistics.median(tz)
            say(f"  k={k} K.X complex64 {mw:10.1f} us (spread {(max(tw) - min(tw)) / mw:5.1%}, K = {mat / mw / 1e3:6.0f} GB/s = "
                f"{mat / mw / 1e3 / rate:5.1%} of the read rate, {8 * M * N * k / mw / 1e6:5.1f} TFLOP/s)  {k} single complex64 {ms:10.1f} us  "
                f"ratio {ms / mw:5.2f} (<= {k}){mark(ms / mw, k)}  complex128 k-wide {mz:10.1f} us  ratio {mz / mw:5.2f} (<= 2){mark(mz / mw, 2)}"
                f"  [{Dc.multi_last_kernel} | {Dc.last_kernel} | {Dz.multi_last_kernel}]")
            del Xc, Yc, Xz, Yz
        # ---- batched loops
        if M == N and not args.no_loops:
            Dz.build_jacobi(False); Dc.build_jacobi_c64()
            xt = torch.complex(torch.rand(N, dtype=torch.float64, device="cuda", generator=g) + 1,
                               torch.rand(N, dtype=torch.float64, device="cuda", generator=g) + 1)
            bz = torch.empty_like(xt)
            Dz.matvec(xt, bz)
            para = api.clcg_default_parameters(epsilon=1e-300, abs_diff=0, max_iterations=args.its)
            for name, new_loop, old_loop in (("BiCG-sym", api.dense_clbicg_sym_multi_c64, api.dense_clbicg_sym_multi),
                                             ("PCG", api.dense_clpcg_multi_c64, api.dense_clpcg_multi)):
                for k in KS:
                    Bz = (bz[:, None] * torch.arange(1, k + 1, dtype=torch.float64, device="cuda")[None, :]).contiguous()
                    Bc = Bz.to(torch.complex64).contiguous()
                    rn, ro = [], []
                    for r in range(args.rounds + 1):
                        Mc, Mz = torch.zeros_like(Bc), torch.zeros_like(Bz)
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        i_new = new_loop(Dc, Mc, Bc, para)
                        torch.cuda.synchronize(); t1 = time.perf_counter()
                        i_old = old_loop(Dz, Mz, Bz, para)
                        torch.cuda.synchronize(); t2 = time.perf_counter()
                        if r:
                            rn.append(sum(i.iterations for i in i_new) / (t1 - t0)); ro.append(sum(i.iterations for i in i_old) / (t2 - t1))
                    mn, mo = statistics.median(rn), statistics.median(ro)
                    say(f"  {name} k={k}: complex64 {mn:9.0f} column-iterations/s (spread {(max(rn) - min(rn)) / mn:5.1%}; K = "
                        f"{mn / k * mat / 1e9:5.0f} GB/s = {mn / k * mat / 1e9 / rate:5.1%} of the read rate)  complex128 {mo:9.0f}  "
                        f"ratio {mn / mo:5.2f} (<= 2){mark(mn / mo, 2)}")
        say()
        Dz.destroy(); Dc.destroy()
        del Dz, Dc
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
