"""Dense operators against what a user could do before them, in one process: K.x, K^T.x and K^T.K.x of a
lcg_hip_dense_t with every forced path, beside the same K stored as a CSR matrix with every entry present and multiplied by
lcg_hip_spmv / lcg_hip_spmv_op(layout = 1) -- the emulation on the parent commit's means.

Shapes: 100 x 80 and 1000 x 800 (sample1 / sample2), 4096^2 (128 MiB: inside the Infinity Cache), 8192^2 (512 MiB: beyond it),
200 x 200000 and 200000 x 200 (the skewed shapes of an inversion), 2048^2 complex128.

Per leg: the mean device time of `reps` back-to-back calls between two events after a warm-up; three rounds, each round every
leg of a shape in turn (dense and CSR alternate); medians, and the spread (max - min) / median of the rounds.  Both sides are
called through the C ABI with raw pointers, one ctypes call per launch sequence; a forced path is set before the timing.  Where a
product is a few microseconds the interval between the events is the host's enqueue rate, not kernel time: for those shapes
profiles/dense_small_trace.txt has the kernels' own durations (rocprofv3 --kernel-trace --stats over `--trace --only ...`).  GB/s counts
8 M N (16 M N complex) + the vectors once, over the median; it is printed beside the box's own read rate taken in the same run
(the sum of 4 GiB, as bench.py --full takes it).  K^T.K.x counts K ONCE: what the one-pass form has to move.

CG: iterations per second of lcg_hip_lcg-style CG (LCG_CG) on lcg_hip_dense_ata_ax, 200 iterations from m = 0, wall clock
around the solve, for sample_dense's 1000 x 800 system and a 20000 x 16000 one (2.56 GB).

    python scripts/dense_lab.py [--out profiles/dense_lab.txt] [--rounds 3] [--only SUBSTRING] [--no-cg]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(100, 80, False), (1000, 800, False), (4096, 4096, False), (8192, 8192, False), (200, 200000, False), (200000, 200, False),
          (2048, 2048, True), (16384, 2048, False)]       # the last one: the widest rows the one-pass K^T.K.x takes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="a substring of 'MxN' to run")
    ap.add_argument("--no-cg", action="store_true")
    ap.add_argument("--trace", action="store_true", help="a short run for rocprofv3 --kernel-trace --stats: 20 calls per timing, one round")
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

    say(f"dense_lab: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')}")
    rate = read_rate()
    say(f"this box's read rate in this run (sum of 4 GiB, as bench.py --full): {rate:.0f} GB/s")
    say(f"medians of {args.rounds} rounds; spread = (max - min) / median; ratio = CSR emulation / dense automatic path (> 1: dense is faster)")
    say()
    names = api.DenseMatrix.kernel_names()
    for (M, N, cplx) in SHAPES:
        tag = f"{M}x{N}" + (" c128" if cplx else "")
        if args.only and args.only not in tag:
            continue
        dt = torch.complex128 if cplx else torch.float64
        es = 16 if cplx else 8
        g = torch.Generator(device="cuda"); g.manual_seed(M * 31 + N)
        K = torch.rand((M, N), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
        if cplx:
            K = torch.complex(K, torch.rand((M, N), dtype=torch.float64, device="cuda", generator=g) * 2 - 1)
        xN = torch.ones(N, dtype=dt, device="cuda"); xM = torch.ones(M, dtype=dt, device="cuda")
        yN = torch.empty(N, dtype=dt, device="cuda"); yM = torch.empty(M, dtype=dt, device="cuda"); tM = torch.empty(M, dtype=dt, device="cuda")
        D = api.DenseMatrix.from_array(K)
        rp = (torch.arange(M + 1, dtype=torch.int64, device="cuda") * N).to(torch.int32)
        ci = torch.arange(N, dtype=torch.int32, device="cuda").repeat(M)
        A = api.CsrMatrix.from_csr(rp, ci, K.reshape(-1), n_cols=N)
        del rp, ci
        # K^T.x of the emulation: lcg_hip_spmv_op(layout = 1) where the library offers it for this handle, otherwise the second
        # materialised copy a user has to keep (K^T as a CSR handle of its own)
        AT = None
        if lib.lcg_hip_spmv_op(A.h, xM.data_ptr(), yN.data_ptr(), 1, 0) != 0:
            rpt = (torch.arange(N + 1, dtype=torch.int64, device="cuda") * M).to(torch.int32)
            cit = torch.arange(M, dtype=torch.int32, device="cuda").repeat(N)
            AT = api.CsrMatrix.from_csr(rpt, cit, K.t().contiguous().reshape(-1), n_cols=M)
            del rpt, cit
        api.synchronize()
        mat = es * M * N
        reps = int(min(200, max(10, 2e9 / mat)))
        if args.trace:
            reps = 20
        legs = []       # (label, product, call, bytes)

        # both sides are timed through the C ABI with raw pointers: one ctypes call per launch sequence, nothing else in the loop
        # (the path is forced before the timing, not inside it)
        def dense_leg(variant, product):
            f, fc = (lib.clcg_hip_dense_matvec, True) if cplx else (lib.lcg_hip_dense_matvec, False)
            h, pxN, pxM, pyN, pyM = D.h, xN.data_ptr(), xM.data_ptr(), yN.data_ptr(), yM.data_ptr()
            if product == "Kx":
                call = (lambda: f(h, pxN, pyM, 0, 0)) if fc else (lambda: f(h, pxN, pyM, 0))
            elif product == "KTx":
                call = (lambda: f(h, pxM, pyN, 1, 0)) if fc else (lambda: f(h, pxM, pyN, 1))
            else:
                call = lambda: lib.lcg_hip_dense_ata(h, pxN, pyN)
            return (variant, call)

        def csr_leg(product):
            hA, pxN, pxM, pyN, pyM, ptM = A.h, xN.data_ptr(), xM.data_ptr(), yN.data_ptr(), yM.data_ptr(), tM.data_ptr()
            if AT is None:
                kt = lambda x: lib.lcg_hip_spmv_op(hA, x, pyN, 1, 0)
            else:
                hT = AT.h
                kt = lambda x: lib.lcg_hip_spmv(hT, x, pyN)
            if product == "Kx":
                return (None, lambda: lib.lcg_hip_spmv(hA, pxN, pyM))
            if product == "KTx":
                return (None, lambda: kt(pxM))
            return (None, lambda: lib.lcg_hip_spmv(hA, pxN, ptM) or kt(ptM))      # K^T.(K.x): two products

        vec = es * (M + N)
        for product, variants in (("Kx", (0, 1, 2)), ("KTx", (0,)), ("KTKx", () if cplx else (0, 4, 5, 6))):
            for v in variants:
                if v in (5, 6) and N > 2048:
                    continue
                if v == 6 and mat > (64 << 20):
                    continue                     # one workgroup over a large matrix: nothing to learn, minutes to run
                if lib.lcg_hip_dense_set_kernel(D.h, v) != 0:
                    continue                     # refused for this shape (k_dn_row_split: nothing to split)
                legs.append((f"dense {'auto' if v == 0 else 'forced ' + names[v - 1]}", product, dense_leg(v, product), mat + vec))
            if variants:
                legs.append(("CSR emulation", product, csr_leg(product), None))
        res = {i: [] for i in range(len(legs))}
        kern = {}
        for _ in range(args.rounds):
            for i, (label, product, (variant, call), _) in enumerate(legs):
                if variant is not None:
                    assert lib.lcg_hip_dense_set_kernel(D.h, variant) == 0
                assert call() == 0
                res[i].append(timed(call, reps))
                kern[i] = D.last_kernel if label.startswith("dense") else \
                    ("spmv_op(layout = 1): " if AT is None else "a CSR copy of K^T: ") * (product != "Kx") + lib.lcg_hip_csr_last_kernel(A.h).decode()[:48]
        say(f"{tag}: K = {mat / 2**20:.1f} MiB, {reps} calls per timing")
        auto = {}
        for i, (label, product, _, byts) in enumerate(legs):
            med = statistics.median(res[i]); spread = (max(res[i]) - min(res[i])) / med
            if label == "dense auto":
                auto[product] = i
            line = f"  {product:5s} {label:34s} {med:10.1f} us  spread {spread:5.1%}"
            if byts:
                line += f"  {byts / med / 1e3:7.0f} GB/s = {byts / med / 1e3 / rate:5.1%} of the read rate"
            else:
                base = res[auto[product]]
                line += f"  ratio {med / statistics.median(base):5.2f}  (round by round: {', '.join(f'{c / d:.2f}' for c, d in zip(res[i], base))})"
            say(line + f"  [{kern[i]}]")
        say()
        D.destroy(); A.destroy()
        if AT is not None:
            AT.destroy()
        del K, D, A, AT
        torch.cuda.empty_cache()
    if not args.no_cg and not args.only:
        for (M, N) in ((1000, 800), (20000, 16000)):
            g = torch.Generator(device="cuda"); g.manual_seed(M + N)
            K = torch.rand((M, N), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
            D = api.DenseMatrix.from_array(K)
            del K
            xt = torch.rand(N, dtype=torch.float64, device="cuda", generator=g) + 1
            b = torch.empty_like(xt)
            D.ata(xt, b)
            para = api.lcg_default_parameters(epsilon=1e-300, abs_diff=0, max_iterations=200)
            rates = []
            for r in range(args.rounds + 1):
                m = torch.zeros_like(xt)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                info = api.lcg_solver("lcg_hip_dense_ata_ax", None, m, b, N, para, D, api.LCG_CG)
                torch.cuda.synchronize()
                if r:
                    rates.append(info.iterations / (time.perf_counter() - t0))
            med = statistics.median(rates)
            say(f"CG on lcg_hip_dense_ata_ax, {M}x{N} ({8 * M * N / 1e9:.2f} GB), {info.iterations} iterations: {med:.0f} iterations/s "
                f"(spread {(max(rates) - min(rates)) / med:.1%}; one K per iteration = {8 * M * N * med / 1e9:.0f} GB/s)  [{D.last_kernel}]")
            D.destroy()
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
