"""The batched complex64 IC(0) against what the library had before it, on one MI355X in one process (README):

  (a) one k-wide apply (clcg_hip_ic0_solve_multi_c64) against k single applies (lcg_hip_ic0_solve_c64);
  (b) batched PCG + IC(0) (clcg_hip_lpcg_multi_m_c64) in column-iterations per second against k single solves
      (clcg_hip_solver_preconditioned_c64 with clcg_hip_ic0_mx_c64) at the same sweeps setting;
  (c) the time of a batch to sample14's stop rule (epsilon 1e-6 on |r|^2 / max(|m|, 1)^2) with IC(0) against the same batch with the
      Jacobi diagonal (clcg_hip_lpcg_multi_c64)

at k = 2, 4, 8, exact applies and 2 / 4 sweeps, on case_10K_cA cast to complex64 and on the complex-shifted 1000^2 Laplacian of
profiles/multi_c64_lab.txt.  The contenders alternate over the rounds and the medians are reported (scripts/c64_lab.py's way); every
ratio is the new entry against the older ones, and a ratio below one is a loss, printed in bold.

    python scripts/multi_c64_ic0_lab.py [--rounds 3] [--steps 20] [--out profiles/multi_c64_ic0_lab.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from liblcg_amd import _lib, api  # noqa: E402
from multi_c64_lab import complex_shifted, mark  # noqa: E402

KS = (2, 4, 8)
SWEEPS = (0, 2, 4)
SAMPLE14 = dict(epsilon=1e-6, abs_diff=0, max_iterations=5000)


def sweep_bytes(k, t):
    """One sweep over one triangle of t entries per row, per row and column, by construction (csr_tri.hip, csr_tri_multi.hip): col / val
    12 B per entry and the row pointer's 4 B, shared by the k columns of a batch; x read and y written, 8 B each; gathers not counted."""
    return (12.0 * t + 4.0) / max(k, 1) + 16.0


def pcg_bytes(k, p, t, s):
    """One PCG + IC(0) iteration with s >= 1 sweeps per triangle, per row and column, by construction (solvers_multi_c64.hip,
    solvers_c64.hip): the product's 12 B per entry (shared by k) and A.d written (8); d.Ad -- a batch's finishing lanes re-read d (8),
    the single loop runs a pass (16); the update reads d, m, Ad, r and writes m, r (48); 2 s sweeps; the sums read m, r, s (24); the
    direction reads d, s and writes d (24)."""
    if k == 0:
        return 8.0 + 12.0 * p + 16.0 + 48.0 + 2 * s * sweep_bytes(1, t) + 24.0 + 24.0
    return 8.0 + 12.0 * p / k + 8.0 + 48.0 + 2 * s * sweep_bytes(k, t) + 24.0 + 24.0


def case10k():
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    n, row, col, val, b = read_coo_system(os.path.join(ROOT, "tests", "golden", "case_10K_cA"), True)
    return coo_to_csr_host(n, row, col, val)


def laplace():
    Ar = api.CsrMatrix.laplace2d(1000, 1000)
    out = complex_shifted(Ar, 7)
    Ar.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "multi_c64_ic0_lab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multi_c64_ic0_lab.py measures on the GPU: there is no other way to get these numbers"
    lib = _lib.load()
    assert lib.lcg_hip_init(0) == 0
    api.use_torch_stream()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    say(f"multi_c64_ic0_lab: {torch.cuda.get_device_name(0)}; {args.rounds} rounds alternating the contenders, medians; {args.inner} applies "
        f"per timing, {args.steps} iterations per capped solve; losses in bold")
    for name, make in (("case_10K_cA", case10k), ("complex-shifted laplace 1000^2", laplace)):
        rp, ci, v = make()
        A = api.CsrMatrix.from_csr_c64(rp, ci, v.astype(np.complex64))
        A.build_jacobi(); A.build_ic0()
        n, nnz = A.n, len(ci)
        p, t = nnz / n, (nnz / n + 1) / 2
        del rp, ci, v
        inf = A.ic0_info()
        say()
        say(f"== {name}, complex64: {n} rows, {nnz} entries ({p:.1f} per row; {t:.1f} per row of a triangle); levels {inf['levels_lower']} / "
            f"{inf['levels_upper']}, factor built in {inf['build_ms']:.1f} ms")
        say("   caps by construction (single / batched bytes per row and column), one sweep: "
            + ", ".join(f"k = {k}: {sweep_bytes(0, t) / sweep_bytes(k, t):.2f}x" for k in KS)
            + "; one PCG iteration at 2 / 4 sweeps: "
            + ", ".join(f"k = {k}: {pcg_bytes(0, p, t, 2) / pcg_bytes(k, p, t, 2):.2f}x / {pcg_bytes(0, p, t, 4) / pcg_bytes(k, p, t, 4):.2f}x" for k in KS))
        g = torch.Generator(device="cuda"); g.manual_seed(1)

        def crand(*shape):
            return torch.complex(torch.rand(shape, dtype=torch.float32, device="cuda", generator=g) - 0.5,
                                 torch.rand(shape, dtype=torch.float32, device="cuda", generator=g) - 0.5)

        for k in KS:
            Xt = crand(n, k)
            B = torch.empty_like(Xt)
            A.cspmm_c64(Xt, B); api.synchronize()
            B[:, 1] *= 0.5
            cols = [B[:, j].contiguous() for j in range(k)]
            for s in SWEEPS:
                A.ic0_set_sweeps(s)
                L = A.ic0_info()["launches_per_apply"]
                Y = torch.empty_like(B)
                ys = [torch.empty_like(c) for c in cols]

                def apply_batch():
                    A.ic0_solve_multi_c64(B, Y)

                def apply_singles():
                    for c, y in zip(cols, ys):
                        A.ic0_solve(c, y)

                def timed(f):
                    f(); api.synchronize()
                    e0, e1 = ev(), ev()
                    e0.record()
                    for _ in range(args.inner):
                        f()
                    e1.record(); torch.cuda.synchronize()
                    return e0.elapsed_time(e1) * 1e3 / args.inner

                cap_para = api.clcg_default_parameters(epsilon=1e-30, max_iterations=args.steps)
                s14 = api.clcg_default_parameters(**SAMPLE14)

                def pcg_batch(precond, para):
                    M = torch.zeros_like(B)
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    infos = api.clpcg_multi_c64(A, M, B, para, precond=precond)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0, infos

                def pcg_singles(para):
                    its = 0
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    for c in cols:
                        m = torch.zeros_like(c)
                        its += api.clcg_solver_preconditioned_c64("clcg_hip_csr_ax_c64", "clcg_hip_ic0_mx_c64", None, m, c, n, para, A).iterations
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0, its

                r = {q: [] for q in ("ab", "as", "pb", "ps", "ci", "cj")}
                its_i = its_j = None
                for rnd in range(args.rounds):
                    order = ("b", "s", "s", "b") if rnd % 2 == 0 else ("s", "b", "b", "s")
                    for who in order:
                        if who == "b":
                            r["ab"].append(timed(apply_batch))
                            el, infos = pcg_batch("ic0", cap_para)
                            r["pb"].append(sum(i.iterations for i in infos) / el)
                            el, its_i = pcg_batch("ic0", s14)
                            r["ci"].append(el)
                        else:
                            r["as"].append(timed(apply_singles))
                            el, its = pcg_singles(cap_para)
                            r["ps"].append(its / el)
                            el, its_j = pcg_batch("jacobi", s14)
                            r["cj"].append(el)
                m = {q: float(np.median(x)) for q, x in r.items()}
                what = "exact" if s == 0 else f"{s} sweeps"
                say(f"   k = {k}, {what:>8} ({L:>4} launches per apply):")
                say(f"      (a) apply: batched {m['ab']:9.1f} us   {k} x single {m['as']:9.1f} us   {k} x single / batched = {mark(m['as'] / m['ab'])}"
                    + (f" (cap {sweep_bytes(0, t) / sweep_bytes(k, t):.2f}x)" if s else ""))
                say(f"      (b) PCG + IC(0): batched {m['pb']:9.0f} column-iterations/s   {k} x single {m['ps']:9.0f}   ratio {mark(m['pb'] / m['ps'])}"
                    + (f" (cap {pcg_bytes(0, p, t, s) / pcg_bytes(k, p, t, s):.2f}x)" if s else ""))
                say(f"      (c) to sample14's stop rule: IC(0) batch {m['ci'] * 1e3:9.2f} ms (counts {[i.iterations for i in its_i]}, codes {[i.ret for i in its_i]})   "
                    f"Jacobi batch {m['cj'] * 1e3:9.2f} ms (counts {[i.iterations for i in its_j]})   Jacobi / IC(0) = {mark(m['cj'] / m['ci'])}")
        A.destroy()
        lib.lcg_hip_trim()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
