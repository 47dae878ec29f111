"""SHA-256 of everything IC(0) and ILU(0) compute on a fixed list of small systems, through the Python view of the C ABI only: run
on two builds of the library, the two outputs are identical line for line when the builds compute the same bits.

Systems: case_10K_A; case_1K_cA and case_10K_cA in complex128 and complex64; the 64 x 64 Laplacian; layered_nonsym real and
complex (9,150 rows, wide and narrow levels side by side, stored unsorted with split duplicates); window_edges (1,380 rows on
both sides of the sweep kernel's window); fuzz20k_nonsym; a 1-row matrix.  Per system and factor (ILU(0): fp64 / complex128;
IC(0): every type, on the lower triangle): the factor's arrays; the apply for which = 0, 1, 2 on a fixed right-hand side under
the default schedule and under max_merged = 0; the apply by k = 1, 2, 3 and k = levels sweeps; what _info returns (not the
build's milliseconds); ILU(0)'s right-preconditioned product.  Last, the texts of the refusals a caller can read.

    python scripts/factor_digest.py [--out FILE] [--lib path/to/liblcg_hip.so]
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype} {a.shape} ".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of liblcg_hip.so with the same C ABI")
    args = ap.parse_args()
    import torch
    from liblcg_amd import _lib
    if args.lib:
        _lib.SO_PATH = os.path.abspath(args.lib)
    from liblcg_amd import api
    from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system
    import ic0_checker as IC
    import ic0_sweeps_checker as S
    import ilu0_checker as K
    import ic0_c64_lab as C64
    lib = _lib.load()
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def systems():
        n, row, col, val, _ = read_coo_system(os.path.join(ROOT, "tests", "golden", "case_10K_A"))
        yield "case_10K_A", "f64", coo_to_csr_host(n, row, col, val)
        for tag in ("1K", "10K"):
            rp, ci, v, _ = C64.case(tag)
            yield f"case_{tag}_cA", "c128", (rp, ci, v)
            yield f"case_{tag}_cA", "c64", (rp, ci, v)
        yield "laplace2d 64x64", "f64", S.laplace2d(64)
        for cplx in (False, True):
            rp, ci, v = K.layered_nonsym(K.LAYERS_L, K.LAYERS_U, 41, cplx)
            yield "layered_nonsym", "c128" if cplx else "f64", IC.shuffle_split(rp, ci, v, 42)
        yield "window_edges", "f64", K.window_edges(5)
        yield "fuzz20k_nonsym", "f64", K.random_nonsym(20000, 902)
        yield "one row", "f64", (np.array([0, 1]), np.array([0]), np.array([4.0]))

    dt = {"f64": torch.float64, "c128": torch.complex128, "c64": torch.complex64}
    for name, kind, (rp, ci, v) in systems():
        if kind == "c64":
            A = api.CsrMatrix.from_csr_c64(rp, ci, np.asarray(v).astype(np.complex64))
        else:
            A = api.CsrMatrix.from_csr(rp, ci, np.asarray(v).astype(np.complex128 if kind == "c128" else np.float64))
        n = A.n
        rng = np.random.default_rng(7)
        xh = rng.uniform(-1, 1, n) + (1j * rng.uniform(-1, 1, n) if kind != "f64" else 0)
        x = torch.from_numpy(xh).to(dt[kind]).cuda()
        y = torch.empty_like(x)
        factors = [("IC(0)", lib.lcg_hip_csr_build_ic0_c64 if kind == "c64" else lib.lcg_hip_csr_build_ic0, A.ic0_info, A.ic0_set_sweeps,
                    A.ic0_solve, lib.lcg_hip_csr_ic0_schedule_for_test, lambda: [A.ic0_factor_to_host()], "levels_lower", "levels_upper")]
        if kind != "c64":
            factors.append(("ILU(0)", lib.lcg_hip_csr_build_ilu0, A.ilu0_info, A.ilu0_set_sweeps, A.ilu0_solve,
                            lib.lcg_hip_csr_ilu0_schedule_for_test, lambda: [A.ilu0_factor_to_host(0), A.ilu0_factor_to_host(1)],
                            "levels_L", "levels_U"))
        for fname, build, info, set_sweeps, solve, schedule, arrays, ll, lu in factors:
            tag = f"{name} ({kind}) {fname}"
            rc = build(A.h)
            if rc:
                say(f"{tag}: build returns {rc}: {lib.lcg_hip_last_error().decode()}")
                continue

            def applies(what):
                for which in (0, 1, 2):
                    y.zero_()
                    solve(x, y, which)
                    say(f"{tag} {what} which={which}: {sha(y.cpu().numpy())}")

            def report(what):
                i = info()
                say(f"{tag} info {what}: levels {i[ll]} / {i[lu]}, launches {i['launches_per_apply']}, zero_pivot {i['zero_pivot']}, "
                    f"bytes {i['bytes']}, sweeps {i['sweeps']}")

            for t, tri in enumerate(arrays()):
                say(f"{tag} factor arrays {t}: {sha(*tri)}")
            report("exact")
            applies("exact")
            assert schedule(A.h, 0) == 0
            report("max_merged=0")
            applies("max_merged=0")
            assert schedule(A.h, -1) == 0
            i0 = info()
            for k in (1, 2, 3, max(i0[ll], i0[lu])):
                set_sweeps(k)
                report(f"k={k}")
                applies(f"k={k}")
                if fname == "ILU(0)" and k == 2:
                    y.zero_()
                    (lib.clcg_hip_csr_ax_ilu0(A.h, x.data_ptr(), y.data_ptr(), n, 0, 0) if kind == "c128" else
                     lib.lcg_hip_csr_ax_ilu0(A.h, x.data_ptr(), y.data_ptr(), n))
                    say(f"{tag} k=2 A.(U^-1 L^-1 x): {sha(y.cpu().numpy())}")
            set_sweeps(0)
            if fname == "ILU(0)":
                y.zero_()
                (lib.clcg_hip_csr_ax_ilu0(A.h, x.data_ptr(), y.data_ptr(), n, 0, 0) if kind == "c128" else
                 lib.lcg_hip_csr_ax_ilu0(A.h, x.data_ptr(), y.data_ptr(), n))
                say(f"{tag} exact A.(U^-1 L^-1 x): {sha(y.cpu().numpy())}")
        A.destroy()

    # the refusals' texts: a handle without factors, then one with both
    err = lambda: lib.lcg_hip_last_error().decode()
    A = api.CsrMatrix.from_csr(*S.laplace2d(8))
    Ac = api.CsrMatrix.from_csr(np.array([0, 1, 2]), np.array([0, 1]), np.array([1 + 1j, 2.0]))
    A64 = api.CsrMatrix.from_csr_c64(np.array([0, 1, 2]), np.array([0, 1]), np.array([1 + 1j, 2.0]))
    x = torch.ones(64, dtype=torch.float64, device="cuda")
    y = torch.zeros(72, dtype=torch.float64, device="cuda")
    k = C.c_int()
    px, py = x.data_ptr(), y.data_ptr()

    def refusals(state):
        calls = [("ic0_set_sweeps(2)", lambda: lib.lcg_hip_csr_ic0_set_sweeps(A.h, 2)),
                 ("ic0_set_sweeps(-1)", lambda: lib.lcg_hip_csr_ic0_set_sweeps(A.h, -1)),
                 ("ic0_get_sweeps", lambda: lib.lcg_hip_csr_ic0_get_sweeps(A.h, C.byref(k))),
                 ("ic0_get_sweeps(NULL)", lambda: lib.lcg_hip_csr_ic0_get_sweeps(A.h, None)),
                 ("ic0_set_sweeps(no handle)", lambda: lib.lcg_hip_csr_ic0_set_sweeps(None, 2)),
                 ("ilu0_set_sweeps(2)", lambda: lib.lcg_hip_csr_ilu0_set_sweeps(A.h, 2)),
                 ("ilu0_set_sweeps(-1)", lambda: lib.lcg_hip_csr_ilu0_set_sweeps(A.h, -1)),
                 ("ilu0_get_sweeps", lambda: lib.lcg_hip_csr_ilu0_get_sweeps(A.h, C.byref(k))),
                 ("ilu0_get_sweeps(NULL)", lambda: lib.lcg_hip_csr_ilu0_get_sweeps(A.h, None)),
                 ("ilu0_get_sweeps(no handle)", lambda: lib.lcg_hip_csr_ilu0_get_sweeps(None, C.byref(k))),
                 ("ic0_solve which=2", lambda: lib.lcg_hip_ic0_solve(A.h, 2, px, py)),
                 ("ic0_solve which=3", lambda: lib.lcg_hip_ic0_solve(A.h, 3, px, py)),
                 ("ic0_solve overlap", lambda: lib.lcg_hip_ic0_solve(A.h, 2, py, py + 8)),
                 ("ic0_solve_c64 on f64", lambda: lib.lcg_hip_ic0_solve_c64(A.h, 2, px, py)),
                 ("ic0_solve on c64", lambda: lib.lcg_hip_ic0_solve(A64.h, 2, px, py)),
                 ("ic0_solve_c64 on c64", lambda: lib.lcg_hip_ic0_solve_c64(A64.h, 2, px, py)),
                 ("build_ic0 on c64", lambda: lib.lcg_hip_csr_build_ic0(A64.h)),
                 ("build_ic0_c64 on f64", lambda: lib.lcg_hip_csr_build_ic0_c64(A.h)),
                 ("build_ilu0 on c64", lambda: lib.lcg_hip_csr_build_ilu0(A64.h)),
                 ("ilu0_solve which=2", lambda: lib.lcg_hip_ilu0_solve(A.h, 2, px, py)),
                 ("ilu0_solve which=-1", lambda: lib.lcg_hip_ilu0_solve(A.h, -1, px, py)),
                 ("ilu0_solve overlap", lambda: lib.lcg_hip_ilu0_solve(A.h, 2, py, py + 8)),
                 ("ilu0_solve on c64", lambda: lib.lcg_hip_ilu0_solve(A64.h, 2, px, py)),
                 ("ic0_mx n_size", lambda: lib.lcg_hip_ic0_mx(A.h, px, py, 63)),
                 ("clcg_ic0_mx on real", lambda: lib.clcg_hip_ic0_mx(A.h, px, py, 64, 0, 0)),
                 ("clcg_ic0_mx conjugate", lambda: lib.clcg_hip_ic0_mx(Ac.h, px, py, 2, 0, 1)),
                 ("clcg_ic0_mx_c64 conjugate", lambda: lib.clcg_hip_ic0_mx_c64(A64.h, px, py, 2, 0, 1)),
                 ("ic0_mx on complex", lambda: lib.lcg_hip_ic0_mx(Ac.h, px, py, 2)),
                 ("ilu0_mx n_size", lambda: lib.lcg_hip_ilu0_mx(A.h, px, py, 63)),
                 ("clcg_ilu0_mx on real", lambda: lib.clcg_hip_ilu0_mx(A.h, px, py, 64, 0, 0)),
                 ("clcg_ilu0_mx layout", lambda: lib.clcg_hip_ilu0_mx(Ac.h, px, py, 2, 1, 0)),
                 ("ilu0_mx on complex", lambda: lib.lcg_hip_ilu0_mx(Ac.h, px, py, 2)),
                 ("ax_ilu0 n_size", lambda: lib.lcg_hip_csr_ax_ilu0(A.h, px, py, 63)),
                 ("clcg_ax_ilu0 conjugate", lambda: lib.clcg_hip_csr_ax_ilu0(Ac.h, px, py, 2, 0, 1)),
                 ("ic0_info", lambda: lib.lcg_hip_csr_ic0_info(A.h, None, None, None, None, None, None)),
                 ("ilu0_factor which=2", lambda: lib.lcg_hip_csr_ilu0_factor(A.h, 2, None, None, None)),
                 ("ic0_schedule_for_test(1025)", lambda: lib.lcg_hip_csr_ic0_schedule_for_test(A.h, 1025)),
                 ("ilu0_schedule_for_test(-2)", lambda: lib.lcg_hip_csr_ilu0_schedule_for_test(A.h, -2))]
        for what, call in calls:
            rc = call()
            say(f"refusal {state} {what}: {rc}: {err()}")

    refusals("no factor")
    for M in (A, Ac):
        M.build_ic0()
        M.build_ilu0()
    A64.build_ic0()
    refusals("factors built")
    # pivots: the smallest failing row, named in the text
    P = api.CsrMatrix.from_csr(np.array([0, 2, 4, 5]), np.array([0, 1, 0, 1, 2]), np.array([1.0, 2.0, 2.0, 4.0, 0.0]))
    for what, call in (("build_ic0", lambda: lib.lcg_hip_csr_build_ic0(P.h)), ("build_ilu0", lambda: lib.lcg_hip_csr_build_ilu0(P.h)),
                       ("ic0_solve", lambda: lib.lcg_hip_ic0_solve(P.h, 2, px, py)),
                       ("ilu0_set_sweeps", lambda: lib.lcg_hip_csr_ilu0_set_sweeps(P.h, 1))):
        rc = call()
        say(f"refusal bad pivot {what}: {rc}: {err()}; IC(0) zero_pivot {P.ic0_info()['zero_pivot']}")
    R = api.CsrMatrix.from_csr(np.array([0, 1, 2]), np.array([0, 2]), np.array([1.0, 2.0]), n_cols=3)
    say(f"refusal not square build_ic0: {lib.lcg_hip_csr_build_ic0(R.h)}: {err()}")
    say(f"refusal not square build_ilu0: {lib.lcg_hip_csr_build_ilu0(R.h)}: {err()}")
    for M in (A, Ac, A64, P, R):
        M.destroy()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
