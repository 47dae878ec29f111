"""SHA-256 of everything a caller can read from the batched solvers on a fixed list of small systems, through the Python view of
the C ABI only: run on two builds of the library, the two outputs are identical line for line when the builds compute the same bits
and enqueue the same launches.

Entries: lcg_hip_lcg_multi, lcg_hip_lpcg_multi, lcg_hip_lpcg_multi_m (Jacobi, IC(0), ILU(0)), lcg_hip_lbicgstab_multi (none, Jacobi,
IC(0), ILU(0)), clcg_hip_lbicg_sym_multi, clcg_hip_lpcg_multi, lcg_hip_dense_lcg_multi and lcg_hip_dense_lpcg_multi (normal = 1, 0).
Systems: the CLASS lists of tests/multi_cases.py, multi_bicg_cases.py and multi_cplx_cases.py with the k of their EDGE_CASES, the
shapes of tests/dense_multi_cases.py.  Per system and k: runs capped at 6 iterations under both stop rules in device memory and
under the relative rule in host memory; a converged run (cap 2000) and a run with max_iterations = 0 where the system has at most
CONVERGED_ROWS rows; for k >= 4 a batch of mixed verdicts (a column already optimised, a NaN column, running columns); IC(0) and
ILU(0) as M on the systems of at most FACTOR_ROWS rows.  Per run: the return code, one hash over the solution block, ret,
iterations and the bits of residual, and the four counts of lcg_hip_last_launches -- those where a column ran to the cap; a batch
that stops earlier leaves counts that depend on how far ahead of the device the host had enqueued (see solve()).  Last, the code and
text of every refusal of every entry, with nothing built, then Jacobi, then IC(0), then everything.

What is printed and written is ONE line per entry and system (per entry and state of the handles for the refusals): the SHA-256 of
the runs' lines.  --detail prints those lines too, to find what differs.

    python scripts/multi_digest.py [--out FILE] [--lib path/to/liblcg_hip.so] [--detail]
"""
import argparse
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAP = 6
CONVERGED_ROWS = 2051
FACTOR_ROWS = 8197          # IC(0) / ILU(0) as M up to here: the level schedules of the larger systems take seconds per solve


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype} {a.shape} ".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def aligned(a):
    """A copy of the block a (float64 or complex128) whose base is 16-byte aligned."""
    words = a.size * (2 if np.iscomplexobj(a) else 1)
    raw = np.zeros(words + 2)
    off = 0 if raw.ctypes.data % 16 == 0 else 1
    out = raw[off:off + words].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of liblcg_hip.so with the same C ABI")
    ap.add_argument("--detail", action="store_true", help="print every run's line as well (not written to --out)")
    args = ap.parse_args()
    import torch
    from liblcg_amd import _lib
    if args.lib:
        _lib.SO_PATH = os.path.abspath(args.lib)
    from liblcg_amd import api
    import dense_multi_cases as DC
    import multi_bicg_cases as BC
    import multi_cases as MC
    import multi_cplx_cases as ZC
    lib = _lib.load()
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    groups = {}
    t0 = time.time()

    def say(group, s):
        if args.detail:
            print("    " + s, flush=True)
        groups.setdefault(group, []).append(s)

    err = lambda: lib.lcg_hip_last_error().decode()

    def solve(fn, h, k, extra, M, B, cplx, mem, **para):
        """One batched call.  (rc, digest of the results it leaves, its launch counts or None).  The counts are a fact of the call only
        where a column ran to the cap, so that the host enqueued exactly max_iterations bodies: a batch that stops earlier stops the
        host wherever it has got to ahead of the device (24 bodies at the most), and that number is the machine's timing."""
        p = (api.clcg_default_parameters if cplx else api.lcg_default_parameters)(**para)
        ret = (C.c_int * k)(*([99] * k)); its = (C.c_int * k)(*([-1] * k)); res = (C.c_double * k)()
        if mem == "device":
            Md, Bd = torch.from_numpy(np.ascontiguousarray(M).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(B)).cuda()
            rc = fn(h, k, *extra, Md.data_ptr(), Bd.data_ptr(), C.byref(p), ret, its, res, 1)
            torch.cuda.synchronize()
            out = Md.cpu().numpy()
        else:
            out, Bh = aligned(M), aligned(B)
            rc = fn(h, k, *extra, out.ctypes.data, Bh.ctypes.data, C.byref(p), ret, its, res, 0)
        cnt = [C.c_int(-1) for _ in range(4)]
        lib.lcg_hip_last_launches(*[C.byref(c) for c in cnt])
        cap = para.get("max_iterations", 0)
        return (rc, sha(out, np.array(list(ret)), np.array(list(its)), np.array(list(res)).view(np.uint64)),
                [c.value for c in cnt] if rc == 0 and cap > 0 and max(its) >= cap else None)

    def cases(tag, fn, h, extra, n, k, cplx, B, M0, xt, b, converge=True):
        """The runs of one entry on one system at one k."""
        Z = np.zeros_like(B)

        def one(what, M, Bk, mem, **para):
            rc, d, cnt = solve(fn, h, k, extra, M, Bk, cplx, mem, **para)
            say(tag, f"{tag} k={k} {what}: rc {rc} {d} launches " + (" ".join(map(str, cnt)) if cnt else "(stopped before the cap: the host's lead decides)"))

        for rule, para in MC.RULES.items():
            one(f"capped {rule} device", M0, B, "device", max_iterations=CAP, **para)
        one("capped rel host", M0, B, "host", max_iterations=CAP, **MC.RULES["rel"])
        if converge and n <= CONVERGED_ROWS:
            one("converged abs device", Z, B, "device", max_iterations=2000, **MC.RULES["abs"])
            one("uncapped rel host", Z, B, "host", max_iterations=0, epsilon=1e-8, abs_diff=0)
        if k >= 4:
            # column 0: the guess is the solution (already optimised); 1: a NaN in b; 2: the zero guess, running; the rest as they are
            Bm, Mm = B.copy(), Z.copy()
            Bm[:, 0] = b; Mm[:, 0] = xt
            Bm[:, 1] = b; Bm[n // 2, 1] = np.nan
            Bm[:, 2] = b
            for rule, para in MC.RULES.items():
                one(f"mixed verdicts {rule}", Mm, Bm, "device", max_iterations=CAP, **para)

    def ks_of(mod, key):
        return sorted(k for (kind, n, k) in mod.EDGE_CASES if (kind, n) == key) or list(mod.KS)     # (no edge: a module's main system)

    # ---- real CSR: CG, PCG, PCG with M, BiCGStab ------------------------------------------------------------------------------------
    pcg_entries = [("lcg_hip_lcg_multi", lib.lcg_hip_lcg_multi, ()), ("lcg_hip_lpcg_multi", lib.lcg_hip_lpcg_multi, ())]
    pcg_entries += [(f"lcg_hip_lpcg_multi_m {name}", lib.lcg_hip_lpcg_multi_m, (code,))
                    for name, code in (("jacobi", BC.M_JACOBI), ("ic0", BC.M_IC0), ("ilu0", BC.M_ILU0))]
    for key in MC.CLASS:
        S = MC.system(*key)
        A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
        A.build_jacobi(); A.build_ic0(); A.build_ilu0()
        for k in ks_of(MC, key):
            for name, fn, extra in pcg_entries:
                if extra in ((BC.M_IC0,), (BC.M_ILU0,)) and S["n"] > FACTOR_ROWS:
                    continue
                cases(f"{name} {key[0]}-{key[1]}", fn, A.h, extra, S["n"], k, False, MC.columns(S["n"], S["b"], k), MC.guesses(S, k), S["xt"], S["b"])
        A.destroy()
    bicg_entries = [(f"lcg_hip_lbicgstab_multi {name}", lib.lcg_hip_lbicgstab_multi, (code,))
                    for name, code in (("none", BC.M_NONE), ("jacobi", BC.M_JACOBI), ("ic0", BC.M_IC0), ("ilu0", BC.M_ILU0))]
    for key in BC.CLASS:
        S = BC.system(*key)
        A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
        A.build_jacobi(); A.build_ilu0()
        ic0 = lib.lcg_hip_csr_build_ic0(A.h) == 0           # (the matrices are not symmetric: IC(0) takes the lower triangle, where its pivots hold)
        for k in (BC.KS if S["n"] < 30000 else (2, 8)):
            for name, fn, extra in bicg_entries:
                if (extra == (BC.M_IC0,) and not ic0) or (extra in ((BC.M_IC0,), (BC.M_ILU0,)) and S["n"] > FACTOR_ROWS):
                    continue
                cases(f"{name} {key[0]}-{key[1]}", fn, A.h, extra, S["n"], k, False, BC.columns(S["n"], S["b"], k), BC.guesses(S, k), S["xt"], S["b"])
        A.destroy()

    # ---- complex CSR ---------------------------------------------------------------------------------------------------------------------
    for key in ZC.CLASS:
        S = ZC.system(*key)
        A = api.CsrMatrix.from_csr(S["rp"], S["ci"], S["v"])
        A.build_jacobi()
        for k in ks_of(ZC, key):
            for name, fn in (("clcg_hip_lbicg_sym_multi", lib.clcg_hip_lbicg_sym_multi), ("clcg_hip_lpcg_multi", lib.clcg_hip_lpcg_multi)):
                cases(f"{name} {key[0]}-{key[1]}", fn, A.h, (), S["n"], k, True, ZC.columns(S["n"], S["b"], k), ZC.guesses(S, k), S["xt"], S["b"],
                      converge=key[0] != "case1kc")                  # (case1kc: capped runs only)
        A.destroy()

    # ---- dense -----------------------------------------------------------------------------------------------------------------------------
    for shape in [DC.MAIN + (True,)] + [e + (True,) for e in DC.EDGES] + [(200, 200, False)]:
        S = DC.system(*shape)
        D = api.DenseMatrix.from_array(S["K"])
        D.build_jacobi(shape[2])
        for k in DC.KS:
            for name, fn in (("lcg_hip_dense_lcg_multi", lib.lcg_hip_dense_lcg_multi), ("lcg_hip_dense_lpcg_multi", lib.lcg_hip_dense_lpcg_multi)):
                B = DC.columns(S, k)
                cases(f"{name} normal={int(shape[2])} {shape[0]}x{shape[1]}", fn, D.h, (int(shape[2]),), S["n"], k, False, B, np.zeros_like(B), S["xt"], S["b"])
        D.destroy()

    # ---- the refusals: code and text -----------------------------------------------------------------------------------------------------------
    n, k = 8, 4
    rp = np.arange(n + 1, dtype=np.int32); ci = np.arange(n, dtype=np.int32)
    A = api.CsrMatrix.from_csr(rp, ci, np.full(n, 2.0))                            # nothing built
    R = api.CsrMatrix.from_csr(np.array([0, 1, 2]), np.array([0, 2]), np.array([1.0, 2.0]), n_cols=3)
    Ac = api.CsrMatrix.from_csr(rp, ci, np.full(n, 2.0 + 1.0j))
    Rc = api.CsrMatrix.from_csr(np.array([0, 1, 2]), np.array([0, 2]), np.array([1.0 + 1j, 2.0]), n_cols=3)
    D = api.DenseMatrix.from_array(np.eye(n) * 2.0)
    Dr = api.DenseMatrix.from_array(np.ones((n + 2, n)))
    Dc = api.DenseMatrix.from_array(np.eye(n) + 0j)
    M = torch.zeros(2 * n * 8 + 2, dtype=torch.float64, device="cuda")
    B = torch.ones(2 * n * 8 + 2, dtype=torch.float64, device="cuda")
    pm, pb = M.data_ptr(), B.data_ptr()
    ret = (C.c_int * 8)(); its = (C.c_int * 8)(); res = (C.c_double * 8)()

    def refusals(state):
        for name, fn, extra, cplx, sq, nonsq, other in (
                [("lcg_hip_lcg_multi", lib.lcg_hip_lcg_multi, (), False, A, R, Ac), ("lcg_hip_lpcg_multi", lib.lcg_hip_lpcg_multi, (), False, A, R, Ac)]
                + [(f"lcg_hip_lpcg_multi_m({m})", lib.lcg_hip_lpcg_multi_m, (m,), False, A, R, Ac) for m in (-1, 0, 1, 2, 5)]
                + [(f"lcg_hip_lbicgstab_multi({m})", lib.lcg_hip_lbicgstab_multi, (m,), False, A, R, Ac) for m in (-2, -1, 0, 1, 2, 5)]
                + [("clcg_hip_lbicg_sym_multi", lib.clcg_hip_lbicg_sym_multi, (), True, Ac, Rc, A), ("clcg_hip_lpcg_multi", lib.clcg_hip_lpcg_multi, (), True, Ac, Rc, A)]
                + [(f"{nm}(normal={nrm})", f, (nrm,), False, D, Dr, Dc) for nm, f in (("lcg_hip_dense_lcg_multi", lib.lcg_hip_dense_lcg_multi),
                                                                                     ("lcg_hip_dense_lpcg_multi", lib.lcg_hip_dense_lpcg_multi)) for nrm in (0, 1, 2)]):
            mk = api.clcg_default_parameters if cplx else api.lcg_default_parameters
            good = mk(epsilon=1e-8, abs_diff=0, max_iterations=3)
            for what, kw in (("k=3", dict(kk=3)), ("k=0", dict(kk=0)), ("k=16", dict(kk=16)), ("M misaligned", dict(m=pm + 8)),
                             ("B misaligned", dict(b=pb + 8)), ("M null", dict(m=None)), ("B null", dict(b=None)), ("no handle", dict(h=None)),
                             ("other type's handle", dict(h=other.h)), ("not square", dict(h=nonsq.h)), ("mem=7", dict(mem=7)),
                             ("mem=7, epsilon=0", dict(mem=7, p=mk(epsilon=0.0))), ("epsilon=0", dict(p=mk(epsilon=0.0))),
                             ("epsilon=1", dict(p=mk(epsilon=1.0))), ("max_iterations=-1", dict(p=mk(epsilon=1e-8, max_iterations=-1))),
                             ("default parameters", dict(p=None)), ("as it is", {})):
                a = dict(h=sq.h, kk=k, m=pm, b=pb, p=good, mem=1)
                a.update(kw)
                rc = fn(a["h"], a["kk"], *extra, a["m"], a["b"], C.byref(a["p"]) if a["p"] is not None else None, ret, its, res, a["mem"])
                torch.cuda.synchronize()
                say(f"refusals ({state}) {name}", f"refusal ({state}) {name} {what}: {rc}: {err()}")

    refusals("nothing built")
    A.build_jacobi(); Ac.build_jacobi(); D.build_jacobi(True)
    refusals("Jacobi built, the dense one for K^T.K")
    A.build_ic0(); D.build_jacobi(False)
    refusals("IC(0) built, the dense Jacobi for K")
    A.build_ilu0()
    refusals("all built")
    for h in (A, R, Ac, Rc, D, Dr, Dc):
        h.destroy()
    lines = [f"{g}: {len(runs)} lines {hashlib.sha256(chr(10).join(runs).encode()).hexdigest()}" for g, runs in groups.items()]
    print("\n".join(lines), flush=True)
    print(f"{sum(len(r) for r in groups.values())} runs in {time.time() - t0:.1f} s", file=sys.stderr)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
