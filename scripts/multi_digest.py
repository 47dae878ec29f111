"""SHA-256 of everything a caller can read from the batched solvers on a fixed list of small systems, through the Python view of
the C ABI only: run on two builds of the library, the two outputs are identical line for line when the builds compute the same bits
and enqueue the same launches.

Entries, the loops: lcg_hip_lcg_multi, lcg_hip_lpcg_multi, lcg_hip_lpcg_multi_m (Jacobi, IC(0), ILU(0)), lcg_hip_lbicgstab_multi (none, Jacobi,
IC(0), ILU(0)), clcg_hip_lbicg_sym_multi, clcg_hip_lpcg_multi, lcg_hip_dense_lcg_multi and lcg_hip_dense_lpcg_multi (normal = 1, 0),
clcg_hip_dense_lbicg_sym_multi and clcg_hip_dense_lpcg_multi.  The products under them: lcg_hip_spmm, _spmm_dot, _spmm_dot2 and
clcg_hip_spmm, _spmm_dot on the same CSR systems (the CLASS lists hold a system of more than MM_MG row blocks per class, so the
fold of the partial sums runs); lcg_hip_dense_matmat (both layouts), lcg_hip_dense_ata_multi and lcg_hip_dense_op_multi_dot on the
real dense shapes, clcg_hip_dense_matmat (both layouts, both conjugations) and clcg_hip_dense_op_multi_dot on the sizes of
tests/dense_multi_cplx_cases.py, each under the automatic variant and under the forced row forms (lcg_hip_dense_set_kernel 1, 2; a
refused variant leaves its code and text), with lcg_hip_dense_multi_last_kernel after every call.  Per product: the return code and
one hash over the block it wrote and the sums it returned.
Systems: the CLASS lists of tests/multi_cases.py, multi_bicg_cases.py and multi_cplx_cases.py with the k of their EDGE_CASES, the
shapes of tests/dense_multi_cases.py.  Per system and k: runs capped at 6 iterations under both stop rules in device memory and
under the relative rule in host memory; a converged run (cap 2000) and a run with max_iterations = 0 where the system has at most
CONVERGED_ROWS rows; for k >= 4 a batch of mixed verdicts (a column already optimised, a NaN column, running columns); IC(0) and
ILU(0) as M on the systems of at most FACTOR_ROWS rows.  Per run: the return code, one hash over the solution block, ret,
iterations and the bits of residual, and the four counts of lcg_hip_last_launches -- those where a column ran to the cap; a batch
that stops earlier leaves counts that depend on how far ahead of the device the host had enqueued (see solve()).  Last, the code and
text of every refusal of every entry, with nothing built, then Jacobi, then IC(0), then everything; and of the product entries,
each also with two faults at once, so that the order of their checks is part of the digest.

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
    import dense_multi_cplx_cases as ZD
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

    def block(rows, k, seed, cplx=False):
        """A (rows, k) block of seeded values on the device, float64 or complex128."""
        r = np.random.default_rng(seed)
        a = r.uniform(-1.0, 1.0, (rows, k)) + (1j * r.uniform(-1.0, 1.0, (rows, k)) if cplx else 0.0)
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def product(tag, what, fn, h, k, args, Y, ndots=0, last=None):
        """One product call: Y is what it writes, ndots the doubles it returns, last the handle whose kernel name follows."""
        Y.fill_(-7.0)
        dots = (C.c_double * max(ndots, 1))(*([-7.0] * max(ndots, 1)))
        rc = fn(h, k, *[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args], *([dots] if ndots else []))
        torch.cuda.synchronize()
        name = (" " + lib.lcg_hip_dense_multi_last_kernel(last).decode()) if last is not None else ""
        say(tag, f"{tag} k={k} {what}: rc {rc} {sha(Y.cpu().numpy(), np.array(list(dots)[:ndots]).view(np.uint64))}{name}")

    def csr_products(tag, A, n, k, cplx):
        X, U, Y = block(n, k, 11 * n + k, cplx), block(n, k, 13 * n + k, cplx), block(n, k, 1, cplx)
        if cplx:
            product(f"clcg_hip_spmm {tag}", "A.X", lib.clcg_hip_spmm, A.h, k, (X, Y), Y)
            product(f"clcg_hip_spmm_dot {tag}", "A.X, sums", lib.clcg_hip_spmm_dot, A.h, k, (X, Y, U), Y, 2 * k)
        else:
            product(f"lcg_hip_spmm {tag}", "A.X", lib.lcg_hip_spmm, A.h, k, (X, Y), Y)
            product(f"lcg_hip_spmm_dot {tag}", "A.X, sums", lib.lcg_hip_spmm_dot, A.h, k, (X, Y, U), Y, k)
            product(f"lcg_hip_spmm_dot2 {tag}", "A.X, both sums", lib.lcg_hip_spmm_dot2, A.h, k, (X, Y, U), Y, 2 * k)

    def variants(tag, D):
        """The automatic variant, then the forced row forms the handle accepts (a refusal leaves its code and text)."""
        for v in (0, 1, 2):
            rc = lib.lcg_hip_dense_set_kernel(D.h, v)
            if rc:
                say(tag, f"{tag} variant {v}: refused {rc}: {err()}")
            else:
                yield v
        lib.lcg_hip_dense_set_kernel(D.h, 0)

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
            csr_products(f"{key[0]}-{key[1]}", A, S["n"], k, False)
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
            csr_products(f"{key[0]}-{key[1]}", A, S["n"], k, True)
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
        m, n = shape[0], shape[1]
        tag = f"{m}x{n}"
        for v in variants(f"lcg_hip_dense_set_kernel {tag}", D):
            for k in DC.KS:
                Xn, Xm, U, Yn, Ym = block(n, k, 17 * n + k), block(m, k, 19 * m + k), block(n, k, 23 * n + k), block(n, k, 1), block(m, k, 1)
                product(f"lcg_hip_dense_matmat {tag}", f"variant {v} K.X", lib.lcg_hip_dense_matmat, D.h, k, (Xn, Ym, 0), Ym, last=D.h)
                product(f"lcg_hip_dense_matmat {tag}", f"variant {v} K^T.X", lib.lcg_hip_dense_matmat, D.h, k, (Xm, Yn, 1), Yn, last=D.h)
                product(f"lcg_hip_dense_ata_multi {tag}", f"variant {v}", lib.lcg_hip_dense_ata_multi, D.h, k, (Xn, Yn), Yn, last=D.h)
                for normal in (1, 0) if m == n else (1,):
                    product(f"lcg_hip_dense_op_multi_dot {tag}", f"variant {v} normal={normal}", lib.lcg_hip_dense_op_multi_dot, D.h, k,
                            (normal, Xn, Yn, U), Yn, k, last=D.h)
        D.destroy()

    # ---- complex dense -------------------------------------------------------------------------------------------------------------------
    for n in ZD.SIZES:
        S = ZD.system(n)
        D = api.DenseMatrix.from_array(S["K"])
        D.build_jacobi(False)
        tag = f"{n}x{n}"
        for v in variants(f"lcg_hip_dense_set_kernel complex {tag}", D):
            for k in ZD.KS:
                X, U, Y = block(n, k, 29 * n + k, True), block(n, k, 31 * n + k, True), block(n, k, 1, True)
                for layout in (0, 1):
                    for conj in (0, 1):
                        product(f"clcg_hip_dense_matmat {tag}", f"variant {v} layout={layout} conjugate={conj}", lib.clcg_hip_dense_matmat, D.h, k,
                                (X, Y, layout, conj), Y, last=D.h)
                product(f"clcg_hip_dense_op_multi_dot {tag}", f"variant {v}", lib.clcg_hip_dense_op_multi_dot, D.h, k, (X, Y, U), Y, 2 * k, last=D.h)
                B = ZD.columns(S, k)
                for name, fn in (("clcg_hip_dense_lbicg_sym_multi", lib.clcg_hip_dense_lbicg_sym_multi), ("clcg_hip_dense_lpcg_multi", lib.clcg_hip_dense_lpcg_multi)):
                    cases(f"{name} variant {v} {tag}", fn, D.h, (), n, k, True, B, np.zeros_like(B), S["xt"], S["b"])
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

    def product_refusals():
        """The product entries: every fault alone and two at once (which of the two is named says where the checks stand)."""
        dots = (C.c_double * 16)()
        px, py, pu = pm, pb, pm + 16 * n * 4          # X, Y in different tensors; U in X's tensor, behind a complex block of k = 4 columns
        csr = [("lcg_hip_spmm", lib.lcg_hip_spmm, A, Ac, False, 0), ("lcg_hip_spmm_dot", lib.lcg_hip_spmm_dot, A, Ac, False, 1),
               ("lcg_hip_spmm_dot2", lib.lcg_hip_spmm_dot2, A, Ac, False, 1), ("clcg_hip_spmm", lib.clcg_hip_spmm, Ac, A, True, 0),
               ("clcg_hip_spmm_dot", lib.clcg_hip_spmm_dot, Ac, A, True, 1)]
        for name, fn, good, other, cplx, dotted in csr:
            for what, kw in (("k=3", dict(kk=3)), ("X misaligned", dict(x=px + 8)), ("Y null", dict(y=None)), ("no handle", dict(h=None)),
                             ("other type's handle", dict(h=other.h)), ("dense handle", dict(h=D.h)), ("null dots", dict(d=None)),
                             ("other type's handle and null dots", dict(h=other.h, d=None)), ("no handle and null dots", dict(h=None, d=None)),
                             ("k=3 and null dots", dict(kk=3, d=None)), ("U misaligned and other type's handle", dict(u=pu + 8, h=other.h)),
                             ("as it is", {})):
                a = dict(h=good.h, kk=k, x=px, y=py, u=pu, d=dots)
                a.update(kw)
                rc = fn(a["h"], a["kk"], a["x"], a["y"], *((a["u"], a["d"]) if dotted else ()))
                torch.cuda.synchronize()
                say(f"refusals products {name}", f"refusal {name} {what}: {rc}: {err()}")
        dense = [("lcg_hip_dense_matmat", lib.lcg_hip_dense_matmat, D, Dc, (0,), 0), ("lcg_hip_dense_ata_multi", lib.lcg_hip_dense_ata_multi, D, Dc, (), 0),
                 ("lcg_hip_dense_op_multi_dot", lib.lcg_hip_dense_op_multi_dot, D, Dc, (1,), 1),
                 ("clcg_hip_dense_matmat", lib.clcg_hip_dense_matmat, Dc, D, (0, 0), 0),
                 ("clcg_hip_dense_op_multi_dot", lib.clcg_hip_dense_op_multi_dot, Dc, D, (), 1)]
        for name, fn, good, other, extra, dotted in dense:
            for what, kw in (("k=3", dict(kk=3)), ("X misaligned", dict(x=px + 8)), ("Y null", dict(y=None)), ("no handle", dict(h=None)),
                             ("other type's handle", dict(h=other.h)), ("CSR handle", dict(h=A.h)), ("X and Y overlap", dict(y=px + 16)),
                             ("X misaligned and X and Y overlap", dict(x=px + 8, y=px + 16)), ("other type's handle and X and Y overlap", dict(h=other.h, y=px + 16)),
                             ("bad flag", dict(extra=tuple(7 for _ in extra))), ("bad flag and X and Y overlap", dict(extra=tuple(7 for _ in extra), y=px + 16)),
                             ("not square", dict(h=Dr.h)), ("dots without U", dict(u=None)), ("Y overlaps U and dots without U", dict(u=None, y=px + 16)),
                             ("other type's handle and null dots", dict(h=other.h, d=None)), ("as it is", {})):
                a = dict(h=good.h, kk=k, x=px, y=py, u=pu, d=dots, extra=extra)
                a.update(kw)
                if name.startswith("lcg_hip_dense_op"):
                    args = (a["h"], a["kk"], *a["extra"], a["x"], a["y"], a["u"], a["d"])
                elif dotted:
                    args = (a["h"], a["kk"], a["x"], a["y"], a["u"], a["d"])
                else:
                    args = (a["h"], a["kk"], a["x"], a["y"], *a["extra"])
                rc = fn(*args)
                torch.cuda.synchronize()
                say(f"refusals products {name}", f"refusal {name} {what}: {rc}: {err()}")

    product_refusals()
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
