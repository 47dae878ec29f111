#!/usr/bin/env python3
"""Generate tests/golden/ref_pins.npz from the REAL liblcg native back-end.

Run where the reference sources exist (the compiled reference is needed):

    make -C oracle ref && python tests/golden/make_ref_pins.py

The cases, their inputs and the record keys are those of tests/test_oracle_vs_ref.py (imported
from it), so the pins and the checks cannot drift apart.  Each record holds the reference's return
code, iteration count, last monitored residual, solution vector (as the SHA-256 of its bytes, with
its first entries) and -- for the complex solvers that draw a shadow residual from srand(time(0)) --
the clock second that seeded the draw.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import test_oracle_vs_ref as T  # noqa: E402
from liblcg_amd.coo_io import coo_to_csr_host, read_coo_system  # noqa: E402
from oracle import pyoracle as po  # noqa: E402


def main():
    ref, port = po.Oracle("reference"), po.Oracle("port")
    out = {"sizes": np.array([ref.lib.ref_sizeof_lcg_para(), ref.lib.ref_sizeof_clcg_para()], np.int64)}

    def put(key, r):
        for k, a in T.record(r).items():
            out[f"{key}/{k}"] = a
        print(key, r["ret"], r["iters"], r["residual"], r.get("seed_before", ""))

    n, row, col, val, _ = read_coo_system(os.path.join(HERE, "case_10K_A"))
    rp, ci, v = coo_to_csr_host(n, row, col, val)
    for sid, jac in T.RHS_SIDS:
        b, m0 = T.rhs_inputs(n, sid)
        for eps, ad in T.RHS_TOLS:
            put(T.rhs_key(sid, eps, ad), ref.solve(sid, rp, ci, v, b, m0=m0, para=T.rhs_para(eps, ad), jacobi=bool(jac)))

    for tag, n, band, sym, pattern, sids in T.GEN_SYSTEMS:
        grp, gci, gv, b, m0 = T.gen_inputs(port, tag, n, band, sym, pattern)
        for sid in sids:
            for eps, ad in T.GEN_TOLS:
                put(T.gen_key(tag, sid, eps), ref.solve(sid, grp, gci, gv, b, m0=m0, para=T.gen_para(eps, ad), jacobi=(sid == 1)))

    n, row, col, val, b = read_coo_system(os.path.join(HERE, "case_1K_cA"), True)
    rp, ci, v = coo_to_csr_host(n, row, col, val)
    for kind, sids, para in (("seed_replay", T.SEED_REPLAY_SIDS, T.seed_replay_para()), ("other_two", T.OTHER_TWO_SIDS, T.other_two_para())):
        for sid in sids:
            while True:
                r = ref.csolve(sid, rp, ci, v, b, para=para)
                if r["seed_before"] == r["seed_after"]:
                    break
            put(T.cplx_key(kind, sid), r)

    a, b = T.dot_inputs()
    out["dot"] = np.array([ref.dot(a, b)], np.float64)
    assert tuple(out["sizes"]) == (ctypes.sizeof(po.Para), ctypes.sizeof(po.CPara))
    np.savez_compressed(os.path.join(HERE, "ref_pins.npz"), **out)
    print("wrote", os.path.join(HERE, "ref_pins.npz"))


if __name__ == "__main__":
    main()
