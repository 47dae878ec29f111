"""-m gpu: consecutive blocks per XCD in the symmetric product's one slice (csr_sym.hip; LCG_HIP_SYM_GROUP).  G = 1, 2, 4 or 8: the
workgroups of every full window of 8 G blocks are permuted so that one XCD takes G consecutive blocks; the same blocks, the same
sums in the same order, so y and every carried sum keep their bits for every G -- compared as 64-bit integers with the product of
the mode off, which is held to exact row sums (exact_ref).  Inner ranges of 70 blocks (one window and six blocks at G = 8, more
windows below), exactly 64, 19 (a window at G = 2 only), 10 and 3 (no window: the order stays), n never a multiple of 64; offsets
without a straddling line (64), with the partner in the same or the neighbouring block (37), and 16 pairs.  The systems and helpers
are those of test_gpu_sym_runs.py.

The count is the process's (the environment is read once), so the default runs in this process and every other count in a child of
its own: this file run as a program does the same cases and prints what it found as one JSON line; the children run side by side."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import exact_ref as X
import test_gpu_sym_runs as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GROUPS = {1: None, 2: "one slice, two consecutive blocks per XCD", 4: "one slice, four consecutive blocks per XCD", 8: "one slice, eight consecutive blocks per XCD"}
DEFAULT = 4         # csr_sym.hip: SYM_GROUP_DEFAULT
OFFSETS = [("1 pair, 64", R.P1_64), ("1 pair, 37", R.P1_37), ("16 pairs", R.P16)]
RANGES = [70, 64, 19, 10, 3]


def rows_for_inner(offs, S, tail=37):
    """n so that ONE slice gets an inner range of exactly S blocks and the last block of the matrix is partial."""
    m = max(offs)
    inner0 = R.plan(10 ** 6, offs, 1)[3]
    n = 64 * (inner0 + S) + m + tail
    assert R.plan(n, offs, 1)[3:] == (inner0, S) and n % 64 != 0
    return n


def named(k, G):
    """The kernel string names the group when it is not one, and one slice always."""
    if "k_spmv_ldsp_sym" not in k or "one slice" not in k:
        return False
    return GROUPS[G] in k if G > 1 else "blocks per XCD" not in k


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run_cases(api, lib, G):
    """Every case under the count G this process runs with.  Asserts what one process can see (the kernel string, the bits of the
    mode off, exact row sums) and returns what the counts must agree on: hashes of y, the carried sums, the solvers' answers."""
    out = {}
    # products
    for name, offs in OFFSETS:
        for S in RANGES:
            rng = np.random.default_rng(1900 + 10 * len(offs) + S)
            n = rows_for_inner(offs, S)
            rp, col, val = R.system(n, offs, rng)
            x = rng.standard_normal(n)
            xd = torch.from_numpy(x).cuda()
            A = api.CsrMatrix.from_csr(rp, col, val)
            A.set_kernel(-64)
            assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
            A.set_sym_runs(0, 1)
            y_off = torch.full((n,), 4.0, dtype=torch.float64, device="cuda")
            A.spmv(xd, y_off); api.synchronize()
            assert "k_spmv_ldsp_sym" not in R.kernel(lib, A)
            X.assert_rows(y_off.cpu().numpy(), rp, col, val, x, (name, S))
            A.set_sym_runs(1, 1)
            y = torch.full((n,), 5.0, dtype=torch.float64, device="cuda")
            A.spmv(xd, y); api.synchronize()
            k, took = R.kernel(lib, A), A.sym_runs()
            assert took == (1, S, "taken"), (took, S)
            assert named(k, G), (G, k)
            assert R.bits_equal(y, y_off), (name, S, G)
            out[f"product {name} S {S}"] = sha(y)
            A.destroy()
    # carried dot and solves: 16 pairs, an inner range of 90 blocks (G = 8: one window and 26 blocks behind it)
    rng = np.random.default_rng(1960)
    n = rows_for_inner(R.P16, 90)
    rp, col, val = R.system(n, R.P16, rng)
    A = api.CsrMatrix.from_csr(rp, col, val)
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    x = torch.from_numpy(rng.standard_normal(n)).cuda()
    u = torch.from_numpy(rng.standard_normal(n)).cuda()
    b = torch.from_numpy(rng.standard_normal(n)).cuda()
    A.set_kernel(0)
    got = {}
    for mode in (1, 0):
        A.set_sym_runs(mode, 1)
        for uname, uu in (("u=x", x), ("u", u)):
            y = torch.full((n,), 2.0, dtype=torch.float64, device="cuda")
            res = (C.c_double * 2)()
            assert lib.lcg_hip_spmv_dot(A.h, x.data_ptr(), y.data_ptr(), uu.data_ptr(), res) == 0
            k = R.kernel(lib, A)
            assert "carrying the dot" in k and (named(k, G) if mode else "k_spmv_ldsp_sym" not in k), (G, mode, k)
            got[mode, uname] = (y, res[0], res[1])
    for uname in ("u=x", "u"):
        a, c = got[1, uname], got[0, uname]
        assert R.bits_equal(a[0], c[0]) and a[1] == c[1] and a[2] == c[2], (G, uname, a[1:], c[1:])
        out[f"dot {uname}"] = [sha(a[0]), float(a[1]).hex(), float(a[2]).hex()]
    X.assert_rows(got[0, "u"][0].cpu().numpy(), rp, col, val, x.cpu().numpy(), ("carried dot",))
    for eps, cap in ((1e-300, 30), (1e-12, 200)):
        off = R._solve(api, lib, A, n, b, eps, cap, 0, 1)
        assert off[1][1] == 30 if cap == 30 else 3 < off[1][1] < 200, off
        on = R._solve(api, lib, A, n, b, eps, cap, 1, 1)
        assert named(R.kernel(lib, A), G), (G, R.kernel(lib, A))
        assert on == off, (G, on, off)
        out[f"solve cap {cap}"] = [on[0], on[1][0], on[1][1], float(on[1][2]).hex()]
    A.destroy()
    # eight slices: their own placement whatever the count says; the kernel string names no group
    rng = np.random.default_rng(1970)
    n = R.rows_for(R.P16, 3)
    rp, col, val = R.system(n, R.P16, rng)
    xs = rng.standard_normal(n)
    A = api.CsrMatrix.from_csr(rp, col, val)
    ys, k_on, took, *_ = R.on_off(api, lib, A, n, xs, 8)
    assert took == (8, 24, "taken"), took
    assert "k_spmv_ldsp_sym" in k_on and "eight slices" in k_on and "blocks per XCD" not in k_on, k_on
    assert R.bits_equal(ys[0], ys[1])
    X.assert_rows(ys[1].cpu().numpy(), rp, col, val, xs, ("eight slices",))
    out["eight slices"] = sha(ys[0])
    A.destroy()
    return out


@pytest.fixture(scope="module")
def default_run():
    from liblcg_amd import _lib, api
    assert torch.cuda.is_available()
    assert "LCG_HIP_SYM_GROUP" not in os.environ, "the suite runs with the default count"
    return run_cases(api, _lib.load(), DEFAULT)


def test_default(default_run):
    """Nothing set: four consecutive blocks per XCD, says the kernel string; every product, carried sum and solve has the bits of the
    mode off (asserted case by case in run_cases)."""
    assert len(default_run) == len(OFFSETS) * len(RANGES) + 2 + 2 + 1


def test_every_count_and_a_bad_one(default_run):
    """LCG_HIP_SYM_GROUP = 1, 2, 4, 8 in a child each: the same cases pass there under that count's kernel string, and the hashes of y,
    the carried sums, the iterates' SHA-256, the counts and the residuals are those of the default.  A value that is no count (3) is
    ignored: the default's kernel string, the same bits."""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    kids = {v: subprocess.Popen(cmd, env=dict(os.environ, LCG_HIP_SYM_GROUP=str(v)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for v in (1, 2, 4, 8, 3)}
    try:
        for v, p in kids.items():
            so, se = p.communicate(timeout=120)
            assert p.returncode == 0, (v, so[-500:], se[-3000:])
            got = json.loads(so.strip().splitlines()[-1])
            assert got["G"] == (v if v in GROUPS else DEFAULT), (v, got["G"])
            assert got["cases"] == json.loads(json.dumps(default_run)), (v, {k: (w, default_run.get(k)) for k, w in got["cases"].items() if w != default_run.get(k)})
    finally:        # whatever ended the loop, no child stays behind with the GPU open
        for p in kids.values():
            if p.poll() is None:
                p.kill()
            p.wait()


if __name__ == "__main__":
    from liblcg_amd import _lib, api
    asked = int(os.environ["LCG_HIP_SYM_GROUP"])
    G = asked if asked in GROUPS else DEFAULT
    print(json.dumps({"G": G, "cases": run_cases(api, _lib.load(), G)}))
