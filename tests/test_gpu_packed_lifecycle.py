"""-m gpu: the life cycle of ONE handle's packed plan (csr_packed.hip) under all four of its setters -- lcg_hip_csr_set_packed,
_set_run_stretches, _set_sym_runs / _set_sym_slices -- and destroy.  After every change of a switch the handle must multiply, name its
kernel, report its plan and account for its memory exactly as a fresh handle that was given the same switches before its first
product: whatever a setter releases is released whole, whatever it keeps is what a first build would have made.  The one exception
is kept on purpose and asserted as it is: switching the symmetric mode off releases the half store alone, so the plan built for it
keeps its stretches' offset tables (192 bytes per stretch).  The systems and helpers are those of tests/test_gpu_sym_runs.py."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
from test_gpu_sym_runs import P7, P16, bits_equal, kernel, plan, rows_for, system

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NX = 2
TABLE_BYTES = 16 * 12       # one stretch's offset table: four wavefronts x RS_QMIN = 12 slots (rows of up to 48 entries), 4 bytes each


@pytest.fixture(scope="module")
def api():
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


@pytest.fixture(scope="module")
def lib():
    from liblcg_amd import _lib
    return _lib.load()


def extra_bytes(lib, A):
    b = C.c_int64(0)
    assert lib.lcg_hip_csr_plan_info(A.h, None, C.byref(b)) == 0
    return b.value


def report(lib, A):
    """Everything a caller can ask about the plan: kernel name, (run blocks, blocks), (stretches, their blocks), (slices, sliced
    blocks, status), plan bytes."""
    pb, rb = C.c_int64(0), C.c_int64(0)
    runs = lib.lcg_hip_csr_packed_runs(A.h, C.byref(pb))
    st = lib.lcg_hip_csr_run_stretches(A.h, C.byref(rb))
    return {"kernel": kernel(lib, A), "runs": (runs, pb.value), "stretches": (st, rb.value), "sym": A.sym_runs(), "extra": extra_bytes(lib, A)}


def apply(lib, A, packed, stretches, sym):
    assert lib.lcg_hip_csr_set_packed(A.h, packed) == 0
    assert lib.lcg_hip_csr_set_run_stretches(A.h, stretches) == 0
    A.set_sym_runs(*sym)


@pytest.mark.parametrize("name,offs", [("7 pairs", P7), ("16 pairs", P16)])
def test_setters_on_one_handle(api, lib, name, offs):
    """Three blocks per slice of eight (a stretch of 26 and more run blocks, an inner range for two slices), n no multiple of 64."""
    rng = np.random.default_rng(4100 + len(offs))
    n = rows_for(offs, 3)
    rp, col, val = system(n, offs, rng)
    x = rng.standard_normal(n)
    xd = torch.from_numpy(x).cuda()
    b0, b1, Q, inner0, Sx = plan(n, offs, NX)
    assert b1 - b0 >= 2 and Sx >= 1 and 2000 < n < 5000

    def product(A, fill):
        y = torch.full((n,), fill, dtype=torch.float64, device="cuda")
        A.spmv(xd, y); api.synchronize()
        return y

    A = api.CsrMatrix.from_csr(rp, col, val)
    A.set_kernel(-64)
    before = extra_bytes(lib, A)        # no plan of any kind yet
    # (what the step sets on the living handle, the switches a fresh handle gets: packed mode, stretches, (symmetric mode, slices))
    steps = [("stretches off, symmetric off", lambda: apply(lib, A, 1, 0, (0, 0)), (1, 0, (0, 0))),
             ("set_run_stretches(1)", lambda: lib.lcg_hip_csr_set_run_stretches(A.h, 1), (1, 1, (0, 0))),
             ("set_sym_runs(1, 2)", lambda: A.set_sym_runs(1, NX), (1, 1, (1, NX))),
             ("set_packed(0)", lambda: lib.lcg_hip_csr_set_packed(A.h, 0), (0, 1, (1, NX))),
             ("set_packed(1)", lambda: lib.lcg_hip_csr_set_packed(A.h, 1), (1, 1, (1, NX))),
             ("set_run_stretches(0)", lambda: lib.lcg_hip_csr_set_run_stretches(A.h, 0), (1, 0, (1, NX))),
             # (the mode alone first: the half store goes and the plan stays.  Through set_sym_runs(0, 0) at once the change of the
             #  slice count, made while the mode still wants a stretch, would release the whole plan.)
             ("symmetric mode off, slices kept", lambda: lib.lcg_hip_csr_set_sym_runs(A.h, 0), (1, 0, (0, NX))),
             ("set_sym_runs(0, 0)", lambda: A.set_sym_runs(0, 0), (1, 0, (0, 0)))]
    tables_stay = ("symmetric mode off, slices kept", "set_sym_runs(0, 0)")
    y_first, nstretch = None, 0
    for i, (what, change, switches) in enumerate(steps):
        assert change() in (None, 0), what
        y = product(A, 3.0 + i)
        got = report(lib, A)
        F = api.CsrMatrix.from_csr(rp, col, val)
        F.set_kernel(-64)
        apply(lib, F, *switches)
        yf = product(F, -7.0 - i)
        want = report(lib, F)
        F.destroy()
        print(f"{name}, n {n}, step {i + 1} {what}: {got}")
        assert bits_equal(y, yf), what
        if y_first is None:
            y_first = y
            X.assert_rows(y.cpu().numpy(), rp, col, val, x, (name, what))
        assert bits_equal(y, y_first), what         # (every form of the product adds a row's entries in the same order)
        packed, stretches, (sym, _) = switches
        if what in tables_stay:
            # the one place where the handle deliberately differs from a fresh one: only the half store is released, the plan that was
            # built while stretches were looked for stays, and with it its stretches' offset tables, resident though unused
            # (tests/test_gpu_sym_runs.py allows "< 1 KB" for them); a fresh handle with both switches off never looks for stretches
            assert got["extra"] - want["extra"] == TABLE_BYTES * nstretch, (what, got, want)
            got["extra"] = want["extra"]
        assert got == want, (what, got, want)
        # and what each state is, so that the two handles cannot agree on something else
        if packed == 0:
            assert got["kernel"].startswith("k_spmv_lds1 ") and got["extra"] == before and got["runs"][0] == 0, (what, got)
            assert got["stretches"] == (0, 0) and got["sym"] == (0, 0, "not tried"), (what, got)
            continue
        assert got["kernel"].startswith("k_spmv_ldsp (") and got["runs"][0] >= b1 - b0 and got["runs"][1] == (n + 63) // 64, (what, got)
        assert ("k_spmv_ldsp_sym" in got["kernel"]) == (sym == 1), (what, got)
        assert got["sym"] == ((NX, NX * Sx, "taken") if sym == 1 else (0, 0, "not tried")), (what, got)
        if stretches:
            nstretch = got["stretches"][0]
            assert nstretch >= 1 and got["stretches"][1] >= b1 - b0, (what, got)
        else:
            assert got["stretches"] == (0, 0), (what, got)
    A.destroy()
    assert not A.h


def test_released_plan_keeps_its_numbers(api, lib):
    """What the status queries answer once a plan is released -- on purpose what they always answered: lcg_hip_csr_packed_runs keeps
    counting blocks of the released plan's rows per block, and the traffic model of the latest product (which used the plan) stays
    what it was until the next product.  Rows of 49 entries: the packed form takes blocks of 32 rows, so the count differs from a
    fresh handle's (blocks of 64)."""
    rng = np.random.default_rng(4177)
    offs = list(range(1, 49, 2))                        # 24 pairs
    n = 2000 + 37
    rp, col, val = system(n, offs, rng)
    x = rng.standard_normal(n)
    xd = torch.from_numpy(x).cuda()

    def look(A):
        y = torch.full((n,), 9.0, dtype=torch.float64, device="cuda")
        A.spmv(xd, y); api.synchronize()
        return y

    def ask(A):
        pb = C.c_int64(0)
        runs = lib.lcg_hip_csr_packed_runs(A.h, C.byref(pb))
        return runs, pb.value, lib.lcg_hip_csr_last_traffic_model(A.h), extra_bytes(lib, A)

    A = api.CsrMatrix.from_csr(rp, col, val)
    fresh = ask(A)
    assert fresh[:2] == (0, (n + 63) // 64) and fresh[3] == 0, fresh
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    y1 = look(A)
    k1, built = kernel(lib, A), ask(A)
    print(f"long rows, n {n}: {k1}; built {built}")
    assert k1.startswith("k_spmv_ldsp (LDS-staged, long rows"), k1
    R = 32
    assert built[:2] == (0, (n + R - 1) // R) and built[3] > 0, built
    X.assert_rows(y1.cpu().numpy(), rp, col, val, x, "long rows")
    assert lib.lcg_hip_csr_set_packed(A.h, 0) == 0
    released = ask(A)
    print(f"released {released}")
    assert released == (0, (n + R - 1) // R, built[2], 0), (released, built)     # the block count and the last product's model stay; the memory is back
    y2 = look(A)
    k2, plain = kernel(lib, A), ask(A)
    assert k2.startswith("k_spmv_lds1 ") and bits_equal(y1, y2), k2
    assert plain[:2] == (0, (n + R - 1) // R) and plain[3] == 0, plain          # (still the released plan's rows per block)
    assert plain[2] == 12 * len(col) + 4 * (n + 1) + 16 * n, plain              # the CSR arrays as they are
    assert lib.lcg_hip_csr_set_packed(A.h, 1) == 0
    y3 = look(A)
    assert kernel(lib, A) == k1 and ask(A) == built and bits_equal(y1, y3)
    A.destroy()
