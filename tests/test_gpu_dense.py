"""Dense operators on the GPU (liblcg_amd/csrc/dense.hip): K.x, K^T.x, K^T.K.x and the four complex forms against exact
integer sums (bit for bit) and per-row rounding bounds (tests/exact_ref.py), every kernel path reached, the same bits from call
to call, the Jacobi builds against tests/dense_checker.py, and the solver loops through the dense callbacks against the
oracle's own loops driven by the checker's product."""
import ctypes as C
import math

import numpy as np
import pytest

import dense_checker as dc
import exact_ref as er

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 4097), (4097, 1), (3, 5000), (5000, 3), (100, 80), (1000, 800), (2048, 2048), (8191, 1025)]
FORCED_ROW = (1, 2)            # lcg_hip_dense_set_kernel: k_dn_row, k_dn_row_split
FORCED_ATA = (4, 5, 6)         # two passes, one pass, one workgroup


@pytest.fixture(scope="module")
def api():
    import torch
    from liblcg_amd import api as a
    assert torch.cuda.is_available()
    return a


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _product(api, D, x, out_len, layout=0, conj=0, ata=False):
    import torch
    xd = _dev(x)
    y = torch.full((out_len,), float("nan"), dtype=xd.dtype, device="cuda")
    if ata:
        D.ata(xd, y)
    else:
        D.matvec(xd, y, layout, conj)
    api.synchronize()
    return y.cpu().numpy()


def _full(rng, shape, cplx=False):
    v = rng.standard_normal(shape) * np.exp2(rng.integers(-6, 7, shape))
    if cplx:
        v = v + 1j * rng.standard_normal(shape) * np.exp2(rng.integers(-6, 7, shape))
    return v


def _forms(cplx):
    return [(0, 0), (1, 0), (0, 1), (1, 1)] if cplx else [(0, 0), (1, 0)]


def _op(K, layout, conj):
    A = K.conj() if conj else K
    return A.T if layout else A


def _can_split(m, n, cplx):
    """lcg_hip_dense_set_kernel(K, 2) is refused where the columns cannot be cut: rows of fewer than 32 packs (16 bytes each:
    two fp64 entries or one c128 entry), or M >= 8192 (every row already has a wavefront of its own and the chip is full)."""
    return (n if cplx else (n + 1) // 2) >= 32 and m < 8192


def _ata_bits(m, n):
    p = (52 - math.ceil(math.log2(m * n))) // 3
    assert p >= 1
    return p


def test_exact_sums_and_every_path(api):
    """Integer data: the device's y equals the exact sum bit for bit, whatever the summation order.  The union of the kernels
    the automatic runs took and the forced runs must be the library's whole list: a path no shape reaches fails here."""
    seen = set()
    for (m, n, pad) in [(m, n, 0) for (m, n) in SHAPES] + [(37, 29, 11)]:       # the last one: ld > N
        for cplx in (False, True):
            rng = np.random.default_rng(m * 7919 + n + cplx)
            p = er.int_bits(max(m, n), "c128" if cplx else "f64")
            K = er.int_values(rng, (m, n), p, cplx)
            if pad:
                wide = np.full((m, n + pad), 7.0, K.dtype); wide[:, :n] = K
                D = api.DenseMatrix.from_array(wide[:, :n])
            else:
                D = api.DenseMatrix.from_array(K)
            assert (D.m, D.n) == (m, n)
            for variant in (0,) + FORCED_ROW:
                if variant == 2 and not _can_split(m, n, cplx):
                    assert api.L.load().lcg_hip_dense_set_kernel(D.h, variant) == -2003       # refused: nothing to split
                    continue
                D.set_kernel(variant)
                for layout, conj in _forms(cplx):
                    if variant and layout:
                        continue
                    x = er.int_values(rng, m if layout else n, p, cplx)
                    A = _op(K, layout, conj)
                    y = _product(api, D, x, A.shape[0], layout, conj)
                    er.assert_exact(y, er.exact_int_product(*dc.dense_as_csr(A), x), (m, n, cplx, layout, conj, variant))
                    seen.add(D.last_kernel)
                    if variant:
                        assert D.last_kernel == api.DenseMatrix.kernel_names()[variant - 1]
            D.destroy()
        # K^T.K.x: both stages exact integers
        p = _ata_bits(m, n)
        rng = np.random.default_rng(m * 31 + n)
        K = er.int_values(rng, (m, n), p); x = er.int_values(rng, n, p)
        want = (K.astype(np.int64).T @ (K.astype(np.int64) @ x.astype(np.int64))).astype(np.float64)
        D = api.DenseMatrix.from_rows([K[i] for i in range(m)])
        for variant in (0,) + FORCED_ATA:
            if variant in (5, 6) and n > 2048:
                assert api.L.load().lcg_hip_dense_set_kernel(D.h, variant) == -2003       # refused, and says why
                continue
            D.set_kernel(variant)
            y = _product(api, D, x, n, ata=True)
            er.assert_exact(y, want, (m, n, "ata", variant))
            seen.add(D.last_kernel)
            if variant:
                assert D.last_kernel == api.DenseMatrix.kernel_names()[variant - 1]
        D.destroy()
    assert seen == set(api.DenseMatrix.kernel_names()), (sorted(seen), api.DenseMatrix.kernel_names())


@pytest.mark.parametrize("shape", SHAPES + [(37, 29)])
def test_full_mantissa_rows_within_the_rounding_bound(api, shape):
    m, n = shape
    for cplx in (False, True):
        rng = np.random.default_rng(m * 131 + n + cplx)
        K = _full(rng, (m, n), cplx)
        D = api.DenseMatrix.from_array(_dev(K))              # device-sourced
        for variant in (0,) + FORCED_ROW:
            if variant == 2 and not _can_split(m, n, cplx):
                continue
            D.set_kernel(variant)
            for layout, conj in _forms(cplx):
                if variant and layout:
                    continue
                x = _full(rng, m if layout else n, cplx)
                A = np.ascontiguousarray(_op(K, layout, conj))
                y = _product(api, D, x, A.shape[0], layout, conj)
                er.assert_rows(y, *dc.dense_as_csr(A), x, tag=(shape, cplx, layout, conj, variant))
        D.destroy()
    # K^T.K.x: the second stage against the device's own first stage (each stage is one product under the bound)
    rng = np.random.default_rng(m + n)
    K = _full(rng, (m, n)); x = _full(rng, n)
    D = api.DenseMatrix.from_array(K)
    t = _product(api, D, x, m)
    er.assert_rows(t, *dc.dense_as_csr(K), x, tag=(shape, "t"))
    for variant in (0,) + FORCED_ATA:
        if variant in (5, 6) and n > 2048:
            continue
        D.set_kernel(variant)
        y = _product(api, D, x, n, ata=True)
        # y_j = sum_i K(i,j) t_i with t_i within its bound of the exact K.x: the error of t passes through |K^T| |dt|
        KT = np.ascontiguousarray(K.T)
        ref = er.hp_product(*dc.dense_as_csr(KT), t)
        err = er.row_errors(y, ref)
        dt = er.bound_f64(np.full(m, n), er.hp_product(*dc.dense_as_csr(K), x)[2])
        bound = er.bound_f64(np.full(n, m), ref[2]) + 2.0 * (np.abs(KT) @ dt)
        assert np.all(err <= bound), (shape, variant, float(np.max(err / bound)))
    D.destroy()


def test_same_bits_from_call_to_call_and_from_either_source(api):
    for (m, n) in [(1000, 800), (3, 5000), (2048, 2048), (8191, 1025)]:
        for cplx in (False, True):
            rng = np.random.default_rng(m + 3 * n + cplx)
            K = _full(rng, (m, n), cplx)
            Dh = api.DenseMatrix.from_array(K); Dd = api.DenseMatrix.from_array(_dev(K))
            Dr = api.DenseMatrix.from_rows([K[i] for i in range(m)], is_complex=cplx)
            for layout, conj in _forms(cplx):
                x = _full(rng, m if layout else n, cplx)
                first = _product(api, Dh, x, n if layout else m, layout, conj)
                for D in (Dh, Dh, Dh, Dh, Dd, Dr):
                    again = _product(api, D, x, n if layout else m, layout, conj)
                    assert np.array_equal(first.view(np.float64), again.view(np.float64)), (m, n, cplx, layout, conj)
                if layout:
                    continue
                for variant in FORCED_ROW:              # the forced row forms: five calls each, and from either source
                    if variant == 2 and not _can_split(m, n, cplx):
                        continue
                    for D in (Dh, Dd):
                        D.set_kernel(variant)
                    first = _product(api, Dh, x, m, 0, conj)
                    for D in (Dh, Dh, Dh, Dh, Dd):
                        again = _product(api, D, x, m, 0, conj)
                        assert np.array_equal(first.view(np.float64), again.view(np.float64)), (m, n, cplx, conj, variant)
                for D in (Dh, Dd):
                    D.set_kernel(0)
            if not cplx:
                x = _full(rng, n)
                for variant in (0,) + FORCED_ATA:
                    if variant in (5, 6) and n > 2048:
                        continue
                    for D in (Dh, Dd):
                        D.set_kernel(variant)
                    first = _product(api, Dh, x, n, ata=True)
                    for D in (Dh, Dh, Dh, Dh, Dd):
                        assert np.array_equal(first, _product(api, D, x, n, ata=True)), (m, n, "ata", variant)
            for D in (Dh, Dd, Dr):
                D.destroy()


def test_handles_of_the_other_kind_and_bad_vectors_are_refused(api):
    import torch
    lib = api.L.load()
    E_ARG = -2003
    rp = np.arange(5, dtype=np.int32); ci = np.arange(4, dtype=np.int32)
    A = api.CsrMatrix.from_csr(rp, ci, np.ones(4))
    D = api.DenseMatrix.from_array(np.eye(4))
    Dc = api.DenseMatrix.from_array(np.eye(4) + 0j)
    x = torch.ones(8, dtype=torch.float64, device="cuda"); y = torch.full((8,), 5.0, dtype=torch.float64, device="cuda")
    assert lib.lcg_hip_dense_matvec(A.h, x.data_ptr(), y.data_ptr(), 0) == E_ARG
    assert lib.lcg_hip_dense_ata(A.h, x.data_ptr(), y.data_ptr()) == E_ARG
    assert lib.lcg_hip_dense_build_jacobi(A.h, 0, None) == E_ARG
    assert lib.lcg_hip_dense_destroy(A.h) == E_ARG
    assert lib.lcg_hip_spmv(D.h, x.data_ptr(), y.data_ptr()) == E_ARG and b"dense" in lib.lcg_hip_last_error()
    assert lib.lcg_hip_spmv_op(D.h, x.data_ptr(), y.data_ptr(), 1, 0) == E_ARG
    assert lib.lcg_hip_csr_build_ic0(D.h) == E_ARG and lib.lcg_hip_csr_build_ilu0(D.h) == E_ARG
    assert lib.lcg_hip_csr_destroy(D.h) == E_ARG
    # every exported entry that takes a CSR handle refuses the dense one before it reads anything else of it: the list is
    # taken from the prototypes (a handle or a callback's instance as first argument, every name that is not a dense entry)
    from liblcg_amd import _lib
    not_handles = {"lcg_hip_set_stream", "lcg_hip_memcpy", "lcg_hip_solver", "lcg_hip_solver_preconditioned", "lcg_hip_solver_constrained",
                   "lcg_hip_lcg", "lcg_hip_lcgs", "clcg_hip_solver", "clcg_hip_solver_preconditioned", "clcg_hip_solver_c64",
                   "clcg_hip_solver_preconditioned_c64", "lcg_hip_set_shadow_vector", "lcg_hip_comm_unique_id", "lcg_hip_p2p_export",
                   "lcg_hip_allreduce_sum", "lcg_hip_gen_xtrue"}
    tried = []
    for name, (res, args) in _lib.SIGNATURES.items():
        if not args or args[0] is not _lib.vp or "dense" in name or name in not_handles:
            continue
        zeros = [0.0 if a is C.c_double else 0 if a in (C.c_int, C.c_int64, C.c_uint64, C.c_uint) else None for a in args[1:]]
        lib.lcg_hip_dense_rows(D.h)                     # (clears nothing; the next line must set the text anew)
        got = getattr(lib, name)(D.h, *zeros)
        want = {C.c_int: E_ARG, C.c_int64: E_ARG, C.c_char_p: b"", _lib.vp: None, None: None}[res]
        assert got == want, (name, got)
        assert name.encode() in lib.lcg_hip_last_error() and b"dense" in lib.lcg_hip_last_error(), (name, lib.lcg_hip_last_error())
        tried.append(name)
    assert len(tried) >= 59 and {"lcg_hip_csr_build_jacobi", "lcg_hip_csr_rows", "lcg_hip_csr_nnz", "lcg_hip_csr_arrays", "lcg_hip_csr_last_kernel",
                                 "lcg_hip_jacobi_mx", "clcg_hip_jacobi_mx", "lcg_hip_spmv_c64", "lcg_hip_csr_distribute"} <= set(tried), tried
    assert all("_csr_" not in n or n in tried or _lib.SIGNATURES[n][1][0] is not _lib.vp for n in _lib.SIGNATURES)
    assert (lib.lcg_hip_dense_rows(D.h), lib.lcg_hip_dense_cols(D.h)) == (4, 4)      # and the dense handle is unharmed
    # value types, x == y, layout
    assert lib.clcg_hip_dense_matvec(D.h, x.data_ptr(), y.data_ptr(), 0, 0) == E_ARG
    assert lib.lcg_hip_dense_matvec(Dc.h, x.data_ptr(), y.data_ptr(), 0) == E_ARG
    assert lib.lcg_hip_dense_matvec(D.h, x.data_ptr(), x.data_ptr(), 0) == E_ARG
    assert lib.lcg_hip_dense_matvec(D.h, x.data_ptr(), y.data_ptr(), 2) == E_ARG
    assert lib.lcg_hip_dense_matvec(D.h, None, y.data_ptr(), 0) == E_ARG
    # a callback with the wrong n records the error and writes nothing; as a solve it ends with LCG_HIP_E_ARG
    lib.lcg_hip_dense_ata_ax(D.h, x.data_ptr(), y.data_ptr(), 5)
    api.synchronize()
    assert b"n_size = 5" in lib.lcg_hip_last_error() and torch.all(y == 5.0)
    m = torch.zeros(5, dtype=torch.float64, device="cuda"); b = torch.ones(5, dtype=torch.float64, device="cuda")
    with pytest.raises(api.LcgHipError):
        api.lcg_solver("lcg_hip_dense_ata_ax", None, m, b, 5, api.lcg_default_parameters(), D, api.LCG_CG)
    with pytest.raises(api.LcgHipError):
        api.lcg_solver("lcg_hip_dense_ata_ax", None, m[:4], b[:4], 4, api.lcg_default_parameters(), A, api.LCG_CG)
    lib.lcg_hip_dense_jacobi_mx(D.h, x.data_ptr(), y.data_ptr(), 4)
    assert b"build_jacobi" in lib.lcg_hip_last_error()
    assert (lib.lcg_hip_dense_rows(D.h), lib.lcg_hip_dense_cols(D.h)) == (4, 4)
    for h in (A, D, Dc):
        h.destroy()


def test_build_jacobi_against_the_checker(api):
    import torch
    lib = api.L.load()
    rng = np.random.default_rng(11)
    for (m, n) in [(100, 80), (1000, 800), (5000, 3), (3, 5000)]:
        K = _full(rng, (m, n))
        D = api.DenseMatrix.from_array(K)
        d = torch.empty(n, dtype=torch.float64, device="cuda")
        D.build_jacobi(True, d)
        dh = d.cpu().numpy()
        # the column sums of squares: within gamma(M + 1) of the exact sum (M rounded squares, any order)
        L = np.longdouble
        exact = np.sum(K.astype(L) ** 2, axis=0)
        assert np.all(np.abs((dh.astype(L) - exact).astype(np.float64)) <= er.gamma(m + 1) * exact.astype(np.float64)), (m, n)
        np.testing.assert_allclose(dh, dc.normal_diagonal(K), rtol=float(2 * er.gamma(m + 1)))
        x = _full(rng, n)
        z = torch.empty(n, dtype=torch.float64, device="cuda")
        lib.lcg_hip_dense_jacobi_mx(D.h, _dev(x).data_ptr(), z.data_ptr(), n); api.synchronize()
        assert np.array_equal(z.cpu().numpy(), x * (1.0 / dh)), (m, n)         # the reciprocal is one division
        D.destroy()
    for cplx in (False, True):
        K = _full(rng, (300, 300), cplx)
        D = api.DenseMatrix.from_array(K)
        d = torch.empty(300, dtype=torch.complex128 if cplx else torch.float64, device="cuda")
        D.build_jacobi(False, d)
        assert np.array_equal(d.cpu().numpy().view(np.float64), np.diag(K).copy().view(np.float64))
        x = _full(rng, 300, cplx)
        z = torch.empty_like(d)
        if cplx:
            lib.clcg_hip_dense_jacobi_mx(D.h, _dev(x).data_ptr(), z.data_ptr(), 300, 0, 0)
        else:
            lib.lcg_hip_dense_jacobi_mx(D.h, _dev(x).data_ptr(), z.data_ptr(), 300)
        api.synchronize()
        np.testing.assert_allclose(z.cpu().numpy(), x / np.diag(K), rtol=1e-14)
        D.destroy()
    # a zero or non-finite diagonal is named
    K = _full(rng, (6, 6)); K[:, 4] = 0.0
    D = api.DenseMatrix.from_array(K)
    assert lib.lcg_hip_dense_build_jacobi(D.h, 1, None) == -2003 and b"entry 4" in lib.lcg_hip_last_error()
    assert lib.lcg_hip_dense_build_jacobi(D.h, 0, None) == -2003 and b"entry 4" in lib.lcg_hip_last_error()
    D.destroy()
    K = _full(rng, (6, 5))
    D = api.DenseMatrix.from_array(K)
    assert lib.lcg_hip_dense_build_jacobi(D.h, 0, None) == -2003          # not square
    D.destroy()


# ---------------------------------------------------------------------------------------------- solvers through the callbacks
FACTOR, FLOOR = 50.0, 1e-9          # tests/conftest.py: check_converged_run's factor and floor


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _late_band(x_ref, x_alt, xt):
    """check_converged_run's rule 3 for the iterate two iterations short of the earlier stop, relative to |x_ref|: the floor, FACTOR
    x the oracle's own response (here: its serial-order against its pairwise-order product), or a quarter of the error the oracle
    has left there -- two finite-precision runs whose products round differently drift apart by a fraction of the error that is
    left (tests/conftest.py)."""
    return max(FLOOR, FACTOR * _rel(x_alt, x_ref), 0.25 * _rel(xt, x_ref))


def _close_to_the_solution(x, x_ref, xt, wide, tag):
    """check_converged_run's rule 2: the converged iterate is as close to the solution b was made from as the oracle's, within a
    factor (10; the loops whose counts wander: 100)."""
    e_gpu, e_ref = np.linalg.norm(x - xt), np.linalg.norm(x_ref - xt)
    assert e_gpu <= (100.0 if wide else 10.0) * max(e_ref, 1e-14 * np.linalg.norm(xt)), (tag, "distance to the solution", e_gpu, e_ref)


class _RealOracle:
    """The oracle's own loops (oracle/lcg_oracle.h:84-97) with a Python product: the checker's serial order, or numpy's."""
    NAMES = ["orc_lcg", "orc_lpcg", "orc_lcgs", "orc_lbicgstab", "orc_lbicgstab2", "orc_lpg", "orc_lspg"]

    def __init__(self, K, low, hig):
        from oracle import pyoracle as po
        self.po, self.lib, self.K, self.low, self.hig = po, po.Oracle("port").lib, K, low, hig
        self.inv = 1.0 / dc.normal_diagonal(K)
        self.AX = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int)
        self.PF = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_int)

    def run(self, sid, b, cap, eps, serial=True):
        n = self.K.shape[1]
        K = self.K

        def ax(_, xp, yp, nn):
            x = np.ctypeslib.as_array(xp, (nn,)); y = np.ctypeslib.as_array(yp, (nn,))
            y[:] = dc.ata(K, x) if serial else K.T @ (K @ x)

        def mx(_, xp, yp, nn):
            np.ctypeslib.as_array(yp, (nn,))[:] = np.ctypeslib.as_array(xp, (nn,)) * self.inv

        last = [0]

        def pf(_, mp, conv, par, nn, k):
            last[0] = k
            return 0

        a, mf, p = self.AX(ax), self.AX(mx), self.PF(pf)
        para = self.po.default_para(epsilon=eps, abs_diff=0, max_iterations=cap)
        m = np.zeros(n); b = np.ascontiguousarray(b)
        f = getattr(self.lib, self.NAMES[sid]); f.restype = C.c_int
        vp = lambda v: v.ctypes.data_as(C.c_void_p)
        if sid == 1:
            ret = f(a, mf, p, vp(m), vp(b), n, C.byref(para), None)
        elif sid >= 5:
            ret = f(a, p, vp(m), vp(b), vp(self.low), vp(self.hig), n, C.byref(para), None)
        else:
            ret = f(a, p, vp(m), vp(b), n, C.byref(para), None)
        return dict(x=m, ret=ret, iters=last[0])


def _gpu_real(api, D, sid, b, n, cap, eps, low, hig, device):
    import torch
    para = api.lcg_default_parameters(epsilon=eps, abs_diff=0, max_iterations=cap)
    if device:
        m = torch.zeros(n, dtype=torch.float64, device="cuda"); bb = _dev(b); lo, hi = _dev(low), _dev(hig)
    else:
        m = np.zeros(n); bb = np.ascontiguousarray(b); lo, hi = low, hig
    if sid == api.LCG_PCG:
        info = api.lcg_solver_preconditioned("lcg_hip_dense_ata_ax", "lcg_hip_dense_jacobi_mx", None, m, bb, n, para, D)
    elif sid >= api.LCG_PG:
        info = api.lcg_solver_constrained("lcg_hip_dense_ata_ax", None, m, bb, lo, hi, n, para, D, sid)
    else:
        info = api.lcg_solver("lcg_hip_dense_ata_ax", None, m, bb, n, para, D, sid)
    x = m.cpu().numpy() if device else m
    return info, x


def test_real_solvers_through_the_normal_equations_callback(api, capsys):
    """sample1.cpp's system at 1000 x 800 with a seeded generator: all seven solvers on lcg_hip_dense_ata_ax (PCG with the
    column-square Jacobi, PG / SPG in the box 1 <= m <= 2) against the oracle's loops fed the checker's product.  Capped runs
    (5, 20) compare iterates within max(FLOOR, FACTOR x the oracle's own spread between the serial-order and the pairwise-order
    product).  Converged runs follow tests/conftest.py: check_converged_run with that spread as the oracle's response: the return
    code, the count band, the reported residual, the distance to the solution, and the iterate two iterations short of the
    earlier stop (_late_band).  A solver whose oracle run does not converge within the cap is compared capped only.
    Measured on the MI355X: the late CG iterate moved from 3.7e-9 to 2.6e-8 of |x| between two fold orders of the products
    (both runs 1e-6 from the solution, the oracle's own spread 2.7e-10), which is what the rule's third term is for; the worst
    ratio of a difference to its band is printed and recorded in DESIGN.md section 14."""
    rng = np.random.default_rng(2024)
    M, N = 1000, 800
    K = rng.uniform(-1.0, 1.0, (M, N)); xt = rng.uniform(1.0, 2.0, N)
    b = dc.ata(K, xt)
    low, hig = np.full(N, 1.0), np.full(N, 2.0)
    orc = _RealOracle(K, low, hig)
    D = api.DenseMatrix.from_array(K)
    D.build_jacobi(True)
    eps, worst, capped_only = 1e-10, 0.0, []
    for sid in range(7):
        wide = sid in (api.LCG_CGS, api.LCG_BICGSTAB, api.LCG_BICGSTAB2)
        for cap in (5, 20):
            ref, alt = orc.run(sid, b, cap, eps), orc.run(sid, b, cap, eps, serial=False)
            band = max(FLOOR, FACTOR * _rel(alt["x"], ref["x"]))
            for device in ((True, False) if sid in (api.LCG_CG, api.LCG_PG) else (True,)):
                info, x = _gpu_real(api, D, sid, b, N, cap, eps, low, hig, device)
                r = _rel(x, ref["x"]); worst = max(worst, r / band)
                print(f"solver {sid} cap {cap} device {device}: rel diff {r:.2e} band {band:.2e}")
                assert r <= band, (sid, cap, device, r, band)
        ref, alt = orc.run(sid, b, 600, eps), orc.run(sid, b, 600, eps, serial=False)
        if ref["ret"] != 0 or alt["ret"] != 0:
            capped_only.append(sid)
            continue
        info, x = _gpu_real(api, D, sid, b, N, 600, eps, low, hig, True)
        assert info.ret == ref["ret"] == 0, (sid, info.ret)
        dit = abs(ref["iters"] - alt["iters"])
        cnt = max(3, 4 * dit, 0.3 * ref["iters"]) if wide else max(3, 3 * dit, 0.05 * ref["iters"])
        assert abs(info.iterations - ref["iters"]) <= cnt, (sid, info.iterations, ref["iters"], dit)
        assert info.residual <= eps
        _close_to_the_solution(x, ref["x"], xt, wide, sid)
        Kc = min(info.iterations, ref["iters"], alt["iters"]) - 2
        if Kc >= 1:
            rK, aK = orc.run(sid, b, Kc, eps), orc.run(sid, b, Kc, eps, serial=False)
            band = _late_band(rK["x"], aK["x"], xt)
            iK, xK = _gpu_real(api, D, sid, b, N, Kc, eps, low, hig, True)
            # both capped runs stopped at the cap, at the same count: an iterate of another count is not compared
            assert iK.ret == rK["ret"] == aK["ret"] == -1019 and iK.iterations == rK["iters"] == aK["iters"] == Kc, \
                (sid, Kc, iK.ret, rK["ret"], iK.iterations, rK["iters"], aK["iters"])
            r = _rel(xK, rK["x"]); worst = max(worst, r / band)
            print(f"solver {sid} converged in {info.iterations} (oracle {ref['iters']} / {alt['iters']}); at {Kc}: rel diff {r:.2e} band {band:.2e}")
            assert r <= band, (sid, Kc, r, band)
    print(f"worst ratio to the band: {worst:.3g}; compared capped only (the oracle does not converge in 600): {capped_only}")
    D.destroy()


def test_complex_solvers_through_the_dense_callback(api):
    """sample3.cpp's system at 300 x 300: a seeded dense complex symmetric K; BiCG (asks for K^H.x), BiCG-sym, CGS, BiCGStab and
    TFQMR on clcg_hip_dense_ax against the oracle's loops fed the checker's product, with the rules of the real test."""
    from oracle import pyoracle as po
    lib = po.Oracle("port").lib
    rng = np.random.default_rng(77)
    n = 300
    G = rng.uniform(-1, 1, (n, n)) + 1j * rng.uniform(-1, 1, (n, n))
    K = (G + G.T) / 2 + np.diag(np.full(n, 40.0 + 20.0j))
    xt = rng.uniform(1, 2, n) + 1j * rng.uniform(1, 2, n)
    b = dc.cmatvec(K, xt)
    rbar0 = rng.uniform(1, 2, n) + 1j * rng.uniform(1, 2, n)
    AX = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int)
    PF = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_int)
    names = {api.CLCG_BICG: "orc_clbicg", api.CLCG_BICG_SYM: "orc_clbicg_symmetric", api.CLCG_CGS: "orc_clcgs",
             api.CLCG_BICGSTAB: "orc_clbicgstab", api.CLCG_TFQMR: "orc_cltfqmr"}
    forms_asked = set()

    def oracle(sid, cap, eps, serial=True):
        def ax(_, xp, yp, nn, layout, conj):
            forms_asked.add((sid, layout, conj))
            x = np.ctypeslib.as_array(xp, (2 * nn,)).view(np.complex128); y = np.ctypeslib.as_array(yp, (2 * nn,)).view(np.complex128)
            y[:] = dc.cmatvec(K, x, layout, conj) if serial else _op(K, layout, conj) @ x
        last = [0]

        def pf(_, mp, conv, par, nn, k):
            last[0] = k
            return 0
        a, p = AX(ax), PF(pf)
        para = po.default_cpara(epsilon=eps, abs_diff=0, max_iterations=cap)
        m = np.zeros(n, np.complex128)
        f = getattr(lib, names[sid]); f.restype = C.c_int
        vp = lambda v: v.ctypes.data_as(C.c_void_p)
        args = [a, p, vp(m), vp(b), n, C.byref(para), None]
        if sid in (api.CLCG_CGS, api.CLCG_BICGSTAB, api.CLCG_TFQMR):
            args.append(vp(rbar0))
        return dict(x=m, ret=f(*args), iters=last[0])

    D = api.DenseMatrix.from_array(K)

    def gpu(sid, cap, eps, device=True):
        import torch
        para = api.clcg_default_parameters(epsilon=eps, abs_diff=0, max_iterations=cap)
        m = torch.zeros(n, dtype=torch.complex128, device="cuda") if device else np.zeros(n, np.complex128)
        info = api.clcg_solver("clcg_hip_dense_ax", None, m, _dev(b) if device else b, n, para, D, sid, shadow=rbar0)
        return info, (m.cpu().numpy() if device else m)

    eps, worst, capped_only = 1e-20, 0.0, []
    for sid in names:
        for cap in (5, 20):
            ref, alt = oracle(sid, cap, eps), oracle(sid, cap, eps, serial=False)
            band = max(FLOOR, FACTOR * _rel(alt["x"], ref["x"]))
            for device in ((True, False) if sid == api.CLCG_BICG else (True,)):
                _, x = gpu(sid, cap, eps, device)
                r = _rel(x, ref["x"]); worst = max(worst, r / band)
                print(f"complex solver {sid} cap {cap} device {device}: rel diff {r:.2e} band {band:.2e}")
                assert r <= band, (sid, cap, device, r, band)
        ref, alt = oracle(sid, 300, eps), oracle(sid, 300, eps, serial=False)
        if ref["ret"] != 0 or alt["ret"] != 0:
            capped_only.append(sid)
            continue
        info, x = gpu(sid, 300, eps)
        assert info.ret == 0, (sid, info.ret)
        dit = abs(ref["iters"] - alt["iters"])
        assert abs(info.iterations - ref["iters"]) <= max(3, 4 * dit, 0.3 * ref["iters"]), (sid, info.iterations, ref["iters"])
        _close_to_the_solution(x, ref["x"], xt, True, sid)
        Kc = min(info.iterations, ref["iters"], alt["iters"]) - 2
        if Kc >= 1:
            rK, aK = oracle(sid, Kc, eps), oracle(sid, Kc, eps, serial=False)
            band = _late_band(rK["x"], aK["x"], xt)
            iK, xK = gpu(sid, Kc, eps)
            # (the complex loops' code at the cap: -1019 here as in the reference, oracle/lcg_oracle.h's ORC_C_ value in the oracle)
            assert iK.ret == -1019 and rK["ret"] == aK["ret"] and rK["ret"] in (-1019, -1020), (sid, Kc, iK.ret, rK["ret"], aK["ret"])
            assert iK.iterations == rK["iters"] == aK["iters"] == Kc, (sid, Kc, iK.iterations, rK["iters"], aK["iters"])
            r = _rel(xK, rK["x"]); worst = max(worst, r / band)
            print(f"complex solver {sid} converged in {info.iterations} (oracle {ref['iters']}); at {Kc}: rel diff {r:.2e} band {band:.2e}")
            assert r <= band, (sid, Kc, r, band)
    assert (api.CLCG_BICG, 1, 1) in forms_asked            # clbicg asks for the conjugate transpose (clcg.cpp:187)
    print(f"worst ratio to the band: {worst:.3g}; compared capped only (the oracle does not converge in 300): {capped_only}")
    D.destroy()
