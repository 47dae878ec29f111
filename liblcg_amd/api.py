"""Thin Python front of the C ABI, shaped like liblcg's entry points.

``lcg_solver`` / ``lcg_solver_preconditioned`` / ``clcg_solver`` take the same arguments, in
the same order and with the same meaning as the reference's functions (lcg.h:71-72, 90-91;
clcg.h:74-76); vectors are torch CUDA tensors (device resident, nothing copied) or numpy arrays
(host in/out, copied by the library like lcg_solver_cuda does).  torch is used for memory only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._lib import CAXFUNC, CPROGRESS, CPROGRESS_C64, AXFUNC, PROGRESS, ClcgPara, LcgPara  # noqa: F401

LCG_CG, LCG_PCG, LCG_CGS, LCG_BICGSTAB, LCG_BICGSTAB2, LCG_PG, LCG_SPG = range(7)
CLCG_BICG, CLCG_BICG_SYM, CLCG_CGS, CLCG_BICGSTAB, CLCG_TFQMR, CLCG_PCG, CLCG_PBICG = range(7)
MEM_HOST, MEM_DEVICE = 0, 1
GEN_SCRAMBLED, GEN_DIAGONALS, GEN_ROW_RANDOM_BAND = 0, 1, 2


class LcgHipError(RuntimeError):
    pass


def _chk(rc: int, what: str):
    if rc <= -2000:
        raise LcgHipError(f"{what}: rc={rc}: {L.load().lcg_hip_last_error().decode()}")
    return rc


def lcg_default_parameters(**kw) -> LcgPara:
    p = L.load().lcg_hip_default_parameters()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def clcg_default_parameters(**kw) -> ClcgPara:
    p = L.load().clcg_hip_default_parameters()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(x):
    """(address, mem) of a torch CUDA tensor or a numpy array."""
    if isinstance(x, np.ndarray):
        return x.ctypes.data, MEM_HOST
    import torch
    if isinstance(x, torch.Tensor):
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return x.data_ptr(), (MEM_DEVICE if x.is_cuda else MEM_HOST)
    raise TypeError(type(x))


def use_torch_stream():
    """Run the library on torch's current stream (so torch ops and ours are ordered)."""
    import torch
    _chk(L.load().lcg_hip_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream)), "set_stream")


def use_own_stream():
    """Back to the library's own stream (lcg_hip_set_stream(NULL)); it waits for what was enqueued on the previous one."""
    _chk(L.load().lcg_hip_set_stream(None), "set_stream")


class CsrMatrix:
    """An HBM-resident CSR matrix (handle ``lcg_hip_csr_t``)."""
    is_c64 = False      # values are complex64 (from_csr_c64)

    def __init__(self, handle: int, n_rows: int, is_complex: bool, keep=()):
        self.h = C.c_void_p(handle)
        self.n = n_rows
        self.is_complex = is_complex
        self._keep = keep

    # -- construction ---------------------------------------------------------------------
    @classmethod
    def from_csr(cls, rowptr, col, val, n_cols=None, adopt=False):
        lib = L.load()
        is_c = bool(np.iscomplexobj(val)) if isinstance(val, np.ndarray) else val.is_complex()
        if isinstance(val, np.ndarray):
            rowptr = np.ascontiguousarray(rowptr, np.int32); col = np.ascontiguousarray(col, np.int32)
            val = np.ascontiguousarray(val, np.complex128 if is_c else np.float64)
        n = len(rowptr) - 1
        nnz = len(col)
        (pr, mem), (pc, _), (pv, _) = _ptr(rowptr), _ptr(col), _ptr(val)
        h = C.c_void_p()
        _chk(lib.lcg_hip_csr_create(C.byref(h), n, n_cols or n, nnz, pr, pc, pv, int(is_c), mem, int(adopt)), "csr_create")
        return cls(h.value, n, is_c, keep=(rowptr, col, val) if adopt else ())

    @classmethod
    def from_csr_c64(cls, rowptr, col, val, n_cols=None, adopt=False):
        """A complex64 matrix (lcg_hip_csr_create_c64): val is cast to complex64 (numpy) or must be a torch.complex64
        tensor.  Products: spmv_c64 / 'clcg_hip_csr_ax_c64'; solvers: clcg_solver_c64, clcg_solver_preconditioned_c64."""
        lib = L.load()
        if isinstance(val, np.ndarray):
            rowptr = np.ascontiguousarray(rowptr, np.int32); col = np.ascontiguousarray(col, np.int32)
            val = np.ascontiguousarray(val, np.complex64)
        else:
            import torch
            if val.dtype != torch.complex64:
                raise TypeError(f"from_csr_c64 takes complex64 values, not {val.dtype}")
        n = len(rowptr) - 1
        (pr, mem), (pc, _), (pv, _) = _ptr(rowptr), _ptr(col), _ptr(val)
        h = C.c_void_p()
        _chk(lib.lcg_hip_csr_create_c64(C.byref(h), n, n_cols or n, len(col), pr, pc, pv, mem, int(adopt)), "csr_create_c64")
        M = cls(h.value, n, True, keep=(rowptr, col, val) if adopt else ())
        M.is_c64 = True
        return M

    def spmv_c64(self, x, y, layout=0, conjugate=0):
        """y = op(A).x for a complex64 matrix (torch.complex64 CUDA tensors)."""
        return _chk(L.load().lcg_hip_spmv_c64(self.h, _ptr(x)[0], _ptr(y)[0], layout, conjugate), "spmv_c64")

    @classmethod
    def from_coo(cls, n, row, col, val):
        lib = L.load()
        is_c = bool(np.iscomplexobj(val))
        row = np.ascontiguousarray(row, np.int32); col = np.ascontiguousarray(col, np.int32)
        val = np.ascontiguousarray(val, np.complex128 if is_c else np.float64)
        h = C.c_void_p()
        _chk(lib.lcg_hip_csr_from_coo(C.byref(h), n, len(row), row.ctypes.data, col.ctypes.data, val.ctypes.data,
                                      int(is_c), MEM_HOST), "csr_from_coo")
        return cls(h.value, n, is_c)

    @classmethod
    def generate(cls, n, npairs=16, band=0, symmetric=True, seed=1, diag_shift=0.01, r0=0, r1=None, pattern=None):
        """pattern: GEN_SCRAMBLED, GEN_DIAGONALS (offsets <= band, the same in every row), GEN_ROW_RANDOM_BAND
        (columns within +-band drawn per row); None = DIAGONALS when band > 0 else SCRAMBLED."""
        lib = L.load()
        r1 = n if r1 is None else r1
        if pattern is None:
            pattern = GEN_DIAGONALS if band > 0 else GEN_SCRAMBLED
        h = C.c_void_p()
        _chk(lib.lcg_hip_csr_generate_ex(C.byref(h), n, npairs, pattern, band, int(symmetric), seed, diag_shift, r0, r1), "csr_generate")
        return cls(h.value, r1 - r0, False)

    @classmethod
    def laplace2d(cls, nx, ny, r0=0, r1=None):
        lib = L.load()
        r1 = nx * ny if r1 is None else r1
        h = C.c_void_p()
        _chk(lib.lcg_hip_csr_laplace2d(C.byref(h), nx, ny, r0, r1), "csr_laplace2d")
        return cls(h.value, r1 - r0, False)

    # -- queries ---------------------------------------------------------------------------
    @property
    def nnz(self) -> int:
        return L.load().lcg_hip_csr_nnz(self.h)

    def arrays_to_host(self):
        """(rowptr, col, val) copied to numpy (tests / CPU baseline)."""
        lib = L.load()
        pr, pc, pv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _chk(lib.lcg_hip_csr_arrays(self.h, C.byref(pr), C.byref(pc), C.byref(pv)), "csr_arrays")
        nnz = self.nnz
        rowptr = np.empty(self.n + 1, np.int32); col = np.empty(nnz, np.int32)
        val = np.empty(nnz, np.complex128 if self.is_complex else np.float64)
        for dst, src in ((rowptr, pr), (col, pc), (val, pv)):
            _chk(lib.lcg_hip_memcpy(dst.ctypes.data, src, dst.nbytes, 2), "memcpy d2h")
        return rowptr, col, val

    def set_kernel(self, variant: int):
        _chk(L.load().lcg_hip_csr_set_kernel(self.h, variant), "set_kernel")

    def set_sym_runs(self, mode: int, slices: int = 0):
        """Symmetric run stretches (lcg_hip_csr_set_sym_runs): mode -1 automatic, 0 off, 1 forced; slices 0 (the default: one), 1, 2, 4 or 8."""
        _chk(L.load().lcg_hip_csr_set_sym_slices(self.h, slices), "set_sym_slices")
        _chk(L.load().lcg_hip_csr_set_sym_runs(self.h, mode), "set_sym_runs")

    def sym_runs(self):
        """(slices in use or 0, blocks the symmetric kernel multiplies, status text) of the latest plan (lcg_hip_csr_sym_runs)."""
        blocks, why = C.c_int64(0), C.c_char_p()
        nx = L.load().lcg_hip_csr_sym_runs(self.h, C.byref(blocks), C.byref(why))
        return int(nx), blocks.value, (why.value or b"").decode()

    def build_jacobi(self, diag_out=None):
        p = None if diag_out is None else _ptr(diag_out)[0]
        _chk(L.load().lcg_hip_csr_build_jacobi(self.h, p), "build_jacobi")

    # -- IC(0) preconditioner (csr_ic0.hip) -------------------------------------------------
    def build_ic0(self):
        """Factor A ~ L.L^T with zero fill on the device; pass "lcg_hip_ic0_mx" / "clcg_hip_ic0_mx" (a complex64 matrix:
        "clcg_hip_ic0_mx_c64", factored in fp32) as Mfp afterwards.  The factor is applied exactly, level by level, until
        ic0_set_sweeps(k) asks for k Jacobi sweeps per triangle; every build resets that to 0."""
        if self.is_c64:
            _chk(L.load().lcg_hip_csr_build_ic0_c64(self.h), "build_ic0_c64")
        else:
            _chk(L.load().lcg_hip_csr_build_ic0(self.h), "build_ic0")

    def ic0_info(self) -> dict:
        ll, lu, la, zp = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        ms, nb = C.c_double(), C.c_int64()
        _chk(L.load().lcg_hip_csr_ic0_info(self.h, C.byref(ll), C.byref(lu), C.byref(la), C.byref(zp), C.byref(ms), C.byref(nb)),
             "ic0_info")
        sw = C.c_int(0)
        if L.load().lcg_hip_csr_ic0_get_sweeps(self.h, C.byref(sw)) != 0:      # (a failed factor has no setting)
            sw.value = 0
        return {"levels_lower": ll.value, "levels_upper": lu.value, "launches_per_apply": la.value,
                "zero_pivot": zp.value, "build_ms": ms.value, "bytes": nb.value, "sweeps": sw.value}

    def ic0_set_sweeps(self, k):
        """k >= 1: apply the factor by k Jacobi sweeps per triangle (one launch each over all rows, 2k per apply) instead of the
        exact level-scheduled solves; 0: exact again.  Holds for ic0_solve and the ic0_mx callbacks until the next build_ic0."""
        _chk(L.load().lcg_hip_csr_ic0_set_sweeps(self.h, int(k)), "ic0_set_sweeps")

    def ic0_factor_to_host(self):
        """(rowptr, col, val) of L copied to numpy: natural row order, rows sorted, the diagonal last (complex64 values for
        a complex64 matrix)."""
        lib = L.load()
        pr, pc, pv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _chk(lib.lcg_hip_csr_ic0_factor(self.h, C.byref(pr), C.byref(pc), C.byref(pv)), "ic0_factor")
        rowptr = np.empty(self.n + 1, np.int32)
        _chk(lib.lcg_hip_memcpy(rowptr.ctypes.data, pr, rowptr.nbytes, 2), "memcpy d2h")
        nnz = int(rowptr[-1])
        col = np.empty(nnz, np.int32)
        val = np.empty(nnz, np.complex64 if self.is_c64 else np.complex128 if self.is_complex else np.float64)
        for dst, src in ((col, pc), (val, pv)):
            _chk(lib.lcg_hip_memcpy(dst.ctypes.data, src, dst.nbytes, 2), "memcpy d2h")
        return rowptr, col, val

    def ic0_solve(self, x, y, which=2):
        """y = L^-1 x (which 0), L^-T x (1) or (L.L^T)^-1 x (2); device tensors, on the library's stream."""
        if self.is_c64:
            _chk(L.load().lcg_hip_ic0_solve_c64(self.h, which, _ptr(x)[0], _ptr(y)[0]), "ic0_solve_c64")
        else:
            _chk(L.load().lcg_hip_ic0_solve(self.h, which, _ptr(x)[0], _ptr(y)[0]), "ic0_solve")

    def ic0_solve_multi(self, X, Y, which=2):
        """ic0_solve for the k = 2, 4 or 8 columns of X at once (lcg_hip_ic0_solve_multi): X, Y (n, k) C-contiguous float64 CUDA
        tensors, 16-byte aligned.  Column j has the bits of ic0_solve on column j; the factor is read once for all of them."""
        k = _block_k(X, Y)
        _chk(L.load().lcg_hip_ic0_solve_multi(self.h, k, which, _ptr(X)[0], _ptr(Y)[0]), "ic0_solve_multi")

    def ic0_solve_multi_c64(self, X, Y, which=2):
        """ic0_solve of a complex64 matrix for the k = 2, 4 or 8 columns of X at once (clcg_hip_ic0_solve_multi_c64): X, Y (n, k)
        C-contiguous complex64 CUDA tensors, 16-byte aligned.  Column j has the bits of ic0_solve on column j; the fp32 factor
        is read once for all of them."""
        k = _block_k(X, Y, cplx="c64")
        _chk(L.load().clcg_hip_ic0_solve_multi_c64(self.h, k, which, _ptr(X)[0], _ptr(Y)[0]), "ic0_solve_multi_c64")

    # -- ILU(0) preconditioner (csr_ilu0.hip) -----------------------------------------------
    def build_ilu0(self):
        """Factor A ~ L.U (unit lower L) with zero fill on the device, fp64 and complex128 matrices; pass "lcg_hip_ilu0_mx" /
        "clcg_hip_ilu0_mx" as Mfp afterwards, or "lcg_hip_csr_ax_ilu0" / "clcg_hip_csr_ax_ilu0" as Afp of a loop without an
        Mfp (right preconditioning: solve for u from u = 0, then ilu0_solve(u, x)).  Applied exactly, level by level, until
        ilu0_set_sweeps(k); every build resets that to 0.  Lives beside an IC(0) factor on the same matrix."""
        _chk(L.load().lcg_hip_csr_build_ilu0(self.h), "build_ilu0")

    def ilu0_info(self) -> dict:
        ll, lu, la, zp = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        ms, nb = C.c_double(), C.c_int64()
        _chk(L.load().lcg_hip_csr_ilu0_info(self.h, C.byref(ll), C.byref(lu), C.byref(la), C.byref(zp), C.byref(ms), C.byref(nb)),
             "ilu0_info")
        sw = C.c_int(0)
        if L.load().lcg_hip_csr_ilu0_get_sweeps(self.h, C.byref(sw)) != 0:     # (a failed factor has no setting)
            sw.value = 0
        return {"levels_L": ll.value, "levels_U": lu.value, "launches_per_apply": la.value,
                "zero_pivot": zp.value, "build_ms": ms.value, "bytes": nb.value, "sweeps": sw.value}

    def ilu0_set_sweeps(self, k):
        """k >= 1: apply the factor by k Jacobi sweeps per triangle (L: k - 1 launches, one when k = 1; U: k) instead of the
        exact level-scheduled solves; 0: exact again.  Holds for ilu0_solve and the four callbacks until the next build_ilu0."""
        _chk(L.load().lcg_hip_csr_ilu0_set_sweeps(self.h, int(k)), "ilu0_set_sweeps")

    def ilu0_factor_to_host(self, which):
        """(rowptr, col, val) of L (which 0: rows sorted, unit diagonal not stored) or U (1: rows sorted, diagonal first)
        copied to numpy."""
        lib = L.load()
        pr, pc, pv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _chk(lib.lcg_hip_csr_ilu0_factor(self.h, int(which), C.byref(pr), C.byref(pc), C.byref(pv)), "ilu0_factor")
        rowptr = np.empty(self.n + 1, np.int32)
        _chk(lib.lcg_hip_memcpy(rowptr.ctypes.data, pr, rowptr.nbytes, 2), "memcpy d2h")
        nnz = int(rowptr[-1])
        col = np.empty(nnz, np.int32)
        val = np.empty(nnz, np.complex128 if self.is_complex else np.float64)
        for dst, src in ((col, pc), (val, pv)):
            if nnz:
                _chk(lib.lcg_hip_memcpy(dst.ctypes.data, src, dst.nbytes, 2), "memcpy d2h")
        return rowptr, col, val

    def ilu0_solve(self, x, y, which=2):
        """y = L^-1 x (which 0), U^-1 x (1) or U^-1 L^-1 x (2); device tensors, on the library's stream."""
        _chk(L.load().lcg_hip_ilu0_solve(self.h, which, _ptr(x)[0], _ptr(y)[0]), "ilu0_solve")

    def ilu0_solve_multi(self, X, Y, which=2):
        """ilu0_solve for the k = 2, 4 or 8 columns of X at once (lcg_hip_ilu0_solve_multi); as ic0_solve_multi."""
        k = _block_k(X, Y)
        _chk(L.load().lcg_hip_ilu0_solve_multi(self.h, k, which, _ptr(X)[0], _ptr(Y)[0]), "ilu0_solve_multi")

    def spmv(self, x, y):
        _chk(L.load().lcg_hip_spmv(self.h, _ptr(x)[0], _ptr(y)[0]), "spmv")

    def spmm(self, X, Y):
        """Y = A.X for the k = 2, 4 or 8 columns of X in one launch (lcg_hip_spmm): X (n_cols, k) and Y (n_rows, k) are C-contiguous
        float64 CUDA tensors, 16-byte aligned.  Real fp64 matrices on one GPU."""
        k = _block_k(X, Y)
        _chk(L.load().lcg_hip_spmm(self.h, k, _ptr(X)[0], _ptr(Y)[0]), "spmm")

    def spmm_dot2(self, X, Y, U):
        """spmm carrying two sums per column (lcg_hip_spmm_dot2): returns a float64 array of 2k, [j] = Y_j . U_j and
        [k + j] = Y_j . Y_j -- what BiCGStab takes after its second product.  X, Y, U as spmm's blocks."""
        k = _block_k(X, Y, U)
        out = (C.c_double * (2 * k))()
        _chk(L.load().lcg_hip_spmm_dot2(self.h, k, _ptr(X)[0], _ptr(Y)[0], _ptr(U)[0], out), "spmm_dot2")
        return np.array(out[:], dtype=np.float64)

    def cspmm(self, X, Y):
        """Y = A.X for the k = 2, 4 or 8 complex columns of X in one launch (clcg_hip_spmm): X (n_cols, k) and Y (n_rows, k) are
        C-contiguous complex128 CUDA tensors, 16-byte aligned.  Complex128 matrices on one GPU."""
        k = _block_k(X, Y, cplx=True)
        _chk(L.load().clcg_hip_spmm(self.h, k, _ptr(X)[0], _ptr(Y)[0]), "cspmm")

    def cspmm_dot(self, X, Y, U):
        """cspmm carrying one unconjugated sum per column (clcg_hip_spmm_dot): returns a complex128 array of k,
        [j] = sum_i Y_ij U_ij -- what the batched complex loops take after their product.  X, Y, U as cspmm's blocks."""
        k = _block_k(X, Y, U, cplx=True)
        out = (C.c_double * (2 * k))()
        _chk(L.load().clcg_hip_spmm_dot(self.h, k, _ptr(X)[0], _ptr(Y)[0], _ptr(U)[0], out), "cspmm_dot")
        return np.array(out[:], dtype=np.float64).view(np.complex128)

    def cspmm_inner(self, X, Y, u):
        """cspmm carrying one conjugated sum per column against ONE vector (clcg_hip_spmm_inner): returns a complex128 array of k,
        [j] = sum_i conj(u_i) Y_ij -- what the batched complex BiCGStab takes after its first product.  X, Y as cspmm's blocks; u a
        contiguous 1-D complex128 vector of n_rows elements shared by all columns, 16-byte aligned."""
        k = _block_k(X, Y, cplx=True)
        if isinstance(u, np.ndarray):
            ok = u.ndim == 1 and u.dtype == np.complex128 and u.flags["C_CONTIGUOUS"]
        else:
            import torch
            ok = isinstance(u, torch.Tensor) and u.dim() == 1 and u.dtype == torch.complex128 and u.is_contiguous()
        if not ok or u.shape[0] != Y.shape[0]:
            raise ValueError("u is a contiguous 1-D complex128 vector with one element per row of Y")
        out = (C.c_double * (2 * k))()
        _chk(L.load().clcg_hip_spmm_inner(self.h, k, _ptr(X)[0], _ptr(Y)[0], _ptr(u)[0], out), "cspmm_inner")
        return np.array(out[:], dtype=np.float64).view(np.complex128)

    def cspmm_dot2(self, X, Y, U):
        """cspmm carrying two sums per column (clcg_hip_spmm_dot2): returns (a complex128 array of k, [j] = sum_i conj(Y_ij) U_ij;
        a float64 array of k, [j] = sum_i |Y_ij|^2) -- what the batched complex BiCGStab takes after its second product.  X, Y, U as
        cspmm's blocks."""
        k = _block_k(X, Y, U, cplx=True)
        out = (C.c_double * (3 * k))()
        _chk(L.load().clcg_hip_spmm_dot2(self.h, k, _ptr(X)[0], _ptr(Y)[0], _ptr(U)[0], out), "cspmm_dot2")
        return np.array(out[:2 * k], dtype=np.float64).view(np.complex128), np.array(out[2 * k:], dtype=np.float64)

    def cspmm_c64(self, X, Y):
        """Y = A.X for the k = 2, 4 or 8 complex64 columns of X in one launch (clcg_hip_spmm_c64): X (n_cols, k) and Y (n_rows, k) are
        C-contiguous complex64 CUDA tensors, 16-byte aligned.  Complex64 matrices (from_csr_c64) on one GPU."""
        k = _block_k(X, Y, cplx="c64")
        _chk(L.load().clcg_hip_spmm_c64(self.h, k, _ptr(X)[0], _ptr(Y)[0]), "cspmm_c64")

    def cspmm_dot_c64(self, X, Y, U):
        """cspmm_c64 carrying one unconjugated sum per column (clcg_hip_spmm_dot_c64): returns a complex128 array of k,
        [j] = sum_i Y_ij U_ij in fp64 -- what the batched complex64 loops take after their product.  X, Y, U as cspmm_c64's blocks."""
        k = _block_k(X, Y, U, cplx="c64")
        out = (C.c_double * (2 * k))()
        _chk(L.load().clcg_hip_spmm_dot_c64(self.h, k, _ptr(X)[0], _ptr(Y)[0], _ptr(U)[0], out), "cspmm_dot_c64")
        return np.array(out[:], dtype=np.float64).view(np.complex128)

    # -- sparse least squares: K^T.x, K^T.K.x on a rectangular matrix (csr_normal.hip) ------------
    @property
    def n_cols(self) -> int:
        return L.load().lcg_hip_csr_cols(self.h)

    def build_normal(self):
        """Materialise K^T and the work vectors beside the matrix (lcg_hip_csr_build_normal): what spmv_t, ata, the k-wide forms, the
        callbacks 'lcg_hip_csr_ata_ax' / 'lcg_hip_csr_jacobi_normal_mx' and the csr_normal_* loops need.  Idempotent."""
        _chk(L.load().lcg_hip_csr_build_normal(self.h), "build_normal")

    def normal_info(self) -> dict:
        lc, nb, ms = C.c_int(), C.c_int64(), C.c_double()
        _chk(L.load().lcg_hip_csr_normal_info(self.h, C.byref(lc), C.byref(nb), C.byref(ms)), "normal_info")
        return {"longest_column": lc.value, "extra_bytes": nb.value, "build_ms": ms.value}

    def normal_to_host(self):
        """(rowptr, col, val) of K^T copied to numpy: rows by source row, duplicates in K's own entry order."""
        lib = L.load()
        pr, pc, pv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _chk(lib.lcg_hip_csr_normal_arrays(self.h, C.byref(pr), C.byref(pc), C.byref(pv)), "normal_arrays")
        nnz = self.nnz
        rowptr = np.empty(self.n_cols + 1, np.int32); col = np.empty(nnz, np.int32); val = np.empty(nnz, np.float64)
        for dst, src in ((rowptr, pr), (col, pc), (val, pv)):
            if dst.nbytes:
                _chk(lib.lcg_hip_memcpy(dst.ctypes.data, src, dst.nbytes, 2), "memcpy d2h")
        return rowptr, col, val

    def spmv_t(self, x, y):
        """y (n_cols) = K^T.x (n_rows) (lcg_hip_spmv_t): how b = K^T.d is formed."""
        _chk(L.load().lcg_hip_spmv_t(self.h, _ptr(x)[0], _ptr(y)[0]), "spmv_t")

    def ata(self, x, y):
        """y = K^T.(K.x), both of n_cols elements (lcg_hip_csr_ata)."""
        _chk(L.load().lcg_hip_csr_ata(self.h, _ptr(x)[0], _ptr(y)[0]), "csr_ata")

    def spmm_t(self, X, Y):
        """Y (n_cols, k) = K^T.X (n_rows, k) for k = 2, 4 or 8 columns (lcg_hip_spmm_t); blocks as spmm's."""
        k = _block_k(X, Y)
        _chk(L.load().lcg_hip_spmm_t(self.h, k, _ptr(X)[0], _ptr(Y)[0]), "spmm_t")

    def ata_multi(self, X, Y):
        """Y = K^T.(K.X) for the k columns of X, both matrices read once for all of them (lcg_hip_csr_ata_multi).  X, Y: (n_cols, k)."""
        k = _block_k(X, Y)
        _chk(L.load().lcg_hip_csr_ata_multi(self.h, k, _ptr(X)[0], _ptr(Y)[0]), "csr_ata_multi")

    def ata_multi_dot(self, X, Y, U):
        """ata_multi carrying the sum the batched loops take after it (lcg_hip_csr_ata_multi_dot): returns a float64 array of k,
        [j] = Y_j . U_j.  X, Y, U: (n_cols, k) blocks."""
        k = _block_k(X, Y, U)
        out = (C.c_double * k)()
        _chk(L.load().lcg_hip_csr_ata_multi_dot(self.h, k, _ptr(X)[0], _ptr(Y)[0], _ptr(U)[0], out), "csr_ata_multi_dot")
        return np.array(out[:], dtype=np.float64)

    def build_jacobi_normal(self, diag_out=None):
        """The reciprocals of diag(K^T.K) = the columns' sums of squares (lcg_hip_csr_build_jacobi_normal), kept beside
        build_jacobi()'s; diag_out (a float64 CUDA tensor of n_cols) receives the sums.  Mfp: 'lcg_hip_csr_jacobi_normal_mx'."""
        p = None if diag_out is None else _ptr(diag_out)[0]
        _chk(L.load().lcg_hip_csr_build_jacobi_normal(self.h, p), "build_jacobi_normal")

    def distribute(self, n_global: int, mode: int = 0):
        _chk(L.load().lcg_hip_csr_distribute(self.h, n_global, mode), "csr_distribute")

    def destroy(self):
        if self.h:
            L.load().lcg_hip_csr_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class DenseMatrix:
    """An HBM-resident dense matrix (handle ``lcg_hip_dense_t``): K.x, K^T.x, K^T.K.x and the callbacks
    'lcg_hip_dense_ata_ax', 'lcg_hip_dense_ax', 'clcg_hip_dense_ax', 'lcg_hip_dense_jacobi_mx', 'clcg_hip_dense_jacobi_mx'."""
    KERNEL_AUTO, KERNEL_ROW, KERNEL_ROW_SPLIT, KERNEL_COL, KERNEL_ATA_TWO_PASS, KERNEL_ATA_ONE_PASS, KERNEL_ATA_SMALL = range(7)
    is_c64 = False      # entries are complex64 (from_array_c64): the *_c64 methods and callbacks serve it, the others refuse it

    def __init__(self, handle: int, m: int, n: int, is_complex: bool):
        self.h = C.c_void_p(handle)
        self.m, self.n, self.is_complex = m, n, is_complex

    @classmethod
    def from_array(cls, K):
        """K: a 2-d numpy array (host; copied) or torch CUDA tensor (device; copied), row-major; the last axis may be a
        view of a wider array (its stride is the leading dimension)."""
        lib = L.load()
        if isinstance(K, np.ndarray):
            is_c = bool(np.iscomplexobj(K))
            if (K.ndim != 2 or K.strides[1] != K.itemsize or K.dtype not in (np.float64, np.complex128) or K.strides[0] % K.itemsize
                    or (K.shape[0] > 1 and K.strides[0] < K.shape[1] * K.itemsize)):
                K = np.ascontiguousarray(K, np.complex128 if is_c else np.float64)
            ld, ptr, mem = K.strides[0] // K.itemsize, K.ctypes.data, MEM_HOST
        else:
            is_c = K.is_complex()
            if K.dim() != 2 or K.stride(1) != 1:
                raise ValueError("a 2-d tensor with unit stride along its rows is needed")
            ld, ptr, mem = K.stride(0), K.data_ptr(), (MEM_DEVICE if K.is_cuda else MEM_HOST)
        m, n = K.shape
        if ld < n:
            if m != 1:          # a broadcast or overlapping-rows view: never read with a pitch it does not have
                raise ValueError(f"rows {ld} entries apart hold {n} entries: make the array contiguous first")
            ld = n              # one row: its stride means nothing
        h = C.c_void_p()
        _chk(lib.lcg_hip_dense_create(C.byref(h), m, n, ptr, ld, int(is_c), mem), "dense_create")
        return cls(h.value, m, n, is_c)

    @classmethod
    def from_array_c64(cls, K):
        """A complex64 matrix (lcg_hip_dense_create_c64), 8 bytes per entry, nothing widened: K is a 2-d numpy complex64 array (host;
        copied) or a torch.complex64 tensor (copied), row-major; the last axis may be a view of a wider array.  Products:
        matvec_c64, cmatmat_c64, cop_multi_dot_c64; callbacks 'clcg_hip_dense_ax_c64', 'clcg_hip_dense_jacobi_mx_c64' for
        clcg_solver_c64 / clcg_solver_preconditioned_c64; batched loops: dense_clbicg_sym_multi_c64, dense_clpcg_multi_c64."""
        lib = L.load()
        if isinstance(K, np.ndarray):
            if K.dtype != np.complex64:
                raise TypeError(f"from_array_c64 takes complex64 entries, not {K.dtype}")
            if (K.ndim != 2 or K.strides[1] != K.itemsize or K.strides[0] % K.itemsize
                    or (K.shape[0] > 1 and K.strides[0] < K.shape[1] * K.itemsize)):
                K = np.ascontiguousarray(K)
            ld, ptr, mem = K.strides[0] // K.itemsize, K.ctypes.data, MEM_HOST
        else:
            import torch
            if K.dtype != torch.complex64:
                raise TypeError(f"from_array_c64 takes complex64 entries, not {K.dtype}")
            if K.dim() != 2 or K.stride(1) != 1:
                raise ValueError("a 2-d tensor with unit stride along its rows is needed")
            ld, ptr, mem = K.stride(0), K.data_ptr(), (MEM_DEVICE if K.is_cuda else MEM_HOST)
        m, n = K.shape
        if ld < n:
            if m != 1:
                raise ValueError(f"rows {ld} entries apart hold {n} entries: make the array contiguous first")
            ld = n
        h = C.c_void_p()
        _chk(lib.lcg_hip_dense_create_c64(C.byref(h), m, n, ptr, ld, mem), "dense_create_c64")
        D = cls(h.value, m, n, True)
        D.is_c64 = True
        return D

    @classmethod
    def from_array_f32(cls, K):
        """A real matrix kept as fp32 (lcg_hip_dense_create_f32), 4 bytes per entry: K is a 2-d numpy float32 array (host; copied) or a
        torch.float32 tensor (copied), row-major; the last axis may be a view of a wider array.  Nothing is cast in either direction: a
        float64 array is refused (from_array takes it), and from_array keeps widening a float32 one.  Vectors, sums and solver state stay
        fp64 and every method and callback of a real fp64 matrix serves the handle, with the bits of from_array(K.astype(float64))."""
        lib = L.load()
        if isinstance(K, np.ndarray):
            if K.dtype != np.float32:
                raise TypeError(f"from_array_f32 takes float32 entries, not {K.dtype}")
            if (K.ndim != 2 or K.strides[1] != K.itemsize or K.strides[0] % K.itemsize
                    or (K.shape[0] > 1 and K.strides[0] < K.shape[1] * K.itemsize)):
                K = np.ascontiguousarray(K)
            ld, ptr, mem = K.strides[0] // K.itemsize, K.ctypes.data, MEM_HOST
        else:
            import torch
            if K.dtype != torch.float32:
                raise TypeError(f"from_array_f32 takes float32 entries, not {K.dtype}")
            if K.dim() != 2 or K.stride(1) != 1:
                raise ValueError("a 2-d tensor with unit stride along its rows is needed")
            ld, ptr, mem = K.stride(0), K.data_ptr(), (MEM_DEVICE if K.is_cuda else MEM_HOST)
        m, n = K.shape
        if ld < n:
            if m != 1:
                raise ValueError(f"rows {ld} entries apart hold {n} entries: make the array contiguous first")
            ld = n
        h = C.c_void_p()
        _chk(lib.lcg_hip_dense_create_f32(C.byref(h), m, n, ptr, ld, mem), "dense_create_f32")
        return cls(h.value, m, n, False)

    @property
    def value_bytes(self) -> int:
        """Bytes per stored entry of K (lcg_hip_dense_value_bytes): 4 (from_array_f32), 8 (float64, complex64) or 16 (complex128)."""
        return _chk(L.load().lcg_hip_dense_value_bytes(self.h), "dense_value_bytes")

    def matvec_c64(self, x, y, layout=0, conjugate=0):
        """y = op(K).x for a complex64 matrix (clcg_hip_dense_matvec_c64): torch.complex64 CUDA tensors; layout 1: K^T, conjugate 1:
        conj(K) / K^H."""
        return _chk(L.load().clcg_hip_dense_matvec_c64(self.h, _ptr(x)[0], _ptr(y)[0], layout, conjugate), "dense_matvec_c64")

    def build_jacobi_c64(self, diag_out=None):
        """The complex64 reciprocals 1 / K(i,i) of a square complex64 matrix (lcg_hip_dense_build_jacobi_c64); diag_out (a
        torch.complex64 CUDA tensor of n) receives the diagonal."""
        p = None if diag_out is None else _ptr(diag_out)[0]
        return _chk(L.load().lcg_hip_dense_build_jacobi_c64(self.h, p), "dense_build_jacobi_c64")

    def cmatmat_c64(self, X, Y, conjugate=0):
        """Y = K.X (conjugate 1: conj(K).X) for the k = 2, 4 or 8 complex64 columns of X with K read once for all of them, on the fp32
        matrix instruction (clcg_hip_dense_matmat_c64): X (n, k), Y (m, k) C-contiguous complex64 CUDA tensors, 16-byte aligned."""
        k = _block_k(X, Y, cplx="c64")
        return _chk(L.load().clcg_hip_dense_matmat_c64(self.h, k, _ptr(X)[0], _ptr(Y)[0], conjugate), "dense_cmatmat_c64")

    def cop_multi_dot_c64(self, X, Y, U):
        """Y = K.X (square complex64 K) carrying one unconjugated sum per column (clcg_hip_dense_op_multi_dot_c64): returns a
        complex128 array of k, [j] = sum_i Y_ij U_ij in fp64.  X, Y, U: (n, k) complex64 blocks."""
        k = _block_k(X, Y, U, cplx="c64")
        out = (C.c_double * (2 * k))()
        _chk(L.load().clcg_hip_dense_op_multi_dot_c64(self.h, k, _ptr(X)[0], _ptr(Y)[0], _ptr(U)[0], out), "dense_cop_multi_dot_c64")
        return np.array(out[:], dtype=np.float64).view(np.complex128)

    @staticmethod
    def kernel_names_c64():
        lib, out, i = L.load(), [], 0
        while True:
            s = lib.clcg_hip_dense_kernel_name_c64(i)
            if s is None:
                return out
            out.append(s.decode()); i += 1

    @classmethod
    def from_rows(cls, rows, is_complex=False):
        """rows: a sequence of 1-d numpy arrays of one length (liblcg's lcg_float ** layout)."""
        lib = L.load()
        rows = [np.ascontiguousarray(r, np.complex128 if is_complex else np.float64) for r in rows]
        ptrs = (C.c_void_p * len(rows))(*[r.ctypes.data for r in rows])
        h = C.c_void_p()
        _chk(lib.lcg_hip_dense_create_rows(C.byref(h), len(rows), len(rows[0]), ptrs, int(is_complex)), "dense_create_rows")
        return cls(h.value, len(rows), len(rows[0]), is_complex)

    def matvec(self, x, y, layout=0, conjugate=0):
        lib = L.load()
        if self.is_complex:
            return _chk(lib.clcg_hip_dense_matvec(self.h, _ptr(x)[0], _ptr(y)[0], layout, conjugate), "dense_matvec")
        return _chk(lib.lcg_hip_dense_matvec(self.h, _ptr(x)[0], _ptr(y)[0], layout), "dense_matvec")

    def ata(self, x, y):
        return _chk(L.load().lcg_hip_dense_ata(self.h, _ptr(x)[0], _ptr(y)[0]), "dense_ata")

    def build_jacobi(self, normal=True, diag_out=None):
        p = None if diag_out is None else _ptr(diag_out)[0]
        return _chk(L.load().lcg_hip_dense_build_jacobi(self.h, int(normal), p), "dense_build_jacobi")

    def set_kernel(self, variant: int):
        return _chk(L.load().lcg_hip_dense_set_kernel(self.h, variant), "dense_set_kernel")

    @property
    def last_kernel(self) -> str:
        return L.load().lcg_hip_dense_last_kernel(self.h).decode()

    @staticmethod
    def kernel_names():
        lib, out, i = L.load(), [], 0
        while True:
            s = lib.lcg_hip_dense_kernel_name(i)
            if s is None:
                return out
            out.append(s.decode()); i += 1

    def matmat(self, X, Y, layout=0):
        """Y = K.X (layout 0: X (n, k), Y (m, k)) or K^T.X (layout 1: X (m, k), Y (n, k)) for the k = 2, 4 or 8 columns of X with K
        read once for all of them (lcg_hip_dense_matmat): C-contiguous float64 CUDA tensors, 16-byte aligned.  Real fp64 matrices."""
        k = _block_k(X, Y)
        return _chk(L.load().lcg_hip_dense_matmat(self.h, k, _ptr(X)[0], _ptr(Y)[0], layout), "dense_matmat")

    def ata_multi(self, X, Y):
        """Y = K^T.(K.X) for the k columns of X, K read twice for all of them (lcg_hip_dense_ata_multi).  X, Y: (n, k) blocks."""
        k = _block_k(X, Y)
        return _chk(L.load().lcg_hip_dense_ata_multi(self.h, k, _ptr(X)[0], _ptr(Y)[0]), "dense_ata_multi")

    def op_multi_dot(self, X, Y, U, normal=True):
        """Y = (K^T.K if normal else K).X carrying, per column, the sum the batched loops take after it (lcg_hip_dense_op_multi_dot):
        returns a float64 array of k, [j] = Y_j . U_j.  X, Y, U: (n, k) blocks."""
        k = _block_k(X, Y, U)
        out = (C.c_double * k)()
        _chk(L.load().lcg_hip_dense_op_multi_dot(self.h, k, int(normal), _ptr(X)[0], _ptr(Y)[0], _ptr(U)[0], out), "dense_op_multi_dot")
        return np.array(out[:], dtype=np.float64)

    def cmatmat(self, X, Y, layout=0, conjugate=0):
        """Y = op(K).X for the k = 2, 4 or 8 complex columns of X with K read once for all of them (clcg_hip_dense_matmat): layout 0
        K.X (X (n, k), Y (m, k)), layout 1 K^T.X (X (m, k), Y (n, k)); conjugate 1: conj(K) / K^H.  C-contiguous complex128 CUDA
        tensors, 16-byte aligned.  Complex128 matrices."""
        k = _block_k(X, Y, cplx=True)
        return _chk(L.load().clcg_hip_dense_matmat(self.h, k, _ptr(X)[0], _ptr(Y)[0], layout, conjugate), "dense_cmatmat")

    def cop_multi_dot(self, X, Y, U):
        """Y = K.X (square complex128 K) carrying one unconjugated sum per column (clcg_hip_dense_op_multi_dot): returns a complex128
        array of k, [j] = sum_i Y_ij U_ij -- what the batched complex loops take after their product.  X, Y, U: (n, k) blocks."""
        k = _block_k(X, Y, U, cplx=True)
        out = (C.c_double * (2 * k))()
        _chk(L.load().clcg_hip_dense_op_multi_dot(self.h, k, _ptr(X)[0], _ptr(Y)[0], _ptr(U)[0], out), "dense_cop_multi_dot")
        return np.array(out[:], dtype=np.float64).view(np.complex128)

    @property
    def multi_last_kernel(self) -> str:
        return L.load().lcg_hip_dense_multi_last_kernel(self.h).decode()

    @staticmethod
    def cmulti_kernel_names():
        lib, out, i = L.load(), [], 0
        while True:
            s = lib.clcg_hip_dense_multi_kernel_name(i)
            if s is None:
                return out
            out.append(s.decode()); i += 1

    @staticmethod
    def multi_kernel_names():
        lib, out, i = L.load(), [], 0
        while True:
            s = lib.lcg_hip_dense_multi_kernel_name(i)
            if s is None:
                return out
            out.append(s.decode()); i += 1

    def destroy(self):
        if self.h:
            L.load().lcg_hip_dense_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


@dataclass
class SolveInfo:
    ret: int
    iterations: int
    residual: float


def _cb(fn, proto):
    """None, an exported C symbol name, a raw address, or a Python callable -> (address, keepalive)."""
    lib = L.load()
    if fn is None:
        return None, None
    if isinstance(fn, str):
        return L.fnptr(lib, fn), None
    if isinstance(fn, (int, C.c_void_p)):
        return fn, None
    cfn = proto(fn)
    return C.cast(cfn, C.c_void_p), cfn


def _instance(instance):
    if isinstance(instance, (CsrMatrix, DenseMatrix)):
        return instance.h
    return instance


def lcg_solver(Afp, Pfp, m, B, n_size, param, instance, solver_id=LCG_CGS) -> SolveInfo:
    """lcg_solver(), lcg.h:71-72.  Afp: 'lcg_hip_csr_ax' (built-in) or a Python callable
    (instance, x_ptr, Ax_ptr, n) that launches device work on lcg_hip_get_stream()."""
    lib = L.load()
    a, k1 = _cb(Afp, AXFUNC); p, k2 = _cb(Pfp, PROGRESS)
    (pm, mem), (pb, mem_b) = _ptr(m), _ptr(B)
    if mem != mem_b:
        raise ValueError("m and B must live in the same memory space")
    rc = lib.lcg_hip_solver(a, p, pm, pb, n_size, C.byref(param) if param is not None else None,
                            _instance(instance), solver_id, mem)
    _chk(rc, "lcg_solver")
    return SolveInfo(rc, lib.lcg_hip_last_iterations(), lib.lcg_hip_last_residual())


def lcg_solver_preconditioned(Afp, Mfp, Pfp, m, B, n_size, param, instance, solver_id=LCG_PCG) -> SolveInfo:
    """lcg_solver_preconditioned(), lcg.h:90-91."""
    lib = L.load()
    a, k1 = _cb(Afp, AXFUNC); mm, k3 = _cb(Mfp, AXFUNC); p, k2 = _cb(Pfp, PROGRESS)
    (pm, mem), (pb, _) = _ptr(m), _ptr(B)
    rc = lib.lcg_hip_solver_preconditioned(a, mm, p, pm, pb, n_size, C.byref(param) if param is not None else None,
                                           _instance(instance), solver_id, mem)
    _chk(rc, "lcg_solver_preconditioned")
    return SolveInfo(rc, lib.lcg_hip_last_iterations(), lib.lcg_hip_last_residual())


def lcg_solver_constrained(Afp, Pfp, m, B, low, hig, n_size, param, instance, solver_id=LCG_PG) -> SolveInfo:
    """lcg_solver_constrained(), lcg.h:111-113 (LCG_PG / LCG_SPG)."""
    lib = L.load()
    a, k1 = _cb(Afp, AXFUNC); p, k2 = _cb(Pfp, PROGRESS)
    (pm, mem), (pb, _), (pl, _), (ph, _) = _ptr(m), _ptr(B), _ptr(low), _ptr(hig)
    rc = lib.lcg_hip_solver_constrained(a, p, pm, pb, pl, ph, n_size, C.byref(param) if param is not None else None,
                                        _instance(instance), solver_id, mem)
    _chk(rc, "lcg_solver_constrained")
    return SolveInfo(rc, lib.lcg_hip_last_iterations(), lib.lcg_hip_last_residual())


def lcg(Afp, Pfp, m, B, n_size, param, instance, Gk=None, Dk=None, ADk=None) -> SolveInfo:
    """lcg() with optional caller workspaces (device tensors), lcg.h:135-137."""
    lib = L.load()
    a, k1 = _cb(Afp, AXFUNC); p, k2 = _cb(Pfp, PROGRESS)
    (pm, mem), (pb, _) = _ptr(m), _ptr(B)
    ws = [None if w is None else _ptr(w)[0] for w in (Gk, Dk, ADk)]
    rc = lib.lcg_hip_lcg(a, p, pm, pb, n_size, C.byref(param) if param is not None else None, _instance(instance),
                         ws[0], ws[1], ws[2], mem)
    _chk(rc, "lcg")
    return SolveInfo(rc, lib.lcg_hip_last_iterations(), lib.lcg_hip_last_residual())


def _block_k(*blocks, cplx=False):
    """k of 2-D (n, k) C-contiguous float64 (cplx: complex128; cplx="c64": complex64) blocks of vectors (numpy arrays or torch
    tensors), all alike."""
    name = "complex64" if cplx == "c64" else ("complex128" if cplx else "float64")
    k = None
    for X in blocks:
        if isinstance(X, np.ndarray):
            ok = X.ndim == 2 and X.dtype == np.dtype(name) and X.flags["C_CONTIGUOUS"]
        else:
            import torch
            ok = isinstance(X, torch.Tensor) and X.dim() == 2 and X.dtype == getattr(torch, name) and X.is_contiguous()
        if not ok:
            raise ValueError(f"a block of vectors is a 2-D (n, k) C-contiguous {name} array or tensor")
        if k is not None and X.shape[1] != k:
            raise ValueError("blocks of vectors with different k")
        k = int(X.shape[1])
    return k


PRECONDS = {"jacobi": 0, "ic0": 1, "ilu0": 2}       # LCG_HIP_M_JACOBI, LCG_HIP_M_IC0, LCG_HIP_M_ILU0
M_NONE = -1                                         # LCG_HIP_M_NONE


def _multi(name, A, M, B, param, precond=None, cplx=False):
    lib = L.load()
    k = _block_k(M, B, cplx=cplx)
    if tuple(M.shape) != tuple(B.shape):
        raise ValueError("M and B must have the same shape")
    (pm, mem), (pb, mem_b) = _ptr(M), _ptr(B)
    if mem != mem_b:
        raise ValueError("M and B must live in the same memory space")
    ret = (C.c_int * k)(); its = (C.c_int * k)(); res = (C.c_double * k)()
    lead = (_instance(A), k) if precond is None else (_instance(A), k, precond)
    rc = getattr(lib, name)(*lead, pm, pb, C.byref(param) if param is not None else None, ret, its, res, mem)
    _chk(rc, name)
    if rc:
        raise LcgHipError(f"{name}: rc={rc}")
    return [SolveInfo(ret[j], its[j], res[j]) for j in range(k)]


def lcg_multi(A, M, B, param) -> list:
    """Batched CG (lcg_hip_lcg_multi): M (in/out) and B are (n, k) blocks of k = 2, 4 or 8 columns, every column solved as if it
    were alone while the matrix is read once per iteration for all of them.  Returns one SolveInfo per column."""
    return _multi("lcg_hip_lcg_multi", A, M, B, param)


def lpcg_multi(A, M, B, param, precond="jacobi") -> list:
    """Batched PCG.  precond "jacobi": the built-in Jacobi (lcg_hip_lpcg_multi; A.build_jacobi() first); "ic0" / "ilu0": the
    handle's factor (A.build_ic0() / A.build_ilu0() first) applied to all columns at once at its sweeps setting
    (lcg_hip_lpcg_multi_m).  As lcg_multi."""
    if precond not in PRECONDS:
        raise ValueError('precond is "jacobi", "ic0" or "ilu0"')
    if precond == "jacobi":
        return _multi("lcg_hip_lpcg_multi", A, M, B, param)
    return _multi("lcg_hip_lpcg_multi_m", A, M, B, param, PRECONDS[precond])


def dense_lcg_multi(K, M, B, param, normal=True) -> list:
    """Batched CG on a dense matrix (lcg_hip_dense_lcg_multi): the operator is K^T.K (normal: sample1's normal equations) or K
    (square); M (in/out) and B are (n, k) blocks of k = 2, 4 or 8 columns, every column solved as if it were alone while K is read
    once per product for all of them.  Returns one SolveInfo per column, as lcg_multi."""
    return _multi("lcg_hip_dense_lcg_multi", K, M, B, param, int(normal))


def dense_lpcg_multi(K, M, B, param, normal=True) -> list:
    """Batched PCG on a dense matrix with the reciprocals of K.build_jacobi(normal) (lcg_hip_dense_lpcg_multi).  As dense_lcg_multi."""
    return _multi("lcg_hip_dense_lpcg_multi", K, M, B, param, int(normal))


@dataclass
class BoxSolveInfo(SolveInfo):
    products: int       # A.x calls the reference would have made for this column alone: 1 + its trial points


def _box_multi(name, lead, M, B, low, hig, param, solver_id):
    lib = L.load()
    k = _block_k(M, B)
    if tuple(M.shape) != tuple(B.shape):
        raise ValueError("M and B must have the same shape")
    (pm, mem), (pb, mem_b), (pl, mem_l), (ph, mem_h) = _ptr(M), _ptr(B), _ptr(low), _ptr(hig)
    if not mem == mem_b == mem_l == mem_h:
        raise ValueError("M, B, low and hig must live in the same memory space")
    if int(low.shape[0]) != int(M.shape[0]) or int(hig.shape[0]) != int(M.shape[0]):
        raise ValueError("low and hig are vectors of n = M.shape[0] elements")
    ret = (C.c_int * k)(); its = (C.c_int * k)(); prods = (C.c_int * k)(); res = (C.c_double * k)()
    rc = getattr(lib, name)(*lead, solver_id, pm, pb, pl, ph, C.byref(param) if param is not None else None, ret, its, prods, res, mem)
    _chk(rc, name)
    if rc:
        raise LcgHipError(f"{name}: rc={rc}")
    return [BoxSolveInfo(ret[j], its[j], res[j], prods[j]) for j in range(k)]


def lcg_solver_constrained_multi(A, M, B, low, hig, param, solver_id=LCG_PG) -> list:
    """Batched box-constrained solve (lcg_hip_solver_constrained_multi): LCG_PG / LCG_SPG per column as lcg_solver_constrained
    runs them, for the k = 2, 4 or 8 columns of the (n, k) blocks M (in/out) and B; low, hig: one vector of n bounds each, shared by
    all columns.  The matrix is read once per trial step for all columns and the line search runs on the device.  Returns one
    BoxSolveInfo per column: ret, iterations, residual and products."""
    return _box_multi("lcg_hip_solver_constrained_multi", (_instance(A), _block_k(M, B)), M, B, low, hig, param, solver_id)


def dense_solver_constrained_multi(K, M, B, low, hig, param, solver_id=LCG_PG, normal=True) -> list:
    """Batched box-constrained solve on a dense matrix (lcg_hip_dense_solver_constrained_multi): the operator is K^T.K (normal)
    or K (square).  As lcg_solver_constrained_multi."""
    return _box_multi("lcg_hip_dense_solver_constrained_multi", (_instance(K), _block_k(M, B), int(normal)), M, B, low, hig, param, solver_id)


def csr_normal_lcg_multi(K, M, B, param) -> list:
    """Batched CG on K^T.K of a rectangular CSR matrix (lcg_hip_csr_normal_lcg_multi; K.build_normal() first): M (in/out) and B are
    (n_cols, k) blocks of k = 2, 4 or 8 columns, every column solved as if it were alone while K and K^T are read once per iteration
    for all of them.  Returns one SolveInfo per column, as dense_lcg_multi."""
    return _multi("lcg_hip_csr_normal_lcg_multi", K, M, B, param)


def csr_normal_lpcg_multi(K, M, B, param) -> list:
    """Batched PCG on K^T.K with the reciprocals of K.build_jacobi_normal() (lcg_hip_csr_normal_lpcg_multi).  As csr_normal_lcg_multi."""
    return _multi("lcg_hip_csr_normal_lpcg_multi", K, M, B, param)


def csr_normal_solver_constrained_multi(K, M, B, low, hig, param, solver_id=LCG_PG) -> list:
    """Batched box-constrained solve on K^T.K of a rectangular CSR matrix (lcg_hip_csr_normal_solver_constrained_multi).  As
    lcg_solver_constrained_multi."""
    return _box_multi("lcg_hip_csr_normal_solver_constrained_multi", (_instance(K), _block_k(M, B)), M, B, low, hig, param, solver_id)


def lbicgstab_multi(A, M, B, param, precond=None) -> list:
    """Batched BiCGStab for a square real matrix, symmetric or not (lcg_hip_lbicgstab_multi).  precond None: plain; "jacobi",
    "ic0", "ilu0": right-preconditioned in x-space with the handle's diagonal or factor (built first) applied to all columns at
    once -- M holds the solution itself, nothing is applied afterwards.  As lcg_multi."""
    if precond is not None and precond not in PRECONDS:
        raise ValueError('precond is None, "jacobi", "ic0" or "ilu0"')
    return _multi("lcg_hip_lbicgstab_multi", A, M, B, param, M_NONE if precond is None else PRECONDS[precond])


def clbicg_sym_multi(A, M, B, param) -> list:
    """Batched BiCG for a complex-symmetric complex128 matrix (clcg_hip_lbicg_sym_multi): M (in/out) and B are (n, k) complex128
    blocks of k = 2, 4 or 8 columns, every column solved as if it were alone while the matrix is read once per iteration for all
    of them.  param: a ClcgPara (or None).  Returns one SolveInfo per column."""
    return _multi("clcg_hip_lbicg_sym_multi", A, M, B, param, cplx=True)


def clbicgstab_multi(A, M, B, param, precond=None) -> list:
    """Batched BiCGStab for a square complex128 matrix, symmetric or not (clcg_hip_lbicgstab_multi).  precond None: plain; "jacobi":
    right-preconditioned in x-space with the handle's diagonal (A.build_jacobi() first) -- M holds the solution itself, nothing is
    applied afterwards.  The shadow residual is the next complex solve's (lcg_hip_set_shadow_seed / _vector), one vector for all
    columns.  As clbicg_sym_multi."""
    if precond not in (None, "jacobi"):
        raise ValueError('precond is None or "jacobi"')
    return _multi("clcg_hip_lbicgstab_multi", A, M, B, param, M_NONE if precond is None else PRECONDS[precond], cplx=True)


def clpcg_multi(A, M, B, param) -> list:
    """Batched complex PCG with the handle's Jacobi diagonal (clcg_hip_lpcg_multi; A.build_jacobi() first).  A column whose sums
    turn NaN stops with CLCG_NAN_VALUE (the single-vector loop runs to the cap).  As clbicg_sym_multi."""
    return _multi("clcg_hip_lpcg_multi", A, M, B, param, cplx=True)


def clbicg_sym_multi_c64(A, M, B, param) -> list:
    """Batched BiCG for a complex-symmetric complex64 matrix (clcg_hip_lbicg_sym_multi_c64; CsrMatrix.from_csr_c64): M (in/out) and
    B are (n, k) complex64 blocks of k = 2, 4 or 8 columns, every column solved as clcg_solver_c64(CLCG_BICG_SYM) would solve it
    alone while the matrix is read once per iteration for all of them.  param: a ClcgPara (or None).  Returns one SolveInfo per
    column."""
    return _multi("clcg_hip_lbicg_sym_multi_c64", A, M, B, param, cplx="c64")


def clpcg_multi_c64(A, M, B, param, precond="jacobi") -> list:
    """Batched complex64 PCG.  precond "jacobi": the handle's Jacobi diagonal (clcg_hip_lpcg_multi_c64; A.build_jacobi() first);
    "ic0": the handle's fp32 IC(0) factor (A.build_ic0() first) applied to all columns at once at its sweeps setting
    (clcg_hip_lpcg_multi_m_c64).  As clbicg_sym_multi_c64."""
    if precond not in ("jacobi", "ic0"):
        raise ValueError('precond is "jacobi" or "ic0"')
    if precond == "jacobi":
        return _multi("clcg_hip_lpcg_multi_c64", A, M, B, param, cplx="c64")
    return _multi("clcg_hip_lpcg_multi_m_c64", A, M, B, param, PRECONDS[precond], cplx="c64")


def dense_clbicg_sym_multi(K, M, B, param) -> list:
    """Batched BiCG on a square complex-symmetric complex128 dense matrix (clcg_hip_dense_lbicg_sym_multi): K is read once per
    iteration for all k = 2, 4 or 8 columns.  As clbicg_sym_multi."""
    return _multi("clcg_hip_dense_lbicg_sym_multi", K, M, B, param, cplx=True)


def dense_clpcg_multi(K, M, B, param) -> list:
    """Batched complex PCG on a dense matrix with the reciprocals of K.build_jacobi(normal=False)
    (clcg_hip_dense_lpcg_multi).  As clpcg_multi."""
    return _multi("clcg_hip_dense_lpcg_multi", K, M, B, param, cplx=True)


def dense_clbicg_sym_multi_c64(K, M, B, param) -> list:
    """Batched BiCG on a square complex-symmetric complex64 dense matrix (clcg_hip_dense_lbicg_sym_multi_c64;
    DenseMatrix.from_array_c64): K is read once per iteration for all k = 2, 4 or 8 columns.  As clbicg_sym_multi_c64."""
    return _multi("clcg_hip_dense_lbicg_sym_multi_c64", K, M, B, param, cplx="c64")


def dense_clpcg_multi_c64(K, M, B, param) -> list:
    """Batched complex64 PCG on a dense matrix with the reciprocals of K.build_jacobi_c64() (clcg_hip_dense_lpcg_multi_c64).  As
    clbicg_sym_multi_c64."""
    return _multi("clcg_hip_dense_lpcg_multi_c64", K, M, B, param, cplx="c64")


def lcgs(Afp, Pfp, m, B, n_size, param, instance, *workspaces) -> SolveInfo:
    """lcgs() with optional caller workspaces RK,R0T,PK,AX,UK,QK,WK, lcg.h:166-169."""
    lib = L.load()
    a, k1 = _cb(Afp, AXFUNC); p, k2 = _cb(Pfp, PROGRESS)
    (pm, mem), (pb, _) = _ptr(m), _ptr(B)
    ws = list(workspaces) + [None] * (7 - len(workspaces))
    ws = [None if w is None else _ptr(w)[0] for w in ws]
    rc = lib.lcg_hip_lcgs(a, p, pm, pb, n_size, C.byref(param) if param is not None else None, _instance(instance),
                          *ws, mem)
    _chk(rc, "lcgs")
    return SolveInfo(rc, lib.lcg_hip_last_iterations(), lib.lcg_hip_last_residual())


def clcg_solver(Afp, Pfp, m, B, n_size, param, instance, solver_id=CLCG_BICG, shadow_seed=None, shadow=None) -> SolveInfo:
    """clcg_solver(), clcg.h:74-76.  m, B: complex128 (torch CUDA or numpy)."""
    lib = L.load()
    a, k1 = _cb(Afp, CAXFUNC); p, k2 = _cb(Pfp, CPROGRESS)
    (pm, mem), (pb, _) = _ptr(m), _ptr(B)
    if shadow_seed is not None:
        lib.lcg_hip_set_shadow_seed(shadow_seed)
    if shadow is not None:
        sh = np.ascontiguousarray(shadow, np.complex128)
        lib.lcg_hip_set_shadow_vector(sh.ctypes.data, len(sh))
    rc = lib.clcg_hip_solver(a, p, pm, pb, n_size, C.byref(param) if param is not None else None,
                             _instance(instance), solver_id, mem)
    _chk(rc, "clcg_solver")
    return SolveInfo(rc, lib.lcg_hip_last_iterations(), lib.lcg_hip_last_residual())


def clcg_solver_preconditioned(Afp, Mfp, Pfp, m, B, n_size, param, instance, solver_id=CLCG_PCG) -> SolveInfo:
    """clcg_solver_preconditioned_cuda(), clcg_cuda.h:105-108 -> clpcg."""
    lib = L.load()
    a, k1 = _cb(Afp, CAXFUNC); mm, k3 = _cb(Mfp, CAXFUNC); p, k2 = _cb(Pfp, CPROGRESS)
    (pm, mem), (pb, _) = _ptr(m), _ptr(B)
    rc = lib.clcg_hip_solver_preconditioned(a, mm, p, pm, pb, n_size, C.byref(param) if param is not None else None,
                                            _instance(instance), solver_id, mem)
    _chk(rc, "clcg_solver_preconditioned")
    return SolveInfo(rc, lib.lcg_hip_last_iterations(), lib.lcg_hip_last_residual())


def _c64_vectors(m, B):
    import torch
    for v in (m, B):
        if isinstance(v, np.ndarray) and v.dtype != np.complex64 or isinstance(v, torch.Tensor) and v.dtype != torch.complex64:
            raise TypeError(f"the complex64 solvers take complex64 vectors, not {v.dtype}")
    (pm, mem), (pb, mem_b) = _ptr(m), _ptr(B)
    if mem != mem_b:
        raise ValueError("m and B must live in the same memory space")
    return pm, pb, mem


def clcg_solver_c64(Afp, Pfp, m, B, n_size, param, instance, solver_id=CLCG_BICG) -> SolveInfo:
    """clcg_solver_cuda() of clcg_cudaf.cu (CLCG_BICG, CLCG_BICG_SYM).  m, B: complex64 (torch CUDA or numpy); Afp
    'clcg_hip_csr_ax_c64' or a callable (instance, x_ptr, Ax_ptr, n, layout, conjugate)."""
    lib = L.load()
    a, k1 = _cb(Afp, CAXFUNC); p, k2 = _cb(Pfp, CPROGRESS_C64)
    pm, pb, mem = _c64_vectors(m, B)
    rc = lib.clcg_hip_solver_c64(a, p, pm, pb, n_size, C.byref(param) if param is not None else None,
                                 _instance(instance), solver_id, mem)
    _chk(rc, "clcg_solver_c64")
    return SolveInfo(rc, lib.lcg_hip_last_iterations(), lib.lcg_hip_last_residual())


def clcg_solver_preconditioned_c64(Afp, Mfp, Pfp, m, B, n_size, param, instance, solver_id=CLCG_PCG) -> SolveInfo:
    """clcg_solver_preconditioned_cuda() of clcg_cudaf.cu -> clpcg in complex64; Mfp e.g. 'clcg_hip_jacobi_mx_c64' or, after
    build_ic0(), 'clcg_hip_ic0_mx_c64'."""
    lib = L.load()
    a, k1 = _cb(Afp, CAXFUNC); mm, k3 = _cb(Mfp, CAXFUNC); p, k2 = _cb(Pfp, CPROGRESS_C64)
    pm, pb, mem = _c64_vectors(m, B)
    rc = lib.clcg_hip_solver_preconditioned_c64(a, mm, p, pm, pb, n_size, C.byref(param) if param is not None else None,
                                                _instance(instance), solver_id, mem)
    _chk(rc, "clcg_solver_preconditioned_c64")
    return SolveInfo(rc, lib.lcg_hip_last_iterations(), lib.lcg_hip_last_residual())


# ---- kernel-level helpers ------------------------------------------------------------------------
def dot(a, b) -> float:
    out = C.c_double()
    _chk(L.load().lcg_hip_dot(a.numel(), _ptr(a)[0], _ptr(b)[0], C.byref(out)), "dot")
    return out.value


def nrm2(a) -> float:
    out = C.c_double()
    _chk(L.load().lcg_hip_nrm2(a.numel(), _ptr(a)[0], C.byref(out)), "nrm2")
    return out.value


def cdot(a, b, conj=False) -> complex:
    out = (C.c_double * 2)()
    f = L.load().clcg_hip_inner if conj else L.load().clcg_hip_dot
    _chk(f(a.numel(), _ptr(a)[0], _ptr(b)[0], out), "cdot")
    return complex(out[0], out[1])


def gen_xtrue(n, seed, r0, r1, out):
    _chk(L.load().lcg_hip_gen_xtrue(n, seed, r0, r1, _ptr(out)[0]), "gen_xtrue")


def synchronize():
    _chk(L.load().lcg_hip_synchronize(), "synchronize")


CG_AUTO, CG_CLASSIC, CG_ONE_REDUCTION = 0, 1, 2


def set_cg_schedule(schedule: int):
    """lcg_hip_set_cg_schedule: classic two-reduction CG or the one-reduction rearrangement."""
    _chk(L.load().lcg_hip_set_cg_schedule(schedule), "set_cg_schedule")
