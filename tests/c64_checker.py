"""NumPy restatements of the three loops of clcg_cudaf.cu -- clbicg (:86-252), clbicg_symmetric (:254-401) and clpcg
(:403-558) -- written from the math and the cited lines, as the GPU's complex64 loops (liblcg_amd/csrc/solvers_c64.hip) are.

Precision rule (the one the library states): vectors and the reference's float scalars (ak, betak, m_mod, rk_mod, the residual) are
complex64 / float32; every dot (cublasCdotc / Cdotu) and norm (cublasScnrm2) takes exact products, sums them in fp64 and is rounded
to fp32 once.  With dtype=np.complex128 the same loops run in double throughout (for checks against a direct solver).

The operator is given as callables: ax(x) = A.x and, for BiCG, ahx(x) = A^H.x (what the reference asks its callback for with
CUSPARSE_OPERATION_CONJUGATE_TRANSPOSE, :217).  mx(r) is the preconditioner of clpcg.
"""
import numpy as np

CLCG_CONVERGENCE, CLCG_STOP, CLCG_ALREADY = 0, 1, 2
LCG_REACHED_MAX_ITERATIONS = -1019
CLCG_NAN_VALUE = -1019      # (the same number as the real enum's cap code: util.h's two enums)
CLCG_INVILAD_VARIABLE_SIZE, CLCG_INVILAD_MAX_ITERATIONS, CLCG_INVILAD_EPSILON = -1023, -1022, -1021
CLCG_INVALID_POINTER, CLCG_UNKNOWN_SOLVER = -1018, -1016
CLCG_BICG, CLCG_BICG_SYM, CLCG_PCG = 0, 1, 5


class Prec:
    def __init__(self, dtype):
        self.C = np.dtype(dtype).type
        self.R = np.float32 if self.C is np.complex64 else np.float64

    def dotu(self, a, b):
        return self.C(np.dot(a.astype(np.complex128), b.astype(np.complex128)))

    def dotc(self, a, b):
        return self.C(np.vdot(a.astype(np.complex128), b.astype(np.complex128)))

    def nrm(self, a):
        a = a.astype(np.complex128)
        return self.R(np.sqrt(np.sum(a.real * a.real + a.imag * a.imag)))

    def div(self, a, b):
        """cuCdivf's scaled quotient, in the working precision."""
        R = self.R
        ar, ai, br, bi = R(a.real), R(a.imag), R(b.real), R(b.imag)
        s = R(abs(br) + abs(bi))
        oos = R(R(1) / s)
        ars, ais, brs, bis = R(ar * oos), R(ai * oos), R(br * oos), R(bi * oos)
        s = R(brs * brs + bis * bis)
        oos = R(R(1) / s)
        return self.C(complex(R((ars * brs + ais * bis) * oos), R((ais * brs - ars * bis) * oos)))

    def resid(self, rk, mm, abs_diff, n):
        R = self.R
        return R(rk / R(n)) if abs_diff else R(rk * rk / (mm * mm))


def check_args(n, para, m, b):
    """clcg_cudaf.cu:94-101 in order (the cuBLAS / cuSPARSE handle checks have no counterpart)."""
    if n <= 0:
        return CLCG_INVILAD_VARIABLE_SIZE
    if para.get("max_iterations", 0) < 0:
        return CLCG_INVILAD_MAX_ITERATIONS
    eps = para.get("epsilon", 1e-6)
    if eps <= 0.0 or eps >= 1.0:
        return CLCG_INVILAD_EPSILON
    if m is None or b is None:
        return CLCG_INVALID_POINTER
    return 0


def _norms(P, m, r, abs_diff, n, state=None):
    if state is not None:       # the library's NaN scan on the sums |m|^2, |r|^2 (no counterpart in the reference: it spins)
        state["nan"] = bool(np.isnan(np.sum(np.abs(m.astype(np.complex128)) ** 2)) or np.isnan(np.sum(np.abs(r.astype(np.complex128)) ** 2)))
    mm = P.nrm(m)
    if mm < 1.0:
        mm = P.R(1.0)
    rk = P.nrm(r)
    return P.resid(rk, mm, abs_diff, n)


def _loop(P, state, step, para, n, progress):
    """The loop head shared by the three loops (:153-197, and its twins): already optimised, progress, convergence, cap, then a body."""
    eps, max_it = para.get("epsilon", 1e-6), para.get("max_iterations", 0)
    res = state["residual"]
    if res <= eps:      # (under abs_diff only |r| / n: the reference reads m_mod uninitialised at :162)
        if progress is not None:
            progress(state["m"], res, 0)
        return CLCG_ALREADY, 0
    t = 0
    while True:
        res = state["residual"]
        if progress is not None and progress(state["m"], res, t):
            return CLCG_STOP, t
        if res <= eps:
            return CLCG_CONVERGENCE, t
        if max_it > 0 and t + 1 > max_it:
            return LCG_REACHED_MAX_ITERATIONS, t
        t += 1
        step()
        if state.get("nan"):
            return CLCG_NAN_VALUE, t


def bicg(ax, ahx, b, m0, para, dtype=np.complex64, progress=None):
    """clbicg, clcg_cudaf.cu:86-252."""
    P = Prec(dtype); C = P.C
    n = len(b); ad = para.get("abs_diff", 0)
    m = np.array(m0, dtype); b = np.asarray(b, dtype)
    r1 = (b - ax(m).astype(dtype)).astype(dtype)                  # :129-133
    d1 = r1.copy(); r2 = np.conj(r1); d2 = r2.copy()                # :134-138
    st = {"m": m, "rho": P.dotc(r2, r1)}                            # :140
    st["residual"] = _norms(P, m, r1, ad, n)                        # :143-150

    def step():
        nonlocal r1, r2, d1, d2
        Ax = ax(d1).astype(dtype)                                   # :199
        ak = P.div(st["rho"], P.dotc(d2, Ax))                       # :201-202
        st["m"] = (st["m"] + ak * d1).astype(dtype)                 # :206
        r1 = (r1 + (-ak) * Ax).astype(dtype)                        # :207
        st["residual"] = _norms(P, st["m"], r1, ad, n, st)              # :209-215
        AHd = ahx(d2).astype(dtype)                                 # :217
        r2 = (r2 + C(np.conj(-ak)) * AHd).astype(dtype)             # :219
        nxt = P.dotc(r2, r1)                                        # :221
        bk = P.div(nxt, st["rho"]); st["rho"] = nxt                 # :222-224
        d1 = (bk * d1 + r1).astype(dtype)                           # :226-227
        d2 = (C(np.conj(bk)) * d2 + r2).astype(dtype)               # :229-230
    ret, t = _loop(P, st, step, para, n, progress)
    return {"ret": ret, "iters": t, "x": st["m"], "residual": float(st["residual"])}


def bicg_sym(ax, b, m0, para, dtype=np.complex64, progress=None):
    """clbicg_symmetric, clcg_cudaf.cu:254-401."""
    P = Prec(dtype)
    n = len(b); ad = para.get("abs_diff", 0)
    m = np.array(m0, dtype); b = np.asarray(b, dtype)
    r = (b - ax(m).astype(dtype)).astype(dtype)                     # :293-297
    d = r.copy()                                                    # :298
    st = {"m": m, "rho": P.dotu(r, r)}                              # :301
    st["residual"] = _norms(P, m, r, ad, n)                         # :304-311

    def step():
        nonlocal r, d
        Ax = ax(d).astype(dtype)                                    # :360
        ak = P.div(st["rho"], P.dotu(d, Ax))                        # :362-363
        st["m"] = (st["m"] + ak * d).astype(dtype)                  # :366
        r = (r + (-ak) * Ax).astype(dtype)                          # :367
        st["residual"] = _norms(P, st["m"], r, ad, n, st)               # :369-375
        nxt = P.dotu(r, r)                                          # :377
        bk = P.div(nxt, st["rho"]); st["rho"] = nxt                 # :378-379
        d = (bk * d + r).astype(dtype)                              # :381-382
    ret, t = _loop(P, st, step, para, n, progress)
    return {"ret": ret, "iters": t, "x": st["m"], "residual": float(st["residual"])}


def pcg(ax, mx, b, m0, para, dtype=np.complex64, progress=None):
    """clpcg, clcg_cudaf.cu:403-558."""
    P = Prec(dtype)
    n = len(b); ad = para.get("abs_diff", 0)
    m = np.array(m0, dtype); b = np.asarray(b, dtype)
    r = (b - ax(m).astype(dtype)).astype(dtype)                     # :445-449
    d = mx(r).astype(dtype)                                         # :451
    st = {"m": m, "rho": P.dotu(r, d)}                              # :454
    st["residual"] = _norms(P, m, r, ad, n)                         # :457-464

    def step():
        nonlocal r, d
        Ax = ax(d).astype(dtype)                                    # :513
        ak = P.div(st["rho"], P.dotu(d, Ax))                        # :514-515
        st["m"] = (st["m"] + ak * d).astype(dtype)                  # :518
        r = (r + (-ak) * Ax).astype(dtype)                          # :519
        st["residual"] = _norms(P, st["m"], r, ad, n, st)               # :521-527
        s = mx(r).astype(dtype)                                     # :532
        nxt = P.dotu(r, s)                                          # :529
        bk = P.div(nxt, st["rho"]); st["rho"] = nxt                 # :533-534
        d = (bk * d + s).astype(dtype)                              # :536-537
    ret, t = _loop(P, st, step, para, n, progress)
    return {"ret": ret, "iters": t, "x": st["m"], "residual": float(st["residual"])}


def solver(sid, *args, **kw):
    """clcg_solver_cuda's dispatch (:42-60): the id first, then the loop's own argument checks."""
    if sid not in (CLCG_BICG, CLCG_BICG_SYM):
        return {"ret": CLCG_UNKNOWN_SOLVER}
    return bicg(*args, **kw) if sid == CLCG_BICG else bicg_sym(*args, **kw)


# ---- operators on host CSR arrays -------------------------------------------------------------------------------------
def csr_ops(rp, ci, v, dtype=np.complex64):
    """ax, ahx, at_x, conj_x in complex128 on the values rounded to `dtype` (exact sums of the rounded inputs, then the caller
    rounds).  Built on scipy.sparse."""
    import scipy.sparse as sp
    n = len(rp) - 1
    A = sp.csr_matrix((np.asarray(v, dtype).astype(np.complex128), ci, rp), shape=(n, n))
    AH = A.conj().T.tocsr(); AT = A.T.tocsr(); AC = A.conj().tocsr()

    def f(M):
        return lambda x: M @ np.asarray(x).astype(np.complex128)
    return {"A": f(A), "AH": f(AH), "AT": f(AT), "conj": f(AC), "matrix": A}


def jacobi(rp, ci, v, dtype=np.complex64):
    """z = x * (1 / diag) in the working precision (the reciprocal by cuCdivf's formula, as the device computes it)."""
    P = Prec(dtype)
    n = len(rp) - 1
    d = np.zeros(n, dtype)
    for i in range(n):
        for k in range(rp[i], rp[i + 1]):
            if ci[k] == i:
                d[i] = v[k]
                break
    inv = np.array([P.div(P.C(1.0), P.C(x)) for x in d], dtype)
    return lambda x: (inv * np.asarray(x, dtype)).astype(dtype)
