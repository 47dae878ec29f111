/*
 * lcg_hip_staging.h -- entries of liblcg_hip.so that wait here for their place in lcg_hip.h.
 *
 * Every entry that lcg_hip.h declares has a line in the stream-coverage table of the test suite (tests/stream_cases.py), and a
 * feature pull request does not edit existing tests.  An entry that such a pull request adds is therefore declared here, with its full
 * contract, exported by the library and bound by the Python front (liblcg_amd._lib.STAGING_SIGNATURES) like any other; the test
 * pull request that gives it its table line moves its declaration, word for word, into lcg_hip.h and out of this file.  Nothing
 * else distinguishes a staged entry: the ABI rules, codes, memory convention and types are lcg_hip.h's.
 */
#ifndef LCG_HIP_STAGING_H
#define LCG_HIP_STAGING_H

#include "lcg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* clcg_hip_spmm carrying, per column, the CONJUGATED sum against ONE vector: dots[2 j], dots[2 j + 1] = re, im of the sum over i of
 * conj(u_i) (A.X)_ij, j < k (2k doubles on the host, after a stream synchronise) -- clcg_inner(rbar0, A.p), clcg.cpp:621, what the
 * batched BiCGStab takes after its first product.  u is one vector of n_rows complex elements (interleaved re, im) shared by all k
 * columns, not a block: the kernel reads it once per row, 16 bytes, not k x 16; its base 16-byte aligned.  Each element's product is
 * formed as the single-vector loops form it (re = u.re y.re + u.im y.im, im = u.re y.im - u.im y.re).  Y has the bits of
 * clcg_hip_spmm's in every case.  The sums ride in the product's epilogue as per-workgroup partial sums added in a fixed order:
 * column j's sum depends on A, X_j and u alone, bit for bit, whatever k is, wherever the column stands, whatever the other columns
 * hold (NaN and Inf included), from call to call.  Arguments and handles are checked as clcg_hip_spmm_dot's, before the device is
 * touched: LCG_HIP_E_ARG (lcg_hip_last_error() says why), Y untouched. */
int clcg_hip_spmm_inner(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *u, double *dots);
/* clcg_hip_spmm carrying, per column, the two sums the batched BiCGStab takes after its second product (t = A.s): dots3[2 j],
 * dots3[2 j + 1] = re, im of the sum over i of conj((A.X)_ij) U_ij -- clcg_inner(As, sk), clcg.cpp:631 -- and dots3[2 k + j] = the
 * sum over i of |(A.X)_ij|^2 -- clcg_inner(As, As), :632, real, carried as one sum -- j < k (3k doubles on the host, after a stream
 * synchronise).  U is a block like X and Y.  Products, the bits of Y, the order of the sums, what column j's sums depend on and the
 * checks: clcg_hip_spmm_inner's, with U_j in the place of u. */
int clcg_hip_spmm_dot2(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *U, double *dots3);
/* Batched complex BiCGStab (clbicgstab, clcg.cpp:524-679) over k = 2, 4 or 8 right-hand sides against one square complex128 CSR
 * matrix on one GPU, symmetric or not, Hermitian or not: no product with A^H is taken.  M (in/out) and B are blocks of k complex
 * vectors in clcg_hip_spmm's layout and live where `mem` says; layout, mem, ret / iterations / residual and "returns 0 when the loop
 * ran" are clcg_hip_lbicg_sym_multi's.  Each column runs the reference's recurrence as if it were alone: r = p = B - A.m,
 * rho = <rbar0, r> (conjugated: clcg_inner), both "already optimised" criteria in the reference's order, the 4th-power stop rule at
 * the loop head, (sum |r|^2)^2 / max((sum |m|^2)^2, 1), or sum |r|^2 / n with abs_diff, ak = rho / <rbar0, A.p>,
 * wk = <A.s, s> / <A.s, A.s>, the NaN scan of m after the update, betak = rho' ak / (rho wk), its own count and code:
 * CLCG_CONVERGENCE, LCG_REACHED_MAX_ITERATIONS (-1019, as the complex loops return at the cap), CLCG_ALREADY_OPTIMIZIED,
 * CLCG_NAN_VALUE, whose count is the iteration in which the NaN appeared (t after its t++).  A breakdown (<rbar0, A.p> = 0 or
 * A.s = 0) ends that column alone with CLCG_NAN_VALUE.
 * The shadow residual rbar0 is ONE vector of n for all columns: lcg_hip_set_shadow_vector's vector, consumed by this call, or the
 * draw from lcg_hip_set_shadow_seed -- what clcg_hip_solver(CLCG_BICGSTAB) takes, so column j of a batch and a single solve of
 * column j at the same seed see the same rbar0.  There is no redraw: the reference redraws while |rho| < 1e-8 and spins for ever on
 * r = 0; here, as in the single-vector loop, the "already optimised" tests come first and a zero column ends with
 * CLCG_ALREADY_OPTIMIZIED at count 0.
 * Schedule, precond = LCG_HIP_M_NONE: two products and three k-wide passes per iteration, every scalar step in the prologue of the
 * pass that consumes it,
 *     v = A.p carrying <rb,v> | [ak] s = r - ak v | t = A.s carrying <t,s>, |t|^2 | [wk] m += ak p + wk s; r = s - wk t + sums | [close] p = r + betak (p - wk v)
 * LCG_HIP_M_JACOBI (needs lcg_hip_csr_build_jacobi(A); without it LCG_NULL_PRECONDITION_MATRIX): right preconditioning carried in
 * x-space exactly as lcg_hip_lbicgstab_multi carries it, ph = p ./ diag and sh = s ./ diag written by the passes that write p and s
 * with the complex reciprocal diagonal, v = A.ph, t = A.sh, m += ak ph + wk sh; M holds the solution itself and nothing is applied
 * after the loop.  LCG_HIP_M_IC0, LCG_HIP_M_ILU0 and any other value: LCG_HIP_E_ARG (there are no k-wide complex applies).
 * A column that has stopped is final: its elements of M, r, p, s (ph, sh) are not stored to again, and one NaN column never keeps
 * a batch alive at max_iterations = 0.  Returns 0 when the loop ran, whatever the columns' verdicts; LCG_HIP_E_ARG (k, null or
 * misaligned M / B, a real / complex64 / dense / sharded / non-square handle, mem, precond; before the device is touched),
 * CLCG_INVILAD_MAX_ITERATIONS, CLCG_INVILAD_EPSILON, LCG_NULL_PRECONDITION_MATRIX, or a runtime failure.  No progress callback, no
 * caller workspaces; column j's iterate, count, residual and code depend on A, its diagonal, rbar0, column j of B and M and param
 * alone, bit for bit: whatever the other columns hold, whatever k is, wherever the column stands, from call to call. */
int clcg_hip_lbicgstab_multi(lcg_hip_csr_t A, int k, int precond, double *M, const double *B, const clcg_para *param,
                             int *ret, int *iterations, double *residual, int mem);

#ifdef __cplusplus
}
#endif
#endif /* LCG_HIP_STAGING_H */
