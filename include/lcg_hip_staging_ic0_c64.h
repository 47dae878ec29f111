/*
 * lcg_hip_staging_ic0_c64.h -- the batched complex64 IC(0) entries of liblcg_hip.so, waiting for their place in lcg_hip.h.
 *
 * The rule is lcg_hip_staging.h's: every entry that lcg_hip.h declares has a line in the stream-coverage table of the test suite
 * (tests/stream_cases.py), and a feature pull request does not edit existing tests, so an entry that such a pull request adds is
 * declared outside lcg_hip.h, with its full contract, exported by the library and bound by the Python front like any other; the test
 * pull request that gives it its table line moves its declaration, word for word, into lcg_hip.h.
 *
 * Why a file of its own: the suite also pins lcg_hip_staging.h to the names it held when its own test was written
 * (tests/test_multi_cbicg_cases_cpu.py compares that header, liblcg_amd._lib.STAGING_SIGNATURES and a fixed list), so a further
 * staged entry cannot join that file without editing that test.  These two are bound in liblcg_amd._lib.STAGING_IC0_C64_SIGNATURES.
 * Nothing else distinguishes them: the ABI rules, codes, memory convention and types are lcg_hip.h's.
 */
#ifndef LCG_HIP_STAGING_IC0_C64_H
#define LCG_HIP_STAGING_IC0_C64_H

#include "lcg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The handle's complex64 IC(0) factor (lcg_hip_csr_build_ic0_c64) applied to a block of k = 2, 4 or 8 complex64 vectors
 * (clcg_hip_spmm_c64's layout: n x k interleaved (re, im) float pairs, row-major, the base 16-byte aligned): which = 0 L^-1, 1 L^-T
 * (unconjugated: M = L.L^T is complex-symmetric), 2 both.  The apply follows lcg_hip_csr_ic0_set_sweeps: exact level-scheduled
 * solves, or s Jacobi sweeps per triangle, each sweep ONE launch that reads the triangle once for all k columns.  Column j has the
 * bits of lcg_hip_ic0_solve_c64 on column j alone -- one fp32 accumulator from x_i, the products subtracted in column order, one
 * scaled division by the stored diagonal -- whatever the other columns hold (NaN and Inf included), whatever k is, wherever the
 * column stands, from call to call.  The k-wide work vectors belong to the factor (8 bytes per element and column): the first call
 * at a k larger than any before may allocate and wait, later ones only launch; lcg_hip_csr_ic0_info's byte count includes them.
 * LCG_HIP_E_ARG (lcg_hip_last_error() says why), checked in this order before the device is touched, Y untouched: k not 2, 4 or 8;
 * a null or misaligned block; a real / complex128 / dense / sharded handle; no complex64 factor; which outside 0..2; X and Y
 * overlapping. */
int clcg_hip_ic0_solve_multi_c64(lcg_hip_csr_t A, int k, int which, const float *X, float *Y);
/* clcg_hip_lpcg_multi_c64 with the preconditioner named.  LCG_HIP_M_JACOBI is clcg_hip_lpcg_multi_c64 itself, bit for bit.
 * LCG_HIP_M_IC0 applies the handle's complex64 IC(0) factor k wide at its sweeps setting -- clcg_hip_solver_preconditioned_c64 with
 * clcg_hip_ic0_mx_c64 as MxProduct, per column -- between the update pass and a pass of the sums (one apply per iteration for all
 * columns; its launches count as vector passes in lcg_hip_last_launches):
 *     A.d carrying d.Ad | [ak] m += ak d; r -= ak Ad | s = (L.L^T)^-1 r | sums |m|^2, |r|^2, r.s | [close] d = s + bk d
 * Precision rule, stop rule, "already optimised", the NaN stop, per-column freezing, codes and counts are clcg_hip_lpcg_multi_c64's.
 * A column that has stopped is final in M, r and d; the apply's output s is scratch and is formed for every column.
 * LCG_HIP_M_ILU0 (there is no complex64 ILU(0)), LCG_HIP_M_NONE and any other precond: LCG_HIP_E_ARG, the text names precond.  No
 * complex64 factor, or no Jacobi diagonal: LCG_NULL_PRECONDITION_MATRIX, nothing run, ret[] untouched.  The other refusals, in
 * clcg_hip_lpcg_multi_c64's order: LCG_HIP_E_ARG (k, null or misaligned M / B, a real / complex128 / dense / sharded / non-square
 * handle, mem; before the device is touched), CLCG_INVILAD_MAX_ITERATIONS, CLCG_INVILAD_EPSILON.  Column j's iterate, count, residual
 * and code depend on A, its factor and sweeps setting, column j of B and M and param alone, bit for bit: whatever the other columns
 * hold, whatever k is, wherever the column stands, from call to call. */
int clcg_hip_lpcg_multi_m_c64(lcg_hip_csr_t A, int k, int precond, float *M, const float *B, const clcg_para *param,
                              int *ret, int *iterations, double *residual, int mem);

#ifdef __cplusplus
}
#endif
#endif /* LCG_HIP_STAGING_IC0_C64_H */
