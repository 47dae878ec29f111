/*
 * lcg_hip_staging_box_multi.h -- the batched box-constrained entries of liblcg_hip.so, waiting for their place in lcg_hip.h.
 *
 * The rule is lcg_hip_staging.h's: every entry that lcg_hip.h declares has a line in the stream-coverage table of the test suite
 * (tests/stream_cases.py), and a feature pull request does not edit existing tests, so an entry that such a pull request adds is
 * declared outside lcg_hip.h, with its full contract, exported by the library and bound by the Python front like any other; the test
 * pull request that gives it its table line (tests/multi_box_cases.py holds the lines ready) moves its declaration, word for word,
 * into lcg_hip.h -- it moves into lcg_hip.h with its stream-coverage line.
 *
 * Why a file of its own: the suite pins lcg_hip_staging.h and lcg_hip_staging_ic0_c64.h to the names they held when their own tests
 * were written, so a further staged entry cannot join either file without editing those tests.  These two are bound in
 * liblcg_amd._lib.STAGING_BOX_MULTI_SIGNATURES.  Nothing else distinguishes them: the ABI rules, codes, memory convention and types
 * are lcg_hip.h's.
 */
#ifndef LCG_HIP_STAGING_BOX_MULTI_H
#define LCG_HIP_STAGING_BOX_MULTI_H

#include "lcg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lcg_solver_constrained (lcg_hip_solver_constrained) over k = 2, 4 or 8 right-hand sides against one real fp64 CSR matrix on one
 * GPU: solver_id LCG_SPG runs lspg (lcg.cpp:1224-1446), any other value lpg (lcg.cpp:1054-1204), as lcg_hip_solver_constrained
 * does.  k, the blocks M (in/out) and B, mem, ret / iterations / residual and "returns 0 when the loop ran, whatever the columns'
 * verdicts" are lcg_hip_lcg_multi's.  low, hig: ONE vector of n doubles each, shared by all k columns and read once per row, living
 * where `mem` says (no alignment asked); per-column bounds are out of scope.  products (host array of k, or NULL): products[j] is
 * the number of A.x calls the reference would have made for column j alone -- 1 for the set-up plus one per trial point -- final
 * once the column has stopped: what shows that a column took the reference's line-search path.
 *
 * Each column runs the reference's recurrence as if it were alone: the guess projected into the box, g = A.m - b, |m|^2 clamped
 * at 1, both "already optimised" criteria in the reference's order, the stop rule and the cap at the loop head, Barzilai-Borwein
 * steps s.s / s.y starting from param->step; SPG: d = P(m - lambda g) - m, trial points m + a d with a = 1, beta, beta^2, ... while
 * q(m + a d) > max(the last maxi_m accepted q) + sigma a g.d, with q = sum(0.5 m_i (A.m)_i - b_i m_i), the history slot
 * (t + 1) mod maxi_m, unused slots -1e30 and q of the projected guess in slot 0.  The loop is device resident: the host only
 * enqueues bodies, each one k-wide product of the pending trial points plus two k-wide passes; the line search's decision is taken
 * on the device per column, so columns drift apart in trial count and none is idle, and a column's count is its accepted steps.
 * The cap is per column, on the device.  All sums are binary trees over leaves that depend on n alone: column j's iterate, count,
 * products, residual and code depend on A, low, hig, column j of B and M and param alone, bit for bit -- whatever k is, wherever
 * the column stands, whatever the other columns hold (NaN and Inf included), from call to call.  A column that has stopped is
 * final: its column of M is not stored to again.
 *
 * Deviations from the reference:
 *  1. Breakdown.  The reference has no guard for s.y = 0: once an iterate stops moving (s = 0 at active bounds) it computes 0 / 0,
 *     fills m with NaN on the next iteration and runs to the cap.  Here a column whose new step s.s / s.y is not finite at the close
 *     of an accepted step ends there with LCG_NAN_VALUE, after the convergence test and the cap have had their turn; its count is
 *     that iteration, its iterate the last accepted one, finite and inside the box (the rule of clcg_hip_lbicgstab_multi).
 *  2. NaN sums.  A column whose |m|^2 or |g|^2 is NaN after an accepted step ends with LCG_NAN_VALUE where the reference would run
 *     on, so no column keeps a batch alive when max_iterations = 0.
 *  3. No progress callback: LCG_STOP never occurs.
 *
 * Refusals, in this order.  LCG_HIP_E_ARG before the device is touched, ret untouched, lcg_hip_last_error() says why: k not 2, 4
 * or 8; a null or misaligned M / B; a null low / hig; a complex / complex64 / dense / sharded / non-square handle; mem.  Then the
 * reference's parameter codes in its order -- lpg: LCG_INVILAD_MAX_ITERATIONS, LCG_INVILAD_EPSILON (epsilon <= 0),
 * LCG_INVALID_LAMBDA (step <= 0, and its quirk: epsilon >= 1); lspg: LCG_INVILAD_MAX_ITERATIONS, LCG_INVILAD_EPSILON,
 * LCG_INVALID_LAMBDA, LCG_INVALID_SIGMA, LCG_INVALID_BETA, LCG_INVALID_MAXIM.  Then lspg's maxi_m > 64: LCG_HIP_E_ARG (the history
 * lives in device memory sized for at most 64 slots per column). */
int lcg_hip_solver_constrained_multi(lcg_hip_csr_t A, int k, int solver_id, double *M, const double *B,
                                     const double *low, const double *hig, const lcg_para *param,
                                     int *ret, int *iterations, int *products, double *residual, int mem);
/* The same loop, contract and codes on a dense handle: A = K^T.K (normal = 1; n = N) or K (normal = 0, square), as
 * lcg_hip_dense_lcg_multi reaches them -- K is read once per product for all k columns.  LCG_HIP_E_ARG in the order above, with
 * the handle's refusals those of lcg_hip_dense_lcg_multi (not a real dense handle; normal = 0 on a K that is not square), then mem,
 * then normal neither 0 nor 1.  The product's launches are counted as lcg_hip_dense_lcg_multi counts them. */
int lcg_hip_dense_solver_constrained_multi(lcg_hip_dense_t K, int k, int normal, int solver_id, double *M, const double *B,
                                           const double *low, const double *hig, const lcg_para *param,
                                           int *ret, int *iterations, int *products, double *residual, int mem);

#ifdef __cplusplus
}
#endif
#endif /* LCG_HIP_STAGING_BOX_MULTI_H */
