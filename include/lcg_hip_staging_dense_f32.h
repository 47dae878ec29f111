/*
 * lcg_hip_staging_dense_f32.h -- real dense operators stored in fp32: the entries of liblcg_hip.so that make such a handle and tell
 * the element widths apart, waiting for their place in lcg_hip.h.
 *
 * The rule is lcg_hip_staging.h's: every entry that lcg_hip.h declares has a line in the stream-coverage table of the test suite
 * (tests/stream_cases.py), and a feature pull request does not edit existing tests, so an entry that such a pull request adds is
 * declared outside lcg_hip.h, with its full contract, exported by the library and bound by the Python front like any other; the test
 * pull request that gives it its table line (tests/dense_f32_cases.py holds the lines ready) moves its declaration, word for word,
 * into lcg_hip.h -- it moves into lcg_hip.h with its stream-coverage line.
 *
 * Why a file of its own: the suite pins the earlier staging headers to the names they held when their own tests were written, so a
 * further staged entry cannot join any of them without editing those tests.  These entries are bound in
 * liblcg_amd._lib.STAGING_DENSE_F32_SIGNATURES.  Nothing else distinguishes them: the ABI rules, codes, memory convention and types
 * are lcg_hip.h's.
 *
 * The workload.  For a dense operator the matrix is the whole cost of an iteration, and sensitivity kernels of gravity, magnetic and
 * integral-equation problems are computed in single precision or to single-precision accuracy; widened to fp64 for
 * lcg_hip_dense_create they cost 8 bytes per entry in every product.  An fp32 handle keeps K at 4 bytes per entry and does everything
 * else in fp64: vectors, sums, tables, reciprocals and solver state are a real fp64 handle's, and no signature changes.
 *
 * The contract, in one sentence: an fp32 handle is the fp64 handle of the widened matrix -- (double)val[i * ld + j], an exact
 * conversion, subnormals included -- and gives the same bits.  That holds for every entry below the create, under the automatic
 * choice of kernels and under every variant lcg_hip_dense_set_kernel forces, because the kernels differ only in how a pack of two
 * columns arrives (8 bytes widened in registers instead of 16) and the plans are functions of the shape and the forced variant alone,
 * never of the element width.
 *
 * Which entries serve it: every entry that serves a real fp64 dense handle, with unchanged signatures -- lcg_hip_dense_matvec (both
 * layouts), lcg_hip_dense_ata (two-pass, one-pass and one-workgroup forms), the callbacks lcg_hip_dense_ata_ax, lcg_hip_dense_ax
 * and lcg_hip_dense_jacobi_mx, lcg_hip_dense_build_jacobi (both `normal` values), lcg_hip_dense_set_kernel, _last_kernel, _rows,
 * _cols and _destroy, lcg_hip_dense_matmat, _ata_multi, _op_multi_dot and _multi_last_kernel, lcg_hip_dense_lcg_multi and
 * _lpcg_multi, lcg_hip_dense_solver_constrained_multi.  The kernel names they report are the fp64 handle's.  The complex entries and
 * the _c64 entries refuse it exactly as they refuse a real fp64 handle; there is no lcg_hip_dense_create_rows for fp32.
 */
#ifndef LCG_HIP_STAGING_DENSE_F32_H
#define LCG_HIP_STAGING_DENSE_F32_H

#include "lcg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An M x N real matrix resident in HBM as fp32.  val: row-major floats, row i at val + i * ld (ld >= N), living where `mem` says; it
 * is copied, by a pack kernel on the device.  The checks and codes are lcg_hip_dense_create's: LCG_HIP_E_ARG for a NULL handle pointer
 * or val, M or N not positive, ld < N, a mem that is neither LCG_HIP_MEM_HOST nor LCG_HIP_MEM_DEVICE (all before the device is
 * touched, *K set to NULL), LCG_HIP_E_NO_DEVICE where there is none.  Storage: the fp64 handle's geometry at half the bytes -- rows
 * padded to whole 8-byte packs (columns 2p and 2p + 1), ceil(N / 2) packs per row, pads zero, 64 bytes of slack: 4 bytes per entry.
 * Memory: a source on the host passes through a device staging buffer of at most 256 MiB, a run of rows at a time, freed before the
 * call returns; a source on the device is read in place.  The call drains the stream. */
int lcg_hip_dense_create_f32(lcg_hip_dense_t *K, int m_rows, int n_cols, const float *val, int64_t ld, int mem);

/* Bytes per stored entry of K: 4 (lcg_hip_dense_create_f32), 8 (a real fp64 handle; a complex64 one, a float pair) or 16
 * (complex128).  A query answered on the host for every dense handle; LCG_HIP_E_ARG for anything else. */
int lcg_hip_dense_value_bytes(lcg_hip_dense_t K);

#ifdef __cplusplus
}
#endif
#endif /* LCG_HIP_STAGING_DENSE_F32_H */
