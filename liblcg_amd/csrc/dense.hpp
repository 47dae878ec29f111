// dense.hpp -- what the dense units share (dense.hip: the single-vector products; dense_multi.hip: the k-wide kernels and their host
// flow for real and complex128 handles; dense_multi_cplx.hip: the complex entries; dense_c64.hip: everything of a complex64 handle):
// the handle and the plans of the row and column forms.  Not installed.
// DESIGN.md sections 14, 19, 20, 25 and 27.
#pragma once

#include <algorithm>

#include "internal.hpp"

namespace lcgh {
// what a handle owns for its k-wide products, sized for the largest k so far (dense_multi.hip: dnm_reserve)
struct DenseMulti {
    int kmax = 0;
    double *t = nullptr;        // the M x k block between the two products of K^T.(K.X) (real handles)
    double *part = nullptr;     // the k-wide slot table: k (complex handles: 2k) doubles per output row and slot
    const char *last_kernel = "";
};
}

struct lcg_hip_dense {
    uint64_t kind = lcgh::KIND_DENSE;   // internal.hpp: the word both kinds of handle begin with
    int M = 0, N = 0;
    bool cplx = false;
    bool c64 = false;           // the element type is complex64 (lcg_hip_dense_create_c64; cplx stays false): a pack is two (re, im) float pairs,
                                // part and invdiag hold floats, t is not allocated.  Served by dense_c64.hip's entries and by no other
    bool f32 = false;           // the entries are stored as fp32 (lcg_hip_dense_create_f32; cplx and c64 stay false): a pack is the 8 bytes of
                                // columns 2p and 2p + 1 and val points at float2; everything else is a real fp64 handle's and every entry for
                                // one serves it.  Looked at where a kernel is launched on val, nowhere else
    int64_t ldp = 0;            // packs per stored row
    int NP = 0;                 // packs that hold a row's entries: N (c128) or ceil(N / 2)
    double2 *val = nullptr;     // M * ldp packs + slack (f32: float2 packs, dn_val32)
    double *t = nullptr;        // the M-vector between the two products of K^T.K.x
    double *part = nullptr;     // the partial-sum table
    int64_t part_doubles = 0;
    double *invdiag = nullptr;  // N (or 2 N) doubles after lcg_hip_dense_build_jacobi (c64: N float pairs after lcg_hip_dense_build_jacobi_c64)
    int invdiag_normal = -1;    // which operator the reciprocals belong to: 1 K^T.K, 0 K (-1: none built)
    int variant = 0;
    const char *last_kernel = "";
    lcgh::DenseMulti *multi = nullptr;  // made by the first k-wide product (dense_multi.hip: dnm_reserve), freed with the handle
};

namespace lcgh {

enum { DN_AUTO = 0, DN_ROW = 1, DN_ROW_SPLIT = 2, DN_COL = 3, DN_ATA2 = 4, DN_ATA1 = 5, DN_ATA_SMALL = 6 };

static inline int pow2ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- plans (pure functions of the shape: the tables are sized from them) ----------------------------------------------------
struct RowPlan { int W, S, pps; };
struct ColPlan { int CW, CT, RS, rps; };

// strips of the row form: enough wavefronts for the chip when there are few rows (forced: also where the rows are short)
static inline RowPlan row_plan(int M, int NP, bool split, bool forced)
{
    RowPlan r;
    int S = 1;
    if (split) {
        const int cap = std::max(1, forced ? NP / 16 : NP / 256);
        S = std::min((int)cdiv(8192, M), cap);      // 8192 wavefronts: 32 per compute unit
    }
    r.pps = (int)cdiv(NP, S);
    r.S = (int)cdiv(NP, r.pps);
    r.W = std::min(64, std::max(4, pow2ceil(r.pps)));
    return r;
}
static inline bool row_split_auto(int M, int NP) { return M < 1024 && row_plan(M, NP, true, false).S >= 2; }

static inline ColPlan col_plan(int M, int NP)
{
    ColPlan c;
    c.CW = std::min(256, pow2ceil(NP));
    const int RG = 256 / c.CW;
    c.CT = (int)cdiv(NP, c.CW);
    const int rs_max = (int)cdiv(M, (int64_t)RG * 16);      // at least two batches of eight rows per thread
    const int RS = std::max(1, std::min((int)cdiv(1024, c.CT), rs_max));
    c.rps = (int)(cdiv(cdiv(M, RS), RG) * RG);
    c.RS = (int)cdiv(M, c.rps);
    return c;
}

// How a pack of K arrives: 16 bytes as they are, or (f32 handles) 8 bytes of two floats widened to the same double2 -- exactly, a
// float is a double.  The one seam between the element widths: everything after the load is the fp64 code, so an fp32 handle gives
// the bits of the fp64 handle of the widened matrix
__device__ __forceinline__ double2 ldpack(const double2 *p) { return *p; }
__device__ __forceinline__ double2 ldpack(const float2 *p) { const float2 v = *p; return make_double2((double)v.x, (double)v.y); }
static inline const float2 *dn_val32(const lcg_hip_dense *K) { return reinterpret_cast<const float2 *>(K->val); }

// doubles per element of K and of a block of vectors: the one place the complex factor 2 of the k-wide slot sizes comes from
static inline int dn_words(const lcg_hip_dense *K) { return K->cplx ? 2 : 1; }

// dense_multi.hip: the k-wide host flow, written once for real and complex128 handles (it branches on K->cplx)
void dnm_release(lcg_hip_dense *K);     // the k-wide work memory of a handle that goes (the caller has drained the device)
// a real (cplx: a complex128) dense handle, or nullptr with the entry's name and the reason in lcg_hip_last_error()
lcg_hip_dense *dnm_handle(const char *entry, const void *h, bool cplx = false);
// the handle's M x k block and k-wide slot table: the first call at a k larger than any before allocates and waits, later ones return
int dnm_reserve(lcg_hip_dense *K, int k);
// Y[M x k] = K.X and Y[N x k] = K^T.X (complex with conjugate: conj(K).X, K^H.X).  *launches grows by the kernels enqueued.  Checked
// handle, reserved k.
int dnm_row_product(lcg_hip_dense *K, int k, const double *X, double *Y, int conjugate, int variant, hipStream_t s, const int *done,
                    int *launches);
int dnm_col_product(lcg_hip_dense *K, int k, const double *X, double *Y, int conjugate, hipStream_t s, const int *done, int *launches);
// Y = (normal ? K^T.K : K).X for the k columns and, with U, column j's Y_j . U_j as *slots <= MM_MG partial sums: real at
// dots[j * MM_MG ...] (multi.hpp's table format), complex the UNCONJUGATED sum's re at dots[(2 j) * MM_MG ...] and im at
// dots[(2 j + 1) * MM_MG ...] (multi_cplx.hpp's), added in index order by msum.  *launches grows by the kernels enqueued.  Checked
// handle, reserved k; normal = 1 on real handles only.
int dnm_op(lcg_hip_dense *K, int k, int normal, const double *X, double *Y, hipStream_t s, const int *done, const double *U, double *dots,
           int *slots, int *launches);
// what the *_dense_op_multi_dot entries do after their checks: reserve, dnm_op, and with U and dots the read-out (multi_dots_read)
int dnm_op_dot_run(lcg_hip_dense *K, int k, int normal, const double *X, double *Y, const double *U, double *dots);
// y[j] = the sum of the table's S slots of n doubles each, in k_dnm_fold's fixed order.  The one fold of the dense units, type-blind:
// dense.hip's single-vector forms (done = nullptr) and the complex forms fold with it too
void dnm_fold_launch(const double *part, int S, int64_t n, double *y, hipStream_t s, const int *done);
// entry `index` of the k-wide kernel names of real (cplx: complex128) handles, or nullptr
const char *dnm_kernel_name(bool cplx, int index);
// LCG_HIP_E_ARG with the text every entry for real or complex128 dense handles answers a complex64 one with (the two places a dense
// handle's type is looked at: dense.hip's dense_of and dnm_handle)
int refuse_c64_dense(const char *entry);

// dense_c64.hip: the complex64 handle as the batched complex64 loops see it (solvers_multi_c64.hip)
// a complex64 dense handle, or nullptr with the entry's name and the reason in lcg_hip_last_error()
lcg_hip_dense *cdn_handle(const char *entry, const void *h);
// the handle's fp32 k-wide slot table, as dnm_reserve
int cdnm_reserve(lcg_hip_dense *K, int k);
// Y = K.X for the k complex64 columns and, with U, column j's UNCONJUGATED sum Y_j . U_j as *slots <= MM_MG partial sums in
// cspmm_c64_launch's table format (multi_c64.hpp).  *launches grows by the kernels enqueued.  Checked square handle, reserved k
int cdnm_op(lcg_hip_dense *K, int k, const float *X, float *Y, hipStream_t s, const int *done, const float *U, double *dots, int *slots,
            int *launches);

} // namespace lcgh
