// csr_plan.hpp -- what csr.hip (the plain row-block kernels, the choice and dispatch, the handle's C ABI), csr_packed.hip (the packed
// row-block product: its plan, its kernels, its setters), csr_sym.hip (the plan's symmetric run stretch) and csr_choice.hip (which
// kernel family a matrix, or a stretch of its rows, gets) share.  Not installed.
#pragma once

#include <chrono>
#include <string>
#include <type_traits>
#include <vector>

#include "devcommon.hpp"
#include "csr_sym.hpp"

namespace lcgh {

constexpr int PK_R = 64;            // rows per block of the packed form and of every per-block statistic

struct PlanTimer {      // adds the host time of a build (it ends on a drained stream) to the part's plan_ms
    const CsrPart &P; hipStream_t s; std::chrono::steady_clock::time_point t0;
    PlanTimer(const CsrPart &p, hipStream_t st) : P(p), s(st), t0(std::chrono::steady_clock::now()) {}
    ~PlanTimer() { (void)hipStreamSynchronize(s); P.plan_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

struct RangePlan {
    std::vector<CsrPart> parts;
    std::vector<int> r0;            // first row of each range
    std::vector<const char *> seen; // last_kernel of each range when `desc` was composed
    std::string desc;
};

// csr_choice.hip: true when P's products go through that format (statistics measured and plan built on first use)
bool binned_chosen(const CsrPart &P, hipStream_t s);
bool tiled_chosen(const CsrPart &P, hipStream_t s);
bool ranges_chosen(const CsrPart &P, hipStream_t s);
void ranges_free(const CsrPart &P);
void long_rows_free(const CsrPart &P);
int long_rows_launch(const CsrPart &P, const double *x, double *y, hipStream_t s, const int *done);

// ---- the packed row-block product (csr_packed.hip: k_spmv_ldsp, k_spmv_run1 / k_spmv_run1d) --------------------------------------
// What one build produces (packed_build), owned by the part through CsrPart::pk_plan: there from the first build on, its memory
// released by packed_free and by nothing else (the numbers of a released plan stay until the next build or the part's end).
struct PackedPlan {
    int *base = nullptr, *ofs = nullptr;    // per block of R rows: smallest column (or the block's form: k_pk_meta), first group
    void *data = nullptr;                   // 16 bytes per group of 6 / 7 packed columns (run blocks: row 0's columns, template blocks: offsets and masks)
    int maxrow = 0;                         // longest row (chooses the gather batch of the kernel)
    int bits = 21;                          // width of a packed column: 18 (seven per group) or 21 (six)
    int R = PK_R;                           // rows per block (64; 32 / 16 for long rows)
    int dof = 1;                            // long rows: every row's entries come in groups of dof consecutive columns (one packed field per group)
    int runs = 0, tpls = 0;                 // blocks stored as runs (row 0's columns only) / as templates (<= 64 diagonals + a mask per row)
    long groups = 0;                        // 16-byte groups of `data`
    RunStretches rs;                        // the (up to four) longest stretches of run blocks
    int *rs_off = nullptr;                  // their offset tables
    long rs_blocks = 0, rs_groups = 0;      // blocks they cover; 16-byte groups of per-block columns those blocks no longer read
    SymRun sym;                             // symmetric run stretch (csr_sym.hip): NX = 0: none
    double *sym_H = nullptr;                // its half store
    long sym_tiles = 0;                     // and that store's tiles
};
inline PackedPlan *packed_plan(const CsrPart &P) { return static_cast<PackedPlan *>(P.pk_plan); }

// What one part's A.x runs (csr.hip: ax_choose): the kernel family and its template arguments
enum class Ax { none, long_rows, ranges, binned, tiled, run1, ldsp, ldsp_long, lds1, ldsw, wave };
struct AxChoice {
    Ax family = Ax::none;
    int R = 0, T = 0;               // rows per block (the LDS-staged families), lanes per row (k_spmv_wave)
    int ns = 0, bits = 0, win = 0;  // k_spmv_ldsp: gathers per lane in the first batch, bits per column; LDS window (+ k_spmv_lds1)
    bool onewin = false;            // every block's slice fits the largest window
};

// csr_packed.hip.  Build the packed columns of P once (device; two short synchronisations); true when a plan of that kind (runs only:
// pk_state 2, for k_spmv_run1; else pk_state 1 with R rows per block) is ready.  One-shot: a part that failed stays at pk_state -1.
bool packed_build(const CsrPart &P, hipStream_t s, bool runs_only, int R = PK_R);
inline bool packed_ready(const CsrPart &P, hipStream_t s, int R = PK_R) { return packed_build(P, s, false, R); }
// (packed_free, which releases it: internal.hpp -- comm.hip calls it too)
// what ax_choose asks of a plan that is ready
int packed_maxrow(const CsrPart &P);
int packed_bits(const CsrPart &P);
int ldsp_ns(const CsrPart &P, int R);       // k_spmv_ldsp's gathers per lane in its first batch
int pk_window(int max_slice);               // the smallest instantiated LDS window (entries) that holds max_slice
// The launches: each names what it ran in P.last_kernel and returns 0 or a failure's code (< 0).
// pp: a shard's pushing blocks ride in front of the grid (64 rows per block only).
int packed_run1_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, hipStream_t s, const int *done);
int packed_ldsp_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, hipStream_t s, const int *done, const PushPlan *pp);
int packed_ldsp_long_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, hipStream_t s, const int *done);
// carrying the dot.  run1d: 1 = launched, *slots sums wait in part; 0 = rows too long or too many workgroups for it, nothing launched.
int packed_run1d_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, const double *u, int yy, double *part, int *slots,
                        hipStream_t s, const int *done);
// ldsp: 1 = launched, *nsum per-block sums wait in P.dot_part (dot_part_fold); 0 = no memory for them, nothing launched
int packed_ldsp_dot_launch(const CsrPart &P, const AxChoice &c, const double *x, double *y, const double *u, int yy, int *nsum, hipStream_t s,
                           const int *done, const PushPlan *pp);
// the <= 512-way second stage of a product's nsum sums in P.dot_part (the tiled product's too): part[0 .. *slots), y.y from part[AXP_CAP]
int dot_part_fold(const CsrPart &P, int nsum, int yy, double *part, int *slots, hipStream_t s, const int *done);
int64_t packed_traffic_bytes(const CsrPart &P, const char *kernel_name);    // the matrix's side of what the named product of this family reads (row pointers, x, y: the caller's)
int64_t packed_plan_bytes(const CsrPart &P);                                // the plan, the stretches' tables and the half store
// csr.hip
bool ensure_dot_part(const CsrPart &P, long count);     // P.dot_part holds 2 * count sums (shared with the tiled product)
void op_copies_free(lcg_hip_csr *A);                    // first half of the rewrite protocol: every setter's (A, 0)

// csr_sym.hip: the symmetric run stretch of a part's packed plan
bool sym_runs_wanted(const CsrPart &P);                     // the mode, the part and (automatic mode) its size ask for one
void sym_runs_build(const CsrPart &P, hipStream_t s);       // from the plan's run stretches (csr_packed.hip: run_stretches_build), once per plan
inline bool sym_runs_in_use(const CsrPart &P) { return P.pk_state == 1 && packed_plan(P)->sym.NX > 0; }
int64_t sym_runs_bytes(const CsrPart &P);                   // the half store (0: none, or no plan)
int sym_group_in_use(const CsrPart &P);                     // consecutive blocks per XCD its kernel's workgroups are dealt in: 1, 2, 4 or 8 (one slice only)
// y = A.x for the rows of the sliced range; the other blocks are the caller's (csr_packed.hip: ldsp_launch)
void sym_runs_launch(const CsrPart &P, bool dot, const double *x, double *y, hipStream_t s, const int *done, const DotPlan &dp);

// end of a block of a product that carries its dot (k_spmv_ldsp<DOT>, k_spmv_ldsp_sym<DOT>): the first wavefront holds the finished rows
// (vfin) and their u; one sum per block
__device__ __forceinline__ void ldsp_dot_tail(const DotPlan &dp, int bid, int j0, double vfin, double uv)
{
    if (threadIdx.x >= 64) return;      // uniform per wavefront: the finished rows sit in wavefront 0 (all of it at 64 rows per block,
    if (j0 != 0) vfin = 0.0;            // its first 32 / 16 lanes at 32 / 16 -- the other lanes add zeros)
    const double a0 = wave_sum(vfin * uv);
    if ((threadIdx.x & 63) == WSUM_LANE) dp.part[bid] = a0;
    if (dp.yy) {                        // uniform
        const double a1 = wave_sum(vfin * vfin);
        if ((threadIdx.x & 63) == WSUM_LANE) dp.part[dp.stride + bid] = a1;
    }
}

// the LDS-staged kernels of csr.hip and csr_packed.hip
// native vector types: arrays of these stay in registers (arrays of HIP's struct-wrapped int4 /
// double2 were demoted to scratch here: 2x slower)
typedef int v4i __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));
template <class V> struct LdsCfg { static constexpr int CH = sizeof(V) == 8 ? 2240 : 1344; };      // entries of the largest LDS window
// the smaller windows (pk_window; why these: the comment above k_spmv_ldsp, csr_packed.hip)
constexpr int PK_CH_SMALL = 2208;
constexpr int PK_CH_7 = 1872, PK_CH_8 = 1696;
// f(std::integral_constant<int, V>()) for the V of Vs that equals v (false: none does).  Only the listed values are instantiated:
// the lists at the launches name exactly the template arguments their kernels are built for.
template <int... Vs, class F> static bool pick(int v, F &&f) { return ((v == Vs ? (f(std::integral_constant<int, Vs>()), true) : false) || ...); }
// csr.hip
void launch_max_slice(int n, int R, const int *rowptr, int *out, hipStream_t s);     // out[0] = max over blocks of R rows of their entries (atomicMax; zero it first)

} // namespace lcgh
