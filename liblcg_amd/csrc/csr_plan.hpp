// csr_plan.hpp -- what csr.hip (the row-block kernels, the dispatch, the handle's C ABI) and csr_choice.hip (which kernel family a
// matrix, or a stretch of its rows, gets) share.  Not installed.
#pragma once

#include <chrono>
#include <string>
#include <vector>

#include "devcommon.hpp"

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
// csr_sym.hip: the symmetric run stretch of a part's packed plan
bool sym_runs_wanted(const CsrPart &P);                     // the mode, the part and (automatic mode) its size ask for one
void sym_runs_build(const CsrPart &P, hipStream_t s);       // from the part's run stretches (csr.hip: run_stretches_build), once per plan
inline bool sym_runs_in_use(const CsrPart &P) { return P.pk_state == 1 && P.pk_sym.NX > 0; }
int64_t sym_runs_bytes(const CsrPart &P);                   // the half store
int sym_group_in_use(const CsrPart &P);                     // consecutive blocks per XCD its kernel's workgroups are dealt in: 1, 2, 4 or 8 (one slice only)
// y = A.x for the rows of the sliced range; the other blocks are the caller's (csr.hip: ldsp_launch)
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

// csr.hip
template <class V> struct LdsCfg { static constexpr int CH = sizeof(V) == 8 ? 2240 : 1344; };      // entries of the largest LDS window
void launch_max_slice(int n, int R, const int *rowptr, int *out, hipStream_t s);     // out[0] = max over blocks of R rows of their entries (atomicMax; zero it first)

} // namespace lcgh
