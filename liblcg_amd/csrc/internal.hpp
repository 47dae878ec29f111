// internal.hpp -- shared declarations of liblcg_hip (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "lcg_hip.h"
#include "pool.hpp"

namespace lcgh {

// Run-time switches: the library reads the documented ones only ("Run-time switches").
// LCG_HIP_DEBUG=1: the plan builders, the placement of the product's output and the direct exchange say on stderr what they chose and
// why; 2: a solve also synchronises after every launch and names it (fault isolation)
inline int debug_level()
{
    static const int lv = [] { const char *e = std::getenv("LCG_HIP_DEBUG"); return e ? atoi(e) : 0; }();
    return lv;
}
inline bool debug_on() { return debug_level() != 0; }


constexpr int VB = 256;     // threads per block of every vector / scalar kernel
constexpr int MAXG = 2048;  // most blocks a reducing kernel launches = stride of the partial-sum table
constexpr int MAXR = 8;     // most simultaneous reductions of one kernel

enum { ST_RUNNING = 0, ST_CONVERGED = 1, ST_NAN = 2, ST_ALREADY = 3, ST_COMM = 4 };

// Direct all-reduce over peer-mapped mailboxes (comm.hip, "direct all-reduce").  Handed by value to
// the scalar kernel; all pointers are device addresses valid on THIS rank.
constexpr int XG_SLOT = 16;     // doubles per (parity, source) slot: MAXR values + the sequence word, 128 B
constexpr int XG_MAXP = 64;     // most ranks (one lane of one wavefront per peer)
struct XgBox {
    double *mine = nullptr;             // my mailbox [2][P][XG_SLOT], uncached/fine-grained device memory
    double *const *peers = nullptr;     // [P]: every rank's mailbox as mapped into this process (peers[me] == mine)
    unsigned long long *seq = nullptr;  // all-reduces issued so far (advanced by the kernel itself)
    int *fail = nullptr;                // raised when a peer's contribution did not arrive in time
    long long timeout_ticks = 0;        // wall_clock64 ticks (100 MHz)
    int P = 0, me = 0;
};

// Direct neighbour exchange (comm.hip, dist mode 2): the rank that OWNS a piece of x writes it into
// the neighbours' receive buffers over the peer mappings and then raises a flag word there; the
// neighbour's remote-column product waits for the flags of the call it belongs to.
constexpr int XG_MAXSEG = 8;        // most neighbours of a rank under this mode
constexpr int PUSH_CHUNK = 4096;    // doubles one pushing block moves
struct DevState;
struct WaitPlan {
    int n = 0;
    unsigned long long seq = 0;
    long long timeout_ticks = 0;
    int *fail = nullptr;
    const unsigned long long *flag[XG_MAXSEG];  // the neighbours' flag words in MY flag array
};
struct PushPlan {
    int nseg = 0, nflag = 0, nblocks = 0;
    unsigned long long seq = 0;         // number of this A.x call (same on every rank)
    unsigned int *ticket = nullptr;     // blocks finished so far (the last one raises the flags)
    const double *src[XG_MAXSEG];
    double *dst[XG_MAXSEG];             // peer memory
    long count[XG_MAXSEG];              // doubles
    int first_block[XG_MAXSEG + 1];
    unsigned long long *flag[XG_MAXSEG];        // my flag word in each neighbour's flag array
    // RECEIVING blocks behind the product's blocks (one-stream direct exchange): block j of them waits for the neighbours' flags of
    // this call and copies chunk j of what they wrote from the landing zone into the gather buffer -- k_recv's work without its
    // launch, overlapped with the product's tail (devcommon.hpp: recv_block)
    int nrecv = 0, rnseg = 0;
    const double *rsrc[XG_MAXSEG];
    double *rdst[XG_MAXSEG];
    long rcount[XG_MAXSEG];
    int rfirst[XG_MAXSEG + 1];
    WaitPlan wp;
    DevState *rst = nullptr;            // where a time-out is recorded (may be null)
};


// Partial sums per running sum: slots 0 .. g[r]-1 of table row r hold the r-th sum's partials (one per block of the reducing
// pass).  One running sum (two with yy) may instead come from the epilogue of an A.x kernel that leaves one partial per
// workgroup -- up to AXP_CAP of them -- in a buffer of its own: ax_n entries at axp feed sum ax_row, those at axp + AXP_CAP feed
// sum ax_row + 1.  Everything is added in a fixed order: the same bits wherever and however often the reduction runs.
constexpr int AXP_CAP = 16384;
struct PartCount {
    int g[MAXR];
    const double *axp = nullptr;
    int ax_n = 0, ax_row = -1, ax_yy = 0;
    void all(int v) { for (int r = 0; r < MAXR; r++) g[r] = v; ax_row = -1; ax_n = 0; ax_yy = 0; }
};

// Sums an A.x kernel leaves beside y (one GPU, solver loops): workgroup w adds its rows' y_i * u_i into part[w] and, when yy is
// set, y_i * y_i into part[AXP_CAP + w] -- the dot that follows every A.x of the Krylov loops without its own pass over y.
struct DotPlan {
    const double *u = nullptr;
    double *part = nullptr;
    int yy = 0;
    int stride = AXP_CAP;   // distance of the y.y sums from the y.u sums in `part`
    int ux = 0;             // u is the product's own x (CG, PCG: d.Ad): a run block that holds its diagonal takes u from its gathers
    int dof = 1;            // k_spmv_ldsp, long rows: a packed column field stands for `dof` consecutive columns (csr_packed.hip: k_pk_dof)
};

// Stretches of run blocks (csr_packed.hip: k_pk_stretch / the stretch path of k_spmv_ldsp): consecutive full 64-row run blocks [b0, b1) with the
// same L, the same offsets column(row 0, k) - first row and entries that follow each other without a gap.  A block of a stretch
// derives everything it would load from the per-block plan from its number: it travels in the kernel arguments like the two plans above.
constexpr int RS_MAX = 4;
constexpr int RS_QMIN = 12;         // slots per wavefront a table holds at least: the largest first batch of k_spmv_ldsp reads them unconditionally
struct RunStretch {                 // 32 bytes: one scalar load
    int b0 = 0, b1 = 0;             // blocks [b0, b1) (an unused one is empty)
    int s0 = 0;                     // first entry of block b0
    int L = 0, kd = -1;             // entries per row; slot of the diagonal (offset 0) or -1
    int Q = 0;                      // the offset of slot k lies at off[(k % 4) * Q + k / 4]: wavefront w's slots w, w + 4, ... side by side (zeros behind the L-th)
    const int *off = nullptr;       // the table, one per stretch (device)
};
struct RunStretches {
    RunStretch s[RS_MAX];
    int n = 0;
};

struct DevState;

// Mirror of the stop state in host-mapped pinned memory; written by the scalar kernels,
// polled by the host without touching the stream.
struct HostStatus {
    volatile double residual;
    volatile int t;
    volatile int done;
    volatile int status;
    volatile int it;        // written last
};

// Everything the iteration carries between kernels.  Lives in device memory; kernels read
// their coefficients from here so no scalar ever has to visit the host inside the loop.
struct DevState {
    double red[MAXR];   // reduced sums of the latest reduction (all-reduce buffer when sharded)
    double s[32];       // solver scalars (indices: enum in each solver)
    double residual;    // value the next loop head tests (lcg.cpp:208-209)
    double eps;
    double n_global;
    int abs_diff;
    int it;             // iteration bodies started
    int t;              // completed iterations (the reference's t)
    int done;           // set once: every later kernel becomes a no-op
    int status;         // ST_*
    int pub_mask;       // HostStatus is refreshed when (it & pub_mask) == 0, and at every stop
    int zero_guess;     // the initial guess is all zeros (solvers_real.hip: ax_setup): its product is not made, A.m counts as zeros
    HostStatus *host;
};

struct Comm;            // comm.hip

struct Ctx {
    bool inited = false;
    int device = 0;
    hipStream_t stream = nullptr;      // stream in use
    hipStream_t own_stream = nullptr;  // created by the library
    hipStream_t comm_stream = nullptr; // second stream for gather/compute overlap
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    hipEvent_t ev_switch = nullptr;    // lcg_hip_set_stream: the new stream waits for the previous one's queue (made at the first switch)
    double *partials = nullptr;       // [MAXR][MAXG]: the table the latest reducing pass wrote (one of partials_pair)
    DevState *state = nullptr;         // the state the next kernel is handed (one of state_pair: driver.hpp, vecf)
    double *partials_pair[2] = {nullptr, nullptr};
    double *ax_partials = nullptr;     // [2][AXP_CAP]: the sums an A.x kernel carried (csr.hip: k_spmv_lds1d), see PartCount
    DevState *state_pair[2] = {nullptr, nullptr};
    HostStatus *hstat = nullptr;       // pinned, mapped
    HostStatus *hstat_dev = nullptr;   // device alias of hstat
    double *scratch_host = nullptr;    // pinned, 64 doubles
    DevState *snap[2] = {nullptr, nullptr};     // pinned, mapped: per-batch copies of DevState (sharded loop, driver.hpp)
    DevState *snap_dev[2] = {nullptr, nullptr}; // their device aliases (written by the batch's last scalar step)
    hipEvent_t snap_ev[2] = {nullptr, nullptr};
    Comm *comm = nullptr;
    int last_iters = 0;
    double last_residual = 0.0;
    bool in_solve = false;             // a Driver is alive: A.x may honour DevState::done
    const int *ax_skip = nullptr;      // the flag the NEXT built-in products honour instead of DevState::done (solvers_real.hip: ax_setup)
    int ax_rc = 0;                     // first failure of a built-in callback (void by liblcg's typedef) during this solve
    int cg_schedule = 0;               // LCG_HIP_CG_*
    bool profile = false;
    int profile_every = 1;             // time every k-th A.x only (each timed call costs ~2 x 2 us of markers)
    long ax_seq = 0;
    std::vector<hipEvent_t> prof_ev;   // pairs
    int prof_used = 0;
    double last_ax_mean_us = 0.0;
    int last_ax_calls = 0;
    int prof_pending = 0;              // events of the finished solve not yet turned into last_ax_mean_us (done on demand)
    DevState *state_stage = nullptr;   // pinned: the initial state of a solve on its way to the device (no stream sync)
    Pool pool;                         // the work vectors kept between solves (pool.hpp)
    PlaceState place;                  // where the product's output lies: memo, bounds, mode, reports (pool.hpp; the code: placement.hip)
    // what the latest solve enqueued: vector passes, scalar steps (a step that sums over ranks is one step, whatever it launches),
    // reductions over ranks (RCCL or mailboxes), products (lcg_hip_last_launches)
    int cnt_vec = 0, cnt_scal = 0, cnt_allreduce = 0, cnt_ax = 0;
    unsigned shadow_seed = 1;
    std::vector<double> shadow_vec;    // explicit rbar0 for the next complex solve
    std::string err;
};

Ctx &ctx();
int ensure_init();
// the flag a built-in product falls through on (null outside a solve)
inline const int *ax_flag(Ctx &c) { return c.ax_skip ? c.ax_skip : (c.in_solve ? &c.state->done : nullptr); }
int fail(hipError_t e, const char *what, const char *file, int line);
int arg_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));     // LCG_HIP_E_ARG, the text into the error string
int launched(const char *what);     // 0, or fail() with what the launches since the last look left in hipGetLastError()

#define HIPCHK(call)                                                        \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) return ::lcgh::fail(e_, #call, __FILE__, __LINE__); \
    } while (0)

// ---- CSR handle ------------------------------------------------------------------------
struct CsrPart {
    int n_rows = 0;
    int64_t nnz = 0;
    int *rowptr = nullptr;
    int *col = nullptr;
    double *val = nullptr;
    bool owned = false;
    bool padded = false;           // >= 64 readable bytes follow col[nnz] and val[nnz]
    mutable int slice_R = 0;       // rows per block the next field was computed for (0 = not yet)
    mutable int max_slice = 0;     // largest block slice, entries (csr.hip: k_max_slice)
    // packed column indices for the one-window kernel (csr_packed.hip), plan built on first use
    mutable int pk_mode = -1;      // -1 auto (large real matrices), 0 never, 1 whenever eligible
    mutable int pk_state = 0;      // 0 not tried, 1 ready, 2 ready for k_spmv_run1 only (run blocks' columns), -1 not eligible
    mutable void *pk_plan = nullptr;                        // csr_plan.hpp: PackedPlan, owned (packed_free)
    mutable int rs_mode = 0;                                // run stretches: 0 (default: measured slower) every run block loads its per-block plan, 1 the blocks of a stretch do not
    // symmetric run stretch (csr_sym.hip): the longest stretch whose values mirror each other bit for bit reads a half store
    mutable int sym_mode = -1;                              // -1 automatic (what the automatic mode takes), 0 off, 1 forced
    mutable int sym_nx = 0;                                 // slices of the sliced range: 0 the process's default, 1, 2, 4, 8
    bool sym_whole = false;                                 // the main part of a real fp64 handle while it is not sharded (set where the handle is made, cleared by lcg_hip_csr_distribute): no shard, no op(A) copy, no range
    mutable const char *sym_why = "not tried";              // why the stretch is (not) taken
    mutable double *dot_part = nullptr;                     // [2][dot_cap]: per-block (per-chunk) sums of a product that carries its dot (k_spmv_ldsp<DOT>, k_tile_spmv2<DOT>)
    mutable long dot_cap = 0;
    // two-pass "binned" product for scattered columns (csr_binned.hip), plan built on first use
    int64_t n_cols = 0;            // columns the part addresses (0 = unknown: never binned)
    mutable int bn_mode = -1;      // -1 auto (large real matrices whose row blocks span more of x than the L2 holds), 0 never, 1 whenever eligible
    mutable int bn_state = 0;      // 0 not tried, 1 plan ready, -1 not eligible / not chosen
    mutable void *bn_plan = nullptr;
    mutable const char *bn_why = "not tried";   // why the plan is (not) there
    mutable double mean_span = -1.0;    // mean column span of a 64-row block (-1 = not measured)
    mutable double line_ratio = -1.0;   // distinct 128-byte lines of x per entry of a 64-row block (-1 = not measured; csr_choice.hip: k_line_ratio)
    mutable double diag_like = -1.0;    // fraction of entries whose column is one more than the entry above them (-1 = not measured)
    // one-pass "tiled" product for row-random bands (csr_tiled.hip), plan built on first use
    mutable int tl_mode = -1;      // -1 auto, 0 never, 1 whenever eligible
    mutable int tl_state = 0;      // 0 not tried, 1 plan ready, -1 not eligible / not chosen
    mutable void *tl_plan = nullptr;
    mutable const char *tl_why = "not tried";
    // row ranges (csr_choice.hip, "row ranges"): a matrix whose row blocks fall into different column-pattern classes is multiplied range by
    // range, each range -- a view of this part's arrays -- choosing its own kernel family
    int64_t end_abs = -1;          // a view only: offset one past its last entry in the shared col / val (-1: this part owns offsets 0 .. nnz)
    mutable int rg_mode = -1;      // -1 auto (>= 4M entries), 0 never, 1 whenever two classes are found
    mutable int rg_state = 0;      // 0 not tried, 1 split, -1 one range
    mutable void *rg_plan = nullptr;
    int lr_mode = 0;               // a view only: 1 = rows far longer than an LDS window live here (csr_choice.hip: long_rows_launch)
    mutable void *lr_plan = nullptr;
    mutable const char *last_kernel = "";   // name of the kernel family the latest product used
    mutable double plan_ms = 0.0;           // host time spent choosing a kernel family and building its copy of the matrix (first product)
};

} // namespace lcgh

// Both kinds of handle begin with a word that says which kind they are (cleared when the handle is destroyed): an entry looks at
// that word and at nothing else of a handle of the other kind.
namespace lcgh {
constexpr uint64_t KIND_CSR = 0x3152534347434C4Cull, KIND_DENSE = 0x534E454447434C4Cull;
inline bool dense_handle(const void *h) { return h && *static_cast<const uint64_t *>(h) == KIND_DENSE; }
// a CSR entry handed a dense handle: LCG_HIP_E_ARG with the entry's name; `park` also ends a running solve (void callbacks)
inline int refuse_dense(const char *entry, bool park = false)
{
    ctx().err = std::string(entry) + ": the handle is a dense matrix (lcg_hip_dense_t); this entry takes a CSR matrix";
    if (park && !ctx().ax_rc) ctx().ax_rc = LCG_HIP_E_ARG;
    return LCG_HIP_E_ARG;
}
} // namespace lcgh
// first line of every exported entry that takes a lcg_hip_csr_t; the arguments after the handle are what the entry returns then
#define NOT_DENSE(h, ...) do { if (::lcgh::dense_handle(h)) { ::lcgh::refuse_dense(__func__); return __VA_ARGS__; } } while (0)
#define NOT_DENSE_CB(h) do { if (::lcgh::dense_handle(h)) { ::lcgh::refuse_dense(__func__, true); return; } } while (0)

namespace lcgh { struct TriFactor; }    // csr_tri.hpp
namespace lcgh { struct CsrNormal; }    // csr_normal.hpp
struct lcg_hip_csr {
    uint64_t kind = lcgh::KIND_CSR;
    int n_rows = 0;         // local rows
    int n_cols = 0;         // columns addressed by `main` (global when sharded)
    bool is_complex = false;
    lcgh::CsrPart main;     // the whole shard (global columns)
    lcgh::CsrPart op[4];    // [1] conj(A), [2] A^T, [3] A^H as their own CSR, built on first use (csr_build.hip: op_part)
    double *invdiag = nullptr;  // reciprocal diagonal (1 or 2 doubles per row)
    int variant = 0;        // SpMV kernel choice (0 auto)
    double mean_row = 0.0;
    // --- sharded operation (comm.hip) ---
    bool distributed = false;
    int dist_mode = 0;
    int64_t n_global = 0;
    int64_t row0 = 0;           // first global row of this shard
    int64_t rows_per_rank = 0;
    lcgh::CsrPart loc;          // entries whose column is owned by this rank (LOCAL column index)
    lcgh::CsrPart rem;          // the others (column index into xfull / halo buffer)
    lcgh::CsrPart remc;         // rem without its empty rows: own rowptr, rem's col/val (comm.hip: dist_split)
    int *rem_rows = nullptr;    // local row of each remc row
    double *rem_y = nullptr;    // remc . xfull, scattered into y after the local product
    double *xfull = nullptr;    // gather buffer
    double *op_z = nullptr;     // (A_r)^T . x_r over the padded global height, and one rows-per-rank block behind it (dist_spmv_op)
    void *halo = nullptr;       // neighbour-exchange plan (comm.hip)
    void *direct = nullptr;     // direct (peer-mapped) exchange state (comm.hip, mode 2)
    lcgh::TriFactor *ic0 = nullptr;     // incomplete-Cholesky factor L, L^T and their level schedules (csr_tri.hpp), copies: built by lcg_hip_csr_build_ic0
    lcgh::TriFactor *ilu0 = nullptr;    // incomplete-LU factor L, U and their level schedules (csr_tri.hpp), copies: built by lcg_hip_csr_build_ilu0
    // --- complex64 values (csr_c64.hip) ---
    bool c64 = false;           // main.val holds n_nnz interleaved (re, im) floats (8 B per entry); is_complex stays false
    void *c64p = nullptr;       // the products' plans and the Jacobi reciprocals of such a matrix (csr_c64.hip: C64Data)
    // --- the normal equations of a rectangular real matrix (csr_normal.hip) ---
    lcgh::CsrNormal *normal = nullptr;  // K^T as a CSR of its own, the vectors between the two products, the reciprocals of diag(K^T.K): built by lcg_hip_csr_build_normal
};

namespace lcgh {

// csr.hip
int spmv_launch(const CsrPart &P, bool is_complex, int variant, double mean_row, const double *x,
                double *y, bool accumulate, hipStream_t s, const int *done_flag);
// the same product with `pp.nblocks` pushing blocks in front of the grid (comm.hip, dist mode 2)
int spmv_launch_push(const CsrPart &P, bool is_complex, int variant, double mean_row, const double *x, double *y,
                     hipStream_t s, const int *done_flag, const PushPlan &pp);
// csr_packed.hip: everything a part's packed plan holds goes (stretch tables and half store included) and the part is "not tried"
// again -- the one place that releases it (the part's stream work must have ended).  part_goes: the part is being destroyed; otherwise
// the released plan's numbers stay readable for the status queries, as they always did
void packed_free(const CsrPart &P, bool part_goes = false);
void sym_runs_reset(CsrPart &P);            // csr_packed.hip: the half store goes and, where the part's mode wants one, its packed plan is built again at the next product
void sym_runs_free(const CsrPart &P);       // csr_sym.hip: the half store of a part's symmetric run stretch goes (the part's stream work must have ended)
int jacobi_launch(const lcg_hip_csr *A, const double *x, double *z, int n, hipStream_t s);       // csr_build.hip
// y = A.x with the sums y.u (and y.y) riding in the product: 1 = done, *slots partial sums wait in part[0 .. *slots) (and
// part[AXP_CAP ..)); 0 = this matrix / kernel family cannot (nothing was launched: the caller multiplies and reduces as before); < 0 failure
int csr_ax_dot(lcg_hip_csr *A, const double *x, double *y, const double *u, int yy, double *part, int *slots, hipStream_t s,
               const int *done_flag);
// the packed kernel of one part carrying y.u (and y.y), optionally with a shard's pushing blocks in front: 1 launched, 0 not this part
int csr_part_ax_dot(const CsrPart &P, int variant, double mean_row, const double *x, double *y, const double *u, int yy, double *part,
                    int *slots, hipStream_t s, const int *done_flag, const PushPlan *pp, int *nofold);
// csr_binned.hip
int binned_ready(const CsrPart &P, hipStream_t s);      // 1 plan ready, 0 not eligible, < 0 failure
int binned_launch(const CsrPart &P, const double *x, double *y, hipStream_t s, const int *done_flag);
void binned_free(CsrPart &P);
long binned_traffic_bytes(const CsrPart &P);
size_t binned_plan_bytes(const CsrPart &P);
// csr_tiled.hip
int tiled_ready(const CsrPart &P, hipStream_t s, double min_fill);      // 1 plan ready, 0 not eligible, < 0 failure
int tiled_launch(const CsrPart &P, const double *x, double *y, hipStream_t s, const int *done_flag, const PushPlan *push = nullptr,
                 const DotPlan *dot = nullptr);
int tiled_chunks(const CsrPart &P);         // chunks of 1024 rows = per-chunk sums a dot-carrying tiled product leaves
void tiled_free(CsrPart &P);
long tiled_traffic_bytes(const CsrPart &P);
long tiled_tile_copy_bytes(const CsrPart &P);
size_t tiled_plan_bytes(const CsrPart &P);
// csr_build.hip
int op_part(lcg_hip_csr *A, int layout, int conjugate, const CsrPart **out);
int alloc_part(CsrPart &P, int n_rows, long nnz, bool cplx);        // owned, padded arrays of a part
int device_exclusive_scan(int n, const int *counts, int *rowptr, hipStream_t s, long *total);
// T = S^T with sorted rows by k_tr_count / k_tr_fill / k_row_sort (op(A), the IC(0) factor's L^T); drains the stream
int transpose_launch(int n, int nt, long nnz, const int *rowptr, const int *col, const double *val, int *rpT, int *colT, double *valT,
                     bool cplx, int conj, int *cnt, hipStream_t s);
void row_sort_launch(int n, const int *rowptr, int *col, double *val, bool cplx, hipStream_t s);    // k_row_sort: by (column, value)
void perm_sort_launch(int n, const int *rowptr, int *perm, int longest, hipStream_t s);     // k_perm_sort: ascending, rows of at most `longest` entries
// csr_normal.hip
void normal_free(lcg_hip_csr *A);           // the normal state goes (lcg_hip_csr_destroy)
void normal_stale(lcg_hip_csr *A);          // the arrays may be rewritten (the set_*(A, 0) protocol): the state is rebuilt from them at its next use
// csr_tri.hip
void tri_factor_free(TriFactor *&F);                                 // an IC(0) / ILU(0) factor and everything it holds; F = nullptr
// csr.hip
void free_part(CsrPart &P);                                          // a part's arrays and every plan built beside them

// csr_c64.hip
void c64_free(lcg_hip_csr *A);
int c64_build_jacobi(lcg_hip_csr *A, void *diag_out);
const float *c64_builtin_invdiag(const void *Mfp, void *inst, int n);     // the reciprocals behind clcg_hip_jacobi_mx_c64 (else null)
// An entry that serves fp64 / complex128 matrices only, handed a complex64 one: LCG_HIP_E_ARG with lcg_hip_last_error() naming the
// entry (0: A may be used).  The bytes of such a matrix are never read as doubles.
inline int refuse_c64(const lcg_hip_csr *A, const char *entry)
{
    if (!A || !A->c64) return 0;
    ctx().err = std::string(entry) + ": the matrix holds complex64 values; this entry serves fp64 and complex128 matrices "
                "(complex64: lcg_hip_spmv_c64, clcg_hip_csr_ax_c64, clcg_hip_jacobi_mx_c64, lcg_hip_csr_build_ic0_c64, "
                "lcg_hip_ic0_solve_c64, clcg_hip_ic0_mx_c64)";
    return LCG_HIP_E_ARG;
}
#define TRY_C64(A, entry) do { int rc_ = ::lcgh::refuse_c64((A), (entry)); if (rc_) return rc_; } while (0)

// comm.hip
int comm_allreduce(double *dev, int count, hipStream_t s);
bool comm_active();
bool xg_box(XgBox *out);        // true when the direct all-reduce is connected and enabled
int dist_spmv(lcg_hip_csr *A, const double *x, double *y);
// the sharded product, carrying y.u where it can: the local product's partial sums (folded) followed by the remote-column kernel's, in
// part[0 .. *slots).  The product is ALWAYS made: 1 = with the sum, 2 = without it (the caller reduces in its own pass), < 0 failure
int dist_ax_dot(lcg_hip_csr *A, const double *x, double *y, const double *u, int yy, double *part, int *slots);
int dist_spmv_op(lcg_hip_csr *A, const CsrPart &T, const double *x, double *y);     // y = this rank's rows of A^T.x / A^H.x (T = (A_r)^T, csr_build.hip: op_part)

} // namespace lcgh
