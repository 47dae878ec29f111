/*
 * lcg_hip.h -- C ABI of liblcg_hip.so: an MI355X (gfx950) implementation of the
 * conjugate-gradient iteration hot path of liblcg, behind liblcg's own solver
 * entry points and callback types.
 *
 * Every entry point names the reference interface (path:line under
 * /root/reference/src/lib) it stands in for.  Plain C: opaque handles, POD
 * structs, raw pointers and sizes; no C++/torch types cross this boundary.
 * The C++ header include/lcg_dropin.hpp layers the reference's exact C++
 * signatures (default arguments, std::complex) over these symbols.
 *
 * Memory convention.  The iteration is device resident.  `mem` says where the
 * caller's m (in/out) and B (in) live:
 *   LCG_HIP_MEM_HOST   host pointers; copied in, solved on the GPU, m copied back
 *                      (the behaviour of lcg_solver_cuda, lcg_cuda.cu:103-111,210)
 *   LCG_HIP_MEM_DEVICE device pointers; nothing is copied.
 * Callbacks ALWAYS receive device pointers (as the reference's CUDA callbacks
 * do, lcg_cuda.h:45-46) and must enqueue their work on lcg_hip_get_stream()
 * without synchronising.  The progress callback receives the device m.
 *
 * All functions return 0 / a liblcg status code (util.h:69-90) unless noted;
 * LCG_HIP_E_* (<= -2000) report runtime failures (HIP/RCCL errors, missing GPU).
 * There is no CPU fallback: without a usable GPU every compute entry fails.
 */
#ifndef LCG_HIP_H
#define LCG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ types */

/* util.h:95-148 (bit-compatible, 64 bytes) */
typedef struct lcg_para {
    int    max_iterations;   /* 0 = until convergence */
    double epsilon;          /* in (0,1) */
    int    abs_diff;         /* 0: |g|^2/max(|m|^2,1)   1: |g|/N   (lcg.cpp:208-209) */
    double restart_epsilon;  /* unused by the solvers provided here */
    double step;
    double sigma;
    double beta;
    int    maxi_m;
} lcg_para;

/* util.h:247-273 (24 bytes) */
typedef struct clcg_para {
    int    max_iterations;
    double epsilon;
    int    abs_diff;         /* complex residual is |<r,r>|^2/max(|<m,m>|^2,1): clcg.cpp:295-296 */
} clcg_para;

/* util.h:32-64 (the reference's own type name; the entry points below take it as int) */
typedef enum lcg_solver_enum { LCG_CG = 0, LCG_PCG = 1, LCG_CGS = 2, LCG_BICGSTAB = 3, LCG_BICGSTAB2 = 4, LCG_PG = 5, LCG_SPG = 6 } lcg_solver_enum;
/* util.h:187-221 */
typedef enum clcg_solver_enum { CLCG_BICG = 0, CLCG_BICG_SYM = 1, CLCG_CGS = 2, CLCG_BICGSTAB = 3, CLCG_TFQMR = 4,
                                CLCG_PCG = 5, CLCG_PBICG = 6 } clcg_solver_enum;
/* util.h:69-90 */
enum {
    LCG_SUCCESS = 0, LCG_CONVERGENCE = 0, LCG_STOP = 1, LCG_ALREADY_OPTIMIZIED = 2,
    LCG_UNKNOWN_ERROR = -1024, LCG_INVILAD_VARIABLE_SIZE = -1023, LCG_INVILAD_MAX_ITERATIONS = -1022,
    LCG_INVILAD_EPSILON = -1021, LCG_INVILAD_RESTART_EPSILON = -1020,
    LCG_REACHED_MAX_ITERATIONS = -1019, LCG_NULL_PRECONDITION_MATRIX = -1018, LCG_NAN_VALUE = -1017,
    LCG_INVALID_POINTER = -1016, LCG_INVALID_LAMBDA = -1015, LCG_INVALID_SIGMA = -1014,
    LCG_INVALID_BETA = -1013, LCG_INVALID_MAXIM = -1012, LCG_SIZE_NOT_MATCH = -1011
};
/* util.h:226-242.  NB the complex loops return LCG_REACHED_MAX_ITERATIONS (-1019) and
 * LCG_ALREADY_OPTIMIZIED from the REAL enum (clcg.cpp:126,164); kept as is. */
enum {
    CLCG_SUCCESS = 0, CLCG_CONVERGENCE = 0, CLCG_STOP = 1, CLCG_ALREADY_OPTIMIZIED = 2,
    CLCG_UNKNOWN_ERROR = -1024, CLCG_INVILAD_VARIABLE_SIZE = -1023, CLCG_INVILAD_MAX_ITERATIONS = -1022,
    CLCG_INVILAD_EPSILON = -1021, CLCG_REACHED_MAX_ITERATIONS = -1020, CLCG_NAN_VALUE = -1019,
    CLCG_INVALID_POINTER = -1018, CLCG_SIZE_NOT_MATCH = -1017, CLCG_UNKNOWN_SOLVER = -1016
};
enum {
    LCG_HIP_E_RUNTIME = -2000,   /* a HIP call failed (lcg_hip_last_error() has the text) */
    LCG_HIP_E_NO_DEVICE = -2001, /* no usable gfx950 device */
    LCG_HIP_E_COMM = -2002,      /* RCCL missing or a collective failed */
    LCG_HIP_E_ARG = -2003        /* bad handle / argument to a non-solver entry */
};
enum { LCG_HIP_MEM_HOST = 0, LCG_HIP_MEM_DEVICE = 1 };

/* lcg.h:37-38.  x and prod_Ax are DEVICE pointers. Also the type of M^-1.x (lcg.h:90). */
typedef void (*lcg_axfunc_ptr)(void *instance, const double *x, double *prod_Ax, const int n_size);
/* lcg.h:53-54.  m is the DEVICE solution vector; non-zero return stops with LCG_STOP. */
typedef int (*lcg_progress_ptr)(void *instance, const double *m, const double converge,
                                const lcg_para *param, const int n_size, const int k);
/* clcg.h:40-41.  Complex vectors are interleaved (re,im) doubles == std::complex<double>.
 * layout: 0 MatNormal / 1 MatTranspose; conjugate: 0 NonConjugate / 1 Conjugate
 * (algebra.h:31-50).  The solvers here only ever pass (0,0), as clcg.cpp:463,474,620,630,707,759,771. */
typedef void (*clcg_hip_axfunc_ptr)(void *instance, const double *x, double *prod_Ax,
                                    const int n_size, int layout, int conjugate);
/* clcg.h:56-57 */
typedef int (*clcg_hip_progress_ptr)(void *instance, const double *m, const double converge,
                                     const clcg_para *param, const int n_size, const int k);

/* clcg_cudaf.h's callbacks with complex64 vectors: interleaved (re,im) floats == cuComplex == std::complex<float>.  x and
 * prod_Ax are DEVICE pointers; layout / conjugate as clcg_hip_axfunc_ptr (BiCG asks for A^H.x: layout 1, conjugate 1 --
 * CUSPARSE_OPERATION_CONJUGATE_TRANSPOSE, clcg_cudaf.cu:217).  Replaces clcg_axfunc_cudaf_ptr, whose cuSPARSE descriptors
 * do not cross this boundary. */
typedef void (*clcg_hip_axfunc_c64_ptr)(void *instance, const float *x, float *prod_Ax, const int n_size,
                                        int layout, int conjugate);
/* clcg_progress_cudaf_ptr: m is the DEVICE solution vector, converge the fp32 residual; non-zero stops with CLCG_STOP. */
typedef int (*clcg_hip_progress_c64_ptr)(void *instance, const float *m, const float converge,
                                         const clcg_para *param, const int n_size, const int k);

/* ------------------------------------------------------- runtime / stream */
int  lcg_hip_init(int device);                 /* selects the device; idempotent. */
/* lcg_hip_set_stream: NULL = the library's own stream.  Two rules:
 *   1. a stream other than the current one waits (one event, on the device: nothing is drained, the host does not wait) for
 *      everything the library has enqueued on the previous stream, so work enqueued after the switch never overtakes work
 *      enqueued before it -- the enqueue-only entries share scratch per handle and per context.  Setting the current stream
 *      again does nothing;
 *   2. the previous stream must still exist at the call: switch away from a stream BEFORE destroying it.
 * Work that OTHERS put on either stream is the caller's to order.  hip_stream is a stream the caller created (hipStreamCreate*);
 * the runtime's special handles hipStreamLegacy / hipStreamPerThread are not accepted (events cannot be recorded on them). */
int  lcg_hip_set_stream(void *hip_stream);
void *lcg_hip_get_stream(void);                /* stream callbacks must launch on */
int  lcg_hip_synchronize(void);   /* also where a timed-out direct exchange (multi-GPU) surfaces: LCG_HIP_E_COMM */
/* Blocking copy on the library stream.  kind: 1 host->device, 2 device->host, 3 device->device
 * (the cudaMemcpy calls of the reference's GPU samples, e.g. sample8.cu:160-166). */
int  lcg_hip_memcpy(void *dst, const void *src, uint64_t bytes, int kind);
const char *lcg_hip_last_error(void);
lcg_para  lcg_hip_default_parameters(void);    /* util.h:153,163 */
clcg_para clcg_hip_default_parameters(void);   /* util.h:278,287 */
/* Facts about the most recent solve on this thread (liblcg reports them only through Pfp). */
int    lcg_hip_last_iterations(void);
double lcg_hip_last_residual(void);
/* Mean device time of the A.x callback over the last solve, in microseconds, from HIP
 * events recorded on the solver stream around each call; 0 unless profiling was enabled.
 * on = 1 times every call, on = k > 1 every k-th call (two stream markers per timed call). */
int    lcg_hip_set_profiling(int on);
double lcg_hip_last_ax_mean_us(void);
int    lcg_hip_last_ax_calls(void);
/* (With the built-in product the solve's SET-UP product y = A.m0 -- lcg.cpp:168, 314, 476, 648 -- carries no event pair and is not
 * counted: whether it is made at all is decided on the device (an all-zero guess needs none), so the figures above are about the
 * products of the iterations.  One consequence for matrices with Inf / NaN ENTRIES: the reference's A.0 already poisons g with
 * 0 x Inf = NaN before the loop, here the first NaN appears one product later -- LCG_NAN_VALUE is returned either way.) */
/* What the latest solve enqueued: vector passes, scalar steps (a step that sums over ranks counts once), reductions over ranks, A.x
 * callbacks (the set-up product included).  Any pointer may be NULL.  bench.py divides by the iterations: launches per iteration. */
int    lcg_hip_last_launches(int *vector_passes, int *scalar_steps, int *rank_reductions, int *products);
/* Always 0.  (Round 3 counted here the scalar steps that ran in the last block of a sharded product -- an opt-in experiment that
 * measured no gain, DESIGN 9, and was retired in round 4; the entry stays so that the library's exports do not change.) */
int    lcg_hip_last_finisher_steps(void);
/* The solvers keep their temporaries (the reference allocates and frees them per call, lcg.cpp:158-166,266-271) for the
 * next solve; this gives the idle ones back to the device. */
int    lcg_hip_trim(void);
/* How plain CG (LCG_CG, lcg.cpp:143-274) -- and PCG with the built-in Jacobi (lpcg, lcg.cpp:293-434: the same rearrangement
 * with u = M^-1 r, w = A u and u.r, w.u in the one reduction) -- is scheduled.  LCG_HIP_CG_CLASSIC: the reference's own
 * recurrence, two reductions per iteration (d.Ad, then m.m/g.g).  LCG_HIP_CG_ONE_REDUCTION: the
 * Chronopoulos-Gear rearrangement of the same recurrence -- w = A.g is applied to the gradient,
 * A.d follows from Ad = beta Ad - w, and g.g, g.w, m.m share ONE reduction (one RCCL all-reduce
 * per iteration instead of two); same iterates in exact arithmetic, same stop rule and counts.
 * LCG_HIP_CG_AUTO (default): one-reduction when the rows are sharded and, on one GPU, for systems of fewer than 2^20 rows
 * (a launch then costs more than the one word per row the rearrangement moves in addition: two launches instead of three) unless A.x or M is a callback of the
 * caller's own -- such a callback sees the reference's sequence of calls (the rearrangement makes one product more before the first
 * stop test); classic otherwise.  tests/test_gpu_solvers.py::test_cg_schedules_on_an_ill_conditioned_system holds both schedules
 * to the oracle's classic loop on a system of condition number 3.6e6 (iteration count, true residual, monitored = true). */
enum { LCG_HIP_CG_AUTO = 0, LCG_HIP_CG_CLASSIC = 1, LCG_HIP_CG_ONE_REDUCTION = 2 };
int    lcg_hip_set_cg_schedule(int schedule);
/* Where the work vectors lie.  The reference allocates its temporaries wherever malloc puts them (lcg.cpp:158-166); on an MI355X
 * the vector a large product WRITES is 8-10 % faster or slower to write depending on whether it shares one of the device's three
 * groups of memory with the matrix's value array (a property of the PAIR of allocations, constant for their lifetime, invisible in
 * any address the process can see: profiles/r04_placement.txt), and the vectors the loop reads beside the matrix pay a
 * little of the same.  Before the first iteration of a real solver whose A.x is lcg_hip_csr_ax the library therefore times y = A.B
 * into each work vector of the solve that it owns itself (and into idle vectors of its pool) and deals the ROLES by weight -- the
 * products' outputs (A.d; A.p and A.s), the vector the product reads, the rest -- the fastest vectors to the heaviest roles.  Where
 * the solve has too few fast vectors, once per matrix: chunks of 1 GiB allocated one after the other until the product into one of
 * them (every fourth, later every eighth, is timed) is clearly faster.  HARD BOUNDS of that walk, each looked at after every single
 * allocation: 128 chunks; 60 ms on the wall clock; at most min(64 GiB, a quarter of the memory that was free when it started) held
 * at once; never into the last 8 GiB of free memory (the clock is read between calls: another chunk is allocated only while the
 * time used plus the dearest allocation so far fits the 60 ms; a first chunk that takes more than 5 ms -- a device that clears
 * what it hands out because all of its memory has been in use since boot -- is the last); no walk at all on a device that is shared (more than 4 GiB were in use by others -- other ranks, the host program's own pool -- when the library was
 * initialised); and no walk once the library has given back more than 1 GiB in the process's life (matrices destroyed, vectors
 * trimmed, an earlier walk's chunks): out of recycled memory ONE 1 GiB allocation costs 30 ms .. 0.5 s, which no bound looked at
 * between calls can hold -- the walk belongs to the first large system of a process.  The chunk found is kept and cut
 * into work vectors (lcg_hip_trim gives it back), the others are given back at once.  A timing that fails means "not tried": the
 * solve goes on with its vectors as allocated.  Roles only: no arithmetic changes, iterates
 * are bit-identical (tests/test_gpu_placement.py).  Results are remembered per (matrix, vector), so later solves time nothing.
 * mode: -1 automatic (real; this process's product streams >= 768 MB), 0 never, 1 for every real matrix with the built-in callback
 * (no walk below that size).  LCG_HIP_PLACE in the environment sets the initial mode. */
int    lcg_hip_set_placement(int mode);
/* The latest solve's placement: vectors timed (0 = everything came from memory, or not tried), roles moved, and what the first
 * output role's product took as allocated / as placed, microseconds (0 when not tried).  Any pointer may be NULL. */
int    lcg_hip_last_placement(int *timed, int *moved, double *us_as_allocated, double *us_as_placed);
/* The pool of work vectors the solvers keep between solves (lcg_hip_trim gives the idle ones back): how many vectors, their bytes, and how
 * many of them are slots of an arena (a 1 GiB chunk the placement kept and cut up).  Any pointer may be NULL. */
int    lcg_hip_pool_info(int *vectors, int64_t *bytes, int *arena_slots);
/* Test hook: one allocation of slots x slot_bytes joins the pool as an arena of `slots` idle vectors -- what the placement's walk leaves
 * behind, without the walk (tests/test_gpu_placement.py: solves take their vectors from it, lcg_hip_trim gives it back as a whole). */
int    lcg_hip_pool_add_arena_for_test(uint64_t slot_bytes, int slots);
/* Test hook: the walk's bounds (0 / negative = the production value): least streamed bytes for a matrix to be placed at all, chunk
 * size, chunk limit, wall-clock limit, most bytes held; force_find_at >= 0 takes the k-th TIMED chunk as the faster place whatever the
 * clock says (so that arena creation and eviction run deterministically at a few million rows); allow_shared = 1 lifts the shared-device
 * rule, the fresh-allocator rule and the look-ahead of the clock (a test walks many times in one process), 2 the shared-device rule only.  tests/test_gpu_placement.py drives walk -> arena -> second matrix -> eviction -> trim with it. */
int    lcg_hip_placement_tune_for_test(uint64_t stream_min_bytes, uint64_t chunk_bytes, int max_chunks, double wall_ms, uint64_t hold_max_bytes,
                                       int force_find_at, int allow_shared);
/* The latest walk: chunks allocated, its wall time (ms), the most bytes it held at once, whether a place was kept, and which bound or
 * finding ended it ("found", "wall clock", "hold limit", "chunk limit", "free-memory floor", "no fresh memory", ...).  Any pointer may be NULL.  Returns the
 * number of walks this process has made so far. */
int    lcg_hip_last_placement_walk(int *chunks, double *wall_ms, int64_t *held_bytes, int *found, const char **ended);

/* ----------------------------------------------------------- solver entry */
/* lcg.h:71-72 lcg_solver() -> lcg.cpp:59-82.  solver_id: LCG_CG, LCG_CGS, LCG_BICGSTAB,
 * LCG_BICGSTAB2; anything else runs CGS exactly as the reference's default branch does. */
int lcg_hip_solver(lcg_axfunc_ptr Afp, lcg_progress_ptr Pfp, double *m, const double *B,
                   int n_size, const lcg_para *param, void *instance, int solver_id, int mem);
/* lcg.h:90-91 lcg_solver_preconditioned() -> lpcg, lcg.cpp:293-434 (solver_id ignored, :90). */
int lcg_hip_solver_preconditioned(lcg_axfunc_ptr Afp, lcg_axfunc_ptr Mfp, lcg_progress_ptr Pfp,
                                  double *m, const double *B, int n_size, const lcg_para *param,
                                  void *instance, int solver_id, int mem);
/* lcg.h:111-113 lcg_solver_constrained() -> lcg.cpp:121-140: LCG_SPG runs lspg (lcg.cpp:1224-1446),
 * every other id lpg (lcg.cpp:1054-1204).  low/hig live where m and B live (`mem`). */
int lcg_hip_solver_constrained(lcg_axfunc_ptr Afp, lcg_progress_ptr Pfp, double *m, const double *B,
                               const double *low, const double *hig, int n_size, const lcg_para *param,
                               void *instance, int solver_id, int mem);
/* lcg.h:135-137 lcg() with caller workspaces (DEVICE pointers or NULL), lcg.cpp:143-274. */
int lcg_hip_lcg(lcg_axfunc_ptr Afp, lcg_progress_ptr Pfp, double *m, const double *B, int n_size,
                const lcg_para *param, void *instance, double *Gk, double *Dk, double *ADk, int mem);
/* lcg.h:166-169 lcgs() with caller workspaces (DEVICE pointers or NULL), lcg.cpp:437-612. */
int lcg_hip_lcgs(lcg_axfunc_ptr Afp, lcg_progress_ptr Pfp, double *m, const double *B, int n_size,
                 const lcg_para *param, void *instance, double *RK, double *R0T, double *PK,
                 double *AX, double *UK, double *QK, double *WK, int mem);
/* clcg.h:74-76 clcg_solver() -> clcg.cpp:46-74.  solver_id: CLCG_BICG (the callback is asked
 * for A^H.x, clcg.cpp:187), CLCG_BICG_SYM, CLCG_CGS, CLCG_BICGSTAB, CLCG_TFQMR; other ids run
 * CGS like the reference's default branch.  The shadow residual of CGS/BiCGStab/TFQMR is drawn from
 * lcg_hip_set_shadow_seed() (default 1) instead of srand(time(0)) (lcg_complex.cpp:118-127). */
int clcg_hip_solver(clcg_hip_axfunc_ptr Afp, clcg_hip_progress_ptr Pfp, double *m, const double *B,
                    int n_size, const clcg_para *param, void *instance, int solver_id, int mem);
/* clcg_solver_preconditioned_cuda() (clcg_cuda.h:105-108) -> clpcg (clcg_cuda.cu:403-558): PCG for
 * complex-symmetric A with unconjugated products; monitors |r|^2/max(|m|^2,1) (or |r|/N), as that
 * CUDA loop does.  Mfp has the complex callback type; clcg_hip_jacobi_mx is the ready-made one.
 * solver_id = CLCG_PBICG runs clpbicg instead (clcg_solver_preconditioned_eigen's default, clcg_eigen.h:87-92,
 * clcg_eigen.cpp:685-802): preconditioned BiCG with two products per iteration, A.p and conj(A).ps (the callback's
 * conjugate flag), Eigen's conjugating dot and the CPU loops' 4th-power stop rule (|<r,r>|^2 / max(|<m,m>|^2, 1), or
 * |r|^2 / N with abs_diff); every other id runs clpcg.  Neither loop has a CPU twin in the reference that builds here. */
int clcg_hip_solver_preconditioned(clcg_hip_axfunc_ptr Afp, clcg_hip_axfunc_ptr Mfp, clcg_hip_progress_ptr Pfp,
                                   double *m, const double *B, int n_size, const clcg_para *param,
                                   void *instance, int solver_id, int mem);
/* Complex64 (single-precision complex) solvers: clcg_cudaf.cu, the CUDA fp32 family.  m, B: n interleaved float pairs where `mem`
 * says.  clcg_solver_cuda (clcg_cudaf.cu:42-60): CLCG_BICG runs clbicg (:86-252; the callback is asked for A^H.x, :217),
 * CLCG_BICG_SYM clbicg_symmetric (:254-401); any other id returns CLCG_UNKNOWN_SOLVER before the arguments are checked.
 * Vectors and the reference's float scalars (ak, betak, norms, residual) are fp32; dots and norms sum exact products in fp64 in a
 * fixed order and are rounded to fp32 once (bit-identical from run to run).  Stop rule |r|^2 / max(|m|, 1)^2, or |r| / n with
 * abs_diff (which then tests |r| / n only, where the reference reads m_mod uninitialised: :162).  Codes as the reference,
 * LCG_REACHED_MAX_ITERATIONS at the cap.  Where the reference spins to the cap after a breakdown (for ever with max_iterations = 0),
 * these stop at the first iteration whose |m|^2 or |r|^2 is NaN with CLCG_NAN_VALUE, as the c128 loops do.  Afp == NULL returns
 * CLCG_INVALID_POINTER.
 * clcg_hip_csr_ax_c64 is the ready-made A.x. */
int clcg_hip_solver_c64(clcg_hip_axfunc_c64_ptr Afp, clcg_hip_progress_c64_ptr Pfp, float *m, const float *B,
                        int n_size, const clcg_para *param, void *instance, int solver_id, int mem);
/* clcg_solver_preconditioned_cuda (clcg_cudaf.cu:66-84): CLCG_PCG runs clpcg (:403-558: unconjugated dots, complex-symmetric A),
 * any other id returns CLCG_UNKNOWN_SOLVER; Mfp == NULL returns LCG_NULL_PRECONDITION_MATRIX.  clcg_hip_jacobi_mx_c64 is the
 * ready-made Jacobi (its reciprocal multiply then rides in the update pass); clcg_hip_ic0_mx_c64, after
 * lcg_hip_csr_build_ic0_c64, the ready-made fp32 IC(0) (sample14.cu's MxProduct). */
int clcg_hip_solver_preconditioned_c64(clcg_hip_axfunc_c64_ptr Afp, clcg_hip_axfunc_c64_ptr Mfp, clcg_hip_progress_c64_ptr Pfp,
                                       float *m, const float *B, int n_size, const clcg_para *param, void *instance,
                                       int solver_id, int mem);
int lcg_hip_set_shadow_seed(unsigned seed);
/* Replace the drawn shadow residual by an explicit vector (n complex, host memory) for the
 * next complex solve only; lets a test replay the reference's own rbar0. */
int lcg_hip_set_shadow_vector(const double *rbar0_host, int n_size);

/* --------------------------------------------------------------- matrices */
/* A CSR matrix resident in HBM: int32 rowptr[n+1] / col[nnz] (base 0), fp64 or c128 val.
 * This is what the reference's GPU samples assemble with cusparseXcoo2csr +
 * cusparseCreateCsr (sample8.cu:169-173, sample10.cu:177-181). */
typedef struct lcg_hip_csr *lcg_hip_csr_t;

/* Copy (mem == HOST, or DEVICE with adopt == 0) or adopt without copying (DEVICE, adopt != 0;
 * the caller keeps the arrays alive) a CSR matrix.  is_complex: val holds interleaved c128.
 * adopt == 2 additionally promises >= 64 readable bytes after col[nnz] and val[nnz], which
 * admits the fastest A.x kernel (copied matrices always have that slack). */
int lcg_hip_csr_create(lcg_hip_csr_t *A, int n_rows, int n_cols, int64_t nnz, const int *rowptr,
                       const int *col, const double *val, int is_complex, int mem, int adopt);
/* The same with complex64 values: val = nnz interleaved (re, im) floats (cuComplex; the CUDA_C_32F matrix of clcg_cudaf.cu's
 * callers, sample14.cu).  Copy / adopt as lcg_hip_csr_create (adopt == 2: 64 readable bytes behind col[nnz] and val[nnz]).
 * Such a handle serves lcg_hip_spmv_c64, clcg_hip_csr_ax_c64, clcg_hip_jacobi_mx_c64, lcg_hip_csr_build_jacobi, the complex64
 * IC(0) entries (lcg_hip_csr_build_ic0_c64, lcg_hip_ic0_solve_c64, clcg_hip_ic0_mx_c64) and the read-only queries
 * (lcg_hip_csr_arrays and lcg_hip_csr_ic0_factor then hand back `val` typed const double *: it points to interleaved float pairs --
 * cast it to const float *); every other entry that takes a matrix (set_kernel / packed / binned / tiled / ranges, distribute, build_ic0,
 * lcg_hip_ic0_solve, lcg_hip_spmv, lcg_hip_spmv_op, lcg_hip_spmv_dot) and the fp64 / c128 ready-made callbacks return LCG_HIP_E_ARG
 * (lcg_hip_last_error() says why); a c128 or real handle in the _c64 entries likewise.  Not shardable. */
int lcg_hip_csr_create_c64(lcg_hip_csr_t *A, int n_rows, int n_cols, int64_t nnz, const int *rowptr,
                           const int *col, const float *val, int mem, int adopt);
/* COO (row-sorted or not) -> CSR on the device: data/README:1-10 files, sample8.cu:30-64,169. */
int lcg_hip_csr_from_coo(lcg_hip_csr_t *A, int n, int64_t nnz, const int *row, const int *col,
                         const double *val, int is_complex, int mem);
int lcg_hip_csr_destroy(lcg_hip_csr_t A);
int lcg_hip_csr_rows(lcg_hip_csr_t A);
int64_t lcg_hip_csr_nnz(lcg_hip_csr_t A);
/* Device pointers of the arrays (for callers that want to inspect or reuse them). */
int lcg_hip_csr_arrays(lcg_hip_csr_t A, const int **rowptr, const int **col, const double **val);
/* Select the SpMV kernel: 0 auto, otherwise lanes per row (2,4,...,64) for the
 * wavefront kernel, or -1 for the LDS-staged variant. */
int lcg_hip_csr_set_kernel(lcg_hip_csr_t A, int variant);
/* Packed column indices for the LDS-staged real A.x (64 rows per block, block-relative columns of 18
 * or 21 bits, seven or six per 16 bytes: 10.3 / 10.7 instead of 12 bytes of stream per entry, -9 % time
 * on the headline system, bit-identical y).  Built on the device at the first product, kept beside the plain
 * column array (+2.67 B per entry).  mode: -1 automatic (matrices of >= 4M entries whose blocks
 * span < 2^21 columns), 0 never (frees the packed copy), 1 whenever eligible.  LCG_HIP_PACKED=0/1
 * overrides for the whole process. */
int lcg_hip_csr_set_packed(lcg_hip_csr_t A, int mode);
/* Blocks of the packed form stored as RUNS: every row of the block has the same number of entries and every entry's column is
 * one more than the entry in the same slot of the row above (constant diagonals, stencils away from the edges).  Such a
 * block carries row 0's columns only -- 8.06 instead of 10.3 bytes of stream per entry -- and its x gathers leave together
 * with the value stream (-22 % on the headline A.x, bit-identical y).  Returns the number of run blocks of the packed copy
 * (0 before the first product built it, or when there are none); *blocks_out (may be NULL) = all blocks of 64 rows. */
int64_t lcg_hip_csr_packed_runs(lcg_hip_csr_t A, int64_t *blocks_out);
/* STRETCHES of run blocks: consecutive full run blocks with the same row length and the same offsets column - row, their entries
 * one behind the other (the interior of a constant-diagonal system is one stretch).  The four longest (of >= 2 blocks) travel in the
 * kernel's arguments and their blocks load neither row pointers nor their per-block plan (bit-identical y and carried sums).
 * mode: 0 off (default), 1 on; LCG_HIP_RUN_STRETCHES=0/1 overrides for the whole process.  OFF by default: on the headline system the
 * blocks' staggered starts behind their own cold loads serve the value stream better than starting together -- same-box A/B 1542-1555
 * CG iterations/s without, 1514-1529 with (profiles/run_stretches_ab.txt).  No reference counterpart. */
int lcg_hip_csr_set_run_stretches(lcg_hip_csr_t A, int mode);
/* Stretches the packed kernel runs from (0 before the first product built them, when switched off or when there are none);
 * *blocks_out (may be NULL) = the blocks they cover. */
int64_t lcg_hip_csr_run_stretches(lcg_hip_csr_t A, int64_t *blocks_out);
/* SYMMETRIC run stretches: a stretch whose row length is 2p + 1 with the diagonal in slot p, whose offsets column - row are
 * antisymmetric and whose values mirror each other BIT FOR BIT (val(i, k) == val(i + off[k], 2p - k): +-0, a NaN's payload or one ulp
 * refuse it) keeps a HALF STORE beside the CSR arrays: per block of 64 rows one tile of its diagonal and p upper diagonals, (p + 1) x 512
 * bytes, laid out in the order the product's workgroups are dispatched.  The blocks of the stretch's inner range (the stretch minus
 * the ceil(largest offset / 64) + 1 blocks in front, from the next multiple of eight blocks on) are multiplied by k_spmv_ldsp_sym, which
 * reads a lower entry as its partner row's upper entry: half the value stream from memory, bit-identical y and carried sums.  The
 * longest qualifying stretch of a real fp64 matrix on one GPU is taken (not a sharded handle, not a transposed copy, not a row range).
 * mode: -1 automatic, 0 off, 1 forced (any qualifying stretch whose inner range has as many blocks as slices); LCG_HIP_SYM_RUNS=-1/0/1
 * overrides for the whole process.  The automatic mode (the default) takes such a stretch where the product streams >= 512 MB: 1619-1632
 * against 1463-1551 CG iterations/s on the 10M-row, 33-diagonal system (profiles/sym_runs_ab.txt).  MEMORY: the half store is about half
 * the value array again (1.33 GB for that system); the CSR arrays stay as they are; lcg_hip_csr_plan_info counts it.  Setting the mode frees the half store or has the plan built
 * again at the next product.  The half store is a copy of VALUES (the rest of the packed form copies columns only): in the rewrite
 * protocol below (lcg_hip_csr_set_binned) it goes, like the op(A) copies, with any of set_packed / set_tiled / set_binned / set_ranges (A, 0)
 * and with set_sym_runs itself (a device synchronisation; the packed plan is built again at the next product, which checks the new
 * values and builds the half store again -- or refuses them).  The offsets must ascend in storage order (sorted rows).  No reference counterpart. */
int lcg_hip_csr_set_sym_runs(lcg_hip_csr_t A, int mode);
/* Slices of the inner range: 1 (blocks in row order: the default, and what was measured fastest -- DESIGN 3.1), 2, 4 or 8 (workgroup w takes
 * block (w % slices) * S + w / slices of it: with 8 a contiguous eighth of the rows per XCD, the tiles interleaved in dispatch order);
 * 0 = the default, one.  LCG_HIP_SYM_NX=1/2/4/8 overrides for the whole process, as LCG_HIP_SYM_RUNS does the mode.  A change has the
 * plan built again at the next product. */
int lcg_hip_csr_set_sym_slices(lcg_hip_csr_t A, int slices);
/* Slices of the symmetric stretch the product runs from (0: none); *blocks_out (may be NULL) = the blocks k_spmv_ldsp_sym multiplies,
 * *status_out (may be NULL) = "taken", or why the latest plan refused ("refused: ..."), or "not tried" (a static string). */
int64_t lcg_hip_csr_sym_runs(lcg_hip_csr_t A, int64_t *blocks_out, const char **status_out);
/* Blocks of 64 rows the packed form stores as TEMPLATE blocks: every entry on one of <= 64 diagonals (the union of the rows'), rows of
 * <= 32 entries, and a 64-bit mask per row saying which diagonals the row has -- what a stencil's blocks look like where grid boundaries pass
 * through them.  Like run blocks they stream values only and are bit-identical to the plain row-block kernel.
 * No reference counterpart. */
int64_t lcg_hip_csr_packed_templates(lcg_hip_csr_t A);
/* Two-pass "binned" A.x for matrices whose columns are scattered over more of x than any cache holds (the
 * arbitrary user CSR of sample8.cu:96-103 at its worst): pass 1 expands x into entry order with a 64 KB slice
 * of x in LDS per workgroup, pass 2 streams val and the expanded x and sums the rows in LDS (one wavefront per
 * 2048 rows, ds_add_f64) -- 28.5 streamed bytes per entry instead of 12 + a cache line per gather.  The plan
 * (re-ordered copy of the matrix: +26.5 B per entry) is built on the device at the first product.
 * mode: -1 automatic (real matrices of >= 4M entries and >= 1M columns whose 64-row blocks span on average
 * >= 2^20 columns, whose columns do not run along diagonals and
 * whose gathers mostly have a cache line of x of their own (share >= 0.5: block-structured
 * matrices stay with the row-block kernels), 0 never (frees the plan), 1 whenever eligible.
 * LCG_HIP_BINNED=0/1 overrides for the whole process.  y differs from the row-block kernels' y in the last
 * bits (products are rounded before the add); on gfx950 it is bit-identical from call to call and from plan to plan
 * (lanes of one ds_add_f64 that meet in a row are serialised by the LDS in lane order: verified by test, not an ISA promise).
 * The packed, tiled and binned forms, the row ranges, a symmetric stretch's half store and the op(A) copies of lcg_hip_spmv_op / clcg_hip_csr_ax are COPIES of
 * the matrix made at their first use: a caller who rewrites the VALUES or COLUMNS of an adopted matrix (lcg_hip_csr_create with
 * adopt != 0; same row pointers, columns in range) afterwards drops them with set_packed / set_tiled / set_binned /
 * set_ranges(A, 0) -- any one of them frees the op(A) copies, each frees its own plan -- and re-arms the automatic choice with
 * set_*(A, -1); every product then follows the new arrays.  New ROW POINTERS need a new handle (the kernel choice keeps what it
 * read from them), and so does a rewritten complex64 matrix (lcg_hip_csr_create_c64: its set_* entries refuse, its op(A) copies
 * are built once) and a sharded one (lcg_hip_csr_distribute: its rows' local and remote parts are copies split out of the arrays,
 * which the setters do not rebuild). */
int lcg_hip_csr_set_binned(lcg_hip_csr_t A, int mode);
/* One-pass "tiled" A.x for matrices whose rows draw their columns at random from a band: the row-block kernels
 * find x in the L2 there but move a 128-byte line per 8-byte gather.  A workgroup owns 8 x 1024 rows (sums in LDS),
 * walks the column tiles they touch (2048 columns; a loader wavefront copies the next tile of x into LDS by LDS-DMA while
 * eight consumer wavefronts stream the rows' entries of the current one: 2 KB per step of 192 entries = values + three
 * 21-bit (row, column) pairs per 64-bit word, 10.67 B per entry where CSR has 12).  mode: -1 automatic (real matrices of
 * >= 4M entries whose columns do not run along diagonals, whose gathers mostly have a cache line of x of their own
 * (share >= 0.18) and whose (workgroup, tile) pairs hold >= 700 entries on average), 0 never (frees the plan), 1 whenever eligible;
 * LCG_HIP_TILED=0/1 overrides for the process.  Same last-bit deviation from the row-block kernels as the binned product; y is bit-identical from call to
 * call and from plan to plan ON gfx950 (a row is summed by one wavefront in stream order; lanes of one ds_add_f64 that meet
 * in a row are serialised by the LDS in lane order -- verified by tests/test_gpu_binned.py, not promised by the ISA). */
int lcg_hip_csr_set_tiled(lcg_hip_csr_t A, int mode);
const char *lcg_hip_csr_tiled_status(lcg_hip_csr_t A);
/* Row ranges: a matrix whose rows fall into different column-pattern classes (a stencil in most rows, scattered columns in the
 * rest) is multiplied range by range, every range choosing its own kernel family among the ones above; the rows are cut where
 * the class of their 2048-row chunks changes (share of entries that continue a diagonal, mean column span of a 64-row block).
 * A range's product is bit-identical to the product of that range as a matrix of its own.  mode: -1 automatic (real matrices of
 * >= 4M entries, ranges of >= 256K entries, at most 8), 0 never, 1 whenever two classes are found; LCG_HIP_RANGES=0/1 overrides
 * for the process.  lcg_hip_csr_last_kernel then reads "rows [a, b): <kernel> | rows [b, c): <kernel> ...".
 * The reference has no counterpart (its A.x is the user's callback: lcg.h:37-38); speed only. */
int lcg_hip_csr_set_ranges(lcg_hip_csr_t A, int mode);
/* Number of row ranges the latest product used (0: one kernel family for all rows); first_row[0 .. min(cap, ranges)) = their first rows. */
int lcg_hip_csr_ranges(lcg_hip_csr_t A, int cap, int *first_row);
/* Why A has (or has not) a binned plan: "ready", or the reason it is not used (static string). */
const char *lcg_hip_csr_binned_status(lcg_hip_csr_t A);
/* Name of the kernel family the latest product with A used (static string; "" before the first product). */
const char *lcg_hip_csr_last_kernel(lcg_hip_csr_t A);
/* Bytes the latest product's kernels stream from / to memory per call BY CONSTRUCTION -- what must move for the kernel
 * family that ran: CSR row-block kernels 12 B per entry; packed columns 8 B + 16 B per group of 6-7 columns (run blocks:
 * row 0's columns only); tiled product 2 KB per step of 192 entries (10.67 B per entry) + tile lists; binned product both
 * passes (28.5 B per entry) -- each plus row pointers, x once and y.  0 for complex matrices and before the first product.
 * (SURVEY's algorithmic figure, 12 nnz + 4 (N + 1) + 16 N, is what bench.py's roofline.achieved is quoted on; this is the
 * physical companion: bench.py's roofline.must_move_bytes.) */
int64_t lcg_hip_csr_last_traffic_model(lcg_hip_csr_t A);
/* What the first product spent on A beside the CSR arrays: *build_ms = host time of choosing a kernel family and building
 * its copy of the matrix (packed columns / tiled stream / binned streams; the builders drain the stream), *extra_bytes =
 * device memory those copies hold.  Either pointer may be NULL. */
int lcg_hip_csr_plan_info(lcg_hip_csr_t A, double *build_ms, int64_t *extra_bytes);
/* Extract the diagonal and keep its reciprocal for lcg_hip_jacobi_mx
 * (lcg_smDcsr_get_diagonal algebra_cuda.cu:40-57,85-92; clcg_smZcsr_get_diagonal
 * lcg_complex_cuda.cu:46-63).  diag_out (device, n values) may be NULL.  A complex64 handle keeps complex64 reciprocals (for
 * clcg_hip_jacobi_mx_c64) and diag_out, if given, receives n interleaved float pairs. */
int lcg_hip_csr_build_jacobi(lcg_hip_csr_t A, double *diag_out);

/* Ready-made callbacks; pass the lcg_hip_csr_t as `instance`. */
void lcg_hip_csr_ax(void *instance, const double *x, double *prod_Ax, const int n_size);      /* cudaAx, sample8.cu:96-103 */
void lcg_hip_jacobi_mx(void *instance, const double *x, double *prod_Mx, const int n_size);   /* sample1.cpp:55-62 (z = x/diag, reciprocal form) */
void clcg_hip_csr_ax(void *instance, const double *x, double *prod_Ax, const int n_size,
                     int layout, int conjugate);                                                /* sample10.cu:90-97 */
void clcg_hip_jacobi_mx(void *instance, const double *x, double *prod_Mx, const int n_size,
                        int layout, int conjugate);                                             /* sample10.cu:99-120 (Jacobi branch) */
/* The complex64 ones.  clcg_hip_csr_ax_c64 = lcg_hip_spmv_c64 (all four forms; sample14.cu's cusparseSpMV callback);
 * clcg_hip_jacobi_mx_c64: z = x .* (1 / diag) after lcg_hip_csr_build_jacobi, layout / conjugate ignored.  (The fp32 IC(0)
 * callback, clcg_hip_ic0_mx_c64, is declared with the IC(0) entries below.) */
void clcg_hip_csr_ax_c64(void *instance, const float *x, float *prod_Ax, const int n_size,
                         int layout, int conjugate);
void clcg_hip_jacobi_mx_c64(void *instance, const float *x, float *prod_Mx, const int n_size,
                            int layout, int conjugate);

/* ---------------------------------------------------------------- IC(0) preconditioner */
/* Incomplete Cholesky with zero fill on the pattern of A's lower triangle (diagonal included; the upper triangle is ignored,
 * duplicate entries are summed, columns may come in any order): A ~ L.L^T, unconjugated with the principal square root for
 * complex A.  Factored on the device over the forward solve's level schedule; L and L^T are copies (rebuild after rewriting an
 * adopted matrix), freed by lcg_hip_csr_destroy.  Rebuilds on repeat.  LCG_HIP_E_ARG for a non-square or sharded matrix or a
 * failed pivot (<= 0 or not finite, real; 0 or not finite, complex): lcg_hip_last_error() names the smallest such row.
 * Stands in for cusparseDcsric02 (sample8.cu:183-238), cusparseZcsric02 (sample10.cu:226-266) and
 * clcg_incomplete_Cholesky_cuda_full (preconditioner_cuda.cu:207-259; sample12.cu:153, sample13.cu:156).
 * Serves fp64 and complex128 handles; a complex64 handle returns LCG_HIP_E_ARG (its entry is lcg_hip_csr_build_ic0_c64). */
int  lcg_hip_csr_build_ic0(lcg_hip_csr_t A);
/* The same for a handle from lcg_hip_csr_create_c64, in fp32 complex arithmetic throughout (cuCmulf / cuCdivf's products and
 * quotients, the principal fp32 square root; the order of operations of the other types): the same rules (square, not
 * sharded, rebuild on repeat, LCG_HIP_E_ARG naming the smallest failed pivot row: 0 or not finite).  A real or complex128
 * handle returns LCG_HIP_E_ARG.  Stands in for clcg_incomplete_Cholesky_cuda_half with cuComplex (preconditioner_cuda.cu;
 * sample14.cu). */
int  lcg_hip_csr_build_ic0_c64(lcg_hip_csr_t A);
/* Levels of L and L^T, kernel launches of one full apply, the failed pivot's row (-1 = none; what
 * cusparseXcsric02_zeroPivot reports), host milliseconds of the build, device bytes held by the factor.  Any pointer may be NULL.
 * With sweeps set (lcg_hip_csr_ic0_set_sweeps) the launches are the sweep apply's 2k and the bytes include its two vectors.
 * This, lcg_hip_csr_ic0_factor and lcg_hip_csr_ic0_schedule_for_test serve every value type. */
int  lcg_hip_csr_ic0_info(lcg_hip_csr_t A, int *levels_lower, int *levels_upper, int *launches_per_apply,
                          int *zero_pivot, double *build_ms, int64_t *bytes);
/* How a factor is applied.  sweeps = 0 (the state after every build): the two triangular solves are exact, level by level.
 * sweeps = k >= 1: every later apply on this handle -- lcg_hip_ic0_solve / _c64 for each `which`, and the three callbacks below --
 * replaces each triangular solve T y = x (T = D + N, D its diagonal) by k Jacobi sweeps from y = 0:
 *     y(1)_i = x_i / T(i,i),   y(j+1)_i = (x_i - sum_p T(i,c_p) y(j)_{c_p}) / T(i,i),   result y(k),
 * each sweep one launch over all rows that reads y(j) and writes y(j+1) elsewhere (2k launches per full apply, no dependency
 * between rows).  The operator is S^T.S with S = sum_{j<k} (-D^-1 N)^j D^-1: symmetric positive definite for a real factor
 * and every k, complex symmetric for a complex one, and the same in every iteration, so PCG may use it.  A row is summed as
 * the exact solve sums it, so k >= the triangle's level count returns the exact solve's bits.  which = 2 feeds L's result to
 * L^T's sweeps.  Serves every value type.  Allocates (k >= 1) or frees (0) two vectors of the factor's type; not stream
 * work otherwise, and may be called between solves.  LCG_HIP_E_ARG for a NULL handle, a handle without a factor, sweeps < 0. */
int  lcg_hip_csr_ic0_set_sweeps(lcg_hip_csr_t A, int sweeps);
int  lcg_hip_csr_ic0_get_sweeps(lcg_hip_csr_t A, int *sweeps);
/* Device arrays of L in natural row order: rows sorted by column, the diagonal last.  For a complex64 factor `val` points to
 * interleaved float pairs (cast it to const float *, as for lcg_hip_csr_arrays). */
int  lcg_hip_csr_ic0_factor(lcg_hip_csr_t A, const int **rowptr, const int **col, const double **val);
/* y = L^-1 x (which 0), L^-T x (1) or (L.L^T)^-1 x (2) on the current stream; x, y on the device and not overlapping
 * (cusparseDcsrsv2_solve, sample8.cu:105-119; cusparseSpSV, sample12.cu:153). */
int  lcg_hip_ic0_solve(lcg_hip_csr_t A, int which, const double *x, double *y);
/* The same for a complex64 factor (lcg_hip_csr_build_ic0_c64), fp32 throughout, with the same checks (which, overlap, factor
 * present; another handle type: LCG_HIP_E_ARG).  cusparseSpSV with CUDA_C_32F (sample14.cu). */
int  lcg_hip_ic0_solve_c64(lcg_hip_csr_t A, int which, const float *x, float *y);
/* Ready-made preconditioner callbacks, z = (L.L^T)^-1 x; pass the lcg_hip_csr_t as `instance`.  A handle without a factor, the
 * wrong value type, n_size other than the row count or conjugate = 1 end the solve with LCG_HIP_E_ARG; layout is ignored
 * (M is (complex-)symmetric). */
void lcg_hip_ic0_mx(void *instance, const double *x, double *prod_Mx, const int n_size);          /* sample8.cu:105-119 */
void clcg_hip_ic0_mx(void *instance, const double *x, double *prod_Mx, const int n_size,
                     int layout, int conjugate);                                                  /* sample10.cu:99-120 (IC branch) */
/* The complex64 one, for clcg_hip_solver_preconditioned_c64 (sample14.cu's MxProduct: the SpSV with L, then with L^T).  Neither
 * allocates nor synchronises; honours the solve's stop flag. */
void clcg_hip_ic0_mx_c64(void *instance, const float *x, float *prod_Mx, const int n_size,
                         int layout, int conjugate);
/* Test hook: the widest level a one-workgroup launch may take over several levels (0: one launch per level; -1: production). */
int  lcg_hip_csr_ic0_schedule_for_test(lcg_hip_csr_t A, int max_merged_rows);

/* ---------------------------------------------------------------- ILU(0) preconditioner */
/* Incomplete LU with zero fill on the pattern of A (every entry; one explicit zero is added on every diagonal, duplicate
 * entries are summed, columns may come in any order): A ~ L.U with a unit lower L, unconjugated for complex A,
 *     w(i,j) = A(i,j) - sum_{k < min(i,j)} L(i,k) U(k,j),   U(i,j) = w(i,j) (j >= i),   L(i,j) = w(i,j) / U(j,j) (j < i).
 * No square root is taken, so a symmetric indefinite or a non-symmetric matrix factors where IC(0) cannot: the only failed
 * pivot is U(i,i) that is 0 or not finite (a negative real pivot is fine).  Factored on the device over L's forward level
 * schedule; L and U are copies (rebuild after rewriting an adopted matrix), freed by lcg_hip_csr_destroy, held in a slot of
 * their own: IC(0) and ILU(0) may live on one handle.  Rebuilds on repeat.  LCG_HIP_E_ARG for a non-square or sharded matrix,
 * a complex64 handle or a failed pivot: lcg_hip_last_error() names the smallest such row.
 * Stands in for cusparseZcsrilu02 and its analysis (sample11.cu:231-262) and for lcg_incomplete_LU / clcg_incomplete_LU of
 * the Eigen back-end (preconditioner_eigen.h:109-119; sample7).  Serves fp64 and complex128 handles. */
int  lcg_hip_csr_build_ilu0(lcg_hip_csr_t A);
/* Levels of L (forward) and of U (backward, from U's own pattern), kernel launches of one full apply, the failed pivot's row
 * (-1 = none; what cusparseXcsrilu02_zeroPivot reports), host milliseconds of the build, device bytes held by the factor.
 * Any pointer may be NULL.  With sweeps set the launches are what the sweep apply really launches, 2k - 1 for k >= 2 and 2
 * for k = 1 (below), and the bytes include its two vectors. */
int  lcg_hip_csr_ilu0_info(lcg_hip_csr_t A, int *levels_L, int *levels_U, int *launches_per_apply, int *zero_pivot,
                           double *build_ms, int64_t *bytes);
/* How the factor is applied, with the contract of lcg_hip_csr_ic0_set_sweeps.  sweeps = 0 (the state after every build): two
 * exact triangular solves, level by level.  sweeps = k >= 1: each solve T y = x (T = D + N) becomes k Jacobi sweeps from
 * y = 0, y(j+1) = D^-1 (x - N y(j)), every sweep one launch over all rows; D = I for L, so L's first sweep is y = x and
 * costs no launch of its own when k >= 2 (the second sweep reads x), one copy when k = 1.  A row is summed as the exact solve
 * sums it, so k >= the triangle's level count returns the exact solve's bits.  The operator is the same in every iteration.
 * For a symmetric A, U = D.L^T and the sweep operator is P^T D^-1 P with P = sum_{j<k} (-N)^j, N = L - I, D = diag U: it stays
 * symmetric in exact arithmetic for every k, so PCG may use it (positive definite when every pivot is positive).
 * Allocates (k >= 1) or frees (0) two vectors; LCG_HIP_E_ARG for a NULL handle, a handle without a factor, sweeps < 0. */
int  lcg_hip_csr_ilu0_set_sweeps(lcg_hip_csr_t A, int sweeps);
int  lcg_hip_csr_ilu0_get_sweeps(lcg_hip_csr_t A, int *sweeps);
/* Device arrays of L (which 0: rows sorted by column, the unit diagonal not stored) or U (which 1: rows sorted, the diagonal
 * first), in natural row order. */
int  lcg_hip_csr_ilu0_factor(lcg_hip_csr_t A, int which, const int **rowptr, const int **col, const double **val);
/* y = L^-1 x (which 0), U^-1 x (1) or U^-1 L^-1 x (2) on the current stream; x, y on the device and not overlapping.  Neither
 * allocates nor synchronises; honours a running solve's stop flag (the two cusparseZcsrsv2_solve of sample11.cu:100-121). */
int  lcg_hip_ilu0_solve(lcg_hip_csr_t A, int which, const double *x, double *y);
/* Ready-made preconditioner callbacks, z = U^-1 L^-1 x; pass the lcg_hip_csr_t as `instance`.  A handle without a factor, the
 * wrong value type or n_size other than the row count end the solve with LCG_HIP_E_ARG; so do layout = 1 and conjugate = 1
 * (M = L.U is not symmetric in general; the PCG and PBiCG loops ask for (0, 0)). */
void lcg_hip_ilu0_mx(void *instance, const double *x, double *prod_Mx, const int n_size);
void clcg_hip_ilu0_mx(void *instance, const double *x, double *prod_Mx, const int n_size,
                      int layout, int conjugate);                                                 /* sample11.cu:100-121 (cudaMx_ILU) */
/* Right preconditioning for the loops that take no Mfp (lcg_hip_solver: LCG_BICGSTAB, LCG_BICGSTAB2, LCG_CGS;
 * clcg_hip_solver: the loops that ask for (layout, conjugate) = (0, 0) only): an Afp that computes y = A.(U^-1 L^-1 x) -- the
 * factor's apply into a vector the factor owns, then the handle's ordinary product.  Solve A.M^-1 u = b from u = 0 with it,
 * then x = M^-1 u by lcg_hip_ilu0_solve(A, 2, u, x).  The residual b - A.M^-1 u is b - A.x, the same vector either way; the
 * relative stop rule divides by max(u.u, 1), so it sees |u|, not |x|.  The solver treats these as callbacks of the caller's
 * own (the product carries no dot, nothing is timed or placed).  Same failures as the Mfp callbacks above. */
void lcg_hip_csr_ax_ilu0(void *instance, const double *x, double *prod_Ax, const int n_size);
void clcg_hip_csr_ax_ilu0(void *instance, const double *x, double *prod_Ax, const int n_size,
                          int layout, int conjugate);
/* Test hook: the widest level a one-workgroup launch may take over several levels (0: one launch per level; -1: production). */
int  lcg_hip_csr_ilu0_schedule_for_test(lcg_hip_csr_t A, int max_merged_rows);

/* ---------------------------------------------------------------- dense operators */
/* A dense M x N matrix resident in HBM, row-major, fp64 or complex128 (interleaved): the operator of liblcg's own samples,
 * whose products are lcg_matvec (algebra.cpp:165-193) and clcg_matvec (lcg_complex.cpp:169-234).  A handle of its own kind:
 * both kinds of handle begin with a word that says which kind they are.  Every lcg_hip_dense_* / clcg_hip_dense_* entry returns
 * LCG_HIP_E_ARG for a handle that is not a dense one (a CSR handle included), and EVERY entry that takes a lcg_hip_csr_t, or a
 * CSR handle as a callback's instance, refuses a dense handle before it reads anything else of it: LCG_HIP_E_ARG from the entries
 * that return a status or a count, "" / NULL from those that return a string or a pointer, and a callback ends the solve with
 * LCG_HIP_E_ARG; lcg_hip_last_error() names the entry.  A handle is at least 8 readable bytes.  The library keeps ONE copy, rows padded to 16 bytes, and no second copy for the transposed or conjugated
 * forms: 8 bytes per entry and product (16 complex) where a full CSR stores 12 (20) and gathers x. */
typedef struct lcg_hip_dense *lcg_hip_dense_t;

/* Copy an m_rows x n_cols matrix: val[i * ld + j] (ld >= n_cols, counted in entries: doubles, or complex pairs when is_complex),
 * host (mem = LCG_HIP_MEM_HOST) or device memory.  LCG_HIP_E_ARG for a NULL pointer, m_rows or n_cols <= 0, ld < n_cols. */
int lcg_hip_dense_create(lcg_hip_dense_t *K, int m_rows, int n_cols, const double *val, int64_t ld, int is_complex, int mem);
/* The same from liblcg's own layout: m_rows HOST row pointers (lcg_float ** / lcg_complex **: lcg_malloc(m, n), algebra.cpp:60-98). */
int lcg_hip_dense_create_rows(lcg_hip_dense_t *K, int m_rows, int n_cols, const double *const *rows, int is_complex);
int lcg_hip_dense_destroy(lcg_hip_dense_t K);
int lcg_hip_dense_rows(lcg_hip_dense_t K);
int lcg_hip_dense_cols(lcg_hip_dense_t K);
/* lcg_matvec: layout 0 (MatNormal) y[M] = K.x[N]; layout 1 (MatTranspose) y[N] = K^T.x[M].  x, y: device vectors, x != y; launched
 * on the library's stream, neither allocates nor synchronises.  Every product is bit-identical from call to call. */
int lcg_hip_dense_matvec(lcg_hip_dense_t K, const double *x, double *y, int layout);
/* clcg_matvec's four forms.  conjugate = 1 is the reference's Conjugate (lcg_complex.cpp:184-185, 198-199): conj(K).x or K^H.x --
 * the ENTRIES are conjugated, x is not. */
int clcg_hip_dense_matvec(lcg_hip_dense_t K, const double *x, double *y, int layout, int conjugate);
/* y[N] = K^T.(K.x[N]), real K: the normal-equations product of sample1.cpp:48-53.  The M-vector in between belongs to the handle. */
int lcg_hip_dense_ata(lcg_hip_dense_t K, const double *x, double *y);
/* Ready-made callbacks; pass the lcg_hip_dense_t as `instance`.  A handle of another kind, the wrong value type or an n_size that
 * is not the matrix's N end the solve with LCG_HIP_E_ARG (lcg_hip_last_error() says which) and write nothing. */
void lcg_hip_dense_ata_ax(void *instance, const double *x, double *prod_Ax, const int n_size);    /* sample1.cpp:48-53 (CalAx) */
void lcg_hip_dense_ax(void *instance, const double *x, double *prod_Ax, const int n_size);        /* y = K.x, square K */
void clcg_hip_dense_ax(void *instance, const double *x, double *prod_Ax, const int n_size,
                       int layout, int conjugate);                                                 /* sample3.cpp:44-49 (CalAx) */
/* The Jacobi preconditioner of the samples.  normal = 1 (real K): d_i = sum_j K(j,i)^2, the diagonal of K^T.K, by one more
 * column-form pass (sample1.cpp:98-107).  normal = 0 (square K, real or complex): d_i = K(i,i).  The reciprocals are kept for the
 * callbacks below; diag_out (device, N values; may be NULL) receives d.  LCG_HIP_E_ARG when an entry of d is zero or not finite:
 * lcg_hip_last_error() names the smallest such index.  Synchronises. */
int lcg_hip_dense_build_jacobi(lcg_hip_dense_t K, int normal, double *diag_out);
void lcg_hip_dense_jacobi_mx(void *instance, const double *x, double *prod_Mx, const int n_size);  /* sample1.cpp:55-62, reciprocal form */
void clcg_hip_dense_jacobi_mx(void *instance, const double *x, double *prod_Mx, const int n_size,
                              int layout, int conjugate);
/* Name of the kernel family the latest product with K used ("" before the first), and the list of all of them
 * (index 0, 1, ...; NULL behind the last): k_dn_row, k_dn_row_split, k_dn_col, k_dn_ata_two_pass, k_dn_ata_one_pass,
 * k_dn_ata_small. */
const char *lcg_hip_dense_last_kernel(lcg_hip_dense_t K);
const char *lcg_hip_dense_kernel_name(int index);
/* Force a path: 0 automatic; 1 k_dn_row and 2 k_dn_row_split for K.x; 4 two passes, 5 one pass and 6 the one-workgroup form for
 * K^T.K.x (5, 6: real K, N <= 2048; 6 is never chosen automatically; 2 is refused where there is nothing to split: rows of
 * fewer than 32 16-byte packs, or M >= 8192).  K^T.x has one form (3 is accepted and changes nothing).  A forced path holds for the
 * products it names; the others stay automatic. */
int lcg_hip_dense_set_kernel(lcg_hip_dense_t K, int variant);
/* The same products over k = 2, 4 or 8 right-hand sides with K read ONCE for all of them.  A block of k vectors is
 * lcg_hip_spmm's: one array of rows x k doubles, row-major (X[i * k + j] = row i of column j), its base 16-byte aligned.  Any other k,
 * a null block or a misaligned base: LCG_HIP_E_ARG before the device or the handle is looked at.  Real fp64 dense handles on one GPU:
 * a handle that is not a dense one (a CSR handle included), a complex dense handle, a layout outside 0 / 1, normal = 0 on a
 * non-square K, or X and Y overlapping return LCG_HIP_E_ARG with lcg_hip_last_error() naming the entry and the reason, Y untouched.
 * Column j's bits depend on K, the handle's forced variant and column j of X (and U) alone: the same whatever k is, whatever the
 * other columns hold (NaN and Inf included), from call to call.  They need not be the bits of lcg_hip_dense_matvec on that column.
 * lcg_hip_dense_set_kernel's variants 1 / 2 force the k-wide row form / split row form as they do for K.x; 4 - 6 are not looked at.
 * The M x k block between the two products of K^T.(K.X) and the k-wide table of partial sums belong to the handle: the first call at
 * a k larger than any before may allocate and wait, later ones only launch; lcg_hip_dense_destroy frees them. */
/* Y = K.X (layout 0: X is N x k, Y is M x k) or Y = K^T.X (layout 1: X is M x k, Y is N x k), K read once for all k columns. */
int lcg_hip_dense_matmat(lcg_hip_dense_t K, int k, const double *X, double *Y, int layout);
/* Y[N x k] = K^T.(K.X): two passes over K; the M x k block in between belongs to the handle. */
int lcg_hip_dense_ata_multi(lcg_hip_dense_t K, int k, const double *X, double *Y);
/* The operator of the batched loops with the sum they take after it: Y = (normal ? K^T.K : K).X and, with U != NULL,
 * dots[j] = Y_j . U_j (host, k values, after a stream synchronise; NULL dots = enqueue only).  normal = 0 needs square K.  The sum
 * costs no pass over K: one k-wide launch over Y and U leaves at most 512 partial sums per column, added in a fixed order. */
int lcg_hip_dense_op_multi_dot(lcg_hip_dense_t K, int k, int normal, const double *X, double *Y, const double *U, double *dots);
/* Name of the k-wide kernel family the latest k-wide product with K used ("" before the first), and the list of all of them
 * (index 0, 1, ...; NULL behind the last): k_dnm_row, k_dnm_row_split, k_dnm_col, k_dnm_ata_two_pass.  The single-vector names
 * (lcg_hip_dense_last_kernel, lcg_hip_dense_kernel_name) are not touched by the k-wide products. */
const char *lcg_hip_dense_multi_last_kernel(lcg_hip_dense_t K);
const char *lcg_hip_dense_multi_kernel_name(int index);
/* Batched CG and PCG on a dense handle: lcg_hip_lcg_multi / lcg_hip_lpcg_multi's loop, contract and codes, word for word, with the
 * operator A = K^T.K (normal = 1: sample1.cpp's CalAx, the normal equations) or A = K (normal = 0, square K).  M (in/out) and B are
 * N x k blocks where `mem` says.  PCG uses the reciprocals of lcg_hip_dense_build_jacobi(K, normal, ...): none built, or built for
 * the other operator, returns LCG_NULL_PRECONDITION_MATRIX.  Per iteration K is read twice (normal = 1) or once for all k columns.
 * Column j's results depend on K, column j of B and M and param alone, bit for bit: whatever k is, whatever the other columns hold,
 * from call to call.  lcg_hip_last_launches counts every kernel of the operator (its products, folds and the carried sum) as a
 * product. */
int lcg_hip_dense_lcg_multi (lcg_hip_dense_t K, int k, int normal, double *M, const double *B, const lcg_para *param,
                             int *ret, int *iterations, double *residual, int mem);
int lcg_hip_dense_lpcg_multi(lcg_hip_dense_t K, int k, int normal, double *M, const double *B, const lcg_para *param,
                             int *ret, int *iterations, double *residual, int mem);
/* The complex128 twins: the products of clcg_hip_dense_matvec over k = 2, 4 or 8 right-hand sides with K read ONCE
 * for all of them.  A block of k complex vectors is clcg_hip_spmm's: one array of rows x k interleaved (re, im) pairs, row-major
 * (column j of row i is doubles 2 (i k + j) and 2 (i k + j) + 1), its base 16-byte aligned.  Any other k, a null block or a misaligned
 * base: LCG_HIP_E_ARG before the device or the handle is looked at.  Complex128 dense handles on one GPU: a handle that is not a dense
 * one (a CSR handle included), a real dense handle, a non-square K where the loops' operator is asked for, a layout or conjugate
 * outside 0 / 1, or X and Y overlapping return LCG_HIP_E_ARG with lcg_hip_last_error() naming the entry and the reason, Y untouched.
 * Column j's bits depend on K, the handle's forced variant and column j of X (and U) alone: the same whatever k is, wherever the
 * column stands in the block, whatever the other columns hold (NaN and Inf included), from call to call.  They need not be the bits
 * of clcg_hip_dense_matvec on that column.  lcg_hip_dense_set_kernel's variants 1 / 2 force the k-wide row form / split row form.
 * The k-wide table of partial sums belongs to the handle: the first call at a k larger than any before may allocate and wait, later
 * ones only launch; lcg_hip_dense_destroy frees it.  The real k-wide entries above keep refusing complex handles. */
/* Y = op(K).X: layout 0 K.X (X is N x k, Y is M x k), layout 1 K^T.X (X is M x k, Y is N x k); conjugate 1 takes conj(K) / K^H. */
int clcg_hip_dense_matmat(lcg_hip_dense_t K, int k, const double *X, double *Y, int layout, int conjugate);
/* The operator of the batched complex loops with the sum they take after it: Y = K.X for square K and, with U != NULL, the
 * UNCONJUGATED dots[2 j], dots[2 j + 1] = re, im of sum_i Y_ij U_ij (clcg_dot; host, 2k values, after a stream synchronise; NULL
 * dots = enqueue only).  The sum costs no pass over K: one k-wide launch over Y and U leaves at most 512 partial sums per component,
 * added in a fixed order. */
int clcg_hip_dense_op_multi_dot(lcg_hip_dense_t K, int k, const double *X, double *Y, const double *U, double *dots);
/* The list of the complex k-wide kernel families (index 0, 1, ...; NULL behind the last): k_zdnm_row, k_zdnm_row_split, k_zdnm_col.
 * lcg_hip_dense_multi_last_kernel reports them for a complex handle. */
const char *clcg_hip_dense_multi_kernel_name(int index);
/* Batched complex BiCG-sym and PCG on a square complex128 dense handle: clcg_hip_lbicg_sym_multi / clcg_hip_lpcg_multi's loops,
 * contract and codes, word for word (below), with A = K: the stop rules, both "already optimised" criteria, the NaN rule with PCG's
 * deviation, frozen-means-final, ret / iterations / residual per column, `mem`, 0 when the loop ran.  K is meant to be complex
 * symmetric (not checked).  PCG uses the reciprocals of lcg_hip_dense_build_jacobi(K, 0, ...): none built returns
 * LCG_NULL_PRECONDITION_MATRIX after the parameter checks.  Per iteration K is read once for all k columns.  Column j's results depend
 * on K, the forced variant, column j of B and M and param alone, bit for bit.  lcg_hip_last_launches counts every kernel of the
 * operator (its product, fold and the carried sum) as a product. */
int clcg_hip_dense_lbicg_sym_multi(lcg_hip_dense_t K, int k, double *M, const double *B, const clcg_para *param,
                                   int *ret, int *iterations, double *residual, int mem);
int clcg_hip_dense_lpcg_multi(lcg_hip_dense_t K, int k, double *M, const double *B, const clcg_para *param,
                              int *ret, int *iterations, double *residual, int mem);

/* ---------------------------------------------------------------- kernels */
/* Stand-alone launches of the hot-path kernels on the current stream (device pointers).
 * Scalar results are written to host memory after a stream synchronise. */
int lcg_hip_spmv(lcg_hip_csr_t A, const double *x, double *y);                  /* y = A.x */
/* y = op(A).x, layout 1 = transpose, conjugate 1 = conjugated entries (A^H = both): the
 * MatTranspose / Conjugate products the reference's callbacks are asked for (clcg.h:40-41,
 * clcg.cpp:187; cusparseSpMV with CUSPARSE_OPERATION_*TRANSPOSE in sample9.cu:97). */
int lcg_hip_spmv_op(lcg_hip_csr_t A, const double *x, double *y, int layout, int conjugate);
/* (On a sharded matrix: layout = 1 only -- every rank multiplies the transpose of its rows with its slice of x and
 * ncclReduceScatter sums the contributions into the ranks' row blocks; conj(A).x alone returns LCG_HIP_E_RUNTIME.) */
/* y = A.x together with the sums the Krylov loops take right after it (lcg.cpp:234 d.Ad, :548-552 Ap.r0, :735-740 As.s and
 * As.As): result2[0] = y.u, result2[1] = y.y (host, after a stream synchronise; NULL = enqueue only).  Where the kernel family
 * allows, the sums ride in the product's epilogue (what the built-in solvers use on one GPU: lcg_hip_csr_last_kernel says
 * "carrying the dot"); otherwise product and reduction run as two launches.  Real matrices. */
int lcg_hip_spmv_dot(lcg_hip_csr_t A, const double *x, double *y, const double *u, double *result2);
/* Y = A.X for k = 2, 4 or 8 vectors in ONE launch: col / val are read once for all of them.  A block of k vectors is one array
 * of rows x k doubles, row-major (X[i * k + j] = row i of column j; X: n_cols rows, Y: n_rows), its base 16-byte aligned; other
 * counts are padded with zero columns.  Any other k, a null pointer or a misaligned base: LCG_HIP_E_ARG before the device is
 * touched.  Real fp64 CSR handles on one GPU: complex, complex64, dense and sharded handles return LCG_HIP_E_ARG
 * (lcg_hip_last_error() says why).  Column j's sums are added in an order fixed by the matrix alone: the same bits whatever the
 * other columns hold, whatever k is, from call to call.  Reads the plain CSR arrays: no single-vector plan is built or used. */
int lcg_hip_spmm(lcg_hip_csr_t A, int k, const double *X, double *Y);
/* The same product carrying, per column, the sum the batched loops take right after it (d.Ad): dots[j] = (A.X)_j . U_j, j < k
 * (host, after a stream synchronise).  The sums ride in the product's epilogue as per-workgroup partial sums added in a fixed order. */
int lcg_hip_spmm_dot(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *U, double *dots);
/* The same product carrying TWO sums per column, the ones BiCGStab takes right after its second product (lcg.cpp:733-741, As.s
 * and As.As): dots2[j] = (A.X)_j . U_j and dots2[k + j] = (A.X)_j . (A.X)_j, j < k (host, after a stream synchronise).  dots2[j]
 * has the bits of lcg_hip_spmm_dot's dots[j] for the same inputs; column j's two sums depend on A, X_j and U_j alone, bit for
 * bit, whatever k is and whatever the other columns hold.  Arguments and handles are checked as lcg_hip_spmm_dot's: LCG_HIP_E_ARG
 * before the device is touched, Y untouched. */
int lcg_hip_spmm_dot2(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *U, double *dots2);
/* Batched CG (lcg.cpp:143-274) and PCG with the built-in Jacobi (lcg.cpp:293-434; needs lcg_hip_csr_build_jacobi(A)) over
 * k = 2, 4 or 8 right-hand sides against one real fp64 CSR matrix on one GPU: M (in/out) and B are blocks of k vectors in
 * lcg_hip_spmm's layout and live where `mem` says.  Each column runs the reference's recurrence as if it were alone -- its own
 * alpha, beta, stop test, "already optimised" test, NaN scan, count and code -- while one multi-vector product per iteration reads
 * the matrix once for all of them.  A column that has stopped is final: its column of M is not written again.  ret, iterations,
 * residual: host arrays of k (or NULL) receiving each column's liblcg code (LCG_CONVERGENCE, LCG_REACHED_MAX_ITERATIONS,
 * LCG_ALREADY_OPTIMIZIED, LCG_NAN_VALUE), iteration count and residual; lcg_hip_last_iterations / _residual report the column
 * that ran longest.  Returns 0 when the loop ran, whatever the columns' verdicts; LCG_HIP_E_ARG (k, null or misaligned M / B, a
 * complex / complex64 / dense / sharded / non-square handle; before the device is touched), LCG_INVILAD_MAX_ITERATIONS,
 * LCG_INVILAD_EPSILON, LCG_NULL_PRECONDITION_MATRIX (no Jacobi diagonal), or a runtime failure.  No progress callback, no caller
 * workspaces; column j's results depend on A, column j of B and M and param alone, bit for bit. */
int lcg_hip_lcg_multi(lcg_hip_csr_t A, int k, double *M, const double *B, const lcg_para *param,
                      int *ret, int *iterations, double *residual, int mem);
int lcg_hip_lpcg_multi(lcg_hip_csr_t A, int k, double *M, const double *B, const lcg_para *param,
                       int *ret, int *iterations, double *residual, int mem);
/* The handle's IC(0) / ILU(0) factor applied to a block of k = 2, 4 or 8 vectors (lcg_hip_spmm's layout): which = 0 L^-1,
 * 1 L^-T (IC) / U^-1 (ILU), 2 both.  The apply follows lcg_hip_csr_{ic0,ilu0}_set_sweeps: exact level-scheduled solves, or s
 * Jacobi sweeps per triangle, each sweep ONE launch that reads the triangle once for all k columns.  Column j has the bits of
 * lcg_hip_ic0_solve / lcg_hip_ilu0_solve on column j alone, whatever the other columns hold (NaN and Inf included), whatever k
 * is, from call to call.  The k-wide work vectors belong to the factor: the first call at a k larger than any before may
 * allocate and wait, later ones only launch; lcg_hip_csr_{ic0,ilu0}_info's byte count includes them.  LCG_HIP_E_ARG (bad k, null
 * or misaligned block, complex / complex64 / dense / sharded handle, no factor, which outside 0..2, X and Y overlapping) before
 * the device is touched, Y untouched. */
int lcg_hip_ic0_solve_multi (lcg_hip_csr_t A, int k, int which, const double *X, double *Y);
int lcg_hip_ilu0_solve_multi(lcg_hip_csr_t A, int k, int which, const double *X, double *Y);
enum { LCG_HIP_M_JACOBI = 0, LCG_HIP_M_IC0 = 1, LCG_HIP_M_ILU0 = 2 };
/* lcg_hip_lpcg_multi with the preconditioner named: LCG_HIP_M_JACOBI is lcg_hip_lpcg_multi itself, bit for bit; LCG_HIP_M_IC0 /
 * LCG_HIP_M_ILU0 apply the handle's factor k wide at its sweeps setting, between the update pass and the pass of the sums (one
 * apply per iteration for all columns; its launches count as vector passes in lcg_hip_last_launches).  Any other precond:
 * LCG_HIP_E_ARG; no factor (or no Jacobi diagonal): LCG_NULL_PRECONDITION_MATRIX.  Everything else as lcg_hip_lpcg_multi. */
int lcg_hip_lpcg_multi_m(lcg_hip_csr_t A, int k, int precond, double *M, const double *B, const lcg_para *param,
                         int *ret, int *iterations, double *residual, int mem);
enum { LCG_HIP_M_NONE = -1 };   /* no preconditioner (lcg_hip_lbicgstab_multi only) */
/* Batched BiCGStab (lcg.cpp:629-794) over k = 2, 4 or 8 right-hand sides for a square real fp64 CSR matrix on one GPU, symmetric
 * or not; layout, mem, ret / iterations / residual, "returns 0 when the loop ran" and the parameter checks are
 * lcg_hip_lpcg_multi_m's.  Each column runs the reference's recurrence as if it were alone -- its own ak, wk, betak and rkr0_T,
 * r0_T = p = r = B - A.m, both "already optimised" criteria in the reference's order, the stop test at the loop head, the NaN
 * scan of m after the update, its own count and code; a breakdown (Apk.r0_T = 0 or As.As = 0) ends that column alone with
 * LCG_NAN_VALUE.  Schedule, precond = LCG_HIP_M_NONE: two products and three k-wide passes per iteration,
 *     v = A.p carrying v.r0 | [ak] s = r - ak v | t = A.s carrying t.s, t.t | [wk] m += ak p + wk s; r = s - wk t + sums | [close] p = r + betak (p - wk v)
 * LCG_HIP_M_JACOBI / _IC0 / _ILU0: right preconditioning carried in x-space,
 *     ph = M^-1 p; v = A.ph; s = r - ak v; sh = M^-1 s; t = A.sh; m += ak ph + wk sh; r = s - wk t; p = r + betak (p - wk v)
 * so M (the block) holds the solution itself, the stop rule sees |m| and nothing is applied after the loop (the single-vector
 * lcg_hip_csr_ax_ilu0 route iterates on u and needs a final ilu0_solve; this one does not).  In exact arithmetic the residuals are
 * those of A.M^-1 u = b - A.m0 from u = 0, and m = m0 + M^-1 u.  A factor is applied k wide at the handle's sweeps setting, twice
 * per iteration (its launches count as vector passes in lcg_hip_last_launches); the Jacobi multiply rides in the passes that write
 * p and s.  A column that has stopped is final: its columns of m, r, p and s are not stored to again.  NaN count: a column that
 * ends with LCG_NAN_VALUE reports the iteration in which the NaN appeared (t after its t++), as the batched CG does -- one more
 * than the last count the reference's progress callback saw.  Column j's results depend on A, its factor, column j of B and M and
 * param alone, bit for bit: whatever the other columns hold, whatever k is, from call to call.  Any other precond: LCG_HIP_E_ARG;
 * no factor or no Jacobi diagonal: LCG_NULL_PRECONDITION_MATRIX. */
int lcg_hip_lbicgstab_multi(lcg_hip_csr_t A, int k, int precond, double *M, const double *B, const lcg_para *param,
                            int *ret, int *iterations, double *residual, int mem);
/* Y = A.X for k = 2, 4 or 8 COMPLEX vectors in ONE launch against a complex128 CSR handle: col / val (20 bytes per entry) are read
 * once for all of them.  A block of k complex vectors is one array of rows x k interleaved (re, im) pairs, row-major: column j of
 * row i is doubles 2 (i k + j) and 2 (i k + j) + 1 (X: n_cols rows, Y: n_rows), its base 16-byte aligned; other counts are padded
 * with zero columns.  Any other k, a null pointer or a misaligned base: LCG_HIP_E_ARG before the device or the handle is looked at.
 * Complex128 CSR handles on one GPU: real, complex64, dense and sharded handles return LCG_HIP_E_ARG (lcg_hip_last_error() says
 * why), Y untouched; lcg_hip_spmm serves the real ones.  Column j's sums are added in an order fixed by the matrix alone: the same
 * bits whatever the other columns hold (NaN and Inf included), whatever k is, from call to call.  Reads the plain CSR arrays: no
 * single-vector plan is built or used. */
int clcg_hip_spmm(lcg_hip_csr_t A, int k, const double *X, double *Y);
/* The same product carrying, per column, the sum the batched complex loops take right after it (d.Ad): dots[2 j], dots[2 j + 1] =
 * re, im of the UNCONJUGATED sum over i of (A.X)_ij U_ij (clcg_dot, cublasZdotu), j < k (2k doubles on the host, after a stream
 * synchronise).  The sums ride in the product's epilogue as per-workgroup partial sums added in a fixed order: column j's sum
 * depends on A, X_j and U_j alone, bit for bit. */
int clcg_hip_spmm_dot(lcg_hip_csr_t A, int k, const double *X, double *Y, const double *U, double *dots);
/* Batched BiCG for complex-symmetric A (clbicg_symmetric, clcg.cpp:228-364) and PCG with the handle's reciprocal Jacobi diagonal
 * (clpcg, clcg_cuda.cu:403-558; needs lcg_hip_csr_build_jacobi(A)) over k = 2, 4 or 8 right-hand sides against one square
 * complex128 CSR matrix on one GPU: M (in/out) and B are blocks of k complex vectors in clcg_hip_spmm's layout and live where `mem`
 * says.  Each column runs the reference's recurrence as if it were alone -- its own ak, bk and rr (PCG: r.s), unconjugated inner
 * products, its own stop test, "already optimised" test, count and code -- while one multi-vector product per iteration reads the
 * matrix once for all of them.  Three launches per iteration:
 *     A.d carrying d.Ad | [ak] m += ak d; r -= ak Ad (PCG: s = r / diag) + sums | [close] d = r + bk d (PCG: s + bk d)
 * BiCG-sym: the 4th-power stop rule of the CPU complex loops, (sum |r|^2)^2 / max((sum |m|^2)^2, 1), or sum |r|^2 / n with
 * abs_diff; both "already optimised" criteria in the reference's order; the NaN scan of m after the update ends that column with
 * CLCG_NAN_VALUE, its count the iteration in which the NaN appeared (t after its t++).  PCG: the real loops' rule, sum |r|^2 /
 * max(sum |m|^2, 1), or sqrt(sum |r|^2) / n with abs_diff, where |m|^2 takes no part ("already optimised" included).  One
 * deliberate deviation: the reference's clpcg and clcg_hip_solver_preconditioned(CLCG_PCG) have no NaN scan and a broken system
 * runs to the cap; in a batch a column whose sum |m|^2, sum |r|^2 or r.s is NaN stops with CLCG_NAN_VALUE at that iteration, as
 * the complex64 loops do -- otherwise one NaN column would keep the batch alive for ever at max_iterations = 0.
 * A column that has stopped is final: its elements of M, r, d and s are not stored to again.  ret, iterations, residual: host
 * arrays of k (or NULL) receiving each column's code (CLCG_CONVERGENCE, LCG_REACHED_MAX_ITERATIONS (-1019, as the complex loops
 * return at the cap), CLCG_ALREADY_OPTIMIZIED, CLCG_NAN_VALUE), iteration count and residual; lcg_hip_last_iterations / _residual
 * report the column that ran longest.  Returns 0 when the loop ran, whatever the columns' verdicts; LCG_HIP_E_ARG (k, null or
 * misaligned M / B, a real / complex64 / dense / sharded / non-square handle; before the device is touched),
 * CLCG_INVILAD_MAX_ITERATIONS, CLCG_INVILAD_EPSILON, LCG_NULL_PRECONDITION_MATRIX (PCG without a Jacobi diagonal), or a runtime
 * failure.  No progress callback, no caller workspaces; column j's iterate, count, residual and code depend on A, its diagonal,
 * column j of B and M and param alone, bit for bit: whatever the other columns hold, whatever k is, from call to call. */
int clcg_hip_lbicg_sym_multi(lcg_hip_csr_t A, int k, double *M, const double *B, const clcg_para *param,
                             int *ret, int *iterations, double *residual, int mem);
int clcg_hip_lpcg_multi(lcg_hip_csr_t A, int k, double *M, const double *B, const clcg_para *param,
                        int *ret, int *iterations, double *residual, int mem);
/* y = op(A).x for a complex64 handle (layout / conjugate as lcg_hip_spmv_op: A, A^T, conj(A), A^H), summed in fp32 as cuSPARSE's
 * CUDA_C_32F (clcg_cudaf.cu's Afp), each row in one fixed order: bit-identical from call to call.  k_c64_rows (W lanes per row,
 * each pair of entries one 16-byte value load and one 8-byte column load, row ends masked by selects) and, for rows of more than max(256, 64 W) entries, k_c64_long (one workgroup per row);
 * chosen at the first product of each form, whose transposed / conjugated copy is built then on the device
 * (lcg_hip_csr_last_kernel names them).  Later calls neither allocate nor synchronise. */
int lcg_hip_spmv_c64(lcg_hip_csr_t A, const float *x, float *y, int layout, int conjugate);
/* Y = A.X for k = 2, 4 or 8 COMPLEX64 vectors in ONE launch against a complex64 CSR handle (lcg_hip_csr_create_c64): col / val (12
 * bytes per entry) are read once for all of them; the batched form of lcg_hip_spmv_c64, summed in fp32 as cuSPARSE's CUDA_C_32F
 * (clcg_cudaf.cu's Afp, :254-401, :403-558).  A block of k complex64 vectors is one array of rows x k interleaved (re, im) float
 * pairs, row-major: column j of row i is floats 2 (i k + j) and 2 (i k + j) + 1 (X: n_cols rows, Y: n_rows), its base 16-byte
 * aligned; other counts are padded with zero columns.  Any other k, a null pointer or a misaligned base: LCG_HIP_E_ARG before the
 * device or the handle is looked at.  Complex64 CSR handles on one GPU: real, complex128, dense and sharded handles return
 * LCG_HIP_E_ARG (lcg_hip_last_error() says why), Y untouched; clcg_hip_spmm serves the complex128 ones.  Per entry acc = a x + acc
 * in fp32 in lcg_hip_spmv_c64's fma order; column j's sums are added in an order fixed by the matrix alone: the same bits whatever
 * the other columns hold (NaN and Inf included), whatever k is, wherever the column stands, from call to call.  Reads the plain
 * CSR arrays: no single-vector plan is built or used. */
int clcg_hip_spmm_c64(lcg_hip_csr_t A, int k, const float *X, float *Y);
/* The same product carrying, per column, the sum the batched complex64 loops take right after it (d.Ad): dots[2 j], dots[2 j + 1] =
 * re, im of the UNCONJUGATED sum over i of (A.X)_ij U_ij (cublasCdotu), j < k -- exact fp64 products of the fp32 values, summed in
 * fp64 (2k doubles on the host, after a stream synchronise).  The sums ride in the product's epilogue as per-workgroup partial
 * sums added in a fixed order: column j's sum depends on A, X_j and U_j alone, bit for bit. */
int clcg_hip_spmm_dot_c64(lcg_hip_csr_t A, int k, const float *X, float *Y, const float *U, double *dots);
/* Batched BiCG for complex-symmetric A (clbicg_symmetric, clcg_cudaf.cu:254-401) and PCG with the handle's reciprocal Jacobi
 * diagonal (clpcg, clcg_cudaf.cu:403-558; needs lcg_hip_csr_build_jacobi(A)) over k = 2, 4 or 8 right-hand sides against one
 * square complex64 CSR matrix on one GPU: M (in/out) and B are blocks of k complex64 vectors in clcg_hip_spmm_c64's layout and live
 * where `mem` says.  Each column runs clcg_hip_solver_c64's / clcg_hip_solver_preconditioned_c64's recurrence as if it were alone
 * -- fp32 vectors and scalars, every dot and norm an fp64 sum of exact products rounded to fp32 once, its own ak, bk and rho,
 * unconjugated inner products, its own stop test, "already optimised" test, count and code -- while one multi-vector product per
 * iteration reads the matrix once for all of them.  Three launches per iteration:
 *     A.d carrying d.Ad | [ak] m += ak d; r -= ak Ad (PCG: s = inv .* r) + sums | [close] d = r + bk d (PCG: s + bk d)
 * Stop rule of both: |r|^2 / max(|m|, 1)^2 in fp32, or |r| / n with abs_diff ("already optimised" then tests |r| / n only); a
 * column ends with CLCG_NAN_VALUE at the first iteration whose sum |m|^2 or |r|^2 is NaN.  A column that has stopped is final: its
 * elements of M, r, d and s are not stored to again.  ret, iterations, residual: host arrays of k (or NULL) receiving each column's
 * code (CLCG_CONVERGENCE, LCG_REACHED_MAX_ITERATIONS (-1019, as the complex loops return at the cap), CLCG_ALREADY_OPTIMIZIED,
 * CLCG_NAN_VALUE), iteration count and residual; lcg_hip_last_iterations / _residual report the column that ran longest.  Returns 0
 * when the loop ran, whatever the columns' verdicts; LCG_HIP_E_ARG (k, null or misaligned M / B, a real / complex128 / dense /
 * sharded / non-square handle; before the device is touched), CLCG_INVILAD_MAX_ITERATIONS, CLCG_INVILAD_EPSILON,
 * LCG_NULL_PRECONDITION_MATRIX (PCG without a Jacobi diagonal), or a runtime failure.  No progress callback, no caller workspaces;
 * column j's iterate, count, residual and code depend on A, its diagonal, column j of B and M and param alone, bit for bit:
 * whatever the other columns hold, whatever k is, from call to call. */
int clcg_hip_lbicg_sym_multi_c64(lcg_hip_csr_t A, int k, float *M, const float *B, const clcg_para *param,
                                 int *ret, int *iterations, double *residual, int mem);
int clcg_hip_lpcg_multi_c64(lcg_hip_csr_t A, int k, float *M, const float *B, const clcg_para *param,
                            int *ret, int *iterations, double *residual, int mem);
int lcg_hip_dot(int n, const double *a, const double *b, double *result);      /* lcg_dot, algebra.cpp:154-163; cublasDdot lcg_cuda.cu:187 */
int lcg_hip_nrm2(int n, const double *a, double *result);                      /* cublasDznrm2-style 2-norm */
int lcg_hip_axpy(int n, double alpha, const double *x, double *y);             /* y += alpha*x, cublasDaxpy lcg_cuda.cu:190 */
int lcg_hip_scal(int n, double alpha, double *x);                              /* cublasDscal lcg_cuda.cu:203 */
int lcg_hip_set2box(int n, const double *low, const double *hig, double *a);    /* a = clamp(a): lcg_set2box_cuda, algebra_cuda.cu:26-38,79-85 */
int lcg_hip_vecmul(int n, const double *a, const double *b, double *c);        /* lcg_vecMvecD_element_wise, algebra_cuda.cu:59-67 */
int lcg_hip_vecdiv(int n, const double *a, const double *b, double *c);        /* lcg_vecDvecD_element_wise, algebra_cuda.cu:69-77 */
int clcg_hip_dot(int n, const double *a, const double *b, double *result2);    /* clcg_dot (unconjugated), lcg_complex.cpp:143-154 */
int clcg_hip_inner(int n, const double *a, const double *b, double *result2);  /* clcg_inner (conj a), lcg_complex.cpp:156-167 */
int clcg_hip_axpy(int n, const double *alpha2, const double *x, double *y);    /* cublasZaxpy clcg_cuda.cu */
int clcg_hip_vecdiv(int n, const double *a, const double *b, double *c);       /* clcg_vecDvecZ_element_wise, lcg_complex_cuda.cu:95-103 */

/* ----------------------------------------------------- synthetic systems */
/* The benchmark family of BASELINE.json configs 2-5 (definition: DESIGN.md, CPU twin:
 * oracle/csr_oracle.c).  Rows [r0,r1) of the n-row matrix are generated on the device with
 * GLOBAL column indices. band > 0: banded variant, band == 0: scrambled affine maps. */
int lcg_hip_csr_generate(lcg_hip_csr_t *A, int64_t n, int npairs, int64_t band, int symmetric,
                         uint64_t seed, double diag_shift, int64_t r0, int64_t r1);
/* The same family with the column pattern named (twin: orc_gen_init_ex):
 *   LCG_HIP_GEN_SCRAMBLED        columns (a_k*i + c_k) mod n and the inverse maps: anywhere in the matrix
 *   LCG_HIP_GEN_DIAGONALS        columns i +- c_k, the SAME npairs offsets c_k <= band in every row
 *                                (2*npairs constant diagonals: a DIA matrix stored as CSR)
 *   LCG_HIP_GEN_ROW_RANDOM_BAND  every row draws its own columns inside (i - band, i + band): rows are cut into
 *                                blocks of the largest power of two <= band/2 and map k sends block b onto block
 *                                b+1 by a keyed bijection of the in-block position (so the mirror entry is
 *                                computable and A stays symmetric without a transpose) */
enum { LCG_HIP_GEN_SCRAMBLED = 0, LCG_HIP_GEN_DIAGONALS = 1, LCG_HIP_GEN_ROW_RANDOM_BAND = 2 };
int lcg_hip_csr_generate_ex(lcg_hip_csr_t *A, int64_t n, int npairs, int pattern, int64_t band, int symmetric,
                            uint64_t seed, double diag_shift, int64_t r0, int64_t r1);
int lcg_hip_gen_xtrue(int64_t n, uint64_t seed, int64_t r0, int64_t r1, double *x_dev);
/* 5-point Laplacian on an nx x ny grid (BASELINE.json config 2), rows [r0,r1). */
int lcg_hip_csr_laplace2d(lcg_hip_csr_t *A, int nx, int ny, int64_t r0, int64_t r1);

/* ------------------------------------------------------------ multi-GPU */
/* One process per GPU.  The row range [r0,r1) of every vector and of A lives on this rank;
 * A.x all-gathers x over RCCL, every inner product is summed with an RCCL all-reduce
 * (nothing comparable exists in the reference: SURVEY.md sections 2 #22-23, 8e).
 * Rendezvous: rank 0 calls lcg_hip_comm_unique_id(), ships the 128 bytes to the other
 * ranks by any means (e.g. a torch.distributed broadcast), then all call comm_init. */
int lcg_hip_comm_unique_id(void *id128);
int lcg_hip_comm_init(int nranks, int rank, const void *id128);
int lcg_hip_comm_destroy(void);
int lcg_hip_comm_rank(void);
int lcg_hip_comm_size(void);
/* Path of the shared object the collectives were bound from ("" before the first lcg_hip_comm_* call).  By default the copy of
 * librccl already mapped into the process (the host program's), else librccl.so from the loader's path; LCG_HIP_RCCL_LIB=<path>
 * binds exactly that file instead, privately (a site's own RCCL build; tests/fake_rccl for several ranks on one GPU). */
const char *lcg_hip_comm_library(void);
/* Bind a row shard (created with GLOBAL column indices over n_global columns) to the
 * communicator: splits it into local-column and remote-column parts and sizes the gather
 * buffer.  rows_per_rank = ceil(n_global / nranks); rank r owns rows
 * [r*rows_per_rank, min(n_global,(r+1)*rows_per_rank)).  mode: 0 all-gather, 1 neighbour
 * (halo) exchange of only the referenced entries (both RCCL, on a second stream beside the
 * local product), 2 direct neighbour exchange: needs the mailboxes (lcg_hip_p2p_*), uses no
 * collective call and no second stream -- the owner's A.x kernel carries a few extra blocks that
 * write its boundary entries of x into the neighbours' receive buffers over the peer mappings
 * and raise a flag there; the neighbours' remote-column product waits for that flag.  At most 8
 * neighbours per rank; returns LCG_HIP_E_COMM on EVERY rank when any rank cannot set it up, so
 * that all of them can fall back to mode 1 or 0 together. */
int lcg_hip_csr_distribute(lcg_hip_csr_t A, int64_t n_global, int mode);
/* x entries this rank receives per A.x under the chosen mode (plan volume, for reporting). */
int64_t lcg_hip_csr_exchange_volume(lcg_hip_csr_t A);
int lcg_hip_allreduce_sum(double *dev_values, int count);
int lcg_hip_barrier(void);
/* Direct all-reduce over xGMI peer mappings (optional; RCCL stays the fallback and the courier
 * of x).  The <= 8 sums of a sync point are a latency problem, not a bandwidth one: every rank
 * owns a small uncached mailbox in its HBM, maps every peer's mailbox through HIP IPC, and the
 * scalar kernel of a sync point writes its sums straight into all peers' mailboxes, waits for
 * theirs and adds them in rank order -- reduce, exchange and scalar step in ONE kernel instead
 * of reduce | ncclAllReduce | scalar step, and the same bits on every rank.
 *   lcg_hip_p2p_export   allocate my mailbox, return its 64-byte IPC handle
 *   lcg_hip_p2p_connect  handles = nranks x 64 bytes in rank order (shipped like the unique id)
 *   lcg_hip_p2p_selftest `rounds` all-reduces of known values with a short timeout; 0 = all correct
 *   lcg_hip_p2p_enable   route the solvers' sync points (and lcg_hip_allreduce_sum) through it;
 *                        the caller makes sure all ranks pass the same value
 *   lcg_hip_p2p_status   0 = not connected, 1 = connected, 2 = enabled, -1 = an exchange timed out
 *                        (synchronises the stream; the path must not be used any more)
 * A contribution that does not arrive within the timeout (default 20 s, LCG_HIP_P2P_TIMEOUT_MS)
 * ends the solve on every rank with LCG_HIP_E_COMM instead of hanging. */
#define LCG_HIP_P2P_HANDLE_BYTES 64
int lcg_hip_p2p_export(void *handle64);
int lcg_hip_p2p_connect(int nranks, int rank, const void *handles);
int lcg_hip_p2p_selftest(int rounds);
int lcg_hip_p2p_enable(int on);
int lcg_hip_p2p_status(void);
/* Time-out of the waits on peer data (mailbox sums at once; a matrix's direct exchange from its next
 * lcg_hip_csr_distribute(A, n, 2) on): short while a node's links are being probed, long in production. */
int lcg_hip_p2p_set_timeout_ms(int ms);
int lcg_hip_p2p_disconnect(void);
/* Test hooks for the sharded product on ONE GPU: split a shard as rank `rank` of `nranks`
 * with no communicator; the caller fills the other ranks' slices of the gather buffer
 * (lcg_hip_csr_xfull) itself and then calls lcg_hip_spmv. */
int lcg_hip_csr_split_for_test(lcg_hip_csr_t A, int64_t n_global, int nranks, int rank);
double *lcg_hip_csr_xfull(lcg_hip_csr_t A);
/* Measurement hook: ONE PART of a sharded product alone (stream-ordered like the product; collective for part 1) -- 1: the x exchange
 * of modes 0 / 1 on the second stream, fork and join included; 2: the local-column product; 4: the remote-column part out of whatever
 * the gather buffer holds.  bench.py's comm_probe times them so that a multi-GPU line says where an iteration goes. */
int lcg_hip_csr_ax_part_for_probe(lcg_hip_csr_t A, const double *x, double *y, int part);
/* After split_for_test and after filling the gather buffer: run the direct exchange (mode 2) with
 * this rank standing in for its neighbours -- the real kernel chain (pushing blocks in the A.x grid,
 * flags, waiting remote-column product) on one GPU, with the true product as result. */
int lcg_hip_csr_direct_selfloop_for_test(lcg_hip_csr_t A, int nranks, int rank);
int64_t lcg_hip_csr_local_nnz(lcg_hip_csr_t A);
int lcg_hip_csr_need_ranges_for_test(lcg_hip_csr_t A, int nranks, int64_t *lohi /* [2*nranks] */);

#ifdef __cplusplus
}
#endif
#endif /* LCG_HIP_H */
