// solvers_c64.hip -- device-resident complex64 BiCG, BiCG-symmetric and PCG: clcg_cudaf.cu's three loops (clbicg :86-252,
// clbicg_symmetric :254-401, clpcg :403-558).
//
// Vectors are interleaved (re, im) floats; the scalars the reference holds as float (ak, betak, the norms, the residual) are
// computed in fp32 on the device and kept in DevState's double slots (exactly representable there).  Dots and norms (cublasCdotc /
// Cdotu / Scnrm2) take exact fp64 products, sum them in fp64 in the fixed tree every reducing pass uses (devcommon.hpp: k_vec,
// reduce_partials), and are rounded to fp32 once, in the scalar step: the same bits from run to run, and a stop test that does not
// wobble with the reduction order.  The vector updates (cublasCaxpy, Cscal) are fp32.
//
// Stop rule, as clcg_cudaf.cu: residual = |r|^2 / max(|m|, 1)^2 in fp32 (|.| the rounded 2-norms), or |r| / n with abs_diff.
// Under abs_diff the reference's "already optimised" test reads m_mod uninitialised (:162); here, as in the c128 clpcg port
// (solvers_cplx.hip: FinZPcg, citing clcg_cuda.cu:456-466), abs_diff tests |r| / n only.  The reference loops have no NaN scan
// and spin to the cap (for ever with max_iterations = 0) after a breakdown; these stop at the first iteration whose |m|^2 or |r|^2
// is NaN with CLCG_NAN_VALUE, as the c128 loops do (the sums are there anyway: no extra pass).
//
// Kernel functors carry a C64 prefix: k_vec / k_scal are instantiated per translation unit (tests/test_abi.py).
#include <functional>

#include "c64common.hpp"
#include "driver.hpp"

namespace lcgh {

enum { F_AK = 0, F_BK = 2, F_RHO = 4, F_RK = 6, F_MM = 7 };     // DevState::s slots (complex values take two)

__device__ __forceinline__ float2 fld(const float *p, long i) { return reinterpret_cast<const float2 *>(p)[i]; }
__device__ __forceinline__ void fst(float *p, long i, float2 v) { reinterpret_cast<float2 *>(p)[i] = v; }
__device__ __forceinline__ float2 fget(const DevState *st, int k) { return make_float2((float)st->s[k], (float)st->s[k + 1]); }
__device__ __forceinline__ void fput(DevState *st, int k, float2 v) { st->s[k] = v.x; st->s[k + 1] = v.y; }
__device__ __forceinline__ float2 fconj(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float2 fneg(float2 a) { return make_float2(-a.x, -a.y); }
__device__ __forceinline__ float2 fmul(float2 a, float2 b) { return c64_mul(a, b); }
__device__ __forceinline__ float2 faxpy(float2 a, float2 x, float2 y)     // y + a x  (cublasCaxpy)
{
    const float2 p = fmul(a, x);
    return make_float2(y.x + p.x, y.y + p.y);
}
__device__ __forceinline__ float2 fdiv(float2 a, float2 b) { return c64_div(a, b); }     // cuCdivf's scaled formula
// fp64 accumulation of exact products of fp32 values
__device__ __forceinline__ void f_acc_norm(double *acc, float2 a) { *acc += (double)a.x * a.x + (double)a.y * a.y; }
__device__ __forceinline__ void f_acc_dotu(double *acc, float2 a, float2 b)       // a.b        (cublasCdotu)
{
    acc[0] += (double)a.x * b.x - (double)a.y * b.y;
    acc[1] += (double)a.x * b.y + (double)a.y * b.x;
}
__device__ __forceinline__ void f_acc_dotc(double *acc, float2 a, float2 b)       // conj(a).b  (cublasCdotc)
{
    acc[0] += (double)a.x * b.x + (double)a.y * b.y;
    acc[1] += (double)a.x * b.y - (double)a.y * b.x;
}
// the reference's float scalars from the fp64 sums: rounded once
__device__ __forceinline__ float f_nrm(double s) { return (float)sqrt(s); }
__device__ __forceinline__ float2 f_cplx(const double *s) { return make_float2((float)s[0], (float)s[1]); }
__device__ __forceinline__ float f_resid(const DevState *st, float rk, float mm)
{
    return st->abs_diff ? rk / (float)st->n_global : rk * rk / (mm * mm);
}
// sums[0] = |m|^2, sums[1] = |r|^2: m_mod (clamped at 1 as :146) and rk_mod into their slots; the residual they give
__device__ __forceinline__ float f_norms(DevState *st, const double *sum)
{
    float mm = f_nrm(sum[0]);
    if (mm < 1.0f) mm = 1.0f;
    const float rk = f_nrm(sum[1]);
    st->s[F_MM] = mm; st->s[F_RK] = rk;
    return f_resid(st, rk, mm);
}

// ---- scalar steps --------------------------------------------------------------------------------
struct FinC64Init {         // sums: |m|^2, |r|^2, rho (2): the already-optimised test (:153-171)
    static constexpr int NR = 4;
    __device__ void operator()(DevState *st, const double *sum) const
    {
        const float r = f_norms(st, sum);
        fput(st, F_RHO, f_cplx(sum + 2));
        st->residual = r;
        if (r <= st->eps) { st->done = 1; st->status = ST_ALREADY; }
        publish(st);
    }
};
struct FinC64Alpha {        // ak = rho / sum (cuCdivf); the first scalar step of a body: counts it
    static constexpr int NR = 2;
    __device__ void operator()(DevState *st, const double *sum) const
    {
        st->it++;
        if (st->done) return;
        fput(st, F_AK, fdiv(fget(st, F_RHO), f_cplx(sum)));
    }
};
struct FinC64Close {        // sums: |m|^2, |r|^2, rho_new (2): betak = new / old, rho = new, t++, the stop test of the next loop head
    static constexpr int NR = 4;
    __device__ void operator()(DevState *st, const double *sum) const
    {
        if (!st->done && (sum[0] != sum[0] || sum[1] != sum[1])) {      // a NaN in m or r (a breakdown: rho or the step's dot 0)
            st->t++; st->done = 1; st->status = ST_NAN;
        } else if (!st->done) {
            const float r = f_norms(st, sum);
            const float2 nw = f_cplx(sum + 2);
            fput(st, F_BK, fdiv(nw, fget(st, F_RHO)));
            fput(st, F_RHO, nw);
            st->t++;
            st->residual = r;
            if (r <= st->eps) { st->done = 1; st->status = ST_CONVERGED; }
        }
        publish(st);
    }
};

// ---- passes ---------------------------------------------------------------------------------------
template <bool CONJ>
struct OpC64Dot {           // acc = conj(a).b (CONJ, Cdotc) or a.b (Cdotu)
    static constexpr int NR = 2, SKIP = SKIP_DONE;
    DevState *st; const float *a, *b;
    __device__ void prep() {}
    template <class T> __device__ void apply(long i, double *acc)
    {
        if (CONJ) f_acc_dotc(acc, fld(a, i), fld(b, i)); else f_acc_dotu(acc, fld(a, i), fld(b, i));
    }
};
struct OpC64Xpay {          // d = b d + r   (Cscal + Caxpy: :381-382, :536-537)
    static constexpr int NR = 0, SKIP = SKIP_DIR;
    DevState *st; float *d; const float *r; float2 bk;
    __device__ void prep() { bk = fget(st, F_BK); }
    template <class T> __device__ void apply(long i, double *)
    {
        const float2 bd = fmul(bk, fld(d, i)), rv = fld(r, i);
        fst(d, i, make_float2(bd.x + rv.x, bd.y + rv.y));
    }
};

// BiCG-symmetric (:254-401)
struct OpC64SymInit {       // r = B - Ax; d = r; |m|^2, |r|^2, r.r   (:293-311)
    static constexpr int NR = 4, SKIP = SKIP_NEVER;
    DevState *st; const float *Ax, *B, *m; float *r, *d;
    __device__ void prep() {}
    template <class T> __device__ void apply(long i, double *acc)
    {
        const float2 rv = faxpy(make_float2(-1.f, 0.f), fld(Ax, i), fld(B, i));
        fst(r, i, rv); fst(d, i, rv);
        f_acc_norm(acc, fld(m, i)); f_acc_norm(acc + 1, rv);
        f_acc_dotu(acc + 2, rv, rv);
    }
};
struct OpC64Update {        // m += ak d; r -= ak Ax; |m|^2, |r|^2, r.r (:366-377) or, with z, r.z after z = inv .* r (clpcg, built-in Jacobi)
    static constexpr int NR = 4, SKIP = SKIP_DONE;
    DevState *st; float *m, *r, *z; const float *d, *Ax, *inv; float2 ak;
    __device__ void prep() { ak = fget(st, F_AK); }
    template <class T> __device__ void apply(long i, double *acc)
    {
        const float2 mv = faxpy(ak, fld(d, i), fld(m, i));
        const float2 rv = faxpy(fneg(ak), fld(Ax, i), fld(r, i));
        fst(m, i, mv); fst(r, i, rv);
        f_acc_norm(acc, mv); f_acc_norm(acc + 1, rv);
        if (z) {
            const float2 zv = fmul(fld(inv, i), rv);
            fst(z, i, zv);
            f_acc_dotu(acc + 2, rv, zv);
        } else {
            f_acc_dotu(acc + 2, rv, rv);
        }
    }
};

// BiCG (:86-252): the callback is asked for A^H.x (:217)
struct OpC64BicgInit {      // r1 = B - Ax; d1 = r1; r2 = d2 = conj(r1); |m|^2, |r1|^2, <r2, r1>   (:129-150)
    static constexpr int NR = 4, SKIP = SKIP_NEVER;
    DevState *st; const float *Ax, *B, *m; float *r1, *r2, *d1, *d2;
    __device__ void prep() {}
    template <class T> __device__ void apply(long i, double *acc)
    {
        const float2 rv = faxpy(make_float2(-1.f, 0.f), fld(Ax, i), fld(B, i)), rc = fconj(rv);
        fst(r1, i, rv); fst(d1, i, rv); fst(r2, i, rc); fst(d2, i, rc);
        f_acc_norm(acc, fld(m, i)); f_acc_norm(acc + 1, rv);
        f_acc_dotc(acc + 2, rc, rv);
    }
};
struct OpC64BicgUpd1 {      // m += ak d1; r1 -= ak Ax   (:206-207)
    static constexpr int NR = 0, SKIP = SKIP_DONE;
    DevState *st; float *m, *r1; const float *d1, *Ax; float2 ak;
    __device__ void prep() { ak = fget(st, F_AK); }
    template <class T> __device__ void apply(long i, double *)
    {
        fst(m, i, faxpy(ak, fld(d1, i), fld(m, i)));
        fst(r1, i, faxpy(fneg(ak), fld(Ax, i), fld(r1, i)));
    }
};
struct OpC64BicgUpd2 {      // r2 += conj(-ak) A^H d2; |m|^2, |r1|^2, <r2, r1>   (:209-221)
    static constexpr int NR = 4, SKIP = SKIP_DONE;
    DevState *st; float *r2; const float *AHd, *m, *r1; float2 cak;
    __device__ void prep() { cak = fconj(fneg(fget(st, F_AK))); }
    template <class T> __device__ void apply(long i, double *acc)
    {
        const float2 r2v = faxpy(cak, fld(AHd, i), fld(r2, i));
        fst(r2, i, r2v);
        f_acc_norm(acc, fld(m, i)); f_acc_norm(acc + 1, fld(r1, i));
        f_acc_dotc(acc + 2, r2v, fld(r1, i));
    }
};
struct OpC64BicgDir {       // d1 = b d1 + r1; d2 = conj(b) d2 + r2   (:226-230)
    static constexpr int NR = 0, SKIP = SKIP_DIR;
    DevState *st; float *d1, *d2; const float *r1, *r2; float2 bk;
    __device__ void prep() { bk = fget(st, F_BK); }
    template <class T> __device__ void apply(long i, double *)
    {
        const float2 a = fmul(bk, fld(d1, i)), b = fmul(fconj(bk), fld(d2, i)), r1v = fld(r1, i), r2v = fld(r2, i);
        fst(d1, i, make_float2(a.x + r1v.x, a.y + r1v.y));
        fst(d2, i, make_float2(b.x + r2v.x, b.y + r2v.y));
    }
};

// PCG for complex-symmetric A (:403-558)
struct OpC64Resid {         // r = B - Ax   (:445-449)
    static constexpr int NR = 0, SKIP = SKIP_NEVER;
    DevState *st; const float *Ax, *B; float *r;
    __device__ void prep() {}
    template <class T> __device__ void apply(long i, double *) { fst(r, i, faxpy(make_float2(-1.f, 0.f), fld(Ax, i), fld(B, i))); }
};
template <int SKIPMODE>
struct OpC64PcgSums {       // |m|^2, |r|^2, r.s   (:454-464, :521-532)
    static constexpr int NR = 4, SKIP = SKIPMODE;
    DevState *st; const float *m, *r, *s;
    __device__ void prep() {}
    template <class T> __device__ void apply(long i, double *acc)
    {
        const float2 rv = fld(r, i);
        f_acc_norm(acc, fld(m, i)); f_acc_norm(acc + 1, rv);
        f_acc_dotu(acc + 2, rv, fld(s, i));
    }
};

// ---- host side -------------------------------------------------------------------------------------
static int c64_check_args(const clcg_para &p, int n, const float *m, const float *B)
{   // clcg_cudaf.cu:94-101 (and twins :262-269, :409-416), in that order
    if (n <= 0) return CLCG_INVILAD_VARIABLE_SIZE;
    if (p.max_iterations < 0) return CLCG_INVILAD_MAX_ITERATIONS;
    if (p.epsilon <= 0.0 || p.epsilon >= 1.0) return CLCG_INVILAD_EPSILON;
    if (m == nullptr || B == nullptr) return CLCG_INVALID_POINTER;
    return 0;
}

// One complex64 solve's plumbing: driver.hpp's Solve with float vectors and the _c64 callback types.
struct C64Solve {
    Ctx &c;
    HostBridge hb;
    Workspace ws;
    Driver drv;
    clcg_para para; void *inst; clcg_hip_axfunc_c64_ptr Afp; clcg_hip_progress_c64_ptr Pfp;
    int n;
    size_t nb;              // bytes of one vector
    float *m = nullptr;
    C64Solve(const clcg_para &p, int n_, void *inst_, clcg_hip_axfunc_c64_ptr A, clcg_hip_progress_c64_ptr P)
        : c(ctx()), drv(c, n_, true, p.max_iterations, p.epsilon, p.abs_diff), para(p), inst(inst_), Afp(A), Pfp(P), n(n_),
          nb(sizeof(float) * 2 * (size_t)n_)
    { drv.user_cb = A != clcg_hip_csr_ax_c64; }
    int open(int mem, float *&m_, const float *&B)
    {
        double *md = reinterpret_cast<double *>(m_);
        const double *bd = reinterpret_cast<const double *>(B);
        TRY(hb.open(mem, md, bd, nb, c.stream));
        m_ = reinterpret_cast<float *>(md); B = reinterpret_cast<const float *>(bd); m = m_;
        return 0;
    }
    int get(float *&out) { double *p = nullptr; TRY(ws.get(p, nullptr, nb)); out = reinterpret_cast<float *>(p); return 0; }
    int start() { return drv.init_state(global_rows_of(c, n, (const void *)Afp, inst)); }
    int finish(int rc) { const int rc2 = hb.close(c.stream); return rc <= -2000 ? rc : (rc2 ? rc2 : rc); }
    int axop(const float *x, float *y, int layout, int conj) { return drv.timed_ax([&] { Afp(inst, x, y, n, layout, conj); }); }
    int ax(const float *x, float *y) { return axop(x, y, 0, 0); }
    int run_loop(const std::function<int()> &body)
    {
        auto pfp = [&](double resid, int t) -> int { return Pfp(inst, m, (float)resid, &para, n, t); };
        return drv.run(body, Pfp != nullptr, pfp, LCG_REACHED_MAX_ITERATIONS, CLCG_NAN_VALUE);
    }
};

static int solve_c64_bicg(clcg_hip_axfunc_c64_ptr Afp, clcg_hip_progress_c64_ptr Pfp, float *m, const float *B, int n,
                          const clcg_para *param, void *inst, int mem)
{
    const clcg_para p = param ? *param : clcg_hip_default_parameters();
    TRY(c64_check_args(p, n, m, B));
    if (Afp == nullptr) return CLCG_INVALID_POINTER;
    TRY(ensure_init());
    C64Solve k(p, n, inst, Afp, Pfp);
    TRY(k.open(mem, m, B));
    float *r1, *r2, *d1, *d2, *Ax;
    TRY(k.get(r1)); TRY(k.get(r2)); TRY(k.get(d1)); TRY(k.get(d2)); TRY(k.get(Ax));
    TRY(k.start());
    DevState *st = k.c.state;

    TRY(k.ax(m, Ax));                                                   // clcg_cudaf.cu:129
    TRY(k.drv.vec(OpC64BicgInit{st, Ax, B, m, r1, r2, d1, d2}));        // :133-150
    TRY(k.drv.scal(FinC64Init{}));                                      // :153-171
    int rc = k.run_loop([&]() -> int {
        TRY(k.ax(d1, Ax));                                              // :199
        TRY(k.drv.vec(OpC64Dot<true>{st, d2, Ax}));                     // :201
        TRY(k.drv.vecf(FinC64Alpha{}, OpC64BicgUpd1{st, m, r1, d1, Ax, {}}));   // :202-204 | :206-207
        TRY(k.axop(d2, Ax, 1, 1));                                      // :217  A^H.d2
        TRY(k.drv.vec(OpC64BicgUpd2{st, r2, Ax, m, r1, {}}));           // :209-215, :219-221
        TRY(k.drv.vecf(FinC64Close{}, OpC64BicgDir{st, d1, d2, r1, r2, {}}));   // :222-225 | :226-230
        return 0;
    });
    return k.finish(rc);
}

static int solve_c64_bicg_sym(clcg_hip_axfunc_c64_ptr Afp, clcg_hip_progress_c64_ptr Pfp, float *m, const float *B, int n,
                              const clcg_para *param, void *inst, int mem)
{
    const clcg_para p = param ? *param : clcg_hip_default_parameters();
    TRY(c64_check_args(p, n, m, B));
    if (Afp == nullptr) return CLCG_INVALID_POINTER;
    TRY(ensure_init());
    C64Solve k(p, n, inst, Afp, Pfp);
    TRY(k.open(mem, m, B));
    float *r, *d, *Ax;
    TRY(k.get(r)); TRY(k.get(d)); TRY(k.get(Ax));
    TRY(k.start());
    DevState *st = k.c.state;

    TRY(k.ax(m, Ax));                                                   // clcg_cudaf.cu:293
    TRY(k.drv.vec(OpC64SymInit{st, Ax, B, m, r, d}));                   // :297-311
    TRY(k.drv.scal(FinC64Init{}));                                      // :314-332
    int rc = k.run_loop([&]() -> int {
        TRY(k.ax(d, Ax));                                               // :360
        TRY(k.drv.vec(OpC64Dot<false>{st, d, Ax}));                     // :362
        TRY(k.drv.vecf(FinC64Alpha{}, OpC64Update{st, m, r, nullptr, d, Ax, nullptr, {}}));   // :363-364 | :366-377
        TRY(k.drv.vecf(FinC64Close{}, OpC64Xpay{st, d, r, {}}));        // :378-379 | :381-382
        return 0;
    });
    return k.finish(rc);
}

static int solve_c64_pcg(clcg_hip_axfunc_c64_ptr Afp, clcg_hip_axfunc_c64_ptr Mfp, clcg_hip_progress_c64_ptr Pfp, float *m,
                         const float *B, int n, const clcg_para *param, void *inst, int mem)
{
    const clcg_para p = param ? *param : clcg_hip_default_parameters();
    TRY(c64_check_args(p, n, m, B));
    if (Afp == nullptr) return CLCG_INVALID_POINTER;
    if (Mfp == nullptr) return LCG_NULL_PRECONDITION_MATRIX;
    TRY(ensure_init());
    C64Solve k(p, n, inst, Afp, Pfp);
    TRY(k.open(mem, m, B));
    float *r, *d, *s, *Ax;
    TRY(k.get(r)); TRY(k.get(d)); TRY(k.get(s)); TRY(k.get(Ax));
    TRY(k.start());
    DevState *st = k.c.state;
    if (Mfp != clcg_hip_jacobi_mx_c64) k.drv.user_cb = true;
    const float *inv = c64_builtin_invdiag((const void *)Mfp, inst, n);    // built-in Jacobi: z = inv .* r folds into the update pass

    TRY(k.ax(m, Ax));                                                   // clcg_cudaf.cu:445
    TRY(k.drv.vec(OpC64Resid{st, Ax, B, r}));                           // :449
    TRY(k.drv.checked_mx([&] { Mfp(inst, r, d, n, 0, 0); }));           // :451
    TRY(k.drv.vec(OpC64PcgSums<SKIP_NEVER>{st, m, r, d}));              // :454-464
    TRY(k.drv.scal(FinC64Init{}));                                      // :467-485
    int rc = k.run_loop([&]() -> int {
        TRY(k.ax(d, Ax));                                               // :513
        TRY(k.drv.vec(OpC64Dot<false>{st, d, Ax}));                     // :514
        if (inv) {
            TRY(k.drv.vecf(FinC64Alpha{}, OpC64Update{st, m, r, s, d, Ax, inv, {}}));      // :515-516 | :518-532
        } else {
            TRY(k.drv.vecf(FinC64Alpha{}, OpC64BicgUpd1{st, m, r, d, Ax, {}}));            // :515-516 | :518-519
            TRY(k.drv.checked_mx([&] { Mfp(inst, r, s, n, 0, 0); }));   // :529
            TRY(k.drv.vec(OpC64PcgSums<SKIP_DONE>{st, m, r, s}));       // :521-527, :532
        }
        TRY(k.drv.vecf(FinC64Close{}, OpC64Xpay{st, d, s, {}}));        // :533-534 | :536-537  d = b d + s
        return 0;
    });
    return k.finish(rc);
}

} // namespace lcgh

using namespace lcgh;

// clcg_solver_cuda (clcg_cudaf.cu:42-60): CLCG_BICG, CLCG_BICG_SYM; any other id CLCG_UNKNOWN_SOLVER, before the arguments are looked at
extern "C" int clcg_hip_solver_c64(clcg_hip_axfunc_c64_ptr Afp, clcg_hip_progress_c64_ptr Pfp, float *m, const float *B, int n,
                                   const clcg_para *param, void *instance, int solver_id, int mem)
{
    switch (solver_id) {
    case CLCG_BICG: return solve_c64_bicg(Afp, Pfp, m, B, n, param, instance, mem);
    case CLCG_BICG_SYM: return solve_c64_bicg_sym(Afp, Pfp, m, B, n, param, instance, mem);
    default: return CLCG_UNKNOWN_SOLVER;
    }
}

// clcg_solver_preconditioned_cuda (clcg_cudaf.cu:66-84): CLCG_PCG; any other id CLCG_UNKNOWN_SOLVER
extern "C" int clcg_hip_solver_preconditioned_c64(clcg_hip_axfunc_c64_ptr Afp, clcg_hip_axfunc_c64_ptr Mfp, clcg_hip_progress_c64_ptr Pfp,
                                                  float *m, const float *B, int n, const clcg_para *param, void *instance,
                                                  int solver_id, int mem)
{
    if (solver_id != CLCG_PCG) return CLCG_UNKNOWN_SOLVER;
    return solve_c64_pcg(Afp, Mfp, Pfp, m, B, n, param, instance, mem);
}
