// dense.hip -- dense operators: K.x, K^T.x, K^T.K.x on a row-major matrix resident in HBM, and the callbacks that hand
// them to the solver loops (lcg_matvec algebra.cpp:165-193, clcg_matvec lcg_complex.cpp:169-234; CalAx of sample1.cpp:48-53
// and sample3.cpp:44-49).  DESIGN.md section 14.
//
// Storage: one copy, rows padded to whole 16-byte PACKS (two fp64 entries, or one c128 entry), pads zero, 64 bytes of slack
// behind the last row.  Every kernel reads K one pack per lane and load.  No atomics: a product that is cut over workgroups
// leaves one partial per workgroup in a table slot of its own and a fold adds the slots in one fixed order, so every product is
// bit-identical from call to call.
//
//   k_dn_row         y_i = sum_j K(i,j) x_j      W lanes per row (4 .. 64), butterfly sum over the lanes
//   k_dn_row_split   the same with the columns cut into strips over gridDim.y (few rows, long rows) + k_dnm_fold (dense_multi.hip)
//   k_dn_col         y_j = sum_i K(i,j) x_i      a lane owns one pack of columns and walks a strip of rows + k_dnm_fold
//   k_dn_ata1        y = K^T.(K.x) in one pass   a workgroup keeps whole rows in registers between the two products
//                                                (rows of <= 1024 packs); forced to one workgroup: k_dn_ata_small
//
// A handle made by lcg_hip_dense_create_f32 keeps K as fp32, packs of 8 bytes, and runs the *_f32 twin of each kernel: the same body
// text behind ldpack's widening load, under the same plans, so its results are the bits of the fp64 handle of the widened matrix.  The
// twins are copies, not one template over the pack's type: as one template the fp64 kernels compiled to other code.
#include <cmath>
#include <cstring>

#include "dense.hpp"
#include "lcg_hip_staging_dense_f32.h"

namespace lcgh {

static const char *const DN_NAMES[] = {"k_dn_row", "k_dn_row_split", "k_dn_col", "k_dn_ata_two_pass", "k_dn_ata_one_pass",
                                       "k_dn_ata_small"};

// ---- kernels ---------------------------------------------------------------------------------------------------------------
// (ldpack, how a pack arrives: dense.hpp)

// one pack of a row times its entries of x, added to acc: real rows sum into acc.x; complex ones into (re, im)
template <bool CX, bool CONJ>
__device__ __forceinline__ void row_term(double2 &acc, const double2 k, const double *x, int p, int N)
{
    if (CX) {
        const double xr = x[2 * (int64_t)p], xi = x[2 * (int64_t)p + 1];
        if (CONJ) { acc.x += k.x * xr + k.y * xi; acc.y += k.x * xi - k.y * xr; }
        else { acc.x += k.x * xr - k.y * xi; acc.y += k.x * xi + k.y * xr; }
    } else {
        const int j = 2 * p;
        const double x0 = x[j], x1 = j + 1 < N ? x[j + 1] : 0.0;
        acc.x += k.x * x0 + k.y * x1;
    }
}

// Row form.  Row i = blockIdx.x * (256 / W) + tid / W; its lanes take the packs [p0, p1) of strip blockIdx.y, W apart.
// S == 1: out = y.  S > 1: out = the table, slot s at out + s * M values.
template <bool CX, bool CONJ, int W>
__global__ __launch_bounds__(256) void k_dn_row(const double2 *__restrict__ K, int64_t ldp, int M, int N, int NP, int pps,
                                                const double *__restrict__ x, double *__restrict__ out)
{
    const int sub = threadIdx.x % W;
    const int i = blockIdx.x * (256 / W) + threadIdx.x / W;
    const int p0 = blockIdx.y * pps;
    const int p1 = i < M ? min(NP, p0 + pps) : p0;        // (a row beyond M walks nothing but still joins the butterfly)
    const double2 *row = K + (int64_t)min(i, M - 1) * ldp;
    double2 acc = make_double2(0.0, 0.0);
    int p = p0 + sub;
    for (; p + 3 * W < p1; p += 4 * W) {
        const double2 k0 = ldpack(row + p), k1 = ldpack(row + p + W), k2 = ldpack(row + p + 2 * W), k3 = ldpack(row + p + 3 * W);
        row_term<CX, CONJ>(acc, k0, x, p, N);
        row_term<CX, CONJ>(acc, k1, x, p + W, N);
        row_term<CX, CONJ>(acc, k2, x, p + 2 * W, N);
        row_term<CX, CONJ>(acc, k3, x, p + 3 * W, N);
    }
    for (; p < p1; p += W) row_term<CX, CONJ>(acc, ldpack(row + p), x, p, N);
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        acc.x += __shfl_xor(acc.x, o, W);
        if (CX) acc.y += __shfl_xor(acc.y, o, W);
    }
    if (sub == 0 && i < M) {
        const int64_t at = (int64_t)blockIdx.y * M + i;
        if (CX) { out[2 * at] = acc.x; out[2 * at + 1] = acc.y; }
        else out[at] = acc.x;
    }
}

// k_dn_row on fp32 packs (real): the same lanes, packs and order of additions behind the widening load, eight loads in flight
template <int W>
__global__ __launch_bounds__(256) void k_dn_row_f32(const float2 *__restrict__ K, int64_t ldp, int M, int N, int NP, int pps,
                                                    const double *__restrict__ x, double *__restrict__ out)
{
    const int sub = threadIdx.x % W;
    const int i = blockIdx.x * (256 / W) + threadIdx.x / W;
    const int p0 = blockIdx.y * pps;
    const int p1 = i < M ? min(NP, p0 + pps) : p0;        // (a row beyond M walks nothing but still joins the butterfly)
    const float2 *row = K + (int64_t)min(i, M - 1) * ldp;
    double2 acc = make_double2(0.0, 0.0);
    int p = p0 + sub;
    for (; p + 7 * W < p1; p += 8 * W) {
        double2 k[8];
#pragma unroll
        for (int u = 0; u < 8; u++) k[u] = ldpack(row + p + u * W);
#pragma unroll
        for (int u = 0; u < 8; u++) row_term<false, false>(acc, k[u], x, p + u * W, N);
    }
    for (; p + 3 * W < p1; p += 4 * W) {
        const double2 k0 = ldpack(row + p), k1 = ldpack(row + p + W), k2 = ldpack(row + p + 2 * W), k3 = ldpack(row + p + 3 * W);
        row_term<false, false>(acc, k0, x, p, N);
        row_term<false, false>(acc, k1, x, p + W, N);
        row_term<false, false>(acc, k2, x, p + 2 * W, N);
        row_term<false, false>(acc, k3, x, p + 3 * W, N);
    }
    for (; p < p1; p += W) row_term<false, false>(acc, ldpack(row + p), x, p, N);
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        acc.x += __shfl_xor(acc.x, o, W);
    }
    if (sub == 0 && i < M) {
        out[(int64_t)blockIdx.y * M + i] = acc.x;
    }
}

template <bool CX, bool CONJ, bool SQ>
__device__ __forceinline__ void col_term(double2 &acc, const double2 k, const double *x, int i)
{
    if (SQ) { acc.x += k.x * k.x; acc.y += k.y * k.y; return; }
    if (CX) {
        const double xr = x[2 * (int64_t)i], xi = x[2 * (int64_t)i + 1];
        if (CONJ) { acc.x += k.x * xr + k.y * xi; acc.y += k.x * xi - k.y * xr; }
        else { acc.x += k.x * xr - k.y * xi; acc.y += k.x * xi + k.y * xr; }
    } else {
        const double xv = x[i];
        acc.x += k.x * xv; acc.y += k.y * xv;
    }
}

// Column form.  A workgroup owns CW packs of columns (blockIdx.x) and the rows [r0, r0 + rps) (blockIdx.y); thread (cp, rg)
// walks the rows r0 + rg, r0 + rg + RG, ... of pack cp (RG = 256 / CW: every wavefront load is a contiguous run of a row, or of
// a few rows where the rows are short).  The RG sums of a pack are added in rg order, then written to slot blockIdx.y of out
// (n_out doubles per slot; gridDim.y == 1: out = y).  SQ: sum_i K(i,j)^2 (the Jacobi build), x is not read.
template <bool CX, bool CONJ, bool SQ>
__global__ __launch_bounds__(256) void k_dn_col(const double2 *__restrict__ K, int64_t ldp, int M, int N, int NP, int CW, int rps,
                                                const double *__restrict__ x, double *__restrict__ out, int64_t n_out)
{
    __shared__ double2 sh[256];
    const int RG = 256 / CW;
    const int cp = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int p = blockIdx.x * CW + cp;
    const bool live = p < NP;
    const int r0 = blockIdx.y * rps, r1 = min(M, r0 + rps);
    double2 acc = make_double2(0.0, 0.0);
    if (live) {
        const double2 *col = K + p;
        int i = r0 + rg;
        for (; i + 7 * RG < r1; i += 8 * RG) {
            double2 k[8];
#pragma unroll
            for (int u = 0; u < 8; u++) k[u] = ldpack(col + (int64_t)(i + u * RG) * ldp);
#pragma unroll
            for (int u = 0; u < 8; u++) col_term<CX, CONJ, SQ>(acc, k[u], x, i + u * RG);
        }
        for (; i < r1; i += RG) col_term<CX, CONJ, SQ>(acc, ldpack(col + (int64_t)i * ldp), x, i);
    }
    if (RG > 1) {
        sh[threadIdx.x] = acc;
        __syncthreads();
        if (rg == 0)
            for (int g = 1; g < RG; g++) { const double2 v = sh[g * CW + cp]; acc.x += v.x; acc.y += v.y; }
    }
    if (rg == 0 && live) {
        double *o = out + (int64_t)blockIdx.y * n_out;
        const int64_t j = 2 * (int64_t)p;           // c128: the pack's (re, im); fp64: its two columns
        o[j] = acc.x;
        if (CX || j + 1 < N) o[j + 1] = acc.y;
    }
}

// k_dn_col on fp32 packs (real): the same mapping and order behind the widening load, sixteen rows in flight
template <bool SQ>
__global__ __launch_bounds__(256) void k_dn_col_f32(const float2 *__restrict__ K, int64_t ldp, int M, int N, int NP, int CW, int rps,
                                                    const double *__restrict__ x, double *__restrict__ out, int64_t n_out)
{
    constexpr int UN = 16;
    __shared__ double2 sh[256];
    const int RG = 256 / CW;
    const int cp = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int p = blockIdx.x * CW + cp;
    const bool live = p < NP;
    const int r0 = blockIdx.y * rps, r1 = min(M, r0 + rps);
    double2 acc = make_double2(0.0, 0.0);
    if (live) {
        const float2 *col = K + p;
        int i = r0 + rg;
        for (; i + (UN - 1) * RG < r1; i += UN * RG) {
            double2 k[UN];
#pragma unroll
            for (int u = 0; u < UN; u++) k[u] = ldpack(col + (int64_t)(i + u * RG) * ldp);
#pragma unroll
            for (int u = 0; u < UN; u++) col_term<false, false, SQ>(acc, k[u], x, i + u * RG);
        }
        for (; i < r1; i += RG) col_term<false, false, SQ>(acc, ldpack(col + (int64_t)i * ldp), x, i);
    }
    if (RG > 1) {
        sh[threadIdx.x] = acc;
        __syncthreads();
        if (rg == 0)
            for (int g = 1; g < RG; g++) { const double2 v = sh[g * CW + cp]; acc.x += v.x; acc.y += v.y; }
    }
    if (rg == 0 && live) {
        double *o = out + (int64_t)blockIdx.y * n_out;
        const int64_t j = 2 * (int64_t)p;
        o[j] = acc.x;
        if (j + 1 < N) o[j + 1] = acc.y;
    }
}

// K^T.(K.x) in one pass over K (real).  Thread (cp, rg) of a workgroup of BS threads holds the packs cp, cp + CW, ... (U of them)
// of RB rows at a time (rows base + r * RG + rg); the row's t = K(i,:).x is summed over its CW lanes (butterfly inside a wavefront,
// then the row's wavefronts in order through LDS) and goes straight back into acc += K(i,:) t while the row is still in registers.
// Workgroup b walks the row batches b, b + G, ...; at the end its RG sums per column are added in rg order into slot b of out
// (gridDim.x == 1: out = y).
template <int BS, int U, int RB>
__global__ __launch_bounds__(BS) void k_dn_ata1(const double2 *__restrict__ K, int64_t ldp, int M, int N, int NP, int CW,
                                                 const double *__restrict__ x, double *__restrict__ out)
{
    __shared__ double2 sh[BS];
    __shared__ double sw[RB][BS / 64];
    const int RG = BS / CW;
    const int cp = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int wave = threadIdx.x / 64;
    double xa[U], xb[U];
    double2 acc[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int p = cp + u * CW, j = 2 * p;
        xa[u] = p < NP ? x[j] : 0.0;
        xb[u] = p < NP && j + 1 < N ? x[j + 1] : 0.0;
        acc[u] = make_double2(0.0, 0.0);
    }
    const int step = RG * RB;
    for (int64_t base = (int64_t)blockIdx.x * step; base < M; base += (int64_t)gridDim.x * step) {
        double2 k[RB][U];
        double s[RB];
#pragma unroll
        for (int r = 0; r < RB; r++) {
            const int64_t i = base + r * RG + rg;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int p = cp + u * CW;
                k[r][u] = i < M && p < NP ? ldpack(K + i * ldp + p) : make_double2(0.0, 0.0);
            }
        }
#pragma unroll
        for (int r = 0; r < RB; r++) {
            s[r] = 0.0;
#pragma unroll
            for (int u = 0; u < U; u++) s[r] += k[r][u].x * xa[u] + k[r][u].y * xb[u];
        }
        if (CW <= 64) {
            for (int o = CW / 2; o > 0; o >>= 1) {
#pragma unroll
                for (int r = 0; r < RB; r++) s[r] += __shfl_xor(s[r], o, 64);
            }
        } else {
            for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
                for (int r = 0; r < RB; r++) s[r] += __shfl_xor(s[r], o, 64);
            }
            if ((threadIdx.x & 63) == 0) {
#pragma unroll
                for (int r = 0; r < RB; r++) sw[r][wave] = s[r];
            }
            __syncthreads();
            const int wpr = CW / 64, w0 = rg * wpr;
#pragma unroll
            for (int r = 0; r < RB; r++) {
                double t = sw[r][w0];
                for (int w = 1; w < wpr; w++) t += sw[r][w0 + w];
                s[r] = t;
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < RB; r++) {
#pragma unroll
            for (int u = 0; u < U; u++) { acc[u].x += k[r][u].x * s[r]; acc[u].y += k[r][u].y * s[r]; }
        }
    }
    double *o = out + (int64_t)blockIdx.x * N;
#pragma unroll
    for (int u = 0; u < U; u++) {
        double2 a = acc[u];
        if (RG > 1) {
            __syncthreads();
            sh[threadIdx.x] = a;
            __syncthreads();
            if (rg == 0)
                for (int g = 1; g < RG; g++) { const double2 v = sh[g * CW + cp]; a.x += v.x; a.y += v.y; }
        }
        const int p = cp + u * CW, j = 2 * p;
        if (rg == 0 && p < NP) {
            o[j] = a.x;
            if (j + 1 < N) o[j + 1] = a.y;
        }
    }
}

// k_dn_ata1 on fp32 packs: the rows stay floats in registers between the two products (half the registers) and are widened where
// they are used; the same mapping and order
template <int BS, int U, int RB>
__global__ __launch_bounds__(BS) void k_dn_ata1_f32(const float2 *__restrict__ K, int64_t ldp, int M, int N, int NP, int CW,
                                                     const double *__restrict__ x, double *__restrict__ out)
{
    __shared__ double2 sh[BS];
    __shared__ double sw[RB][BS / 64];
    const int RG = BS / CW;
    const int cp = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int wave = threadIdx.x / 64;
    double xa[U], xb[U];
    double2 acc[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int p = cp + u * CW, j = 2 * p;
        xa[u] = p < NP ? x[j] : 0.0;
        xb[u] = p < NP && j + 1 < N ? x[j + 1] : 0.0;
        acc[u] = make_double2(0.0, 0.0);
    }
    const int step = RG * RB;
    for (int64_t base = (int64_t)blockIdx.x * step; base < M; base += (int64_t)gridDim.x * step) {
        float2 k[RB][U];
        double s[RB];
#pragma unroll
        for (int r = 0; r < RB; r++) {
            const int64_t i = base + r * RG + rg;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int p = cp + u * CW;
                k[r][u] = i < M && p < NP ? K[i * ldp + p] : make_float2(0.0f, 0.0f);
            }
        }
#pragma unroll
        for (int r = 0; r < RB; r++) {
            s[r] = 0.0;
#pragma unroll
            for (int u = 0; u < U; u++) { const double2 kk = ldpack(&k[r][u]); s[r] += kk.x * xa[u] + kk.y * xb[u]; }
        }
        if (CW <= 64) {
            for (int o = CW / 2; o > 0; o >>= 1) {
#pragma unroll
                for (int r = 0; r < RB; r++) s[r] += __shfl_xor(s[r], o, 64);
            }
        } else {
            for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
                for (int r = 0; r < RB; r++) s[r] += __shfl_xor(s[r], o, 64);
            }
            if ((threadIdx.x & 63) == 0) {
#pragma unroll
                for (int r = 0; r < RB; r++) sw[r][wave] = s[r];
            }
            __syncthreads();
            const int wpr = CW / 64, w0 = rg * wpr;
#pragma unroll
            for (int r = 0; r < RB; r++) {
                double t = sw[r][w0];
                for (int w = 1; w < wpr; w++) t += sw[r][w0 + w];
                s[r] = t;
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < RB; r++) {
#pragma unroll
            for (int u = 0; u < U; u++) { const double2 kk = ldpack(&k[r][u]); acc[u].x += kk.x * s[r]; acc[u].y += kk.y * s[r]; }
        }
    }
    double *o = out + (int64_t)blockIdx.x * N;
#pragma unroll
    for (int u = 0; u < U; u++) {
        double2 a = acc[u];
        if (RG > 1) {
            __syncthreads();
            sh[threadIdx.x] = a;
            __syncthreads();
            if (rg == 0)
                for (int g = 1; g < RG; g++) { const double2 v = sh[g * CW + cp]; a.x += v.x; a.y += v.y; }
        }
        const int p = cp + u * CW, j = 2 * p;
        if (rg == 0 && p < NP) {
            o[j] = a.x;
            if (j + 1 < N) o[j + 1] = a.y;
        }
    }
}

// z = x .* d (the reciprocal diagonal), n values
template <bool CX>
__global__ __launch_bounds__(256) void k_dn_scale(const double *__restrict__ d, const double *__restrict__ x, double *__restrict__ z, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (CX) {
        const double dr = d[2 * i], di = d[2 * i + 1], xr = x[2 * i], xi = x[2 * i + 1];
        z[2 * i] = dr * xr - di * xi; z[2 * i + 1] = dr * xi + di * xr;
    } else z[i] = d[i] * x[i];
}

// d = the diagonal of a square K
template <bool CX>
__global__ __launch_bounds__(256) void k_dn_diag(const double2 *__restrict__ K, int64_t ldp, int n, double *__restrict__ d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *row = reinterpret_cast<const double *>(K + (int64_t)i * ldp);
    if (CX) { d[2 * i] = row[2 * (int64_t)i]; d[2 * i + 1] = row[2 * (int64_t)i + 1]; }
    else d[i] = row[i];
}
__global__ __launch_bounds__(256) void k_dn_diag_f32(const float2 *__restrict__ K, int64_t ldp, int n, double *__restrict__ d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    d[i] = (double)reinterpret_cast<const float *>(K + (int64_t)i * ldp)[i];
}

// Row i of an fp32 source, ld floats apart, into the handle's packs: thread (i, p) writes pack p of row i, the pad of an odd N as zero.
// (the source is only 4-byte aligned: two scalar loads)
__global__ __launch_bounds__(256) void k_dn_pack_f32(const float *__restrict__ src, int64_t ld, int rows, int N, int NP, float2 *__restrict__ dst,
                                                     int64_t ldp)
{
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (int64_t)rows * NP) return;
    const int64_t i = at / NP;
    const int p = (int)(at - i * NP), j = 2 * p;
    const float *row = src + i * ld;
    dst[i * ldp + p] = make_float2(row[j], j + 1 < N ? row[j + 1] : 0.0f);
}

// ---- plans (pure functions of the shape: the table is sized from them when the handle is made; the row and column plans: dense.hpp)
struct AtaPlan { int BS, U, RB, CW, G; bool ok; };

static AtaPlan ata_plan(int M, int NP, int N, bool small)
{
    AtaPlan a{};
    a.ok = NP <= 1024;
    if (!a.ok) return a;
    if (small) { a.BS = 1024; a.U = 1; a.RB = 2; a.CW = pow2ceil(NP); a.G = 1; return a; }
    a.BS = 256;
    a.U = NP <= 256 ? 1 : NP <= 512 ? 2 : 4;
    a.RB = a.U == 4 ? 2 : 4;
    a.CW = a.U == 1 ? pow2ceil(NP) : 256;
    const int RG = a.BS / a.CW;
    a.G = (int)std::min<int64_t>(cdiv(M, (int64_t)RG * a.RB * 2), 1024);
    return a;
}
// Rows of at most this many entries take the one-pass K^T.K.x (where it measured faster than two passes)
constexpr int ATA1_MAX_N = 2048;
static int64_t table_doubles(int M, int N, int NP, bool cplx)
{
    const int c = cplx ? 2 : 1;
    int64_t need = 0;
    for (int forced = 0; forced < 2; forced++) need = std::max(need, (int64_t)row_plan(M, NP, true, forced).S * M * c);
    need = std::max(need, (int64_t)col_plan(M, NP).RS * N * c);
    if (!cplx && ata_plan(M, NP, N, false).ok) need = std::max(need, (int64_t)ata_plan(M, NP, N, false).G * N);
    return need + 2;
}

// ---- launches --------------------------------------------------------------------------------------------------------------
// the slots of a table added in k_dnm_fold's fixed order (dense_multi.hip: the one fold of the dense units; no batch to stop here)
static void fold_launch(const double *part, int S, int64_t n, double *y, hipStream_t s) { dnm_fold_launch(part, S, n, y, s, nullptr); }

template <bool CX, bool CONJ>
static void row_dispatch(const lcg_hip_dense *K, const RowPlan &r, const double *x, double *out, hipStream_t s)
{
    const dim3 grid((unsigned)cdiv(K->M, 256 / r.W), (unsigned)r.S);
#define DN_ROW_CASE(w) case w: hipLaunchKernelGGL((k_dn_row<CX, CONJ, w>), grid, dim3(256), 0, s, K->val, K->ldp, K->M, K->N, K->NP, r.pps, x, out); break;
    switch (r.W) { DN_ROW_CASE(4) DN_ROW_CASE(8) DN_ROW_CASE(16) DN_ROW_CASE(32) default: DN_ROW_CASE(64) }
#undef DN_ROW_CASE
}
static void row_dispatch_f32(const lcg_hip_dense *K, const RowPlan &r, const double *x, double *out, hipStream_t s)
{
    const dim3 grid((unsigned)cdiv(K->M, 256 / r.W), (unsigned)r.S);
#define DN_ROW_CASE(w) case w: hipLaunchKernelGGL((k_dn_row_f32<w>), grid, dim3(256), 0, s, dn_val32(K), K->ldp, K->M, K->N, K->NP, r.pps, x, out); break;
    switch (r.W) { DN_ROW_CASE(4) DN_ROW_CASE(8) DN_ROW_CASE(16) DN_ROW_CASE(32) default: DN_ROW_CASE(64) }
#undef DN_ROW_CASE
}

// y[M] = K.x or conj(K).x
static int row_product(lcg_hip_dense *K, const double *x, double *y, int conjugate, int variant, hipStream_t s)
{
    const bool forced = variant == DN_ROW_SPLIT;
    const bool split = forced || (variant != DN_ROW && row_split_auto(K->M, K->NP));
    const RowPlan r = row_plan(K->M, K->NP, split, forced);
    double *out = r.S > 1 ? K->part : y;
    if (K->f32) row_dispatch_f32(K, r, x, out, s);
    else if (!K->cplx) row_dispatch<false, false>(K, r, x, out, s);
    else if (conjugate) row_dispatch<true, true>(K, r, x, out, s);
    else row_dispatch<true, false>(K, r, x, out, s);
    if (r.S > 1) fold_launch(K->part, r.S, (int64_t)K->M * (K->cplx ? 2 : 1), y, s);
    K->last_kernel = r.S > 1 ? DN_NAMES[1] : DN_NAMES[0];       // what ran
    return launched("dense row product");
}

// y[N] = K^T.x or K^H.x; sq: y[N] = column sums of squares (real)
static int col_product(lcg_hip_dense *K, const double *x, double *y, int conjugate, bool sq, hipStream_t s)
{
    const ColPlan c = col_plan(K->M, K->NP);
    const int64_t n_out = (int64_t)K->N * (K->cplx ? 2 : 1);
    double *out = c.RS > 1 ? K->part : y;
    const dim3 grid((unsigned)c.CT, (unsigned)c.RS);
#define DN_COL(cx, cj, q) hipLaunchKernelGGL((k_dn_col<cx, cj, q>), grid, dim3(256), 0, s, K->val, K->ldp, K->M, K->N, K->NP, c.CW, c.rps, x, out, n_out)
#define DN_COL32(q) hipLaunchKernelGGL((k_dn_col_f32<q>), grid, dim3(256), 0, s, dn_val32(K), K->ldp, K->M, K->N, K->NP, c.CW, c.rps, x, out, n_out)
    if (K->f32) { if (sq) DN_COL32(true); else DN_COL32(false); }
    else if (sq) DN_COL(false, false, true);
    else if (!K->cplx) DN_COL(false, false, false);
    else if (conjugate) DN_COL(true, true, false);
    else DN_COL(true, false, false);
#undef DN_COL
#undef DN_COL32
    if (c.RS > 1) fold_launch(K->part, c.RS, n_out, y, s);
    if (!sq) K->last_kernel = DN_NAMES[2];
    return launched("dense column product");
}

static int ata_one_pass(lcg_hip_dense *K, const double *x, double *y, bool small, hipStream_t s)
{
    const AtaPlan a = ata_plan(K->M, K->NP, K->N, small);
    double *out = a.G > 1 ? K->part : y;
#define DN_ATA(bs, u, rb) hipLaunchKernelGGL((k_dn_ata1<bs, u, rb>), dim3((unsigned)a.G), dim3(bs), 0, s, K->val, K->ldp, K->M, K->N, K->NP, a.CW, x, out)
#define DN_ATA32(bs, u, rb) hipLaunchKernelGGL((k_dn_ata1_f32<bs, u, rb>), dim3((unsigned)a.G), dim3(bs), 0, s, dn_val32(K), K->ldp, K->M, K->N, K->NP, a.CW, x, out)
    if (K->f32) {
        if (small) DN_ATA32(1024, 1, 2);
        else if (a.U == 1) DN_ATA32(256, 1, 4);
        else if (a.U == 2) DN_ATA32(256, 2, 4);
        else DN_ATA32(256, 4, 2);
    }
    else if (small) DN_ATA(1024, 1, 2);
    else if (a.U == 1) DN_ATA(256, 1, 4);
    else if (a.U == 2) DN_ATA(256, 2, 4);
    else DN_ATA(256, 4, 2);
#undef DN_ATA
#undef DN_ATA32
    if (a.G > 1) fold_launch(K->part, a.G, K->N, y, s);
    K->last_kernel = small ? DN_NAMES[5] : DN_NAMES[4];
    return launched("dense K^T.K.x");
}

static int ata_product(lcg_hip_dense *K, const double *x, double *y, hipStream_t s)
{
    int v = K->variant;
    if (v == DN_ATA1 || v == DN_ATA_SMALL) {
        if (K->NP > 1024) return arg_error("lcg_hip_dense_ata_ax: the one-pass forms keep a row in one workgroup's registers: N <= 2048 (N = %d)", K->N);
        return ata_one_pass(K, x, y, v == DN_ATA_SMALL, s);
    }
    if (v != DN_ATA2) {
        // (the one-workgroup form is never the automatic choice: on the one system it is meant for, 100 x 80, it never measured faster
        // than the one-pass form (8.2 against 7.8, 7.9 against 6.8 us in two runs) -- DESIGN.md 14; it stays as a forced path for the lab and the tests)
        if (ata_plan(K->M, K->NP, K->N, false).ok && K->N <= ATA1_MAX_N) return ata_one_pass(K, x, y, false, s);
    }
    int rc = row_product(K, x, K->t, 0, v == DN_ATA2 ? DN_AUTO : v, s);
    if (!rc) rc = col_product(K, K->t, y, 0, false, s);
    K->last_kernel = DN_NAMES[3];
    return rc;
}

// any_type: the entry serves complex64 handles too (the queries, set_kernel, destroy); every other one refuses them
static lcg_hip_dense *dense_of(const void *h, const char *entry, bool any_type = false)
{
    if (!dense_handle(h)) { arg_error("%s: the handle is not a dense matrix (lcg_hip_dense_create)", entry); return nullptr; }
    lcg_hip_dense *K = static_cast<lcg_hip_dense *>(const_cast<void *>(h));
    if (K->c64 && !any_type) { refuse_c64_dense(entry); return nullptr; }
    return K;
}

int refuse_c64_dense(const char *entry)
{
    return arg_error("%s: the matrix holds complex64 values (lcg_hip_dense_create_c64); its entries are the _c64 ones", entry);
}

static void dense_release(lcg_hip_dense *K)
{
    if (K->val) hipFree(K->val);
    if (K->t) hipFree(K->t);
    if (K->part) hipFree(K->part);
    if (K->invdiag) hipFree(K->invdiag);
    dnm_release(K);
    delete K;
}

// the handle with its device arrays, K zeroed (pads and slack included)
static int dense_alloc(lcg_hip_dense **out, int M, int N, bool cplx, bool f32 = false)
{
    lcg_hip_dense *K = new lcg_hip_dense;
    K->M = M; K->N = N; K->cplx = cplx; K->f32 = f32;
    K->NP = cplx ? N : (N + 1) / 2;
    K->ldp = K->NP;
    const size_t bytes = (size_t)M * (size_t)K->ldp * (f32 ? 8 : 16) + 64;
    K->part_doubles = table_doubles(M, N, K->NP, cplx);
    hipError_t e = hipMalloc(&K->val, bytes);
    if (e == hipSuccess) e = hipMalloc(&K->t, sizeof(double) * (cplx ? 2 : 1) * (size_t)M);
    if (e == hipSuccess) e = hipMalloc(&K->part, sizeof(double) * (size_t)K->part_doubles);
    if (e == hipSuccess) e = hipMemsetAsync(K->val, 0, bytes, ctx().stream);
    if (e != hipSuccess) { dense_release(K); return fail(e, "dense matrix allocation", __FILE__, __LINE__); }
    *out = K;
    return 0;
}

static int dense_publish(lcg_hip_dense_t *out, lcg_hip_dense *K, hipError_t e)
{
    if (e == hipSuccess) e = hipStreamSynchronize(ctx().stream);
    if (e != hipSuccess) { dense_release(K); return fail(e, "dense matrix copy", __FILE__, __LINE__); }
    *out = K;
    return 0;
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_dense_create(lcg_hip_dense_t *K, int m_rows, int n_cols, const double *val, int64_t ld, int is_complex, int mem)
{
    if (!K) return arg_error("lcg_hip_dense_create: the handle pointer is NULL");
    *K = nullptr;
    if (!val) return arg_error("lcg_hip_dense_create: val is NULL");
    if (m_rows <= 0 || n_cols <= 0) return arg_error("lcg_hip_dense_create: M = %d, N = %d (both must be positive)", m_rows, n_cols);
    if (ld < n_cols) return arg_error("lcg_hip_dense_create: ld = %lld < N = %d", (long long)ld, n_cols);
    if (mem != LCG_HIP_MEM_HOST && mem != LCG_HIP_MEM_DEVICE) return arg_error("lcg_hip_dense_create: mem = %d", mem);
    int rc = ensure_init(); if (rc) return rc;
    lcg_hip_dense *D = nullptr;
    rc = dense_alloc(&D, m_rows, n_cols, is_complex != 0); if (rc) return rc;
    const size_t es = is_complex ? 16 : 8;
    const hipMemcpyKind kind = mem == LCG_HIP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    hipError_t e;
    if (ld == n_cols && (size_t)ld * es == (size_t)D->ldp * 16) e = hipMemcpyAsync(D->val, val, (size_t)m_rows * (size_t)ld * es, kind, ctx().stream);
    else e = hipMemcpy2DAsync(D->val, (size_t)D->ldp * 16, val, (size_t)ld * es, (size_t)n_cols * es, (size_t)m_rows, kind, ctx().stream);
    return dense_publish(K, D, e);
}

// An fp32 source packed on the device.  A source on the host is staged through device memory a run of rows at a time (at most 256 MiB),
// so the transient cost of the call is that buffer, not a second matrix.
int lcg_hip_dense_create_f32(lcg_hip_dense_t *K, int m_rows, int n_cols, const float *val, int64_t ld, int mem)
{
    if (!K) return arg_error("lcg_hip_dense_create_f32: the handle pointer is NULL");
    *K = nullptr;
    if (!val) return arg_error("lcg_hip_dense_create_f32: val is NULL");
    if (m_rows <= 0 || n_cols <= 0) return arg_error("lcg_hip_dense_create_f32: M = %d, N = %d (both must be positive)", m_rows, n_cols);
    if (ld < n_cols) return arg_error("lcg_hip_dense_create_f32: ld = %lld < N = %d", (long long)ld, n_cols);
    if (mem != LCG_HIP_MEM_HOST && mem != LCG_HIP_MEM_DEVICE) return arg_error("lcg_hip_dense_create_f32: mem = %d", mem);
    int rc = ensure_init(); if (rc) return rc;
    lcg_hip_dense *D = nullptr;
    rc = dense_alloc(&D, m_rows, n_cols, false, true); if (rc) return rc;
    hipStream_t s = ctx().stream;
    float2 *dst = reinterpret_cast<float2 *>(D->val);
    auto pack = [&](const float *src, int64_t lds, int i0, int rows) {
        const int64_t work = (int64_t)rows * D->NP;
        hipLaunchKernelGGL(k_dn_pack_f32, dim3((unsigned)cdiv(work, 256)), dim3(256), 0, s, src, lds, rows, n_cols, D->NP, dst + (int64_t)i0 * D->ldp, D->ldp);
        return hipGetLastError();
    };
    hipError_t e = hipSuccess;
    const int chunk = (int)std::min<int64_t>(m_rows, std::max<int64_t>(1, ((int64_t)64 << 20) / n_cols));      // rows per launch: <= 2^26 entries
    if (mem == LCG_HIP_MEM_DEVICE) {
        for (int i0 = 0; i0 < m_rows && e == hipSuccess; i0 += chunk) e = pack(val + (int64_t)i0 * ld, ld, i0, std::min(chunk, m_rows - i0));
    } else {
        float *stage = nullptr;
        e = hipMalloc(&stage, sizeof(float) * (size_t)chunk * (size_t)n_cols);
        for (int i0 = 0; i0 < m_rows && e == hipSuccess; i0 += chunk) {
            const int rows = std::min(chunk, m_rows - i0);
            e = hipMemcpy2DAsync(stage, sizeof(float) * (size_t)n_cols, val + (int64_t)i0 * ld, sizeof(float) * (size_t)ld, sizeof(float) * (size_t)n_cols,
                                 (size_t)rows, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = pack(stage, n_cols, i0, rows);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (stage) (void)hipFree(stage);
    }
    return dense_publish(K, D, e);
}

int lcg_hip_dense_value_bytes(lcg_hip_dense_t K)
{
    if (!dense_of(K, "lcg_hip_dense_value_bytes", true)) return LCG_HIP_E_ARG;
    return K->f32 ? 4 : K->cplx ? 16 : 8;       // (complex64: a float pair)
}

int lcg_hip_dense_create_rows(lcg_hip_dense_t *K, int m_rows, int n_cols, const double *const *rows, int is_complex)
{
    if (!K) return arg_error("lcg_hip_dense_create_rows: the handle pointer is NULL");
    *K = nullptr;
    if (!rows) return arg_error("lcg_hip_dense_create_rows: rows is NULL");
    if (m_rows <= 0 || n_cols <= 0) return arg_error("lcg_hip_dense_create_rows: M = %d, N = %d (both must be positive)", m_rows, n_cols);
    for (int i = 0; i < m_rows; i++) if (!rows[i]) return arg_error("lcg_hip_dense_create_rows: row %d is NULL", i);
    int rc = ensure_init(); if (rc) return rc;
    lcg_hip_dense *D = nullptr;
    rc = dense_alloc(&D, m_rows, n_cols, is_complex != 0); if (rc) return rc;
    const size_t rowd = (size_t)D->ldp * 2, used = (size_t)n_cols * (is_complex ? 2 : 1);
    std::vector<double> stage((size_t)m_rows * rowd, 0.0);      // the padded layout, assembled on the host: one copy
    for (int i = 0; i < m_rows; i++) std::memcpy(stage.data() + (size_t)i * rowd, rows[i], used * sizeof(double));
    hipError_t e = hipMemcpyAsync(D->val, stage.data(), stage.size() * sizeof(double), hipMemcpyHostToDevice, ctx().stream);
    return dense_publish(K, D, e);      // (drains the stream: `stage` may go)
}

int lcg_hip_dense_destroy(lcg_hip_dense_t K)
{
    if (!dense_of(K, "lcg_hip_dense_destroy", true)) return LCG_HIP_E_ARG;
    K->kind = 0;
    if (ctx().inited) (void)hipDeviceSynchronize();
    dense_release(K);
    return 0;
}

int lcg_hip_dense_rows(lcg_hip_dense_t K) { return dense_of(K, "lcg_hip_dense_rows", true) ? K->M : LCG_HIP_E_ARG; }
int lcg_hip_dense_cols(lcg_hip_dense_t K) { return dense_of(K, "lcg_hip_dense_cols", true) ? K->N : LCG_HIP_E_ARG; }
const char *lcg_hip_dense_last_kernel(lcg_hip_dense_t K) { return dense_of(K, "lcg_hip_dense_last_kernel", true) ? K->last_kernel : ""; }
const char *lcg_hip_dense_kernel_name(int index)
{
    return index >= 0 && index < (int)(sizeof DN_NAMES / sizeof *DN_NAMES) ? DN_NAMES[index] : nullptr;
}

int lcg_hip_dense_set_kernel(lcg_hip_dense_t K, int variant)
{
    if (!dense_of(K, "lcg_hip_dense_set_kernel", true)) return LCG_HIP_E_ARG;
    if (variant < DN_AUTO || variant > DN_ATA_SMALL) return arg_error("lcg_hip_dense_set_kernel: variant = %d (0 .. %d)", variant, (int)DN_ATA_SMALL);
    if (K->c64 && variant > DN_COL) return arg_error("lcg_hip_dense_set_kernel: a complex64 matrix has no K^T.K.x forms (variant = %d)", variant);
    if ((variant == DN_ATA1 || variant == DN_ATA_SMALL) && (K->cplx || K->NP > 1024))
        return arg_error("lcg_hip_dense_set_kernel: the one-pass K^T.K.x serves real matrices of N <= 2048");
    if (variant == DN_ROW_SPLIT && row_plan(K->M, K->NP, true, true).S < 2)
        return arg_error("lcg_hip_dense_set_kernel: k_dn_row_split needs rows of >= 32 packs and M < 8192 (M = %d, N = %d): nothing to split", K->M, K->N);
    K->variant = variant;
    return 0;
}

static int dense_matvec(lcg_hip_dense_t K, const double *x, double *y, int layout, int conjugate, bool want_cplx, const char *entry)
{
    if (!dense_of(K, entry)) return LCG_HIP_E_ARG;
    if (K->cplx != want_cplx) return arg_error("%s: the matrix is %s", entry, K->cplx ? "complex (clcg_hip_dense_matvec)" : "real (lcg_hip_dense_matvec)");
    if (!x || !y) return arg_error("%s: x or y is NULL", entry);
    if (x == y) return arg_error("%s: x and y are the same vector", entry);
    if (layout < 0 || layout > 1 || conjugate < 0 || conjugate > 1) return arg_error("%s: layout = %d, conjugate = %d", entry, layout, conjugate);
    return layout ? col_product(K, x, y, conjugate, false, ctx().stream) : row_product(K, x, y, conjugate, K->variant, ctx().stream);
}

int lcg_hip_dense_matvec(lcg_hip_dense_t K, const double *x, double *y, int layout)
{
    return dense_matvec(K, x, y, layout, 0, false, "lcg_hip_dense_matvec");
}

int clcg_hip_dense_matvec(lcg_hip_dense_t K, const double *x, double *y, int layout, int conjugate)
{
    return dense_matvec(K, x, y, layout, conjugate, true, "clcg_hip_dense_matvec");
}

int lcg_hip_dense_ata(lcg_hip_dense_t K, const double *x, double *y)
{
    if (!dense_of(K, "lcg_hip_dense_ata")) return LCG_HIP_E_ARG;
    if (K->cplx) return arg_error("lcg_hip_dense_ata: the matrix is complex");
    if (!x || !y) return arg_error("lcg_hip_dense_ata: x or y is NULL");
    if (x == y) return arg_error("lcg_hip_dense_ata: x and y are the same vector");
    return ata_product(K, x, y, ctx().stream);
}

// The callback types return void (lcg.h:37-38, clcg.h:40-41): a failure is parked in Ctx::ax_rc, where the solver loop picks it
// up right after the call and ends the solve with that code (driver.hpp: timed_ax / checked_mx); nothing was written.
static void dn_park(int rc) { if (rc && !ctx().ax_rc) ctx().ax_rc = rc; }
static int dn_size(const lcg_hip_dense *K, int n, int want, const char *entry)
{
    return n == want ? 0 : arg_error("%s: n_size = %d, the matrix has %d %s", entry, n, want, K->M == K->N ? "rows" : "columns");
}

void lcg_hip_dense_ata_ax(void *instance, const double *x, double *y, const int n)
{
    lcg_hip_dense *K = dense_of(instance, "lcg_hip_dense_ata_ax");
    if (!K) return dn_park(LCG_HIP_E_ARG);
    if (dn_size(K, n, K->N, "lcg_hip_dense_ata_ax")) return dn_park(LCG_HIP_E_ARG);
    dn_park(lcg_hip_dense_ata(K, x, y));
}

void lcg_hip_dense_ax(void *instance, const double *x, double *y, const int n)
{
    lcg_hip_dense *K = dense_of(instance, "lcg_hip_dense_ax");
    if (!K) return dn_park(LCG_HIP_E_ARG);
    if (K->M != K->N) return dn_park(arg_error("lcg_hip_dense_ax: the matrix is %d x %d, not square (lcg_hip_dense_ata_ax multiplies by K^T.K)", K->M, K->N));
    if (dn_size(K, n, K->N, "lcg_hip_dense_ax")) return dn_park(LCG_HIP_E_ARG);
    dn_park(lcg_hip_dense_matvec(K, x, y, 0));
}

void clcg_hip_dense_ax(void *instance, const double *x, double *y, const int n, int layout, int conjugate)
{
    lcg_hip_dense *K = dense_of(instance, "clcg_hip_dense_ax");
    if (!K) return dn_park(LCG_HIP_E_ARG);
    if (K->M != K->N) return dn_park(arg_error("clcg_hip_dense_ax: the matrix is %d x %d, not square", K->M, K->N));
    if (dn_size(K, n, K->N, "clcg_hip_dense_ax")) return dn_park(LCG_HIP_E_ARG);
    dn_park(clcg_hip_dense_matvec(K, x, y, layout, conjugate));
}

int lcg_hip_dense_build_jacobi(lcg_hip_dense_t K, int normal, double *diag_out)
{
    if (!dense_of(K, "lcg_hip_dense_build_jacobi")) return LCG_HIP_E_ARG;
    if (normal != 0 && normal != 1) return arg_error("lcg_hip_dense_build_jacobi: normal = %d (0: 1 / K(i,i), 1: 1 / sum_j K(j,i)^2)", normal);
    if (normal && K->cplx) return arg_error("lcg_hip_dense_build_jacobi: the column sums of squares serve real matrices (sample1.cpp:98-107)");
    if (!normal && K->M != K->N) return arg_error("lcg_hip_dense_build_jacobi: the matrix is %d x %d: its diagonal needs a square one", K->M, K->N);
    Ctx &c = ctx();
    const int w = K->cplx ? 2 : 1, n = K->N;
    const size_t bytes = sizeof(double) * (size_t)w * (size_t)n;
    if (!K->invdiag) HIPCHK(hipMalloc(&K->invdiag, bytes));
    K->invdiag_normal = -1;
    std::vector<double> d((size_t)w * n);
    if (normal) {       // one more column-form pass
        int rc = col_product(K, nullptr, K->invdiag, 0, true, c.stream); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(d.data(), K->invdiag, bytes, hipMemcpyDeviceToHost, c.stream));
    } else {
        const dim3 grid((unsigned)cdiv(n, 256));
        if (K->f32) hipLaunchKernelGGL(k_dn_diag_f32, grid, dim3(256), 0, c.stream, dn_val32(K), K->ldp, n, K->invdiag);
        else if (K->cplx) hipLaunchKernelGGL(k_dn_diag<true>, grid, dim3(256), 0, c.stream, K->val, K->ldp, n, K->invdiag);
        else hipLaunchKernelGGL(k_dn_diag<false>, grid, dim3(256), 0, c.stream, K->val, K->ldp, n, K->invdiag);
        int rc = launched("dense diagonal"); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(d.data(), K->invdiag, bytes, hipMemcpyDeviceToHost, c.stream));
    }
    HIPCHK(hipStreamSynchronize(c.stream));
    if (diag_out) HIPCHK(hipMemcpyAsync(diag_out, d.data(), bytes, hipMemcpyHostToDevice, c.stream));
    std::vector<double> r((size_t)w * n);
    for (int i = 0; i < n; i++) {
        if (!K->cplx) {
            if (d[i] == 0.0 || !std::isfinite(d[i])) { hipStreamSynchronize(c.stream); hipFree(K->invdiag); K->invdiag = nullptr;
                return arg_error("lcg_hip_dense_build_jacobi: diagonal entry %d is %g", i, d[i]); }
            r[i] = 1.0 / d[i];
        } else {
            const double a = d[2 * (size_t)i], b = d[2 * (size_t)i + 1];
            if ((a == 0.0 && b == 0.0) || !std::isfinite(a) || !std::isfinite(b)) { hipStreamSynchronize(c.stream); hipFree(K->invdiag); K->invdiag = nullptr;
                return arg_error("lcg_hip_dense_build_jacobi: diagonal entry %d is (%g, %g)", i, a, b); }
            // 1 / (a + i b) by the scaled division (Smith): no a^2 + b^2 that overflows or underflows before the quotient does
            if (std::fabs(a) >= std::fabs(b)) { const double q = b / a, den = a + b * q; r[2 * (size_t)i] = 1.0 / den; r[2 * (size_t)i + 1] = -q / den; }
            else { const double q = a / b, den = a * q + b; r[2 * (size_t)i] = q / den; r[2 * (size_t)i + 1] = -1.0 / den; }
        }
    }
    HIPCHK(hipMemcpyAsync(K->invdiag, r.data(), bytes, hipMemcpyHostToDevice, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    K->invdiag_normal = normal;     // (the batched PCG asks: dense_multi.hip)
    return 0;
}

static int dense_jacobi(void *instance, const double *x, double *z, int n, bool cplx, const char *entry)
{
    lcg_hip_dense *K = dense_of(instance, entry);
    if (!K) return LCG_HIP_E_ARG;
    if (K->cplx != cplx) return arg_error("%s: the matrix is %s", entry, K->cplx ? "complex" : "real");
    if (!K->invdiag) return arg_error("%s: lcg_hip_dense_build_jacobi() was not called", entry);
    if (dn_size(K, n, K->N, entry)) return LCG_HIP_E_ARG;
    if (!x || !z) return arg_error("%s: x or z is NULL", entry);
    const dim3 grid((unsigned)cdiv(n, 256));
    if (cplx) hipLaunchKernelGGL(k_dn_scale<true>, grid, dim3(256), 0, ctx().stream, K->invdiag, x, z, n);
    else hipLaunchKernelGGL(k_dn_scale<false>, grid, dim3(256), 0, ctx().stream, K->invdiag, x, z, n);
    return launched(entry);
}

void lcg_hip_dense_jacobi_mx(void *instance, const double *x, double *z, const int n)
{
    dn_park(dense_jacobi(instance, x, z, n, false, "lcg_hip_dense_jacobi_mx"));
}

void clcg_hip_dense_jacobi_mx(void *instance, const double *x, double *z, const int n, int layout, int conjugate)
{
    (void)layout; (void)conjugate;      // as clcg_hip_jacobi_mx: the diagonal is its own transpose, and the loops ask for (0, 0)
    dn_park(dense_jacobi(instance, x, z, n, true, "clcg_hip_dense_jacobi_mx"));
}

} // extern "C"
