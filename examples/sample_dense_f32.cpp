// sample_dense_f32.cpp -- sample_dense.cpp's flow (liblcg's sample1.cpp: a dense 1000 x 800 kernel K, the normal equations
// K^T.K m = K^T.K m_true solved by all seven real solvers, the preconditioner 1 / sum_j K(j,i)^2, the box 1 <= m <= 2) from a kernel
// computed in SINGLE precision: K is handed over as floats and stays fp32 in HBM (lcg_hip_dense_create_f32,
// include/lcg_hip_staging_dense_f32.h), 4 bytes per entry in every product instead of 8; vectors, sums and solver state are fp64 and
// nothing else changes -- the same callbacks, the same solvers.  The results are the bits of a run on the kernel widened to double.
// Plain C++: compile with g++.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_dense_f32.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_dense_f32 && ./sample_dense_f32
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lcg_dropin.hpp"
#include "lcg_hip_staging_dense_f32.h"

// a fixed-seed generator of its own (the reference seeds with time(0)): xorshift64*, uniform in [lo, hi)
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform(double lo, double hi)
{
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    const uint64_t r = rng_state * 0x2545F4914F6CDD1Dull;
    return lo + (hi - lo) * (double)(r >> 11) / 9007199254740992.0;
}

int main(int argc, char **argv)
{
    const int M = argc > 2 ? atoi(argv[1]) : 1000, N = argc > 2 ? atoi(argv[2]) : 800;
    std::vector<float> kernel((size_t)M * N);                    // row-major, ld = N
    for (size_t e = 0; e < kernel.size(); e++) kernel[e] = (float)uniform(-1.0, 1.0);
    std::vector<double> fm(N), B(N), tmp(M), m(N), low(N, 1.0), hig(N, 2.0);
    for (int j = 0; j < N; j++) fm[j] = uniform(1.0, 2.0);
    // B = K^T.(K.m_true) with the float entries as they are (widened exactly): the system the device sees
    for (int i = 0; i < M; i++) { double s = 0.0; for (int j = 0; j < N; j++) s += (double)kernel[(size_t)i * N + j] * fm[j]; tmp[i] = s; }
    for (int j = 0; j < N; j++) { double s = 0.0; for (int i = 0; i < M; i++) s += (double)kernel[(size_t)i * N + j] * tmp[i]; B[j] = s; }

    lcg_hip_dense_t K = nullptr;
    int rc = lcg_hip_dense_create_f32(&K, M, N, kernel.data(), N, LCG_HIP_MEM_HOST);
    if (rc) { fprintf(stderr, "lcg_hip_dense_create_f32: %s\n", lcg_hip_last_error()); return 3; }
    printf("K: %d x %d, %d bytes per entry\n", lcg_hip_dense_rows(K), lcg_hip_dense_cols(K), lcg_hip_dense_value_bytes(K));
    rc = lcg_hip_dense_build_jacobi(K, 1, nullptr);
    if (rc) { fprintf(stderr, "lcg_hip_dense_build_jacobi: %s\n", lcg_hip_last_error()); return 3; }

    lcg_para para = lcg_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 0; para.max_iterations = 2000;
    struct { const char *name; lcg_solver_enum id; } runs[] = {{"CG", LCG_CG}, {"PCG", LCG_PCG}, {"CGS", LCG_CGS}, {"BICGSTAB", LCG_BICGSTAB},
                                                              {"BICGSTAB2", LCG_BICGSTAB2}, {"PG", LCG_PG}, {"SPG", LCG_SPG}};
    int bad = 0;
    for (auto &r : runs) {
        std::fill(m.begin(), m.end(), 0.0);
        int ret;
        if (r.id == LCG_PCG) ret = lcg_solver_preconditioned(lcg_hip_dense_ata_ax, lcg_hip_dense_jacobi_mx, nullptr, m.data(), B.data(), N, &para, K);
        else if (r.id == LCG_PG || r.id == LCG_SPG) ret = lcg_solver_constrained(lcg_hip_dense_ata_ax, nullptr, m.data(), B.data(), low.data(), hig.data(), N, &para, K, r.id);
        else ret = lcg_solver(lcg_hip_dense_ata_ax, nullptr, m.data(), B.data(), N, &para, K, r.id);
        double e = 0.0;
        for (int j = 0; j < N; j++) e = std::fmax(e, std::fabs(m[j] - fm[j]));
        printf("%s: ret=%d (%s) iterations=%d residual=%.3e maximal error=%.3e kernel=%s\n", r.name, ret, lcg_status_text(ret),
               lcg_hip_last_iterations(), lcg_hip_last_residual(), e, lcg_hip_dense_last_kernel(K));
        if (ret <= LCG_HIP_E_RUNTIME) bad = 1;                       // a runtime failure; a capped run is a report, as in the reference
        if ((r.id == LCG_CG || r.id == LCG_PCG) && (ret != 0 || e > 1e-3)) bad = 1;
    }
    lcg_hip_dense_destroy(K);
    return bad;
}
