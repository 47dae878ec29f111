// sample_dense_multi.cpp -- the system of liblcg's sample1.cpp (a dense 1000 x 800 kernel K, the normal equations
// K^T.K m = K^T d) for EIGHT data vectors: one batched solve (lcg_hip_dense_lcg_multi: K is read twice per iteration for all eight
// columns) against eight lcg_solver calls on the ready-made CalAx (lcg_hip_dense_ata_ax: K is read per column).  Prints both sets
// of iteration counts and the largest difference between the two sets of solutions.  Plain C++: compile with g++.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_dense_multi.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_dense_multi && ./sample_dense_multi
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lcg_dropin.hpp"

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
    const int M = argc > 2 ? atoi(argv[1]) : 1000, N = argc > 2 ? atoi(argv[2]) : 800, k = 8;
    std::vector<std::vector<double> > kernel(M, std::vector<double>(N));       // lcg_malloc(M, N)'s layout: M rows
    std::vector<const double *> rows(M);
    for (int i = 0; i < M; i++) {
        for (int j = 0; j < N; j++) kernel[i][j] = uniform(-1.0, 1.0);
        rows[i] = kernel[i].data();
    }
    // eight models and their data: column c of the blocks (row-major N x k; over-aligned: the blocks' bases must be 16-byte aligned)
    std::vector<double> raw((size_t)3 * N * k + 2);
    double *base = raw.data() + (((uintptr_t)raw.data() & 15) ? 1 : 0);
    double *FM = base, *B = base + (size_t)N * k, *X = base + (size_t)2 * N * k;
    std::vector<double> tmp(M), b(N), m(N), single((size_t)N * k);
    for (int c = 0; c < k; c++) {
        for (int j = 0; j < N; j++) FM[(size_t)j * k + c] = uniform(1.0, 2.0);
        for (int i = 0; i < M; i++) { double s = 0.0; for (int j = 0; j < N; j++) s += kernel[i][j] * FM[(size_t)j * k + c]; tmp[i] = s; }
        for (int j = 0; j < N; j++) { double s = 0.0; for (int i = 0; i < M; i++) s += kernel[i][j] * tmp[i]; B[(size_t)j * k + c] = s; }
    }

    lcg_hip_dense_t K = nullptr;
    int rc = lcg_hip_dense_create_rows(&K, M, N, rows.data(), 0);
    if (rc) { fprintf(stderr, "lcg_hip_dense_create_rows: %s\n", lcg_hip_last_error()); return 3; }

    lcg_para para = lcg_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 0; para.max_iterations = 2000;

    // eight solves, one per data vector
    int its1[8], bad = 0;
    for (int c = 0; c < k; c++) {
        for (int j = 0; j < N; j++) { b[j] = B[(size_t)j * k + c]; m[j] = 0.0; }
        const int ret = lcg_solver(lcg_hip_dense_ata_ax, nullptr, m.data(), b.data(), N, &para, K, LCG_CG);
        if (ret != 0) { fprintf(stderr, "lcg_solver, column %d: %d (%s)\n", c, ret, lcg_status_text(ret)); bad = 1; }
        its1[c] = lcg_hip_last_iterations();
        for (int j = 0; j < N; j++) single[(size_t)j * k + c] = m[j];
    }
    // one batched solve
    int ret8[8], its8[8];
    double res8[8];
    for (size_t e = 0; e < (size_t)N * k; e++) X[e] = 0.0;
    rc = lcg_hip_dense_lcg_multi(K, k, 1, X, B, &para, ret8, its8, res8, LCG_HIP_MEM_HOST);
    if (rc) { fprintf(stderr, "lcg_hip_dense_lcg_multi: %d %s\n", rc, lcg_hip_last_error()); return 3; }
    int vec = 0, products = 0;
    lcg_hip_last_launches(&vec, nullptr, nullptr, &products);

    double diff = 0.0, err = 0.0;
    for (size_t e = 0; e < (size_t)N * k; e++) { diff = std::fmax(diff, std::fabs(X[e] - single[e])); err = std::fmax(err, std::fabs(X[e] - FM[e])); }
    printf("eight lcg_solver calls, iterations:");
    for (int c = 0; c < k; c++) printf(" %d", its1[c]);
    printf("\none lcg_hip_dense_lcg_multi, iterations:");
    for (int c = 0; c < k; c++) { printf(" %d", its8[c]); if (ret8[c] != 0 || std::abs(its8[c] - its1[c]) > 3) bad = 1; }
    printf("\nlargest difference between the two sets of solutions: %.3e; largest error of the batch: %.3e\n", diff, err);
    printf("the batched solve enqueued %d operator kernels and %d vector passes (%s)\n", products, vec, lcg_hip_dense_multi_last_kernel(K));
    if (diff > 1e-6 || err > 1e-3) bad = 1;
    lcg_hip_dense_destroy(K);
    return bad;
}
