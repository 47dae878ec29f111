// sample_dense_complex.cpp -- the workload of liblcg's sample3.cpp (a dense complex symmetric N x N kernel, CalAx =
// clcg_matvec, the complex solvers; clbicg asks the callback for the conjugate-transpose form; sample3.cpp:44-49),
// written against include/lcg_dropin.hpp.  The kernel lives in HBM as a lcg_hip_dense_t and CalAx calls the
// clcg_matvec overload on the device vectors the solver hands it.  Plain C++: compile with g++.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_dense_complex.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_dense_complex && ./sample_dense_complex
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lcg_dropin.hpp"

static uint64_t rng_state = 0xD1B54A32D192ED03ull;     // a fixed seed (the reference seeds with time(0))
static double uniform(double lo, double hi)
{
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    const uint64_t r = rng_state * 0x2545F4914F6CDD1Dull;
    return lo + (hi - lo) * (double)(r >> 11) / 9007199254740992.0;
}

static int failed = 0;
static void CalAx(void *instance, const lcg_complex *x, lcg_complex *prod_Ax, const int, lcg_matrix_e layout, clcg_complex_e conjugate)
{   // sample3.cpp:44-49
    if (clcg_matvec(static_cast<lcg_hip_dense_t>(instance), x, prod_Ax, layout, conjugate)) failed = 1;
}

int main(int argc, char **argv)
{
    const int N = argc > 1 ? atoi(argv[1]) : 1000;
    std::vector<lcg_complex> kernel((size_t)N * N), fm(N), B(N), m(N);
    for (int i = 0; i < N; i++)
        for (int j = i; j < N; j++) {
            lcg_complex v(uniform(-1.0, 1.0), uniform(-1.0, 1.0));
            if (i == j) v += lcg_complex(2.0 * std::sqrt((double)N), std::sqrt((double)N));      // keeps every solver's run short
            kernel[(size_t)i * N + j] = kernel[(size_t)j * N + i] = v;
        }
    for (int j = 0; j < N; j++) fm[j] = lcg_complex(uniform(1.0, 2.0), uniform(1.0, 2.0));
    for (int i = 0; i < N; i++) { lcg_complex s(0.0, 0.0); for (int j = 0; j < N; j++) s += kernel[(size_t)i * N + j] * fm[j]; B[i] = s; }

    lcg_hip_dense_t K = nullptr;
    int rc = lcg_hip_dense_create(&K, N, N, reinterpret_cast<const double *>(kernel.data()), N, 1, LCG_HIP_MEM_HOST);
    if (rc) { fprintf(stderr, "lcg_hip_dense_create: %s\n", lcg_hip_last_error()); return 3; }

    clcg_para para = clcg_default_parameters();
    para.epsilon = 1e-20; para.abs_diff = 0; para.max_iterations = 1000;
    struct { const char *name; clcg_solver_enum id; } runs[] = {{"BICG", CLCG_BICG}, {"BICG_SYM", CLCG_BICG_SYM}, {"CGS", CLCG_CGS},
                                                               {"BICGSTAB", CLCG_BICGSTAB}, {"TFQMR", CLCG_TFQMR}};
    int bad = 0;
    for (auto &r : runs) {
        std::fill(m.begin(), m.end(), lcg_complex(0.0, 0.0));
        const int ret = clcg_solver(r.id == CLCG_BICG_SYM ? clcg_dense_ax : CalAx, nullptr, m.data(), B.data(), N, &para, K, r.id);
        double e = 0.0;
        for (int j = 0; j < N; j++) e = std::fmax(e, std::abs(m[j] - fm[j]));
        printf("%s: ret=%d (%s) iterations=%d residual=%.3e maximal error=%.3e kernel=%s\n", r.name, ret, lcg_status_text(ret),
               lcg_hip_last_iterations(), lcg_hip_last_residual(), e, lcg_hip_dense_last_kernel(K));
        if (ret <= LCG_HIP_E_RUNTIME || failed) bad = 1;
        if ((r.id == CLCG_BICG || r.id == CLCG_BICG_SYM) && (ret != 0 || e > 1e-3)) bad = 1;
    }
    lcg_hip_dense_destroy(K);
    return bad;
}
