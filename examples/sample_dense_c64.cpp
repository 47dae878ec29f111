// sample_dense_c64.cpp -- liblcg's sample3 system (a dense complex-symmetric N x N kernel) held and solved in SINGLE precision, the way
// sample14 runs its CSR matrix: the kernel lives in HBM as a complex64 dense handle (8 bytes per entry where sample_dense_complex's
// handle holds 16), one BiCG-sym solve goes through clcg_hip_solver_c64 with the ready-made callback clcg_hip_dense_ax_c64, then four
// scaled right-hand sides go through the batched loops clcg_hip_dense_lbicg_sym_multi_c64 and clcg_hip_dense_lpcg_multi_c64, which read
// the kernel once per iteration for all four columns.
// Plain C++ against the C ABI (include/lcg_hip.h, include/lcg_hip_staging_dense_c64.h): no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_dense_c64.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_dense_c64 && ./sample_dense_c64
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lcg_hip.h"
#include "lcg_hip_staging_dense_c64.h"

typedef std::complex<float> fc;

static uint64_t rng_state = 0xD1B54A32D192ED03ull;     // a fixed seed (the reference seeds with time(0))
static double uniform(double lo, double hi)
{
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    const uint64_t r = rng_state * 0x2545F4914F6CDD1Dull;
    return lo + (hi - lo) * (double)(r >> 11) / 9007199254740992.0;
}

// a block of k complex64 vectors: n * k (re, im) float pairs, row-major, the base 16-byte aligned
struct Block {
    std::vector<float> store;
    fc *p;
    Block(size_t n, int k) : store(2 * n * k + 4, 0.0f)
    {
        float *d = store.data();
        while ((uintptr_t)d & 15) d++;
        p = reinterpret_cast<fc *>(d);
    }
    float *raw() { return reinterpret_cast<float *>(p); }
};

int main(int argc, char **argv)
{
    const int N = argc > 1 ? atoi(argv[1]) : 500, k = 4;
    std::vector<fc> kernel((size_t)N * N), fm(N), B(N), m(N, fc(0.f, 0.f));
    for (int i = 0; i < N; i++)
        for (int j = i; j < N; j++) {
            std::complex<double> v(uniform(-1.0, 1.0), uniform(-1.0, 1.0));
            if (i == j) v += std::complex<double>(2.0 * std::sqrt((double)N), std::sqrt((double)N));    // keeps every solver's run short
            kernel[(size_t)i * N + j] = kernel[(size_t)j * N + i] = fc((float)v.real(), (float)v.imag());
        }
    for (int j = 0; j < N; j++) fm[j] = fc((float)uniform(1.0, 2.0), (float)uniform(1.0, 2.0));
    for (int i = 0; i < N; i++) {
        std::complex<double> s(0.0, 0.0);
        for (int j = 0; j < N; j++) s += std::complex<double>(kernel[(size_t)i * N + j]) * std::complex<double>(fm[j]);
        B[i] = fc((float)s.real(), (float)s.imag());
    }

    lcg_hip_dense_t K = nullptr;
    int rc = lcg_hip_dense_create_c64(&K, N, N, reinterpret_cast<const float *>(kernel.data()), N, LCG_HIP_MEM_HOST);
    if (rc) { fprintf(stderr, "lcg_hip_dense_create_c64: %s\n", lcg_hip_last_error()); return 3; }
    rc = lcg_hip_dense_build_jacobi_c64(K, nullptr);
    if (rc) { fprintf(stderr, "lcg_hip_dense_build_jacobi_c64: %s\n", lcg_hip_last_error()); lcg_hip_dense_destroy(K); return 3; }

    clcg_para para = clcg_hip_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 0; para.max_iterations = 1000;
    bool ok = true;

    // one right-hand side: BiCG for symmetric K through the callback
    rc = clcg_hip_solver_c64(clcg_hip_dense_ax_c64, nullptr, reinterpret_cast<float *>(m.data()), reinterpret_cast<const float *>(B.data()), N,
                             &para, K, CLCG_BICG_SYM, LCG_HIP_MEM_HOST);
    double e = 0.0;
    for (int j = 0; j < N; j++) e = std::fmax(e, (double)std::abs(m[j] - fm[j]));
    printf("BICG_SYM: ret=%d iterations=%d residual=%.3e maximal error=%.3e kernel=%s\n", rc, lcg_hip_last_iterations(),
           lcg_hip_last_residual(), e, lcg_hip_dense_last_kernel(K));
    if (rc <= LCG_HIP_E_RUNTIME) { fprintf(stderr, "clcg_hip_solver_c64: %s\n", lcg_hip_last_error()); lcg_hip_dense_destroy(K); return 3; }
    ok = ok && rc == CLCG_CONVERGENCE && e < 1e-3;

    // four scaled right-hand sides at once
    const float scale[k] = {1.0f, 1e-2f, -1.0f, 2.0f};
    Block Bk(N, k);
    for (int i = 0; i < N; i++)
        for (int j = 0; j < k; j++) Bk.p[(size_t)i * k + j] = scale[j] * B[i];
    for (int loop = 0; loop < 2; loop++) {
        Block M(N, k);
        int ret[k], its[k];
        double res[k];
        const char *name = loop ? "clcg_hip_dense_lpcg_multi_c64" : "clcg_hip_dense_lbicg_sym_multi_c64";
        rc = loop ? clcg_hip_dense_lpcg_multi_c64(K, k, M.raw(), Bk.raw(), &para, ret, its, res, LCG_HIP_MEM_HOST)
                  : clcg_hip_dense_lbicg_sym_multi_c64(K, k, M.raw(), Bk.raw(), &para, ret, its, res, LCG_HIP_MEM_HOST);
        if (rc) { fprintf(stderr, "%s: rc=%d %s\n", name, rc, lcg_hip_last_error()); lcg_hip_dense_destroy(K); return 3; }
        printf("%s (%s)\n", name, lcg_hip_dense_multi_last_kernel(K));
        for (int j = 0; j < k; j++) {
            double ej = 0.0;
            for (int i = 0; i < N; i++) ej = std::fmax(ej, (double)std::abs(M.p[(size_t)i * k + j] - scale[j] * fm[i]));
            printf("column %d (%g b): ret=%d iterations=%d residual=%.3e maximal error=%.3e\n", j, (double)scale[j], ret[j], its[j], res[j], ej);
            ok = ok && ret[j] == CLCG_CONVERGENCE && ej < 1e-3 * std::fabs((double)scale[j]) + 1e-5;
        }
    }
    lcg_hip_dense_destroy(K);
    return ok ? 0 : 1;
}
