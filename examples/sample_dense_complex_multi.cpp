// sample_dense_complex_multi.cpp -- several sources against one frequency on a DENSE operator: liblcg's sample3 system (a dense
// complex-symmetric K through clcg_matvec) solved against FOUR right-hand sides -- K.x_true, 1e-2 times it, a point source and a zero
// column (how a caller with three sources pads to k = 4) -- by both batched complex loops on the dense handle:
// clcg_hip_dense_lbicg_sym_multi (BiCG for symmetric K) and clcg_hip_dense_lpcg_multi (PCG with the reciprocals of K's diagonal).
// Every column gets its own verdict, count and residual; the 16 N^2 bytes of K are read once per iteration for all four.
// Plain C++ against the C ABI (include/lcg_hip.h): no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_dense_complex_multi.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_dense_complex_multi && ./sample_dense_complex_multi
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <vector>

#include "lcg_hip.h"

typedef std::complex<double> zc;

// a block of k complex vectors: n * k (re, im) pairs, row-major, the base 16-byte aligned (lcg_hip.h: clcg_hip_dense_matmat)
struct Block {
    std::vector<double> store;
    zc *p;
    Block(size_t n, int k) : store(2 * n * k + 1, 0.0)
    {
        double *d = store.data() + (((uintptr_t)store.data() & 15) ? 1 : 0);
        p = reinterpret_cast<zc *>(d);
    }
    double *raw() { return reinterpret_cast<double *>(p); }
};

int main()
{
    const int n = 300, k = 4;
    // K = (G + G^T) / 2 + (40 + 20i) I with G's parts in [-1, 1) from a small generator: symmetric, not Hermitian, diagonally dominant
    std::vector<zc> G((size_t)n * n), K((size_t)n * n);
    uint32_t s = 2024u;
    for (size_t e = 0; e < G.size(); e++) {
        s = s * 1664525u + 1013904223u; const double re = (s >> 8) * (2.0 / 16777216.0) - 1.0;
        s = s * 1664525u + 1013904223u; const double im = (s >> 8) * (2.0 / 16777216.0) - 1.0;
        G[e] = zc(re, im);
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) K[(size_t)i * n + j] = 0.5 * (G[(size_t)i * n + j] + G[(size_t)j * n + i]) + (i == j ? zc(40.0, 20.0) : zc(0.0, 0.0));
    lcg_hip_dense_t D = nullptr;
    int rc = lcg_hip_dense_create(&D, n, n, reinterpret_cast<const double *>(K.data()), n, 1, LCG_HIP_MEM_HOST);
    if (rc) { std::cerr << "dense_create: " << lcg_hip_last_error() << "\n"; return 3; }
    rc = lcg_hip_dense_build_jacobi(D, 0, nullptr);
    if (rc) { std::cerr << "dense_build_jacobi: " << lcg_hip_last_error() << "\n"; lcg_hip_dense_destroy(D); return 3; }

    std::vector<zc> xt(n), b(n, zc(0.0, 0.0));
    for (int i = 0; i < n; i++) xt[i] = zc(1.0 + std::fabs(std::sin(0.7 * i)), 1.0 + std::fabs(std::cos(0.31 * i)));
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) b[i] += K[(size_t)i * n + j] * xt[j];
    Block B(n, k);
    for (int i = 0; i < n; i++) { B.p[(size_t)i * k + 0] = b[i]; B.p[(size_t)i * k + 1] = 1e-2 * b[i]; }
    B.p[(size_t)(n / 2) * k + 2] = zc(1.0, 0.0);        // column 2: a point source; column 3 stays zero

    clcg_para para = clcg_hip_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 1;
    bool ok = true;
    for (int loop = 0; loop < 2; loop++) {
        Block M(n, k);
        int ret[k], its[k];
        double res[k];
        const char *name = loop ? "clcg_hip_dense_lpcg_multi" : "clcg_hip_dense_lbicg_sym_multi";
        rc = loop ? clcg_hip_dense_lpcg_multi(D, k, M.raw(), B.raw(), &para, ret, its, res, LCG_HIP_MEM_HOST)
                  : clcg_hip_dense_lbicg_sym_multi(D, k, M.raw(), B.raw(), &para, ret, its, res, LCG_HIP_MEM_HOST);
        if (rc) { std::cerr << name << ": rc=" << rc << " " << lcg_hip_last_error() << "\n"; lcg_hip_dense_destroy(D); return 3; }
        std::printf("%s (%s)\n", name, lcg_hip_dense_multi_last_kernel(D));
        double e0 = 0.0, e1 = 0.0;
        for (int i = 0; i < n; i++) { e0 += std::norm(M.p[(size_t)i * k] - xt[i]); e1 += std::norm(M.p[(size_t)i * k + 1] - 1e-2 * xt[i]); }
        const double dist[k] = {std::sqrt(e0), std::sqrt(e1), -1.0, 0.0};
        for (int j = 0; j < k; j++) {
            std::printf("column %d: ret=%d iterations=%d residual=%.3e", j, ret[j], its[j], res[j]);
            if (dist[j] >= 0.0) std::printf(" distance_to_truth=%.3e", dist[j]);
            std::printf("\n");
        }
        ok = ok && ret[0] == CLCG_CONVERGENCE && ret[1] == CLCG_CONVERGENCE && ret[2] == CLCG_CONVERGENCE &&
             ret[3] == CLCG_ALREADY_OPTIMIZIED && its[3] == 0 && std::sqrt(e0) / n < 1e-6;
    }
    lcg_hip_dense_destroy(D);
    return ok ? 0 : 1;
}
