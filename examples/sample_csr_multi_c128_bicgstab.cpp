// sample_csr_multi_c128_bicgstab.cpp -- several sources against one frequency in a medium with a one-way term: the 40 x 40 five-point
// Laplacian with a complex shift on the diagonal and an upwind convection term (west and south neighbours weigh more than east and
// north), so the matrix is complex, NOT symmetric and not Hermitian -- what clcg_hip_lbicg_sym_multi cannot take.  Solved against FOUR
// right-hand sides -- A.x_true, 1e-3 times it, a point source and a zero column (how a caller with three sources pads to k = 4) -- by
// the batched complex BiCGStab, plain and right-preconditioned with the built-in Jacobi.  Every column gets its own verdict, count
// and residual; the matrix is read twice per iteration for all four, and no product with A^H is taken.
// Plain C++ against the C ABI (include/lcg_hip_staging.h, which includes lcg_hip.h): no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_multi_c128_bicgstab.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_multi_c128_bicgstab && ./sample_csr_multi_c128_bicgstab
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <vector>

#include "lcg_hip_staging.h"

typedef std::complex<double> zc;

// a block of k complex vectors: n * k (re, im) pairs, row-major, the base 16-byte aligned (lcg_hip.h: clcg_hip_spmm)
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
    const int nx = 40, n = nx * nx, k = 4;
    // CSR of the shifted convection-diffusion operator, columns ascending; the shift 0.05 + 0.3i (0.2 + u_i), u_i in [0, 1) from a
    // small generator; upwind weights -1.5 (south, west) and -0.5 (east, north)
    std::vector<int> rp(1, 0), ci;
    std::vector<zc> val;
    uint32_t s = 12345u;
    for (int y = 0; y < nx; y++)
        for (int x = 0; x < nx; x++) {
            const int i = y * nx + x;
            s = s * 1664525u + 1013904223u;
            const double u = (s >> 8) * (1.0 / 16777216.0);
            if (y > 0) { ci.push_back(i - nx); val.push_back(-1.5); }
            if (x > 0) { ci.push_back(i - 1); val.push_back(-1.5); }
            ci.push_back(i); val.push_back(zc(4.05, 0.3 * (0.2 + u)));
            if (x < nx - 1) { ci.push_back(i + 1); val.push_back(-0.5); }
            if (y < nx - 1) { ci.push_back(i + nx); val.push_back(-0.5); }
            rp.push_back((int)ci.size());
        }
    lcg_hip_csr_t A = nullptr;
    int rc = lcg_hip_csr_create(&A, n, n, (int64_t)val.size(), rp.data(), ci.data(), reinterpret_cast<const double *>(val.data()), 1,
                                LCG_HIP_MEM_HOST, 0);
    if (rc) { std::cerr << "csr_create: " << lcg_hip_last_error() << "\n"; return 3; }
    lcg_hip_csr_build_jacobi(A, nullptr);

    std::vector<zc> xt(n), b(n, zc(0.0, 0.0));
    for (int i = 0; i < n; i++) xt[i] = zc(std::sin(0.7 * i), 0.5 * std::cos(0.31 * i));
    for (int i = 0; i < n; i++)
        for (int e = rp[i]; e < rp[i + 1]; e++) b[i] += val[e] * xt[ci[e]];
    Block B(n, k);
    for (int i = 0; i < n; i++) { B.p[(size_t)i * k + 0] = b[i]; B.p[(size_t)i * k + 1] = 1e-3 * b[i]; }
    B.p[(size_t)(n / 2 + nx / 2) * k + 2] = zc(1.0, 0.0);       // column 2: a point source; column 3 stays zero

    clcg_para para = clcg_hip_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 1;
    lcg_hip_set_shadow_seed(7);                                 // one shadow residual for all columns, drawn from this seed
    bool ok = true;
    for (int pre = 0; pre < 2; pre++) {
        Block M(n, k);
        int ret[k], its[k];
        double res[k];
        const char *name = pre ? "jacobi" : "plain";
        rc = clcg_hip_lbicgstab_multi(A, k, pre ? (int)LCG_HIP_M_JACOBI : (int)LCG_HIP_M_NONE, M.raw(), B.raw(), &para, ret, its, res,
                                      LCG_HIP_MEM_HOST);
        if (rc) { std::cerr << "clcg_hip_lbicgstab_multi: rc=" << rc << " " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
        for (int j = 0; j < k; j++) std::printf("%s column %d: ret=%d iterations=%d residual=%.3e\n", name, j, ret[j], its[j], res[j]);
        double e0 = 0.0;
        for (int i = 0; i < n; i++) e0 += std::norm(M.p[(size_t)i * k] - xt[i]);
        std::printf("%s averaged_error: column 0 %.3e; longest column: %d iterations\n", name, std::sqrt(e0) / n, lcg_hip_last_iterations());
        ok = ok && ret[0] == CLCG_CONVERGENCE && ret[1] == CLCG_CONVERGENCE && ret[2] == CLCG_CONVERGENCE &&
             ret[3] == CLCG_ALREADY_OPTIMIZIED && its[3] == 0 && std::sqrt(e0) / n < 1e-6;
    }
    lcg_hip_csr_destroy(A);
    return ok ? 0 : 1;
}
