// sample_csr_multi_bicgstab.cpp -- several right-hand sides against a NON-SYMMETRIC matrix: 2-D convection-diffusion with first-order
// upwinding on a 100 x 100 grid (kron(I, T1) + kron(T2, I), T1 = tridiag(-1 - pe, 2 + pe, -1), T2 = tridiag(-1 - pe/2, 2 + pe/2, -1),
// pe = 2), generated here, solved against FOUR right-hand sides -- b = A.x* with x*_i = 1 + (i mod 7) / 7, 2 b, the first unit vector
// scaled, and a zero column -- by lcg_hip_lbicgstab_multi: first plain, then right-preconditioned with the handle's ILU(0) factor
// applied by 4 Jacobi sweeps per triangle.  Matrix and factor are read once per product / apply for all four columns; every column gets
// its own verdict and count, and its true residual |b - A.x| / n is recomputed on the host.  The preconditioned block holds the
// solution itself: nothing is applied after the loop.
// Plain C++ against the C ABI (include/lcg_hip.h): no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_multi_bicgstab.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_multi_bicgstab && ./sample_csr_multi_bicgstab
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <vector>

#include "lcg_hip.h"

// a block of k vectors: n * k doubles, row-major, the base 16-byte aligned (lcg_hip.h: lcg_hip_spmm)
struct Block {
    std::vector<double> store;
    double *p;
    Block(size_t n, int k) : store(n * k + 1, 0.0), p(store.data() + (((uintptr_t)store.data() & 15) ? 1 : 0)) {}
};

int main()
{
    const int g = 100, n = g * g, k = 4;
    const double pe = 2.0;
    std::vector<int> rowptr(1, 0), col;
    std::vector<double> val;
    for (int y = 0; y < g; y++)
        for (int x = 0; x < g; x++) {
            const int i = y * g + x;
            if (y > 0) { col.push_back(i - g); val.push_back(-1.0 - pe / 2); }
            if (x > 0) { col.push_back(i - 1); val.push_back(-1.0 - pe); }
            col.push_back(i); val.push_back(4.0 + 1.5 * pe);
            if (x < g - 1) { col.push_back(i + 1); val.push_back(-1.0); }
            if (y < g - 1) { col.push_back(i + g); val.push_back(-1.0); }
            rowptr.push_back((int)col.size());
        }
    std::vector<double> xs(n), b(n, 0.0);
    for (int i = 0; i < n; i++) xs[i] = 1.0 + (i % 7) / 7.0;
    for (int i = 0; i < n; i++)
        for (int e = rowptr[i]; e < rowptr[i + 1]; e++) b[i] += val[e] * xs[col[e]];

    lcg_hip_csr_t A = nullptr;
    int rc = lcg_hip_csr_create(&A, n, n, (int64_t)val.size(), rowptr.data(), col.data(), val.data(), 0, LCG_HIP_MEM_HOST, 0);
    if (rc) { std::cerr << "csr_create: " << lcg_hip_last_error() << "\n"; return 3; }
    rc = lcg_hip_csr_build_ilu0(A);
    if (!rc) rc = lcg_hip_csr_ilu0_set_sweeps(A, 4);
    if (rc) { std::cerr << "ILU(0): " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }

    Block B(n, k);
    for (int i = 0; i < n; i++) { B.p[(size_t)i * k + 0] = b[i]; B.p[(size_t)i * k + 1] = 2.0 * b[i]; }
    B.p[2] = 1e-3;                                      // column 2: the first unit vector, scaled; column 3 stays zero
    lcg_para para = lcg_hip_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 1;
    bool ok = true;
    int plain_its[k] = {0, 0, 0, 0};
    const int precond[2] = {LCG_HIP_M_NONE, LCG_HIP_M_ILU0};
    const char *name[2] = {"plain", "ilu0"};
    for (int run = 0; run < 2; run++) {
        Block M(n, k);
        int ret[k], its[k];
        double res[k];
        rc = lcg_hip_lbicgstab_multi(A, k, precond[run], M.p, B.p, &para, ret, its, res, LCG_HIP_MEM_HOST);
        if (rc) { std::cerr << "lcg_hip_lbicgstab_multi: rc=" << rc << " " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
        // each column's true residual |b - A.x| / n, summed on the host
        double tres[k] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < n; i++)
            for (int j = 0; j < k; j++) {
                double y = 0.0;
                for (int e = rowptr[i]; e < rowptr[i + 1]; e++) y += val[e] * M.p[(size_t)col[e] * k + j];
                const double d = B.p[(size_t)i * k + j] - y;
                tres[j] += d * d;
            }
        for (int j = 0; j < k; j++) {
            tres[j] = std::sqrt(tres[j]) / n;
            std::printf("%s column %d: ret=%d iterations=%d residual=%.3e true_residual=%.3e\n", name[run], j, ret[j], its[j], res[j], tres[j]);
            ok = ok && ret[j] == (j == 3 ? LCG_ALREADY_OPTIMIZIED : LCG_CONVERGENCE) && tres[j] < 2e-10;
            if (run == 0) plain_its[j] = its[j];
            else if (j < 3) ok = ok && its[j] < plain_its[j];
        }
        double e0 = 0.0;
        for (int i = 0; i < n; i++) { const double d0 = M.p[(size_t)i * k] - xs[i]; e0 += d0 * d0; }
        std::printf("%s averaged_error: column 0 %.3e; longest column: %d iterations\n", name[run], std::sqrt(e0) / n, lcg_hip_last_iterations());
        ok = ok && std::sqrt(e0) / n < 1e-6;
    }
    lcg_hip_csr_destroy(A);
    return ok ? 0 : 1;
}
