// sample_csr_multi.cpp -- several right-hand sides in one call: data/case_10K_A (sample8.cu's system) solved against FOUR
// right-hand sides -- its own b, 2 b, the first unit vector scaled, and a zero column (how a caller with three right-hand sides pads
// to k = 4) -- by lcg_hip_lpcg_multi: batched PCG with the built-in Jacobi.  Every column gets its own verdict, count and residual;
// the matrix is read once per iteration for all four.
// Plain C++ against the C ABI (include/lcg_hip.h): no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_multi.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_multi && ./sample_csr_multi tests/golden
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "lcg_hip.h"

static bool read_system(const std::string &path, int &n, std::vector<int> &row, std::vector<int> &col,
                        std::vector<double> &val, std::vector<double> &b)
{   // data/README:1-10
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    int nz = 0;
    in.read((char *)&n, sizeof(int)); in.read((char *)&nz, sizeof(int));
    row.resize(nz); col.resize(nz); val.resize(nz); b.resize(n);
    for (int i = 0; i < nz; i++) {
        in.read((char *)&row[i], sizeof(int)); in.read((char *)&col[i], sizeof(int)); in.read((char *)&val[i], sizeof(double));
    }
    in.read((char *)b.data(), sizeof(double) * n);
    return (bool)in;
}

// a block of k vectors: n * k doubles, row-major, the base 16-byte aligned (lcg_hip.h: lcg_hip_spmm)
struct Block {
    std::vector<double> store;
    double *p;
    Block(size_t n, int k) : store(n * k + 1, 0.0), p(store.data() + (((uintptr_t)store.data() & 15) ? 1 : 0)) {}
};

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    const int k = 4;
    int n = 0, n2 = 0;
    std::vector<int> row, col;
    std::vector<double> val, b, ans;
    if (!read_system(dir + "/case_10K_A", n, row, col, val, b)) { std::cerr << "cannot read " << dir << "/case_10K_A\n"; return 2; }
    {
        std::ifstream in(dir + "/case_10K_B", std::ios::binary);
        in.read((char *)&n2, sizeof(int)); ans.resize(n2); in.read((char *)ans.data(), sizeof(double) * n2);
    }
    lcg_hip_csr_t A = nullptr;
    int rc = lcg_hip_csr_from_coo(&A, n, (int64_t)val.size(), row.data(), col.data(), val.data(), 0, LCG_HIP_MEM_HOST);
    if (rc) { std::cerr << "csr_from_coo: " << lcg_hip_last_error() << "\n"; return 3; }
    lcg_hip_csr_build_jacobi(A, nullptr);

    Block B(n, k), M(n, k);
    for (int i = 0; i < n; i++) { B.p[(size_t)i * k + 0] = b[i]; B.p[(size_t)i * k + 1] = 2.0 * b[i]; }
    B.p[2] = 1e-3;                                      // column 2: the first unit vector, scaled; column 3 stays zero
    lcg_para para = lcg_hip_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 1;
    int ret[k], its[k];
    double res[k];
    rc = lcg_hip_lpcg_multi(A, k, M.p, B.p, &para, ret, its, res, LCG_HIP_MEM_HOST);
    if (rc) { std::cerr << "lcg_hip_lpcg_multi: rc=" << rc << " " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
    for (int j = 0; j < k; j++) std::printf("column %d: ret=%d iterations=%d residual=%.3e\n", j, ret[j], its[j], res[j]);
    double e0 = 0.0, e1 = 0.0;
    for (int i = 0; i < n; i++) {
        const double d0 = M.p[(size_t)i * k] - ans[i], d1 = M.p[(size_t)i * k + 1] - 2.0 * ans[i];
        e0 += d0 * d0; e1 += d1 * d1;
    }
    std::printf("averaged_error: column 0 %.3e, column 1 %.3e; longest column: %d iterations\n", std::sqrt(e0) / n, std::sqrt(e1) / n,
                lcg_hip_last_iterations());
    lcg_hip_csr_destroy(A);
    const bool ok = ret[0] == LCG_CONVERGENCE && ret[1] == LCG_CONVERGENCE && ret[2] == LCG_CONVERGENCE && ret[3] == LCG_ALREADY_OPTIMIZIED &&
                    std::sqrt(e0) / n < 1e-6 && std::sqrt(e1) / n < 2e-6;
    return ok ? 0 : 1;
}
