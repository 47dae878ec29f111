// sample_csr_multi_ic0.cpp -- several right-hand sides AND a real preconditioner: data/case_10K_A (sample8.cu's system) solved
// against FOUR right-hand sides -- its own b, 2 b, the first unit vector scaled, and a zero column -- by lcg_hip_lpcg_multi_m with
// the handle's IC(0) factor applied by 4 Jacobi sweeps per triangle.  The matrix AND the factor are read once per iteration for all
// four columns; every column gets its own verdict and count, and its true residual |b - A.x| / n is recomputed on the host.
// Plain C++ against the C ABI (include/lcg_hip.h): no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_multi_ic0.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_multi_ic0 && ./sample_csr_multi_ic0 tests/golden
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
    rc = lcg_hip_csr_build_ic0(A);
    if (!rc) rc = lcg_hip_csr_ic0_set_sweeps(A, 4);
    if (rc) { std::cerr << "IC(0): " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }

    Block B(n, k), M(n, k);
    for (int i = 0; i < n; i++) { B.p[(size_t)i * k + 0] = b[i]; B.p[(size_t)i * k + 1] = 2.0 * b[i]; }
    B.p[2] = 1e-3;                                      // column 2: the first unit vector, scaled; column 3 stays zero
    lcg_para para = lcg_hip_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 1;
    int ret[k], its[k];
    double res[k];
    rc = lcg_hip_lpcg_multi_m(A, k, LCG_HIP_M_IC0, M.p, B.p, &para, ret, its, res, LCG_HIP_MEM_HOST);
    if (rc) { std::cerr << "lcg_hip_lpcg_multi_m: rc=" << rc << " " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
    // each column's true residual |b - A.x| / n, summed on the host from the COO entries
    double tres[k] = {0.0, 0.0, 0.0, 0.0};
    {
        Block Y(n, k);
        for (size_t e = 0; e < val.size(); e++)
            for (int j = 0; j < k; j++) Y.p[(size_t)row[e] * k + j] += val[e] * M.p[(size_t)col[e] * k + j];
        for (int i = 0; i < n; i++)
            for (int j = 0; j < k; j++) { const double d = B.p[(size_t)i * k + j] - Y.p[(size_t)i * k + j]; tres[j] += d * d; }
        for (int j = 0; j < k; j++) tres[j] = std::sqrt(tres[j]) / n;
    }
    for (int j = 0; j < k; j++)
        std::printf("column %d: ret=%d iterations=%d residual=%.3e true_residual=%.3e\n", j, ret[j], its[j], res[j], tres[j]);
    double e0 = 0.0, e1 = 0.0;
    for (int i = 0; i < n; i++) {
        const double d0 = M.p[(size_t)i * k] - ans[i], d1 = M.p[(size_t)i * k + 1] - 2.0 * ans[i];
        e0 += d0 * d0; e1 += d1 * d1;
    }
    std::printf("averaged_error: column 0 %.3e, column 1 %.3e; longest column: %d iterations\n", std::sqrt(e0) / n, std::sqrt(e1) / n,
                lcg_hip_last_iterations());
    lcg_hip_csr_destroy(A);
    const bool ok = ret[0] == LCG_CONVERGENCE && ret[1] == LCG_CONVERGENCE && ret[2] == LCG_CONVERGENCE && ret[3] == LCG_ALREADY_OPTIMIZIED &&
                    std::sqrt(e0) / n < 1e-6 && std::sqrt(e1) / n < 2e-6 && tres[0] < 2e-10 && tres[1] < 2e-10 && tres[2] < 2e-10;
    return ok ? 0 : 1;
}
