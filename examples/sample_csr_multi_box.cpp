// sample_csr_multi_box.cpp -- bounds on the model, several data vectors in one call: data/case_10K_A solved between -5 and 8 against
// FOUR right-hand sides -- its own b, 1e-6 b (its solution lies inside the box), a fixed pseudo-random vector and a zero column (how a
// caller with three right-hand sides pads to k = 4) -- by lcg_hip_solver_constrained_multi, once with the projected gradient (LCG_PG)
// and once with the spectral projected gradient (LCG_SPG), capped at 40 iterations.  Every column gets its own verdict, count, residual
// and the number of A.x products liblcg's lcg_solver_constrained would have spent on it alone; the matrix is read once per trial
// step for all four, and the line search runs on the device.
// Plain C++ against the C ABI (include/lcg_hip_staging_box_multi.h, which includes lcg_hip.h): no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_multi_box.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_multi_box && ./sample_csr_multi_box tests/golden
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "lcg_hip_staging_box_multi.h"

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
    int n = 0;
    std::vector<int> row, col;
    std::vector<double> val, b;
    if (!read_system(dir + "/case_10K_A", n, row, col, val, b)) { std::cerr << "cannot read " << dir << "/case_10K_A\n"; return 2; }
    lcg_hip_csr_t A = nullptr;
    int rc = lcg_hip_csr_from_coo(&A, n, (int64_t)val.size(), row.data(), col.data(), val.data(), 0, LCG_HIP_MEM_HOST);
    if (rc) { std::cerr << "csr_from_coo: " << lcg_hip_last_error() << "\n"; return 3; }

    Block B(n, k);
    uint64_t s = 88172645463325252ull;                  // xorshift64: column 2
    for (int i = 0; i < n; i++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        B.p[(size_t)i * k + 0] = b[i];
        B.p[(size_t)i * k + 1] = 1e-6 * b[i];
        B.p[(size_t)i * k + 2] = (double)(s >> 11) / 9007199254740992.0 - 0.5;
    }
    std::vector<double> low(n, -5.0), hig(n, 8.0);      // one pair of bounds per row, shared by all columns
    lcg_para para = lcg_hip_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 1; para.max_iterations = 40;
    bool ok = true;
    const int solvers[2] = {LCG_PG, LCG_SPG};
    for (int q = 0; q < 2; q++) {
        Block M(n, k);
        int ret[k], its[k], products[k];
        double res[k];
        rc = lcg_hip_solver_constrained_multi(A, k, solvers[q], M.p, B.p, low.data(), hig.data(), &para, ret, its, products, res, LCG_HIP_MEM_HOST);
        if (rc) { std::cerr << "lcg_hip_solver_constrained_multi: rc=" << rc << " " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
        std::printf("%s\n", q ? "LCG_SPG" : "LCG_PG");
        int active = 0;
        for (size_t i = 0; i < (size_t)n * k; i++) {
            ok = ok && M.p[i] >= -5.0 && M.p[i] <= 8.0;
            if (i % k == 0 && (M.p[i] <= -5.0 || M.p[i] >= 8.0)) active++;
        }
        for (int j = 0; j < k; j++) std::printf("column %d: ret=%d iterations=%d products=%d residual=%.3e\n", j, ret[j], its[j], products[j], res[j]);
        std::printf("column 0: %d components at a bound\n", active);
        ok = ok && active > 0 && ret[3] == LCG_ALREADY_OPTIMIZIED && products[3] == 1;
        for (int j = 0; j < 3; j++) ok = ok && ret[j] == LCG_REACHED_MAX_ITERATIONS && its[j] == 40 && products[j] >= 41;
    }
    lcg_hip_csr_destroy(A);
    return ok ? 0 : 1;
}
