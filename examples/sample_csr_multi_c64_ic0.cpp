// sample_csr_multi_c64_ic0.cpp -- liblcg's sample14.cu flow for FOUR sources at once: the bundled complex system case_10K_cA cast to
// single precision, factored by the fp32 incomplete Cholesky IC(0), and solved against four right-hand sides -- its own b, 2 b, the
// first unit vector, and a zero column -- by clcg_hip_lpcg_multi_m_c64 with the factor's two triangular solves applied to all four
// columns at once (sample14.cu: one clcg_solver_cuda call per source, two cusparseSpSV calls per iteration each).  The matrix AND
// the factor are read once per iteration for all four columns; every column gets its own verdict and count under sample14's stop
// rule, epsilon = 1e-6 on |r|^2 / max(|m|, 1)^2, and that quantity is recomputed on the host in double from the returned iterate
// (true_residual).  lcg_hip_csr_ic0_set_sweeps(A, s) before the solve would apply the factor by s Jacobi sweeps per triangle instead.
// Plain C++ against the C ABI (include/lcg_hip_staging_ic0_c64.h, which includes lcg_hip.h): no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_multi_c64_ic0.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_multi_c64_ic0 && ./sample_csr_multi_c64_ic0 tests/golden
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "lcg_hip_staging_ic0_c64.h"

typedef std::complex<float> cf;
typedef std::complex<double> cd;

static bool read_system(const std::string &path, int &n, std::vector<int> &row, std::vector<int> &col, std::vector<cf> &val,
                        std::vector<cf> &b)
{   // data/README:1-10: complex values as interleaved doubles, cast to single precision
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    int nz = 0;
    in.read((char *)&n, sizeof(int)); in.read((char *)&nz, sizeof(int));
    row.resize(nz); col.resize(nz); val.resize(nz); b.resize(n);
    for (int i = 0; i < nz; i++) {
        double v[2];
        in.read((char *)&row[i], sizeof(int)); in.read((char *)&col[i], sizeof(int)); in.read((char *)v, sizeof v);
        val[i] = cf((float)v[0], (float)v[1]);
    }
    for (int i = 0; i < n; i++) { double v[2]; in.read((char *)v, sizeof v); b[i] = cf((float)v[0], (float)v[1]); }
    return (bool)in;
}

// a block of k complex64 vectors: n * k (re, im) float pairs, row-major, the base 16-byte aligned (lcg_hip.h: clcg_hip_spmm_c64)
struct Block {
    std::vector<cf> store;
    cf *p;
    Block(size_t n, int k) : store(n * k + 1, cf(0.f, 0.f)), p(store.data() + (((uintptr_t)store.data() & 15) ? 1 : 0)) {}
    float *f() { return reinterpret_cast<float *>(p); }
};

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    const int k = 4;
    int n = 0;
    std::vector<int> row, col;
    std::vector<cf> val, b;
    if (!read_system(dir + "/case_10K_cA", n, row, col, val, b)) { std::cerr << "cannot read " << dir << "/case_10K_cA\n"; return 2; }
    // COO -> CSR on the host (sample14.cu: cusparseXcoo2csr)
    std::vector<int> rowptr(n + 1, 0), cidx(col.size());
    std::vector<cf> cval(val.size());
    for (size_t e = 0; e < row.size(); e++) rowptr[row[e] + 1]++;
    for (int i = 0; i < n; i++) rowptr[i + 1] += rowptr[i];
    {
        std::vector<int> next(rowptr.begin(), rowptr.end() - 1);
        for (size_t e = 0; e < row.size(); e++) { const int p = next[row[e]]++; cidx[p] = col[e]; cval[p] = val[e]; }
    }
    lcg_hip_csr_t A = nullptr;
    int rc = lcg_hip_csr_create_c64(&A, n, n, (int64_t)cval.size(), rowptr.data(), cidx.data(),
                                    reinterpret_cast<const float *>(cval.data()), LCG_HIP_MEM_HOST, 0);
    if (rc) { std::cerr << "csr_create_c64: " << lcg_hip_last_error() << "\n"; return 3; }
    rc = lcg_hip_csr_build_ic0_c64(A);
    if (rc) { std::cerr << "build_ic0_c64: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
    int launches = 0;
    lcg_hip_csr_ic0_info(A, nullptr, nullptr, &launches, nullptr, nullptr, nullptr);
    std::printf("IC(0) c64: %d launches per apply, for all %d columns\n", launches, k);

    Block B(n, k), M(n, k);
    for (int i = 0; i < n; i++) { B.p[(size_t)i * k + 0] = b[i]; B.p[(size_t)i * k + 1] = 2.0f * b[i]; }
    B.p[2] = cf(1.f, 0.f);                              // column 2: the first unit vector; column 3 stays zero
    clcg_para para = clcg_hip_default_parameters();
    para.epsilon = 1e-6; para.abs_diff = 0;             // sample14.cu
    para.max_iterations = 1000;                         // (sample14 runs uncapped; a guard only)
    int ret[k], its[k];
    double res[k];
    rc = clcg_hip_lpcg_multi_m_c64(A, k, LCG_HIP_M_IC0, M.f(), B.f(), &para, ret, its, res, LCG_HIP_MEM_HOST);
    if (rc) { std::cerr << "clcg_hip_lpcg_multi_m_c64: rc=" << rc << " " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
    // each column's |b - A.x|^2 / max(|x|, 1)^2 in double, summed on the host from the COO entries
    double tres[k];
    {
        std::vector<cd> Y((size_t)n * k, cd(0.0, 0.0));
        for (size_t e = 0; e < val.size(); e++)
            for (int j = 0; j < k; j++) Y[(size_t)row[e] * k + j] += cd(val[e]) * cd(M.p[(size_t)col[e] * k + j]);
        for (int j = 0; j < k; j++) {
            double r2 = 0.0, m2 = 0.0;
            for (int i = 0; i < n; i++) {
                r2 += std::norm(cd(B.p[(size_t)i * k + j]) - Y[(size_t)i * k + j]);
                m2 += std::norm(cd(M.p[(size_t)i * k + j]));
            }
            tres[j] = r2 / std::max(m2, 1.0);
        }
    }
    for (int j = 0; j < k; j++)
        std::printf("column %d: ret=%d iterations=%d residual=%.3e true_residual=%.3e\n", j, ret[j], its[j], res[j], tres[j]);
    std::printf("longest column: %d iterations\n", lcg_hip_last_iterations());
    lcg_hip_csr_destroy(A);
    const bool ok = ret[0] == CLCG_CONVERGENCE && ret[1] == CLCG_CONVERGENCE && ret[2] == CLCG_CONVERGENCE && ret[3] == CLCG_ALREADY_OPTIMIZIED;
    return ok ? 0 : 1;
}
