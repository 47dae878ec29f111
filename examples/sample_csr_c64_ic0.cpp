// sample_csr_c64_ic0.cpp -- liblcg's sample14.cu as that program runs it: the bundled complex system case_1K_cA cast to single
// precision, factored by an fp32 incomplete Cholesky IC(0) (sample14.cu: clcg_incomplete_Cholesky_cuda_half with cuComplex),
// solved by PCG with the two triangular solves L, then L^T, as the preconditioner (sample14.cu's MxProduct: two cusparseSpSV
// calls with CUDA_C_32F), epsilon = 1e-6 on |r|^2 / max(|m|, 1)^2, and the error against case_1K_cB reported as sample14 does
// (avg_error).  Plain C++ on the C ABI: no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_c64_ic0.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_c64_ic0 && ./sample_csr_c64_ic0 tests/golden
#include <cmath>
#include <complex>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "lcg_hip.h"

typedef std::complex<float> cf;

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

static float avg_error(const std::vector<cf> &a, const std::vector<cf> &b)
{   // sample14.cu's avg_error
    float s = 0.f;
    for (size_t i = 0; i < a.size(); i++) { const cf d = a[i] - b[i]; s += d.real() * d.real() + d.imag() * d.imag(); }
    return std::sqrt(s) / a.size();
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    int n = 0, n2 = 0;
    std::vector<int> row, col;
    std::vector<cf> val, b, ans;
    if (!read_system(dir + "/case_1K_cA", n, row, col, val, b)) { std::cerr << "cannot read " << dir << "/case_1K_cA\n"; return 2; }
    {
        std::ifstream in(dir + "/case_1K_cB", std::ios::binary);
        in.read((char *)&n2, sizeof(int));
        ans.resize(n2);
        for (int i = 0; i < n2; i++) { double v[2]; in.read((char *)v, sizeof v); ans[i] = cf((float)v[0], (float)v[1]); }
        if (!in || n2 != n) { std::cerr << "cannot read " << dir << "/case_1K_cB\n"; return 2; }
    }
    // COO -> CSR on the host (sample14.cu: cusparseXcoo2csr)
    std::vector<int> rowptr(n + 1, 0), cidx(col.size());
    std::vector<cf> cval(val.size());
    for (size_t k = 0; k < row.size(); k++) rowptr[row[k] + 1]++;
    for (int i = 0; i < n; i++) rowptr[i + 1] += rowptr[i];
    {
        std::vector<int> next(rowptr.begin(), rowptr.end() - 1);
        for (size_t k = 0; k < row.size(); k++) { const int p = next[row[k]]++; cidx[p] = col[k]; cval[p] = val[k]; }
    }
    lcg_hip_csr_t A = nullptr;
    int rc = lcg_hip_csr_create_c64(&A, n, n, (int64_t)cval.size(), rowptr.data(), cidx.data(),
                                    reinterpret_cast<const float *>(cval.data()), LCG_HIP_MEM_HOST, 0);
    if (rc) { std::cerr << "csr_create_c64: " << lcg_hip_last_error() << "\n"; return 3; }
    // the fp32 factor and both level schedules (sample14.cu: clcg_incomplete_Cholesky_cuda_half, cusparseSpSV_analysis x 2)
    rc = lcg_hip_csr_build_ic0_c64(A);
    if (rc) { std::cerr << "build_ic0_c64: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
    int lev_l = 0, lev_u = 0, launches = 0;
    double build_ms = 0.0;
    int64_t bytes = 0;
    lcg_hip_csr_ic0_info(A, &lev_l, &lev_u, &launches, nullptr, &build_ms, &bytes);
    std::printf("IC(0) c64: levels %d / %d, %d launches per apply, build %.2f ms, %lld bytes\n", lev_l, lev_u, launches, build_ms,
                (long long)bytes);

    clcg_para para = clcg_hip_default_parameters();
    para.epsilon = 1e-6; para.abs_diff = 0;         // sample14.cu
    para.max_iterations = 1000;                     // (sample14 runs uncapped; a guard only)
    std::vector<cf> m(n, cf(0.f, 0.f));
    const int ret = clcg_hip_solver_preconditioned_c64(clcg_hip_csr_ax_c64, clcg_hip_ic0_mx_c64, nullptr,
                                                       reinterpret_cast<float *>(m.data()), reinterpret_cast<const float *>(b.data()),
                                                       n, &para, A, CLCG_PCG, LCG_HIP_MEM_HOST);
    if (ret <= LCG_HIP_E_RUNTIME) { std::cerr << "solver: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
    std::printf("PCG-IC0: ret=%d iterations: %d residual: %.3e\n", ret, lcg_hip_last_iterations(), lcg_hip_last_residual());
    std::printf("Averaged error (compared with ans_x): %.6e\n", (double)avg_error(m, ans));
    lcg_hip_csr_destroy(A);
    return ret == CLCG_CONVERGENCE ? 0 : 1;
}
