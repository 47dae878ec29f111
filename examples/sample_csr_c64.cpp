// sample_csr_c64.cpp -- liblcg's sample14.cu on the complex64 entries: the bundled complex system case_10K_cA cast to single
// precision (sample14.cu:154-170), solved with BiCG for complex-symmetric A and with PCG, and the error against case_10K_cB
// reported as sample14 does (avg_error, sample14.cu:71-81).  sample14 preconditions its PCG with an fp32 IC(0); this one uses
// the ready-made Jacobi (clcg_hip_jacobi_mx_c64), and sample_csr_c64_ic0.cpp runs sample14's IC(0) leg.  Plain C++ on the C ABI:
// no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_c64.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_c64 && ./sample_csr_c64 tests/golden
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
{   // sample14.cu:71-81
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
    if (!read_system(dir + "/case_10K_cA", n, row, col, val, b)) { std::cerr << "cannot read " << dir << "/case_10K_cA\n"; return 2; }
    {
        std::ifstream in(dir + "/case_10K_cB", std::ios::binary);
        in.read((char *)&n2, sizeof(int));
        ans.resize(n2);
        for (int i = 0; i < n2; i++) { double v[2]; in.read((char *)v, sizeof v); ans[i] = cf((float)v[0], (float)v[1]); }
        if (!in || n2 != n) { std::cerr << "cannot read " << dir << "/case_10K_cB\n"; return 2; }
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
    rc = lcg_hip_csr_build_jacobi(A, nullptr);
    if (rc) { std::cerr << "build_jacobi: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }

    clcg_para para = clcg_hip_default_parameters();
    para.epsilon = 1e-6; para.abs_diff = 0;         // sample14.cu:254-255
    para.max_iterations = 1000;
    int worst = 0;
    for (int leg = 0; leg < 2; leg++) {
        std::vector<cf> m(n, cf(0.f, 0.f));
        float *mp = reinterpret_cast<float *>(m.data());
        const float *bp = reinterpret_cast<const float *>(b.data());
        const int ret = leg == 0 ? clcg_hip_solver_c64(clcg_hip_csr_ax_c64, nullptr, mp, bp, n, &para, A, CLCG_BICG_SYM, LCG_HIP_MEM_HOST)
                                 : clcg_hip_solver_preconditioned_c64(clcg_hip_csr_ax_c64, clcg_hip_jacobi_mx_c64, nullptr, mp, bp, n, &para,
                                                                      A, CLCG_PCG, LCG_HIP_MEM_HOST);
        if (ret <= LCG_HIP_E_RUNTIME) { std::cerr << "solver: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
        std::printf("%s: ret=%d iterations: %d residual: %.3e\n", leg == 0 ? "BiCG-sym" : "PCG-Jacobi", ret, lcg_hip_last_iterations(),
                    lcg_hip_last_residual());
        std::printf("Averaged error (compared with ans_x): %.6e\n", (double)avg_error(m, ans));
        if (ret != CLCG_CONVERGENCE && ret != LCG_REACHED_MAX_ITERATIONS) worst = 1;
    }
    lcg_hip_csr_destroy(A);
    return worst;
}
