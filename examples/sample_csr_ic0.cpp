// sample_csr_ic0.cpp -- the PCG leg of liblcg's sample8.cu as that program runs it: preconditioned by incomplete
// Cholesky IC(0) (sample8.cu:105-119,183-238) instead of the Jacobi of sample_csr.cpp.  Reads data/case_10K_A, solves,
// reports the error against data/case_10K_B, written against liblcg's own entry points (include/lcg_dropin.hpp).
// Plain C++: no HIP headers, no vendor handles -- compile with g++ and link liblcg_hip.so.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_ic0.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_ic0 && ./sample_csr_ic0 tests/golden
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "lcg_dropin.hpp"

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

static double avg_error(const std::vector<double> &a, const std::vector<double> &b)
{   // sample8.cu:66-74
    double s = 0.0;
    for (size_t i = 0; i < a.size(); i++) s += (a[i] - b[i]) * (a[i] - b[i]);
    return std::sqrt(s) / a.size();
}

static int progress(void *, const lcg_float *, const lcg_float converge, const lcg_para *param, const int, const int k)
{   // sample8.cu:122-129
    if (converge <= param->epsilon) std::clog << "Iteration-times: " << k << "\tconvergence: " << converge << std::endl;
    return 0;
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
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
    // sample8.cu:183-238 (csric02 analysis + factor, csrsv2 analysis of L and L^T) in one call
    rc = lcg_hip_csr_build_ic0(A);
    if (rc) { std::cerr << "build_ic0: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
    int lev_l = 0, lev_u = 0, launches = 0, zero_pivot = 0;
    double build_ms = 0.0;
    int64_t bytes = 0;
    lcg_hip_csr_ic0_info(A, &lev_l, &lev_u, &launches, &zero_pivot, &build_ms, &bytes);
    std::printf("IC(0): levels %d / %d, %d launches per apply, build %.2f ms, %lld bytes\n", lev_l, lev_u, launches, build_ms,
                (long long)bytes);

    lcg_para para = lcg_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 1;
    std::vector<double> m(n, 0.0);
    // the PCG leg of sample8.cu, its MxProduct being the two triangular solves (sample8.cu:105-119)
    const int ret = lcg_solver_preconditioned(lcg_hip_csr_ax, lcg_hip_ic0_mx, progress, m.data(), b.data(), n, &para, A);
    const double err = avg_error(m, ans);
    std::printf("PCG-IC0: ret=%d (%s) iterations: %d mean error: %.3e\n", ret, lcg_status_text(ret), lcg_hip_last_iterations(), err);
    lcg_hip_csr_destroy(A);
    return ret != 0 || !(err < 1e-6) ? 1 : 0;
}
