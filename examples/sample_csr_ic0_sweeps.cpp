// sample_csr_ic0_sweeps.cpp -- the run of sample_csr_ic0.cpp (sample8.cu's PCG leg on data/case_10K_A, preconditioned by IC(0))
// twice: with the factor applied exactly, level by level, and with lcg_hip_csr_ic0_set_sweeps(A, 4): four Jacobi sweeps per
// triangle, eight launches over all rows instead of a walk through L's levels.  Prints both iteration counts, the Jacobi
// count beside them, and the error against data/case_10K_B.  Plain C++: compile with g++ and link liblcg_hip.so.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_ic0_sweeps.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_ic0_sweeps && ./sample_csr_ic0_sweeps tests/golden
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
    rc = lcg_hip_csr_build_ic0(A);
    if (!rc) rc = lcg_hip_csr_build_jacobi(A, nullptr);
    if (rc) { std::cerr << "build: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }

    lcg_para para = lcg_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 1;
    std::vector<double> m(n);
    int bad = 0;
    const int sweeps[] = {0, 4, -1};                    // exact solves, four sweeps, Jacobi
    for (int k : sweeps) {
        int launches = 0, set = 0;
        if (k >= 0) {
            rc = lcg_hip_csr_ic0_set_sweeps(A, k);
            if (rc) { std::cerr << "ic0_set_sweeps: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
            lcg_hip_csr_ic0_get_sweeps(A, &set);
            lcg_hip_csr_ic0_info(A, nullptr, nullptr, &launches, nullptr, nullptr, nullptr);
        }
        std::fill(m.begin(), m.end(), 0.0);
        const int ret = lcg_solver_preconditioned(lcg_hip_csr_ax, k >= 0 ? lcg_hip_ic0_mx : lcg_hip_jacobi_mx, progress, m.data(),
                                                  b.data(), n, &para, A);
        const double err = avg_error(m, ans);
        if (k < 0) std::printf("PCG-Jacobi: ret=%d (%s) iterations: %d mean error: %.3e\n", ret, lcg_status_text(ret),
                               lcg_hip_last_iterations(), err);
        else std::printf("PCG-IC0 %s (sweeps %d, %d launches per apply): ret=%d (%s) iterations: %d mean error: %.3e\n",
                         k ? "sweeps" : "exact", set, launches, ret, lcg_status_text(ret), lcg_hip_last_iterations(), err);
        if (ret != 0 || !(err < 1e-6)) bad++;
    }
    lcg_hip_csr_destroy(A);
    return bad ? 1 : 0;
}
