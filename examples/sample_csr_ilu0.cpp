// sample_csr_ilu0.cpp -- liblcg's sample11.cu as that program runs it: a complex symmetric system solved by CLCG_PCG
// preconditioned with incomplete LU, ILU(0) (csrilu02 and two csrsv2 solves, unit-lower L then U, as the Mfp callback), here on
// data/case_10K_cA (sample11's own case_1M_cA is not bundled) -- and what liblcg has no loop for: a real NON-symmetric system
// (2-D convection-diffusion, first-order upwinding) solved by BiCGStab, plain and right-preconditioned by the same factor:
// Afp = lcg_hip_csr_ax_ilu0 computes A.(U^-1 L^-1 u), and x = U^-1 L^-1 u after the solve.
// Plain C++ against the C ABI (include/lcg_hip.h): no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_ilu0.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_ilu0 && ./sample_csr_ilu0 tests/golden
#include <cmath>
#include <complex>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "lcg_hip.h"

typedef std::complex<double> cplx;

static bool read_complex_system(const std::string &path, int &n, std::vector<int> &row, std::vector<int> &col,
                                std::vector<cplx> &val, std::vector<cplx> &b)
{   // data/README: n, nz, then (row, col, re, im) triplets, then b
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    int nz = 0;
    in.read((char *)&n, sizeof(int)); in.read((char *)&nz, sizeof(int));
    row.resize(nz); col.resize(nz); val.resize(nz); b.resize(n);
    for (int i = 0; i < nz; i++) {
        in.read((char *)&row[i], sizeof(int)); in.read((char *)&col[i], sizeof(int)); in.read((char *)&val[i], sizeof(cplx));
    }
    in.read((char *)b.data(), sizeof(cplx) * n);
    return (bool)in;
}

static void print_info(lcg_hip_csr_t A)
{
    int lev_l = 0, lev_u = 0, launches = 0, zero_pivot = 0;
    double build_ms = 0.0;
    int64_t bytes = 0;
    lcg_hip_csr_ilu0_info(A, &lev_l, &lev_u, &launches, &zero_pivot, &build_ms, &bytes);
    std::printf("ILU(0): levels %d / %d, %d launches per apply, build %.2f ms, %lld bytes\n", lev_l, lev_u, launches, build_ms,
                (long long)bytes);
}

// sample11's flow: factor, then PCG with z = U^-1 L^-1 r as Mfp
static int complex_leg(const std::string &dir)
{
    int n = 0, n2 = 0;
    std::vector<int> row, col;
    std::vector<cplx> val, b, ans;
    if (!read_complex_system(dir + "/case_10K_cA", n, row, col, val, b)) { std::cerr << "cannot read " << dir << "/case_10K_cA\n"; return 2; }
    {
        std::ifstream in(dir + "/case_10K_cB", std::ios::binary);
        in.read((char *)&n2, sizeof(int)); ans.resize(n2); in.read((char *)ans.data(), sizeof(cplx) * n2);
    }
    lcg_hip_csr_t A = nullptr;
    int rc = lcg_hip_csr_from_coo(&A, n, (int64_t)val.size(), row.data(), col.data(), (const double *)val.data(), 1, LCG_HIP_MEM_HOST);
    if (rc) { std::cerr << "csr_from_coo: " << lcg_hip_last_error() << "\n"; return 3; }
    rc = lcg_hip_csr_build_ilu0(A);                      // sample11.cu: csrilu02 analysis + factor, csrsv2 analysis of L and U
    if (rc) { std::cerr << "build_ilu0: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
    print_info(A);
    clcg_para para = clcg_hip_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 1;
    std::vector<cplx> m(n, cplx(0.0, 0.0));
    const int ret = clcg_hip_solver_preconditioned(clcg_hip_csr_ax, clcg_hip_ilu0_mx, nullptr, (double *)m.data(), (const double *)b.data(), n,
                                                   &para, A, CLCG_PCG, LCG_HIP_MEM_HOST);
    double s = 0.0;
    for (int i = 0; i < n; i++) s += std::norm(m[i] - ans[i]);
    std::printf("PCG-ILU0 (complex): ret=%d iterations: %d error: %.3e\n", ret, lcg_hip_last_iterations(), std::sqrt(s));
    lcg_hip_csr_destroy(A);
    return ret != 0 || !(std::sqrt(s) <= 1e-5) ? 1 : 0;
}

// kron(I, T1) + kron(T2, I) on a k x k grid, T1 = tridiag(-1 - pe, 2 + pe, -1), T2 = tridiag(-1 - pe/2, 2 + pe/2, -1): rows sorted
static void convdiff(int k, double pe, std::vector<int> &rp, std::vector<int> &ci, std::vector<double> &v)
{
    rp.assign(1, 0);
    for (int y = 0; y < k; y++)
        for (int x = 0; x < k; x++) {
            const int i = y * k + x;
            if (y > 0) { ci.push_back(i - k); v.push_back(-1.0 - pe / 2); }
            if (x > 0) { ci.push_back(i - 1); v.push_back(-1.0 - pe); }
            ci.push_back(i); v.push_back((2.0 + pe) + (2.0 + pe / 2));
            if (x + 1 < k) { ci.push_back(i + 1); v.push_back(-1.0); }
            if (y + 1 < k) { ci.push_back(i + k); v.push_back(-1.0); }
            rp.push_back((int)ci.size());
        }
}

static void product(const std::vector<int> &rp, const std::vector<int> &ci, const std::vector<double> &v, const std::vector<double> &x,
                    std::vector<double> &y)
{
    for (size_t i = 0; i + 1 < rp.size(); i++) {
        double s = 0.0;
        for (int p = rp[i]; p < rp[i + 1]; p++) s += v[p] * x[ci[p]];
        y[i] = s;
    }
}

static int real_leg()
{
    const int k = 64, n = k * k;
    std::vector<int> rp, ci;
    std::vector<double> v, xs(n), b(n);
    convdiff(k, 1.0, rp, ci, v);
    for (int i = 0; i < n; i++) xs[i] = 1.0 + (i % 10) / 10.0;
    product(rp, ci, v, xs, b);
    lcg_hip_csr_t A = nullptr;
    int rc = lcg_hip_csr_create(&A, n, n, (int64_t)v.size(), rp.data(), ci.data(), v.data(), 0, LCG_HIP_MEM_HOST, 0);
    if (rc) { std::cerr << "csr_create: " << lcg_hip_last_error() << "\n"; return 3; }
    rc = lcg_hip_csr_build_ilu0(A);
    if (rc) { std::cerr << "build_ilu0: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
    print_info(A);
    lcg_para para = lcg_hip_default_parameters();
    para.epsilon = 1e-10;
    std::vector<double> m(n, 0.0), u(n, 0.0), x(n), r(n);
    int ret = lcg_hip_solver(lcg_hip_csr_ax, nullptr, m.data(), b.data(), n, &para, A, LCG_BICGSTAB, LCG_HIP_MEM_HOST);
    std::printf("BiCGStab plain: ret=%d iterations: %d\n", ret, lcg_hip_last_iterations());
    // right preconditioning: A.M^-1 u = b from u = 0 ...
    const int ret2 = lcg_hip_solver(lcg_hip_csr_ax_ilu0, nullptr, u.data(), b.data(), n, &para, A, LCG_BICGSTAB, LCG_HIP_MEM_HOST);
    const int it2 = lcg_hip_last_iterations();
    // ... then x = U^-1 L^-1 u.  A program whose vectors live on the device calls lcg_hip_ilu0_solve(A, 2, u, x); this one keeps
    // host vectors, so it takes the factor home once and does the two substitutions here.
    std::vector<int> lrp(n + 1), urp(n + 1);
    const int *d_rp = nullptr, *d_ci = nullptr;
    const double *d_v = nullptr;
    lcg_hip_csr_ilu0_factor(A, 0, &d_rp, &d_ci, &d_v);
    lcg_hip_memcpy(lrp.data(), d_rp, sizeof(int) * (n + 1), 2);
    std::vector<int> lci(lrp[n] + 1); std::vector<double> lv(lrp[n] + 1);
    lcg_hip_memcpy(lci.data(), d_ci, sizeof(int) * lrp[n], 2); lcg_hip_memcpy(lv.data(), d_v, sizeof(double) * lrp[n], 2);
    lcg_hip_csr_ilu0_factor(A, 1, &d_rp, &d_ci, &d_v);
    lcg_hip_memcpy(urp.data(), d_rp, sizeof(int) * (n + 1), 2);
    std::vector<int> uci(urp[n]); std::vector<double> uv(urp[n]);
    lcg_hip_memcpy(uci.data(), d_ci, sizeof(int) * urp[n], 2); lcg_hip_memcpy(uv.data(), d_v, sizeof(double) * urp[n], 2);
    for (int i = 0; i < n; i++) {                       // L has a unit diagonal that is not stored
        double s = u[i];
        for (int p = lrp[i]; p < lrp[i + 1]; p++) s -= lv[p] * x[lci[p]];
        x[i] = s;
    }
    for (int i = n - 1; i >= 0; i--) {                  // U's rows begin with the diagonal
        double s = x[i];
        for (int p = urp[i] + 1; p < urp[i + 1]; p++) s -= uv[p] * x[uci[p]];
        x[i] = s / uv[urp[i]];
    }
    product(rp, ci, v, x, r);
    double rr = 0.0, bb = 0.0, ee = 0.0;
    for (int i = 0; i < n; i++) { rr += (b[i] - r[i]) * (b[i] - r[i]); bb += b[i] * b[i]; ee += (x[i] - xs[i]) * (x[i] - xs[i]); }
    std::printf("BiCGStab right ILU0: ret=%d iterations: %d residual: %.3e error: %.3e\n", ret2, it2, std::sqrt(rr / bb), std::sqrt(ee));
    lcg_hip_csr_destroy(A);
    return ret != 0 || ret2 != 0 || !(std::sqrt(rr / bb) < 1e-4) ? 1 : 0;
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    const int a = complex_leg(dir);
    const int b = real_leg();
    return a ? a : b;
}
