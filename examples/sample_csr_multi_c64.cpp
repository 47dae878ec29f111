// sample_csr_multi_c64.cpp -- several sources against one frequency in single precision: sample14.cu's system (the bundled complex
// case_10K_cA cast to complex64, sample14.cu:154-170) solved against EIGHT right-hand sides -- its own b scaled by 1, 1/2, -1, 2,
// 1/4, -1/2, 4 and -2, so that case_10K_cB scaled alike is every column's answer -- once as ONE batch (clcg_hip_lbicg_sym_multi_c64,
// then clcg_hip_lpcg_multi_c64 with the built-in Jacobi: the matrix is read once per iteration for all eight) and once as eight
// single solves (clcg_hip_solver_c64 / clcg_hip_solver_preconditioned_c64).  Every column's code, count and averaged error
// (sample14.cu:71-81) is printed for both.  Plain C++ against the C ABI (include/lcg_hip.h): no HIP headers, no vendor handles.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_multi_c64.cpp -Lliblcg_amd/lib -llcg_hip
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_multi_c64 && ./sample_csr_multi_c64 tests/golden
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "lcg_hip.h"

typedef std::complex<float> cf;

// a block of k complex64 vectors: n * k (re, im) float pairs, row-major, the base 16-byte aligned (lcg_hip.h: clcg_hip_spmm_c64)
struct Block {
    std::vector<float> store;
    cf *p;
    Block(size_t n, int k) : store(2 * n * k + 4, 0.f)
    {
        float *d = store.data();
        while ((uintptr_t)d & 15) d++;
        p = reinterpret_cast<cf *>(d);
    }
    float *raw() { return reinterpret_cast<float *>(p); }
};

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

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    const int k = 8;
    const float scale[k] = {1.f, 0.5f, -1.f, 2.f, 0.25f, -0.5f, 4.f, -2.f};
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
    rc = lcg_hip_csr_build_jacobi(A, nullptr);
    if (rc) { std::cerr << "build_jacobi: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }

    Block B(n, k);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < k; j++) B.p[(size_t)i * k + j] = scale[j] * b[i];

    clcg_para para = clcg_hip_default_parameters();
    para.epsilon = 1e-6; para.abs_diff = 0;         // sample14.cu:254-255
    para.max_iterations = 200;
    bool ok = true;
    for (int loop = 0; loop < 2; loop++) {
        const char *name = loop ? "clcg_hip_lpcg_multi_c64" : "clcg_hip_lbicg_sym_multi_c64";
        Block M(n, k);
        int ret[k], its[k];
        double res[k];
        rc = loop ? clcg_hip_lpcg_multi_c64(A, k, M.raw(), B.raw(), &para, ret, its, res, LCG_HIP_MEM_HOST)
                  : clcg_hip_lbicg_sym_multi_c64(A, k, M.raw(), B.raw(), &para, ret, its, res, LCG_HIP_MEM_HOST);
        if (rc) { std::cerr << name << ": rc=" << rc << " " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
        std::printf("%s\n", name);
        for (int j = 0; j < k; j++) {
            // the same column alone
            std::vector<cf> m(n, cf(0.f, 0.f)), bj(n);
            for (int i = 0; i < n; i++) bj[i] = scale[j] * b[i];
            float *mp = reinterpret_cast<float *>(m.data());
            const float *bp = reinterpret_cast<const float *>(bj.data());
            const int sret = loop ? clcg_hip_solver_preconditioned_c64(clcg_hip_csr_ax_c64, clcg_hip_jacobi_mx_c64, nullptr, mp, bp, n,
                                                                       &para, A, CLCG_PCG, LCG_HIP_MEM_HOST)
                                  : clcg_hip_solver_c64(clcg_hip_csr_ax_c64, nullptr, mp, bp, n, &para, A, CLCG_BICG_SYM, LCG_HIP_MEM_HOST);
            if (sret <= LCG_HIP_E_RUNTIME) { std::cerr << "solver: " << lcg_hip_last_error() << "\n"; lcg_hip_csr_destroy(A); return 3; }
            const int sits = lcg_hip_last_iterations();
            double eb = 0.0, es = 0.0;          // avg_error, sample14.cu:71-81
            for (int i = 0; i < n; i++) {
                const cf want = scale[j] * ans[i];
                eb += std::norm(M.p[(size_t)i * k + j] - want); es += std::norm(m[i] - want);
            }
            std::printf("column %d: batch ret=%d iterations=%d error=%.6e | single ret=%d iterations=%d error=%.6e\n", j, ret[j], its[j],
                        std::sqrt(eb) / n, sret, sits, std::sqrt(es) / n);
            ok = ok && (ret[j] == CLCG_CONVERGENCE || ret[j] == LCG_REACHED_MAX_ITERATIONS);
        }
    }
    lcg_hip_csr_destroy(A);
    return ok ? 0 : 1;
}
