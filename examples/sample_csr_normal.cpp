// sample_csr_normal.cpp -- the flow of liblcg's sample1.cpp (the normal equations K^T.K m = K^T d through a callback that multiplies
// by K and then by K^T) with a SPARSE kernel: K is 4000 x 500 with 8 entries per row, and the damping sqrt(lambda) I is stacked under
// it as 500 one-entry rows (K^T.K + lambda I = K'^T.K' with K' = [K; sqrt(lambda) I]), 4500 x 500 in all.  b = K'^T d is formed by
// lcg_hip_spmv_t, CG and PCG (the column-square Jacobi) run through the ready-made callbacks lcg_hip_csr_ata_ax and
// lcg_hip_csr_jacobi_normal_mx, and four data vectors are solved by one lcg_hip_csr_normal_lcg_multi.  K^T.K is never formed.
// Plain C++: compile with g++.
//
//   g++ -O2 -std=c++11 -Iinclude examples/sample_csr_normal.cpp -Lliblcg_amd/lib -llcg_hip -ldl
//       -Wl,-rpath,$PWD/liblcg_amd/lib -o sample_csr_normal && ./sample_csr_normal
//
// A limitation this program has to work around: lcg_hip_spmv_t, like lcg_hip_spmv, takes DEVICE vectors, and the library has no entry
// that allocates device memory.  In a program built with hipcc the two vectors come from hipMalloc.  This one stays a single plain-C++
// file like its neighbours, so it borrows the allocator of the HIP runtime that liblcg_hip.so has already loaded (dlsym; -ldl where the
// C library does not carry it).  That is a shift of this example, not an interface: without the HIP headers, form b on the host --
// the solvers and the batched loops below take host vectors.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include <dlfcn.h>

#include "lcg_dropin.hpp"
#include "lcg_hip_staging_csr_normal.h"

// a fixed-seed generator of its own (the reference seeds with time(0)): xorshift64*, uniform in [lo, hi)
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform(double lo, double hi)
{
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    const uint64_t r = rng_state * 0x2545F4914F6CDD1Dull;
    return lo + (hi - lo) * (double)(r >> 11) / 9007199254740992.0;
}

int main()
{
    const int M0 = 4000, N = 500, T = 8, k = 4, M = M0 + N;
    const double lambda = 1e-2;
    // K' in CSR: T distinct columns per data row, then sqrt(lambda) on the diagonal of the stacked rows
    std::vector<int> rowptr(M + 1, 0), col;
    std::vector<double> val;
    for (int i = 0; i < M0; i++) {
        int c[T];
        for (int q = 0; q < T; q++) {
            bool again = true;
            while (again) {
                c[q] = (int)uniform(0.0, (double)N) % N;
                again = false;
                for (int p = 0; p < q; p++) again = again || c[p] == c[q];
            }
            col.push_back(c[q]); val.push_back(uniform(-1.0, 1.0));
        }
        rowptr[i + 1] = (int)col.size();
    }
    for (int j = 0; j < N; j++) { col.push_back(j); val.push_back(std::sqrt(lambda)); rowptr[M0 + j + 1] = (int)col.size(); }
    const int64_t nnz = (int64_t)col.size();

    // k models and their data d = K'.m (the stacked rows' data are sqrt(lambda) m: the damped problem's solution is m itself)
    std::vector<double> fm((size_t)N * k), d((size_t)M * k);
    for (size_t e = 0; e < fm.size(); e++) fm[e] = uniform(1.0, 2.0);
    for (int c = 0; c < k; c++)
        for (int i = 0; i < M; i++) {
            double s = 0.0;
            for (int p = rowptr[i]; p < rowptr[i + 1]; p++) s += val[p] * fm[(size_t)col[p] * k + c];
            d[(size_t)i * k + c] = s;
        }

    lcg_hip_csr_t K = nullptr;
    int rc = lcg_hip_csr_create(&K, M, N, nnz, rowptr.data(), col.data(), val.data(), 0, LCG_HIP_MEM_HOST, 0);
    if (rc) { fprintf(stderr, "lcg_hip_csr_create: %d %s\n", rc, lcg_hip_last_error()); return 3; }
    rc = lcg_hip_csr_build_normal(K);
    if (!rc) rc = lcg_hip_csr_build_jacobi_normal(K, nullptr);
    if (rc) { fprintf(stderr, "the normal state: %d %s\n", rc, lcg_hip_last_error()); return 3; }
    int longest = 0; int64_t extra = 0; double ms = 0.0;
    lcg_hip_csr_normal_info(K, &longest, &extra, &ms);
    printf("K' is %d x %d with %lld entries; K'^T built in %.2f ms, longest column %d, %lld bytes beside the matrix\n", lcg_hip_csr_rows(K),
           lcg_hip_csr_cols(K), (long long)nnz, ms, longest, (long long)extra);

    // b = K'^T d, column by column, on the device (lcg_hip_spmv_t)
    std::vector<double> raw((size_t)2 * N * k + 2);
    double *base = raw.data() + (((uintptr_t)raw.data() & 15) ? 1 : 0);        // (the blocks' bases must be 16-byte aligned)
    double *B = base, *X = base + (size_t)N * k;
    {
        // (the head of this file: in a HIP program these two lines are hipMalloc)
        typedef int (*malloc_fn)(void **, size_t);
        typedef int (*free_fn)(void *);
        malloc_fn dev_malloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
        free_fn dev_free = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
        std::vector<double> dcol(M), bcol(N);
        double *dd = nullptr, *db = nullptr;
        if (!dev_malloc || !dev_free || dev_malloc((void **)&dd, sizeof(double) * M) || dev_malloc((void **)&db, sizeof(double) * N)) {
            fprintf(stderr, "no device memory for the data vector\n"); return 3;
        }
        for (int c = 0; c < k; c++) {
            for (int i = 0; i < M; i++) dcol[i] = d[(size_t)i * k + c];
            rc = lcg_hip_memcpy(dd, dcol.data(), sizeof(double) * M, 1);
            if (!rc) rc = lcg_hip_spmv_t(K, dd, db);
            if (!rc) rc = lcg_hip_synchronize();
            if (!rc) rc = lcg_hip_memcpy(bcol.data(), db, sizeof(double) * N, 2);
            if (rc) { fprintf(stderr, "lcg_hip_spmv_t: %d %s\n", rc, lcg_hip_last_error()); return 3; }
            for (int j = 0; j < N; j++) B[(size_t)j * k + c] = bcol[j];
        }
        dev_free(dd); dev_free(db);
    }

    lcg_para para = lcg_default_parameters();
    para.epsilon = 1e-10; para.abs_diff = 0; para.max_iterations = 2000;
    int bad = 0;

    // CG and PCG on column 0 through the callbacks
    std::vector<double> b(N), m(N), single(N);
    for (int j = 0; j < N; j++) b[j] = B[(size_t)j * k];
    int ret = lcg_solver(lcg_hip_csr_ata_ax, nullptr, m.data(), b.data(), N, &para, K, LCG_CG);
    const int it_cg = lcg_hip_last_iterations();
    if (ret != 0) { fprintf(stderr, "lcg_solver: %d (%s) %s\n", ret, lcg_status_text(ret), lcg_hip_last_error()); bad = 1; }
    single = m;
    for (int j = 0; j < N; j++) m[j] = 0.0;
    ret = lcg_solver_preconditioned(lcg_hip_csr_ata_ax, lcg_hip_csr_jacobi_normal_mx, nullptr, m.data(), b.data(), N, &para, K);
    const int it_pcg = lcg_hip_last_iterations();
    if (ret != 0) { fprintf(stderr, "lcg_solver_preconditioned: %d (%s) %s\n", ret, lcg_status_text(ret), lcg_hip_last_error()); bad = 1; }
    double e_cg = 0.0, e_pcg = 0.0;
    for (int j = 0; j < N; j++) { e_cg = std::fmax(e_cg, std::fabs(single[j] - fm[(size_t)j * k])); e_pcg = std::fmax(e_pcg, std::fabs(m[j] - fm[(size_t)j * k])); }
    printf("CG through lcg_hip_csr_ata_ax: %d iterations, largest error %.3e; PCG with lcg_hip_csr_jacobi_normal_mx: %d iterations, largest error %.3e\n",
           it_cg, e_cg, it_pcg, e_pcg);

    // one batched solve of all four data vectors
    int ret4[4], its4[4];
    double res4[4];
    for (size_t e = 0; e < (size_t)N * k; e++) X[e] = 0.0;
    rc = lcg_hip_csr_normal_lcg_multi(K, k, X, B, &para, ret4, its4, res4, LCG_HIP_MEM_HOST);
    if (rc) { fprintf(stderr, "lcg_hip_csr_normal_lcg_multi: %d %s\n", rc, lcg_hip_last_error()); return 3; }
    double err = 0.0, diff = 0.0;
    for (size_t e = 0; e < (size_t)N * k; e++) err = std::fmax(err, std::fabs(X[e] - fm[e]));
    for (int j = 0; j < N; j++) diff = std::fmax(diff, std::fabs(X[(size_t)j * k] - single[j]));
    printf("one lcg_hip_csr_normal_lcg_multi, iterations:");
    for (int c = 0; c < k; c++) { printf(" %d", its4[c]); if (ret4[c] != 0) bad = 1; }
    printf("\nlargest error of the batch: %.3e; column 0 against the single CG solve: %.3e\n", err, diff);
    if (std::abs(its4[0] - it_cg) > 3 || err > 1e-3 || diff > 1e-6 || e_cg > 1e-3 || e_pcg > 1e-3) bad = 1;
    lcg_hip_csr_destroy(K);
    return bad;
}
