// multi_ops.hpp -- the matrix as the real batched loops see it (solvers_multi.hip: CG, PCG; solvers_multi_box.hip: PG, SPG): a small
// operator argument over a CSR handle, a rectangular CSR handle's K^T.K or a dense handle's K^T.K / K.  Host code only.  Not installed.
#pragma once

#include "multi_loop.hpp"
#include "csr_tri.hpp"
#include "csr_normal.hpp"
#include "dense.hpp"

namespace lcgh {

// rows(), invdiag() (the Jacobi reciprocals), big_doubles(k) (what the product's carried sum needs on its way to the table) and
// apply(): Y = A.X for the K columns and, with U, column j's (A.X)_j . U_j as *slots partial sums in `dots` (multi.hpp's table
// format).  TREE: the passes of solvers_multi.hip add their sums as multi_loop.hpp's binary tree, so that a column's bits do not
// depend on K either.  factor(): a triangular factor as M (null: the built-in Jacobi).
struct CsrOp {
    static constexpr bool TREE = false;      // (the sums these entries have always computed)
    lcg_hip_csr *A;
    const TriFactor *F;
    int rows() const { return A->n_rows; }
    const double *invdiag() const { return A->invdiag; }
    const TriFactor *factor() const { return F; }
    size_t big_doubles(int k) const { return spmm_big_doubles(A->main, k); }
    int apply(Ctx &c, int k, const double *X, double *Y, const int *done, const double *U = nullptr, double *big = nullptr,
              double *dots = nullptr, int *slots = nullptr) const
    {
        c.cnt_ax++;
        return spmm_launch(A->main, k, X, Y, c.stream, done, U, big, dots, slots);
    }
};
// K^T.K of a rectangular CSR handle with its normal state (csr_normal.hip): K.X into the state's M x k block, then K^T over the
// materialised transpose, which carries the sum; two launches, both counted as products, both under the same stop flag.  The columns'
// sums are the product kernel's (an order fixed by K^T alone) and the passes' are trees: a column's bits do not depend on k
struct CsrNormalOp {
    static constexpr bool TREE = true;
    lcg_hip_csr *A;
    int rows() const { return A->n_cols; }
    const double *invdiag() const { return A->normal->invdiag; }
    const TriFactor *factor() const { return nullptr; }
    size_t big_doubles(int k) const { return spmm_big_doubles(A->normal->T, k); }
    int apply(Ctx &c, int k, const double *X, double *Y, const int *done, const double *U = nullptr, double *big = nullptr,
              double *dots = nullptr, int *slots = nullptr) const
    {
        c.cnt_ax += 2;
        TRY(spmm_launch(A->main, k, X, A->normal->tk, c.stream, done));
        return spmm_launch(A->normal->T, k, A->normal->tk, Y, c.stream, done, U, big, dots, slots);
    }
};
// K^T.K or K of a dense handle (dense_multi.hip): the product is two to five launches, all counted as products
struct DenseOp {
    static constexpr bool TREE = true;
    lcg_hip_dense *D;
    int normal;
    int rows() const { return D->N; }
    const double *invdiag() const { return D->invdiag; }
    const TriFactor *factor() const { return nullptr; }
    size_t big_doubles(int) const { return 0; }
    int apply(Ctx &c, int k, const double *X, double *Y, const int *done, const double *U = nullptr, double * = nullptr,
              double *dots = nullptr, int *slots = nullptr) const
    {
        int launches = 0;
        const int rc = dnm_op(D, k, normal, X, Y, c.stream, done, U, dots, slots, &launches);
        c.cnt_ax += launches;
        return rc;
    }
};

} // namespace lcgh
