// One-sided Jacobi SVD entry point (jacobi.hip).
#pragma once
#include "ctx.h"
namespace lrn {
static constexpr int JAC_SMALL = 96;
// A (n x n, col-major) is overwritten by U*Sigma; V (n x n) receives the right singular
// vectors, accumulated from the identity (may be null: no accumulation, the rotations of A are the same);
// sigma[n] the singular values (unsorted).  A warm start multiplies A by the previous vectors beforehand (prepw.hip::svd_of_cc).
int jacobi_svd(lrn_ctx* c, double* A, double* V, double* sigma, int n, int* sweeps_out);
}  // namespace lrn
