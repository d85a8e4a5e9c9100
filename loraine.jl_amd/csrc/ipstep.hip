// Device-resident interior-point step: everything of the reference's per-iteration host work
// that touches msz x msz matrices:
//   residual Rd, right-hand sides (makeRHS, corrector my_kron term), find_step with its two
//   extreme-eigenvalue problems per block, the predictor point / RNT, the iterate update and
//   the matrix parts of find_mu / check_convergence.
// Reference: src/predictor_corrector.jl:8-16,186,248-326 ; src/Solvers.jl:480-511 ;
// src/kron_etc.jl.  nvar-/nlin-vectors and scalars stay with the host driver.
//
// The lrn_ip_* entry points at the end drive one static function per step and per route of the NT scaling (eigen-free:
// b.nt_free, prepw.hip::prepare_w_ns; SVD: prepare_w_block).  The n x n helpers are in matops.hip, the Lyapunov solve in
// lyap.hip, eigmin (predictor_corrector.jl:272,285; Solvers.jl:503,505) is a Lanczos iteration on the device (lz.hip).
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/loraine_hip.h"
#include "ops.h"

namespace lrn {

// RNT = -(Mx + Mx') ./ (D_i + D_j)   (predictor_corrector.jl:308-309)
__global__ void rnt_kernel(const double* __restrict__ Mx, const double* __restrict__ D, double* __restrict__ out, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    out[e] = -(Mx[e] + Mx[(long)j + (long)i * n]) / (D[i] + D[j]);
  }
}

// inner = G'RdG + diag(D - sigma_mu/D) - RNT    (predictor_corrector.jl:186)
__global__ void corr_inner_kernel(const double* __restrict__ GRG, const double* __restrict__ D, const double* __restrict__ RNT,
                                  double sigma_mu, double* __restrict__ out, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    double v = GRG[e] - RNT[e];
    if (i == j) v += D[i] - sigma_mu / D[i];
    out[e] = v;
  }
}

// TX = -I - T (+ a Ki + R): L_X^-1 dX L_X^-T in the eigen-free scaling (a = sigma_mu / c, Ki = (K/c)^-1; R may be null)
__global__ void tx_kernel(const double* __restrict__ T, double a, const double* __restrict__ Ki, const double* __restrict__ R,
                          double* __restrict__ out, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    double v = -T[e];
    if ((int)(e % n) == (int)(e / n)) v -= 1.0;
    if (R) v += a * Ki[e] + R[e];
    out[e] = v;
  }
}

int ensure_resident(lrn_ctx* c, LmiBlock& b) {
  size_t mm_ = (size_t)b.msz * b.msz * 8;
  for (DBuf* d : {&b.Cd, &b.Rd, &b.delX, &b.delS, &b.Xn, &b.Sn, &b.RNT, &b.t0, &b.t1, &b.t2})
    if (d->bytes < mm_) LRN_TRY(ensure(c, *d, mm_, true));
  b.resident = true;
  return LRN_OK;
}

// A block as the steps below see it: sizes, the grid of the element-wise kernels and the arrays by name.  Taken after
// ensure_resident; the arrays of the scaling (W .. Qm) are those of the route that ran last and may be null.
struct Blk {
  LmiBlock* b;
  int m;                  // msz
  long mm;                // msz^2
  size_t bytes;           // of one msz x msz array
  unsigned g;             // workgroups of an element-wise pass
  double *X, *S, *Cd, *Rd, *delX, *delS, *Xn, *Sn, *RNT, *t0, *t1, *t2;
  double *G, *Gi, *D, *DDsi, *Si;                           // SVD route (Si: both)
  double *LXf, *LXt, *Zh, *Ki, *Bs, *TX, *Qm;               // eigen-free route
};

static int block_view(lrn_ctx* c, LmiBlock& b, Blk* v) {
  LRN_TRY(ensure_resident(c, b));
  auto p = [](DBuf& d) { return d.as<double>(); };
  const long mm = (long)b.msz * b.msz;
  *v = Blk{&b, b.msz, mm, (size_t)mm * 8, nb(mm),
           p(b.X), p(b.S), p(b.Cd), p(b.Rd), p(b.delX), p(b.delS), p(b.Xn), p(b.Sn), p(b.RNT), p(b.t0), p(b.t1), p(b.t2),
           p(b.G), p(b.Gi), p(b.D), p(b.DDsi), p(b.Si),
           p(b.LXf), p(b.LXt), p(b.Zh), p(b.Ki), p(b.Bs), p(b.TX), p(b.Qm)};
  return LRN_OK;
}

// the view of block il for an entry point that addresses one block
static int block_at(lrn_ctx* c, int il, Blk* v) {
  if (!c || il < 0 || il >= c->nlmi) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  return block_view(c, c->lmi[il], v);
}

// ------------------------------------------------------------------ right-hand sides
// v1 += AA vec(W (Rd + S) W); with aax: aax += AA vec(X) beside it, and W M W only where AA reads it when every constraint
// is sparse (one product instead of two).  Without aax always both products.
static int rhs_pred_block(lrn_ctx* c, const Blk& v, double* aax) {
  LmiBlock& b = *v.b;
  double* v1 = c->v1.as<double>();
  lin3(c->stream, v.t0, v.mm, 1.0, v.Rd, 1.0, v.S);
  if (aax && wmw_pattern_ok(c, b)) {
    LRN_TRY(aa_times(c, b, v.X, aax));
    return aa_times_wmw_pattern(c, b, v.t0, v.t1, v1);
  }
  LRN_TRY(wmw(c, b, v.t0, v.t1, v.t2));
  if (aax) return aa_times2(c, b, v.X, aax, v.t2, v1);
  return aa_times(c, b, v.t2, v1);
}

// The corrector's term v1 += AA vec(G (G'RdG + D - sigma_mu/D - RNT) G')   (predictor_corrector.jl:186), per route.
// Eigen-free: = AA vec(W Rd W + X - sigma_mu Si - G RNT G') with Qm = G RNT G'.  On the pattern: AA vec(W Rd W) where AA
// reads it, AA vec(X - sigma_mu Si - Qm) by itself
static int rhs_corr_eigenfree_pattern(lrn_ctx* c, const Blk& v, double sigma_mu) {
  LRN_TRY(aa_times_wmw_pattern(c, *v.b, v.Rd, v.t1, c->v1.as<double>()));
  lin3(c->stream, v.t0, v.mm, 1.0, v.X, -sigma_mu, v.Si, -1.0, v.Qm);
  return aa_times(c, *v.b, v.t0, c->v1.as<double>());
}

static int rhs_corr_eigenfree_full(lrn_ctx* c, const Blk& v, double sigma_mu) {
  LRN_TRY(wmw(c, *v.b, v.Rd, v.t1, v.t2));
  lin3(c->stream, v.t0, v.mm, 1.0, v.t2, 1.0, v.X, -sigma_mu, v.Si);
  lin3(c->stream, v.t2, v.mm, 1.0, v.t0, -1.0, v.Qm);
  return aa_times(c, *v.b, v.t2, c->v1.as<double>());
}

static int rhs_corr_svd(lrn_ctx* c, const Blk& v, double sigma_mu) {
  hipStream_t st = c->stream;
  // t1 = G' Rd G
  LRN_TRY(gemm_nn(st, v.m, v.G, true, v.Rd, false, v.t0));
  LRN_TRY(gemm_nn(st, v.m, v.t0, false, v.G, false, v.t1));
  hipLaunchKernelGGL(corr_inner_kernel, dim3(v.g), dim3(256), 0, st, v.t1, v.D, v.RNT, sigma_mu, v.t0, v.m);
  // my_kron(G,G,inner) = vec(G inner G')
  LRN_TRY(gemm_nn(st, v.m, v.G, false, v.t0, false, v.t1));
  LRN_TRY(gemm_nn(st, v.m, v.t1, false, v.G, true, v.t2));
  return aa_times(c, *v.b, v.t2, c->v1.as<double>());
}

// ------------------------------------------------------------------ find_step
// delX from delS and the smallest eigenvalues of the two scaled directions (predictor_corrector.jl:253-285), per route.
// t3 = Xn is free here: Xn / Sn are rebuilt by lrn_ip_update after the step lengths.
//
// Eigen-free: everything in the L_X basis (prepw.hip::prepare_w_ns): Bs = L_X' dS L_X, T = Z Bs Z / c,
// TX = L_X^-1 dX L_X^-T = -I - T (+ sigma_mu K^-1 + R), dX = L_X TX L_X'                  (:253-257)
static int find_step_eigenfree(lrn_ctx* c, const Blk& v, int predict, double sigma_mu, double* lamX, double* lamS) {
  hipStream_t st = c->stream;
  const int m = v.m;
  const double ns_c = v.b->ns_c;
  double* t3 = v.Xn;
  LRN_TRY(pgemm_nt(c, st, m, v.LXt, v.delS, v.t0, GEMM_KFROM_M));                      // L_X' upper triangular
  // (both second products are symmetric in exact arithmetic: from msz 1500 on the lower tiles + mirror, half the work;
  // below, the full product and the average of the two triangles)
  LRN_TRY(sym_product(c, st, m, v.t0, v.LXt, v.t1, v.Bs, 1.0, GEMM_KFROM_N));
  LRN_TRY(pgemm_nt(c, st, m, v.Zh, v.Bs, v.t0));
  LRN_TRY(sym_product(c, st, m, v.t0, v.Zh, v.t1, t3, 1.0 / ns_c, 0));
  hipLaunchKernelGGL(tx_kernel, dim3(v.g), dim3(256), 0, st, t3, sigma_mu / ns_c, v.Ki,
                     predict ? (const double*)nullptr : v.RNT, v.TX, m);
  LRN_TRY(pgemm_nt(c, st, m, v.LXf, v.TX, v.t0, GEMM_KTO_M));                          // L_X lower triangular
  LRN_TRY(pgemm_nt_sym(c, st, m, v.t0, v.LXf, v.delX, 1.0, GEMM_KTO_N));
  // the scaled directions of the step-length rule are orthogonally similar to TX and T               (:263-285)
  return eigmin_certified_pair(c, v.TX, t3, m, lamX, lamS);
}

static int find_step_svd(lrn_ctx* c, const Blk& v, int predict, double sigma_mu, double* lamX, double* lamS) {
  hipStream_t st = c->stream;
  const int m = v.m;
  double *t0 = v.t0, *t1 = v.t1, *t2 = v.t2, *t3 = v.Xn;
  // t2 = W delS W                                                (:253)
  LRN_TRY(wmw(c, *v.b, v.delS, t1, t2));
  if (predict) {
    // delX = mat(-X - W delS W)                                  (:255)
    lin3(st, t0, v.mm, -1.0, v.X, -1.0, t2);
  } else {
    // delX = mat(sigma_mu Si - X - W delS W + G RNT G')          (:257)
    lin3(st, t0, v.mm, sigma_mu, v.Si, -1.0, v.X, -1.0, t2);
    LRN_TRY(gemm_nn(st, m, v.G, false, v.RNT, false, t1));
    LRN_TRY(gemm_nn(st, m, t1, false, v.G, true, t2));
    lin3(st, t0, v.mm, 1.0, t0, 1.0, t2);
  }
  sym_half(st, t0, v.delX, m);
  // step lengths: eigmin of DDsi-scaled G' delS G and Gi delX Gi'   (:263-291)
  LRN_TRY(gemm_nn(st, m, v.Gi, false, v.delX, false, t0));
  LRN_TRY(gemm_nn(st, m, t0, false, v.Gi, true, t1));
  scale_sym(st, t1, v.DDsi, t2, m);
  LRN_TRY(gemm_nn(st, m, v.G, true, v.delS, false, t0));
  LRN_TRY(gemm_nn(st, m, t0, false, v.G, false, t1));
  scale_sym(st, t1, v.DDsi, t3, m);
  return eigmin_certified_pair(c, t2, t3, m, lamX, lamS);
}

// the step-length rule from the smallest eigenvalue of a scaled direction   (predictor_corrector.jl:274-291)
static double step_length(double lam, double tau) { return lam > -1e-6 ? 0.99 : std::min(1.0, -tau / lam); }

// ------------------------------------------------------------------ update
// Xn = X + alpha delX, Sn = S + beta delS, *tr_dev = <Xn, Sn>
static int predict_point(lrn_ctx* c, const Blk& v, double alpha, double beta, double* tr_dev) {
  lin3(c->stream, v.Xn, v.mm, 1.0, v.X, alpha, v.delX);
  lin3(c->stream, v.Sn, v.mm, 1.0, v.S, beta, v.delS);
  return dot_dev(c, v.Xn, v.Sn, v.mm, tr_dev);
}

// Qm = G RNT G' without the eigenvectors: N = L_X^-1 dX dS L_X = TX Bs, Yh R + R Yh = -(N Zh + Zh N') / c, Qm = L_X R L_X'.
// *ok = false: the Lyapunov iteration did not converge (K far from well conditioned), Qm is not formed
static int second_order_eigenfree(lrn_ctx* c, const Blk& v, bool* ok) {
  LmiBlock& b = *v.b;
  hipStream_t st = c->stream;
  const int m = v.m;
  tic(c);
  LRN_TRY(pgemm_nt(c, st, m, v.TX, v.Bs, v.t0));                                       // N
  SlabSrc prod;
  LRN_TRY(prod_slabs(c, st, m, v.t0, v.Zh, v.t1, 1.0, 0, &prod));                      // N Zh
  symadd(st, sym_grid(m), prod, m, -1.0 / b.ns_c, v.t2, nullptr, nullptr);
  int steps = 0;
  LRN_TRY(lyap_solve(c, b, v.t2, v.RNT, v.t0, ok, &steps));
  c->counts["lyap_steps"] += steps;
  c->counts["lyap_solves"] += 1;
  if (*ok) {
    LRN_TRY(pgemm_nt(c, st, m, v.LXf, v.RNT, v.t0, GEMM_KTO_M));
    LRN_TRY(pgemm_nt_sym(c, st, m, v.t0, v.LXf, v.Qm, 1.0, GEMM_KTO_N));
  }
  toc(c, "lyap");
  return LRN_OK;
}

// RNT = -(Gi delX delS G + its transpose) ./ (D_i + D_j)     (predictor_corrector.jl:308-309)
static int second_order_svd(lrn_ctx* c, const Blk& v) {
  hipStream_t st = c->stream;
  LRN_TRY(gemm_nn(st, v.m, v.Gi, false, v.delX, false, v.t0));
  LRN_TRY(gemm_nn(st, v.m, v.t0, false, v.delS, false, v.t1));
  LRN_TRY(gemm_nn(st, v.m, v.t1, false, v.G, false, v.t2));
  hipLaunchKernelGGL(rnt_kernel, dim3(v.g), dim3(256), 0, st, v.t2, v.D, v.RNT, v.m);
  return LRN_OK;
}

// the corrector's step: X <- sym(X + alpha delX), S <- sym(S + beta delS)
static void take_step(lrn_ctx* c, const Blk& v, double alpha, double beta) {
  v.b->chol_valid = false;
  lin3(c->stream, v.t0, v.mm, 1.0, v.X, alpha, v.delX);
  sym_half(c->stream, v.t0, v.X, v.m);
  lin3(c->stream, v.t0, v.mm, 1.0, v.S, beta, v.delS);
  sym_half(c->stream, v.t0, v.S, v.m);
}

}  // namespace lrn

using namespace lrn;

extern "C" int lrn_ip_set_c(lrn_ctx* c, int il, const double* C) {
  Blk v;
  LRN_TRY(block_at(c, il, &v));
  if (!C) return LRN_ERR_ARG;
  return copy_in(c, v.Cd, C, v.bytes);
}

extern "C" int lrn_ip_set_iterate(lrn_ctx* c, int il, const double* X, const double* S) {
  Blk v;
  LRN_TRY(block_at(c, il, &v));
  if (!X || !S) return LRN_ERR_ARG;
  LRN_TRY(copy_in(c, v.X, X, v.bytes));
  LRN_TRY(copy_in(c, v.S, S, v.bytes));
  LRN_HIP(c, hipMemsetAsync(v.RNT, 0, v.bytes, c->stream));
  v.b->have_Vprev = false;
  v.b->chol_valid = false;
  return LRN_OK;
}

extern "C" int lrn_ip_get_iterate(lrn_ctx* c, int il, double* X, double* S) {
  Blk v;
  LRN_TRY(block_at(c, il, &v));
  if (X) LRN_TRY(copy_out(c, X, v.X, v.bytes));
  if (S) LRN_TRY(copy_out(c, S, v.S, v.bytes));
  return LRN_OK;
}

extern "C" int lrn_ip_add_diag(lrn_ctx* c, int il, int which, double eps) {
  Blk v;
  LRN_TRY(block_at(c, il, &v));
  if (which != 1 && which != 2) return LRN_ERR_ARG;
  v.b->chol_valid = false;
  add_diag_mat(c->stream, which == 1 ? v.X : v.S, v.m, eps);
  return LRN_OK;
}

extern "C" int lrn_ip_prepare_w(lrn_ctx* c, int il, int* info) {
  Blk v;
  LRN_TRY(block_at(c, il, &v));
  if (!info) return LRN_ERR_ARG;
  LmiBlock& b = *v.b;
  PhaseTimer timer(c, c->profile);
  bool conv = false;
  if (c->opt.nt_mode == 1 && b.msz > 1) LRN_TRY(prepare_w_ns(c, b, info, &conv));
  if (!conv && *info == 0) {
    b.nt_free = false;
    LRN_TRY(prepare_w_block(c, b, info));
  }
  timer.stop("prepare_w");
  return LRN_OK;
}

extern "C" int lrn_ip_aa_x(lrn_ctx* c, double* out) {
  if (!c || !out) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_HIP(c, hipMemsetAsync(c->v1.p, 0, (size_t)n * 8, c->stream));
  for (auto& b : c->lmi) LRN_TRY(aa_times(c, b, b.X.as<double>(), c->v1.as<double>()));
  return copy_out(c, out, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_ip_residual_d(lrn_ctx* c, const double* y) {
  if (!c || !y) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  LRN_TRY(copy_in(c, c->v0.p, y, (size_t)c->nvar * 8));
  tic(c);
  for (auto& b : c->lmi) {
    Blk v;
    LRN_TRY(block_view(c, b, &v));
    LRN_TRY(aat_to_mat(c, b, c->v0.as<double>(), v.t0));
    lin3(c->stream, v.Rd, v.mm, 1.0, v.Cd, -1.0, v.S, -1.0, v.t0);
  }
  toc(c, "residual_d");
  return LRN_OK;
}

extern "C" int lrn_ip_rhs_pred(lrn_ctx* c, double* out) {
  if (!c || !out) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_HIP(c, hipMemsetAsync(c->v1.p, 0, (size_t)n * 8, c->stream));
  for (auto& b : c->lmi) {
    Blk v;
    LRN_TRY(block_view(c, b, &v));
    LRN_TRY(rhs_pred_block(c, v, nullptr));
  }
  return copy_out(c, out, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_ip_rhs_pred2(lrn_ctx* c, double* aax_out, double* out) {
  if (!c || !aax_out || !out) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(ensure(c, c->v2, (size_t)(n + 64) * 8));
  tic(c);
  LRN_HIP(c, hipMemsetAsync(c->v1.p, 0, (size_t)n * 8, c->stream));
  LRN_HIP(c, hipMemsetAsync(c->v2.p, 0, (size_t)n * 8, c->stream));
  for (auto& b : c->lmi) {
    Blk v;
    LRN_TRY(block_view(c, b, &v));
    LRN_TRY(rhs_pred_block(c, v, c->v2.as<double>()));
  }
  toc(c, "rhs");
  LRN_TRY(copy_out(c, aax_out, c->v2.p, (size_t)n * 8));
  return copy_out(c, out, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_ip_rhs_corr(lrn_ctx* c, double sigma_mu, double* out) {
  if (!c || !out) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  tic(c);
  LRN_HIP(c, hipMemsetAsync(c->v1.p, 0, (size_t)n * 8, c->stream));
  for (auto& b : c->lmi) {
    Blk v;
    LRN_TRY(block_view(c, b, &v));
    if (!b.nt_free) LRN_TRY(rhs_corr_svd(c, v, sigma_mu));
    else if (wmw_pattern_ok(c, b)) LRN_TRY(rhs_corr_eigenfree_pattern(c, v, sigma_mu));
    else LRN_TRY(rhs_corr_eigenfree_full(c, v, sigma_mu));
  }
  toc(c, "rhs");
  return copy_out(c, out, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_ip_find_step(lrn_ctx* c, int predict, double sigma_mu, double tau, const double* dely,
                                double* alpha, double* beta) {
  if (!c || !dely || !alpha || !beta) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  LRN_TRY(copy_in(c, c->v0.p, dely, (size_t)c->nvar * 8));
  PhaseTimer timer(c, c->profile);
  for (int il = 0; il < c->nlmi; ++il) {
    LmiBlock& b = c->lmi[il];
    Blk v;
    LRN_TRY(block_view(c, b, &v));
    // delS = Rd - mat(AA' dely)                                   (:252)
    LRN_TRY(aat_to_mat(c, b, c->v0.as<double>(), v.t0));
    lin3(c->stream, v.delS, v.mm, 1.0, v.Rd, -1.0, v.t0);
    double lamX = 0.0, lamS = 0.0;
    if (b.nt_free) LRN_TRY(find_step_eigenfree(c, v, predict, sigma_mu, &lamX, &lamS));
    else LRN_TRY(find_step_svd(c, v, predict, sigma_mu, &lamX, &lamS));
    alpha[il] = step_length(lamX, tau);
    beta[il] = step_length(lamS, tau);
  }
  timer.stop("find_step");
  return LRN_OK;
}

extern "C" int lrn_ip_update(lrn_ctx* c, int predict, const double* alpha, const double* beta, double* trXnSn) {
  if (!c || !alpha || !beta) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  LRN_TRY(ensure(c, c->redout, 64 * 8));
  for (int il = 0; il < c->nlmi; ++il) {
    LmiBlock& b = c->lmi[il];
    Blk v;
    LRN_TRY(block_view(c, b, &v));
    if (!predict) {
      take_step(c, v, alpha[0], beta[0]);
      continue;
    }
    LRN_TRY(predict_point(c, v, alpha[il], beta[il], c->redout.as<double>() + il));
    if (b.nt_free) {
      bool ok = false;
      LRN_TRY(second_order_eigenfree(c, v, &ok));
      if (ok) continue;
      // take the SVD for this iteration
      c->counts["lyap_fallback"] += 1;
      int info = 0;
      LRN_TRY(prepare_w_block(c, b, &info));
      if (info != 0) return set_error(c, LRN_ERR_STATE, "SVD fallback of the NT scaling failed (info %d)", info);
      b.nt_free = false;
      LRN_TRY(block_view(c, b, &v));          // (the arrays of the SVD route are final only now)
    }
    LRN_TRY(second_order_svd(c, v));
  }
  if (predict && trXnSn && c->nlmi > 0) LRN_TRY(copy_out(c, trXnSn, c->redout.p, (size_t)c->nlmi * 8));
  LRN_HIP(c, hipGetLastError());
  return LRN_OK;
}

extern "C" int lrn_ip_stats(lrn_ctx* c, double* out5) {
  if (!c || !out5) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  LRN_TRY(ensure(c, c->redout, (size_t)std::max(64, 5 * c->nlmi) * 8));
  for (int il = 0; il < c->nlmi; ++il) {
    Blk v;
    LRN_TRY(block_view(c, c->lmi[il], &v));
    double* o = c->redout.as<double>() + 5 * il;
    LRN_TRY(dot_dev(c, v.X, v.S, v.mm, o + 0));
    LRN_TRY(dot_dev(c, v.Rd, nullptr, v.mm, o + 3));
    LRN_TRY(dot_dev(c, v.Cd, v.X, v.mm, o + 4));
  }
  LRN_TRY(copy_out(c, out5, c->redout.p, (size_t)5 * c->nlmi * 8));
  for (int il = 0; il < c->nlmi; ++il) {
    LmiBlock& b = c->lmi[il];
    double lx = 0, ls = 0;
    bool have = false;
    if (c->opt.nt_mode == 1 && b.msz > 1) {
      // the callers consume max(0, -eigmin) (Solvers.jl:503-511): a successful Cholesky factorisation IS the certificate
      // that both terms vanish, and the next prepare_W starts with exactly these two factorisations -- they are kept
      // (b.chol_valid).  Reported then: the smallest pivots (positive upper bounds of the smallest eigenvalues).
      int info = 0;
      double piv[2] = {0.0, 0.0};
      LRN_TRY(nt_factor(c, b, &info, piv));
      if (info == 0) { lx = piv[0]; ls = piv[1]; have = true; c->counts["stats_chol"] += 1; }
    }
    if (!have) LRN_TRY(eigmin_certified_pair(c, b.X.as<double>(), b.S.as<double>(), b.msz, &lx, &ls));
    out5[5 * il + 1] = lx;
    out5[5 * il + 2] = ls;
    out5[5 * il + 3] = std::sqrt(out5[5 * il + 3]);
  }
  return LRN_OK;
}
