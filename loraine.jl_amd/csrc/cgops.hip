// The CG recurrence, the low-rank preconditioners and the device-resident PCG.
// Replaces MyM_no / MyM_beta / MyM, Prec_for_CG_beta, Prec_for_CG_tilS_prep, prec_alpha_S! (reference
// src/Solvers.jl:572-904) and cg of ConjugateGradients.jl 0.1 (call sites src/predictor_corrector.jl:134,235).
// This file holds: Prec and symv_rows_kernel, the CG kernels, prec_setup / prec_apply / prec_dense_*, the operator
// selection (op_select, op_apply), pcg_dev and the extern "C" entry points (lrn_matvec, lrn_matvec_partial, lrn_make_rhs,
// lrn_prec_*, lrn_pcg).  The operator itself -- MyA, Ax = AA vec(W mat(AA' x) W) -- and every other pass over the
// constraint data live in dataops.hip.
//
// H_alpha apply uses the algebraically identical "ts" form of the SMW formula:
//   ts = D^-1/2 AA (U (x) Z)   (nvar x k*msz, built once per IP iteration)
//   M^-1 x = D^-1/2 [ v - ts (I + ts' ts)^-1 ts' v ],  v = D^-1/2 x
// i.e. two bandwidth-bound GEMVs and one POTRS on the (k*msz)^2 factor -- this also covers
// erank > 1 without materialising kron(Umat, Z) (Solvers.jl:759 would need msz^2 x k*msz).
#include <algorithm>
#include <cmath>

#include "../../include/loraine_hip.h"
#include "ctx.h"
#include "jacobi.h"
#include "ops.h"
#include "fac_cols.h"

namespace lrn {

struct Prec {
  int kind = 0, erank = 0, ksz = 0;
  double dsum = 0.0;
  DBuf d;        // nvar
  DBuf ts;       // nvar x ksz
  DBuf cholS;
  DBuf workS;    // chol_work_doubles of the factorisations of Z and S + I, then NB x ksz of the solve with cholS
  DBuf y, y2, y3, y4, zpart;
  DBuf E, Um, AU, sig;
  // H_alpha with linear constraints: AAAATtau = tau^2 I + C_lin diag(X_lin ./ S_lin) C_lin' is not
  // diagonal (Solvers.jl:743-745); its dense Cholesky factor L_D replaces the D^-1/2 scalings
  bool has_LD = false;
  DBuf LD, Cd;
  DBuf workD;    // chol_work_doubles(nvar) of the factorisation, then NB x max(ksz, 1) of the solves with L_D
  // SMW core as an explicit inverse (option prec_inv): Sm = S + I, Ainv = (S + I)^-1 = L^-T L^-1
  bool has_inv = false;
  DBuf Sm, Ainv;
  // the whole preconditioner as one dense symmetric matrix (lower triangle), round 4:
  //   M^-1 = D^-1/2 (I - ts (S + I)^-1 ts') D^-1/2
  // -- inside lrn_pcg the seven launches of the SMW apply become one pass over nvar (nvar + 1) / 2 doubles (symv_lower)
  bool has_dense = false;
  DBuf Minv, T1;
  DBuf Tf;       // ts from the rank-k factors: T = Vd' Um, (nvar khat) x erank
};

// y = alpha M x + beta z for a symmetric n x n matrix, 16 rows per workgroup, x staged in LDS (n <= 8192): one launch
// (the solves through cholS are eight launches of 15-20 us at ksz = 801)
__global__ __launch_bounds__(256) void symv_rows_kernel(const double* __restrict__ M, int n, const double* __restrict__ x,
                                                        const double* __restrict__ z, double alpha, double beta,
                                                        double* __restrict__ y) {
  extern __shared__ double xs_[];
  __shared__ double sh_[16 * 16];
  const int t = threadIdx.x;
  for (int i = t; i < n; i += 256) xs_[i] = x[i];
  __syncthreads();
  const int r = t & 15, g = t >> 4;
  const int i = blockIdx.x * 16 + r;
  double acc = 0.0;
  if (i < n) {
    const double* mrow = M + i;
#pragma unroll 4
    for (int col = g; col < n; col += 16) acc += mrow[(size_t)col * n] * xs_[col];
  }
  sh_[g * 16 + r] = acc;
  __syncthreads();
  if (t < 16) {
    double v = 0.0;
#pragma unroll
    for (int gg = 0; gg < 16; ++gg) v += sh_[gg * 16 + t];
    const int ii = blockIdx.x * 16 + t;
    if (ii < n) y[ii] = alpha * v + (z ? beta * z[ii] : 0.0);
  }
}

void prec_free(lrn_ctx* c) {
  if (!c->prec) return;
  Prec* p = c->prec;
  for (DBuf* d : {&p->d, &p->ts, &p->cholS, &p->workS, &p->y, &p->y2, &p->y3, &p->y4, &p->zpart, &p->E, &p->Um,
                  &p->AU, &p->sig, &p->LD, &p->workD, &p->Cd, &p->Sm, &p->Ainv, &p->Minv, &p->T1, &p->Tf})
    release(*d);
  delete p;
  c->prec = nullptr;
}

// ------------------------------------------------------------------ vector kernels (single workgroup)
__device__ __forceinline__ double wg_sum1024(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < 16; ++i) s += sh[i];
  return s;
}

// scal: [0]=gamma [1]=pAp [2]=alpha [3]=rr [4]=flag(alpha invalid) [5]=beta [6]=||b|| [7]=zr
__global__ __launch_bounds__(1024) void cg_norm_kernel(const double* __restrict__ b, int n, double* __restrict__ scal, int slot) {
  __shared__ double sh[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) s += b[i] * b[i];
  s = wg_sum1024(s, sh);
  if (threadIdx.x == 0) scal[slot] = s;
}

// ---- the CG recurrence as two multi-workgroup launches per iteration (round 4; round 3: two single-workgroup kernels of
// 33 + 15 us at nvar 20 000 and a host read between them).
//   cg_b_kernel(it): q = p'Ap (from the partial sums the operator left, or a redundant dot per workgroup), alpha = g / q,
//                    x += alpha p, r -= alpha Ap on the workgroup's slice, z = M^-1 r inline when the preconditioner is
//                    diagonal (none, H_beta), partial sums of r'r and z'r
//   cg_d_kernel(it): r'r -> the convergence test of ConjugateGradients.jl (relative residual <= tol); z'r, beta,
//                    p = z + beta p on the slice
// Every workgroup forms the global scalars itself from the same partials in the same order: no grid barrier, no atomics,
// all workgroups take the same branch.  scal[8] = exit code once the iteration has ended (30 converged, -13 alpha
// invalid), scal[9] = the iteration it ended in, both mirrored to host-mapped words: the host queues iterations ahead of
// the test it has read (option pcg_lookahead); kernels queued beyond the last iteration find the flag set and leave
// x, r, p alone -- count and result are those of the loop that tests after every step.  g = r'z alternates between
// scal[10] and scal[11] (a workgroup of cg_d_kernel must not overwrite the value its neighbours are still reading).
__device__ __forceinline__ double wg_sum256(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

static constexpr int CG_MAXWG = 256;

__global__ __launch_bounds__(256) void cg_b_kernel(const double* __restrict__ p, const double* __restrict__ Ap,
                                                   double* __restrict__ r, double* __restrict__ x, double* __restrict__ z,
                                                   int kind, const double* __restrict__ d, int n, int per,
                                                   double* __restrict__ scal, const double* __restrict__ qpart, int nq,
                                                   double* __restrict__ rrpart, double* __restrict__ zrpart,
                                                   double* __restrict__ hostw, int it) {
  __shared__ double sh[4];
  if (scal[8] != 0.0) return;
  double q = 0.0;
  if (qpart) for (int i = threadIdx.x; i < nq; i += 256) q += qpart[i];
  else for (int i = threadIdx.x; i < n; i += 256) q += p[i] * Ap[i];
  q = wg_sum256(q, sh);
  const double g = scal[10 + ((it - 1) & 1)];
  const double alpha = g / q;
  const bool bad = !(alpha >= 0.0) || isinf(alpha);
  if (blockIdx.x == 0 && threadIdx.x == 0) { scal[1] = q; scal[2] = alpha; scal[4] = bad ? 1.0 : 0.0; }
  if (bad) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      scal[9] = (double)it;
      hostw[1] = (double)it;
      hostw[0] = -13.0;
      __threadfence_system();
      scal[8] = -13.0;
    }
    return;
  }
  const int i0 = blockIdx.x * per, i1 = min(n, i0 + per);
  double rr = 0.0, zr = 0.0;
  for (int i = i0 + threadIdx.x; i < i1; i += 256) {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * Ap[i];
    r[i] = ri;
    rr += ri * ri;
    if (kind == 0) { z[i] = ri; zr += ri * ri; }                       // MyM_no   (Solvers.jl:620-622)
    else if (kind == 2) { const double zi = ri / d[i]; z[i] = zi; zr += zi * ri; }   // MyM_beta (:670-672)
  }
  rr = wg_sum256(rr, sh);
  zr = wg_sum256(zr, sh);
  if (threadIdx.x == 0) { rrpart[blockIdx.x] = rr; zrpart[blockIdx.x] = zr; }
}

// first != 0: the start of the iteration, p = z, g = z'r (no test, no beta)
__global__ __launch_bounds__(256) void cg_d_kernel(const double* __restrict__ z, const double* __restrict__ r,
                                                   double* __restrict__ p, int n, int per, int nwg,
                                                   double* __restrict__ scal, const double* __restrict__ rrpart,
                                                   const double* __restrict__ zrpart, double* __restrict__ hostw, int it,
                                                   double res0, double tol, int first) {
  __shared__ double sh[4];
  if (scal[8] != 0.0) return;
  if (!first) {
    double rr = 0.0;
    for (int i = threadIdx.x; i < nwg; i += 256) rr += rrpart[i];
    rr = wg_sum256(rr, sh);
    if (sqrt(rr) / res0 <= tol) {
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        scal[3] = rr;
        scal[9] = (double)it;
        hostw[1] = (double)it;
        hostw[0] = 30.0;
        __threadfence_system();
        scal[8] = 30.0;
      }
      return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[3] = rr;
  }
  double zr = 0.0;
  if (zrpart) for (int i = threadIdx.x; i < nwg; i += 256) zr += zrpart[i];
  else for (int i = threadIdx.x; i < n; i += 256) zr += z[i] * r[i];
  zr = wg_sum256(zr, sh);
  const double beta = first ? 0.0 : zr / scal[10 + ((it - 1) & 1)];
  const int i0 = blockIdx.x * per, i1 = min(n, i0 + per);
  if (first) for (int i = i0 + threadIdx.x; i < i1; i += 256) p[i] = z[i];
  else for (int i = i0 + threadIdx.x; i < i1; i += 256) p[i] = z[i] + beta * p[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) { scal[10 + (it & 1)] = zr; scal[5] = beta; scal[7] = zr; }
}

__global__ void div_kernel(const double* __restrict__ x, const double* __restrict__ d, double* __restrict__ y, int n, int sq) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = x[i] / (sq ? sqrt(d[i]) : d[i]);
}

__global__ void fill_kernel(double* __restrict__ d, int n, double v) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = v;
}

// y[c] = sum_i ts[i + c*n] v[i]   (one workgroup per column); d != null: v[i] = x[i] / sqrt(d[i]) formed on the fly
__global__ __launch_bounds__(256) void gemv_t_kernel(const double* __restrict__ ts, int n, const double* __restrict__ v,
                                                     const double* __restrict__ d, double* __restrict__ y) {
  __shared__ double sh[4];
  const double* col = ts + (long)blockIdx.x * n;
  double s = 0.0;
  if (d) for (int i = threadIdx.x; i < n; i += 256) s += col[i] * (v[i] / sqrt(d[i]));
  else
  for (int i = threadIdx.x; i < n; i += 256) s += col[i] * v[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) y[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// zpart[chunk][i] = sum_{c in chunk} ts[i + c*n] y[c]
__global__ __launch_bounds__(256) void gemv_n_part_kernel(const double* __restrict__ ts, int n, int ncol, int cper,
                                                          const double* __restrict__ y, double* __restrict__ zpart) {
  int i = blockIdx.x * 256 + threadIdx.x;
  int c0 = blockIdx.y * cper, c1 = min(ncol, c0 + cper);
  if (i >= n) return;
  double s = 0.0;
  for (int cc = c0; cc < c1; ++cc) s += ts[(long)i + (long)cc * n] * y[cc];
  zpart[(long)blockIdx.y * n + i] = s;
}

// out = (v - sum_chunks zpart) / sqrt(d); scaled != 0: v = x / sqrt(d) formed on the fly from x
__global__ void smw_final_kernel(const double* __restrict__ v, const double* __restrict__ zpart, int nchunk, int n,
                                 const double* __restrict__ d, double* __restrict__ out, int scaled) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int k = 0; k < nchunk; ++k) s += zpart[(long)k * n + i];
  const double sd = sqrt(d[i]);
  out[i] = ((scaled ? v[i] / sd : v[i]) - s) / sd;
}

// ------------------------------------------------------------------ H_alpha setup kernels
// Um[:,a] = E[:,idx[a]] * coef[a]
__global__ void umat_kernel(const double* __restrict__ E, int m, const int* __restrict__ idx,
                            const double* __restrict__ coef, int k, double* __restrict__ Um) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m * k) return;
  int i = e % m, a = e / m;
  Um[e] = E[(long)i + (long)idx[a] * m] * coef[a];
}

// Zf = 2 W - Um Um'
__global__ void zfull_kernel(const double* __restrict__ W, const double* __restrict__ Um, int m, int k,
                             double* __restrict__ Zf) {
  long total = (long)m * m;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % m), j = (int)(e / m);
    double s = 0.0;
    for (int a = 0; a < k; ++a) s += Um[i + a * m] * Um[j + a * m];
    Zf[e] = 2.0 * W[e] - s;
  }
}

__global__ void tril2_kernel(double* __restrict__ A, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
    if ((int)(e % n) < (int)(e / n)) A[e] = 0.0;
}

// AU[j, r] += -a_e * Um[c, a] / sqrt(d_j), j = sigma[p]   (one thread per sparse position).  compact (the stored rows of a
// hybrid factored block): AU has ld rows and row p holds position p, scaled by its own d_j all the same
__global__ void au_sparse_kernel(const long* __restrict__ ptr, const int* __restrict__ er, const int* __restrict__ ec,
                                 const double* __restrict__ ev, int p_lo, int p_end, const int* __restrict__ sigma,
                                 const double* __restrict__ Ucol, const double* __restrict__ d, int ld,
                                 double* __restrict__ AU, int compact) {
  int p = p_lo + blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= p_end) return;
  int j = sigma[p];
  double sc = -1.0 / sqrt(d[j]);
  const long row = compact ? p : j;
  for (long e = ptr[p]; e < ptr[p + 1]; ++e) AU[row + (long)er[e] * ld] += sc * ev[e] * Ucol[ec[e]];
}

// dense slot p: AU[sigma[p], r] = -(A_p u)[r] / sqrt(d)   (compact: row p, as above)
__global__ __launch_bounds__(256) void au_dense_kernel(const double* __restrict__ Ad, int m, const int* __restrict__ sigma,
                                                       const double* __restrict__ Ucol, const double* __restrict__ d,
                                                       int ld, double* __restrict__ AU, int compact) {
  const double* A = Ad + (long)blockIdx.x * m * m;
  int j = sigma[blockIdx.x];
  double sc = -1.0 / sqrt(d[j]);
  const long row = compact ? blockIdx.x : j;
  for (int r = threadIdx.x; r < m; r += 256) {
    double s = 0.0;
    for (int cidx = 0; cidx < m; ++cidx) s += A[(long)r + (long)cidx * m] * Ucol[cidx];
    AU[row + (long)r * ld] = sc * s;
  }
}

// ts[sigma[p], col] = C[p, col] for the np stored positions of a hybrid factored block: the rows fac_ts_kernel (facops.hip) left at zero
// (weight-0 factor columns) get their values from the entries, each element written once
__global__ void ts_store_rows_kernel(const double* __restrict__ C, int np, int m, const int* __restrict__ sigma, int nvar,
                                     double* __restrict__ ts) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)np * m) return;
  const int p = (int)(e % np), r = (int)(e / np);
  ts[(long)sigma[p] + (long)r * nvar] = C[e];
}

// Cd[i, l] = C_lin[i, l] * sqrt(xs_l)   (dense nvar x nlin image of the linear block)
__global__ void lin_dense_kernel(const long* __restrict__ ptr, const int* __restrict__ row, const double* __restrict__ val,
                                 const double* __restrict__ xs, int nlin, int n, double* __restrict__ Cd) {
  int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nlin) return;
  double s = sqrt(xs[l]);
  for (long k = ptr[l]; k < ptr[l + 1]; ++k) Cd[(long)row[k] + (long)l * n] += val[k] * s;
}

__global__ void prec_add_diag_kernel(double* __restrict__ S, int n, double v) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) S[(long)i * n + i] += v;
}

__global__ void add_eye_kernel(double* __restrict__ S, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) S[(long)i * n + i] += 1.0;
}


static double tau_of(const std::vector<double>& lam_s, int aamat) {
  // Solvers.jl:646-650 / :715-719
  double mn = lam_s[0], mean = 0.0;
  for (double v : lam_s) { mn = std::min(mn, v); mean += v; }
  mean /= (double)lam_s.size();
  if (aamat == 0) return 1.0 * mn;
  return (mn + mean) / 2.0 - 1.0e-14;
}

int prec_setup(lrn_ctx* c, int kind, int erank, int aamat, int* info) {
  if (info) *info = 0;
  if (!c->prec) c->prec = new Prec();
  Prec* P = c->prec;
  P->kind = kind;
  P->erank = erank;
  P->has_dense = false;
  c->counts["prec_ts_factored"] = 0;
  c->counts["prec_ts_stored_rows"] = 0;
  c->counts["prec_ts_diag_rows"] = 0;
  c->counts["prec_ts_ragged"] = 0;
  const int n = c->nvar;
  hipStream_t st = c->stream;
  if (kind == 0) return LRN_OK;
  if (kind != 1 && kind != 2) return set_error(c, LRN_ERR_ARG, "preconditioner %d not supported", kind);
  if (c->nlmi < 1) return set_error(c, LRN_ERR_STATE, "preconditioner needs at least one LMI block");
  P->has_LD = kind == 1 && c->nlin > 0;
  hipEvent_t a0, a1;
  if (c->profile) { (void)hipEventCreate(&a0); (void)hipEventCreate(&a1); (void)hipEventRecord(a0, st); }
  int ksz = 0;
  for (auto& b : c->lmi) ksz += erank * b.msz;
  P->ksz = ksz;
  LRN_TRY(ensure(c, P->d, (size_t)n * 8));
  double dsum = 0.0;
  struct BlkEig { std::vector<int> idx; std::vector<double> coef; double tau; bool lanczos = false; double trace = 0.0; };
  std::vector<BlkEig> be(c->nlmi);
  for (int il = 0; il < c->nlmi; ++il) {
    LmiBlock& b = c->lmi[il];
    const int m = b.msz, k = erank;
    if (!b.have_G && !b.have_W) return set_error(c, LRN_ERR_STATE, "preconditioner setup needs G or W (lrn_prepare_w)");
    const bool fromW = !b.have_G;     // eigen-free scaling: eig(W) from W itself (its singular values ARE its eigenvalues)
    if (k >= m) return set_error(c, LRN_ERR_ARG, "erank >= matrix size");
    size_t mm = (size_t)m * m * 8;
    LRN_TRY(ensure(c, P->E, mm));
    LRN_TRY(ensure(c, P->sig, (size_t)m * 8));
    const bool use_lz = c->opt.prec_eig == 2 || (c->opt.prec_eig == 0 && m >= 256);
    be[il].lanczos = use_lz;
    be[il].idx.resize(k);
    be[il].coef.resize(k);
    if (use_lz) {
      // the setup only consumes the k largest eigenpairs, lambda_min and the mean of the rest
      // (lanczos.hip): O(steps * msz^2) instead of a full eigendecomposition
      std::vector<double> lam_top(std::max(1, k));
      double lam_min = 0.0, tr = 0.0;
      int steps = 0;
      LRN_TRY(lanczos_extremes(c, b.W.as<double>(), m, k, lam_top.data(), kind == 1 ? P->E.as<double>() : nullptr,
                               &lam_min, &tr, &steps));
      c->counts["prec_lanczos_steps"] = steps;
      double top = 0.0;
      for (int a = 0; a < k; ++a) top += lam_top[a];
      const double mean = (tr - top) / (double)(m - k);
      const double tau = aamat == 0 ? lam_min : (lam_min + mean) / 2.0 - 1.0e-14;     // Solvers.jl:646-650
      be[il].tau = tau;
      be[il].trace = tr;
      if (aamat < 3) dsum += tau * tau;
      for (int a = 0; a < k; ++a) {
        be[il].idx[a] = a;                                                  // Ritz vectors are unit columns 0..k-1
        be[il].coef[a] = std::sqrt(std::max(lam_top[a] - tau, 0.0));
      }
    } else {
      LRN_HIP(c, hipMemcpyAsync(P->E.p, fromW ? b.W.p : b.G.p, mm, hipMemcpyDeviceToDevice, st));
      int sweeps = 0;
      // eig(W) = svd(G)^2 : columns of E become sigma_j u_j   (Solvers.jl:642,706)
      LRN_TRY(jacobi_svd(c, P->E.as<double>(), nullptr, P->sig.as<double>(), m, &sweeps));
      std::vector<double> sg(m);
      LRN_TRY(copy_out(c, sg.data(), P->sig.p, (size_t)m * 8));
      std::vector<int> ord(m);
      for (int i = 0; i < m; ++i) ord[i] = i;
      std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return sg[x] < sg[y]; });   // ascending
      auto lam_of = [&](int i) { return fromW ? sg[i] : sg[i] * sg[i]; };
      std::vector<double> lam_s(m - k);
      for (int i = 0; i < m - k; ++i) lam_s[i] = lam_of(ord[i]);
      double tau = tau_of(lam_s, aamat);
      be[il].tau = tau;
      for (int i = 0; i < m; ++i) be[il].trace += lam_of(i);
      if (aamat < 3) dsum += tau * tau;
      for (int a = 0; a < k; ++a) {
        int id = ord[m - k + a];
        double lam = lam_of(id);
        be[il].idx[a] = id;
        be[il].coef[a] = std::sqrt(std::max(lam - tau, 0.0)) / sg[id];   // Umat = v_l sqrt(lambda_l - tau)
      }
    }
    if (kind == 2) continue;
  }
  P->dsum = dsum;
  hipLaunchKernelGGL(fill_kernel, dim3(nb(n)), dim3(256), 0, st, P->d.as<double>(), n, P->has_LD ? 1.0 : dsum);
  if (P->has_LD) {
    // L_D L_D' = dsum I + (C_lin sqrt(xs)) (C_lin sqrt(xs))'
    const int nl = c->nlin;
    LRN_TRY(ensure(c, P->Cd, (size_t)n * nl * 8));
    LRN_TRY(ensure(c, P->LD, (size_t)n * n * 8));
    LRN_TRY(ensure(c, P->workD, (chol_work_doubles(n) + (size_t)CHOL_NB * std::max(ksz, 1)) * 8));
    LRN_HIP(c, hipMemsetAsync(P->Cd.p, 0, (size_t)n * nl * 8, st));
    hipLaunchKernelGGL(lin_dense_kernel, dim3(nb(nl)), dim3(256), 0, st, c->cl_ptr.as<long>(), c->cl_rown.as<int>(),
                       c->cl_val.as<double>(), c->lin_xs.as<double>(), nl, n, P->Cd.as<double>());
    GemmDesc gd;
    gd.A = P->Cd.as<double>(); gd.sAm = 1; gd.sAk = n;
    gd.B = P->Cd.as<double>(); gd.sBk = n; gd.sBn = 1;
    gd.C = P->LD.as<double>(); gd.sCm = 1; gd.sCn = n;
    gd.M = gd.N = n; gd.K = nl;
    gd.flags = GEMM_TRI_LOWER;
    LRN_TRY(gemm(st, gd));
    hipLaunchKernelGGL(prec_add_diag_kernel, dim3(nb(n)), dim3(256), 0, st, P->LD.as<double>(), n, dsum);
    LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 4, st));
    LRN_TRY(potrf_lower(st, P->LD.as<double>(), n, n, P->workD.as<double>(), c->info_dev.as<int>()));
    int hd = 0;
    LRN_TRY(copy_out(c, &hd, c->info_dev.p, 4));
    if (hd != 0) { if (info) *info = hd; return LRN_OK; }
  } else if (c->nlin > 0)
    lin_diag(c, P->d.as<double>());
  if (kind == 1) {
    LRN_TRY(ensure(c, P->ts, (size_t)n * ksz * 8));
    int col0 = 0;
    long ts_factored = 0;      // blocks whose part of ts came from the factors ("prec_ts_factored", of the LAST setup)
    long ts_stored = 0;        // rows of ts filled from the stored entries of hybrid blocks ("prec_ts_stored_rows", ditto)
    long ts_diag_rows = 0;     // rows of ts that got the term of their diagonal part ("prec_ts_diag_rows", ditto; option "cg_diag")
    long ts_ragged = 0;        // blocks among ts_factored whose part came from the compacted columns ("prec_ts_ragged", ditto; option "ragged_ts")
    for (int il = 0; il < c->nlmi; ++il) {
      LmiBlock& b = c->lmi[il];
      const int m = b.msz, k = erank;
      size_t mm = (size_t)m * m * 8;
      // eigenvectors again (E was overwritten by later blocks only when nlmi > 1)
      if (c->nlmi > 1) {
        if (be[il].lanczos) {
          std::vector<double> lt(std::max(1, k));
          double lmn, trc;
          LRN_TRY(lanczos_extremes(c, b.W.as<double>(), m, k, lt.data(), P->E.as<double>(), &lmn, &trc, nullptr));
        } else {
          LRN_HIP(c, hipMemcpyAsync(P->E.p, b.have_G ? b.G.p : b.W.p, mm, hipMemcpyDeviceToDevice, st));
          int sw = 0;
          LRN_TRY(jacobi_svd(c, P->E.as<double>(), nullptr, P->sig.as<double>(), m, &sw));
        }
      }
      LRN_TRY(ensure(c, P->Um, (size_t)m * k * 8 + (size_t)k * 16));
      double* Um = P->Um.as<double>();
      double* coef_d = Um + (size_t)m * k;
      int* idx_d = reinterpret_cast<int*>(coef_d + k);
      LRN_TRY(copy_in(c, coef_d, be[il].coef.data(), (size_t)k * 8));
      LRN_TRY(copy_in(c, idx_d, be[il].idx.data(), (size_t)k * 4));
      hipLaunchKernelGGL(umat_kernel, dim3(nb((long)m * k)), dim3(256), 0, st, P->E.as<double>(), m, idx_d, coef_d, k, Um);
      // Z = chol(2 W0 + Um Um') = chol(2W - Um Um')   (Solvers.jl:725-731)
      LRN_TRY(ensure_m(c, m));
      double* Zf = c->m0.as<double>();
      LRN_TRY(ensure(c, P->workS, chol_work_doubles(std::max(m, ksz)) * 8));
      // 2W - UU' is positive definite in exact arithmetic; late in the solve cond(W) passes 1e16 and
      // the rounding of W = GG' can cost the factorisation (the reference's eigen-based W0 is exposed to
      // the same, Solvers.jl:725-731 raise PosDefException).  A preconditioner only has to be SPD:
      // retry with a relative diagonal shift instead of giving up.
      int h = 0;
      for (int attempt = 0; attempt < 4; ++attempt) {
        hipLaunchKernelGGL(zfull_kernel, dim3(nb((long)m * m)), dim3(256), 0, st, b.W.as<double>(), Um, m, k, Zf);
        if (attempt > 0) {
          const double shift = be[il].trace / m * 1e-15 * std::pow(100.0, attempt);
          hipLaunchKernelGGL(prec_add_diag_kernel, dim3(nb(m)), dim3(256), 0, st, Zf, m, shift);
          c->counts["prec_z_shift"] += 1;
        }
        LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 4, st));
        LRN_TRY(potrf_lower(st, Zf, m, m, P->workS.as<double>(), c->info_dev.as<int>()));
        LRN_TRY(copy_out(c, &h, c->info_dev.p, 4));
        if (h == 0) break;
      }
      if (h != 0) { if (info) *info = h; return LRN_OK; }
      hipLaunchKernelGGL(tril2_kernel, dim3(nb((long)m * m)), dim3(256), 0, st, Zf, m);
      // a factored block (option "cg_factored") has no choice to make: there are no entries to take ts from
      if (b.factored || cg_lowrank_ts(c, b, k)) {
        // from the rank-k factors: P = L' V and T = V' Um, then fac_ts of facops.hip (the whole nvar x k m block, every element
        // once).  V = Vd, or under option "ragged_ts" the Rc compacted columns Vc of a block of mixed ranks; a uniform block keeps
        // the padded columns, bit for bit
        const bool rts = ragged_ts_on(c, b);
        if (c->opt.ragged_ts && !rts) c->counts["ragged_ts_fallback"] += 1;
        if (rts) LRN_TRY(ragged_setup(c, b));
        else LRN_TRY(lowrank_dense_factors(c, b));
        const FacCols v = fac_cols(c, b, rts);
        const long R = v.R;
        LRN_TRY(ensure(c, c->BG, (size_t)m * R * 8));
        LRN_TRY(ensure(c, P->Tf, (size_t)R * k * 8));
        if (c->opt.profile_ops) tic(c);      // (measurement, tools/cg_diag_times.py: this product beside the diagonal-row kernel)
        LRN_TRY(cols_product(c, Zf, true, v.V, R, m, c->BG.as<double>()));      // P = L' V, m x R (the upper triangle of Zf is zero: tril2_kernel)
        if (c->opt.profile_ops) toc(c, "prec_ts_p");
        GemmDesc gt;     // T = V' Um, R x k
        gt.A = v.V; gt.sAm = m; gt.sAk = 1;
        gt.B = Um; gt.sBk = 1; gt.sBn = m;
        gt.C = P->Tf.as<double>(); gt.sCm = 1; gt.sCn = R;
        gt.M = (int)R; gt.N = k; gt.K = m;
        LRN_TRY(gemm(st, gt));
        LRN_TRY(fac_ts(c, b, v, c->BG.as<double>(), P->Tf.as<double>(), P->d.as<double>(), k, P->ts.as<double>() + (size_t)col0 * n));
        if (rts) ++ts_ragged;
        ++ts_factored;
        if (b.hybrid()) {
          // the stored constraints have weight-0 columns: their rows came out as zeros.  (D^-1/2 A_s u_a)' Z for these npos_nz
          // rows alone, on a compact npos_nz x msz buffer -- nothing here has nvar rows -- then each row to its natural place
          const int np = b.npos_nz;
          LRN_TRY(ensure(c, P->AU, (size_t)2 * np * m * 8));
          double* AUc = P->AU.as<double>();
          double* Cc = AUc + (size_t)np * m;
          for (int a = 0; a < k; ++a) {
            LRN_HIP(c, hipMemsetAsync(AUc, 0, (size_t)np * m * 8, st));
            const double* Ucol = Um + (size_t)a * m;
            if (b.npos_nz > b.nd)
              hipLaunchKernelGGL(au_sparse_kernel, dim3(nb(b.npos_nz - b.nd)), dim3(256), 0, st, b.ent_ptr.as<long>(),
                                 b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(), b.nd, b.npos_nz,
                                 b.sigma_d.as<int>(), Ucol, P->d.as<double>(), np, AUc, 1);
            if (b.nd > 0)
              hipLaunchKernelGGL(au_dense_kernel, dim3(b.nd), dim3(256), 0, st, b.Adense.as<double>(), m, b.sigma_d.as<int>(),
                                 Ucol, P->d.as<double>(), np, AUc, 1);
            GemmDesc g;
            g.A = AUc; g.sAm = 1; g.sAk = np;
            g.B = Zf; g.sBk = 1; g.sBn = m;
            g.C = Cc; g.sCm = 1; g.sCn = np;
            g.M = np; g.N = m; g.K = m;
            LRN_TRY(gemm(st, g));
            hipLaunchKernelGGL(ts_store_rows_kernel, dim3(nb((long)np * m)), dim3(256), 0, st, Cc, np, m, b.sigma_d.as<int>(), n,
                               P->ts.as<double>() + (size_t)(col0 + a * m) * n);
          }
          ts_stored += np;
        }
        if (b.factored && b.dg_n > 0) {
          // diagonal parts (option "cg_diag": lrn_prec_setup refused the block without it): -(L' diag(a_s) u_a)' / sqrt(d_j) added
          // to the rows fac_ts_kernel wrote the factor part of -- no stored row among them
          if (c->opt.profile_ops) tic(c);
          LRN_TRY(ts_diag(c, b, Zf, Um, k, P->d.as<double>(), P->ts.as<double>() + (size_t)col0 * n));
          if (c->opt.profile_ops) toc(c, "prec_ts_diag");
          ts_diag_rows += b.dg_n;
        }
        col0 += k * m;
        continue;
      }
      // ts[:, block a] = (D^-1/2 AU_a) Z
      LRN_TRY(ensure(c, P->AU, (size_t)n * m * 8));
      for (int a = 0; a < k; ++a) {
        LRN_HIP(c, hipMemsetAsync(P->AU.p, 0, (size_t)n * m * 8, st));
        const double* Ucol = Um + (size_t)a * m;
        if (b.npos_nz > b.nd)
          hipLaunchKernelGGL(au_sparse_kernel, dim3(nb(b.npos_nz - b.nd)), dim3(256), 0, st, b.ent_ptr.as<long>(),
                             b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(), b.nd, b.npos_nz,
                             b.sigma_d.as<int>(), Ucol, P->d.as<double>(), n, P->AU.as<double>(), 0);
        if (b.nd > 0)
          hipLaunchKernelGGL(au_dense_kernel, dim3(b.nd), dim3(256), 0, st, b.Adense.as<double>(), m, b.sigma_d.as<int>(),
                             Ucol, P->d.as<double>(), n, P->AU.as<double>(), 0);
        GemmDesc g;
        g.A = P->AU.as<double>(); g.sAm = 1; g.sAk = n;
        g.B = Zf; g.sBk = 1; g.sBn = m;
        g.C = P->ts.as<double>() + (size_t)(col0 + a * m) * n; g.sCm = 1; g.sCn = n;
        g.M = n; g.N = m; g.K = m;
        LRN_TRY(gemm(st, g));
      }
      col0 += k * m;
    }
    c->counts["prec_ts_factored"] = ts_factored;
    c->counts["prec_ts_stored_rows"] = ts_stored;
    c->counts["prec_ts_diag_rows"] = ts_diag_rows;
    c->counts["prec_ts_ragged"] = ts_ragged;
    if (P->has_LD)      // ts = L_D^-1 t   (the reference: AAAATtau \ t, Solvers.jl:767)
      LRN_TRY(trsm_left_lower(st, P->LD.as<double>(), n, n, false, P->ts.as<double>(), ksz, n,
                              P->workD.as<double>() + chol_work_doubles(n)));
    // S = ts' ts + I ; cholS   (Solvers.jl:804-805)
    LRN_TRY(ensure(c, P->cholS, (size_t)ksz * ksz * 8));
    GemmDesc g;
    g.A = P->ts.as<double>(); g.sAm = n; g.sAk = 1;
    g.B = P->ts.as<double>(); g.sBk = 1; g.sBn = n;
    g.C = P->cholS.as<double>(); g.sCm = 1; g.sCn = ksz;
    g.M = g.N = ksz; g.K = n;
    g.flags = GEMM_TRI_LOWER;
    LRN_TRY(gemm(st, g));
    hipLaunchKernelGGL(add_eye_kernel, dim3(nb(ksz)), dim3(256), 0, st, P->cholS.as<double>(), ksz);
    // explicit (S + I)^-1 with one step of iterative refinement in the apply: three single-launch mat-vecs instead of the
    // eight super-block launches of the two triangular solves per CG iteration (Solvers.jl:883)
    P->has_inv = ksz <= 8192 && (c->opt.prec_inv == 1 || (c->opt.prec_inv < 0 && ksz >= 256));
    if (P->has_inv) {
      LRN_TRY(ensure(c, P->Sm, (size_t)ksz * ksz * 8));
      LRN_HIP(c, hipMemcpyAsync(P->Sm.p, P->cholS.p, (size_t)ksz * ksz * 8, hipMemcpyDeviceToDevice, st));
      mirror_lower(st, P->Sm.as<double>(), ksz);
    }
    LRN_TRY(ensure(c, P->workS, chol_work_doubles(ksz) * 8));
    LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 4, st));
    LRN_TRY(potrf_lower(st, P->cholS.as<double>(), ksz, ksz, P->workS.as<double>(), c->info_dev.as<int>()));
    int h = 0;
    LRN_TRY(copy_out(c, &h, c->info_dev.p, 4));
    if (h != 0) { if (info) *info = h; return LRN_OK; }
    if (P->has_inv) {
      LRN_TRY(ensure(c, P->Ainv, (size_t)ksz * ksz * 8));
      LRN_TRY(ensure_m(c, ksz));
      double* Li = c->m0.as<double>();
      double* LiT = c->m1.as<double>();
      LRN_TRY(ensure(c, P->workS, (chol_work_doubles(ksz) + (size_t)CHOL_NB * ksz) * 8));
      eye_mat(st, Li, ksz);
      LRN_TRY(trsm_left_lower(st, P->cholS.as<double>(), ksz, ksz, false, Li, ksz, ksz,
                              P->workS.as<double>() + chol_work_doubles(ksz)));
      transpose_mat(st, Li, ksz, LiT);
      LRN_TRY(gemm_nt_sym(st, ksz, LiT, LiT, P->Ainv.as<double>(), 1.0));      // L^-T L^-1
    }
    LRN_TRY(ensure(c, P->y, (size_t)(ksz + 64) * 8));
    LRN_TRY(ensure(c, P->y2, (size_t)(ksz + 64) * 8));
    LRN_TRY(ensure(c, P->y3, (size_t)(ksz + 64) * 8));
    LRN_TRY(ensure(c, P->y4, (size_t)(ksz + 64) * 8));
    LRN_TRY(ensure(c, P->zpart, (size_t)32 * n * 8));
  }
  if (c->profile) {
    (void)hipEventRecord(a1, st); (void)hipEventSynchronize(a1);
    float ms = 0; (void)hipEventElapsedTime(&ms, a0, a1);
    c->timing["prec_setup"] += ms; c->counts["prec_setup"] += 1;
    (void)hipEventDestroy(a0); (void)hipEventDestroy(a1);
  }
  LRN_HIP(c, hipGetLastError());
  return LRN_OK;
}

// Minv[i,j] = (delta_ij - G[i,j]) / sqrt(d_i d_j) on the lower triangle (G = T1 ts', lower tiles)
__global__ void minv_finish_kernel(double* __restrict__ Mi, int n, const double* __restrict__ d) {
  const long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int i = (int)(e % n), j = (int)(e / n);
    if (i >= j) Mi[e] = ((i == j ? 1.0 : 0.0) - Mi[e]) / sqrt(d[i] * d[j]);
  }
}

// H_alpha as a dense matrix: is it worth forming for `expected` applications?  (static model, as hop_worthwhile)
static bool prec_dense_worthwhile(const lrn_ctx* c, const Prec* P, long expected) {
  if (!P || P->kind != 1 || P->has_LD || !P->has_inv || c->opt.prec_dense == 1) return false;
  const double n = c->nvar, k = P->ksz;
  if (c->nvar > 8192 || c->nvar < 256) return false;
  if (c->opt.prec_dense == 2) return true;
  const double setup = (6.0 * n * k * k + n * n * k) / 3.5e13 + 80e-6;      // T1 with one refinement step, T1 ts' (lower tiles)
  const double per_apply = 45e-6;                                            // seven launches -> two
  return (double)expected * per_apply > 1.2 * setup;
}

// T1 = ts (S + I)^-1 with one step of refinement (the accuracy of the SMW apply, which refines too), Minv from it
static int prec_dense_build(lrn_ctx* c, Prec* P) {
  const int n = c->nvar, ksz = P->ksz;
  hipStream_t st = c->stream;
  LRN_TRY(ensure(c, P->Minv, (size_t)n * n * 8));
  LRN_TRY(ensure(c, P->T1, (size_t)2 * n * ksz * 8));
  double* T1 = P->T1.as<double>();
  double* R = T1 + (size_t)n * ksz;
  auto mm = [&](const double* A, const double* B, double* C, double alpha, double beta) -> int {   // C = alpha A B + beta C, (n x ksz)(ksz x ksz), B symmetric
    GemmDesc g;
    g.A = A; g.sAm = 1; g.sAk = n;
    g.B = B; g.sBk = 1; g.sBn = ksz;
    g.C = C; g.sCm = 1; g.sCn = n;
    g.M = n; g.N = ksz; g.K = ksz;
    g.alpha = alpha; g.beta = beta;
    return gemm(st, g);
  };
  LRN_TRY(mm(P->ts.as<double>(), P->Ainv.as<double>(), T1, 1.0, 0.0));
  LRN_HIP(c, hipMemcpyAsync(R, P->ts.p, (size_t)n * ksz * 8, hipMemcpyDeviceToDevice, st));
  LRN_TRY(mm(T1, P->Sm.as<double>(), R, -1.0, 1.0));                        // R = ts - T1 (S + I)
  LRN_TRY(mm(R, P->Ainv.as<double>(), T1, 1.0, 1.0));                       // T1 += R (S + I)^-1
  GemmDesc g;                                                               // G = T1 ts' (lower tiles)
  g.A = T1; g.sAm = 1; g.sAk = n;
  g.B = P->ts.as<double>(); g.sBk = n; g.sBn = 1;
  g.C = P->Minv.as<double>(); g.sCm = 1; g.sCn = n;
  g.M = g.N = n; g.K = ksz;
  g.flags = GEMM_TRI_LOWER;
  LRN_TRY(gemm(st, g));
  hipLaunchKernelGGL(minv_finish_kernel, dim3(nb((long)n * n)), dim3(256), 0, st, P->Minv.as<double>(), n, P->d.as<double>());
  P->has_dense = true;
  c->counts["prec_dense_build"] += 1;
  return LRN_OK;
}

// Mx = M^-1 x, device vectors; tmpv: nvar scratch
int prec_apply_dev(lrn_ctx* c, const double* x, double* Mx, double* tmpv) {
  Prec* P = c->prec;
  const int n = c->nvar;
  hipStream_t st = c->stream;
  if (!P || P->kind == 0) {                                  // MyM_no  (Solvers.jl:620-622)
    LRN_HIP(c, hipMemcpyAsync(Mx, x, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    return LRN_OK;
  }
  if (P->kind == 2) {                                        // MyM_beta (Solvers.jl:670-672)
    hipLaunchKernelGGL(div_kernel, dim3(nb(n)), dim3(256), 0, st, x, P->d.as<double>(), Mx, n, 0);
    return LRN_OK;
  }
  if (P->has_dense) {                                        // (lrn_pcg when the cost model formed it; option prec_dense = 2)
    c->counts["prec_dense_apply"] += 1;
    return symv_lower(c, P->Minv.as<double>(), n, nullptr, x, Mx);
  }
  const int ksz = P->ksz;                                    // MyM (Solvers.jl:866-904), ts form
  if (P->has_LD) {      // v = L_D^-1 x  (d holds ones)
    hipLaunchKernelGGL(div_kernel, dim3(nb(n)), dim3(256), 0, st, x, P->d.as<double>(), tmpv, n, 1);
    LRN_TRY(trsm_left_lower(st, P->LD.as<double>(), n, n, false, tmpv, 1, n, P->workD.as<double>() + chol_work_doubles(n)));
    hipLaunchKernelGGL(gemv_t_kernel, dim3(ksz), dim3(256), 0, st, P->ts.as<double>(), n, tmpv, (const double*)nullptr,
                       P->y.as<double>());
  } else {              // v = x ./ sqrt(d) formed inside the two kernels that read it (same operations, one launch less)
    hipLaunchKernelGGL(gemv_t_kernel, dim3(ksz), dim3(256), 0, st, P->ts.as<double>(), n, x, P->d.as<double>(),
                       P->y.as<double>());
  }
  if (P->has_inv) {
    // y2 = Ainv y; refinement: y3 = y - (S + I) y2, y2 += Ainv y3 -- the accuracy of the triangular solves, three launches
    const unsigned g16 = (unsigned)((ksz + 15) / 16);
    const size_t lds = (size_t)ksz * 8;
    hipLaunchKernelGGL(symv_rows_kernel, dim3(g16), dim3(256), lds, st, P->Ainv.as<double>(), ksz, P->y.as<double>(),
                       (const double*)nullptr, 1.0, 0.0, P->y4.as<double>());
    hipLaunchKernelGGL(symv_rows_kernel, dim3(g16), dim3(256), lds, st, P->Sm.as<double>(), ksz, P->y4.as<double>(),
                       P->y.as<double>(), -1.0, 1.0, P->y3.as<double>());
    hipLaunchKernelGGL(symv_rows_kernel, dim3(g16), dim3(256), lds, st, P->Ainv.as<double>(), ksz, P->y3.as<double>(),
                       P->y4.as<double>(), 1.0, 1.0, P->y2.as<double>());
  } else {
    LRN_TRY(potrs_vec(st, P->cholS.as<double>(), ksz, ksz, P->y.as<double>(), P->y2.as<double>(), P->y3.as<double>(),
                      P->y4.as<double>()));
  }
  const int nchunk = std::min(32, std::max(1, ksz / 32));
  const int cper = (ksz + nchunk - 1) / nchunk;
  hipLaunchKernelGGL(gemv_n_part_kernel, dim3((n + 255) / 256, nchunk), dim3(256), 0, st, P->ts.as<double>(), n, ksz,
                     cper, P->y2.as<double>(), P->zpart.as<double>());
  hipLaunchKernelGGL(smw_final_kernel, dim3(nb(n)), dim3(256), 0, st, P->has_LD ? tmpv : x, P->zpart.as<double>(), nchunk, n,
                     P->d.as<double>(), Mx, P->has_LD ? 0 : 1);
  if (P->has_LD)
    LRN_TRY(trsm_left_lower(st, P->LD.as<double>(), n, n, true, Mx, 1, n, P->workD.as<double>() + chol_work_doubles(n)));
  return LRN_OK;
}

// Which operator serves this NT scaling: the assembled Schur matrix (hop.hip) or the matrix-free MyA.  Decided once per
// scaling from the static cost model and the CG iterations of the previous scaling; with a communicator the ranks take
// the decision together (free memory and so the assembly path can differ between them).
int op_select(lrn_ctx* c, bool* use_h) {
  if (c->hop_version != c->scal_version) {
    c->cg_prev_iters = c->cg_cur_iters;
    c->cg_cur_iters = 0;
    bool use = hop_worthwhile(c, c->cg_prev_iters);
    if (c->comm && c->world > 1) {
      double w[1] = {use ? 0.0 : 1.0};
      LRN_TRY(comm_status_max(c, w, 1));
      use = w[0] == 0.0;
    }
    c->hop_use = use;
    c->hop_version = c->scal_version;
  }
  if (c->hop_use) {
    const int rc = hop_prepare(c);
    if (rc != LRN_OK) {
      if (c->comm && c->world > 1) return rc;       // (every rank returns it: the status reduction of the exchange)
      c->hop_use = false;                            // one GPU: the matrix-free operator needs no workspace
      c->counts["hop_fallback"] += 1;
      c->err.clear();
    }
  }
  *use_h = c->hop_use;
  return LRN_OK;
}

// Ap = A p by the selected operator (all-reduced when sharded)
static int op_apply(lrn_ctx* c, bool use_h, const double* p, double* Ap, double* qpart = nullptr, int* nq = nullptr) {
  const bool sharded = c->comm && c->world > 1;
  if (nq) *nq = 0;
  if (use_h) {
    if (c->opt.profile_symv) tic(c);
    LRN_TRY(hop_apply(c, p, Ap, qpart, nq));
    if (c->opt.profile_symv) toc(c, "hop_symv");        // (measurement: this rank's share of H x alone, tools/shard_balance_c5.py)
  } else if (sharded) {
    // one process per GPU: this rank's rows of W M W, then ONE all-reduce of the nvar-vector on this stream -- the
    // recurrence is replicated and stays on the device, as on one GPU
    LRN_TRY(matvec_partial_dev(c, p, Ap, c->rank, c->world));
  } else {
    return matvec_dev(c, p, Ap);
  }
  if (sharded) LRN_TRY(comm_allreduce(c, Ap, c->nvar, 0));
  return LRN_OK;
}

// cg(A, b; tol, maxIter, precon) -- restates ConjugateGradients.jl 0.1 (see oracle.cg)
int pcg_dev(lrn_ctx* c, const double* b, double tol, int maxit, double* x, int* exit_code, int* iters) {
  const int n = c->nvar;
  hipStream_t st = c->stream;
  LRN_TRY(ensure(c, c->cgbuf, (size_t)(6 * (size_t)n + 64) * 8));
  double* r = c->cgbuf.as<double>();
  double* z = r + n;
  double* p = z + n;
  double* Ap = p + n;
  double* tmpv = Ap + n;
  double* scal = tmpv + n;          // 16 doubles
  constexpr int NSLOT = 16;
  if (!c->pin) {
    LRN_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->pin), NSLOT * 16 * 8, hipHostMallocMapped));
    LRN_HIP(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->pin_dev), c->pin, 0));
  }
  if (!c->pcg_ev[0])
    for (int i = 0; i < NSLOT; ++i) LRN_HIP(c, hipEventCreateWithFlags(&c->pcg_ev[i], hipEventDisableTiming));
  volatile double* hs = c->pin;
  // partial sums of the recurrence kernels and of the operator (hop.hip): after the six vectors
  const int nwg = std::max(1, std::min(CG_MAXWG, (n + 255) / 256));
  const int per = (n + nwg - 1) / nwg;
  LRN_TRY(ensure(c, c->cgpart, (size_t)(2 * CG_MAXWG + (n + 63) / 64 + 64) * 8));
  double* rrpart = c->cgpart.as<double>();
  double* zrpart = rrpart + CG_MAXWG;
  double* qpart = zrpart + CG_MAXWG;
  long nmv = 0;
  LRN_HIP(c, hipMemsetAsync(x, 0, (size_t)n * 8, st));
  LRN_HIP(c, hipMemsetAsync(scal, 0, 16 * 8, st));
  hipLaunchKernelGGL(cg_norm_kernel, dim3(1), dim3(1024), 0, st, b, n, scal, 6);
  double bb = 0.0;
  LRN_HIP(c, hipMemcpyAsync(&bb, scal + 6, 8, hipMemcpyDeviceToHost, st));
  LRN_HIP(c, hipStreamSynchronize(st));
  if (std::sqrt(bb) == 0.0) { *exit_code = 1; *iters = 0; return LRN_OK; }
  // r = b - A*0 = b
  LRN_HIP(c, hipMemcpyAsync(r, b, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
  const double residual_0 = std::sqrt(bb);
  if (residual_0 <= tol) { *exit_code = 2; *iters = 0; return LRN_OK; }
  for (int i = 0; i < NSLOT * 16; ++i) hs[i] = 0.0;
  bool use_h = false;
  LRN_TRY(op_select(c, &use_h));
  if (c->prec && !c->prec->has_dense && prec_dense_worthwhile(c, c->prec, c->cg_prev_iters)) LRN_TRY(prec_dense_build(c, c->prec));
  const int kind = (c->prec && (c->prec->kind == 1 || c->prec->kind == 2)) ? c->prec->kind : 0;
  const double* dprec = kind == 2 ? c->prec->d.as<double>() : nullptr;
  LRN_TRY(prec_apply_dev(c, r, z, tmpv));
  hipLaunchKernelGGL(cg_d_kernel, dim3(nwg), dim3(256), 0, st, z, r, p, n, per, nwg, scal, rrpart, (const double*)nullptr,
                     c->pin_dev, 0, residual_0, tol, 1);
  // The host runs `ahead` iterations in front of the convergence test it has read: the exit words of iteration `it` are
  // written to host-mapped memory by its kernels and looked at (behind an event) while iteration it + ahead is queued.
  const int ahead = std::max(0, std::min(NSLOT - 2, c->opt.pcg_lookahead));
  int done_code = 0, done_it = 0;
  auto poll = [&](int it) -> int {          // the words of iteration `it`
    const int s = it % NSLOT;
    LRN_HIP(c, hipEventSynchronize(c->pcg_ev[s]));
    if (hs[s * 16] != 0.0) { done_code = (int)hs[s * 16]; done_it = (int)hs[s * 16 + 1]; }
    return LRN_OK;
  };
  int it = 1;
  for (; it <= maxit && done_code == 0; ++it) {
    int nq = 0;
    LRN_TRY(op_apply(c, use_h, p, Ap, qpart, &nq));
    ++nmv;
    const int s = it % NSLOT;
    hipLaunchKernelGGL(cg_b_kernel, dim3(nwg), dim3(256), 0, st, p, Ap, r, x, z, kind, dprec, n, per, scal,
                       nq > 0 ? qpart : (const double*)nullptr, nq, rrpart, zrpart, c->pin_dev + s * 16, it);
    if (kind == 1) LRN_TRY(prec_apply_dev(c, r, z, tmpv));
    hipLaunchKernelGGL(cg_d_kernel, dim3(nwg), dim3(256), 0, st, z, r, p, n, per, nwg, scal, rrpart,
                       kind == 1 ? (const double*)nullptr : zrpart, c->pin_dev + s * 16, it, residual_0, tol, 0);
    LRN_HIP(c, hipEventRecord(c->pcg_ev[s], st));
    if (it - ahead >= 1) LRN_TRY(poll(it - ahead));
  }
  const int last = std::min(it - 1, maxit);
  for (int k = std::max(1, last - ahead + 1); k <= last && done_code == 0; ++k) LRN_TRY(poll(k));
  LRN_HIP(c, hipStreamSynchronize(st));
  LRN_HIP(c, hipGetLastError());
  c->counts["matvec"] += nmv;
  if (done_code != 0) { *exit_code = done_code; *iters = done_it; }
  else { *exit_code = -2; *iters = maxit; }
  c->cg_cur_iters += *iters;
  return LRN_OK;
}

}  // namespace lrn

using namespace lrn;

// the CG side (mat-vec, H_alpha, PCG) reads the entries of AA: not for factored blocks -- unless option "cg_factored" is set:
// then the operator runs in factor form (dataops.hip) or through H assembled in mode 1 (hop.hip) and ts of H_alpha comes from
// the factors.  One GPU only (partial: lrn_matvec_partial; world > 1: any call) -- the factor routes are not sharded
// ... and not for a block with diagonal parts (lrn_upload_diag), whatever cg_factored says: ts of H_alpha is built from the
// factors and the stored rows and would silently miss them
// ... unless option "cg_diag" is set beside cg_factored: then prec_setup adds the diagonal-row term to ts (diagops.hip::ts_diag);
// the operators carry the diagonal parts anyway.  One GPU and not lrn_matvec_partial, as for cg_factored
static int no_diag(lrn_ctx* c, const char* what, bool partial = false) {
  for (size_t il = 0; il < c->lmi.size(); ++il)
    if (c->lmi[il].factored && c->lmi[il].dg_n > 0) {
      if (c->opt.cg_diag != 0 && c->opt.cg_factored != 0 && (partial || c->world > 1))
        return set_error(c, LRN_ERR_STATE, "%s: block %d is factored with diagonal parts (lrn_upload_diag): option cg_diag runs on "
                                           "one GPU (world = %d) and not through lrn_matvec_partial", what, (int)il, c->world);
      if (cg_diag_on(c)) return LRN_OK;
      return set_error(c, LRN_ERR_STATE, "%s: block %d is factored with diagonal parts (lrn_upload_diag): the CG path does not "
                                         "hold them, such a model is solved with kit = 0", what, (int)il);
    }
  return LRN_OK;
}

static int no_factored(lrn_ctx* c, const char* what, bool partial = false) {
  LRN_TRY(no_diag(c, what, partial));
  for (size_t il = 0; il < c->lmi.size(); ++il)
    if (c->lmi[il].factored) {
      if (c->opt.cg_factored != 0 && (partial || c->world > 1))
        return set_error(c, LRN_ERR_STATE, "%s: block %d is factored (lrn_set_factored): option cg_factored runs on one GPU "
                                           "(world = %d) and not through lrn_matvec_partial", what, (int)il, c->world);
      if (c->opt.cg_factored != 0) return LRN_OK;
      return set_error(c, LRN_ERR_STATE, "%s: block %d is factored (lrn_set_factored): the CG path needs the constraint "
                                         "matrices, factored data is solved with kit = 0", what, (int)il);
    }
  return LRN_OK;
}

extern "C" int lrn_matvec(lrn_ctx* c, const double* x, double* Ax) {
  if (!c || !x || !Ax) return LRN_ERR_ARG;
  LRN_TRY(no_factored(c, "lrn_matvec"));
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v0.p, x, (size_t)n * 8));
  // the assembled-matrix operator only when lrn_pcg chose it for this scaling, or when it is forced (option matvec_h = 2)
  bool use_h = false;
  if (c->opt.matvec_h == 2 || (c->hop_use && c->hop_version == c->scal_version)) LRN_TRY(op_select(c, &use_h));
  tic(c);
  LRN_TRY(op_apply(c, use_h, c->v0.as<double>(), c->v1.as<double>()));
  toc(c, "matvec");
  return copy_out(c, Ax, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_matvec_partial(lrn_ctx* c, const double* x, double* Ax_partial) {
  if (!c || !x || !Ax_partial) return LRN_ERR_ARG;
  LRN_TRY(no_factored(c, "lrn_matvec_partial", true));
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v0.p, x, (size_t)n * 8));
  LRN_TRY(matvec_partial_dev(c, c->v0.as<double>(), c->v1.as<double>(), c->rank, c->world));
  return copy_out(c, Ax_partial, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_make_rhs(lrn_ctx* c, const double* Rp, const double* const* RdS, double* h) {
  if (!c || !Rp || !h || (c->nlmi > 0 && !RdS)) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v1.p, Rp, (size_t)n * 8));
  for (int il = 0; il < c->nlmi; ++il) {
    LmiBlock& b = c->lmi[il];
    if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set");
    LRN_TRY(ensure_m(c, b.msz));
    // wmw reads its middle factor transposed (everywhere else it is symmetric): it gets (Rd+S)', so that a Rd+S that is
    // not symmetric still gives W (Rd+S) W -- with constraint matrices that are not symmetric either the two differ
    LRN_TRY(copy_in(c, c->m1.p, RdS[il], (size_t)b.msz * b.msz * 8));
    transpose_mat(c->stream, c->m1.as<double>(), b.msz, c->m0.as<double>());
    LRN_TRY(wmw(c, b, c->m0.as<double>(), c->m1.as<double>(), c->m2.as<double>()));
    LRN_TRY(aa_times(c, b, c->m2.as<double>(), c->v1.as<double>()));
  }
  return copy_out(c, h, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_prec_setup(lrn_ctx* c, int prec, int erank, int aamat, int* info) {
  if (!c) return LRN_ERR_ARG;
  LRN_TRY(no_factored(c, "lrn_prec_setup"));
  LRN_HIP(c, hipSetDevice(c->device));
  return prec_setup(c, prec, erank, aamat, info);
}

extern "C" int lrn_prec_apply(lrn_ctx* c, const double* x, double* Mx) {
  if (!c || !x || !Mx) return LRN_ERR_ARG;
  LRN_TRY(no_diag(c, "lrn_prec_apply"));
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v0.p, x, (size_t)n * 8));
  if (c->prec && !c->prec->has_dense && c->opt.prec_dense == 2 && prec_dense_worthwhile(c, c->prec, 0))
    LRN_TRY(prec_dense_build(c, c->prec));
  LRN_TRY(prec_apply_dev(c, c->v0.as<double>(), c->v1.as<double>(), c->v2.as<double>()));
  return copy_out(c, Mx, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_pcg(lrn_ctx* c, const double* h, double tol, int maxit, double* x, int* exit_code, int* iters) {
  if (!c || !h || !x || !exit_code || !iters) return LRN_ERR_ARG;
  LRN_TRY(no_factored(c, "lrn_pcg"));
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v0.p, h, (size_t)n * 8));
  hipEvent_t a0, a1;
  if (c->profile) { (void)hipEventCreate(&a0); (void)hipEventCreate(&a1); (void)hipEventRecord(a0, c->stream); }
  const int rc = pcg_dev(c, c->v0.as<double>(), tol, maxit, c->v3.as<double>(), exit_code, iters);
  if (rc != LRN_OK) {
    if (c->profile) { (void)hipEventDestroy(a0); (void)hipEventDestroy(a1); }
    return rc;
  }
  if (c->profile) {
    (void)hipEventRecord(a1, c->stream); (void)hipEventSynchronize(a1);
    float ms = 0; (void)hipEventElapsedTime(&ms, a0, a1);
    c->timing["pcg"] += ms; c->counts["pcg"] += 1; c->counts["pcg_iters"] += *iters;
    (void)hipEventDestroy(a0); (void)hipEventDestroy(a1);
  }
  return copy_out(c, x, c->v3.p, (size_t)n * 8);
}
