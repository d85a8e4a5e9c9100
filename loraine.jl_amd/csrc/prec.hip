// The preconditioners of the CG path: none, H_beta (a diagonal) and the low-rank H_alpha -- setup, apply, dense form.
// Replaces MyM_no / MyM_beta / MyM, Prec_for_CG_beta, Prec_for_CG_tilS_prep, prec_alpha_S! (reference
// src/Solvers.jl:620-904).  Prec is private to this file; cgops.hip and api.hip go through prec.h.
//
// H_alpha apply uses the algebraically identical "ts" form of the SMW formula:
//   ts = D^-1/2 AA (U (x) Z)   (nvar x k*msz, built once per IP iteration)
//   M^-1 x = D^-1/2 [ v - ts (I + ts' ts)^-1 ts' v ],  v = D^-1/2 x
// i.e. two bandwidth-bound GEMVs and one POTRS on the (k*msz)^2 factor -- this also covers
// erank > 1 without materialising kron(Umat, Z) (Solvers.jl:759 would need msz^2 x k*msz).
#include <algorithm>
#include <cmath>

#include "prec.h"
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

// ------------------------------------------------------------------ H_alpha setup, step by step
static double tau_of(double lam_min, double mean_rest, int aamat) {      // Solvers.jl:646-650 / :715-719
  return aamat == 0 ? lam_min : (lam_min + mean_rest) / 2.0 - 1.0e-14;
}

// what the setup keeps of the spectrum of one W: Um = E[:, idx] .* coef', tau, the trace
struct BlkEig { std::vector<int> idx; std::vector<double> coef; double tau = 0.0, trace = 0.0; };

// Spectrum of one block from W, or from G when there is one (eig(W) = svd(G)^2), by Lanczos or Jacobi (option prec_eig).
// The eigenvectors are left in P->E (Lanczos: only if want_E).  e == null: the eigenvectors again and nothing else
static int block_spectrum(lrn_ctx* c, Prec* P, LmiBlock& b, int k, int aamat, bool want_E, BlkEig* e) {
  const int m = b.msz;
  if (!b.have_G && !b.have_W) return set_error(c, LRN_ERR_STATE, "preconditioner setup needs G or W (lrn_prepare_w)");
  const bool fromW = !b.have_G;     // eigen-free scaling: eig(W) from W itself (its singular values ARE its eigenvalues)
  if (k >= m) return set_error(c, LRN_ERR_ARG, "erank >= matrix size");
  const size_t mm = (size_t)m * m * 8;
  LRN_TRY(ensure(c, P->E, mm));
  LRN_TRY(ensure(c, P->sig, (size_t)m * 8));
  if (c->opt.prec_eig == 2 || (c->opt.prec_eig == 0 && m >= 256)) {
    // the setup only consumes the k largest eigenpairs, lambda_min and the mean of the rest
    // (lanczos.hip): O(steps * msz^2) instead of a full eigendecomposition
    std::vector<double> lam_top(std::max(1, k));
    double lam_min = 0.0, tr = 0.0;
    int steps = 0;
    LRN_TRY(lanczos_extremes(c, b.W.as<double>(), m, k, lam_top.data(), want_E ? P->E.as<double>() : nullptr, &lam_min, &tr,
                             e ? &steps : nullptr));
    if (!e) return LRN_OK;
    c->counts["prec_lanczos_steps"] = steps;
    double top = 0.0;
    for (int a = 0; a < k; ++a) top += lam_top[a];
    e->tau = tau_of(lam_min, (tr - top) / (double)(m - k), aamat);
    e->trace = tr;
    for (int a = 0; a < k; ++a) {
      e->idx.push_back(a);                                                // Ritz vectors are unit columns 0..k-1
      e->coef.push_back(std::sqrt(std::max(lam_top[a] - e->tau, 0.0)));
    }
    return LRN_OK;
  }
  LRN_HIP(c, hipMemcpyAsync(P->E.p, fromW ? b.W.p : b.G.p, mm, hipMemcpyDeviceToDevice, c->stream));
  int sweeps = 0;
  // eig(W) = svd(G)^2 : columns of E become sigma_j u_j   (Solvers.jl:642,706)
  LRN_TRY(jacobi_svd(c, P->E.as<double>(), nullptr, P->sig.as<double>(), m, &sweeps));
  if (!e) return LRN_OK;
  std::vector<double> sg(m);
  LRN_TRY(copy_out(c, sg.data(), P->sig.p, (size_t)m * 8));
  std::vector<int> ord(m);
  for (int i = 0; i < m; ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return sg[x] < sg[y]; });   // ascending
  auto lam_of = [&](int i) { return fromW ? sg[i] : sg[i] * sg[i]; };
  double mn = lam_of(ord[0]), sum = 0.0;
  for (int i = 0; i < m - k; ++i) { mn = std::min(mn, lam_of(ord[i])); sum += lam_of(ord[i]); }
  e->tau = tau_of(mn, sum / (double)(m - k), aamat);
  for (int i = 0; i < m; ++i) e->trace += lam_of(i);
  for (int a = 0; a < k; ++a) {
    const int id = ord[m - k + a];
    e->idx.push_back(id);
    e->coef.push_back(std::sqrt(std::max(lam_of(id) - e->tau, 0.0)) / sg[id]);   // Umat = v_l sqrt(lambda_l - tau)
  }
  return LRN_OK;
}

// kind 1 with linear rows: L_D L_D' = dsum I + (C_lin sqrt(xs)) (C_lin sqrt(xs))'; *h = the info of its factorisation
static int ld_factor(lrn_ctx* c, Prec* P, int* h) {
  const int n = c->nvar, nl = c->nlin;
  hipStream_t st = c->stream;
  LRN_TRY(ensure(c, P->Cd, (size_t)n * nl * 8));
  LRN_TRY(ensure(c, P->LD, (size_t)n * n * 8));
  LRN_TRY(ensure(c, P->workD, (chol_work_doubles(n) + (size_t)CHOL_NB * std::max(P->ksz, 1)) * 8));
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
  hipLaunchKernelGGL(prec_add_diag_kernel, dim3(nb(n)), dim3(256), 0, st, P->LD.as<double>(), n, P->dsum);
  LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 4, st));
  LRN_TRY(potrf_lower(st, P->LD.as<double>(), n, n, P->workD.as<double>(), c->info_dev.as<int>()));
  return copy_out(c, h, c->info_dev.p, 4);
}

// Um = E[:, idx] .* coef' into P->Um and Z = chol(2 W0 + Um Um') = chol(2W - Um Um') (Solvers.jl:725-731) into c->m0, upper
// triangle zeroed; *h = the info of the last attempt
static int block_z(lrn_ctx* c, Prec* P, LmiBlock& b, const BlkEig& e, int k, int* h) {
  const int m = b.msz;
  hipStream_t st = c->stream;
  LRN_TRY(ensure(c, P->Um, (size_t)m * k * 8 + (size_t)k * 16));
  double* Um = P->Um.as<double>();
  double* coef_d = Um + (size_t)m * k;
  int* idx_d = reinterpret_cast<int*>(coef_d + k);
  LRN_TRY(copy_in(c, coef_d, e.coef.data(), (size_t)k * 8));
  LRN_TRY(copy_in(c, idx_d, e.idx.data(), (size_t)k * 4));
  hipLaunchKernelGGL(umat_kernel, dim3(nb((long)m * k)), dim3(256), 0, st, P->E.as<double>(), m, idx_d, coef_d, k, Um);
  LRN_TRY(ensure_m(c, m));
  double* Zf = c->m0.as<double>();
  LRN_TRY(ensure(c, P->workS, chol_work_doubles(std::max(m, P->ksz)) * 8));      // (covers the factorisation of S + I as well)
  // 2W - UU' is positive definite in exact arithmetic; late in the solve cond(W) passes 1e16 and
  // the rounding of W = GG' can cost the factorisation (the reference's eigen-based W0 is exposed to
  // the same, Solvers.jl:725-731 raise PosDefException).  A preconditioner only has to be SPD:
  // retry with a relative diagonal shift instead of giving up.
  for (int attempt = 0; attempt < 4; ++attempt) {
    hipLaunchKernelGGL(zfull_kernel, dim3(nb((long)m * m)), dim3(256), 0, st, b.W.as<double>(), Um, m, k, Zf);
    if (attempt > 0) {
      const double shift = e.trace / m * 1e-15 * std::pow(100.0, attempt);
      hipLaunchKernelGGL(prec_add_diag_kernel, dim3(nb(m)), dim3(256), 0, st, Zf, m, shift);
      c->counts["prec_z_shift"] += 1;
    }
    LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 4, st));
    LRN_TRY(potrf_lower(st, Zf, m, m, P->workS.as<double>(), c->info_dev.as<int>()));
    LRN_TRY(copy_out(c, h, c->info_dev.p, 4));
    if (*h == 0) break;
  }
  if (*h == 0) hipLaunchKernelGGL(tril2_kernel, dim3(nb((long)m * m)), dim3(256), 0, st, Zf, m);
  return LRN_OK;
}

// ts[:, a m .. a m + m) of one block, a < k, from its stored entries: (D^-1/2 A u_a)' Z.  Full: every row of the block's
// slice `ts`.  Compact (the stored rows of a hybrid factored block, whose weight-0 factor columns left them at zero): on a
// compact npos_nz x msz buffer -- nothing here has nvar rows -- then each row to its natural place
static int ts_stored_rows(lrn_ctx* c, Prec* P, LmiBlock& b, const double* Zf, int k, bool compact, double* ts) {
  const int n = c->nvar, m = b.msz, ld = compact ? b.npos_nz : n;
  hipStream_t st = c->stream;
  LRN_TRY(ensure(c, P->AU, (size_t)(compact ? 2 : 1) * ld * m * 8));
  double* AU = P->AU.as<double>();
  double* Cc = AU + (size_t)ld * m;      // (compact only)
  for (int a = 0; a < k; ++a) {
    double* tsa = ts + (size_t)a * m * n;
    LRN_HIP(c, hipMemsetAsync(AU, 0, (size_t)ld * m * 8, st));
    const double* Ucol = P->Um.as<double>() + (size_t)a * m;
    if (b.npos_nz > b.nd)
      hipLaunchKernelGGL(au_sparse_kernel, dim3(nb(b.npos_nz - b.nd)), dim3(256), 0, st, b.ent_ptr.as<long>(),
                         b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(), b.nd, b.npos_nz,
                         b.sigma_d.as<int>(), Ucol, P->d.as<double>(), ld, AU, compact ? 1 : 0);
    if (b.nd > 0)
      hipLaunchKernelGGL(au_dense_kernel, dim3(b.nd), dim3(256), 0, st, b.Adense.as<double>(), m, b.sigma_d.as<int>(),
                         Ucol, P->d.as<double>(), ld, AU, compact ? 1 : 0);
    GemmDesc g;
    g.A = AU; g.sAm = 1; g.sAk = ld;
    g.B = Zf; g.sBk = 1; g.sBn = m;
    g.C = compact ? Cc : tsa; g.sCm = 1; g.sCn = ld;
    g.M = ld; g.N = m; g.K = m;
    LRN_TRY(gemm(st, g));
    if (compact)
      hipLaunchKernelGGL(ts_store_rows_kernel, dim3(nb((long)ld * m)), dim3(256), 0, st, Cc, ld, m, b.sigma_d.as<int>(), n, tsa);
  }
  return LRN_OK;
}

// per-setup counters, each the value of the LAST setup: blocks whose part of ts came from the factors, rows of ts filled from
// the stored entries of hybrid blocks, rows that got the term of their diagonal part (option "cg_diag"), blocks among
// `factored` whose part came from the compacted columns (option "ragged_ts")
struct TsCounts { long factored = 0, stored_rows = 0, diag_rows = 0, ragged = 0; };
static void ts_counts_store(lrn_ctx* c, const TsCounts& t) {
  c->counts["prec_ts_factored"] = t.factored;
  c->counts["prec_ts_stored_rows"] = t.stored_rows;
  c->counts["prec_ts_diag_rows"] = t.diag_rows;
  c->counts["prec_ts_ragged"] = t.ragged;
}

// ts of one block from the rank-k factors: P = L' V and T = V' Um, then fac_ts of facops.hip (the whole nvar x k m block, every
// element once).  V = Vd, or under option "ragged_ts" the Rc compacted columns Vc of a block of mixed ranks; a uniform block
// keeps the padded columns, bit for bit.  Then the stored rows of a hybrid block and the diagonal parts
static int ts_from_factors(lrn_ctx* c, Prec* P, LmiBlock& b, const double* Zf, int k, double* ts, TsCounts* tc) {
  const int m = b.msz;
  const double* Um = P->Um.as<double>();
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
  LRN_TRY(gemm(c->stream, gt));
  LRN_TRY(fac_ts(c, b, v, c->BG.as<double>(), P->Tf.as<double>(), P->d.as<double>(), k, ts));
  if (rts) ++tc->ragged;
  ++tc->factored;
  if (b.hybrid()) {
    LRN_TRY(ts_stored_rows(c, P, b, Zf, k, true, ts));
    tc->stored_rows += b.npos_nz;
  }
  if (b.factored && b.dg_n > 0) {
    // diagonal parts (option "cg_diag": lrn_prec_setup refused the block without it): -(L' diag(a_s) u_a)' / sqrt(d_j) added
    // to the rows fac_ts_kernel wrote the factor part of -- no stored row among them
    if (c->opt.profile_ops) tic(c);
    LRN_TRY(ts_diag(c, b, Zf, Um, k, P->d.as<double>(), ts));
    if (c->opt.profile_ops) toc(c, "prec_ts_diag");
    tc->diag_rows += b.dg_n;
  }
  return LRN_OK;
}

// SMW core: S = ts' ts + I and cholS (Solvers.jl:804-805), *h = the info of its factorisation; the explicit inverse where
// option prec_inv asks for it; the work vectors of the apply
static int smw_core(lrn_ctx* c, Prec* P, int* h) {
  const int n = c->nvar, ksz = P->ksz;
  hipStream_t st = c->stream;
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
  LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 4, st));
  LRN_TRY(potrf_lower(st, P->cholS.as<double>(), ksz, ksz, P->workS.as<double>(), c->info_dev.as<int>()));
  LRN_TRY(copy_out(c, h, c->info_dev.p, 4));
  if (*h != 0) return LRN_OK;
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
  for (DBuf* y : {&P->y, &P->y2, &P->y3, &P->y4}) LRN_TRY(ensure(c, *y, (size_t)(ksz + 64) * 8));
  return ensure(c, P->zpart, (size_t)32 * n * 8);
}

int prec_setup(lrn_ctx* c, int kind, int erank, int aamat, int* info) {
  int h = 0;
  if (!info) info = &h;
  *info = 0;
  if (!c->prec) c->prec = new Prec();
  Prec* P = c->prec;
  P->kind = kind;
  P->erank = erank;
  P->has_dense = false;
  TsCounts tc;
  ts_counts_store(c, tc);
  const int n = c->nvar;
  if (kind == 0) return LRN_OK;
  if (kind != 1 && kind != 2) return set_error(c, LRN_ERR_ARG, "preconditioner %d not supported", kind);
  if (c->nlmi < 1) return set_error(c, LRN_ERR_STATE, "preconditioner needs at least one LMI block");
  P->has_LD = kind == 1 && c->nlin > 0;
  PhaseTimer timer(c, c->profile);
  P->ksz = 0;
  for (auto& b : c->lmi) P->ksz += erank * b.msz;
  LRN_TRY(ensure(c, P->d, (size_t)n * 8));
  std::vector<BlkEig> be(c->nlmi);
  P->dsum = 0.0;
  for (int il = 0; il < c->nlmi; ++il) {
    LRN_TRY(block_spectrum(c, P, c->lmi[il], erank, aamat, kind == 1, &be[il]));
    if (aamat < 3) P->dsum += be[il].tau * be[il].tau;
  }
  hipLaunchKernelGGL(fill_kernel, dim3(nb(n)), dim3(256), 0, c->stream, P->d.as<double>(), n, P->has_LD ? 1.0 : P->dsum);
  // a factorisation that fails (L_D, Z after its four attempts, S + I) is an ordinary numerical exit: its info, LRN_OK
  if (P->has_LD) {
    LRN_TRY(ld_factor(c, P, info));
    if (*info != 0) return LRN_OK;
  } else if (c->nlin > 0)
    lin_diag(c, P->d.as<double>());
  if (kind == 1) {
    LRN_TRY(ensure(c, P->ts, (size_t)n * P->ksz * 8));
    double* ts = P->ts.as<double>();
    for (int il = 0; il < c->nlmi; ++il) {
      LmiBlock& b = c->lmi[il];
      // eigenvectors again (E was overwritten by later blocks only when nlmi > 1)
      if (c->nlmi > 1) LRN_TRY(block_spectrum(c, P, b, erank, aamat, true, nullptr));
      LRN_TRY(block_z(c, P, b, be[il], erank, info));
      if (*info != 0) return LRN_OK;
      const double* Zf = c->m0.as<double>();
      // a factored block (option "cg_factored") has no choice to make: there are no entries to take ts from
      if (b.factored || cg_lowrank_ts(c, b, erank)) LRN_TRY(ts_from_factors(c, P, b, Zf, erank, ts, &tc));
      else LRN_TRY(ts_stored_rows(c, P, b, Zf, erank, false, ts));
      ts += (size_t)erank * b.msz * n;
    }
    ts_counts_store(c, tc);
    if (P->has_LD)      // ts = L_D^-1 t   (the reference: AAAATtau \ t, Solvers.jl:767)
      LRN_TRY(trsm_left_lower(c->stream, P->LD.as<double>(), n, n, false, P->ts.as<double>(), P->ksz, n,
                              P->workD.as<double>() + chol_work_doubles(n)));
    LRN_TRY(smw_core(c, P, info));
    if (*info != 0) return LRN_OK;
  }
  timer.stop("prec_setup");
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

// what pcg_dev needs of the last setup (prec.h)
int prec_kind(const lrn_ctx* c) { return c->prec && (c->prec->kind == 1 || c->prec->kind == 2) ? c->prec->kind : 0; }
const double* prec_diag(const lrn_ctx* c) { return prec_kind(c) == 2 ? c->prec->d.as<double>() : nullptr; }
int prec_dense_if_worthwhile(lrn_ctx* c, long expected) {
  if (!c->prec || c->prec->has_dense || !prec_dense_worthwhile(c, c->prec, expected)) return LRN_OK;
  return prec_dense_build(c, c->prec);
}

}  // namespace lrn
