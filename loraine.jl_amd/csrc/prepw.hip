// NT scaling on the device: prepare_W (reference src/prepare_W.jl:28-94).
//   X = L_X L_X', S = L_S L_S'  (blocked Cholesky, chol.hip)        :33-34
//   CC = L_S' L_X                 (MFMA GEMM)                        :39
//   CC V = U diag(D)              (one-sided Jacobi SVD, jacobi.hip) :42
//   G  = L_X V D^-1/2             (column scale + MFMA GEMM)         :60
//   Gi = D^1/2 V' L_X^-1          (blocked TRSM instead of inv(G))   :63
//   W  = G G'                     (MFMA GEMM, lower tiles + mirror)  :64
//   Si = L_S^-T L_S^-1            (TRSM with I, then GEMM)           :68
//   DDsi = 1/sqrt(diag(G' S G))   (GEMM S G + column dots)           :71-74
// prepare_w_block (the reference's SVD route) and prepare_w_ns (eigen-free, below) are drivers over named steps; both start
// from factor_pair.  The element-wise passes they launch are in matops.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/loraine_hip.h"
#include "ctx.h"
#include "jacobi.h"
#include "ops.h"
#include "reduce.h"

namespace lrn {

// colsum_j = sum_i |K_ij|, colsq_j = sum_i K_ij^2   (one workgroup per column)
__global__ __launch_bounds__(256) void colnorm_kernel(const double* __restrict__ K, int n, double* __restrict__ colsum,
                                                      double* __restrict__ colsq) {
  __shared__ double sh[4];
  const double* a = K + (long)blockIdx.x * n;
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { double v = a[i]; s += fabs(v); q += v * v; }
  s = wg_sum<4>(s, sh);
  q = wg_sum<4>(q, sh);
  if (threadIdx.x == 0) {
    colsum[blockIdx.x] = s;
    colsq[blockIdx.x] = q;
  }
}

// sc[0] = c = min(max_j colsum_j, sqrt(sum_j colsq_j)), sc[1] = 1/c   (one workgroup, fixed order)
__global__ __launch_bounds__(256) void normc_kernel(const double* __restrict__ colsum, const double* __restrict__ colsq,
                                                    int n, double* __restrict__ sc) {
  __shared__ double shm[4], shq[4];
  double mx = 0.0, q = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) { mx = fmax(mx, colsum[j]); q += colsq[j]; }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = mx;
  q = wg_sum<4>(q, shq);                      // (its second barrier publishes shm as well)
  if (threadIdx.x == 0) {
    double m1 = fmax(fmax(shm[0], shm[1]), fmax(shm[2], shm[3]));
    double fr = sqrt(q);
    double cc = fmin(m1, fr);
    if (!(cc > 0.0)) cc = 1.0;
    sc[0] = cc;
    sc[1] = 1.0 / cc;
  }
}

__global__ void set_sc_kernel(double* __restrict__ sc, double cval) {
  sc[0] = cval;
  sc[1] = 1.0 / cval;
}

__global__ void scale_dev_kernel(const double* __restrict__ K, const double* __restrict__ sc, long total,
                                 double* __restrict__ Y) {
  const double f = sc[1];
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) Y[e] = K[e] * f;
}

// T = a (3 I - a^2 P) / 2;  part[block] = sum (delta_ij - P_ij)^2 over the block's elements
__global__ __launch_bounds__(256) void ns_t_kernel(const double* __restrict__ P, int n, double a, double* __restrict__ T,
                                                   double* __restrict__ part) {
  __shared__ double sh[4];
  const long total = (long)n * n;
  const double a3 = 0.5 * a * a * a, a1 = 1.5 * a;
  double s = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const double p = P[e];
    const bool dg = (e % n) == (e / n);
    const double r = (dg ? 1.0 : 0.0) - p;
    s += r * r;
    T[e] = (dg ? a1 : 0.0) - a3 * p;
  }
  if (!part) return;
  s = wg_sum<4>(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void sum_sqrt_kernel(const double* __restrict__ part, int np, double* __restrict__ out) {
  __shared__ double sh[4];
  const double s = block_sum_parts(part, np, sh);
  if (threadIdx.x == 0) *out = sqrt(s);
}

// smallest pivot of a Cholesky factor: out = min_i L_ii^2
__global__ __launch_bounds__(256) void min_pivot_kernel(const double* __restrict__ L, int n, double* __restrict__ out) {
  __shared__ double sh[4];
  double m = 1e300;
  for (int i = threadIdx.x; i < n; i += 256) { const double v = L[(long)i * n + i]; m = fmin(m, v * v); }
  m = wave_min(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) *out = fmin(fmin(sh[0], sh[1]), fmin(sh[2], sh[3]));
}

// ------------------------------------------------------------------ streams and the two factorisations
// The second stream with its events evA / evB (the S side of a scaling beside the X side) and, where asked for, the third
// with evC / evD (T Z beside Y T in a Newton-Schulz step): created on first use, here only
static int ensure_side_streams(lrn_ctx* c, bool third) {
  if (!c->stream2) LRN_HIP(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
  if (!c->evA) {
    LRN_HIP(c, hipEventCreateWithFlags(&c->evA, hipEventDisableTiming));
    LRN_HIP(c, hipEventCreateWithFlags(&c->evB, hipEventDisableTiming));
  }
  if (third && !c->stream3) {
    LRN_HIP(c, hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking));
    LRN_HIP(c, hipEventCreateWithFlags(&c->evC, hipEventDisableTiming));
    LRN_HIP(c, hipEventCreateWithFlags(&c->evD, hipEventDisableTiming));
  }
  return LRN_OK;
}

// s2 starts after what st has queued, st continues after what s2 has queued
static int fork_to(lrn_ctx* c, hipStream_t st, hipStream_t s2) {
  if (s2 == st) return LRN_OK;
  LRN_HIP(c, hipEventRecord(c->evA, st));
  LRN_HIP(c, hipStreamWaitEvent(s2, c->evA, 0));
  return LRN_OK;
}
static int join_from(lrn_ctx* c, hipStream_t st, hipStream_t s2) {
  if (s2 == st) return LRN_OK;
  LRN_HIP(c, hipEventRecord(c->evB, s2));
  LRN_HIP(c, hipStreamWaitEvent(st, c->evB, 0));
  return LRN_OK;
}

// LX = chol(b.X) on st, LS = chol(b.S) on s2 (which may be st), lower triangular with stored zeros; cw, cw2: Cholesky work of
// either side.  The verdicts in the reference's order: *info = 1 (X not positive definite, prepare_W.jl:33), 2 (S, :34), 0 --
// nothing else is queued on a failed factor (no output is touched, every pass of the host's +1e-5 I loop costs the two
// factorisations only), and both streams are idle when this returns.  piv_dev (two doubles; may be null): the smallest
// pivots L_ii^2 of the two factors into minpiv[2] beside the verdicts
static int factor_pair(lrn_ctx* c, LmiBlock& b, double* LX, double* LS, double* cw, double* cw2, hipStream_t st,
                       hipStream_t s2, int* info, double* piv_dev, double* minpiv) {
  const int n = b.msz;
  const size_t mm = (size_t)n * n * 8;
  LRN_TRY(ensure(c, c->info_dev, 64));
  int* dinfo[2] = {c->info_dev.as<int>(), c->info_dev.as<int>() + 12};
  const struct { hipStream_t s; double* L; const void* src; double* work; } side[2] = {{st, LX, b.X.p, cw}, {s2, LS, b.S.p, cw2}};
  int h[2] = {0, 0};
  *info = 0;
  LRN_TRY(fork_to(c, st, s2));                               // X, S (and the workspace) are ready
  for (int i = 0; i < 2; ++i) {
    LRN_HIP(c, hipMemcpyAsync(side[i].L, side[i].src, mm, hipMemcpyDeviceToDevice, side[i].s));
    LRN_HIP(c, hipMemsetAsync(dinfo[i], 0, 4, side[i].s));
    LRN_TRY(potrf_lower(side[i].s, side[i].L, n, n, side[i].work, dinfo[i]));
    tril(side[i].s, side[i].L, n);
    if (piv_dev) hipLaunchKernelGGL(min_pivot_kernel, dim3(1), dim3(256), 0, side[i].s, side[i].L, n, piv_dev + i);
  }
  for (int i = 0; i < 2; ++i) {
    LRN_HIP(c, hipMemcpyAsync(&h[i], dinfo[i], 4, hipMemcpyDeviceToHost, side[i].s));
    if (piv_dev) LRN_HIP(c, hipMemcpyAsync(&minpiv[i], piv_dev + i, 8, hipMemcpyDeviceToHost, side[i].s));
  }
  LRN_HIP(c, hipStreamSynchronize(st));
  if (s2 != st) LRN_HIP(c, hipStreamSynchronize(s2));
  if (h[0] != 0 || h[1] != 0) *info = h[0] != 0 ? 1 : 2;
  return LRN_OK;
}

int nt_factor(lrn_ctx* c, LmiBlock& b, int* info, double* minpiv) {
  const int n = b.msz;
  const size_t mm = (size_t)n * n * 8;
  *info = 0;
  b.chol_valid = false;
  LRN_TRY(ensure(c, b.LXf, mm));
  LRN_TRY(ensure(c, b.LSf, mm));
  const size_t cwd = chol_work_doubles(n);
  LRN_TRY(ensure(c, c->lxbuf, (2 * cwd + 16) * 8));
  double* cw = c->lxbuf.as<double>();      // cholesky(X)
  double* cw2 = cw + cwd;                  // cholesky(S): beside cholesky(X) with two streams
  LRN_TRY(ensure_side_streams(c, false));
  hipStream_t s2 = c->opt.prepw_streams ? c->stream2 : c->stream;
  double hp[2] = {0.0, 0.0};
  tic(c);
  LRN_TRY(factor_pair(c, b, b.LXf.as<double>(), b.LSf.as<double>(), cw, cw2, c->stream, s2, info, cw2 + cwd, hp));
  toc(c, "prepw_chol");
  if (*info != 0) return LRN_OK;
  if (minpiv) { minpiv[0] = hp[0]; minpiv[1] = hp[1]; }
  b.chol_valid = true;
  return LRN_OK;
}

// ------------------------------------------------------------------ SVD route
// c->scratch of the SVD route: LX, LS, CC/tmp, V, Y, Y2 (6 n^2) + chol / trsm work x2 (one per stream)
struct SvdWork {
  double *LX, *LS, *CC, *V, *Y, *Y2;
  double *cw, *tw;        // cholesky(X), NB*n of the triangular solves
  double *cw2, *tw2;      // the same for the S side: beside the X side with two streams
};

static int svd_workspace(lrn_ctx* c, int n, SvdWork* w) {
  const size_t nn = (size_t)n * n, cwd = chol_work_doubles(n), twd = (size_t)CHOL_NB * n;
  LRN_TRY(ensure(c, c->scratch, (6 * nn + 2 * (cwd + twd) + 4 * (size_t)n) * 8));
  double* p = c->scratch.as<double>();
  auto take = [&p](size_t k) { double* q = p; p += k; return q; };          // (a braced list is evaluated left to right)
  *w = SvdWork{take(nn), take(nn), take(nn), take(nn), take(nn), take(nn), take(cwd), take(twd), take(cwd), take(twd)};
  return LRN_OK;
}

// Si = LS^-T LS^-1 on s2   (prepare_W.jl:68; on the second stream it overlaps everything up to the end of prepare_w_block)
static int si_from_ls(lrn_ctx* c, LmiBlock& b, const SvdWork& w, hipStream_t s2) {
  const int n = b.msz;
  eye_mat(s2, w.Y2, n);
  LRN_TRY(trsm_left_lower(s2, w.LS, n, n, false, w.Y2, n, n, s2 != c->stream ? w.tw2 : w.tw));
  LRN_TRY(gemm_nn(s2, n, w.Y2, true, w.Y2, false, b.Si.as<double>(), GEMM_TRI_LOWER));
  mirror_lower(s2, b.Si.as<double>(), n);
  return LRN_OK;
}

// SVD of CC = LS' LX = U D V' by one-sided Jacobi on CC' = LX' LS: its columns are rotated by
// U and converge to V D, so V = (columns / D) needs no accumulation of rotations -- the rounds
// are bandwidth-bound (every round streams the whole matrix), this removes the V half of it.
static int svd_of_cc(lrn_ctx* c, LmiBlock& b, const SvdWork& w) {
  const int n = b.msz;
  hipStream_t st = c->stream;
  int sweeps = 0;
  tic(c);
  LRN_TRY(gemm_nn(st, n, w.LX, true, w.LS, false, w.CC));
  // warm start: the left singular vectors of the previous IP iterate nearly orthogonalise the
  // columns of the new CC'
  if (b.have_Vprev && c->opt.jacobi_warm) {
    LRN_TRY(gemm_nn(st, n, w.CC, false, b.Vprev.as<double>(), false, w.Y));
    LRN_HIP(c, hipMemcpyAsync(w.CC, w.Y, (size_t)n * n * 8, hipMemcpyDeviceToDevice, st));
  }
  toc(c, "prepw_gemm");
  tic(c);
  LRN_TRY(jacobi_svd(c, w.CC, nullptr, b.D.as<double>(), n, &sweeps));
  scale_cols(st, w.CC, b.D.as<double>(), n, 2, w.V);
  c->counts["svd_sweeps"] = sweeps;
  toc(c, "prepw_svd");
  return LRN_OK;
}

// G = LX V D^-1/2, Gi = D^1/2 V' LX^-1, W = G G', DDsi = 1/sqrt(diag(G' S G))   (prepare_W.jl:60-74): the triangular solve
// for Gi on s2 beside the GEMMs; Si and Gi are complete when this returns
static int g_gi_w_ddsi(lrn_ctx* c, LmiBlock& b, const SvdWork& w, hipStream_t s2) {
  const int n = b.msz;
  hipStream_t st = c->stream;
  double *D = b.D.as<double>(), *G = b.G.as<double>();
  tic(c);
  // Gi' = LX^-T (V D^1/2)   (second stream: beside the GEMMs below; V, D and Y are free from here on)
  LRN_TRY(fork_to(c, st, s2));
  scale_cols(s2, w.V, D, n, 1, w.Y);
  LRN_TRY(trsm_left_lower(s2, w.LX, n, n, true, w.Y, n, n, s2 != st ? w.tw2 : w.tw));
  transpose_mat(s2, w.Y, n, b.Gi.as<double>());
  // G = LX (V D^-1/2)
  scale_cols(st, w.V, D, n, 0, w.CC);
  LRN_TRY(gemm_nn(st, n, w.LX, false, w.CC, false, G));
  if (c->opt.jacobi_warm) {          // U = LS' G D^-1/2  (G = LS^-T U D^1/2) for the next warm start
    LRN_TRY(ensure(c, b.Vprev, (size_t)n * n * 8));
    LRN_TRY(gemm_nn(st, n, w.LS, true, G, false, w.CC));
    scale_cols(st, w.CC, D, n, 0, b.Vprev.as<double>());
    b.have_Vprev = true;
  }
  // W = G G'
  LRN_TRY(gemm_nn(st, n, G, false, G, true, b.W.as<double>(), GEMM_TRI_LOWER));
  mirror_lower(st, b.W.as<double>(), n);
  // DDsi = 1/sqrt(diag(G' S G))
  LRN_TRY(gemm_nn(st, n, b.S.as<double>(), false, G, false, w.CC));
  coldot_rsqrt(st, G, w.CC, n, b.DDsi.as<double>());
  LRN_TRY(join_from(c, st, s2));
  toc(c, "prepw_gemm");
  LRN_HIP(c, hipGetLastError());
  return LRN_OK;
}

// Two streams (option "prepw_streams"): the S side -- cholesky(S), then Si = LS^-T LS^-1, which nothing before the
// end needs -- runs beside cholesky(X) and the Jacobi SVD, whose launches leave most of the chip idle; after the SVD
// the triangular solve for Gi runs beside the GEMMs for G, W and DDsi.
int prepare_w_block(lrn_ctx* c, LmiBlock& b, int* info) {
  SvdWork w;
  LRN_TRY(svd_workspace(c, b.msz, &w));
  hipStream_t s2 = c->stream;
  if (c->opt.prepw_streams != 0) {
    LRN_TRY(ensure_side_streams(c, false));
    s2 = c->stream2;
  }
  LRN_TRY(factor_pair(c, b, w.LX, w.LS, w.cw, w.cw2, c->stream, s2, info, nullptr, nullptr));
  if (*info != 0) return LRN_OK;
  // from here on an error return must not leave the second stream writing the shared scratch
  struct S2Guard { hipStream_t s; bool on; ~S2Guard() { if (on) (void)hipStreamSynchronize(s); } } guard{s2, s2 != c->stream};
  LRN_TRY(si_from_ls(c, b, w, s2));
  LRN_TRY(svd_of_cc(c, b, w));
  LRN_TRY(g_gi_w_ddsi(c, b, w, s2));
  guard.on = false;                                           // (joined through evB at the end of g_gi_w_ddsi)
  b.have_W = b.have_G = true;
  b.nt_free = false;
  c->scal_version += 1;
  return LRN_OK;
}

// ------------------------------------------------------------------ eigen-free route
// Eigen-free NT scaling (round 3).  The reference takes an SVD of L_S'L_X (prepare_W.jl:39-64) to get G, Gi, D; what
// the iteration consumes of them can be written with K = L_X' S L_X = V D^2 V' alone:
//   W = G G' = L_X K^-1/2 L_X'                                   (prepare_W.jl:64)
//   with B = L_X' dS L_X, T = K^-1/2 B K^-1/2, TX = L_X^-1 dX L_X^-T = -I - T (+ sm K^-1 + R in the corrector):
//   dX = L_X TX L_X' (predictor_corrector.jl:255,257); the scaled directions of the step-length rule (:263-285) are
//   orthogonally similar to TX and T (DDsi.*(Gi dX Gi').*DDsi = V' TX V, DDsi.*(G' dS G).*DDsi = V' T V), same eigmin;
//   G RNT G' (:186, :257, :309) = L_X R L_X' with K^1/2 R + R K^1/2 = -(N K^-1/2 + K^-1/2 N'), N = L_X^-1 dX dS L_X = TX B
//   G (G'RdG + D - sm/D - RNT) G' (:186) = W Rd W + X - sm Si - L_X R L_X'
// Nothing is inverted: products with an explicit L_X^-1 lose the directions through cancellation once cond(X) passes
// 1e10 (control1 left the trajectory at iteration 21 that way); in the L_X basis every term is O(1).
// K is well conditioned along a solve (D^2 = eig(XS) stays near the central path: cond(K) <~ 1e3 where cond(X) reaches
// 1e12), so Y = (K/c)^1/2 and Z = (K/c)^-1/2 come from the coupled Newton-Schulz iteration -- products only, on the MFMA:
//   P = Z Y, T = a (3 I - a^2 P)/2, Y <- Y T, Z <- T Z,
// taken LITERALLY: every iterate is symmetric in exact arithmetic, but the iteration is only stable as written -- with
// any product replaced by its transposed twin (Z Y' for Z Y), or with the iterates symmetrised after each step, the
// rounding-level commutator grows by a factor ~ cond(K)^1/2 per step once the residual is at its floor (measured on
// thetaG11: 2e-7 -> 1e+90 in eleven steps; /tmp-free NumPy reproduction in DESIGN.md).  The direct-to-LDS GEMM computes
// A Bm', so every product also stores its transpose (GemmDesc::C2) for the next one to read.
// With the one-sided scaling a = sqrt(3/(1 + l + l^2)), l <- a l (3 - a^2 l^2)/2 for spec(P)^1/2 in [l, 1]: the map never
// leaves (0, 1], so a wrong guess of l costs steps, never correctness.  c = min(||K||_1, ||K||_F) >= lambda_max(K).
// The steps are queued without host round trips; ||I - P||_F of every step comes back in one copy.
// tools/nt_eigenfree_proto.py emulates the whole route in NumPy against the SVD route of the oracle.
// c->scratch of the eigen-free route: P, T, Y' Z' of the resident set, a second set Ya Ya' Za Za' (8 n^2), then column
// norms, partial sums, residuals, scale
struct NsWork {
  double *Pm, *Tm, *Yt0, *Zt0, *Ya, *Yta, *Za, *Zta;
  double *colsum, *colsq;
  double *part;           // partial sums of ||I - P||_F^2
  double *res;            // res[0 .. maxit): ||I - P||_F at the start of every step, then sc[0 .. 1] = c, 1 / c
  double *sc;
  int npart, maxit;
};

static int ns_workspace(lrn_ctx* c, int n, NsWork* w) {
  const size_t nn = (size_t)n * n;
  const int npart = (int)std::min<size_t>(1024, (nn + 255) / 256);
  const int npart_alloc = std::max(npart, (int)((((long)n + 31) / 32) * (((long)n + 31) / 32 + 1) / 2));      // (gemm_nt_sym_ns: one per tile pair)
  const int maxit = std::max(4, std::min(c->opt.ns_maxit, 120));
  const size_t idle = 2 * nn + (size_t)CHOL_NB * n;           // (behind Zta: L_S^-1, L_S^-T and their solve until round 4)
  LRN_TRY(ensure(c, c->scratch, (8 * nn + idle + 2 * (size_t)n + npart_alloc + maxit + 64) * 8));
  double* p = c->scratch.as<double>();
  auto take = [&p](size_t k) { double* q = p; p += k; return q; };          // (a braced list is evaluated left to right)
  *w = NsWork{take(nn), take(nn), take(nn), take(nn), take(nn), take(nn), take(nn), take(nn + idle),
              take(n), take(n), take(npart_alloc), take(maxit), take(2), npart, maxit};
  return LRN_OK;
}

// K = CC' CC with CC = L_S' L_X (prepare_W.jl:39) into Tm, its column norms and the norm bound c = min(||K||_1, ||K||_F) into
// sc -- NOT L_X' S L_X: with cond(X), cond(S) at 1e10 the entries of |L_X'| |S| |L_X| are 1e10 times those of K and the
// explicit product has no correct digit left (measured: the Newton-Schulz iteration then diverges); through the factors
// the error is that of CC itself, which the SVD shares.  L_S' on s2 beside L_X' (b.LXt, kept for the step) on the stream.
// (round 4: S^-1 no longer through L_S^-1 -- a triangular solve with msz right-hand sides, 436 ms of a 2 s iteration at
// msz 10^4 -- but from what the iteration produces anyway: K = L_X' S L_X  =>  S^-1 = L_X K^-1 L_X', see ns_outputs)
static int ns_build_k(lrn_ctx* c, LmiBlock& b, const NsWork& w, hipStream_t s2) {
  const int n = b.msz;
  hipStream_t st = c->stream;
  double* LXt = b.LXt.as<double>();
  double* LSt = w.Zta;                               // (free until the first Newton-Schulz step, which st orders after its reader)
  transpose_mat(s2, b.LSf.as<double>(), n, LSt);
  if (s2 != st) LRN_HIP(c, hipEventRecord(c->evB, s2));
  transpose_mat(st, b.LXf.as<double>(), n, LXt);
  if (s2 != st) LRN_HIP(c, hipStreamWaitEvent(st, c->evB, 0));
  LRN_TRY(pgemm_nt(c, st, n, LXt, LSt, w.Pm, GEMM_KFROM_M, 1.0));                           // CC' = L_X' L_S (L_X' upper)
  LRN_TRY(pgemm_nt_sym(c, st, n, w.Pm, w.Pm, w.Tm, 1.0));                                  // K = CC' CC
  hipLaunchKernelGGL(colnorm_kernel, dim3(n), dim3(256), 0, st, w.Tm, n, w.colsum, w.colsq);
  hipLaunchKernelGGL(normc_kernel, dim3(1), dim3(256), 0, st, w.colsum, w.colsq, n, w.sc);
  return LRN_OK;
}

// Yh = K / c, and *ell2 = the lower end l^2 of the schedule.  Round 4: where a step of the iteration is expensive (three n^3
// products; msz >= ns_lanczos_min) the scale c and l come from a short Lanczos run on K instead of norm bounds and a fixed
// guess: the norm bound min(||K||_1, ||K||_F) is 1.4-7 x lambda_max on the iterates of theta1 / control1 / maxG11 (more as
// msz grows) and the assumed l^2 = 2e-3 four to forty times below lambda_min / lambda_max -- two to three steps of eight to
// ten.  c keeps a margin over the Ritz value (an eigenvalue above c would turn negative under the scaled map: the residual
// test then sends the iteration to the SVD route); l may be wrong in either direction (costs steps, never correctness).
static int ns_scale_and_schedule(lrn_ctx* c, LmiBlock& b, const NsWork& w, double* ell2) {
  const int n = b.msz;
  hipStream_t st = c->stream;
  *ell2 = std::min(std::max(c->opt.ns_l0, 1e-12), 0.25);
  if (c->opt.ns_lanczos != 0 && n >= c->opt.ns_lanczos_min) {
    double lo = 0.0, hi = 0.0, rh = 0.0;
    LRN_TRY(lanczos_ends(c, w.Tm, n, 24, &lo, &hi, &rh));
    double cn[2] = {0.0, 0.0};
    LRN_TRY(copy_out(c, cn, w.sc, 16));                              // the norm bound (always valid)
    const double cl = 1.05 * (hi + rh);
    if (hi > 0.0 && cl > 0.0 && cl < cn[0]) {
      hipLaunchKernelGGL(set_sc_kernel, dim3(1), dim3(1), 0, st, w.sc, cl);
      if (lo > 0.0) *ell2 = std::min(0.25, std::max(*ell2, 0.5 * lo / cl));
      c->counts["ns_lanczos_scaled"] += 1;
    }
  }
  hipLaunchKernelGGL(scale_dev_kernel, dim3(nb((long)n * n)), dim3(256), 0, st, w.Tm, w.sc, (long)n * n, b.Yh.as<double>());
  return LRN_OK;
}

// The iteration's state: the current set (Y, Y', Z, Z'), the set the next step writes, the steps taken
struct NsState {
  double *Yc, *Ytc, *Zc, *Ztc;
  double *Yn, *Ytn, *Zn, *Ztn;
  int k;
  bool z_is_eye;
  hipStream_t s3;         // T Z beside Y T on this stream (the context's stream: one after the other)
  bool dual;              // the transposed twin of a product from the GEMM epilogue, not from a pass of its own
};

// C = A Bm' and Ct = C' on sx.  The twin: stored by the GEMM epilogue (8-byte scattered stores: 61 against 35 us at msz 800
// on the 64-tile kernel) or by a transpose pass of its own (8 us there)
static int ns_product(lrn_ctx* c, hipStream_t sx, int n, bool dual, const double* A, const double* Bm, double* C, double* Ct) {
  if (dual) return pgemm_nt(c, sx, n, A, Bm, C, 0, 1.0, Ct);
  if (!products_sharded(c, sx, n)) {
    SlabSrc src;                                    // (a mid-size product: its slabs are added by the transpose pass)
    LRN_TRY(gemm_nt_slabs(sx, n, A, Bm, C, 1.0, &src));
    slabs_to_c_and_ct(sx, src, n, C, Ct);
    return LRN_OK;
  }
  LRN_TRY(pgemm_nt(c, sx, n, A, Bm, C, 0, 1.0));
  transpose_mat(sx, C, n, Ct);
  return LRN_OK;
}

// One step P = Z Y, T = a (3 I - a^2 P) / 2, Y <- Y T, Z <- T Z, queued; res[k] = ||I - P||_F.
// P = Z Y is the one product that may be symmetrised (lower tiles + mirror where that halves its cost): with T exactly
// symmetric and Y T, T Z taken literally the iteration stays stable (residual floor 1e-12 instead of 1e-13, NumPy and
// device) -- and T is its own transposed twin.  Y T and T Z are independent: the second one on a third stream, so that two
// workgroups share every CU where one product alone (256 tiles of 128 at msz 2000) leaves each CU a single workgroup
static int ns_step(lrn_ctx* c, int n, const NsWork& w, NsState& s, double a) {
  hipStream_t st = c->stream;
  const size_t mm = (size_t)n * n * 8;
  const double* Pk = s.Yc;                                // Z = I: P = Y (exactly symmetric)
  int np_k = w.npart;
  if (!s.z_is_eye && n < BIG_TILE_MIN_N && !products_sharded(c, st, n)) {
    // (mid sizes: symmetrisation, T and the residual in the pass that adds the product's slabs)
    LRN_TRY(gemm_nt_sym_ns(st, n, s.Zc, s.Ytc, w.Pm, a, w.Tm, w.part, &np_k));
  } else {
    if (!s.z_is_eye) { LRN_TRY(pgemm_nt_sym(c, st, n, s.Zc, s.Ytc, w.Pm, 1.0)); Pk = w.Pm; }
    hipLaunchKernelGGL(ns_t_kernel, dim3(w.npart), dim3(256), 0, st, Pk, n, a, w.Tm, w.part);
  }
  hipLaunchKernelGGL(sum_sqrt_kernel, dim3(1), dim3(256), 0, st, w.part, np_k, w.res + s.k);
  if (!s.z_is_eye && s.s3 != st) {
    LRN_HIP(c, hipEventRecord(c->evC, st));                                          // T, T' are final
    LRN_HIP(c, hipStreamWaitEvent(s.s3, c->evC, 0));
    LRN_TRY(ns_product(c, s.s3, n, s.dual, w.Tm, s.Ztc, s.Zn, s.Ztn));               // T Z
    LRN_HIP(c, hipEventRecord(c->evD, s.s3));
  }
  LRN_TRY(ns_product(c, st, n, s.dual, s.Yc, w.Tm, s.Yn, s.Ytn));                    // Y T
  if (s.z_is_eye) {
    LRN_HIP(c, hipMemcpyAsync(s.Zn, w.Tm, mm, hipMemcpyDeviceToDevice, st));
    LRN_HIP(c, hipMemcpyAsync(s.Ztn, w.Tm, mm, hipMemcpyDeviceToDevice, st));
    s.z_is_eye = false;
  } else if (s.s3 != st) {
    LRN_HIP(c, hipStreamWaitEvent(st, c->evD, 0));
  } else {
    LRN_TRY(ns_product(c, st, n, s.dual, w.Tm, s.Ztc, s.Zn, s.Ztn));                 // T Z
  }
  std::swap(s.Yc, s.Yn); std::swap(s.Ytc, s.Ytn); std::swap(s.Zc, s.Zn); std::swap(s.Ztc, s.Ztn);
  ++s.k;
  return LRN_OK;
}

// The planned steps -- with the one-sided scaling a = sqrt(3/(1 + l + l^2)) until the assumed interval is [1 - 5e-4, 1],
// then two plain ones: 3 (5e-4)^2 -> 1e-12 -- without a host round trip, then plain steps while the residuals ask for them.
// hres: the residuals of all steps and c behind them, as read last; *ok = false: not a matrix this iteration handles
static int ns_iterate(lrn_ctx* c, int n, const NsWork& w, double ell2, NsState& s, bool* ok, std::vector<double>& hres) {
  const int maxit = w.maxit;
  double ell = std::sqrt(ell2);
  while (s.k < maxit && 1.0 - ell > 5e-4) {
    const double a = std::sqrt(3.0 / (1.0 + ell + ell * ell));
    ell = 0.5 * a * ell * (3.0 - a * a * ell * ell);
    LRN_TRY(ns_step(c, n, w, s, a));
  }
  for (int e = 0; e < 2 && s.k < maxit; ++e) LRN_TRY(ns_step(c, n, w, s, 1.0));
  hres.assign(maxit + 2, 0.0);
  *ok = false;
  for (;;) {
    LRN_HIP(c, hipMemcpyAsync(hres.data(), w.res, (size_t)(maxit + 2) * 8, hipMemcpyDeviceToHost, c->stream));
    LRN_HIP(c, hipStreamSynchronize(c->stream));
    const double rl = hres[s.k - 1];         // ||I - P|| at the START of the last step: the step squares it
    if (!(rl == rl) || rl > 1e30) break;     // NaN / overflow
    if (rl <= 1e-6) { *ok = true; break; }   // (the literal iteration is quadratic down to 1e-13: the last step leaves <= 1e-12)
    if (s.k + 1 > maxit) break;
    LRN_TRY(ns_step(c, n, w, s, 1.0));
    if (rl > 1e-2 && s.k + 1 <= maxit) LRN_TRY(ns_step(c, n, w, s, 1.0));
  }
  return LRN_OK;
}

// Yh, Zh from the last set, then W = L_X K^-1/2 L_X' = L_X Z L_X' / sqrt(c) (prepare_W.jl:64), Ki = (K/c)^-1 = Zh^2 (the
// sigma_mu S^-1 term of the corrector in the L_X basis) and Si = S^-1 = L_X K^-1 L_X' = L_X Ki L_X' / c (prepare_W.jl:68):
// products with the triangular factor, nothing inverted
static int ns_outputs(lrn_ctx* c, LmiBlock& b, const NsWork& w, const NsState& s) {
  const int n = b.msz;
  const size_t mm = (size_t)n * n * 8;
  hipStream_t st = c->stream;
  double *LX = b.LXf.as<double>(), *Ki = b.Ki.as<double>();
  if (s.Yc != b.Yh.as<double>()) LRN_HIP(c, hipMemcpyAsync(b.Yh.p, s.Yc, mm, hipMemcpyDeviceToDevice, st));
  if (s.Zc != b.Zh.as<double>()) LRN_HIP(c, hipMemcpyAsync(b.Zh.p, s.Zc, mm, hipMemcpyDeviceToDevice, st));
  LRN_TRY(pgemm_nt(c, st, n, LX, s.Ztc, w.Pm, GEMM_KTO_M, 1.0));                         // (L_X lower triangular)
  LRN_TRY(pgemm_nt_sym(c, st, n, w.Pm, LX, b.W.as<double>(), 1.0 / std::sqrt(b.ns_c), GEMM_KTO_N));
  if (n >= BIG_TILE_MIN_N) LRN_TRY(pgemm_nt_sym(c, st, n, s.Zc, s.Ztc, Ki, 1.0));       // symmetric: lower tiles + mirror
  else LRN_TRY(pgemm_nt(c, st, n, s.Zc, s.Ztc, Ki, 0, 1.0));
  LRN_TRY(pgemm_nt(c, st, n, LX, Ki, w.Pm, GEMM_KTO_M, 1.0));                            // L_X Ki'  (Ki symmetric)
  LRN_TRY(pgemm_nt_sym(c, st, n, w.Pm, LX, b.Si.as<double>(), 1.0 / b.ns_c, GEMM_KTO_N));
  return LRN_OK;
}

int prepare_w_ns(lrn_ctx* c, LmiBlock& b, int* info, bool* converged) {
  const int n = b.msz;
  hipStream_t st = c->stream;
  *info = 0;
  *converged = false;
  b.nt_free = false;
  if (!b.chol_valid) {
    LRN_TRY(nt_factor(c, b, info, nullptr));
    if (*info != 0) return LRN_OK;
  }
  b.chol_valid = false;            // (consumed: whoever changes X, S afterwards need not remember to reset it)
  for (DBuf* d : {&b.LXt, &b.Yh, &b.Zh, &b.Ki, &b.Bs, &b.TX, &b.Qm}) LRN_TRY(ensure(c, *d, (size_t)n * n * 8));
  NsWork w;
  LRN_TRY(ns_workspace(c, n, &w));
  // (sharded products carry collectives: everything on the context's stream then, the order of the calls is the order of
  // the collectives on every rank)
  const bool side = c->opt.prepw_streams && !products_sharded(c, st, n);
  hipStream_t s2 = side ? c->stream2 : st;
  static const int s3_min = getenv("LRN_NS_S3_MIN") ? atoi(getenv("LRN_NS_S3_MIN")) : 1024;      // (measurement knob)
  const bool third = side && n >= s3_min;
  if (third) LRN_TRY(ensure_side_streams(c, true));
  LRN_TRY(fork_to(c, st, s2));
  tic(c);
  double ell2 = 0.0;
  LRN_TRY(ns_build_k(c, b, w, s2));
  LRN_TRY(ns_scale_and_schedule(c, b, w, &ell2));
  toc(c, "prepw_gemm");
  tic(c);
  NsState s{b.Yh.as<double>(), w.Yt0, b.Zh.as<double>(), w.Zt0, w.Ya, w.Yta, w.Za, w.Zta, 0, true, third ? c->stream3 : st,
            c->opt.ns_dual == 1 || (c->opt.ns_dual < 0 && n >= 1500)};
  transpose_mat(st, s.Yc, n, s.Ytc);
  bool ok = false;
  std::vector<double> hres;
  LRN_TRY(ns_iterate(c, n, w, ell2, s, &ok, hres));
  c->counts["ns_steps"] = s.k;
  toc(c, "prepw_ns");
  static const bool trace = getenv("LRN_NS_TRACE") != nullptr;
  if (trace) {
    fprintf(stderr, "[ns n=%d] ok=%d c=%.3e res:", n, (int)ok, hres[w.maxit]);
    for (int i = 0; i < s.k; ++i) fprintf(stderr, " %.2e", hres[i]);
    fprintf(stderr, "\n");
  }
  if (!ok) {
    if (s2 != st) LRN_HIP(c, hipStreamSynchronize(s2));
    c->counts["ns_fallback"] += 1;
    return LRN_OK;
  }
  tic(c);
  b.ns_c = hres[w.maxit];
  LRN_TRY(ns_outputs(c, b, w, s));
  LRN_TRY(join_from(c, st, s2));                              // (the transposes on the second stream)
  toc(c, "prepw_gemm");
  LRN_HIP(c, hipGetLastError());
  b.have_W = true;
  b.have_G = false;
  b.nt_free = true;
  c->scal_version += 1;
  *converged = true;
  return LRN_OK;
}

}  // namespace lrn

using namespace lrn;

extern "C" int lrn_prepare_w(lrn_ctx* c, int il, const double* X, const double* S, double* D, double* G,
                             double* Gi, double* W, double* Si, double* DDsi, int* info) {
  if (!c || il < 0 || il >= c->nlmi || !X || !S || !info) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  LmiBlock& b = c->lmi[il];
  const size_t mm = (size_t)b.msz * b.msz * 8, mv = (size_t)b.msz * 8;
  LRN_TRY(copy_in(c, b.X.p, X, mm));
  LRN_TRY(copy_in(c, b.S.p, S, mm));
  PhaseTimer timer(c, c->profile);
  LRN_TRY(prepare_w_block(c, b, info));
  timer.stop("prepare_w");
  if (*info != 0) return LRN_OK;
  if (D) LRN_TRY(copy_out(c, D, b.D.p, mv));
  if (G) LRN_TRY(copy_out(c, G, b.G.p, mm));
  if (Gi) LRN_TRY(copy_out(c, Gi, b.Gi.p, mm));
  if (W) LRN_TRY(copy_out(c, W, b.W.p, mm));
  if (Si) LRN_TRY(copy_out(c, Si, b.Si.p, mm));
  if (DDsi) LRN_TRY(copy_out(c, DDsi, b.DDsi.p, mv));
  return LRN_OK;
}
