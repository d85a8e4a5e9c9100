// The Lyapunov solve of the eigen-free NT scaling: the second-order term of the corrector without eigenvectors
// (ipstep.hip::second_order_eigenfree is the caller; the derivation is over prepw.hip::prepare_w_ns).
//
// R with Yh R + R Yh = Cm (Yh symmetric positive definite, Cm symmetric) by conjugate gradients in the Frobenius inner
// product: one product Yh p per step (the other half of the operator is its transpose), all scalars stay on the device,
// the host reads the residual history once per batch of steps.  Cm is used as the residual and destroyed.
//
// Round 4 -- the SAME solution from a better conditioned equation (option lyap_form = 1, default).  Zh = Yh^-1 is at hand
// (the coupled Newton-Schulz iteration produces both), and multiplying  Yh R + R Yh = C  by Zh from both sides gives
// Zh R + R Zh = Zh C Zh.  Any positive combination is again a Lyapunov equation for the same R:
//     M R + R M = C / s + s Zh C Zh,      M = Yh / s + s Zh,
// whose coefficient has the spectrum y / s + s / y: with s^2 = tr(Yh) / tr(Zh) (inside [y_min^2, y_max^2], free) its
// condition number is ~ sqrt(cond(Yh)) / 2 and never above cond(Yh) / 2.  Still one product per CG step, two more for the
// right-hand side; NumPy on spectra of cond(K) 1e2 / 1e3 / 1e4: 42 / 77 / 137 steps -> 14 / 21 / 29, same accuracy
// (C5: 32-48 steps of a 10^4-cube product each, 1.1-1.6 s of a 2.8 s iteration).
#include <algorithm>
#include <cmath>
#include <vector>

#include "ops.h"
#include "reduce.h"

namespace lrn {

// alpha = rr_k / <p, Ap> (every workgroup sums the same partials in the same order); R += alpha p; r -= alpha Ap;
// part2[block] = sum r^2
__global__ __launch_bounds__(256) void lyap_xr_kernel(const double* __restrict__ part1, int np1, const double* __restrict__ hist,
                                                      int k, const double* __restrict__ p, const double* __restrict__ Ap,
                                                      double* __restrict__ R, double* __restrict__ r, long total,
                                                      double* __restrict__ part2) {
  __shared__ double sh[4];
  const double pAp = block_sum_parts(part1, np1, sh);
  const double rr = hist[k];
  const double alpha = (pAp > 0.0 && rr > 0.0) ? rr / pAp : 0.0;
  double s = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    R[e] += alpha * p[e];
    const double v = r[e] - alpha * Ap[e];
    r[e] = v;
    s += v * v;
  }
  s = wg_sum<4>(s, sh);
  if (threadIdx.x == 0) part2[blockIdx.x] = s;
}

// beta = rr_{k+1} / rr_k; p = r + beta p; hist[k+1] = rr_{k+1}
__global__ __launch_bounds__(256) void lyap_p_kernel(const double* __restrict__ part2, int np2, double* __restrict__ hist, int k,
                                                     const double* __restrict__ r, double* __restrict__ p, long total) {
  __shared__ double sh[4];
  const double rn = block_sum_parts(part2, np2, sh);
  const double rr = hist[k];
  const double beta = rr > 0.0 ? rn / rr : 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) p[e] = r[e] + beta * p[e];
  if (blockIdx.x == 0 && threadIdx.x == 0) hist[k + 1] = rn;
}

// sc[0] = s = sqrt(tr(Y) / tr(Z)), sc[1] = 1 / s
__global__ __launch_bounds__(256) void lyap_trace2_kernel(const double* __restrict__ Y, const double* __restrict__ Z, int n,
                                                          double* __restrict__ sc) {
  __shared__ double sh[4];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { a += Y[(size_t)i * n + i]; b += Z[(size_t)i * n + i]; }
  const double ty = wg_sum<4>(a, sh), tz = wg_sum<4>(b, sh);
  if (threadIdx.x == 0) {
    double s = (ty > 0.0 && tz > 0.0) ? sqrt(ty / tz) : 1.0;
    if (!(s > 0.0) || isinf(s)) s = 1.0;
    sc[0] = s;
    sc[1] = 1.0 / s;
  }
}

// M = Y / s + s Z
__global__ void lyap_mop_kernel(const double* __restrict__ Y, const double* __restrict__ Z, const double* __restrict__ sc,
                                long total, double* __restrict__ Mop) {
  const double s = sc[0], si = sc[1];
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
    Mop[e] = Y[e] * si + s * Z[e];
}

// C <- C / s + s (T + T') / 2   (T = Zh C Zh up to rounding asymmetry), by 32 x 32 tiles as symadd_kernel
__global__ __launch_bounds__(256) void lyap_rhs_kernel(double* __restrict__ Cm, const double* __restrict__ T, int n,
                                                       const double* __restrict__ sc) {
  __shared__ double ta[32][33], tb[32][33];
  const double s = sc[0], si = sc[1];
  const int nt = (n + 31) / 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (long t = blockIdx.x; t < (long)nt * nt; t += gridDim.x) {
    const int bi = (int)(t % nt) * 32, bj = (int)(t / nt) * 32;
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int i = bi + tx, j = bj + r;
      ta[r][tx] = (i < n && j < n) ? T[(long)i + (long)j * n] : 0.0;
      const int i2 = bj + tx, j2 = bi + r;
      tb[r][tx] = (i2 < n && j2 < n) ? T[(long)i2 + (long)j2 * n] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int i = bi + tx, j = bj + r;
      if (i < n && j < n) {
        const long e = (long)i + (long)j * n;
        Cm[e] = Cm[e] * si + s * 0.5 * (ta[r][tx] + tb[tx][r]);
      }
    }
  }
}

// b.lyap: search direction, operator image, the partial sums of the two dots, the residual history, the combined operator
struct LyapWork {
  double *p, *Ap, *part1, *part2, *hist, *Mop;
  int np;                 // workgroups of the element-wise kernels = partial sums of ||r||^2
};

// the combined form: s from the traces, Mop = Yh / s + s Zh, Cm <- Cm / s + s Zh Cm Zh
static int lyap_combined_setup(lrn_ctx* c, LmiBlock& b, const LyapWork& w, double* Cm, double* work) {
  const int n = b.msz;
  const long nn = (long)n * n;
  hipStream_t st = c->stream;
  const double *Yh = b.Yh.as<double>(), *Zh = b.Zh.as<double>();
  double* sc = w.part2;                               // (two doubles, free until the first lyap_xr_kernel)
  hipLaunchKernelGGL(lyap_trace2_kernel, dim3(1), dim3(256), 0, st, Yh, Zh, n, sc);
  hipLaunchKernelGGL(lyap_mop_kernel, dim3(w.np), dim3(256), 0, st, Yh, Zh, sc, nn, w.Mop);
  LRN_TRY(pgemm_nt(c, st, n, Zh, Cm, work));          // Zh C   (C symmetric)
  LRN_TRY(pgemm_nt(c, st, n, work, Zh, w.Ap));        // Zh C Zh
  hipLaunchKernelGGL(lyap_rhs_kernel, dim3(sym_grid(n)), dim3(256), 0, st, Cm, w.Ap, n, sc);
  return LRN_OK;
}

// CG step k, queued: Ap = Cop p + (Cop p)' with <p, Ap>, then R, r, then p; hist[k + 1] = ||r||^2
static int lyap_cg_step(lrn_ctx* c, int n, const double* Cop, const LyapWork& w, double* R, double* r, double* work, int k) {
  const long nn = (long)n * n;
  hipStream_t st = c->stream;
  const int np1 = (int)sym_grid(n);
  SlabSrc prod;                                       // (mid sizes: the slabs of the product are added by symadd_kernel)
  LRN_TRY(prod_slabs(c, st, n, Cop, w.p, work, 1.0, 0, &prod));
  symadd(st, np1, prod, n, 1.0, w.Ap, w.p, w.part1);
  hipLaunchKernelGGL(lyap_xr_kernel, dim3(w.np), dim3(256), 0, st, w.part1, np1, w.hist, k, w.p, w.Ap, R, r, nn, w.part2);
  hipLaunchKernelGGL(lyap_p_kernel, dim3(w.np), dim3(256), 0, st, w.part2, w.np, w.hist, k, r, w.p, nn);
  return LRN_OK;
}

// How many steps to queue before the next look at the residual history h[0 .. k] (||r||^2 per step): as many as the rate of
// the last two promises (CG only gets faster) -- a step is one n^3 product (31 ms at msz 10^4: none to waste), a look is a
// host round trip (20 us: too many at 800)
static int lyap_next_batch(int n, const std::vector<double>& h, int k, double tol2) {
  int batch = n >= 2000 ? 2 : 4;
  if (k >= 2 && h[k] > 0.0 && h[k] < h[k - 2]) {
    const double f = 0.5 * std::log(h[k - 2] / h[k]);             // decrement of log ||r||^2 per step
    const double m = std::log(h[k] / (tol2 * h[0])) / f;
    const int lo_b = n >= 2000 ? 1 : 2;
    batch = std::max(lo_b, std::min(8, (int)std::floor(0.9 * m + 0.5)));
  }
  return batch;
}

int lyap_solve(lrn_ctx* c, LmiBlock& b, double* Cm, double* R, double* work, bool* ok, int* steps) {
  const int n = b.msz;
  const long nn = (long)n * n;
  hipStream_t st = c->stream;
  const int maxit = std::max(2, c->opt.lyap_maxit);
  const bool combined = c->opt.lyap_form != 0;
  LRN_TRY(ensure(c, b.lyap, ((size_t)(combined ? 3 : 2) * nn + 2 * 1024 + maxit + 16) * 8));
  double* q = b.lyap.as<double>();
  const LyapWork w{q, q + nn, q + 2 * nn, q + 2 * nn + 1024, q + 2 * nn + 2048, q + 2 * nn + 2048 + maxit + 16, dot_parts_count(nn)};
  double* r = Cm;
  const double* Cop = b.Yh.as<double>();             // coefficient matrix of the equation that is iterated on
  if (combined) {
    LRN_TRY(lyap_combined_setup(c, b, w, Cm, work));
    Cop = w.Mop;
  }
  LRN_HIP(c, hipMemsetAsync(R, 0, (size_t)nn * 8, st));
  LRN_HIP(c, hipMemcpyAsync(w.p, r, (size_t)nn * 8, hipMemcpyDeviceToDevice, st));
  dot_via(st, r, nullptr, nn, w.part1, w.hist);
  std::vector<double> h(maxit + 1, 0.0);
  const double tol2 = c->opt.lyap_tol * c->opt.lyap_tol;
  int k = 0;
  *ok = false;
  int batch = std::min(maxit, n >= 2000 ? 6 : 8);      // first look at the residual history
  while (k < maxit) {
    for (const int k1 = std::min(maxit, k + batch); k < k1; ++k) LRN_TRY(lyap_cg_step(c, n, Cop, w, R, r, work, k));
    LRN_HIP(c, hipMemcpyAsync(h.data(), w.hist, (size_t)(k + 1) * 8, hipMemcpyDeviceToHost, st));
    LRN_HIP(c, hipStreamSynchronize(st));
    if (!(h[k] == h[k])) break;                                   // NaN
    if (h[0] == 0.0 || h[k] <= tol2 * h[0]) { *ok = true; break; }
    batch = lyap_next_batch(n, h, k, tol2);
  }
  if (steps) *steps = k;
  return LRN_OK;
}

}  // namespace lrn
