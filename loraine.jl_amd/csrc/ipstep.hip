// Device-resident interior-point step: everything of the reference's per-iteration host work
// that touches msz x msz matrices:
//   residual Rd, right-hand sides (makeRHS, corrector my_kron term), find_step with its two
//   extreme-eigenvalue problems per block, the predictor point / RNT, the iterate update and
//   the matrix parts of find_mu / check_convergence.
// Reference: src/predictor_corrector.jl:8-16,186,248-326 ; src/Solvers.jl:480-511 ;
// src/kron_etc.jl.  nvar-/nlin-vectors and scalars stay with the host driver.
//
// eigmin (predictor_corrector.jl:272,285; Solvers.jl:503,505) is a Lanczos iteration on the
// device (lz.hip); this file holds its callers.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/loraine_hip.h"
#include "ops.h"

namespace lrn {

// out = a*A + b*B + c*C (null pointers skipped), n elements
__global__ void lin3_kernel(double* __restrict__ out, double a, const double* __restrict__ A, double b,
                            const double* __restrict__ B, double c, const double* __restrict__ C, long n) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    double v = 0.0;
    if (A) v += a * A[e];
    if (B) v += b * B[e];
    if (C) v += c * C[e];
    out[e] = v;
  }
}

// out = (M + M')/2 (out may alias M only through the symmetric access pattern -> use a separate out)
__global__ void sym_kernel(const double* __restrict__ M, double* __restrict__ out, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    out[e] = 0.5 * (M[e] + M[(long)j + (long)i * n]);
  }
}

// Q = sym( dd_j * M[i,j] * dd_i )   (predictor_corrector.jl:268-269)
__global__ void scale_sym_kernel(const double* __restrict__ M, const double* __restrict__ dd, double* __restrict__ out, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    out[e] = 0.5 * dd[i] * dd[j] * (M[e] + M[(long)j + (long)i * n]);
  }
}

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

__global__ void add_diag_mat_kernel(double* __restrict__ M, int n, double eps) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) M[(long)i * n + i] += eps;
}
void add_diag_mat(hipStream_t st, double* M, int n, double eps) {
  hipLaunchKernelGGL(add_diag_mat_kernel, dim3((n + 255) / 256), dim3(256), 0, st, M, n, eps);
}

// two-stage reductions: partial[b] = sum A.*B (B may be null -> A.*A)
__global__ __launch_bounds__(256) void dot_part_kernel(const double* __restrict__ A, const double* __restrict__ B, long n,
                                                       double* __restrict__ part) {
  __shared__ double sh[4];
  double s = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) s += A[e] * (B ? B[e] : A[e]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ __launch_bounds__(256) void dot_final_kernel(const double* __restrict__ part, int np, double* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int e = threadIdx.x; e < np; e += 256) s += part[e];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = sh[0] + sh[1] + sh[2] + sh[3];
}

static int dot_dev(lrn_ctx* c, const double* A, const double* B, long n, double* out_dev) {
  const int np = (int)std::min<long>(1024, (n + 255) / 256);
  LRN_TRY(ensure(c, c->redbuf, (size_t)(np + 64) * 8));
  hipLaunchKernelGGL(dot_part_kernel, dim3(np), dim3(256), 0, c->stream, A, B, n, c->redbuf.as<double>());
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(256), 0, c->stream, c->redbuf.as<double>(), np, out_dev);
  return LRN_OK;
}

// ------------------------------------------------------------------ Lyapunov solve (eigen-free NT scaling)
// out = scale (T + T') by 32 x 32 tiles (both reads coalesced); with `dotp`: part[block] = sum dotp .* out over the block's
// tiles.  out is exactly symmetric: (i,j) and (j,i) add the same two numbers.
__global__ __launch_bounds__(256) void symadd_kernel(SlabSrc T, int n, double scale, double* __restrict__ out,
                                                     const double* __restrict__ dotp, double* __restrict__ part) {
  __shared__ double ta[32][33], tb[32][33];
  __shared__ double sh[4];
  const int nt = (n + 31) / 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
  double acc = 0.0;
  for (long t = blockIdx.x; t < (long)nt * nt; t += gridDim.x) {
    const int bi = (int)(t % nt) * 32, bj = (int)(t / nt) * 32;
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int i = bi + tx, j = bj + r;       // tile (bi, bj): element (i, j)
      ta[r][tx] = (i < n && j < n) ? slab_sum(T, (long)i + (long)j * n) : 0.0;
      const int i2 = bj + tx, j2 = bi + r;     // tile (bj, bi): element (i2, j2)
      tb[r][tx] = (i2 < n && j2 < n) ? slab_sum(T, (long)i2 + (long)j2 * n) : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int i = bi + tx, j = bj + r;
      if (i < n && j < n) {
        const double v = scale * (ta[r][tx] + tb[tx][r]);      // T[i,j] + T[j,i]
        out[(long)i + (long)j * n] = v;
        if (dotp) acc += dotp[(long)i + (long)j * n] * v;
      }
    }
  }
  if (!part) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

void symadd(hipStream_t st, unsigned grid, const SlabSrc& T, int n, double scale, double* out, const double* dotp, double* part) {
  hipLaunchKernelGGL(symadd_kernel, dim3(grid), dim3(256), 0, st, T, n, scale, out, dotp, part);
}

__device__ __forceinline__ double block_sum_parts(const double* __restrict__ part, int np, double* sh) {
  double s = 0.0;
  for (int e = threadIdx.x; e < np; e += 256) s += part[e];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// out = (M + M') / 2: the tiled kernel above from msz 512 on (the element-wise one reads M' with stride n)
static void sym_half(hipStream_t st, const double* M, double* out, int n) {
  if (n >= 512) {
    const long nt = (n + 31) / 32;
    hipLaunchKernelGGL(symadd_kernel, dim3((unsigned)std::min<long>(1024, nt * nt)), dim3(256), 0, st, SlabSrc{M, 0, 1}, n, 0.5, out,
                       (const double*)nullptr, (double*)nullptr);
  } else {
    hipLaunchKernelGGL(sym_kernel, dim3(nb((long)n * n)), dim3(256), 0, st, M, out, n);
  }
}

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
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part2[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
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
__global__ __launch_bounds__(256) void lyap_trace2_kernel(const double* __restrict__ Y, const double* __restrict__ Z, int n,
                                                          double* __restrict__ sc) {
  __shared__ double sh[8];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { a += Y[(size_t)i * n + i]; b += Z[(size_t)i * n + i]; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = a; sh[4 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double ty = sh[0] + sh[1] + sh[2] + sh[3], tz = sh[4] + sh[5] + sh[6] + sh[7];
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

static int lyap_solve(lrn_ctx* c, LmiBlock& b, double* Cm, double* R, double* work, bool* ok, int* steps) {
  const int n = b.msz;
  const long nn = (long)n * n;
  hipStream_t st = c->stream;
  const int maxit = std::max(2, c->opt.lyap_maxit);
  const int np = (int)std::min<long>(1024, (nn + 255) / 256);
  const bool combined = c->opt.lyap_form != 0;
  LRN_TRY(ensure(c, b.lyap, ((size_t)(combined ? 3 : 2) * nn + 2 * 1024 + maxit + 16) * 8));
  double* p = b.lyap.as<double>();
  double* Ap = p + nn;
  double* part1 = Ap + nn;
  double* part2 = part1 + 1024;
  double* hist = part2 + 1024;
  double* Mop = hist + maxit + 16;
  double* r = Cm;
  const double* Cop = b.Yh.as<double>();             // coefficient matrix of the equation that is iterated on
  const int ntile0 = (n + 31) / 32;
  if (combined) {
    double* sc = part2;                               // (two doubles, free until the first lyap_xr_kernel)
    hipLaunchKernelGGL(lyap_trace2_kernel, dim3(1), dim3(256), 0, st, b.Yh.as<double>(), b.Zh.as<double>(), n, sc);
    hipLaunchKernelGGL(lyap_mop_kernel, dim3(np), dim3(256), 0, st, b.Yh.as<double>(), b.Zh.as<double>(), sc, nn, Mop);
    LRN_TRY(pgemm_nt(c, st, n, b.Zh.as<double>(), Cm, work));                 // Zh C   (C symmetric)
    LRN_TRY(pgemm_nt(c, st, n, work, b.Zh.as<double>(), Ap));                 // Zh C Zh
    hipLaunchKernelGGL(lyap_rhs_kernel, dim3((unsigned)std::min<long>(1024, (long)ntile0 * ntile0)), dim3(256), 0, st, Cm, Ap, n, sc);
    Cop = Mop;
  }
  LRN_HIP(c, hipMemsetAsync(R, 0, (size_t)nn * 8, st));
  LRN_HIP(c, hipMemcpyAsync(p, r, (size_t)nn * 8, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(dot_part_kernel, dim3(np), dim3(256), 0, st, r, (const double*)nullptr, nn, part1);
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(256), 0, st, part1, np, hist);
  std::vector<double> h(maxit + 1, 0.0);
  const double tol2 = c->opt.lyap_tol * c->opt.lyap_tol;
  int k = 0;
  *ok = false;
  const int ntile = (n + 31) / 32;
  const int np1 = (int)std::min<long>(1024, (long)ntile * ntile);
  int batch = std::min(maxit, n >= 2000 ? 6 : 8);      // first look at the residual history
  while (k < maxit) {
    const int k1 = std::min(maxit, k + batch);
    for (; k < k1; ++k) {
      SlabSrc prod;                                  // (mid sizes: the slabs of the product are added by symadd_kernel)
      LRN_TRY(prod_slabs(c, st, n, Cop, p, work, 1.0, 0, &prod));
      hipLaunchKernelGGL(symadd_kernel, dim3(np1), dim3(256), 0, st, prod, n, 1.0, Ap, p, part1);
      hipLaunchKernelGGL(lyap_xr_kernel, dim3(np), dim3(256), 0, st, part1, np1, hist, k, p, Ap, R, r, nn, part2);
      hipLaunchKernelGGL(lyap_p_kernel, dim3(np), dim3(256), 0, st, part2, np, hist, k, r, p, nn);
    }
    LRN_HIP(c, hipMemcpyAsync(h.data(), hist, (size_t)(k + 1) * 8, hipMemcpyDeviceToHost, st));
    LRN_HIP(c, hipStreamSynchronize(st));
    if (!(h[k] == h[k])) break;                                   // NaN
    if (h[0] == 0.0 || h[k] <= tol2 * h[0]) { *ok = true; break; }
    // how many more steps at the rate of the last two (CG only gets faster): queue that many before the next look --
    // a step is one n^3 product (31 ms at msz 10^4: none to waste), a look is a host round trip (20 us: too many at 800)
    batch = n >= 2000 ? 2 : 4;
    if (k >= 2 && h[k] > 0.0 && h[k] < h[k - 2]) {
      const double f = 0.5 * std::log(h[k - 2] / h[k]);           // decrement of log ||r||^2 per step
      const double m = std::log(h[k] / (tol2 * h[0])) / f;
      const int lo_b = n >= 2000 ? 1 : 2;
      batch = std::max(lo_b, std::min(8, (int)std::floor(0.9 * m + 0.5)));
    }
  }
  if (steps) *steps = k;
  return LRN_OK;
}

// ------------------------------------------------------------------ resident step
static int ensure_resident(lrn_ctx* c, LmiBlock& b) {
  size_t mm_ = (size_t)b.msz * b.msz * 8;
  for (DBuf* d : {&b.Cd, &b.Rd, &b.delX, &b.delS, &b.Xn, &b.Sn, &b.RNT, &b.t0, &b.t1, &b.t2})
    if (d->bytes < mm_) LRN_TRY(ensure(c, *d, mm_, true));
  b.resident = true;
  return LRN_OK;
}

}  // namespace lrn

using namespace lrn;

#define BLK(il)                                                        \
  if (!c || (il) < 0 || (il) >= c->nlmi) return LRN_ERR_ARG;          \
  LRN_HIP(c, hipSetDevice(c->device));                                 \
  LmiBlock& b = c->lmi[(il)];                                          \
  LRN_TRY(ensure_resident(c, b));                                      \
  const size_t mm_ = (size_t)b.msz * b.msz * 8;                        \
  (void)mm_;

extern "C" int lrn_ip_set_c(lrn_ctx* c, int il, const double* C) {
  BLK(il);
  if (!C) return LRN_ERR_ARG;
  return copy_in(c, b.Cd.p, C, mm_);
}

extern "C" int lrn_ip_set_iterate(lrn_ctx* c, int il, const double* X, const double* S) {
  BLK(il);
  if (!X || !S) return LRN_ERR_ARG;
  LRN_TRY(copy_in(c, b.X.p, X, mm_));
  LRN_TRY(copy_in(c, b.S.p, S, mm_));
  LRN_HIP(c, hipMemsetAsync(b.RNT.p, 0, mm_, c->stream));
  b.have_Vprev = false;
  b.chol_valid = false;
  return LRN_OK;
}

extern "C" int lrn_ip_get_iterate(lrn_ctx* c, int il, double* X, double* S) {
  BLK(il);
  if (X) LRN_TRY(copy_out(c, X, b.X.p, mm_));
  if (S) LRN_TRY(copy_out(c, S, b.S.p, mm_));
  return LRN_OK;
}

extern "C" int lrn_ip_add_diag(lrn_ctx* c, int il, int which, double eps) {
  BLK(il);
  if (which != 1 && which != 2) return LRN_ERR_ARG;
  b.chol_valid = false;
  add_diag_mat(c->stream, (which == 1 ? b.X : b.S).as<double>(), b.msz, eps);
  return LRN_OK;
}

extern "C" int lrn_ip_prepare_w(lrn_ctx* c, int il, int* info) {
  BLK(il);
  if (!info) return LRN_ERR_ARG;
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
    LRN_TRY(ensure_resident(c, b));
    const long mm_ = (long)b.msz * b.msz;
    LRN_TRY(aat_to_mat(c, b, c->v0.as<double>(), b.t0.as<double>()));
    hipLaunchKernelGGL(lin3_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.Rd.as<double>(), 1.0, b.Cd.as<double>(),
                       -1.0, b.S.as<double>(), -1.0, b.t0.as<double>(), mm_);
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
    LRN_TRY(ensure_resident(c, b));
    const long mm_ = (long)b.msz * b.msz;
    hipLaunchKernelGGL(lin3_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.t0.as<double>(), 1.0, b.Rd.as<double>(),
                       1.0, b.S.as<double>(), 0.0, (const double*)nullptr, mm_);
    LRN_TRY(wmw(c, b, b.t0.as<double>(), b.t1.as<double>(), b.t2.as<double>()));
    LRN_TRY(aa_times(c, b, b.t2.as<double>(), c->v1.as<double>()));
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
    LRN_TRY(ensure_resident(c, b));
    const long mm_ = (long)b.msz * b.msz;
    hipLaunchKernelGGL(lin3_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.t0.as<double>(), 1.0, b.Rd.as<double>(),
                       1.0, b.S.as<double>(), 0.0, (const double*)nullptr, mm_);
    if (wmw_pattern_ok(c, b)) {          // every constraint sparse: W M W only where AA reads it (one product instead of two)
      LRN_TRY(aa_times(c, b, b.X.as<double>(), c->v2.as<double>()));
      LRN_TRY(aa_times_wmw_pattern(c, b, b.t0.as<double>(), b.t1.as<double>(), c->v1.as<double>()));
      continue;
    }
    LRN_TRY(wmw(c, b, b.t0.as<double>(), b.t1.as<double>(), b.t2.as<double>()));
    LRN_TRY(aa_times2(c, b, b.X.as<double>(), c->v2.as<double>(), b.t2.as<double>(), c->v1.as<double>()));
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
    LRN_TRY(ensure_resident(c, b));
    const int m = b.msz;
    const long mm_ = (long)m * m;
    if (b.nt_free) {
      // G (G'RdG + D - sigma_mu/D - RNT) G' = W Rd W + X - sigma_mu Si - G RNT G'
      if (wmw_pattern_ok(c, b)) {        // AA vec(W Rd W) on the pattern, AA vec(X - sigma_mu Si - G RNT G') by itself
        LRN_TRY(aa_times_wmw_pattern(c, b, b.Rd.as<double>(), b.t1.as<double>(), c->v1.as<double>()));
        hipLaunchKernelGGL(lin3_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.t0.as<double>(), 1.0, b.X.as<double>(), -sigma_mu,
                           b.Si.as<double>(), -1.0, b.Qm.as<double>(), mm_);
        LRN_TRY(aa_times(c, b, b.t0.as<double>(), c->v1.as<double>()));
        continue;
      }
      LRN_TRY(wmw(c, b, b.Rd.as<double>(), b.t1.as<double>(), b.t2.as<double>()));
      hipLaunchKernelGGL(lin3_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.t0.as<double>(), 1.0, b.t2.as<double>(), 1.0,
                         b.X.as<double>(), -sigma_mu, b.Si.as<double>(), mm_);
      hipLaunchKernelGGL(lin3_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.t2.as<double>(), 1.0, b.t0.as<double>(), -1.0,
                         b.Qm.as<double>(), 0.0, (const double*)nullptr, mm_);
      LRN_TRY(aa_times(c, b, b.t2.as<double>(), c->v1.as<double>()));
      continue;
    }
    double* G = b.G.as<double>();
    // t1 = G' Rd G
    LRN_TRY(gemm_nn(c->stream, m, G, true, b.Rd.as<double>(), false, b.t0.as<double>()));
    LRN_TRY(gemm_nn(c->stream, m, b.t0.as<double>(), false, G, false, b.t1.as<double>()));
    hipLaunchKernelGGL(corr_inner_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.t1.as<double>(), b.D.as<double>(),
                       b.RNT.as<double>(), sigma_mu, b.t0.as<double>(), m);
    // my_kron(G,G,inner) = vec(G inner G')
    LRN_TRY(gemm_nn(c->stream, m, G, false, b.t0.as<double>(), false, b.t1.as<double>()));
    LRN_TRY(gemm_nn(c->stream, m, b.t1.as<double>(), false, G, true, b.t2.as<double>()));
    LRN_TRY(aa_times(c, b, b.t2.as<double>(), c->v1.as<double>()));
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
    LRN_TRY(ensure_resident(c, b));
    const int m = b.msz;
    const long mm_ = (long)m * m;
    const unsigned g = nb(mm_);
    double *t0 = b.t0.as<double>(), *t1 = b.t1.as<double>(), *t2 = b.t2.as<double>();
    double *G = b.G.as<double>(), *Gi = b.Gi.as<double>();
    // delS = Rd - mat(AA' dely)                                   (:252)
    LRN_TRY(aat_to_mat(c, b, c->v0.as<double>(), t0));
    hipLaunchKernelGGL(lin3_kernel, dim3(g), dim3(256), 0, c->stream, b.delS.as<double>(), 1.0, b.Rd.as<double>(), -1.0, t0,
                       0.0, (const double*)nullptr, mm_);
    double lamX = 0.0, lamS = 0.0;
    double* t3 = b.Xn.as<double>();          // free here: Xn / Sn are rebuilt by lrn_ip_update after the step lengths
    if (b.nt_free) {
      // everything in the L_X basis (prepw.hip::prepare_w_ns): Bs = L_X' dS L_X, T = Z Bs Z / c,
      // TX = L_X^-1 dX L_X^-T = -I - T (+ sigma_mu K^-1 + R), dX = L_X TX L_X'                  (:253-257)
      const unsigned gs = (unsigned)std::min<long>(1024, ((long)(m + 31) / 32) * ((m + 31) / 32));
      LRN_TRY(pgemm_nt(c, c->stream, m, b.LXt.as<double>(), b.delS.as<double>(), t0, GEMM_KFROM_M));    // L_X' upper triangular
      // (both second products are symmetric in exact arithmetic: from msz 1500 on the lower tiles + mirror, half the work;
      // below, the full product and the average of the two triangles)
      if (m >= BIG_TILE_MIN_N) {
        LRN_TRY(pgemm_nt_sym(c, c->stream, m, t0, b.LXt.as<double>(), b.Bs.as<double>(), 1.0, GEMM_KFROM_N));
      } else {
        SlabSrc prod;
        LRN_TRY(prod_slabs(c, c->stream, m, t0, b.LXt.as<double>(), t1, 1.0, GEMM_KFROM_N, &prod));
        hipLaunchKernelGGL(symadd_kernel, dim3(gs), dim3(256), 0, c->stream, prod, m, 0.5, b.Bs.as<double>(), (const double*)nullptr,
                           (double*)nullptr);
      }
      LRN_TRY(pgemm_nt(c, c->stream, m, b.Zh.as<double>(), b.Bs.as<double>(), t0));
      if (m >= BIG_TILE_MIN_N) {
        LRN_TRY(pgemm_nt_sym(c, c->stream, m, t0, b.Zh.as<double>(), t3, 1.0 / b.ns_c));
      } else {
        SlabSrc prod;
        LRN_TRY(prod_slabs(c, c->stream, m, t0, b.Zh.as<double>(), t1, 1.0 / b.ns_c, 0, &prod));
        hipLaunchKernelGGL(symadd_kernel, dim3(gs), dim3(256), 0, c->stream, prod, m, 0.5, t3, (const double*)nullptr, (double*)nullptr);
      }
      hipLaunchKernelGGL(tx_kernel, dim3(g), dim3(256), 0, c->stream, t3, sigma_mu / b.ns_c, b.Ki.as<double>(),
                         predict ? (const double*)nullptr : b.RNT.as<double>(), b.TX.as<double>(), m);
      LRN_TRY(pgemm_nt(c, c->stream, m, b.LXf.as<double>(), b.TX.as<double>(), t0, GEMM_KTO_M));        // L_X lower triangular
      LRN_TRY(pgemm_nt_sym(c, c->stream, m, t0, b.LXf.as<double>(), b.delX.as<double>(), 1.0, GEMM_KTO_N));
      // the scaled directions of the step-length rule are orthogonally similar to TX and T               (:263-285)
      LRN_TRY(eigmin_certified_pair(c, b.TX.as<double>(), t3, m, &lamX, &lamS));
      alpha[il] = lamX > -1e-6 ? 0.99 : std::min(1.0, -tau / lamX);
      beta[il] = lamS > -1e-6 ? 0.99 : std::min(1.0, -tau / lamS);
      continue;
    }
    // t2 = W delS W                                                (:253)
    LRN_TRY(wmw(c, b, b.delS.as<double>(), t1, t2));
    if (predict) {
      // delX = mat(-X - W delS W)                                  (:255)
      hipLaunchKernelGGL(lin3_kernel, dim3(g), dim3(256), 0, c->stream, t0, -1.0, b.X.as<double>(), -1.0, t2, 0.0,
                         (const double*)nullptr, mm_);
    } else {
      // delX = mat(sigma_mu Si - X - W delS W + G RNT G')          (:257)
      hipLaunchKernelGGL(lin3_kernel, dim3(g), dim3(256), 0, c->stream, t0, sigma_mu, b.Si.as<double>(), -1.0,
                         b.X.as<double>(), -1.0, t2, mm_);
      LRN_TRY(gemm_nn(c->stream, m, G, false, b.RNT.as<double>(), false, t1));
      LRN_TRY(gemm_nn(c->stream, m, t1, false, G, true, t2));
      hipLaunchKernelGGL(lin3_kernel, dim3(g), dim3(256), 0, c->stream, t0, 1.0, t0, 1.0, t2, 0.0, (const double*)nullptr, mm_);
    }
    sym_half(c->stream, t0, b.delX.as<double>(), m);
    // step lengths: eigmin of DDsi-scaled G' delS G and Gi delX Gi'   (:263-291)
    LRN_TRY(gemm_nn(c->stream, m, Gi, false, b.delX.as<double>(), false, t0));
    LRN_TRY(gemm_nn(c->stream, m, t0, false, Gi, true, t1));
    hipLaunchKernelGGL(scale_sym_kernel, dim3(g), dim3(256), 0, c->stream, t1, b.DDsi.as<double>(), t2, m);
    LRN_TRY(gemm_nn(c->stream, m, G, true, b.delS.as<double>(), false, t0));
    LRN_TRY(gemm_nn(c->stream, m, t0, false, G, false, t1));
    hipLaunchKernelGGL(scale_sym_kernel, dim3(g), dim3(256), 0, c->stream, t1, b.DDsi.as<double>(), t3, m);
    LRN_TRY(eigmin_certified_pair(c, t2, t3, m, &lamX, &lamS));
    alpha[il] = lamX > -1e-6 ? 0.99 : std::min(1.0, -tau / lamX);
    beta[il] = lamS > -1e-6 ? 0.99 : std::min(1.0, -tau / lamS);
  }
  timer.stop("find_step");
  return LRN_OK;
}

extern "C" int lrn_ip_update(lrn_ctx* c, int predict, const double* alpha, const double* beta, double* trXnSn) {
  if (!c || !alpha || !beta) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  std::vector<double> tr(c->nlmi, 0.0);
  LRN_TRY(ensure(c, c->redout, 64 * 8));
  for (int il = 0; il < c->nlmi; ++il) {
    LmiBlock& b = c->lmi[il];
    LRN_TRY(ensure_resident(c, b));
    const int m = b.msz;
    const long mm_ = (long)m * m;
    const unsigned g = nb(mm_);
    double *t0 = b.t0.as<double>(), *t1 = b.t1.as<double>(), *t2 = b.t2.as<double>();
    if (predict) {
      hipLaunchKernelGGL(lin3_kernel, dim3(g), dim3(256), 0, c->stream, b.Xn.as<double>(), 1.0, b.X.as<double>(), alpha[il],
                         b.delX.as<double>(), 0.0, (const double*)nullptr, mm_);
      hipLaunchKernelGGL(lin3_kernel, dim3(g), dim3(256), 0, c->stream, b.Sn.as<double>(), 1.0, b.S.as<double>(), beta[il],
                         b.delS.as<double>(), 0.0, (const double*)nullptr, mm_);
      LRN_TRY(dot_dev(c, b.Xn.as<double>(), b.Sn.as<double>(), mm_, c->redout.as<double>() + il));
      if (b.nt_free) {
        // Qm = G RNT G' without the eigenvectors: N = L_X^-1 dX dS L_X = TX Bs, Yh R + R Yh = -(N Zh + Zh N') / c,
        // Qm = L_X R L_X'
        tic(c);
        LRN_TRY(pgemm_nt(c, c->stream, m, b.TX.as<double>(), b.Bs.as<double>(), t0));              // N
        SlabSrc prod;
        LRN_TRY(prod_slabs(c, c->stream, m, t0, b.Zh.as<double>(), t1, 1.0, 0, &prod));            // N Zh
        hipLaunchKernelGGL(symadd_kernel, dim3((unsigned)std::min<long>(1024, ((long)(m + 31) / 32) * ((m + 31) / 32))), dim3(256), 0,
                           c->stream, prod, m, -1.0 / b.ns_c, t2, (const double*)nullptr, (double*)nullptr);
        bool ok = false;
        int steps = 0;
        LRN_TRY(lyap_solve(c, b, t2, b.RNT.as<double>(), t0, &ok, &steps));
        c->counts["lyap_steps"] += steps;
        c->counts["lyap_solves"] += 1;
        if (ok) {
          LRN_TRY(pgemm_nt(c, c->stream, m, b.LXf.as<double>(), b.RNT.as<double>(), t0, GEMM_KTO_M));
          LRN_TRY(pgemm_nt_sym(c, c->stream, m, t0, b.LXf.as<double>(), b.Qm.as<double>(), 1.0, GEMM_KTO_N));
          toc(c, "lyap");
          continue;
        }
        // the Lyapunov iteration did not converge (K far from well conditioned): take the SVD for this iteration
        toc(c, "lyap");
        c->counts["lyap_fallback"] += 1;
        int info = 0;
        LRN_TRY(prepare_w_block(c, b, &info));
        if (info != 0) return set_error(c, LRN_ERR_STATE, "SVD fallback of the NT scaling failed (info %d)", info);
        b.nt_free = false;
      }
      // RNT = -(Gi delX delS G + its transpose) ./ (D_i + D_j)     (:308-309)
      LRN_TRY(gemm_nn(c->stream, m, b.Gi.as<double>(), false, b.delX.as<double>(), false, t0));
      LRN_TRY(gemm_nn(c->stream, m, t0, false, b.delS.as<double>(), false, t1));
      LRN_TRY(gemm_nn(c->stream, m, t1, false, b.G.as<double>(), false, t2));
      hipLaunchKernelGGL(rnt_kernel, dim3(g), dim3(256), 0, c->stream, t2, b.D.as<double>(), b.RNT.as<double>(), m);
    } else {
      b.chol_valid = false;
      hipLaunchKernelGGL(lin3_kernel, dim3(g), dim3(256), 0, c->stream, t0, 1.0, b.X.as<double>(), alpha[0],
                         b.delX.as<double>(), 0.0, (const double*)nullptr, mm_);
      sym_half(c->stream, t0, b.X.as<double>(), m);
      hipLaunchKernelGGL(lin3_kernel, dim3(g), dim3(256), 0, c->stream, t0, 1.0, b.S.as<double>(), beta[0],
                         b.delS.as<double>(), 0.0, (const double*)nullptr, mm_);
      sym_half(c->stream, t0, b.S.as<double>(), m);
    }
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
    LmiBlock& b = c->lmi[il];
    LRN_TRY(ensure_resident(c, b));
    const long mm_ = (long)b.msz * b.msz;
    double* o = c->redout.as<double>() + 5 * il;
    LRN_TRY(dot_dev(c, b.X.as<double>(), b.S.as<double>(), mm_, o + 0));
    LRN_TRY(dot_dev(c, b.Rd.as<double>(), nullptr, mm_, o + 3));
    LRN_TRY(dot_dev(c, b.Cd.as<double>(), b.X.as<double>(), mm_, o + 4));
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

extern "C" int lrn_dbg_get_block(lrn_ctx* c, int il, const char* name, double* out, int* flag) {
  if (!c || il < 0 || il >= c->nlmi || !name || !out) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  LmiBlock& b = c->lmi[il];
  const size_t mm_ = (size_t)b.msz * b.msz * 8, mv = (size_t)b.msz * 8;
  struct { const char* n; DBuf* d; size_t bytes; } tab[] = {
      {"W", &b.W, mm_}, {"Si", &b.Si, mm_}, {"G", &b.G, mm_}, {"Gi", &b.Gi, mm_}, {"D", &b.D, mv}, {"DDsi", &b.DDsi, mv},
      {"X", &b.X, mm_}, {"S", &b.S, mm_}, {"delX", &b.delX, mm_}, {"delS", &b.delS, mm_}, {"RNT", &b.RNT, mm_},
      {"LX", &b.LXf, mm_}, {"LS", &b.LSf, mm_}, {"Bs", &b.Bs, mm_}, {"TX", &b.TX, mm_}, {"Ki", &b.Ki, mm_}, {"Yh", &b.Yh, mm_},
      {"Zh", &b.Zh, mm_}, {"Qm", &b.Qm, mm_}, {"Rd", &b.Rd, mm_}};
  if (flag) *flag = b.nt_free ? 1 : 0;
  c->timing["ns_c"] = b.ns_c;
  for (auto& t : tab)
    if (!strcmp(name, t.n)) {
      if (!t.d->p || t.d->bytes < t.bytes) return set_error(c, LRN_ERR_STATE, "block array %s not allocated", name);
      return copy_out(c, out, t.d->p, t.bytes);
    }
  return set_error(c, LRN_ERR_ARG, "unknown block array %s", name);
}

extern "C" int lrn_dbg_eigmin(lrn_ctx* c, int n, const double* M, double* lam, int* steps) {
  if (!c || n <= 0 || !M || !lam) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  DBuf d;
  LRN_TRY(ensure(c, d, (size_t)n * n * 8));
  LRN_TRY(copy_in(c, d.p, M, (size_t)n * n * 8));
  int rc = steps ? eigmin_dev(c, d.as<double>(), n, lam, steps) : eigmin_certified(c, d.as<double>(), n, lam);
  release(d);
  return rc;
}

// ---- builder-defined synthetic problem on top of lrn_synthetic_dense_model
namespace lrn {
__global__ void synth_x0_kernel(double* __restrict__ X, const double* __restrict__ Q, int n, int r) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    double s = 0.0;
    for (int k = 0; k < r; ++k) s += Q[i + (long)k * n] * Q[j + (long)k * n];
    X[e] = s / n + (i == j ? 1.0 : 0.0);
  }
}
__global__ void eye_add_kernel(double* __restrict__ out, const double* __restrict__ M, double sgn, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
    out[e] = sgn * M[e] + ((int)(e % n) == (int)(e / n) ? 1.0 : 0.0);
}
}  // namespace lrn

extern "C" int lrn_synthetic_dense_problem(lrn_ctx* c, uint64_t seed, double* b_out, double* y0_out, double* normC) {
  if (!c || c->nlmi != 1 || !b_out || !y0_out) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  LmiBlock& b = c->lmi[0];
  LRN_TRY(ensure_resident(c, b));
  const int m = b.msz, n = c->nvar;
  const long mm_ = (long)m * m;
  // host-side small random factors (deterministic LCG-free: splitmix64 + Box-Muller)
  auto next = [&seed]() {
    seed += 0x9E3779B97F4A7C15ull;
    uint64_t z = seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  auto unif = [&]() { return ((double)(next() >> 11) + 0.5) / 9007199254740992.0; };
  auto gauss = [&]() { return std::sqrt(-2.0 * std::log(unif())) * std::cos(6.283185307179586 * unif()); };
  const int r = 8;
  std::vector<double> Q((size_t)m * r), y0(n);
  for (auto& v : Q) v = gauss();
  for (auto& v : y0) v = gauss() / std::sqrt((double)n);
  LRN_TRY(copy_in(c, b.t1.p, Q.data(), Q.size() * 8));
  hipLaunchKernelGGL(synth_x0_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.t0.as<double>(), b.t1.as<double>(), m, r);
  // b = AA vec(X0)
  LRN_HIP(c, hipMemsetAsync(c->v1.p, 0, (size_t)n * 8, c->stream));
  LRN_TRY(aa_times(c, b, b.t0.as<double>(), c->v1.as<double>()));
  LRN_TRY(copy_out(c, b_out, c->v1.p, (size_t)n * 8));
  // C = I + mat(AA' y0)
  LRN_TRY(copy_in(c, c->v0.p, y0.data(), (size_t)n * 8));
  LRN_TRY(aat_to_mat(c, b, c->v0.as<double>(), b.t0.as<double>()));
  hipLaunchKernelGGL(eye_add_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.Cd.as<double>(), b.t0.as<double>(), 1.0, m);
  if (normC) {
    LRN_TRY(ensure(c, c->redout, 64 * 8));
    LRN_TRY(dot_dev(c, b.Cd.as<double>(), nullptr, mm_, c->redout.as<double>()));
    double s = 0;
    LRN_TRY(copy_out(c, &s, c->redout.p, 8));
    *normC = std::sqrt(s);
  }
  memcpy(y0_out, y0.data(), (size_t)n * 8);
  return LRN_OK;
}
