// Element-wise and tiled passes over n x n matrices (column-major) and the two-stage dot product, shared by the NT scaling
// (prepw.hip), the interior-point step (ipstep.hip) and the Lyapunov solve (lyap.hip); declared in one block of ops.h.
#include <algorithm>

#include "ops.h"
#include "reduce.h"

namespace lrn {

__global__ void tril_kernel(double* __restrict__ A, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    if (i < j) A[e] = 0.0;
  }
}

__global__ void eye_kernel(double* __restrict__ V, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
    V[e] = (e % n == e / n) ? 1.0 : 0.0;
}

__global__ void mirror_lower_kernel(double* __restrict__ A, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    if (i < j) A[e] = A[(long)j + (long)i * n];
  }
}

// B[:,j] = A[:,j] * f(d[j]);  mode 0: d^-1/2, 1: d^1/2, 2: d^-1
__global__ void scale_cols_kernel(const double* __restrict__ A, const double* __restrict__ d, int n, int mode,
                                  double* __restrict__ B) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int j = (int)(e / n);
    double s = mode == 2 ? d[j] : sqrt(d[j]);
    B[e] = mode == 1 ? A[e] * s : A[e] / s;
  }
}

__global__ void transpose_kernel(const double* __restrict__ A, int n, double* __restrict__ B) {
  __shared__ double tile[32][33];
  int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  for (int r = threadIdx.y; r < 32; r += 8) {
    int i = bx + threadIdx.x, j = by + r;
    if (i < n && j < n) tile[r][threadIdx.x] = A[(long)i + (long)j * n];
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += 8) {
    int i = by + threadIdx.x, j = bx + r;      // B[i][j] = A[j][i]
    if (i < n && j < n) B[(long)i + (long)j * n] = tile[threadIdx.x][r];
  }
}

__global__ __launch_bounds__(256) void coldot_rsqrt_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                           int n, double* __restrict__ out) {
  __shared__ double sh[4];
  const double* a = A + (long)blockIdx.x * n;
  const double* b = B + (long)blockIdx.x * n;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += a[i] * b[i];
  s = wg_sum<4>(s, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = 1.0 / sqrt(s);
}

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

__global__ void add_diag_mat_kernel(double* __restrict__ M, int n, double eps) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) M[(long)i * n + i] += eps;
}

// two-stage reductions: partial[b] = sum A.*B (B may be null -> A.*A)
__global__ __launch_bounds__(256) void dot_part_kernel(const double* __restrict__ A, const double* __restrict__ B, long n,
                                                       double* __restrict__ part) {
  __shared__ double sh[4];
  double s = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) s += A[e] * (B ? B[e] : A[e]);
  s = wg_sum<4>(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void dot_final_kernel(const double* __restrict__ part, int np, double* __restrict__ out) {
  __shared__ double sh[4];
  const double s = block_sum_parts(part, np, sh);
  if (threadIdx.x == 0) *out = s;
}

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
  acc = wg_sum<4>(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// ------------------------------------------------------------------ host wrappers
// k over `total` elements by workgroups of 256
template <class... P, class... A>
static void elementwise(void (*k)(P...), hipStream_t st, long total, A... a) {
  hipLaunchKernelGGL(k, dim3(nb(total)), dim3(256), 0, st, a...);
}
void tril(hipStream_t st, double* A, int n) { elementwise(tril_kernel, st, (long)n * n, A, n); }
void eye_mat(hipStream_t st, double* V, int n) { elementwise(eye_kernel, st, (long)n * n, V, n); }
void mirror_lower(hipStream_t st, double* A, int n) { elementwise(mirror_lower_kernel, st, (long)n * n, A, n); }
void scale_cols(hipStream_t st, const double* A, const double* d, int n, int mode, double* B) {
  elementwise(scale_cols_kernel, st, (long)n * n, A, d, n, mode, B);
}
void scale_sym(hipStream_t st, const double* M, const double* dd, double* out, int n) {
  elementwise(scale_sym_kernel, st, (long)n * n, M, dd, out, n);
}
void lin3(hipStream_t st, double* out, long n, double a, const double* A, double b, const double* B, double c, const double* C) {
  elementwise(lin3_kernel, st, n, out, a, A, b, B, c, C, n);
}
void transpose_mat(hipStream_t st, const double* A, int n, double* B) {
  hipLaunchKernelGGL(transpose_kernel, dim3((n + 31) / 32, (n + 31) / 32), dim3(32, 8), 0, st, A, n, B);
}
void coldot_rsqrt(hipStream_t st, const double* A, const double* B, int n, double* out) {
  hipLaunchKernelGGL(coldot_rsqrt_kernel, dim3(n), dim3(256), 0, st, A, B, n, out);
}
void add_diag_mat(hipStream_t st, double* M, int n, double eps) {
  hipLaunchKernelGGL(add_diag_mat_kernel, dim3((n + 255) / 256), dim3(256), 0, st, M, n, eps);
}
unsigned sym_grid(int n) {
  const long nt = (n + 31) / 32;
  return (unsigned)std::min<long>(1024, nt * nt);
}
void symadd(hipStream_t st, unsigned grid, const SlabSrc& T, int n, double scale, double* out, const double* dotp, double* part) {
  hipLaunchKernelGGL(symadd_kernel, dim3(grid), dim3(256), 0, st, T, n, scale, out, dotp, part);
}
// the tiled kernel from msz 512 on (the element-wise one reads M' with stride n)
void sym_half(hipStream_t st, const double* M, double* out, int n) {
  if (n >= 512) symadd(st, sym_grid(n), SlabSrc{M, 0, 1}, n, 0.5, out, nullptr, nullptr);
  else elementwise(sym_kernel, st, (long)n * n, M, out, n);
}

int sym_product(lrn_ctx* c, hipStream_t st, int n, const double* A, const double* Bm, double* work, double* out, double alpha,
                int tri) {
  if (n >= BIG_TILE_MIN_N) return pgemm_nt_sym(c, st, n, A, Bm, out, alpha, tri);
  SlabSrc prod;
  LRN_TRY(prod_slabs(c, st, n, A, Bm, work, alpha, tri, &prod));
  symadd(st, sym_grid(n), prod, n, 0.5, out, nullptr, nullptr);
  return LRN_OK;
}

int dot_parts_count(long n) { return (int)std::min<long>(1024, (n + 255) / 256); }
void dot_via(hipStream_t st, const double* A, const double* B, long n, double* part, double* out) {
  const int np = dot_parts_count(n);
  hipLaunchKernelGGL(dot_part_kernel, dim3(np), dim3(256), 0, st, A, B, n, part);
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(256), 0, st, part, np, out);
}
int dot_dev(lrn_ctx* c, const double* A, const double* B, long n, double* out_dev) {
  LRN_TRY(ensure(c, c->redbuf, (size_t)(dot_parts_count(n) + 64) * 8));
  dot_via(c->stream, A, B, n, c->redbuf.as<double>(), out_dev);
  return LRN_OK;
}

}  // namespace lrn
