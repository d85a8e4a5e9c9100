// The n x n products of the NT scaling, the interior-point step and the Lanczos searches (declared in ops.h): every one is
// C = alpha A Bm' or a transposed form of it, on the kernel gemm() picks (gemm_f64.hip), plus the consumers that add the
// split-K slabs of a mid-size product while they transpose or symmetrise it.
#include "ctx.h"
#include "ops.h"
#include "reduce.h"

namespace lrn {

// C (m x n) = alpha A Bm' with K = m, all column-major with leading dimension m: both operands contiguous along the result's
// dimensions -> the direct-to-LDS kernels
static GemmDesc nt_desc(int m, int n, const double* A, const double* Bm, double* C, double alpha, int flags = 0) {
  GemmDesc g;
  g.A = A; g.sAm = 1; g.sAk = m;
  g.B = Bm; g.sBk = m; g.sBn = 1;
  g.C = C; g.sCm = 1; g.sCn = m;
  g.M = m; g.N = n; g.K = m;
  g.alpha = alpha;
  g.flags = flags;
  return g;
}

int gemm_nn(hipStream_t st, int n, const double* A, bool tA, const double* B, bool tB, double* C, int flags) {
  GemmDesc g;
  g.A = A; g.B = B; g.C = C;
  g.M = g.N = g.K = n;
  if (!tA) { g.sAm = 1; g.sAk = n; } else { g.sAm = n; g.sAk = 1; }
  if (!tB) { g.sBk = 1; g.sBn = n; } else { g.sBk = n; g.sBn = 1; }
  g.sCm = 1; g.sCn = n;
  g.flags = flags;
  return gemm(st, g);
}

int gemm_nt(hipStream_t st, int n, const double* A, const double* Bm, double* C, int flags, double alpha, double* Ct) {
  GemmDesc g = nt_desc(n, n, A, Bm, C, alpha, flags);
  g.C2 = Ct;
  return gemm(st, g);
}

int gemm_nt_slabs(hipStream_t st, int n, const double* A, const double* Bm, double* C, double alpha, SlabSrc* src) {
  return gemm_slabs(st, nt_desc(n, n, A, Bm, C, alpha), src);
}

// C = sum of the slabs, Ct = its transpose: 32 x 32 tiles through LDS (round 4: the slab addition of a mid-size product and
// the transpose pass that followed it were two launches and two trips through memory)
__global__ __launch_bounds__(256) void slabs_transpose_kernel(SlabSrc src, int n, double* __restrict__ C, double* __restrict__ Ct) {
  __shared__ double tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int i = bx + tx, j = by + r;
    if (i < n && j < n) {
      const long e = (long)i + (long)j * n;
      const double v = slab_sum(src, e);
      tile[r][tx] = v;
      if (src.n > 1 || src.p != C) C[e] = v;
    }
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int i = by + tx, j = bx + r;      // Ct[i][j] = C[j][i]
    if (i < n && j < n) Ct[(long)i + (long)j * n] = tile[tx][r];
  }
}

void slabs_to_c_and_ct(hipStream_t st, const SlabSrc& src, int n, double* C, double* Ct) {
  hipLaunchKernelGGL(slabs_transpose_kernel, dim3((n + 31) / 32, (n + 31) / 32), dim3(256), 0, st, src, n, C, Ct);
}

// C = (S + S') / 2 for S = the sum of the slabs (or C itself, in place): the tile pair (bi, bj), (bj, bi) by one workgroup.
// T != null: the Newton-Schulz pass on P = C in the same sweep -- T = a (3 I - a^2 P) / 2 and this workgroup's share of
// ||I - P||_F^2 in part[blockIdx.x] (ns_t_kernel's work; C may then be null: nobody reads P itself)
__global__ __launch_bounds__(256) void slabs_sym_kernel(SlabSrc src, int n, double* __restrict__ C, double a, double* __restrict__ T,
                                                        double* __restrict__ part) {
  __shared__ double ta[32][33], tb[32][33];
  __shared__ double sh[4];
  const int nt = (n + 31) / 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  // pair index -> (bi <= bj)
  int bj = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while ((long)(bj + 1) * (bj + 2) / 2 <= (long)blockIdx.x) ++bj;
  while ((long)bj * (bj + 1) / 2 > (long)blockIdx.x) --bj;
  const int bi = (int)(blockIdx.x - (long)bj * (bj + 1) / 2);
  if (bj >= nt) return;
  const int oi = bi * 32, oj = bj * 32;
  for (int r = ty; r < 32; r += 8) {
    const int i = oi + tx, j = oj + r;       // tile (bi, bj): element (i, j)
    ta[r][tx] = (i < n && j < n) ? slab_sum(src, (long)i + (long)j * n) : 0.0;
    const int i2 = oj + tx, j2 = oi + r;     // tile (bj, bi): element (i2, j2)
    tb[r][tx] = (i2 < n && j2 < n) ? slab_sum(src, (long)i2 + (long)j2 * n) : 0.0;
  }
  __syncthreads();
  const double a3 = 0.5 * a * a * a, a1 = 1.5 * a;
  double acc = 0.0;
  for (int r = ty; r < 32; r += 8) {
    const int i = oi + tx, j = oj + r;
    if (i < n && j < n) {
      const double v = 0.5 * (ta[r][tx] + tb[tx][r]);
      if (C) C[(long)i + (long)j * n] = v;
      if (T) {
        const double rr = (i == j ? 1.0 : 0.0) - v;
        acc += rr * rr;
        T[(long)i + (long)j * n] = (i == j ? a1 : 0.0) - a3 * v;
      }
    }
    const int i2 = oj + tx, j2 = oi + r;
    if (bi != bj && i2 < n && j2 < n) {
      const double v = 0.5 * (tb[r][tx] + ta[tx][r]);
      if (C) C[(long)i2 + (long)j2 * n] = v;
      if (T) {
        acc += v * v;                                  // (off the diagonal: the residual entry is -v)
        T[(long)i2 + (long)j2 * n] = -a3 * v;
      }
    }
  }
  if (!T || !part) return;
  acc = wg_sum<4>(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// The same from slabs that hold only the LOWER 64-tiles of the product (rows i, columns j with i / 64 >= j / 64; gemm_slabs
// with GEMM_TRI_LOWER: half the MFMA work).  The pair of 32-tiles (bi <= bj) is filled from the lower one, (bj, bi): C over
// there = the sum, C over here = its transpose; inside a diagonal 32-tile the lower triangle is mirrored.  The result is
// the product's lower triangle mirrored -- exactly symmetric, NOT the average of the two triangles that slabs_sym_kernel
// forms (the form the products of msz >= BIG_TILE_MIN_N have had since round 3: lower tiles + mirror).
__global__ __launch_bounds__(256) void slabs_symlow_kernel(SlabSrc src, int n, double* __restrict__ C, double a, double* __restrict__ T,
                                                           double* __restrict__ part) {
  __shared__ double tl[32][33];
  __shared__ double sh[4];
  const int nt = (n + 31) / 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  int bj = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while ((long)(bj + 1) * (bj + 2) / 2 <= (long)blockIdx.x) ++bj;
  while ((long)bj * (bj + 1) / 2 > (long)blockIdx.x) --bj;
  const int bi = (int)(blockIdx.x - (long)bj * (bj + 1) / 2);
  if (bj >= nt) return;
  const int oi = bi * 32, oj = bj * 32;          // lower tile: rows oj .., columns oi ..
  for (int r = ty; r < 32; r += 8) {
    const int i = oj + tx, j = oi + r;           // element (i, j) of the lower tile, i fastest
    tl[r][tx] = (i < n && j < n) ? slab_sum(src, (long)i + (long)j * n) : 0.0;
  }
  __syncthreads();
  const double a3 = 0.5 * a * a * a, a1 = 1.5 * a;
  double acc = 0.0;
  for (int r = ty; r < 32; r += 8) {
    {   // the lower tile itself: element (oj + tx, oi + r)
      const int i = oj + tx, j = oi + r;
      if (i < n && j < n) {
        const double v = (bi == bj && tx < r) ? tl[tx][r] : tl[r][tx];       // diagonal tile: (i, j) above the diagonal <- (j, i)
        if (C) C[(long)i + (long)j * n] = v;
        if (T) {
          const double rr = (i == j ? 1.0 : 0.0) - v;
          acc += rr * rr;
          T[(long)i + (long)j * n] = (i == j ? a1 : 0.0) - a3 * v;
        }
      }
    }
    if (bi != bj) {   // its mirror image: element (oi + tx, oj + r) = lower (oj + r, oi + tx)
      const int i = oi + tx, j = oj + r;
      if (i < n && j < n) {
        const double v = tl[tx][r];
        if (C) C[(long)i + (long)j * n] = v;
        if (T) {
          acc += v * v;
          T[(long)i + (long)j * n] = -a3 * v;
        }
      }
    }
  }
  if (!T || !part) return;
  acc = wg_sum<4>(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// C = (S + S') / 2 of S = alpha A Bm' from its split-K slabs -- the lower 64-tiles alone where gemm_slabs provides them, else the
// full product (into `full`, which may be C) -- with the pass of slabs_sym_kernel on it (T, part; C may be null)
static int nt_sym_from_slabs(hipStream_t st, int n, const double* A, const double* Bm, double* C, double* full, double alpha,
                             double a, double* T, double* part) {
  SlabSrc src;
  const long nt = (n + 31) / 32;
  const dim3 grid((unsigned)(nt * (nt + 1) / 2));
  // the lower 64-tiles as split-K slabs (src.n == 0: not available for this size)
  LRN_TRY(gemm_slabs(st, nt_desc(n, n, A, Bm, nullptr, alpha, GEMM_TRI_LOWER), &src));
  if (src.n > 0) {      // (round 4: lower 64-tiles only + mirror, as the products of msz >= BIG_TILE_MIN_N)
    hipLaunchKernelGGL(slabs_symlow_kernel, grid, dim3(256), 0, st, src, n, C, a, T, part);
    return LRN_OK;
  }
  LRN_TRY(gemm_nt_slabs(st, n, A, Bm, full, alpha, &src));
  hipLaunchKernelGGL(slabs_sym_kernel, grid, dim3(256), 0, st, src, n, C, a, T, part);
  return LRN_OK;
}

// P = A Bm' symmetrised (not stored) -> T = a (3 I - a^2 P) / 2, partial sums of ||I - P||_F^2 in part[0 .. *npart): the
// Newton-Schulz step's first product with its element-wise pass folded into the slab addition (msz < BIG_TILE_MIN_N, one rank)
int gemm_nt_sym_ns(hipStream_t st, int n, const double* A, const double* Bm, double* scratchC, double a, double* T, double* part,
                   int* npart) {
  const long nt = (n + 31) / 32;
  *npart = (int)(nt * (nt + 1) / 2);
  return nt_sym_from_slabs(st, n, A, Bm, nullptr, scratchC, 1.0, a, T, part);
}

// `tri`: which operand is triangular with explicit zeros in its other triangle (GEMM_KFROM_M / _N: zero for k < m / k < n,
// GEMM_KTO_M / _N: zero for k > m / k > n; one flag) -- the K loop of every tile then covers only the range where that
// operand is not zero: half the work of the products with L_X, L_X', L_S^-T (bitwise the same sums: the skipped terms
// are exact zeros).  Taken where the 128-tile kernel runs (n >= BIG_TILE_MIN_N, even); the sharded product ignores it.
static inline int tri_hint(int n, int tri) { return (n >= BIG_TILE_MIN_N && (n & 1) == 0) ? tri : 0; }

// (M + M')/2 in place
__global__ void sym_inplace_kernel(double* __restrict__ M, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    if (i < j) {
      const long f = (long)j + (long)i * n;
      const double v = 0.5 * (M[e] + M[f]);
      M[e] = v;
      M[f] = v;
    }
  }
}

// upper := lower inside the 128 x 128 diagonal tiles (GEMM_C_MIRROR mirrors the tiles below the diagonal only)
__global__ __launch_bounds__(256) void mirror_diag_tiles_kernel(double* __restrict__ C, int n) {
  const int t0 = blockIdx.x * 128;
  for (int e = threadIdx.x; e < 128 * 128; e += 256) {
    const int i = t0 + (e & 127), j = t0 + (e >> 7);
    if (i < n && j < n && i < j) C[(long)i + (long)j * n] = C[(long)j + (long)i * n];
  }
}

// C = alpha A Bm' for a product that is symmetric in exact arithmetic, returned exactly symmetric: lower tiles + mirror on
// the 128-tile direct-to-LDS kernel where that fills the chip, the plain product and a symmetrising pass below (at msz 800
// the 28 lower tiles of 128 take 121 us, the full product on 64-tiles 35 us)
int gemm_nt_sym(hipStream_t st, int n, const double* A, const double* Bm, double* C, double alpha, int tri) {
  if (n >= BIG_TILE_MIN_N) {
    LRN_TRY(gemm_nt(st, n, A, Bm, C, GEMM_TRI_LOWER | GEMM_C_MIRROR | tri_hint(n, tri), alpha));
    hipLaunchKernelGGL(mirror_diag_tiles_kernel, dim3((n + 127) / 128), dim3(256), 0, st, C, n);
    return LRN_OK;
  }
  return nt_sym_from_slabs(st, n, A, Bm, C, C, alpha, 0.0, nullptr, nullptr);
}

bool products_sharded(const lrn_ctx* c, hipStream_t st, int n) {
  return c->comm && c->world > 1 && c->opt.shard_products != 0 && st == c->stream && n >= c->opt.shard_products_min;
}

static int shard_cols(const lrn_ctx* c, int n, int* c0, int* c1) {
  const int cb = (((n + c->world - 1) / c->world) + 15) & ~15;      // 16-column granularity: aligned operand pointers
  *c0 = std::min(n, c->rank * cb);
  *c1 = std::min(n, *c0 + cb);
  return cb;
}

int pgemm_nt(lrn_ctx* c, hipStream_t st, int n, const double* A, const double* Bm, double* C, int tri, double alpha,
             double* Ct) {
  if (!products_sharded(c, st, n)) return gemm_nt(st, n, A, Bm, C, tri_hint(n, tri), alpha, Ct);
  int c0, c1;
  const int cb = shard_cols(c, n, &c0, &c1);
  if (c1 > c0) {
    LRN_TRY(gemm(st, nt_desc(n, c1 - c0, A, Bm + c0, C + (long)c0 * n, alpha)));      // C[:, c0:c1] = alpha A Bm[c0:c1, :]'
  }
  LRN_TRY(comm_allgather_cols(c, C, n, cb));
  c->counts["pgemm_sharded"] += 1;
  if (Ct) transpose_mat(st, C, n, Ct);
  return LRN_OK;
}

int pgemm_nt_sym(lrn_ctx* c, hipStream_t st, int n, const double* A, const double* Bm, double* C, double alpha, int tri) {
  if (!products_sharded(c, st, n)) return gemm_nt_sym(st, n, A, Bm, C, alpha, tri);
  LRN_TRY(pgemm_nt(c, st, n, A, Bm, C, 0, alpha, nullptr));
  hipLaunchKernelGGL(sym_inplace_kernel, dim3(nb((long)n * n)), dim3(256), 0, st, C, n);
  return LRN_OK;
}

// C = alpha A Bm' for a consumer that can add split-K slabs while it reads: below msz BIG_TILE_MIN_N on one rank the product may come
// back as slabs (src->n > 1, C untouched); otherwise it is in C
int prod_slabs(lrn_ctx* c, hipStream_t st, int n, const double* A, const double* Bm, double* C, double alpha, int tri,
               SlabSrc* src) {
  if (n >= BIG_TILE_MIN_N || products_sharded(c, st, n)) {
    src->p = C; src->stride = 0; src->n = 1;
    return pgemm_nt(c, st, n, A, Bm, C, tri, alpha);
  }
  return gemm_nt_slabs(st, n, A, Bm, C, alpha, src);
}

}  // namespace lrn
