// The data operators: every pass over the constraint data AA outside the Schur assembly.
//   AA vec(Z)    (aa_times, aa_times2: makeRHS, src/makeBBBB.jl:221-228; predictor_corrector.jl:12,186)
//   mat(AA' x)   (aat_to_mat: predictor_corrector.jl:13,252; Solvers.jl:595)
//   MyA, Ax = AA vec(W mat(AA' x) W) (+ C_lin diag(xs) C_lin' x)   (matvec_dev, matvec_partial_dev: Solvers.jl:582-614)
// in all their forms: sparse constraints (one wavefront per constraint / per stored column of AA, a deterministic gather,
// no atomics), dense constraints (three tiers, see dense_route), the pattern-restricted form when mat(AA' x) is sparse,
// the factor form of factored blocks, and the passes split over the ranks of a multi-GPU run.  The two msz^3 products
// of W M W run on the FP64 MFMA GEMM (wmw).  All vectors live in natural constraint order.  Option "profile_ops"
// times each operator by itself (PhaseTimer, ctx.h).  The CG recurrence that calls MyA: cgops.hip; its preconditioners: prec.hip.
#include <algorithm>
#include <cmath>

#include "../../include/loraine_hip.h"
#include "ctx.h"
#include "ops.h"
#include "fac_cols.h"

namespace lrn {

// ------------------------------------------------------------------ AA' x  and  AA vec(Z)
// M[q] = sum_k cq_v[k] * x[cq_j[k]] over the stored columns of AA (sparse constraints):
// one wavefront per stored column (a column can hold one entry per constraint -- e.g. the
// shared corner of thetaG11's 1600 edge blocks), fixed lane partition -> deterministic.
__global__ __launch_bounds__(256) void aat_gather_kernel(const long* __restrict__ cq_q, const long* __restrict__ cq_ptr,
                                                         const int* __restrict__ cq_j, const double* __restrict__ cq_v,
                                                         long ncq, const double* __restrict__ x, double* __restrict__ M) {
  const int lane = threadIdx.x & 63;
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= ncq) return;
  double s = 0.0;
  for (long k = cq_ptr[t] + lane; k < cq_ptr[t + 1]; k += 64) s += cq_v[k] * x[cq_j[k]];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) M[cq_q[t]] = s;
}

// M[q] -= sum_{p<nd} x[sigma[p]] * Adense[p][q]   (scalar tier of the dense passes)
__global__ void aat_dense_kernel(const double* __restrict__ Ad, int nd, long mm, const int* __restrict__ sigma,
                                 const double* __restrict__ x, double* __restrict__ M) {
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < mm; q += (long)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int p = 0; p < nd; ++p) s += x[sigma[p]] * Ad[(long)p * mm + q];
    M[q] -= s;
  }
}

// mat(): (M + M')/2 in place  (kron_etc.jl:13-18)
__global__ void symmetrize_kernel(double* __restrict__ M, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    if (i < j) {
      double a = M[e], b = M[(long)j + (long)i * n];
      double s = (a + b) / 2.0;
      M[e] = s;
      M[(long)j + (long)i * n] = s;
    }
  }
}

// mat() by 32 x 32 tile pairs: tile (bi, bj), bi >= bj, and its mirror image are averaged and written back together, both
// accesses coalesced (symmetrize_kernel reads M' with stride n: 2 ms at msz 10^4 against 0.7)
__global__ __launch_bounds__(256) void symmetrize_tiled_kernel(double* __restrict__ M, int n) {
  __shared__ double ta[32][33], tb[32][33];
  const int nt = (n + 31) / 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (long t = blockIdx.x; t < (long)nt * nt; t += gridDim.x) {
    const int ti = (int)(t % nt), tj = (int)(t / nt);
    if (ti < tj) continue;
    const int bi = ti * 32, bj = tj * 32;
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int i = bi + tx, j = bj + r;       // tile (bi, bj): element (i, j) -> ta[r][tx]
      ta[r][tx] = (i < n && j < n) ? M[(long)i + (long)j * n] : 0.0;
      const int i2 = bj + tx, j2 = bi + r;     // tile (bj, bi): element (i2, j2) -> tb[r][tx]
      tb[r][tx] = (i2 < n && j2 < n) ? M[(long)i2 + (long)j2 * n] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int i = bi + tx, j = bj + r;
      if (i < n && j < n && i != j) {
        const double a = ta[r][tx], b = tb[tx][r];          // M[i,j], M[j,i]
        M[(long)i + (long)j * n] = (i > j ? a + b : b + a) / 2.0;        // (the pair adds in the order of the lower element first, as symmetrize_kernel)
      }
      if (ti != tj) {
        const int i2 = bj + tx, j2 = bi + r;
        if (i2 < n && j2 < n) {
          const double a = tb[r][tx], b = ta[tx][r];        // M[i2,j2] (upper), M[j2,i2] (lower)
          M[(long)i2 + (long)j2 * n] = (b + a) / 2.0;
        }
      }
    }
  }
}

static void symmetrize_dev(hipStream_t st, double* M, int n) {
  const long total = (long)n * n;
  if (n >= 512) {
    const long nt = (n + 31) / 32;
    hipLaunchKernelGGL(symmetrize_tiled_kernel, dim3((unsigned)std::min<long>(4096, nt * nt)), dim3(256), 0, st, M, n);
  } else {
    const long bl = (total + 255) / 256;
    hipLaunchKernelGGL(symmetrize_kernel, dim3((unsigned)(bl < 1 ? 1 : (bl > 4096 ? 4096 : bl))), dim3(256), 0, st, M, n);
  }
}

// out[sigma[p]] += -sum_e a_e Z[r_e,c_e]   (one wavefront per sparse position)
__global__ __launch_bounds__(256) void aa_times_kernel(const long* __restrict__ ptr, const int* __restrict__ er,
                                                       const int* __restrict__ ec, const double* __restrict__ ev,
                                                       const double* __restrict__ Z, int msz, int p_lo, int p_end,
                                                       const int* __restrict__ sigma, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int p = p_lo + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= p_end) return;
  double s = 0.0;
  for (long e = ptr[p] + lane; e < ptr[p + 1]; e += 64) s += ev[e] * Z[(long)er[e] + (long)ec[e] * msz];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) out[sigma[p]] -= s;
}

// ---- the passes over the dense constraint data, scalar tier: one element per lane, any msz and alignment.
// out1[sigma[p]] -= <Adense[p], Z1> (and out2 / Z2 when NZ = 2, in ONE pass over the data), one workgroup per dense slot
template <int NZ>
__global__ __launch_bounds__(256) void aa_dense_dot_kernel(const double* __restrict__ Ad, long mm, const double* __restrict__ Z1,
                                                           const double* __restrict__ Z2, const int* __restrict__ sigma,
                                                           double* __restrict__ out1, double* __restrict__ out2) {
  __shared__ double sh[4 * NZ];
  const double* a = Ad + (long)blockIdx.x * mm;
  double s1 = 0.0, s2 = 0.0;
  for (long q = threadIdx.x; q < mm; q += 256) {
    const double v = a[q];
    s1 += v * Z1[q];
    if (NZ > 1) s2 += v * Z2[q];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off, 64);
    if (NZ > 1) s2 += __shfl_down(s2, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = s1;
    if (NZ > 1) sh[4 + (threadIdx.x >> 6)] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out1[sigma[blockIdx.x]] -= sh[0] + sh[1] + sh[2] + sh[3];
    if (NZ > 1) out2[sigma[blockIdx.x]] -= sh[4] + sh[5] + sh[6] + sh[7];
  }
}

// ---- stream tier: the same passes at sizes where they are HBM streams (C4: 4000 matrices of 32 MB; round 3).  16-byte
// loads, eight of them in flight per lane, and FOUR constraints per workgroup against one read of Z (the scalar tier keeps
// one 8-byte load per lane in flight and re-reads Z from the MALL for every constraint).  Needs msz
// even: every matrix 16-byte aligned.
typedef double v2f64 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void aa_dense_dot4_kernel(const double* __restrict__ Ad, long mm, int nd,
                                                            const double* __restrict__ Z, const int* __restrict__ sigma,
                                                            double* __restrict__ out) {
  __shared__ double sh[4][4];
  const int p0 = blockIdx.x * 4;
  const long n2 = mm >> 1;
  const v2f64* z2 = reinterpret_cast<const v2f64*>(Z);
  const v2f64* a2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) a2[k] = reinterpret_cast<const v2f64*>(Ad + (long)(p0 + k < nd ? p0 + k : p0) * mm);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  long q = threadIdx.x;
  for (; q + 256 < n2; q += 512) {
    const v2f64 z0 = z2[q], z1 = z2[q + 256];
    v2f64 a0[4], a1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { a0[k] = __builtin_nontemporal_load(a2[k] + q); a1[k] = __builtin_nontemporal_load(a2[k] + q + 256); }
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += (a0[k].x * z0.x + a0[k].y * z0.y) + (a1[k].x * z1.x + a1[k].y * z1.y);
  }
  for (; q < n2; q += 256) {
    const v2f64 z0 = z2[q];
#pragma unroll
    for (int k = 0; k < 4; ++k) { const v2f64 a = a2[k][q]; s[k] += a.x * z0.x + a.y * z0.y; }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 4 && p0 + (int)threadIdx.x < nd) {
    const int k = threadIdx.x;
    out[sigma[p0 + k]] -= sh[k][0] + sh[k][1] + sh[k][2] + sh[k][3];
  }
}

// stream tier, two products in one pass (aa_times2)
__global__ __launch_bounds__(256) void aa_dense_dot4x2_kernel(const double* __restrict__ Ad, long mm, int nd,
                                                              const double* __restrict__ Z1, const double* __restrict__ Z2,
                                                              const int* __restrict__ sigma, double* __restrict__ out1,
                                                              double* __restrict__ out2) {
  __shared__ double sh[8][4];
  const int p0 = blockIdx.x * 4;
  const long n2 = mm >> 1;
  const v2f64* y2 = reinterpret_cast<const v2f64*>(Z1);
  const v2f64* z2 = reinterpret_cast<const v2f64*>(Z2);
  const v2f64* a2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) a2[k] = reinterpret_cast<const v2f64*>(Ad + (long)(p0 + k < nd ? p0 + k : p0) * mm);
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long q = threadIdx.x; q < n2; q += 256) {
    const v2f64 y0 = y2[q], z0 = z2[q];
    v2f64 a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = a2[k][q];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s[k] += a[k].x * y0.x + a[k].y * y0.y;
      s[4 + k] += a[k].x * z0.x + a[k].y * z0.y;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 8 && p0 + (int)(threadIdx.x & 3) < nd) {
    const int k = threadIdx.x;
    const double v = sh[k][0] + sh[k][1] + sh[k][2] + sh[k][3];
    if (k < 4) out1[sigma[p0 + k]] -= v;
    else out2[sigma[p0 + k - 4]] -= v;
  }
}

// stream tier: M[q] -= sum_p x[sigma[p]] Adense[p][q], two entries per lane, eight matrices in flight
__global__ __launch_bounds__(256) void aat_dense2_kernel(const double* __restrict__ Ad, int nd, long mm,
                                                         const int* __restrict__ sigma, const double* __restrict__ x,
                                                         double* __restrict__ M) {
  const long n2 = mm >> 1;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= n2) return;
  const v2f64* a2 = reinterpret_cast<const v2f64*>(Ad) + q;
  v2f64 s0 = {0.0, 0.0}, s1 = {0.0, 0.0};
  int p = 0;
  for (; p + 8 <= nd; p += 8) {
    v2f64 a[8];
    double xs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { a[k] = __builtin_nontemporal_load(a2 + (long)(p + k) * n2); xs[k] = x[sigma[p + k]]; }
#pragma unroll
    for (int k = 0; k < 8; k += 2) { s0 += xs[k] * a[k]; s1 += xs[k + 1] * a[k + 1]; }
  }
  // (rotating the order of the matrices per group of workgroups -- eight addresses 32 MB apart meet the same DRAM banks --
  // changes nothing: DESIGN.md Appendix A)
  for (; p < nd; ++p) s0 += x[sigma[p]] * a2[(long)p * n2];
  v2f64* m2 = reinterpret_cast<v2f64*>(M) + q;
  *m2 -= s0 + s1;
}

// ---- tri tier (round 4): the same passes over HALF the bytes.  Every A_k is symmetric, so <A_k, Z> = sum_{i>=j} A_k[i,j] w[i,j] with
// w = Z + Z' below the diagonal, Z on it, and mat(AA'x) is the mirror image of its lower triangle.  Only the column tails
// rows >= j of each matrix are streamed (they are contiguous in the column-major storage), cut into chunks of 64 x 16 bytes
// = 128 rows listed in a table built once per matrix side (TriChunk; the tails start at j rounded down to 16 rows so that
// every chunk is 128-byte aligned: 0.8 % of over-read at msz 2000, covered by zero weights / masked stores).  One wave per
// chunk; the workgroup's four chunks are consecutive in the table, i.e. mostly one contiguous 4 KB piece of a column.
struct TriChunk { long off; int col; int nv2; };      // first element (doubles), column, valid 16-byte pairs (<= 64)

// w = tri-weights of Z: Z + Z' strictly below the diagonal, Z on it, zero above
__global__ void tri_weights_kernel(const double* __restrict__ Z, int n, double* __restrict__ Wt) {
  __shared__ double tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;      // output tile rows bx.., columns by..
  if (bx + 31 < by) {                                          // entirely above the diagonal
    for (int r = threadIdx.y; r < 32; r += 8) {
      const int i = bx + threadIdx.x, j = by + r;
      if (i < n && j < n) Wt[(long)i + (long)j * n] = 0.0;
    }
    return;
  }
  for (int r = threadIdx.y; r < 32; r += 8) {                  // tile[r][t] = Z[by + t, bx + r]  (the transposed block)
    const int i = by + threadIdx.x, j = bx + r;
    if (i < n && j < n) tile[r][threadIdx.x] = Z[(long)i + (long)j * n];
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int i = bx + threadIdx.x, j = by + r;
    if (i < n && j < n) {
      const double a = Z[(long)i + (long)j * n];
      Wt[(long)i + (long)j * n] = i > j ? a + tile[threadIdx.x][r] : (i == j ? a : 0.0);
    }
  }
}

// upper triangle <- lower triangle
__global__ void mirror_lower_tiled_kernel(double* __restrict__ A, int n) {
  __shared__ double tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;      // source tile rows bx.., columns by.. (on or below the diagonal)
  if (bx < by) return;
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int i = bx + threadIdx.x, j = by + r;
    if (i < n && j < n) tile[r][threadIdx.x] = A[(long)i + (long)j * n];
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int i = by + threadIdx.x, j = bx + r;              // destination (i, j) = transposed position
    if (i < n && j < n && i < j) A[(long)i + (long)j * n] = tile[threadIdx.x][r];
  }
}

// out[sigma[p]] -= <A_p, Z> for NZ weight matrices at once (NZ = 1, 2), four constraints per workgroup
template <int NZ>
__global__ __launch_bounds__(256) void aa_dense_tri_dot4_kernel(const double* __restrict__ Ad, long mm, int nd,
                                                                const double* __restrict__ W1, const double* __restrict__ W2,
                                                                const TriChunk* __restrict__ tab, int nch,
                                                                const int* __restrict__ sigma, double* __restrict__ out1,
                                                                double* __restrict__ out2) {
  __shared__ double sh[4 * NZ][4];
  const int p0 = blockIdx.x * 4;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const v2f64* a2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) a2[k] = reinterpret_cast<const v2f64*>(Ad + (long)(p0 + k < nd ? p0 + k : p0) * mm);
  const v2f64* w1 = reinterpret_cast<const v2f64*>(W1);
  const v2f64* w2 = reinterpret_cast<const v2f64*>(NZ > 1 ? W2 : W1);
  double s[4 * NZ];
#pragma unroll
  for (int k = 0; k < 4 * NZ; ++k) s[k] = 0.0;
  for (int ch = w; ch < nch; ch += 8) {
    const TriChunk e0 = tab[ch];
    const bool two = ch + 4 < nch;
    const TriChunk e1 = tab[two ? ch + 4 : ch];
    const bool v0 = lane < e0.nv2, v1 = two && lane < e1.nv2;
    const long q0 = (e0.off >> 1) + (v0 ? lane : 0), q1 = (e1.off >> 1) + (v1 ? lane : 0);
    v2f64 a0[4], a1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { a0[k] = __builtin_nontemporal_load(a2[k] + q0); a1[k] = __builtin_nontemporal_load(a2[k] + q1); }
    v2f64 y0 = w1[q0], y1 = w1[q1];
    if (!v0) y0 = (v2f64){0.0, 0.0};
    if (!v1) y1 = (v2f64){0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += (a0[k].x * y0.x + a0[k].y * y0.y) + (a1[k].x * y1.x + a1[k].y * y1.y);
    if (NZ > 1) {
      v2f64 z0 = w2[q0], z1 = w2[q1];
      if (!v0) z0 = (v2f64){0.0, 0.0};
      if (!v1) z1 = (v2f64){0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 4; ++k) s[4 + k] += (a0[k].x * z0.x + a0[k].y * z0.y) + (a1[k].x * z1.x + a1[k].y * z1.y);
    }
  }
#pragma unroll
  for (int k = 0; k < 4 * NZ; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
    if (lane == 0) sh[k][w] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 4 * NZ && p0 + (int)(threadIdx.x & 3) < nd) {
    const int k = threadIdx.x;
    const double v = (sh[k][0] + sh[k][1]) + (sh[k][2] + sh[k][3]);
    if (k < 4) out1[sigma[p0 + k]] -= v;
    else out2[sigma[p0 + k - 4]] -= v;
  }
}

// lower triangle of M -= sum_p x[sigma[p]] A_p: one wave per chunk, eight matrices in flight per lane
__global__ __launch_bounds__(256) void aat_dense_tri_kernel(const double* __restrict__ Ad, int nd, long mm, int m,
                                                            const int* __restrict__ sigma, const double* __restrict__ x,
                                                            const TriChunk* __restrict__ tab, int nch, double* __restrict__ M) {
  const int lane = threadIdx.x & 63;
  const int ch = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (ch >= nch) return;
  const TriChunk e = tab[ch];
  if (lane >= e.nv2) return;
  const long n2 = mm >> 1;
  const v2f64* a2 = reinterpret_cast<const v2f64*>(Ad) + (e.off >> 1) + lane;
  v2f64 s0 = {0.0, 0.0}, s1 = {0.0, 0.0};
  int p = 0;
  for (; p + 8 <= nd; p += 8) {
    v2f64 a[8];
    double xs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { a[k] = __builtin_nontemporal_load(a2 + (long)(p + k) * n2); xs[k] = x[sigma[p + k]]; }
#pragma unroll
    for (int k = 0; k < 8; k += 2) { s0 += xs[k] * a[k]; s1 += xs[k + 1] * a[k + 1]; }
  }
  for (; p < nd; ++p) s0 += x[sigma[p]] * a2[(long)p * n2];
  const v2f64 t = s0 + s1;
  double* mp = M + e.off + 2 * lane;
  const int r = (int)(e.off - (long)e.col * m) + 2 * lane;      // row of the first element of the pair
  if (r >= e.col) mp[0] -= t.x;
  if (r + 1 >= e.col) mp[1] -= t.y;
}

// is every dense constraint matrix symmetric?  flag[0] = 1 when a pair differs
__global__ __launch_bounds__(256) void dense_sym_check_kernel(const double* __restrict__ Ad, int m, int* __restrict__ flag) {
  const double* A = Ad + (long)blockIdx.x * m * m;
  bool bad = false;
  for (long e = threadIdx.x; e < (long)m * m; e += 256) {
    const int i = (int)(e % m), j = (int)(e / m);
    if (i > j && A[e] != A[(long)j + (long)i * m]) bad = true;
  }
  if (bad) flag[0] = 1;
}

// row-sharded variants (multi-GPU mat-vec): only entries with r0 <= row < r1; Zg holds the rows
// [r0,r1) of Z with leading dimension ldz
__global__ __launch_bounds__(256) void aa_times_rows_kernel(const long* __restrict__ ptr, const int* __restrict__ er,
                                                            const int* __restrict__ ec, const double* __restrict__ ev,
                                                            const double* __restrict__ Zg, int ldz, int r0, int r1,
                                                            int p_lo, int p_end, const int* __restrict__ sigma,
                                                            double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int p = p_lo + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= p_end) return;
  double s = 0.0;
  for (long e = ptr[p] + lane; e < ptr[p + 1]; e += 64) {
    int r = er[e];
    if (r >= r0 && r < r1) s += ev[e] * Zg[(long)(r - r0) + (long)ec[e] * ldz];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) out[sigma[p]] -= s;
}

__global__ __launch_bounds__(256) void aa_dense_dot_rows_kernel(const double* __restrict__ Ad, int m,
                                                                const double* __restrict__ Zg, int ldz, int r0, int r1,
                                                                const int* __restrict__ sigma, double* __restrict__ out) {
  __shared__ double sh[4];
  const double* a = Ad + (long)blockIdx.x * m * m;
  const int nr = r1 - r0;
  double s = 0.0;
  for (long q = threadIdx.x; q < (long)nr * m; q += 256) {
    int r = (int)(q % nr), cc = (int)(q / nr);
    s += a[(long)(r0 + r) + (long)cc * m] * Zg[(long)r + (long)cc * ldz];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[sigma[blockIdx.x]] -= sh[0] + sh[1] + sh[2] + sh[3];
}

// linear block, two deterministic passes (no floating-point atomics):
//   t_l = xs_l * sum_i C[i,l] x_i   (by column);   y_i += sum_l C[i,l] t_l   (by row, CSR built at upload)
__global__ void lin_t_kernel(const long* __restrict__ ptr, const int* __restrict__ row, const double* __restrict__ val,
                             const double* __restrict__ xs, int nlin, const double* __restrict__ x,
                             double* __restrict__ tl) {
  int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nlin) return;
  double t = 0.0;
  for (long k = ptr[l]; k < ptr[l + 1]; ++k) t += val[k] * x[row[k]];
  tl[l] = t * xs[l];
}

__global__ void lin_rows_kernel(const long* __restrict__ rptr, const int* __restrict__ rcol,
                                const double* __restrict__ rval, const double* __restrict__ tl, int n,
                                double* __restrict__ y) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (long k = rptr[i]; k < rptr[i + 1]; ++k) s += rval[k] * tl[rcol[k]];
  y[i] += s;
}

// d_i += sum_l C[i,l]^2 xs_l
__global__ void lin_diag_kernel(const long* __restrict__ rptr, const int* __restrict__ rcol,
                                const double* __restrict__ rval, const double* __restrict__ xs, int n,
                                double* __restrict__ d) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (long k = rptr[i]; k < rptr[i + 1]; ++k) s += rval[k] * rval[k] * xs[rcol[k]];
  d[i] += s;
}

void lin_diag(lrn_ctx* c, double* d) {
  hipLaunchKernelGGL(lin_diag_kernel, dim3(nb(c->nvar)), dim3(256), 0, c->stream, c->cr_ptr.as<long>(), c->cr_col.as<int>(),
                     c->cr_val.as<double>(), c->lin_xs.as<double>(), c->nvar, d);
}

int lin_matvec(lrn_ctx* c, const double* x, double* y) {
  LRN_TRY(ensure(c, c->redbuf, (size_t)std::max(c->nlin, 64) * 8));
  double* tl = c->redbuf.as<double>();
  const unsigned gl = (unsigned)((c->nlin + 255) / 256), gn = (unsigned)((c->nvar + 255) / 256);
  hipLaunchKernelGGL(lin_t_kernel, dim3(gl), dim3(256), 0, c->stream, c->cl_ptr.as<long>(), c->cl_rown.as<int>(),
                     c->cl_val.as<double>(), c->lin_xs.as<double>(), c->nlin, x, tl);
  hipLaunchKernelGGL(lin_rows_kernel, dim3(gn), dim3(256), 0, c->stream, c->cr_ptr.as<long>(), c->cr_col.as<int>(),
                     c->cr_val.as<double>(), tl, c->nvar, y);
  return LRN_OK;
}

// ------------------------------------------------------------------ sparse-aware mat-vec
// When M = mat(AA'x) is sparse (every constraint sparse, e.g. C5: 9 nnz each, 18 per column of M),
// AA vec(W M W) needs Z = W M W only on the pattern of M.  With N = M W  (N(:,q) = M W(:,q)):
//   Z[p,q] = W(:,p) . N(:,q)        -- two contiguous columns
// and N' = W M is a sparse combination of columns of W:  N'(:,r) = sum_s M[s,r] W(:,s).
// 2 nnz(M) msz + nnz(M) msz flop instead of 4 msz^3; the kernels are bandwidth-bound (L2 / MALL).

__global__ __launch_bounds__(256) void sp_gather_kernel(const long* __restrict__ cq_ptr, const int* __restrict__ cq_j,
                                                        const double* __restrict__ cq_v, long ncq,
                                                        const double* __restrict__ x, double* __restrict__ raw) {
  const int lane = threadIdx.x & 63;
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= ncq) return;
  double s = 0.0;
  for (long k = cq_ptr[t] + lane; k < cq_ptr[t + 1]; k += 64) s += cq_v[k] * x[cq_j[k]];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) raw[t] = s;
}

// mat(): (M + M')/2 on the pattern  (kron_etc.jl:13-18)
__global__ void sp_symmetrize_kernel(const double* __restrict__ raw, const int* __restrict__ pc_t, long ncq,
                                     double* __restrict__ Mv) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < ncq) Mv[t] = (raw[t] + raw[pc_t[t]]) / 2.0;
}

// N[r, q] = sum_{t in column r of M} Mv[t] * W[q, row(t)]   for q in [q_lo, q_hi), all r  (msz >= 1500).
// The q-tiles are dealt to the XCDs: XCD x = blockIdx.x % 8 sweeps all row tiles of q-tile 8 (j / R) + x, j = blockIdx.x / 8,
// 64 columns wide, so the 64 x msz slab of W (5 MB at msz 10^4) it gathers from -- every row 36 times at C5 -- stays in its
// own L2 (a grid that walks the row tiles first has the eight L2s miss on the same slab: DESIGN.md Appendix A).  One wave
// per 4 rows r, lanes over q (512-byte segments of W).
__global__ __launch_bounds__(256) void sp_wm_xcd_kernel(const long* __restrict__ pc_ptr, const int* __restrict__ pc_r,
                                                        const double* __restrict__ Mv, const double* __restrict__ W, int m,
                                                        int q_lo, int q_hi, double* __restrict__ N) {
  const int R = (m + 15) / 16, Q = (q_hi - q_lo + 63) / 64;
  const int xcd = blockIdx.x & 7;
  const long j = blockIdx.x >> 3;
  const int qt = 8 * (int)(j / R) + xcd, rt = (int)(j % R);
  if (qt >= Q) return;
  const int lane = threadIdx.x & 63;
  const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = q_lo + qt * 64 + lane;
  const bool live = q < q_hi;
  const double* wq = W + (live ? q : q_lo);
  const int r0 = rt * 16 + 4 * g;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + i;
    if (r >= m) break;
    const long t0 = pc_ptr[r], t1 = pc_ptr[r + 1];
    for (long t = t0; t < t1; t += 4) {
      double w[4], v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = t + k < t1;
        v[k] = ok ? Mv[t + k] : 0.0;
        w[k] = wq[(long)pc_r[ok ? t + k : t] * m];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[i] += v[k] * w[k];
    }
  }
  if (!live) return;
  double* dst = N + (long)q * m + r0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (r0 + i < m) dst[i] = acc[i];
}

// ---- the same operator for matrices that sit in L2 (msz < 1500: thetaG11, msz 801, 3 % of the entries of M stored) --
// round 3.  There the dense route costs two msz^3 products and three passes over msz^2 (97 us per mat-vec at msz 801)
// for 2 x 2 nnz(M) msz flop of useful work.  The gather and the symmetrisation are one launch (one wave per stored
// entry, both halves of (M + M') / 2), N = M W requests its W values ahead of their use, and Z[p, q] = W(:, p) . N(:, q)
// takes ONE WAVE per stored entry (sp_dot_wave_kernel, at every size).
__global__ __launch_bounds__(256) void sp_gather_sym_kernel(const long* __restrict__ cq_ptr, const int* __restrict__ cq_j,
                                                            const double* __restrict__ cq_v, const int* __restrict__ pc_t,
                                                            long ncq, const double* __restrict__ x, double* __restrict__ Mv) {
  // one wave per stored entry (a position can be shared by every constraint: thetaG11's corner entry by 1600)
  const int lane = threadIdx.x & 63;
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= ncq) return;
  const long u = pc_t[t];
  double a = 0.0, b = 0.0;
  for (long k = cq_ptr[t] + lane; k < cq_ptr[t + 1]; k += 64) a += cq_v[k] * x[cq_j[k]];
  if (u != t)
    for (long k = cq_ptr[u] + lane; k < cq_ptr[u + 1]; k += 64) b += cq_v[k] * x[cq_j[k]];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
  // (raw[t] + raw[twin]) / 2 in a fixed order: the twins get the same bits
  if (lane == 0) Mv[t] = (u == t) ? (a + a) / 2.0 : (t < u ? a + b : b + a) / 2.0;
}

// N[r, q] for 4 consecutive r per workgroup, one thread per q; the W values of up to 8 stored entries are requested
// before they are used (one workgroup per CU at this size: nothing else hides the L2 latency).  Columns with more than
// SP_LONG stored entries (thetaG11: one column of 801 among columns of 7) are left to sp_wm_long_kernel.
static constexpr int SP_LONG = 64;
__global__ __launch_bounds__(256) void sp_wm_small_kernel(const long* __restrict__ pc_ptr, const int* __restrict__ pc_r,
                                                          const double* __restrict__ Mv, const double* __restrict__ W, int m,
                                                          int q_lo, int q_hi, double* __restrict__ N) {
  const int q = q_lo + blockIdx.y * 256 + threadIdx.x;
  const int r0 = blockIdx.x * 4;
  const bool live = q < q_hi;
  const double* wq = W + (live ? q : q_lo);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + i;
    if (r >= m) break;
    const long t0 = pc_ptr[r], t1 = pc_ptr[r + 1];
    if (t1 - t0 > SP_LONG) continue;
    for (long t = t0; t < t1; t += 8) {
      double w[8], v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool ok = t + k < t1;
        v[k] = ok ? Mv[t + k] : 0.0;
        w[k] = wq[(long)pc_r[ok ? t + k : t] * m];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[i] += v[k] * w[k];
    }
  }
  if (!live) return;
  double* dst = N + (long)q * m + r0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (r0 + i < m) {
      const long cnt = pc_ptr[r0 + i + 1] - pc_ptr[r0 + i];
      if (cnt <= SP_LONG) dst[i] = acc[i];
    }
}

// N[r, q] of a long column r: one wave per q, the lanes over the stored entries (W(:, q) read at the rows of the
// entries -- ascending, nearly contiguous)
__global__ __launch_bounds__(256) void sp_wm_long_kernel(const long* __restrict__ pc_ptr, const int* __restrict__ pc_r,
                                                         const double* __restrict__ Mv, const double* __restrict__ W, int m,
                                                         int r, int q_lo, int q_hi, double* __restrict__ N) {
  const int lane = threadIdx.x & 63;
  const int q = q_lo + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= q_hi) return;
  const double* wq = W + (long)q * m;
  double s = 0.0;
  for (long t = pc_ptr[r] + lane; t < pc_ptr[r + 1]; t += 64) s += Mv[t] * wq[pc_r[t]];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) N[(long)q * m + r] = s;
}

// Zs[t] = W(:, p_t) . N(:, q_t) for the stored entries t with q_lo <= q_t < q_hi, one wave each; mirror: only p <= q is
// computed and copied to the transposed entry (Z is symmetric)
__global__ __launch_bounds__(256) void sp_dot_wave_kernel(const long* __restrict__ cq_q, const int* __restrict__ pc_t, long ncq,
                                                          const double* __restrict__ W, const double* __restrict__ N, int m,
                                                          int q_lo, int q_hi, int mirror, double* __restrict__ Zs) {
  const int lane = threadIdx.x & 63;
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= ncq) return;
  const long key = cq_q[t];
  const int q = (int)(key / m), p = (int)(key % m);
  if (q < q_lo || q >= q_hi || (mirror && p > q)) return;
  const double* wp = W + (long)p * m;
  const double* nq = N + (long)q * m;
  double s = 0.0;
  for (int i = lane; i < m; i += 64) s += wp[i] * nq[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) {
    Zs[t] = s;
    if (mirror && p != q) Zs[pc_t[t]] = s;
  }
}

// out[sigma[p]] -= sum_e a_e Zs[ent_t[e]]   (entries with column in [c_lo, c_hi))
__global__ __launch_bounds__(256) void sp_aa_times_kernel(const long* __restrict__ ptr, const int* __restrict__ ec,
                                                          const double* __restrict__ ev, const int* __restrict__ ent_t,
                                                          const double* __restrict__ Zs, int c_lo, int c_hi, int p_end,
                                                          const int* __restrict__ sigma, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= p_end) return;
  double s = 0.0;
  for (long e = ptr[p] + lane; e < ptr[p + 1]; e += 64) {
    const int cc = ec[e];
    if (cc >= c_lo && cc < c_hi) s += ev[e] * Zs[ent_t[e]];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) out[sigma[p]] -= s;
}

// ---- the route of the passes over the dense constraint data of a block
// Decided once, where Adense is filled (lrn_upload_model, lrn_synthetic_dense_model); freeing the model resets it.  Data
// that are a stream -- msz even (16-byte pairs), msz >= 256, Adense 16-byte aligned -- take the tri tier when every matrix
// is exactly symmetric (checked here on the device unless sym_known; the chunk table of the column tails is built with
// it), else the stream tier; everything else the scalar tier, at no cost here.
int dense_route_setup(lrn_ctx* c, LmiBlock& b, bool sym_known) {
  b.dense_route = LmiBlock::DENSE_SCALAR;
  b.tri_nch = 0;
  if (b.nd <= 0 || (b.msz & 1) != 0 || b.msz < 256 || ((uintptr_t)b.Adense.p & 15) != 0) return LRN_OK;
  b.dense_route = LmiBlock::DENSE_STREAM;
  if (!sym_known) {
    LRN_TRY(ensure(c, c->info_dev, 64));
    LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 4, c->stream));
    hipLaunchKernelGGL(dense_sym_check_kernel, dim3(b.nd), dim3(256), 0, c->stream, b.Adense.as<double>(), b.msz,
                       c->info_dev.as<int>());
    int f = 1;
    LRN_TRY(copy_out(c, &f, c->info_dev.p, 4));
    LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 4, c->stream));
    if (f != 0) return LRN_OK;
  }
  const int m = b.msz;
  std::vector<TriChunk> tab;
  for (int j = 0; j < m; ++j) {
    const int r0 = j & ~15;
    for (int r = r0; r < m; r += 128) tab.push_back({(long)j * m + r, j, std::min(64, (m - r) / 2)});
  }
  LRN_TRY(ensure(c, b.tri_tab, tab.size() * sizeof(TriChunk)));
  LRN_TRY(copy_in(c, b.tri_tab.p, tab.data(), tab.size() * sizeof(TriChunk)));
  b.tri_nch = (int)tab.size();
  b.dense_route = LmiBlock::DENSE_TRI;
  return LRN_OK;
}

// the tier of one pass: the block's route, except that the stream tier reads (writes) the matrices p1, p2 it is given by
// 16-byte pairs as well -- a misaligned one takes the scalar tier (the tri tier reads its own weight workspace)
static LmiBlock::DenseRoute dense_route(const LmiBlock& b, const double* p1, const double* p2 = nullptr) {
  if (b.dense_route == LmiBlock::DENSE_STREAM && (((uintptr_t)p1 | (uintptr_t)p2) & 15) != 0) return LmiBlock::DENSE_SCALAR;
  return b.dense_route;
}

// w = tri-weights of Z into slot `which` of the block's weight workspace
static int tri_weights(lrn_ctx* c, LmiBlock& b, const double* Z, int which, double** out) {
  const int m = b.msz;
  LRN_TRY(ensure(c, c->triw, (size_t)2 * m * m * 8));
  double* Wt = c->triw.as<double>() + (size_t)which * m * m;
  hipLaunchKernelGGL(tri_weights_kernel, dim3((m + 31) / 32, (m + 31) / 32), dim3(32, 8), 0, c->stream, Z, m, Wt);
  *out = Wt;
  return LRN_OK;
}

// out1[sigma[p]] -= <Adense[p], Z1> for the dense positions [p0, p1) (and out2 / Z2 in the same pass; Z2 null: NZ = 1)
static int dense_dots(lrn_ctx* c, LmiBlock& b, int p0, int p1, const double* Z1, const double* Z2, double* out1,
                      double* out2) {
  const long mm = (long)b.msz * b.msz;
  const int np = p1 - p0;
  const double* Ap0 = b.Adense.as<double>() + (long)p0 * mm;
  const int* sg = b.sigma_d.as<int>() + p0;
  hipStream_t st = c->stream;
  switch (dense_route(b, Z1, Z2)) {
    case LmiBlock::DENSE_TRI: {
      c->counts["op_dense_tri"] += 1;
      double *W1 = nullptr, *W2 = nullptr;
      LRN_TRY(tri_weights(c, b, Z1, 0, &W1));
      if (Z2) {
        LRN_TRY(tri_weights(c, b, Z2, 1, &W2));
        hipLaunchKernelGGL(aa_dense_tri_dot4_kernel<2>, dim3((np + 3) / 4), dim3(256), 0, st, Ap0, mm, np, W1, W2,
                           b.tri_tab.as<TriChunk>(), b.tri_nch, sg, out1, out2);
      } else
        hipLaunchKernelGGL(aa_dense_tri_dot4_kernel<1>, dim3((np + 3) / 4), dim3(256), 0, st, Ap0, mm, np, W1, W1,
                           b.tri_tab.as<TriChunk>(), b.tri_nch, sg, out1, out1);
      break;
    }
    case LmiBlock::DENSE_STREAM:
      c->counts["op_dense_stream"] += 1;
      if (Z2) hipLaunchKernelGGL(aa_dense_dot4x2_kernel, dim3((np + 3) / 4), dim3(256), 0, st, Ap0, mm, np, Z1, Z2, sg, out1, out2);
      else hipLaunchKernelGGL(aa_dense_dot4_kernel, dim3((np + 3) / 4), dim3(256), 0, st, Ap0, mm, np, Z1, sg, out1);
      break;
    case LmiBlock::DENSE_SCALAR:
      c->counts["op_dense_scalar"] += 1;
      if (Z2) hipLaunchKernelGGL(aa_dense_dot_kernel<2>, dim3(np), dim3(256), 0, st, Ap0, mm, Z1, Z2, sg, out1, out2);
      else hipLaunchKernelGGL(aa_dense_dot_kernel<1>, dim3(np), dim3(256), 0, st, Ap0, mm, Z1, Z1, sg, out1, out1);
      break;
  }
  return LRN_OK;
}

// Tm -= sum_{p0 <= p < p1} x[sigma[p]] Adense[p]; tri tier: the lower triangle of Tm only (the caller mirrors it)
static void dense_accumulate(lrn_ctx* c, LmiBlock& b, int p0, int p1, const double* x, double* Tm) {
  const int m = b.msz;
  const long mm = (long)m * m;
  const double* Ap0 = b.Adense.as<double>() + (long)p0 * mm;
  const int* sg = b.sigma_d.as<int>() + p0;
  switch (dense_route(b, Tm)) {
    case LmiBlock::DENSE_TRI:
      c->counts["op_dense_tri"] += 1;
      hipLaunchKernelGGL(aat_dense_tri_kernel, dim3((unsigned)((b.tri_nch + 3) / 4)), dim3(256), 0, c->stream, Ap0, p1 - p0,
                         mm, m, sg, x, b.tri_tab.as<TriChunk>(), b.tri_nch, Tm);
      break;
    case LmiBlock::DENSE_STREAM:
      c->counts["op_dense_stream"] += 1;
      hipLaunchKernelGGL(aat_dense2_kernel, dim3((unsigned)((mm / 2 + 255) / 256)), dim3(256), 0, c->stream, Ap0, p1 - p0, mm,
                         sg, x, Tm);
      break;
    case LmiBlock::DENSE_SCALAR:
      c->counts["op_dense_scalar"] += 1;
      hipLaunchKernelGGL(aat_dense_kernel, dim3(nb(mm)), dim3(256), 0, c->stream, Ap0, p1 - p0, mm, sg, x, Tm);
      break;
  }
}

bool use_sparse_matvec(const lrn_ctx* c, const LmiBlock& b) {
  if (b.factored) return false;        // (no stored column of AA to walk: the data are the factors)
  if (!b.sp_ok || c->opt.matvec_sparse == 1) return false;
  if (c->opt.matvec_sparse == 2) return true;
  // ~4e-12 ncq msz s against 4 msz^3 / 6e13 s.  Below msz ~ 1500 both routes are bound by their launches and L2: the
  // wave-per-entry kernels win where a twelfth of M or less is stored
  if (b.msz < 1500)
    return b.msz >= 256 && (double)b.ncq * 12.0 < (double)b.msz * (double)b.msz && b.sp_long_cols.size() <= 4;
  return (double)b.ncq * 60.0 < (double)b.msz * (double)b.msz;
}

// y += AA vec(W mat(AA'x) W) restricted to the pattern columns [q_lo, q_hi) of Z
static int matvec_sparse_block(lrn_ctx* c, LmiBlock& b, const double* x, double* y, int q_lo, int q_hi, bool mirror) {
  const int m = b.msz;
  hipStream_t st = c->stream;
  c->counts["op_sparse_pattern"] += 1;
  LRN_TRY(ensure(c, c->m1, (size_t)m * m * 8));
  double* N = c->m1.as<double>();
  const bool small = m < 1500;        // W and N sit in L2: one wave per stored entry (see sp_dot_wave_kernel)
  if (small) {
    hipLaunchKernelGGL(sp_gather_sym_kernel, dim3((unsigned)((b.ncq + 3) / 4)), dim3(256), 0, st, b.cq_ptr.as<long>(),
                       b.cq_j.as<int>(), b.cq_v.as<double>(), b.pc_t.as<int>(), b.ncq, x, b.Mv.as<double>());
  } else {
    hipLaunchKernelGGL(sp_gather_kernel, dim3((unsigned)((b.ncq + 3) / 4)), dim3(256), 0, st, b.cq_ptr.as<long>(),
                       b.cq_j.as<int>(), b.cq_v.as<double>(), b.ncq, x, b.Zs.as<double>());
    hipLaunchKernelGGL(sp_symmetrize_kernel, dim3((unsigned)((b.ncq + 255) / 256)), dim3(256), 0, st, b.Zs.as<double>(),
                       b.pc_t.as<int>(), b.ncq, b.Mv.as<double>());
  }
  if (q_hi > q_lo) {
    if (small) {
      hipLaunchKernelGGL(sp_wm_small_kernel, dim3((m + 3) / 4, (q_hi - q_lo + 255) / 256), dim3(256), 0, st,
                         b.pc_ptr.as<long>(), b.pc_r.as<int>(), b.Mv.as<double>(), b.W.as<double>(), m, q_lo, q_hi, N);
      for (int r : b.sp_long_cols)
        hipLaunchKernelGGL(sp_wm_long_kernel, dim3((q_hi - q_lo + 3) / 4), dim3(256), 0, st, b.pc_ptr.as<long>(),
                           b.pc_r.as<int>(), b.Mv.as<double>(), b.W.as<double>(), m, r, q_lo, q_hi, N);
    } else {
      const long R = (m + 15) / 16, Q8 = ((q_hi - q_lo + 63) / 64 + 7) / 8;
      if (8 * Q8 * R >= 0x7fffffffL)      // (msz ~ 1.5e6)
        return set_error(c, LRN_ERR_ARG, "pattern-restricted mat-vec: msz %d needs more workgroups than one launch holds", m);
      hipLaunchKernelGGL(sp_wm_xcd_kernel, dim3((unsigned)(8 * Q8 * R)), dim3(256), 0, st, b.pc_ptr.as<long>(),
                         b.pc_r.as<int>(), b.Mv.as<double>(), b.W.as<double>(), m, q_lo, q_hi, N);
    }
    // one wave per stored entry at every size (round 3)
    hipLaunchKernelGGL(sp_dot_wave_kernel, dim3((unsigned)((b.ncq + 3) / 4)), dim3(256), 0, st, b.cq_q.as<long>(),
                       b.pc_t.as<int>(), b.ncq, b.W.as<double>(), N, m, q_lo, q_hi, mirror ? 1 : 0, b.Zs.as<double>());
    hipLaunchKernelGGL(sp_aa_times_kernel, dim3((b.npos_nz + 3) / 4), dim3(256), 0, st, b.ent_ptr.as<long>(),
                       b.ent_c.as<int>(), b.ent_v.as<double>(), b.ent_t.as<int>(), b.Zs.as<double>(), q_lo, q_hi, b.npos_nz,
                       b.sigma_d.as<int>(), y);
  }
  return LRN_OK;
}

__global__ void vec_add_kernel(double* __restrict__ y, const double* __restrict__ t, long n) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) y[e] += t[e];
}

// multi-GPU: are the passes over the dense constraint matrices split over the ranks?  (communicator present, enough dense
// constraints for every rank; option "shard_passes" = 0 keeps them replicated)
static bool dense_passes_sharded(lrn_ctx* c, const LmiBlock& b) {
  return c->comm && c->world > 1 && c->opt.shard_passes != 0 && b.nd >= 8 * c->world;
}

int wmw(lrn_ctx* c, LmiBlock& b, double* M, double* P, double* Z) {
  const int m = b.msz;
  if (products_sharded(c, c->stream, m)) {      // P = W M' (M symmetric), Z = P W' (W symmetric): column blocks + all-gather
    LRN_TRY(pgemm_nt(c, c->stream, m, b.W.as<double>(), M, P));
    return pgemm_nt_sym(c, c->stream, m, P, b.W.as<double>(), Z);
  }
  GemmDesc g1;     // P = W M   (M symmetric: read as M[n + k*m] -> direct-to-LDS path)
  g1.A = b.W.as<double>(); g1.sAm = 1; g1.sAk = m;
  g1.B = M; g1.sBk = m; g1.sBn = 1;
  g1.C = P; g1.sCm = 1; g1.sCn = m;
  g1.M = g1.N = g1.K = m;
  LRN_TRY(gemm(c->stream, g1));
  if (m >= 1500) return gemm_nt_sym(c->stream, m, P, b.W.as<double>(), Z);      // Z = P W symmetric: lower tiles + mirror
  GemmDesc g2;     // Z = P W   (W symmetric)
  g2.A = P; g2.sAm = 1; g2.sAk = m;
  g2.B = b.W.as<double>(); g2.sBk = m; g2.sBn = 1;
  g2.C = Z; g2.sCm = 1; g2.sCn = m;
  g2.M = g2.N = g2.K = m;
  return gemm(c->stream, g2);
}

// AA vec(W M W) for a dense symmetric M when every constraint of the block is sparse (C5: 9 entries each): the entries
// of Z = W M W are needed on the pattern of the constraints only -- N = M W is one product, Z[p,q] = W(:,p) . N(:,q) one
// wave per stored entry (sp_dot_wave_kernel, sp_aa_times_kernel of the pattern-restricted CG operator) -- instead of the second n^3 product.
bool wmw_pattern_ok(const lrn_ctx* c, const LmiBlock& b) {
  return !b.factored && b.sp_ok && b.nd == 0 && b.msz >= c->opt.wmw_pattern_min && b.have_W;
}

int aa_times_wmw_pattern(lrn_ctx* c, LmiBlock& b, const double* M, double* N, double* y) {
  const int m = b.msz;
  c->counts["op_wmw_pattern"] += 1;
  LRN_TRY(pgemm_nt(c, c->stream, m, M, b.W.as<double>(), N));                   // N = M W' = M W
  hipLaunchKernelGGL(sp_dot_wave_kernel, dim3((unsigned)((b.ncq + 3) / 4)), dim3(256), 0, c->stream, b.cq_q.as<long>(),
                     b.pc_t.as<int>(), b.ncq, b.W.as<double>(), N, m, 0, m, 1, b.Zs.as<double>());
  hipLaunchKernelGGL(sp_aa_times_kernel, dim3((b.npos_nz + 3) / 4), dim3(256), 0, c->stream, b.ent_ptr.as<long>(),
                     b.ent_c.as<int>(), b.ent_v.as<double>(), b.ent_t.as<int>(), b.Zs.as<double>(), 0, m, b.npos_nz,
                     b.sigma_d.as<int>(), y);
  return LRN_OK;
}

int ensure_m(lrn_ctx* c, int m) {
  size_t mm = (size_t)m * m * 8;
  LRN_TRY(ensure(c, c->m0, mm));
  LRN_TRY(ensure(c, c->m1, mm));
  LRN_TRY(ensure(c, c->m2, mm));
  return LRN_OK;
}

// ---- factor form of the two data operators (factored blocks, lrn_set_factored): A_k = V_k diag(d_k) V_k' exists only as the
// dense factor matrix Vd (msz x R, R = nvar khat, column h khat + p = column p of the constraint with H index h) and the
// weights w (d, 0 in the padding).  With AA = -A:
//     (AA vec(Z))_k = -sum_p w_kp v_kp' Z v_kp          Q = Z Vd by one FP64 MFMA product, then per column <Q_c, Vd_c>
//     mat(AA' x)    = -Vd diag(w o (x (x) 1_khat)) Vd'   columns scaled into a workspace, one lower-triangle product, mirrored
// Q and the scaled copy live in the BG workspace (msz x R, what the mode-1 assembly uses for U).  Every sum has a fixed
// order: one wave per constraint walks its khat columns in order, lanes stride the rows, one shuffle tree -- no atomics.
// A hybrid block adds the rows of its few stored constraints through the stored-entry kernels (aa_times_impl,
// aat_to_mat_impl); their factor columns have weight 0 and contribute nothing here.

// out[nat(h)] -= sum_p w[col] <Q(:, col), V(:, col)> over the columns col of unit u of the layout (fac_cols.h), h its H index
// (sigma: H index -> constraint, null = identity): one wave per unit
template <class Cols>
__global__ __launch_bounds__(256) void fac_coldot_kernel(const double* __restrict__ Q, const double* __restrict__ V,
                                                         const double* __restrict__ w, int m, Cols lay,
                                                         const int* __restrict__ sigma, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
  typename Cols::Span span;
  int cnt;
  if (!lay.unit(u, &span, &cnt)) return;
  double s = 0.0;
  for (int p = 0; p < cnt; ++p) {
    const long col = lay.col(span, p);
    const double wp = w[col];
    if (wp == 0.0) continue;                       // padding column (wave-uniform)
    const double* __restrict__ q = Q + col * m;
    const double* __restrict__ v = V + col * m;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
    int r = lane;
    for (; r + 192 < m; r += 256) {
      t0 += q[r] * v[r];
      t1 += q[r + 64] * v[r + 64];
      t2 += q[r + 128] * v[r + 128];
      t3 += q[r + 192] * v[r + 192];
    }
    for (; r < m; r += 64) t0 += q[r] * v[r];
    s += wp * ((t0 + t1) + (t2 + t3));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane != 0) return;
  const int h = lay.unit_h(u, span);
  out[sigma ? sigma[h] : h] -= s;
}

// Vs(:, c) = -w[c] x[nat(c / kh)] Vd(:, c)   (one workgroup per factor column)
__global__ __launch_bounds__(256) void fac_scale_kernel(const double* __restrict__ Vd, const double* __restrict__ w,
                                                        const double* __restrict__ x, const int* __restrict__ sigma, int m,
                                                        int kh, double* __restrict__ Vs) {
  const long col = blockIdx.x;
  const int h = (int)(col / kh);
  const double sc = -(w[col] * x[sigma ? sigma[h] : h]);
  const double* __restrict__ v = Vd + col * m;
  double* __restrict__ o = Vs + col * m;
  for (int r = threadIdx.x; r < m; r += 256) o[r] = sc * v[r];
}

static int fac_workspace(lrn_ctx* c, LmiBlock& b, double** ws) {
  if (!b.have_Vd || !b.has_V) return set_error(c, LRN_ERR_STATE, "factored block without factors (lrn_upload_lowrank)");
  LRN_TRY(ensure(c, c->BG, (size_t)b.msz * (size_t)c->nvar * b.lr_khat * 8));
  *ws = c->BG.as<double>();
  return LRN_OK;
}

// y += AA vec(Z), Z symmetric: Q = Z V by the product every route uses, then the column dots -- or, fused (option
// "fac_quadform", the CG operator only), the quadratic form of facops.hip, Q never stored.  V is Vd, or under option
// "ragged_ops" the compacted columns Vc of a block of mixed ranks (the conditions of the rank-class assembly; a uniform block,
// an empty one and a sharded run keep the padded columns)
static int aa_times_factored(lrn_ctx* c, LmiBlock& b, const double* Z, double* y, bool fused = false) {
  const int m = b.msz;
  const bool rg = ragged_ops_on(c, b);
  if (c->opt.ragged_ops && !rg) c->counts["ragged_ops_fallback"] += 1;
  if (!b.have_Vd || !b.has_V) return set_error(c, LRN_ERR_STATE, "factored block without factors (lrn_upload_lowrank)");
  if (rg) LRN_TRY(ragged_setup(c, b));
  const FacCols v = fac_cols(c, b, rg);
  const int* sigma = c->pos_space ? b.sigma_d.as<int>() : (const int*)nullptr;
  if (fused) {
    LRN_TRY(fac_quadform(c, b, v, Z, sigma, y));
  } else {
    LRN_TRY(ensure(c, c->BG, (size_t)m * v.R * 8));
    double* Q = c->BG.as<double>();
    LRN_TRY(cols_product(c, Z, false, v.V, v.R, m, Q));
    with_layout(c, b, v, [&](auto lay) {
      hipLaunchKernelGGL(fac_coldot_kernel<decltype(lay)>, dim3((v.nunit + 3) / 4), dim3(256), 0, c->stream, Q, v.V, v.w, m, lay,
                         sigma, y);
    });
  }
  c->counts["op_factored"] += 1;
  if (rg) c->counts["op_ragged"] += 1;
  return LRN_OK;
}

// M = mat(AA' x) = -F diag(w o x) F' with F = Vd, exactly symmetric.  F = Y = W Vd (option "fac_op_scaled") gives W mat(AA' x) W
static int aat_to_mat_factored(lrn_ctx* c, LmiBlock& b, const double* x, double* M, const double* F = nullptr) {
  const int m = b.msz, kh = b.lr_khat;
  const long R = (long)c->nvar * kh;
  if (c->opt.ragged_ops) {      // (as in aa_times_factored; F is then Yc = W Vc of fac_scaled_y, or null)
    if (ragged_ops_on(c, b)) {
      if (!b.have_Vd || !b.has_V) return set_error(c, LRN_ERR_STATE, "factored block without factors (lrn_upload_lowrank)");
      if (F && F != b.Yc.as<double>()) return set_error(c, LRN_ERR_STATE, "ragged_ops: scaled factors in the padded layout");
      int ks = 1;
      LRN_TRY(aat_to_mat_ragged(c, b, x, M, F, &ks));
      if (ks == 1)
        hipLaunchKernelGGL(mirror_lower_tiled_kernel, dim3((m + 31) / 32, (m + 31) / 32), dim3(32, 8), 0, c->stream, M, m);
      return LRN_OK;
    }
    c->counts["ragged_ops_fallback"] += 1;
  }
  double* Vs = nullptr;
  LRN_TRY(fac_workspace(c, b, &Vs));
  if (!F) F = b.Vd.as<double>();
  hipLaunchKernelGGL(fac_scale_kernel, dim3((unsigned)R), dim3(256), 0, c->stream, F, b.v_w.as<double>(), x,
                     c->pos_space ? b.sigma_d.as<int>() : (const int*)nullptr, m, kh, Vs);
  GemmDesc g;     // M = Vs F', the tiles on and below the diagonal
  g.A = Vs; g.sAm = 1; g.sAk = m;
  g.B = F; g.sBk = m; g.sBn = 1;
  g.C = M; g.sCm = 1; g.sCn = m;
  g.M = m; g.N = m; g.K = (int)R;
  g.flags = GEMM_TRI_LOWER;
  // From 16 x 16 128-tiles on gemm() no longer splits K by itself, but the lower triangle alone (msz 2000: 136 tiles on 512
  // workgroup slots) leaves most of the chip idle over a long K = R.  K is cut into ks equal parts run as a BATCH of the
  // same kernel into ks slabs, added in a fixed order.  ks by the round model of gemm_f64.hip (1.85 us per K-step of a
  // round of 512 workgroups, 1.25 / 2 for a round of up to 256 / 512) plus the pass over the slabs.
  const long tm = (m + 127) / 128, tiles = tm * (tm + 1) / 2;
  int ks = 1;
  static const int forced = getenv("LRN_FAC_SPLIT") ? atoi(getenv("LRN_FAC_SPLIT")) : 0;      // (measurement: ks, 1 = none)
  if (forced >= 1 && forced <= 16 && R % forced == 0) ks = forced;
  else if (tm * tm >= 256 && tiles < 512) {
    double best = 1e300;
    for (int k : {1, 2, 3, 4, 5, 6, 8}) {
      if (R % k || (k > 1 && R / k < 512)) continue;
      const long wg = tiles * k, rem = wg % 512;
      const double rounds = 2.0 * (double)(wg / 512) + (rem == 0 ? 0.0 : (rem <= 256 ? 1.25 : 2.0));
      const double us = (double)(R / k) / 16.0 * 1.85 * rounds + (k > 1 ? 5.0 + (double)(k + 1) * m * (double)m * 8.0 / 4.0e6 : 0.0);
      if (us < best) { best = us; ks = k; }
    }
  }
  if (ks > 1) {
    const long mm = (long)m * m;
    LRN_TRY(ensure(c, c->slabs, (size_t)ks * mm * 8));
    g.C = c->slabs.as<double>();
    g.K = (int)(R / ks);
    g.batch = ks;
    g.bA = (long)(R / ks) * m; g.bB = (long)(R / ks) * m; g.bC = mm;
    LRN_TRY(gemm(c->stream, g));
    LRN_TRY(reduce_slabs(c->stream, c->slabs.as<double>(), mm, ks, M, mm, 0.0));
  } else {
    LRN_TRY(gemm(c->stream, g));
  }
  hipLaunchKernelGGL(mirror_lower_tiled_kernel, dim3((m + 31) / 32, (m + 31) / 32), dim3(32, 8), 0, c->stream, M, m);
  c->counts["op_factored"] += 1;
  return LRN_OK;
}

// option "profile_ops": one data operator between two events of its own (the phases of the resident loop -- "rhs",
// "residual_d", "find_step" -- contain other products as well), counted whatever it returns
static int op_timed(PhaseTimer& t, const char* key, int rc) {
  t.stop(key);
  return rc;
}

static int aa_times_impl(lrn_ctx* c, LmiBlock& b, const double* Z, double* y, bool factor_form = false, bool fused = false);
static int aa_times2_impl(lrn_ctx* c, LmiBlock& b, const double* Z1, double* y1, const double* Z2, double* y2);
static int aat_to_mat_impl(lrn_ctx* c, LmiBlock& b, const double* x, double* M, bool factor_form = false);
// factor_form (the CG operator under option "cg_lowrank", matvec_dev): a block that is NOT factored goes through its factors
// all the same -- they cover every constraint (cg_lowrank_covered), so the entries are left alone.  A parameter of the call:
// every other caller keeps the entries of such a block
// fused (option "fac_quadform", matvec_dev only): the factor part of a factored block by the fused quadratic form
int aa_times(lrn_ctx* c, LmiBlock& b, const double* Z, double* y, bool factor_form, bool fused) {
  PhaseTimer t(c, c->opt.profile_ops);
  return op_timed(t, "aa_times", aa_times_impl(c, b, Z, y, factor_form, fused));
}
int aa_times2(lrn_ctx* c, LmiBlock& b, const double* Z1, double* y1, const double* Z2, double* y2) {
  PhaseTimer t(c, c->opt.profile_ops);
  return op_timed(t, "aa_times2", aa_times2_impl(c, b, Z1, y1, Z2, y2));
}
int aat_to_mat(lrn_ctx* c, LmiBlock& b, const double* x, double* M, bool factor_form) {
  PhaseTimer t(c, c->opt.profile_ops);
  return op_timed(t, "aat_to_mat", aat_to_mat_impl(c, b, x, M, factor_form));
}

// y += AA vec(Z)
static int aa_times_impl(lrn_ctx* c, LmiBlock& b, const double* Z, double* y, bool factor_form, bool fused) {
  if (factor_form && !b.factored) return aa_times_factored(c, b, Z, y);
  if (b.factored) LRN_TRY(aa_times_factored(c, b, Z, y, fused));      // (a hybrid block goes on with its stored rows; a pure one has none)
  if (b.factored && b.dg_n > 0) LRN_TRY(aa_times_diag(c, b, Z, y));   // (diagonal parts: disjoint from the stored rows, after the factor form)
  if (b.npos_nz > b.nd) c->counts["op_sparse"] += 1;
  if (b.nd > 0) c->counts["op_dense"] += 1;
  if (b.npos_nz > b.nd)
    hipLaunchKernelGGL(aa_times_kernel, dim3((b.npos_nz - b.nd + 3) / 4), dim3(256), 0, c->stream, b.ent_ptr.as<long>(),
                       b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(), Z, b.msz, b.nd, b.npos_nz,
                       b.sigma_d.as<int>(), y);
  if (b.nd <= 0) return LRN_OK;
  if (!dense_passes_sharded(c, b)) return dense_dots(c, b, 0, b.nd, Z, nullptr, y, y);
  // one process per GPU: every pass over the dense constraint data (128 GB at C4, six of them per IP iteration in the
  // replicated part of the loop) is split by constraints; the nvar-vector of partial results is summed by one all-reduce
  // on the library's stream
  const int per = (b.nd + c->world - 1) / c->world;
  const int p0 = std::min(b.nd, c->rank * per), p1 = std::min(b.nd, p0 + per);
  LRN_TRY(ensure(c, c->commvec, (size_t)c->nvar * 8));
  double* part = c->commvec.as<double>();
  LRN_HIP(c, hipMemsetAsync(part, 0, (size_t)c->nvar * 8, c->stream));
  if (p1 > p0) LRN_TRY(dense_dots(c, b, p0, p1, Z, nullptr, part, part));
  LRN_TRY(comm_allreduce(c, part, c->nvar, 0));
  hipLaunchKernelGGL(vec_add_kernel, dim3(nb(c->nvar)), dim3(256), 0, c->stream, y, part, c->nvar);
  return LRN_OK;
}

// y1 += AA vec(Z1), y2 += AA vec(Z2) with the dense constraint data read once (C4: 128 GB per pass)
static int aa_times2_impl(lrn_ctx* c, LmiBlock& b, const double* Z1, double* y1, const double* Z2, double* y2) {
  if (b.factored || b.nd <= 0 || dense_passes_sharded(c, b)) {      // (the sharded pass is 1/world of the data already; factor form: two products)
    LRN_TRY(aa_times_impl(c, b, Z1, y1));
    return aa_times_impl(c, b, Z2, y2);
  }
  c->counts["op_dense"] += 1;
  if (b.npos_nz > b.nd) {
    c->counts["op_sparse"] += 1;
    for (int h = 0; h < 2; ++h)
      hipLaunchKernelGGL(aa_times_kernel, dim3((b.npos_nz - b.nd + 3) / 4), dim3(256), 0, c->stream, b.ent_ptr.as<long>(),
                         b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(), h ? Z2 : Z1, b.msz, b.nd, b.npos_nz,
                         b.sigma_d.as<int>(), h ? y2 : y1);
  }
  return dense_dots(c, b, 0, b.nd, Z1, Z2, y1, y2);
}

// M = mat(AA' x)  (symmetrised msz x msz, kron_etc.jl:13-18)
static int aat_to_mat_stored(lrn_ctx* c, LmiBlock& b, const double* x, double* M);
static int aat_to_mat_impl(lrn_ctx* c, LmiBlock& b, const double* x, double* M, bool factor_form) {
  if (factor_form && !b.factored) return aat_to_mat_factored(c, b, x, M);
  if (!b.factored) return aat_to_mat_stored(c, b, x, M);
  LRN_TRY(aat_to_mat_factored(c, b, x, M));
  if (b.dg_n > 0) LRN_TRY(aat_to_mat_diag(c, b, x, M));      // (diagonal parts: the diagonal of M only)
  if (!b.hybrid()) return LRN_OK;
  // hybrid: the stored rows through the stored-entry kernels into a matrix of their own, then one elementwise sum -- both
  // terms are exactly symmetric, so the sum is
  const long mm = (long)b.msz * b.msz;
  LRN_TRY(ensure(c, c->facM, (size_t)mm * 8));
  LRN_TRY(aat_to_mat_stored(c, b, x, c->facM.as<double>()));
  hipLaunchKernelGGL(vec_add_kernel, dim3(nb(mm)), dim3(256), 0, c->stream, M, c->facM.as<double>(), mm);
  return LRN_OK;
}

// ... from the stored entries of AA: the sparse tier by stored columns, the dense slots by passes over Adense
static int aat_to_mat_stored(lrn_ctx* c, LmiBlock& b, const double* x, double* M) {
  const int m = b.msz;
  const long mm = (long)m * m;
  if (b.ncq > 0) c->counts["op_sparse"] += 1;
  if (b.nd > 0) c->counts["op_dense"] += 1;
  LRN_HIP(c, hipMemsetAsync(M, 0, (size_t)mm * 8, c->stream));
  if (b.ncq > 0)
    hipLaunchKernelGGL(aat_gather_kernel, dim3((unsigned)((b.ncq + 3) / 4)), dim3(256), 0, c->stream, b.cq_q.as<long>(),
                       b.cq_ptr.as<long>(), b.cq_j.as<int>(), b.cq_v.as<double>(), b.ncq, x, M);
  // symmetric dense data: the sparse part is symmetrised first, the dense constraints are added to the LOWER triangle only
  // (half the bytes of the pass) and the result is mirrored -- the same matrix up to the order of the additions
  const bool tri = b.nd > 0 && b.dense_route == LmiBlock::DENSE_TRI;
  if (tri && b.ncq > 0) symmetrize_dev(c->stream, M, m);
  if (b.nd > 0) {
    if (dense_passes_sharded(c, b)) {
      // this rank's constraints into a zeroed buffer, one all-reduce of the msz x msz partial sums, then added to M
      const int per = (b.nd + c->world - 1) / c->world;
      const int p0 = std::min(b.nd, c->rank * per), p1 = std::min(b.nd, p0 + per);
      LRN_TRY(ensure(c, c->commmat, (size_t)mm * 8));
      double* Tm = c->commmat.as<double>();
      LRN_HIP(c, hipMemsetAsync(Tm, 0, (size_t)mm * 8, c->stream));
      if (p1 > p0) dense_accumulate(c, b, p0, p1, x, Tm);
      LRN_TRY(comm_allreduce(c, Tm, mm, 0));
      hipLaunchKernelGGL(vec_add_kernel, dim3(nb(mm)), dim3(256), 0, c->stream, M, Tm, mm);
    } else
      dense_accumulate(c, b, 0, b.nd, x, M);
  }
  if (tri)
    hipLaunchKernelGGL(mirror_lower_tiled_kernel, dim3((m + 31) / 32, (m + 31) / 32), dim3(32, 8), 0, c->stream, M, m);
  else
    symmetrize_dev(c->stream, M, m);
  return LRN_OK;
}

// Y = W Vd of a pure factored block (option "fac_op_scaled"), once per NT scaling: with it
//     W mat(AA' x) W = -W Vd diag(w o x) Vd' W = -Y diag(w o x) Y',
// the scaled copy, lower-triangle product and mirror of aat_to_mat_factored on Y instead of Vd -- no W M W product
// Option "ragged_ops": Yc = W Vc (msz x Rc) instead.  fac_scaled_y (schur_factored.hip) forms and caches either; this is its
// timed and counted call from the operator -- nothing is counted while the cached product is current
static int fac_scaled_y_op(lrn_ctx* c, LmiBlock& b) {
  const bool rg = ragged_ops_on(c, b);
  if ((rg ? b.Yc_version : b.Ys_version) == c->scal_version && (rg ? b.Yc.p : b.Ys.p)) return LRN_OK;
  if (!b.have_Vd || !b.has_V) return set_error(c, LRN_ERR_STATE, "factored block without factors (lrn_upload_lowrank)");
  PhaseTimer t(c, c->opt.profile_ops);
  LRN_TRY(fac_scaled_y(c, b, rg));
  c->counts["fac_scaled_y"] += 1;
  t.stop("fac_scaled_y");
  return LRN_OK;
}

int matvec_dev(lrn_ctx* c, const double* x, double* y) {
  const int n = c->nvar;
  LRN_HIP(c, hipMemsetAsync(y, 0, (size_t)n * 8, c->stream));
  for (auto& b : c->lmi) {
    if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set");
    const int m = b.msz;
    // option "cg_factored": a factored block inside the CG operator.  Two routes are parameters of THIS call (every other
    // caller of aa_times / aat_to_mat keeps its route and bits): the scaled factors Y = W Vd of a pure block, and the fused
    // quadratic form for the factor part of AA vec(.) (a hybrid block's stored rows still go through aa_times_kernel)
    const bool fused = b.factored && fac_quadform_on(c, b);
    if (b.factored && fac_op_scaled_on(c, b)) {
      LRN_TRY(fac_scaled_y_op(c, b));
      LRN_TRY(ensure_m(c, m));
      double* N = c->m0.as<double>();
      {
        PhaseTimer t(c, c->opt.profile_ops);
        LRN_TRY(op_timed(t, "aat_to_mat", aat_to_mat_factored(c, b, x, N, ragged_ops_on(c, b) ? b.Yc.as<double>() : b.Ys.as<double>())));
      }
      LRN_TRY(aa_times(c, b, N, y, false, fused));
      c->counts["op_factored_scaled"] += 1;
      continue;
    }
    // option "cg_lowrank": both data operators of a covered block from its rank-k factors (Vd built on first use, as mode 1 does)
    const bool fac = cg_lowrank_operator(c, b);
    if (!fac && use_sparse_matvec(c, b)) {
      LRN_TRY(matvec_sparse_block(c, b, x, y, 0, m, true));
      continue;
    }
    if (fac) {
      LRN_TRY(lowrank_dense_factors(c, b));
      c->counts["op_factored_cg"] += 1;
    }
    LRN_TRY(ensure_m(c, m));
    double* M = c->m0.as<double>();
    LRN_TRY(aat_to_mat(c, b, x, M, fac));
    LRN_TRY(wmw(c, b, M, c->m1.as<double>(), c->m2.as<double>()));
    LRN_TRY(aa_times(c, b, c->m2.as<double>(), y, fac, fused));
  }
  if (c->nlin > 0) LRN_TRY(lin_matvec(c, x, y));
  LRN_HIP(c, hipGetLastError());
  return LRN_OK;
}

// Partial mat-vec of rank `rank` of `world`: rows R_g of Z = W M W (row blocks of msz/world),
// y_g = AA[:, idx(R_g)] vec(Z[R_g,:]); the caller all-reduces y_g over the ranks
// (one all-reduce of an nvar-vector per mat-vec).  The C_lin term is added by rank 0.
int matvec_partial_dev(lrn_ctx* c, const double* x, double* y, int rank, int world) {
  const int n = c->nvar;
  LRN_HIP(c, hipMemsetAsync(y, 0, (size_t)n * 8, c->stream));
  for (auto& b : c->lmi) {
    if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set");
    const int m = b.msz;
    const int per = (m + world - 1) / world;
    const int r0 = std::min(m, rank * per), r1 = std::min(m, r0 + per);
    if (r1 <= r0) continue;
    const int nr = r1 - r0;
    if (use_sparse_matvec(c, b)) {       // shard the pattern columns of Z instead of its rows
      LRN_TRY(matvec_sparse_block(c, b, x, y, r0, r1, false));
      continue;
    }
    LRN_TRY(ensure_m(c, m));
    double* M = c->m0.as<double>();
    LRN_TRY(aat_to_mat(c, b, x, M));              // replicated: sparse, cheap
    GemmDesc g1;                                  // P_g = W[R_g,:] M
    g1.A = b.W.as<double>() + r0; g1.sAm = 1; g1.sAk = m;
    g1.B = M; g1.sBk = m; g1.sBn = 1;             // M symmetric
    g1.C = c->m1.as<double>(); g1.sCm = 1; g1.sCn = nr;
    g1.M = nr; g1.N = m; g1.K = m;
    LRN_TRY(gemm(c->stream, g1));
    GemmDesc g2;                                  // Z_g = P_g W
    g2.A = c->m1.as<double>(); g2.sAm = 1; g2.sAk = nr;
    g2.B = b.W.as<double>(); g2.sBk = m; g2.sBn = 1;
    g2.C = c->m2.as<double>(); g2.sCm = 1; g2.sCn = nr;
    g2.M = nr; g2.N = m; g2.K = m;
    LRN_TRY(gemm(c->stream, g2));
    if (b.npos_nz > b.nd)
      hipLaunchKernelGGL(aa_times_rows_kernel, dim3((b.npos_nz - b.nd + 3) / 4), dim3(256), 0, c->stream,
                         b.ent_ptr.as<long>(), b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(),
                         c->m2.as<double>(), nr, r0, r1, b.nd, b.npos_nz, b.sigma_d.as<int>(), y);
    if (b.nd > 0)
      hipLaunchKernelGGL(aa_dense_dot_rows_kernel, dim3(b.nd), dim3(256), 0, c->stream, b.Adense.as<double>(), m,
                         c->m2.as<double>(), nr, r0, r1, b.sigma_d.as<int>(), y);
  }
  if (c->nlin > 0 && rank == 0) LRN_TRY(lin_matvec(c, x, y));
  LRN_HIP(c, hipGetLastError());
  return LRN_OK;
}


}  // namespace lrn
