// Schur-complement assembly  H_ij = tr(A_i W A_j W)  (+ C_lin diag(X_lin/S_lin) C_lin'),
// factorisation and solve.  Replaces makeBBBBs / makeBBBBsi / _dot / makeBBBB_rank1
// (reference src/makeBBBB.jl:1-218) and predictor_corrector.jl:36-39,53-90,199.
//
// Every unordered pair {i,j} is computed once, by the constraint that comes first in the
// reference's nnz-sorted order sigmaA (its "owner"), exactly as makeBBBBsi walks it
// (makeBBBB.jl:77,151,192).  The matrix is kept in sigma-POSITION space when nlmi == 1 so
// that an owner's results form one contiguous column of the lower triangle -- this is what
// makes the multi-GPU exchange an all-gather of column blocks.
//
//   owner dense  (positions < nd):   T_i = W A_i W on the FP64 MFMA GEMM
//        GEMM1  P_i = A_i W                      (batched, 2 msz^3)
//        GEMM2  T_i = W P_i, lower 128-tiles only, strictly-lower tiles scaled by 2 (msz^3)
//        GEMM3  H[j,i] = <A_j, T_i> for dense j >= i: one TN GEMM whose K loop skips the
//               upper tiles (packed-symmetric inner product, nvar^2 msz^2 / 2), split-K slabs
//        gather H[j,i] = sum_e a_e T_i[r_e,c_e] for sparse j
//   owner sparse (positions >= nd):  one WAVEFRONT per entry (i,j), lanes over the
//        nnz_i x nnz_j product terms a_e a_f W[c_e,r_f] W[c_f,r_e]   (the _dot kernel);
//        owners with <= 4 nonzeros use one THREAD per entry (the nnz==1 fast path,
//        makeBBBB.jl:188-209, is its 1x1 case).
//   rank-one data (mode -1): BG = B G (sparse x dense), H += (BG BG').^2 with the square
//        fused in the MFMA GEMM epilogue (makeBBBB.jl:7-14).
//   rank-k data (mode 1): U = G' V, H += blocksum(d d' .* (U'U).^2) over khat x khat blocks, again in the
//        epilogue of one MFMA product (assemble_lowrank).
#include <algorithm>

#include "ctx.h"

namespace lrn {

static constexpr int TS = 128;   // packing tile of the lower-stored T
static constexpr int BK_CHUNK = 16;   // K chunk of the GEMM kernels

// ------------------------------------------------------------------ sparse pair kernels
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// LANES lanes per entry (pi, pj >= pi), pi in [p_lo, p_hi):
//     H[i,j] = tr(A_i W A_j W) = sum_{(r,c) in A_i} sum_{(p,q) in A_j} a_rc b_pq W[c,p] W[q,r]
// The kernel is bound by the chain of dependent loads of one entry (entry lists -> W gathers -> reduction), not by
// gather bandwidth (rocprofv3, profiles/r02_sparse_*): what raises its throughput is entries in flight.  LANES = 64 for
// long products; 16 (four entries per wavefront) when nnz_i * nnz_j is a few hundred at most.  W is symmetric: both
// factors are fetched from the COLUMNS of the owner's support, W[p + c*msz] and W[q + r*msz] -- consecutive workgroups
// share pi, so at msz = 10^4 (W = 800 MB) the gathers of an owner stay in a few 80 KB columns (L2-miss traffic of the
// C5 assembly 234 GB -> 50 GB).  Staging the block W[supp_i, supp_j] in LDS was tried (one wave per entry, 8 KB each):
// a fifth of the fabric traffic again but 32 KB of LDS per workgroup cost 12 of 32 waves per CU and the kernel got
// slower (tru9 2.25 -> 2.75 ms, C5 110 -> 140 ms; profiles/r02_sparse_pair_lds_staged_summary.csv).
template <int LANES>
__global__ __launch_bounds__(256) void pair_wave_kernel(
    const long* __restrict__ ptr, const int* __restrict__ er, const int* __restrict__ ec,
    const double* __restrict__ ev, const double* __restrict__ W, int msz, int p_lo, int p_hi,
    int p_end, const int* __restrict__ hidx, double* __restrict__ H, int ldh, int rank, int world,
    int bs) {
  constexpr int PER_WG = 256 / LANES;
  const int lane = threadIdx.x & (LANES - 1), grp = threadIdx.x / LANES;
  const int pi = p_lo + blockIdx.y;
  if (pi >= p_hi) return;
  if (world > 1 && shard_owner(pi / bs, world) != rank) return;
  const int pj = pi + blockIdx.x * PER_WG + grp;
  const bool live = pj < p_end;                 // (whole wavefronts stay together for the shuffles below)
  double acc = 0.0;
  if (live) {
    const long ib = ptr[pi], jb = ptr[pj];
    const int ni = (int)(ptr[pi + 1] - ib), nj = (int)(ptr[pj + 1] - jb);
    const int total = ni * nj;
    for (int idx = lane; idx < total; idx += LANES) {
      int e = idx / nj, f = idx - e * nj;
      int r = er[ib + e], c = ec[ib + e];
      int p = er[jb + f], q = ec[jb + f];
      // A_i[r,c] W[c,p] A_j[p,q] W[q,r]
      acc += ev[ib + e] * ev[jb + f] * W[(long)p + (long)c * msz] * W[(long)q + (long)r * msz];
    }
  }
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, LANES);
  if (live && lane == 0) {
    int hi = hidx[pi], hj = hidx[pj];
    int rr = hi > hj ? hi : hj, cc = hi > hj ? hj : hi;
    H[(long)rr + (long)cc * ldh] += acc;
  }
}

// one thread per entry, owners with <= 4 nonzeros
__global__ __launch_bounds__(256) void pair_thread_kernel(
    const long* __restrict__ ptr, const int* __restrict__ er, const int* __restrict__ ec,
    const double* __restrict__ ev, const double* __restrict__ W, int msz, int p_lo, int p_end,
    const int* __restrict__ hidx, double* __restrict__ H, int ldh, int rank, int world, int bs) {
  const int pi = p_lo + blockIdx.y;
  if (pi >= p_end) return;
  if (world > 1 && shard_owner(pi / bs, world) != rank) return;
  const int pj = pi + blockIdx.x * 256 + threadIdx.x;
  if (pj >= p_end) return;
  const long ib = ptr[pi], jb = ptr[pj];
  const int ni = (int)(ptr[pi + 1] - ib), nj = (int)(ptr[pj + 1] - jb);
  double acc = 0.0;
  for (int e = 0; e < ni; ++e) {
    int r = er[ib + e], c = ec[ib + e];
    double a = ev[ib + e];
    for (int f = 0; f < nj; ++f) {
      int p = er[jb + f], q = ec[jb + f];
      acc += a * ev[jb + f] * W[(long)p + (long)c * msz] * W[(long)q + (long)r * msz];   // both from columns of A_i
    }
  }
  int hi = hidx[pi], hj = hidx[pj];
  int rr = hi > hj ? hi : hj, cc = hi > hj ? hj : hi;
  H[(long)rr + (long)cc * ldh] += acc;
}

// dense owner slot s (T stored lower tiles, strictly-lower x2) x sparse other pj
__global__ __launch_bounds__(256) void dense_sparse_gather_kernel(
    const long* __restrict__ ptr, const int* __restrict__ er, const int* __restrict__ ec,
    const double* __restrict__ ev, const double* __restrict__ T, int msz, int s0, int ns, int p_lo,
    int p_end, const int* __restrict__ hidx, double* __restrict__ H, int ldh) {
  const int s = blockIdx.y;
  if (s >= ns) return;
  const int pj = p_lo + blockIdx.x * 256 + threadIdx.x;
  if (pj >= p_end) return;
  const double* Ts = T + (long)s * msz * msz;
  double acc = 0.0;
  for (long f = ptr[pj]; f < ptr[pj + 1]; ++f) {
    int p = er[f], q = ec[f];
    int tp = p / TS, tq = q / TS;
    double t;
    if (tp == tq) t = Ts[(long)p + (long)q * msz];
    else if (tp > tq) t = 0.5 * Ts[(long)p + (long)q * msz];
    else t = 0.5 * Ts[(long)q + (long)p * msz];
    acc += ev[f] * t;
  }
  int hi = hidx[s0 + s], hj = hidx[pj];
  int rr = hi > hj ? hi : hj, cc = hi > hj ? hj : hi;
  H[(long)rr + (long)cc * ldh] += acc;
}

// out[(r0+i) + (c0+j)*ldo] += sum_s slab_s[i + j*M]   for computed (lower) tiles
// slabs [nw1, nslab) count twice (strictly-lower tiles of the packed symmetric operands, Cholesky path)
__global__ void reduce_slabs_tri_kernel(const double* __restrict__ slabs, long stride, int nslab, int nw1, int M,
                                        int N, double* __restrict__ out, long ldo) {
  long total = (long)M * N;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % M), j = (int)(e / M);
    if (i / TS < j / TS) continue;
    double s = 0.0, s2 = 0.0;
    for (int k = 0; k < nw1; ++k) s += slabs[(long)k * stride + e];
    for (int k = nw1; k < nslab; ++k) s2 += slabs[(long)k * stride + e];
    out[(long)i + (long)j * ldo] += s + 2.0 * s2;
  }
}

// Ut[n + k*m] = L[k + n*m] for k >= n, else 0: the transposed lower Cholesky factor with explicit zeros
__global__ __launch_bounds__(256) void transpose_lower_kernel(const double* __restrict__ L, int m,
                                                              double* __restrict__ Ut) {
  __shared__ double tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;      // bx: rows k of L, by: columns n of L
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8) {
    int k = bx + tx, n = by + j;
    tile[j][tx] = (k < m && n < m && k >= n) ? L[(long)k + (long)n * m] : 0.0;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    int n = by + tx, k = bx + j;
    if (n < m && k < m) Ut[(long)n + (long)k * m] = tile[tx][j];
  }
}

// Hd (nd x nd, slot space, lower) scattered into H through hidx (nlmi > 1)
__global__ void scatter_add_lower_kernel(const double* __restrict__ Hd, int nd, const int* __restrict__ hidx,
                                         double* __restrict__ H, int ldh) {
  long total = (long)nd * nd;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % nd), j = (int)(e / nd);
    if (i < j) continue;
    int hi = hidx[i], hj = hidx[j];
    int rr = hi > hj ? hi : hj, cc = hi > hj ? hj : hi;
    H[(long)rr + (long)cc * ldh] += Hd[e];
  }
}

// BGt[k + h*msz] = sum_e bval_e G[bcol_e + k*msz]     (one workgroup per H-row h)
__global__ __launch_bounds__(256) void bg_kernel(const long* __restrict__ bptr, const int* __restrict__ bcol,
                                                 const double* __restrict__ bval, const double* __restrict__ G,
                                                 int msz, double* __restrict__ BGt) {
  const int h = blockIdx.x;
  const long b = bptr[h], e = bptr[h + 1];
  for (int k = threadIdx.x; k < msz; k += 256) {
    double s = 0.0;
    for (long f = b; f < e; ++f) s += bval[f] * G[(long)bcol[f] + (long)k * msz];
    BGt[(long)k + (long)h * msz] = s;
  }
}

// Bdt[k + h*msz] = B[h, k]  (dense copy of the rank-one factors, zero-filled by the caller)
__global__ void b_dense_kernel(const long* __restrict__ bptr, const int* __restrict__ bcol, const double* __restrict__ bval,
                               int msz, double* __restrict__ Bdt) {
  const int h = blockIdx.x;
  for (long f = bptr[h] + threadIdx.x; f < bptr[h + 1]; f += blockDim.x) Bdt[(long)bcol[f] + (long)h * msz] = bval[f];
}

// U[k + h*msz] = sum_e val_e M[col_e, k]  (one workgroup per factor column h): U = G' V, or U = W V from the symmetric W read
// down its columns (sym, coalesced)
__global__ __launch_bounds__(256) void lowrank_gather_kernel(const long* __restrict__ ptr, const int* __restrict__ col,
                                                             const double* __restrict__ val, const double* __restrict__ M,
                                                             int msz, int sym, double* __restrict__ U) {
  const long h = blockIdx.x;
  const long b = ptr[h], e = ptr[h + 1];
  for (int k = threadIdx.x; k < msz; k += 256) {
    double s = 0.0;
    for (long f = b; f < e; ++f) s += val[f] * (sym ? M[(long)k + (long)col[f] * msz] : M[(long)col[f] + (long)k * msz]);
    U[(long)k + h * msz] = s;
  }
}

// H += C_lin diag(xs) C_lin'  (lower triangle): one thread per target entry sums its contributions in
// a fixed order (lists built at upload) -- no floating-point atomics, results are reproducible
__global__ void lin_schur_kernel(const int* __restrict__ pr, const int* __restrict__ pc, const long* __restrict__ pp,
                                 const int* __restrict__ pl, const double* __restrict__ pw, long np,
                                 const double* __restrict__ xs, double* __restrict__ H, int ldh, int rank, int world,
                                 int bs) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= np) return;
  const int ri = pr[t], rj = pc[t];
  if (world > 1 && shard_owner(rj / bs, world) != rank) return;
  double s = 0.0;
  for (long k = pp[t]; k < pp[t + 1]; ++k) s += pw[k] * xs[pl[k]];
  H[(long)ri + (long)rj * ldh] += s;
}


__global__ void get_diag_kernel(const double* __restrict__ H, int n, double* __restrict__ d) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = H[(long)i * n + i];
}

__global__ void add_diag_kernel(double* __restrict__ H, int n, double eps) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) H[(long)i * n + i] += eps;
}

// natural-index full symmetric copy of the lower-authoritative H
__global__ void export_h_kernel(const double* __restrict__ H, int n, const int* __restrict__ ipos,
                                double* __restrict__ out) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    int hi = ipos ? ipos[i] : i, hj = ipos ? ipos[j] : j;
    int rr = hi > hj ? hi : hj, cc = hi > hj ? hj : hi;
    out[e] = H[(long)rr + (long)cc * n];
  }
}

__global__ void gather_vec_kernel(const double* __restrict__ src, const int* __restrict__ idx, double* __restrict__ dst, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[idx ? idx[i] : i];
}
__global__ void scatter_vec_kernel(const double* __restrict__ src, const int* __restrict__ idx, double* __restrict__ dst, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[idx ? idx[i] : i] = src[i];
}

// ------------------------------------------------------------------ host drivers

static inline unsigned nblocks(long n, int per = 256, long cap = 4096) {
  long b = (n + per - 1) / per;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

// Workgroup-slot quantisation: the chip holds 256 CUs x 2 workgroups of these GEMMs at once and
// all workgroups of a launch take the same time, so a launch of `wgs` workgroups runs in
// ceil(wgs / 512) rounds.  Pick batch sizes / split-K factors that fill the last round.
static constexpr long WG_SLOTS = 512;
static double fill_eff(long wgs) { return (double)wgs / (double)(((wgs + WG_SLOTS - 1) / WG_SLOTS) * WG_SLOTS); }

static int pick_ksplit(long tiles, int max_split) {
  int best = 1;
  double beste = 0.0;
  for (int k = 1; k <= max_split; ++k) {
    if (tiles * k < WG_SLOTS && k < max_split) continue;
    double e = fill_eff(tiles * k);
    if (e >= 0.97) return k;
    if (e > beste) { beste = e; best = k; }
  }
  return best;
}

static long pick_p_batch(int m, long limit) {
  long t1 = (long)((m + 127) / 128) * ((m + 127) / 128);   // GEMM1 tiles per matrix
  long tl = (long)((m + 127) / 128);
  long t2 = tl * (tl + 1) / 2;                              // GEMM2 (lower) tiles per matrix
  long best = std::min<long>(32, limit);
  double beste = 0.0;
  for (long bsz = std::min<long>(16, limit); bsz <= std::min<long>(96, limit); ++bsz) {
    // time-weighted: GEMM1 does 2x the work per tile count ratio
    double e = (2.0 * t1 * fill_eff(t1 * bsz) + (double)t2 * fill_eff(t2 * bsz)) / (2.0 * t1 + t2);
    if (e > beste + 1e-9) { beste = e; best = bsz; }
  }
  return best;
}

// ---- Cholesky path of the dense assembly.  With W = L L' (L lower triangular)
//        H_ij = tr(A_i W A_j W) = < L' A_i L , L' A_j L >,
// so the triangular factor replaces the two full products per constraint (3 msz^3 flop) by
//        GEMM1'  P_k  = A_k L,  lower tiles only, K from the tile's column origin   (2/3 msz^3)
//        GEMM2'  At_k = L' P_k, lower tiles only, K from the tile's row origin      (1/3 msz^3)
// and the inner products become a symmetric rank-k update over the packed lower tiles of all At_k
//        GEMM3'  H[j,i] = <At_j, At_i>   (nvar^2 msz^2 / 2, as before).
// The perturbation is that of a backward-stable Cholesky of W (||L L' - W|| <= c msz eps ||W||), the level W
// itself is known to; when the factorisation of W breaks down (W numerically singular late in a solve) the
// T_k = W A_k W path below takes over.  Multi-GPU: the columns of the matrix variable are dealt to the ranks
// (col_runs) -- all three GEMMs shard and the ranks' partial Schur matrices are summed by one all-reduce.

// out[(i) + (j)*ldo] += sum_s w[s] * slab_s[i + j*M]  (lower 128-tiles; fixed order; weights 1 / 2 are exact)
struct SlabWeights {
  static constexpr int MAXS = 160;
  float w[MAXS];
};
__global__ void reduce_slabs_w_kernel(const double* __restrict__ slabs, long stride, int nslab, SlabWeights sw, int M,
                                      int N, double* __restrict__ out, long ldo) {
  long total = (long)M * N;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % M), j = (int)(e / M);
    if (i / 16 < j / 16) continue;          // (GEMM_DIAG_LOWER: blocks above the diagonal are not computed)
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < nslab; ++k) {
      const double v = slabs[(long)k * stride + e];
      if (sw.w[k] == 1.0f) s1 += v; else s2 += v;
    }
    out[(long)i + (long)j * ldo] += s1 + 2.0 * s2;
  }
}

// Multi-GPU split of the Cholesky path: the COLUMNS of the matrix variable.  Column c of every At_k = L' A_k L needs
// only columns >= c of L and A_k, and <At_i, At_j> is a sum over columns -- so a rank that owns the columns [c0, c1)
// computes those columns of every P_k and At_k and its share of every inner product: all three GEMMs shard, no
// intermediate is exchanged, and the ranks' partial Schur matrices are added by one all-reduce (nvar^2 doubles).
// Every rank gets ONE contiguous column range whose ends are multiples of 16 (the block width of the packed layout):
// the products of a range run on the trailing blocks A[c0:, c0:], L[c0:, c0:] with the 128-tile grid anchored at
// c0, so a range costs whole tiles in GEMM1'/GEMM2' (its last tile column may be partly empty) and exactly its
// packed length in GEMM3'.  col_range_cost prices that (in ms); a dynamic programme over the 16-column units minimises
// the largest load (ties keep the smallest cut).  Python specification: sharding.column_range.
//   GEMM1'  tile column j (K from its origin): (ntm - j) tiles x (M - 128 j) K
//   GEMM2'  tile (i, j), i >= j (K from the row origin): M - 128 i
//   GEMM3'  nd^2 / 2 pairs x 2 flop x packed length of the range
// The constants are a least-squares fit to the per-rank times of the C4 instance replayed on one GPU for 1, 2, 4 and
// 8 ranks (tools/shard_balance.py, profiles/r02_shard_balance.txt; ms at nd = 4000): GEMM1'/GEMM2' cost a fixed
// equivalent of ~220 K per tile on top of their K length (short tiles are dearer per flop; fit within 9 % / 17 %),
// GEMM3' is linear in the packed length (within 0.8 %).
static double col_range_cost(int m, int nd, int c0, int c1, int S) {
  const double M = m - c0;
  const int ntm = (m - c0 + 127) / 128, ntn = (c1 - c0 + 127) / 128;
  // the last tile column of a range may be partly empty: its waves skip the 16-column blocks beyond the range
  // (interleaved block ownership: both wave columns lose a block per 32 columns), but a K-step of the masked loop
  // has a floor (fragment reads, branches, the barrier): measured 0.5-0.7 of a full tile column for 32 of 128 columns,
  // 0.9 for 96
  const int rem = (c1 - c0) - 128 * (ntn - 1);
  const double last = rem >= 128 ? 1.0 : std::min(1.0, 0.4 + 0.65 * (double)((rem + 31) / 32) / 4.0);
  double k1 = 0.0, k2 = 0.0, tiles = 0.0;
  for (int j = 0; j < ntn; ++j) {
    const double f = j == ntn - 1 ? last : 1.0;
    k1 += f * (double)(ntm - j) * (M - 128.0 * j);
    // sum_{i=j}^{ntm-1} (M - 128 i)
    k2 += f * ((double)(ntm - j) * M - 128.0 * (0.5 * (double)(ntm - 1) * ntm - 0.5 * (double)(j - 1) * j));
    tiles += f * (double)(ntm - j);
  }
  const double k3 = 16.0 * (c1 - c0) + (double)(packed_off_base(c1, S) - packed_off_base(c0, S));
  const double s = (double)nd / 4000.0;
  return s * (0.0016774 * (k1 + 219.0 * tiles) + 0.0016283 * (k2 + 228.0 * tiles)) + s * s * 0.00024209 * k3;
}

static std::vector<std::pair<int, int>> col_runs(int m, int nd, int rank, int world) {
  const int S = packed_S(m), nu = S / 16;          // 16-column units
  std::vector<std::pair<int, int>> runs;
  if (world <= 1) { runs.push_back({0, m}); return runs; }
  auto col = [&](int u) { return std::min(m, 16 * u); };
  const int P = std::min(world, nu);
  // dp[p][j] = best largest load of the first j units over p ranks
  std::vector<std::vector<double>> dp(P + 1, std::vector<double>(nu + 1, 1e300));
  std::vector<std::vector<int>> cut(P + 1, std::vector<int>(nu + 1, 0));
  dp[0][0] = 0.0;
  for (int p = 1; p <= P; ++p)
    for (int j = p; j <= nu; ++j)
      for (int i = p - 1; i < j; ++i) {
        if (dp[p - 1][i] >= dp[p][j]) continue;                    // cannot improve on the best found so far
        const double seg = col_range_cost(m, nd, col(i), col(j), S);
        const double v = dp[p - 1][i] > seg ? dp[p - 1][i] : seg;
        if (v < dp[p][j]) { dp[p][j] = v; cut[p][j] = i; }
      }
  std::vector<int> lo(P), hi(P);
  for (int p = P, j = nu; p >= 1; --p) { lo[p - 1] = cut[p][j]; hi[p - 1] = j; j = cut[p][j]; }
  if (rank < P) runs.push_back({col(lo[rank]), col(hi[rank])});
  return runs;
}

// Matrices per launch of the triangular-K products: their workgroups differ in length, so every launch ends with a
// drain of about half the longest workgroup -- fewer, larger launches (measured at C4: GEMM1'+GEMM2' 569 / 555 /
// 547 / 545 ms per step with 64 / 128 / 256 / 500 matrices per launch); up to 8.6 GB of P workspace.
// Round 3: with the masked K-steps cheaper the drains show again -- 16 / 8 / 4 / 2 launches per step: GEMM1' 335.8 / 335.3 /
// 333.6 / 334.3, GEMM2' 177.1 / 176.4 / 175.3 / 175.2 ms; `large` = up to 34 GB (1000 matrices at C4) where the memory
// is there (chol_path_applicable).
static long tri_p_batch(int m, bool large = false) {
  long p = (long)((large ? 34.4e9 : 8.6e9) / ((double)m * m * 8.0));
  return std::max<long>(16, std::min<long>(large ? 1024 : 256, p));
}

static bool chol_path_applicable(lrn_ctx* c, LmiBlock& b, long* pcap_out) {
  if (c->opt.schur_chol == 0) return false;
  if (b.npos_nz != b.nd || b.nd < 2 || b.msz < 2) return false;   // sparse partners gather from T_k = W A_k W itself
  if (c->opt.schur_chol < 0 && b.msz < 256) return false;
  if (c->world > 1 && !c->pos_space) return false;
  // the column split deals 16-column units, whole 128-tiles at a time in GEMM1'/2': with fewer tiles than ranks the
  // Schur column blocks (all ranks busy on full tiles) win
  if (c->world > 1 && c->opt.schur_chol < 0 && (b.msz + 127) / 128 < c->world) return false;
  // multi-GPU: the ranks must enter the same collective.  Everything above is the same on every rank; the memory
  // test below is not (allocator state differs), so the host all-reduces lrn_schur_plan over the ranks and pins
  // the result with option "schur_plan" (sharding.SchurExchange) -- a pinned plan is not re-decided here.
  if (c->world > 1 && c->opt.schur_plan == 0) return false;
  const long mm = (long)b.msz * b.msz;
  long pcap = c->opt.p_batch > 0 ? c->opt.p_batch : tri_p_batch(b.msz);
  if (pcap > b.nd) pcap = b.nd;
  *pcap_out = pcap;
  if (c->world > 1 && c->opt.schur_plan == 1) return true;        // (an allocation failure is then a loud error)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  double avail = ((double)free_b + (double)c->T.bytes + (double)c->P.bytes) * 0.92;
  double need = (double)b.nd * packed_total_elems(b.msz) * 8.0 + (double)pcap * mm * 8.0 + 10.0e9;   // + split-K slabs
  if (need > avail) return false;
  if (c->opt.p_batch <= 0 && c->world == 1) {
    // fewer, larger launches of GEMM1'/2' where a tenth of the memory stays free after them
    const long big = std::min<long>(tri_p_batch(b.msz, true), b.nd);
    if (big > pcap && need + (double)(big - pcap) * mm * 8.0 + 0.10 * (double)total_b <= avail / 0.92) *pcap_out = big;
  }
  return true;
}

// lrn_schur_plan: 1 = the next assembly of this rank would take the Cholesky path (partial sums, all-reduce),
// 0 = Schur column blocks (all-gather) -- from this rank's own view
int schur_plan(lrn_ctx* c, int mode) {
  if (mode == -1 || mode == 1 || c->nlmi != 1) return 0;
  LmiBlock& b = c->lmi[0];
  long pcap = 0;
  const int pin = c->opt.schur_plan;
  c->opt.schur_plan = -1;                      // this rank's own view, whatever was pinned before
  const bool ok = b.nd > 0 && c->opt.schur_chol != 2 && chol_path_applicable(c, b, &pcap);
  c->opt.schur_plan = pin;
  return ok ? 1 : 0;
}

// W = L L' for the assembly: c->wchol = [ L (col-major, strict upper part zeroed) | Ut = L' with explicit zeros |
// potrf work ].  *ok = false when W is not numerically positive definite.
__global__ void tril_inplace_kernel(double* __restrict__ L, int m) {
  long total = (long)m * m;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % m), j = (int)(e / m);
    if (i < j) L[e] = 0.0;
  }
}

static int factor_w(lrn_ctx* c, LmiBlock& b, bool* ok) {
  const int m = b.msz;
  const long mm = (long)m * m;
  *ok = false;
  LRN_TRY(ensure(c, c->wchol, (2 * (size_t)mm + chol_work_doubles(m)) * 8));
  double* Lw = c->wchol.as<double>();
  double* Ut = Lw + mm;
  double* cw = Ut + mm;
  tic(c);
  LRN_HIP(c, hipMemcpyAsync(Lw, b.W.p, (size_t)mm * 8, hipMemcpyDeviceToDevice, c->stream));
  LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 8, c->stream));
  LRN_TRY(potrf_lower(c->stream, Lw, m, m, cw, c->info_dev.as<int>()));
  int h_info = 0;
  LRN_HIP(c, hipMemcpyAsync(&h_info, c->info_dev.p, 4, hipMemcpyDeviceToHost, c->stream));
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  if (h_info != 0) {
    c->counts["wchol_fail"] += 1;
    return LRN_OK;
  }
  hipLaunchKernelGGL(transpose_lower_kernel, dim3((m + 31) / 32, (m + 31) / 32), dim3(256), 0, c->stream, Lw, m, Ut);
  hipLaunchKernelGGL(tril_inplace_kernel, dim3(nblocks(mm)), dim3(256), 0, c->stream, Lw, m);
  toc(c, "wchol");
  *ok = true;
  return LRN_OK;
}

// (W = L L' already in c->wchol, factor_w)
static int assemble_dense_chol(lrn_ctx* c, LmiBlock& b, long P_cap) {
  const int m = b.msz, nd = b.nd, n = c->nvar;
  const long mm = (long)m * m;
  const long Kp = packed_total_elems(m), Kd = packed_diag_elems(m);
  const long cstride = 16L * nd;              // chunk-major: chunk q of At_k at q * cstride + 16 k
  const size_t t_bytes = (size_t)(Kp / 16) * cstride * 8;
  double* Ut = c->wchol.as<double>() + mm;
  // ---- this rank's columns of the matrix variable (all of them on one GPU): [c0, c1), multiples of 16
  const std::vector<std::pair<int, int>> runs = col_runs(m, nd, c->rank, c->world);
  const int S = packed_S(m);
  // ---- workspaces: P (batch of row-major blocks P_k[c0:, c0:c1] = A_k[c0:, c0:] L[c0:, c0:c1]), T (all At_k, packed).
  // P holds only the owned columns (leading dimension = their count rounded to 16), so a rank with a narrow range
  // takes many more matrices per launch: the triangular products end every launch with a drain of unequal
  // workgroups, and 8 ranks would otherwise pay 16 of them on a fraction of the work.
  long p_elems = 0;                       // doubles per matrix
  for (auto& rn : runs) p_elems = std::max(p_elems, (long)(m - rn.first) * (((rn.second - rn.first) + 15) & ~15));
  if (p_elems > 0) {
    long cap = c->opt.p_batch > 0 ? c->opt.p_batch : std::max<long>(16, (long)(8.6e9 / ((double)p_elems * 8.0)));
    // one GPU: 256 matrices per launch, or what chol_path_applicable found room for (up to 1024)
    if (c->opt.p_batch <= 0 && c->world <= 1) cap = std::max<long>(std::min<long>(cap, 256), std::min<long>(P_cap, 1024));
    P_cap = std::min<long>(std::min<long>(cap, nd), 32768);
  }
  LRN_TRY(ensure(c, c->P, (size_t)P_cap * std::max<long>(p_elems, 1) * 8));
  const void* t_before = c->T.p;
  LRN_TRY(ensure(c, c->T, t_bytes));                        // (a fresh allocation comes back zeroed)
  if (c->T.p == t_before && (c->T_layout != 1 || c->T_m != m || c->T_owner != &b))
    LRN_HIP(c, hipMemsetAsync(c->T.p, 0, t_bytes, c->stream));               // padding rows must be zero
  c->T_layout = 1;
  c->T_m = m;
  c->T_owner = &b;
  double* Ad = b.Adense.as<double>();
  double* P = c->P.as<double>();
  double* T = c->T.as<double>();
  for (int a = 0; a < nd; a += (int)P_cap) {
    const int nb = std::min((int)P_cap, nd - a);
    for (auto& rn : runs) {
      // columns [c0, c1): P[c0:, c0:c1] = A[c0:, c0:] L[c0:, c0:c1] and At[c0:, c0:c1] = L[c0:, c0:]' P[c0:, c0:c1] are
      // the same triangular products on the trailing blocks (L lower triangular: nothing above row c0 contributes)
      const int c0 = rn.first, c1 = rn.second;
      const long off = (long)c0 + (long)c0 * m;
      const long ldp = ((c1 - c0) + 15) & ~15;               // P block: (m - c0) rows x ldp, row-major
      tic(c);
      GemmDesc g1;   // P = A_a L, row-major (P[i][j] at j + i*ldp), tiles i >= j, K from the tile's column origin
      g1.A = Ad + (long)a * mm + off; g1.sAm = 1; g1.sAk = m; g1.bA = mm;
      g1.B = Ut + off; g1.sBk = m; g1.sBn = 1; g1.bB = 0;     // op(B)[k][j] = L[k,j] = Ut[j + k*m]
      g1.C = P; g1.sCm = ldp; g1.sCn = 1; g1.bC = p_elems;
      g1.M = g1.K = m - c0; g1.N = c1 - c0; g1.batch = nb;
      // (round 4: of the diagonal tiles of P_k GEMM2' reads only the blocks on and below the block diagonal -- the
      // others meet the stored zeros of L' -- so GEMM1' leaves them out: 28 of 64 blocks of the 16 longest tiles)
      g1.flags = GEMM_TRI_LOWER | GEMM_KFROM_N | (c->opt.gemm_no_skip ? GEMM_NO_SKIP : 0) |
                 (c->opt.gemm_dyn_masks ? GEMM_DYN_MASKS : 0) | (c->opt.gemm1_diag ? GEMM_DIAG_LOWER_Z : 0) |
                 ((c->opt.gemm_lab & 15) << 20);
      if (c->opt.gemm_lab & 32) g1.bA = 0;                       // (measurement: every batch element reads matrix 0 -- cache-resident)
      if (c->opt.gemm_lab & 16) g1.flags &= ~GEMM_KFROM_N;      // (measurement: every tile walks the whole K range -- stored zeros)
      LRN_TRY(gemm(c->stream, g1));
      toc(c, "gemm1");
      tic(c);
      GemmDesc g2;   // At = L' P, tiles i >= j, K from the tile's row origin, stored packed
      g2.A = Ut + off; g2.sAm = 1; g2.sAk = m; g2.bA = 0;     // op(A)[i][k] = L[k,i] = Ut[i + k*m]
      g2.B = P; g2.sBk = ldp; g2.sBn = 1; g2.bB = p_elems;
      g2.C = T + (long)a * 16; g2.sCm = 1; g2.sCn = m; g2.bC = 16;
      g2.pk_cstride = cstride;
      g2.M = g2.K = m - c0; g2.N = c1 - c0; g2.batch = nb;
      g2.flags = GEMM_TRI_LOWER | GEMM_KFROM_M | GEMM_C_PACKED | (c->opt.gemm_no_skip ? GEMM_NO_SKIP : 0) |
                 (c->opt.gemm_dyn_masks ? GEMM_DYN_MASKS : 0) | ((c->opt.gemm_lab & 15) << 20);
      if (c->opt.gemm_lab & 32) g2.bB = 0;
      if (c->opt.gemm_lab & 16) g2.flags &= ~GEMM_KFROM_M;
      g2.pk_m = m;
      g2.pk_off = c0;
      LRN_TRY(gemm(c->stream, g2));
      toc(c, "gemm2");
    }
  }
  // ---- GEMM3': H (+)= sum over this rank's columns of the packed inner products -- the whole lower triangle of H,
  // a partial sum when world > 1 (the ranks' matrices are added by one all-reduce)
  double* H = c->H.as<double>();
  double* Hd = H;
  long ldh = n;
  if (!c->pos_space) {
    LRN_TRY(ensure(c, c->Hd, (size_t)nd * nd * 8, true));
    LRN_HIP(c, hipMemsetAsync(c->Hd.p, 0, (size_t)nd * nd * 8, c->stream));
    Hd = c->Hd.as<double>();
    ldh = nd;
  }
  {
    const int M = nd, N = nd;
    // workgroup tile of GEMM3': 128 x 128, or 160 x 160 (gemm_f64_kseg_lds_kernel<true, 5>: 0.8 of the panel bytes per
    // flop, 100 MFMAs per wave between barriers) where its grid covers the lower triangle with > 5 % less area -- at
    // C4 (4000 = 25 x 160 = 31.25 x 128) both run within 2 % of each other, 128 ahead on most boxes: the kernel is bound
    // by the MFMA pipe at the clock it is left, not by its panel traffic (option "gemm3_tile": 0 auto, 128, 160)
    auto tri_area = [&](long ts) { const long tt = (nd + ts - 1) / ts; return tt * (tt + 1) / 2 * ts * ts; };
    const bool t160 = c->opt.gemm3_tile == 160 ||
                      (c->opt.gemm3_tile == 0 && nd >= 320 && (double)tri_area(160) < 0.95 * (double)tri_area(128));
    const int TS3 = t160 ? 160 : TS;
    long tiles = 0;
    const int tM = (M + TS3 - 1) / TS3;
    for (int tn = 0; tn < tM; ++tn) tiles += tM - tn;
    // GEMM3' runs as two launches: the regular tiles -- all equally long, lock-step through K -- and then the tiles
    // with blocks to skip (diagonal tiles: blocks above the diagonal; the last tile row when nd % 128 != 0).  The
    // split-K factor is chosen for the regular launch (the bulk of the work).
    const bool two_launches = !c->opt.gemm_no_skip && tM > 2;
    if (two_launches) tiles -= tM + ((M % TS3) ? tM - 1 : 0);
    // chunk ranges of the runs and the split-K budget (see below) divided over them by length
    struct RunK { long d0, d1, o0, o1; int ks, nsd; };
    std::vector<RunK> rk;
    long chunks_all = 0;
    for (auto& rn : runs) {
      const int c0 = rn.first, c1 = rn.second;
      RunK r{c0, c1, (Kd + packed_off_base(c0, S)) / 16, (Kd + packed_off_base(c1, S)) / 16, 0, 0};
      chunks_all += (r.d1 - r.d0) + (r.o1 - r.o0);
      rk.push_back(r);
    }
    {   // this rank's share of the USEFUL work of the three GEMMs (bench.py prices the roofline with them; 1 on one
        // GPU): column c of P_k costs 2 (m - c)^2 flop and column c of At_k (m - c)^2, GEMM3' its packed length
      double all = 0.0, own = 0.0;
      for (int cc = 0; cc < m; ++cc) {
        const double w = (double)(m - cc) * (m - cc);
        all += w;
        for (auto& rn : runs) if (cc >= rn.first && cc < rn.second) own += w;
      }
      c->timing["gemm1_share"] = own / all;
      c->timing["gemm2_share"] = own / all;
      c->timing["gemm3_share"] = (double)chunks_all / (double)(Kp / 16);
    }
    // split-K: short workgroups fill the workgroup slots evenly -- measured at C4: GEMM3' 548 / 524 / 509 / 505 ms
    // with 8 / 16 / 32 / 64 splits.  Largest factor <= 64 that fills whole rounds of workgroup slots, leaves every
    // split >= 1024 K-chunks and keeps the slabs within 9 GB.
    int ksplit = pick_ksplit(tiles, (int)std::min<long>(64, std::max<long>(1, chunks_all / 8)));
    for (int k = 64; k > ksplit; --k) {
      if (chunks_all / k < 256 || (double)k * M * N * 8.0 > 9.0e9) continue;
      if (fill_eff(tiles * k) >= 0.97) { ksplit = k; break; }
    }
    if (c->opt.gemm3_ksplit > 0) ksplit = std::min(64, c->opt.gemm3_ksplit);
    // the splits of all runs go into ONE launch: split s walks chunks [kb[s], ke[s]) with slab weight 1 (diagonal
    // 16-blocks) or 2 (strictly-lower blocks)
    SlabWeights sw;
    std::vector<int> kb, ke;
    int budget = std::max(ksplit, 2 * (int)rk.size());
    if (budget > 64) budget = 64;
    for (size_t ri = 0; ri < rk.size(); ++ri) {
      RunK& r = rk[ri];
      const long nd_ = r.d1 - r.d0, no_ = r.o1 - r.o0;
      r.ks = (int)std::max<long>(1, (long)((double)budget * (double)(nd_ + no_) / (double)chunks_all + 0.5));
      r.nsd = r.ks;
      if (no_ > 0) {
        if (r.ks < 2) r.ks = 2;
        r.nsd = (int)((double)r.ks * (double)nd_ / (double)(nd_ + no_) + 0.5);
        r.nsd = std::max(1, std::min(r.ks - 1, r.nsd));
      }
      if ((int)kb.size() + r.ks > 64) {         // rounding pushed the total over the kernel's limit: trim this run
        r.ks = 64 - (int)kb.size();
        if (r.ks < (no_ > 0 ? 2 : 1)) return set_error(c, LRN_ERR_STATE, "split-K budget exceeded (%d runs)", (int)rk.size());
        r.nsd = no_ > 0 ? std::max(1, std::min(r.ks - 1, r.nsd)) : r.ks;
      }
      const int nso = r.ks - r.nsd;
      for (int i = 0; i < r.nsd; ++i) {
        sw.w[kb.size()] = 1.0f;
        kb.push_back((int)(r.d0 + nd_ * i / r.nsd));
        ke.push_back((int)(r.d0 + nd_ * (i + 1) / r.nsd));
      }
      for (int i = 0; i < nso; ++i) {
        sw.w[kb.size()] = 2.0f;
        kb.push_back((int)(r.o0 + no_ * i / nso));
        ke.push_back((int)(r.o0 + no_ * (i + 1) / nso));
      }
    }
    const int nslab = (int)kb.size();
    if (nslab > 0) {
      LRN_TRY(ensure(c, c->slabs, (size_t)nslab * M * N * 8));
      tic(c);
      GemmDesc g3;
      g3.A = T; g3.sAm = 16; g3.sAk = 1;
      g3.B = T; g3.sBk = 1; g3.sBn = 16;
      g3.kflat_cstride = cstride;
      g3.C = c->slabs.as<double>(); g3.sCm = 1; g3.sCn = M;
      g3.M = M; g3.N = N;
      g3.flags = GEMM_TRI_LOWER | GEMM_KFLAT | GEMM_DIAG_LOWER | (c->opt.gemm_no_skip ? GEMM_NO_SKIP : 0) |
                 (t160 ? GEMM_TILE160 : 0) | ((c->opt.gemm_lab & 64) ? GEMM_LAB_SAME_CHUNK : 0);
      g3.kflat_total = Kp; g3.kflat_diag = Kd; g3.kflat_nsd = 1;
      g3.kflat_kb = kb.data(); g3.kflat_ke = ke.data();
      g3.kstagger = c->opt.gemm3_stagger;
      g3.ksplit = nslab; g3.sCs = (long)M * N;
      // regular tiles of every split first, the tiles with skipped blocks last, in one launch (tile_class 3)
      if (two_launches && c->opt.gemm3_sched == 0) {         // measurement: the two classes as two launches
        g3.tile_class = 1;
        LRN_TRY(gemm(c->stream, g3));
        toc(c, "gemm3");
        tic(c);
        g3.tile_class = 2;
      } else {
        g3.tile_class = two_launches ? 3 : 0;
        // a last tile row of height 128 + nd % 128 <= 160 instead of a row of edge tiles, as a second launch
        // (gemm_f64.hip, tile_class 4; option "gemm3_strip")
        if (two_launches && !t160 && c->opt.gemm3_strip && M >= 288 && M % 128 > 0 && M % 128 <= 32) g3.tile_class = 4;
      }
      LRN_TRY(gemm(c->stream, g3));
      toc(c, "gemm3");
      if (g3.tile_class == 4) {
        tic(c);
        g3.tile_class = 5;
        LRN_TRY(gemm(c->stream, g3));
        toc(c, "gemm3s");
      }
    }
    tic(c);
    hipLaunchKernelGGL(reduce_slabs_w_kernel, dim3(nblocks((long)M * N)), dim3(256), 0, c->stream,
                       c->slabs.as<double>(), (long)M * N, nslab, sw, M, N, Hd, ldh);
    toc(c, "reduce3");
  }
  if (!c->pos_space)
    hipLaunchKernelGGL(scatter_add_lower_kernel, dim3(nblocks((long)nd * nd)), dim3(256), 0, c->stream, Hd, nd,
                       b.hidx.as<int>(), H, n);
  c->counts["schur_chol"] += 1;
  if (c->world > 1) c->H_partial = true;      // H holds this rank's partial sum: all-reduce, not all-gather
  return LRN_OK;
}

static int assemble_dense(lrn_ctx* c, LmiBlock& b) {
  const int m = b.msz, nd = b.nd, n = c->nvar;
  const long mm = (long)m * m;
  // Both fast paths need W = L L'.  via_l: the W path below forms T_k = L (L' A_k L) L' on triangular K ranges
  // (4 products, 2 msz^3 flop) instead of W (A_k W) (2 products, 3 msz^3); this is what blocks that also hold sparse
  // constraints run (on any number of ranks, Schur column blocks).  option schur_chol: -1 auto, 0 never factor W, 1 as auto without the size
  // thresholds, 2 T-via-L only.
  bool via_l = false;
  {
    long pcap = 0;
    const bool want_chol = c->opt.schur_chol != 2 && chol_path_applicable(c, b, &pcap);
    const bool want_via_l = c->opt.schur_chol > 0 || (c->opt.schur_chol < 0 && m >= 256);
    if (want_chol || want_via_l) LRN_TRY(factor_w(c, b, &via_l));
    if (via_l && want_chol) return assemble_dense_chol(c, b, pcap);
  }
  double* W = b.W.as<double>();
  double* Ad = b.Adense.as<double>();
  double* H = c->H.as<double>();
  // capacities, per block: blocks of one problem differ in size (a cache keyed on the context once sized
  // the P / T workspaces for the first block and let a larger later block write past them)
  if (b.t_cap == 0 || b.p_cap == 0) {
    size_t free_b = 0, total_b = 0;
    LRN_HIP(c, hipMemGetInfo(&free_b, &total_b));
    long pcap = c->opt.p_batch > 0 ? c->opt.p_batch : (via_l ? tri_p_batch(m) : pick_p_batch(m, nd));
    if (pcap > nd) pcap = nd;
    // memory that is free now plus what the shared workspaces already hold
    double avail = ((double)free_b + (double)c->T.bytes + (double)c->P.bytes + (double)c->P2.bytes) * 0.80 -
                   2.0 * (double)pcap * mm * 8.0 - 1.5e9;
    long tcap = (long)(avail / ((double)mm * 8.0));
    if (c->opt.t_batch > 0) tcap = c->opt.t_batch;
    if (tcap > nd) tcap = nd;
    if (tcap < 1) return set_error(c, LRN_ERR_NOMEM, "not enough device memory for the T workspace");
    b.p_cap = pcap;
    b.t_cap = tcap;
  }
  const long P_cap = b.p_cap, T_cap = b.t_cap;
  LRN_TRY(ensure(c, c->P, (size_t)P_cap * mm * 8));
  const void* t_before = c->T.p;
  LRN_TRY(ensure(c, c->T, (size_t)T_cap * mm * 8));         // (a fresh allocation comes back zeroed)
  if (c->T.p != t_before) { c->T_m = m; c->T_owner = &b; }
  // upper tiles stay zero between assemblies of the SAME block; another block's layout left its data
  if (c->T_m != m || c->T_owner != &b || c->T_layout != 0) {
    LRN_HIP(c, hipMemsetAsync(c->T.p, 0, (size_t)T_cap * mm * 8, c->stream));
    c->T_m = m;
    c->T_owner = &b;
  }
  c->T_layout = 0;
  double* P = c->P.as<double>();
  double* T = c->T.as<double>();
  double* Hd = H;
  long ldh = n;
  if (!c->pos_space) {
    LRN_TRY(ensure(c, c->Hd, (size_t)nd * nd * 8, true));
    LRN_HIP(c, hipMemsetAsync(c->Hd.p, 0, (size_t)nd * nd * 8, c->stream));
    Hd = c->Hd.as<double>();
    ldh = nd;
  }
  // owner groups: contiguous slot ranges this rank owns, each at most T_cap long and
  // starting on a 128 boundary (so that the triangular tile mask lines up)
  std::vector<std::pair<int, int>> groups;
  if (c->world > 1) {
    for (int s0 = 0; s0 < nd; s0 += c->shard_bs)
      if (shard_owner(s0 / c->shard_bs, c->world) == c->rank) {
        int s1 = std::min(nd, s0 + c->shard_bs);
        for (int a = s0; a < s1; a += (int)T_cap) groups.push_back({a, std::min(s1, a + (int)T_cap)});
      }
  } else {
    for (int s0 = 0; s0 < nd; s0 += (int)T_cap) groups.push_back({s0, std::min(nd, s0 + (int)T_cap)});
  }
  for (auto& g : groups) {
    const int s0 = g.first, s1 = g.second, ns = s1 - s0;
    for (int a = s0; a < s1 && via_l; a += (int)P_cap) {
      const int nb = std::min((int)P_cap, s1 - a);
      double* Lw = c->wchol.as<double>();
      double* Ut = Lw + mm;
      LRN_TRY(ensure(c, c->P2, (size_t)P_cap * mm * 8));
      double* P2 = c->P2.as<double>();
      tic(c);
      GemmDesc g1;   // P = A_a L, row-major, tiles i >= j, K from the tile's column origin
      g1.A = Ad + (long)a * mm; g1.sAm = 1; g1.sAk = m; g1.bA = mm;
      g1.B = Ut; g1.sBk = m; g1.sBn = 1; g1.bB = 0;
      g1.C = P; g1.sCm = m; g1.sCn = 1; g1.bC = mm;
      g1.M = g1.N = g1.K = m; g1.batch = nb;
      g1.flags = GEMM_TRI_LOWER | GEMM_KFROM_N | (c->opt.gemm_no_skip ? GEMM_NO_SKIP : 0) |
                 (c->opt.gemm_dyn_masks ? GEMM_DYN_MASKS : 0);
      LRN_TRY(gemm(c->stream, g1));
      GemmDesc g2;   // At = L' P, tiles i >= j (K from the tile's row origin), mirrored: full symmetric, col-major
      g2.A = Ut; g2.sAm = 1; g2.sAk = m; g2.bA = 0;
      g2.B = P; g2.sBk = m; g2.sBn = 1; g2.bB = mm;
      g2.C = P2; g2.sCm = 1; g2.sCn = m; g2.bC = mm;
      g2.M = g2.N = g2.K = m; g2.batch = nb;
      g2.flags = GEMM_TRI_LOWER | GEMM_KFROM_M | GEMM_C_MIRROR;
      LRN_TRY(gemm(c->stream, g2));
      toc(c, "gemm1");
      tic(c);
      GemmDesc g3;   // Q = L At, tiles i >= j, K up to the end of the tile's rows; col-major into P
      g3.A = Lw; g3.sAm = 1; g3.sAk = m; g3.bA = 0;
      g3.B = P2; g3.sBk = m; g3.sBn = 1; g3.bB = mm;            // At symmetric: At[k,n] read as At[n + k*m]
      g3.C = P; g3.sCm = 1; g3.sCn = m; g3.bC = mm;
      g3.M = g3.N = g3.K = m; g3.batch = nb;
      g3.flags = GEMM_TRI_LOWER | GEMM_KTO_M;
      LRN_TRY(gemm(c->stream, g3));
      GemmDesc g4;   // T = Q L', lower tiles (strictly-lower x2), K up to the end of the tile's columns
      g4.A = P; g4.sAm = 1; g4.sAk = m; g4.bA = mm;
      g4.B = Lw; g4.sBk = m; g4.sBn = 1; g4.bB = 0;             // op(B)[k][j] = L[j,k]
      g4.C = T + (long)(a - s0) * mm; g4.sCm = 1; g4.sCn = m; g4.bC = mm;
      g4.M = g4.N = g4.K = m; g4.batch = nb;
      g4.flags = GEMM_TRI_LOWER | GEMM_OFFDIAG_X2 | GEMM_KTO_N;
      LRN_TRY(gemm(c->stream, g4));
      toc(c, "gemm2");
      c->counts["schur_via_l"] += 1;
    }
    for (int a = s0; a < s1 && !via_l; a += (int)P_cap) {
      int nb = std::min((int)P_cap, s1 - a);
      tic(c);
      GemmDesc g1;   // P = A_a W, stored row-major (P^T) so that GEMM2 reads it n-contiguous;
                     // W is symmetric, so it is read as W[n + k*m]: both operands stream
                     // through the direct-to-LDS path
      g1.A = Ad + (long)a * mm; g1.sAm = 1; g1.sAk = m; g1.bA = mm;
      g1.B = W; g1.sBk = m; g1.sBn = 1; g1.bB = 0;
      g1.C = P; g1.sCm = m; g1.sCn = 1; g1.bC = mm;
      g1.M = g1.N = g1.K = m; g1.batch = nb;
      LRN_TRY(gemm(c->stream, g1));
      toc(c, "gemm1");
      tic(c);
      GemmDesc g2;   // T = W P, lower tiles, strictly-lower x2
      g2.A = W; g2.sAm = 1; g2.sAk = m; g2.bA = 0;
      g2.B = P; g2.sBk = m; g2.sBn = 1; g2.bB = mm;
      g2.C = T + (long)(a - s0) * mm; g2.sCm = 1; g2.sCn = m; g2.bC = mm;
      g2.M = g2.N = g2.K = m; g2.batch = nb;
      g2.flags = GEMM_TRI_LOWER | GEMM_OFFDIAG_X2;
      LRN_TRY(gemm(c->stream, g2));
      toc(c, "gemm2");
    }
    // GEMM3: Hd[s0:nd, s0:s1] += A[s0:nd]^T . T   (packed-symmetric dot, lower tiles)
    {
      tic(c);
      const int M = nd - s0, N = ns;
      long tiles = 0;
      int tM = (M + TS - 1) / TS, tN = (N + TS - 1) / TS;
      for (int tn = 0; tn < tN; ++tn) tiles += std::max(0, tM - tn);
      int ksplit = pick_ksplit(tiles, std::min(64, std::max(1, m / 8)));
      for (int k = std::min(64, m / 8); k > ksplit; --k) {      // prefer short workgroups (see GEMM3' above)
        if ((long)m * m / 2 / BK_CHUNK / k < 1024 || (double)k * M * N * 8.0 > 9.0e9) continue;
        if (fill_eff(tiles * k) >= 0.97) { ksplit = k; break; }
      }
      if (c->opt.gemm3_ksplit > 0) ksplit = std::min(64, c->opt.gemm3_ksplit);
      size_t slab_bytes = (size_t)ksplit * M * N * 8;
      LRN_TRY(ensure(c, c->slabs, slab_bytes));
      GemmDesc g3;
      g3.A = Ad + (long)s0 * mm; g3.sAm = mm; g3.sAk = 1;
      g3.B = T; g3.sBk = 1; g3.sBn = mm;
      g3.C = c->slabs.as<double>(); g3.sCm = 1; g3.sCn = M;
      g3.M = M; g3.N = N;
      g3.flags = GEMM_TRI_LOWER | GEMM_KSEG_TRI;
      g3.kseg_ld = m; g3.kseg_cols = m;
      g3.ksplit = ksplit; g3.sCs = (long)M * N;
      LRN_TRY(gemm(c->stream, g3));
      hipLaunchKernelGGL(reduce_slabs_tri_kernel, dim3(nblocks((long)M * N)), dim3(256), 0, c->stream,
                         c->slabs.as<double>(), (long)M * N, ksplit, ksplit, M, N, Hd + (long)s0 + (long)s0 * ldh, ldh);
      toc(c, "gemm3");
    }
    // dense owner x sparse other
    if (b.npos_nz > nd) {
      tic(c);
      int nsp = b.npos_nz - nd;
      for (int y0 = 0; y0 < ns; y0 += 32768) {
        int ny = std::min(32768, ns - y0);
        hipLaunchKernelGGL(dense_sparse_gather_kernel, dim3((nsp + 255) / 256, ny), dim3(256), 0, c->stream,
                           b.ent_ptr.as<long>(), b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(),
                           T + (long)y0 * mm, m, s0 + y0, ny, nd, b.npos_nz, b.hidx.as<int>(), H, n);
      }
      toc(c, "sparse");
    }
  }
  if (!c->pos_space)
    hipLaunchKernelGGL(scatter_add_lower_kernel, dim3(nblocks((long)nd * nd)), dim3(256), 0, c->stream, Hd, nd,
                       b.hidx.as<int>(), H, n);
  return LRN_OK;
}

// owner ranges of one launch: the positions [lo, hi) cut at the column blocks this rank owns (all of them on one GPU) and
// into pieces of at most `piece` owners -- the grid of a launch is (partners of its FIRST owner) x (owners), so a long
// range launches workgroups that find no partner (half of them for one launch over the whole triangle), and a rank of a
// sharded run would launch the seven eighths it does not own just to return (round 4: C5 at 8 ranks 18.1 -> see
// profiles/r04_shard_balance_c5.txt)
static std::vector<std::pair<int, int>> owner_ranges(const lrn_ctx* c, int lo, int hi, int piece) {
  std::vector<std::pair<int, int>> out;
  auto cut = [&](int a, int b) {
    for (int x = a; x < b; x += piece) out.push_back({x, std::min(b, x + piece)});
  };
  if (c->world > 1) {
    for (int c0 = (lo / c->shard_bs) * c->shard_bs; c0 < hi; c0 += c->shard_bs)
      if (shard_owner(c0 / c->shard_bs, c->world) == c->rank) cut(std::max(lo, c0), std::min(hi, c0 + c->shard_bs));
  } else {
    cut(lo, hi);
  }
  return out;
}

static int assemble_sparse(lrn_ctx* c, LmiBlock& b) {
  const int n = c->nvar;
  double* H = c->H.as<double>();
  tic(c);
  if (b.q_wave > b.nd) {
    // entries per wavefront by the typical product length: mean nnz of the sparse owners squared
    double mean_nnz = 0.0;
    for (int p = b.nd; p < b.npos_nz; ++p) mean_nnz += (double)b.nnz[p];
    mean_nnz /= std::max(1, b.npos_nz - b.nd);
    int lanes = c->opt.pair_lanes;
    if (lanes != 4 && lanes != 8 && lanes != 16 && lanes != 64) lanes = mean_nnz * mean_nnz <= 512.0 ? 16 : 64;
    const int per_wg = 256 / lanes;
    for (const auto& rg : owner_ranges(c, b.nd, b.q_wave, 2048)) {
      const int a = rg.first, ny = rg.second - rg.first;
      dim3 grid((b.npos_nz - a + per_wg - 1) / per_wg, ny);
#define LRN_PAIR_LAUNCH(L)                                                                                           \
  hipLaunchKernelGGL(pair_wave_kernel<L>, grid, dim3(256), 0, c->stream, b.ent_ptr.as<long>(), b.ent_r.as<int>(),   \
                     b.ent_c.as<int>(), b.ent_v.as<double>(), b.W.as<double>(), b.msz, a, rg.second,                \
                     b.npos_nz, b.hidx.as<int>(), H, n, c->rank, c->world, c->shard_bs)
      if (lanes == 4) LRN_PAIR_LAUNCH(4);
      else if (lanes == 8) LRN_PAIR_LAUNCH(8);
      else if (lanes == 16) LRN_PAIR_LAUNCH(16);
      else LRN_PAIR_LAUNCH(64);
#undef LRN_PAIR_LAUNCH
    }
  }
  if (b.npos_nz > b.q_wave) {
    for (const auto& rg : owner_ranges(c, b.q_wave, b.npos_nz, 4096)) {
      const int a = rg.first, ny = rg.second - rg.first;
      hipLaunchKernelGGL(pair_thread_kernel, dim3((b.npos_nz - a + 255) / 256, ny), dim3(256), 0, c->stream,
                         b.ent_ptr.as<long>(), b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(),
                         b.W.as<double>(), b.msz, a, b.npos_nz, b.hidx.as<int>(), H, n, c->rank,
                         c->world, c->shard_bs);          // (owners a .. a + ny - 1 by the grid, partners up to npos_nz)
    }
  }
  toc(c, "sparse");
  return LRN_OK;
}

static int assemble_rank1(lrn_ctx* c, LmiBlock& b) {
  const int n = c->nvar, m = b.msz;
  if (!b.has_B) return set_error(c, LRN_ERR_STATE, "rank-one mode requested but no B factors were uploaded");
  // with G: H = ((BG)(BG)').^2 as the reference forms it (makeBBBB.jl:7-14); after the eigen-free scaling only W = GG'
  // exists: H = ((BW) B').^2 against a dense copy of B -- the same matrix
  const bool fromW = !b.have_G;
  if (fromW && !b.have_W) return set_error(c, LRN_ERR_STATE, "rank-one mode needs G or W (lrn_prepare_w / lrn_set_scaling)");
  LRN_TRY(ensure(c, c->BG, (size_t)m * n * 8));
  if (fromW && !b.have_Bd) {
    LRN_TRY(ensure(c, b.Bd, (size_t)m * n * 8));
    LRN_HIP(c, hipMemsetAsync(b.Bd.p, 0, (size_t)m * n * 8, c->stream));
    hipLaunchKernelGGL(b_dense_kernel, dim3(n), dim3(64), 0, c->stream, b.b_ptr.as<long>(), b.b_col.as<int>(),
                       b.b_val.as<double>(), m, b.Bd.as<double>());
    b.have_Bd = true;
  }
  tic(c);
  hipLaunchKernelGGL(bg_kernel, dim3(n), dim3(256), 0, c->stream, b.b_ptr.as<long>(), b.b_col.as<int>(),
                     b.b_val.as<double>(), fromW ? b.W.as<double>() : b.G.as<double>(), m, c->BG.as<double>());
  // owned column blocks of the lower triangle (all of it on one GPU)
  std::vector<std::pair<int, int>> cols;
  if (c->world > 1) {
    for (int c0 = 0; c0 < n; c0 += c->shard_bs)
      if (shard_owner(c0 / c->shard_bs, c->world) == c->rank) cols.push_back({c0, std::min(n, c0 + c->shard_bs)});
  } else {
    cols.push_back({0, n});
  }
  for (auto& cb : cols) {
    const int c0 = cb.first, c1 = cb.second;
    GemmDesc g;     // H[c0:, c0:c1] += ((BG BG')[c0:, c0:c1]).^2, lower tiles of the sub-block
    g.A = c->BG.as<double>() + (long)c0 * m; g.sAm = m; g.sAk = 1;
    g.B = (fromW ? b.Bd.as<double>() : c->BG.as<double>()) + (long)c0 * m; g.sBk = 1; g.sBn = m;
    g.C = c->H.as<double>() + (long)c0 + (long)c0 * n; g.sCm = 1; g.sCn = n;
    g.M = n - c0; g.N = c1 - c0; g.K = m;
    g.beta = 1.0;
    g.flags = GEMM_TRI_LOWER | GEMM_SQUARE;
    LRN_TRY(gemm(c->stream, g));
  }
  toc(c, "rank1");
  return LRN_OK;
}

// Rank-k data (mode 1): A_k = V_k diag(d_k) V_k' with every constraint padded to khat columns (zero columns of weight 0).
// With U = G' V (or W V against the dense copy of V when only W exists, as assemble_rank1 does) and T = U' U (U' V):
//     H_ij = tr(A_i W A_j W) = sum_{p in i, q in j} d_p d_q (u_p' v_q)^2,
// the entrywise square of T weighted by d d' and summed over khat x khat blocks -- one MFMA product whose epilogue does
// all of that (GEMM_SQUARE_BLOCKSUM), T never stored.  A sign flip of a whole constraint leaves H unchanged, so the sign
// convention of AA (row j = -vec(A_j)) does not matter here.  Blocks accumulate (beta = 1) into the zeroed H.
// the dense copy Vd (msz x nvar khat) of the uploaded factors: built on first use, at lrn_set_factored for a factored block
int lowrank_dense_factors(lrn_ctx* c, LmiBlock& b) {
  if (b.have_Vd) return LRN_OK;
  if (!b.has_V) return set_error(c, LRN_ERR_STATE, "no rank-k factors were uploaded (lrn_upload_lowrank)");
  const int m = b.msz;
  const long R = (long)c->nvar * b.lr_khat;
  LRN_TRY(ensure(c, b.Vd, (size_t)m * R * 8));
  LRN_HIP(c, hipMemsetAsync(b.Vd.p, 0, (size_t)m * R * 8, c->stream));
  hipLaunchKernelGGL(b_dense_kernel, dim3((unsigned)R), dim3(64), 0, c->stream, b.v_ptr.as<long>(), b.v_col.as<int>(),
                     b.v_val.as<double>(), m, b.Vd.as<double>());
  b.have_Vd = true;
  return LRN_OK;
}

static int assemble_lowrank(lrn_ctx* c, LmiBlock& b) {
  const int n = c->nvar, m = b.msz;
  if (!b.has_V) return set_error(c, LRN_ERR_STATE, "rank-k mode requested but no factors were uploaded (lrn_upload_lowrank)");
  const bool fromW = !b.have_G;
  if (fromW && !b.have_W) return set_error(c, LRN_ERR_STATE, "rank-k mode needs G or W (lrn_prepare_w / lrn_set_scaling)");
  const int kh = b.lr_khat;
  const long R = (long)n * kh;
  const double* M = fromW ? b.W.as<double>() : b.G.as<double>();
  // U by one dense product or by a gather over the stored factor entries: the gather reads nnz * msz words of G / W, the
  // product does 2 R msz^2 flop -- the gather wins below a density of about 2 %
  const bool dense = c->opt.lowrank_form == 1 || (c->opt.lowrank_form < 0 && (double)b.vnnz > 0.02 * (double)R * m);
  if (dense || fromW) LRN_TRY(lowrank_dense_factors(c, b));
  LRN_TRY(ensure(c, c->BG, (size_t)m * R * 8));
  double* U = c->BG.as<double>();
  tic(c);
  if (dense) {
    GemmDesc g;     // U = G' Vd (or W Vd), msz x R
    g.A = M;
    if (fromW) { g.sAm = 1; g.sAk = m; } else { g.sAm = m; g.sAk = 1; }
    g.B = b.Vd.as<double>(); g.sBk = 1; g.sBn = m;
    g.C = U; g.sCm = 1; g.sCn = m;
    g.M = m; g.N = (int)R; g.K = m;
    LRN_TRY(gemm(c->stream, g));
  } else {
    hipLaunchKernelGGL(lowrank_gather_kernel, dim3((unsigned)R), dim3(256), 0, c->stream, b.v_ptr.as<long>(),
                       b.v_col.as<int>(), b.v_val.as<double>(), M, m, fromW ? 1 : 0, U);
  }
  toc(c, "lowrank_u");     // (U alone; "lowrank" below: U and the blocked product, from the same start)
  // owned column blocks of the lower triangle (all of it on one GPU): H column j <-> U columns j kh .. j kh + kh - 1
  std::vector<std::pair<int, int>> cols;
  if (c->world > 1) {
    for (int c0 = 0; c0 < n; c0 += c->shard_bs)
      if (shard_owner(c0 / c->shard_bs, c->world) == c->rank) cols.push_back({c0, std::min(n, c0 + c->shard_bs)});
  } else {
    cols.push_back({0, n});
  }
  for (auto& cb : cols) {
    const int c0 = cb.first, c1 = cb.second;
    const long u0 = (long)c0 * kh * m;
    GemmDesc g;     // H[c0:, c0:c1] += blocksum(d d' .* (U' U)[c0 kh:, c0 kh:c1 kh].^2), lower blocks
    g.A = U + u0; g.sAm = m; g.sAk = 1;
    g.B = (fromW ? b.Vd.as<double>() : U) + u0; g.sBk = 1; g.sBn = m;
    g.C = c->H.as<double>() + (long)c0 + (long)c0 * n; g.sCm = 1; g.sCn = n;
    g.M = (n - c0) * kh; g.N = (c1 - c0) * kh; g.K = m;
    g.beta = 1.0;
    g.flags = GEMM_TRI_LOWER | GEMM_SQUARE_BLOCKSUM;
    g.blk_w = b.v_w.as<double>() + (long)c0 * kh;
    g.blk_k = kh;
    LRN_TRY(gemm(c->stream, g));
  }
  toc(c, "lowrank");
  if (!c->profile) c->counts["lowrank"] += 1;     // (the route is counted whether or not the phases are timed)
  return LRN_OK;
}

// ---- hybrid factored block: a few constraints S are stored (positions [0, npos_nz)), the others F are factors.  H has three
// parts: H_FF by assemble_lowrank (the stored positions have weight-0 columns and receive + 0), H_SS by assemble_dense /
// assemble_sparse over the stored positions, and the cross terms, with Y = W Vd (msz x R, column hidx[j] khat + p):
//     H_sj = tr(A_s W A_j W) = sum_p d_jp y_jp' A_s y_jp            (A_s from ent_v = +A, d from v_w = +d: the signs agree)
// a sparse quadratic form per column of Y, nnz(A_s) R multiply-adds per stored constraint.
//
// fac_cross_kernel: workgroup (x, y) owns the factored position j = p_f + x and the 32 sparse-tier stored positions
// s0 + 32 y ..; wave v takes the stored positions s0 + 32 y + 4 t + v, t < 8, and keeps their sums in registers.  The khat
// columns of Y of position j are staged in LDS one at a time (LDS: msz * 8 bytes, up to 32 KiB -- five workgroups per CU) or,
// for longer columns, gathered from global memory by the same code; lanes stride the entry list of A_s, one shuffle tree
// adds in a fixed order, the sum is weighted by d_jp and added over p in order.  Each workgroup writes its 32 entries of the
// lower triangle of H exactly once, += because the blocks of a model share H.  No atomics: two assemblies give the same bits.
template <bool LDS>
__global__ __launch_bounds__(256) void fac_cross_kernel(const long* __restrict__ ptr, const int* __restrict__ er,
                                                        const int* __restrict__ ec, const double* __restrict__ ev,
                                                        const double* __restrict__ Y, const double* __restrict__ w, int m, int kh,
                                                        int s_lo, int s_hi, int p_f, int p_end,
                                                        const int* __restrict__ hidx, double* __restrict__ H, int ldh) {
  extern __shared__ double ycol[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = p_f + blockIdx.x;
  if (j >= p_end) return;                        // (whole workgroup)
  const int hj = hidx[j];
  const int sb = s_lo + blockIdx.y * 32 + wave;
  double acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = 0.0;
  for (int p = 0; p < kh; ++p) {
    const long col = (long)hj * kh + p;
    const double wp = w[col];
    if (wp == 0.0) continue;                     // padding column (uniform over the workgroup)
    const double* __restrict__ yg = Y + col * m;
    if (LDS) {
      __syncthreads();                           // the waves are done with the previous column
      for (int r = threadIdx.x; r < m; r += 256) ycol[r] = yg[r];
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int sp = sb + 4 * t;                 // wave-uniform
      if (sp >= s_hi) continue;
      double q = 0.0;
      for (long e = ptr[sp] + lane; e < ptr[sp + 1]; e += 64) {
        const int r = er[e], cc = ec[e];
        q += ev[e] * (LDS ? ycol[r] * ycol[cc] : yg[r] * yg[cc]);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) q += __shfl_down(q, off, 64);
      acc[t] += wp * q;
    }
  }
  if (lane != 0) return;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int sp = sb + 4 * t;
    if (sp >= s_hi) continue;
    const int hs = hidx[sp];
    const int rr = hs > hj ? hs : hj, cc = hs > hj ? hj : hs;
    H[(long)rr + (long)cc * ldh] += acc[t];
  }
}

// stored constraint in dense slot s: Q = A_s Y is one product, H_sj = sum_p d_jp <Q(:, jp), Y(:, jp)> one wave per factored
// position j (the column dot of dataops.hip::fac_coldot_kernel), written once
__global__ __launch_bounds__(256) void fac_cross_coldot_kernel(const double* __restrict__ Q, const double* __restrict__ Y,
                                                               const double* __restrict__ w, int m, int kh, int s, int p_f,
                                                               int p_end, const int* __restrict__ hidx, double* __restrict__ H,
                                                               int ldh) {
  const int lane = threadIdx.x & 63;
  const int j = p_f + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= p_end) return;
  const int hj = hidx[j];
  double acc = 0.0;
  for (int p = 0; p < kh; ++p) {
    const long col = (long)hj * kh + p;
    const double wp = w[col];
    if (wp == 0.0) continue;
    const double* __restrict__ q = Q + col * m;
    const double* __restrict__ y = Y + col * m;
    double t = 0.0;
    for (int r = lane; r < m; r += 64) t += q[r] * y[r];
    acc += wp * t;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane != 0) return;
  const int hs = hidx[s];
  const int rr = hs > hj ? hs : hj, cc = hs > hj ? hj : hs;
  H[(long)rr + (long)cc * ldh] += acc;
}

static int assemble_cross(lrn_ctx* c, LmiBlock& b) {
  const int n = c->nvar, m = b.msz, kh = b.lr_khat;
  const long R = (long)n * kh;
  if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set (call lrn_prepare_w or lrn_set_scaling)");
  const int nf = n - b.npos_nz;
  if (nf <= 0) return LRN_OK;
  // Y = W Vd: what assemble_lowrank left in BG when only W exists, one more product into a workspace of its own otherwise
  const double* Y = c->BG.as<double>();
  tic(c);
  if (b.have_G) {
    LRN_TRY(ensure(c, c->facY, (size_t)m * R * 8));
    GemmDesc g;
    g.A = b.W.as<double>(); g.sAm = 1; g.sAk = m;
    g.B = b.Vd.as<double>(); g.sBk = 1; g.sBn = m;
    g.C = c->facY.as<double>(); g.sCm = 1; g.sCn = m;
    g.M = m; g.N = (int)R; g.K = m;
    LRN_TRY(gemm(c->stream, g));
    Y = c->facY.as<double>();
  }
  toc(c, "hybrid_y");
  tic(c);
  if (b.npos_nz > b.nd) {
    const size_t cap = c->opt.fac_cross_lds == 1 ? 65536 : 32768;      // bytes of one column: forced / by default
    const bool lds = c->opt.fac_cross_lds != 0 && (size_t)m * 8 <= cap;
    const dim3 grid((unsigned)nf, (unsigned)((b.npos_nz - b.nd + 31) / 32));
#define LRN_CROSS_LAUNCH(L, SH)                                                                                        \
  hipLaunchKernelGGL(fac_cross_kernel<L>, grid, dim3(256), SH, c->stream, b.ent_ptr.as<long>(), b.ent_r.as<int>(),    \
                     b.ent_c.as<int>(), b.ent_v.as<double>(), Y, b.v_w.as<double>(), m, kh, b.nd, b.npos_nz, b.npos_nz, n, \
                     b.hidx.as<int>(), c->H.as<double>(), n)
    if (lds) LRN_CROSS_LAUNCH(true, (size_t)m * 8);
    else LRN_CROSS_LAUNCH(false, 0);
#undef LRN_CROSS_LAUNCH
    c->counts[lds ? "hybrid_cross_lds" : "hybrid_cross_global"] += 1;
  }
  if (b.nd > 0) {
    LRN_TRY(ensure(c, c->P, (size_t)m * R * 8));
    double* Q = c->P.as<double>();
    for (int s = 0; s < b.nd; ++s) {
      GemmDesc g;     // Q = A_s Y
      g.A = b.Adense.as<double>() + (long)s * m * m; g.sAm = 1; g.sAk = m;
      g.B = Y; g.sBk = 1; g.sBn = m;
      g.C = Q; g.sCm = 1; g.sCn = m;
      g.M = m; g.N = (int)R; g.K = m;
      LRN_TRY(gemm(c->stream, g));
      hipLaunchKernelGGL(fac_cross_coldot_kernel, dim3((nf + 3) / 4), dim3(256), 0, c->stream, Q, Y, b.v_w.as<double>(), m, kh,
                         s, b.npos_nz, n, b.hidx.as<int>(), c->H.as<double>(), n);
    }
    c->counts["hybrid_cross_dense"] += 1;
  }
  toc(c, "hybrid_cross");
  return LRN_OK;
}

int schur_assemble(lrn_ctx* c, int mode) {
  const int n = c->nvar;
  if (n <= 0) return set_error(c, LRN_ERR_STATE, "no model uploaded");
  if (c->world > 1 && !c->pos_space)
    return set_error(c, LRN_ERR_STATE, "Schur column sharding needs a single LMI block (sigma-position space)");
  hipEvent_t a0, a1;
  if (c->profile) {
    (void)hipEventCreate(&a0);
    (void)hipEventCreate(&a1);
    (void)hipEventRecord(a0, c->stream);
  }
  for (const auto& b : c->lmi)
    if (b.factored && mode != 1)
      return set_error(c, LRN_ERR_STATE, "lrn_schur_assemble: mode %d on a factored block (lrn_set_factored): its constraints "
                                         "exist as factors only, mode 1 assembles from them", mode);
  for (const auto& b : c->lmi)
    if (b.hybrid() && c->world > 1)
      return set_error(c, LRN_ERR_STATE, "lrn_schur_assemble: mode 1 on a factored block with stored constraints runs on one "
                                         "GPU (the cross terms are not sharded)");
  LRN_HIP(c, hipMemsetAsync(c->H.p, 0, (size_t)n * n * 8, c->stream));
  c->H_partial = false;
  c->H_owned_only = false;
  for (auto& b : c->lmi) {
    if (mode == -1) {
      LRN_TRY(assemble_rank1(c, b));
      continue;
    }
    if (mode == 1 && !b.factored && b.has_V && b.v_partial) {
      // factors for some constraints only, and the block is not factored: its AA holds every constraint (a hybrid model the
      // host materialised), the factors do not -- the general assembly over the entries is the exact one
      if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set (call lrn_prepare_w or lrn_set_scaling)");
      if (b.nd > 0) LRN_TRY(assemble_dense(c, b));
      if (b.npos_nz > b.nd) LRN_TRY(assemble_sparse(c, b));
      c->counts["lowrank_from_entries"] += 1;
      continue;
    }
    if (mode == 1) {
      if (b.hybrid()) {     // H_SS from the stored entries, then H_FF and the cross terms (see assemble_cross)
        if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set (call lrn_prepare_w or lrn_set_scaling)");
        if (b.nd > 0) LRN_TRY(assemble_dense(c, b));
        if (b.npos_nz > b.nd) LRN_TRY(assemble_sparse(c, b));
      }
      LRN_TRY(assemble_lowrank(c, b));
      if (b.hybrid()) LRN_TRY(assemble_cross(c, b));
      continue;
    }
    if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set (call lrn_prepare_w or lrn_set_scaling)");
    if (b.nd > 0) LRN_TRY(assemble_dense(c, b));
    if (b.npos_nz > b.nd) LRN_TRY(assemble_sparse(c, b));
  }
  if (c->nlin > 0) {
    tic(c);
    if (c->lp_n > 0)
      hipLaunchKernelGGL(lin_schur_kernel, dim3((unsigned)((c->lp_n + 255) / 256)), dim3(256), 0, c->stream,
                         c->lp_r.as<int>(), c->lp_c.as<int>(), c->lp_ptr.as<long>(), c->lp_l.as<int>(),
                         c->lp_w.as<double>(), c->lp_n, c->lin_xs.as<double>(), c->H.as<double>(), n, c->rank, c->world,
                         c->shard_bs);
    toc(c, "lin");
  }
  if (c->profile) {
    (void)hipEventRecord(a1, c->stream);
    (void)hipEventSynchronize(a1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a0, a1);
    c->timing["assemble"] += ms;
    c->counts["assemble"] += 1;
    (void)hipEventDestroy(a0);
    (void)hipEventDestroy(a1);
  }
  LRN_HIP(c, hipGetLastError());
  c->have_H = true;
  c->H_shifted = false;
  c->have_L = false;
  c->H_version = c->scal_version;
  c->H_mode = mode;
  return LRN_OK;
}

int schur_add_diag(lrn_ctx* c, double eps) {
  if (!c->have_H) return set_error(c, LRN_ERR_STATE, "no assembled H");
  hipLaunchKernelGGL(add_diag_kernel, dim3((c->nvar + 255) / 256), dim3(256), 0, c->stream, c->H.as<double>(),
                     c->nvar, eps);
  c->have_L = false;
  if (eps != 0.0) c->H_shifted = true;
  return LRN_OK;
}

int schur_get(lrn_ctx* c, double* Hout) {
  if (!c->have_H) return set_error(c, LRN_ERR_STATE, "no assembled H");
  const int n = c->nvar;
  size_t bytes = (size_t)n * n * 8;
  LRN_TRY(ensure(c, c->slabs, bytes));     // assembly scratch doubles as staging
  const int* ipos = c->pos_space ? c->lmi[0].ipos_d.as<int>() : nullptr;
  hipLaunchKernelGGL(export_h_kernel, dim3(nblocks((long)n * n)), dim3(256), 0, c->stream, c->H.as<double>(), n,
                     ipos, c->slabs.as<double>());
  return copy_out(c, Hout, c->slabs.p, bytes);
}

int schur_factor(lrn_ctx* c, int* info) {
  if (!c->have_H) return set_error(c, LRN_ERR_STATE, "no assembled H");
  if (c->H_owned_only) return set_error(c, LRN_ERR_STATE, "H holds only this rank's column blocks (call lrn_schur_assemble)");
  const int n = c->nvar;
  size_t bytes = (size_t)n * n * 8;
  LRN_TRY(ensure(c, c->L, bytes));
  LRN_TRY(ensure(c, c->cholwork, chol_work_doubles(n) * 8));
  hipEvent_t a0, a1;
  if (c->profile) { (void)hipEventCreate(&a0); (void)hipEventCreate(&a1); (void)hipEventRecord(a0, c->stream); }
  // H is positive semidefinite by construction; late in a solve its smallest eigenvalues sink below the
  // rounding level of the assembly (tru9: lambda_min = -1e-3 at |H| = 4e12).  Pivots at that level are
  // boosted instead of failing the factorisation.  If more than max(8, n/64) pivots are affected the
  // attempt is abandoned and the strict factorisation decides -- this library never fails where a plain
  // Cholesky succeeds --, and once the caller has entered the reference's +1e-4 I loop (:59-85,
  // lrn_schur_add_diag) only the strict factorisation is used, as there.
  LRN_TRY(ensure(c, c->hdiag, (size_t)n * 8));
  int h_two[2] = {0, 0};
  const bool try_boost = c->opt.pivot_boost > 0.0 && !c->H_shifted;
  for (int attempt = try_boost ? 0 : 1; attempt < 2; ++attempt) {
    LRN_HIP(c, hipMemcpyAsync(c->L.p, c->H.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 8, c->stream));
    if (attempt == 0)
      hipLaunchKernelGGL(get_diag_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->H.as<double>(), n,
                         c->hdiag.as<double>());
    LRN_TRY(potrf_lower_boost(c->stream, c->L.as<double>(), n, n, c->cholwork.as<double>(), c->info_dev.as<int>(),
                              attempt == 0 ? c->hdiag.as<double>() : nullptr, c->opt.pivot_boost, std::max(8, n / 64)));
    LRN_HIP(c, hipMemcpyAsync(h_two, c->info_dev.p, 8, hipMemcpyDeviceToHost, c->stream));
    LRN_HIP(c, hipStreamSynchronize(c->stream));
    if (h_two[0] == 0) break;
  }
  if (c->profile) { (void)hipEventRecord(a1, c->stream); }
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  if (c->profile) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a0, a1);
    c->timing["factor"] += ms; c->counts["factor"] += 1;
    (void)hipEventDestroy(a0); (void)hipEventDestroy(a1);
  }
  const int h_info = h_two[0];
  c->counts["chol_boosted"] = h_two[1];
  if (info) *info = h_info;
  c->have_L = (h_info == 0);
  return LRN_OK;
}

int schur_solve(lrn_ctx* c, const double* h, double* dely) {
  if (!c->have_L) return set_error(c, LRN_ERR_STATE, "no factor (call lrn_schur_factor)");
  const int n = c->nvar;
  hipEvent_t a0, a1;
  LRN_TRY(copy_in(c, c->v0.p, h, (size_t)n * 8));
  if (c->profile) { (void)hipEventCreate(&a0); (void)hipEventCreate(&a1); (void)hipEventRecord(a0, c->stream); }
  const int* sig = c->pos_space ? c->lmi[0].sigma_d.as<int>() : nullptr;
  unsigned nb = (unsigned)((n + 255) / 256);
  // position space: hs[p] = h[sigma[p]]
  hipLaunchKernelGGL(gather_vec_kernel, dim3(nb), dim3(256), 0, c->stream, c->v0.as<double>(), sig, c->v1.as<double>(), n);
  LRN_TRY(potrs_vec(c->stream, c->L.as<double>(), n, n, c->v1.as<double>(), c->v0.as<double>(), c->v2.as<double>(),
                    c->v3.as<double>()));
  hipLaunchKernelGGL(scatter_vec_kernel, dim3(nb), dim3(256), 0, c->stream, c->v0.as<double>(), sig, c->v1.as<double>(), n);
  if (c->profile) {
    (void)hipEventRecord(a1, c->stream);
    (void)hipEventSynchronize(a1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a0, a1);
    c->timing["solve"] += ms; c->counts["solve"] += 1;
    (void)hipEventDestroy(a0); (void)hipEventDestroy(a1);
  }
  return copy_out(c, dely, c->v1.p, (size_t)n * 8);
}

}  // namespace lrn
