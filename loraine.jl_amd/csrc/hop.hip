// CG operator through the ASSEMBLED Schur matrix (round 4).
//
// MyA (reference src/Solvers.jl:582-614) applies  Ax = AA vec(W mat(AA'x) W)  matrix-free because a CPU cannot afford
// the nvar x nvar matrix H of src/makeBBBB.jl:67-218 for every IP iteration.  It is the same linear map: Ax = H x.
// On an MI355X H fits up to nvar ~ 1.5e5 and its assembly is cheap next to hundreds of operator applications (C5: 66 ms
// against 729 applications of 2.6 ms), so when the cost model below says so the operator of lrn_pcg / lrn_matvec is
//   assemble H once per NT scaling (the kit=0 kernels of schur*.hip), then  y = H x  per CG iteration
// as ONE pass over the LOWER triangle: 4 nvar^2 bytes per application, the HBM roofline of the CG iteration.
//
// symv_lower_tiles_kernel: workgroup tile = 128 K rows x 128 columns of the lower triangle (column-major: a wave reads
// 1 KB of one column per load instruction, 16 B per lane).  Every element H[r,c], r >= c, is used twice while in
// registers: y[c] += H[r,c] x[r] (column sums: per-lane partials over the K row segments, one reduce-scatter butterfly
// per four columns) and, for r > c, y[r] += H[r,c] x[c] (row sums: registers across the tile's columns, the four waves
// combined through LDS).  Partial results go to slabs indexed by row block / column chunk and are added in a fixed
// order by symv_lower_reduce_kernel: no floating-point atomics, the result is bit-reproducible.
// One process per GPU: a rank applies the column chunks it owns (the block-cyclic ownership of the Schur columns,
// lrn_common.h::shard_owner) -- with column-block assembly these are the columns it assembled, no exchange of H at
// all -- and the nvar-vector is all-reduced as for the matrix-free operator.
#include <algorithm>
#include <cmath>

#include "../../include/loraine_hip.h"
#include "ctx.h"
#include "ops.h"

namespace lrn {

typedef double v2d __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double shx(double v, int mask) { return __shfl_xor(v, mask, 64); }

// VEC2: rows 2 lane, 2 lane + 1 of each 128-row segment (one 16-byte load; n even); else rows lane, lane + 64
template <int K, bool VEC2, bool MASK>
__device__ __forceinline__ void symv_tile_body(const double* __restrict__ H, int n, int r0, int cw0, int lane,
                                               const double* __restrict__ xs_w, const double (&xr)[K][2],
                                               double (&yr)[K][2], double* __restrict__ colout) {
  const int ra = VEC2 ? 2 * lane : lane, rb = VEC2 ? 2 * lane + 1 : lane + 64;
#pragma unroll 1
  for (int g = 0; g < 32; g += 4) {
    double h[K][4][2];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int rs = r0 + 128 * k;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = cw0 + g + j;
        h[k][j][0] = 0.0;
        h[k][j][1] = 0.0;
        // (wave-uniform) skip of segments that lie entirely above the diagonal of this column
        if (c < n && (!MASK || rs + 127 >= c)) {
          const double* col = H + (size_t)c * n + rs;
          if (VEC2) {
            if (rs + ra < n) {
              const v2d v = *reinterpret_cast<const v2d*>(col + ra);
              h[k][j][0] = v.x;
              h[k][j][1] = v.y;
            }
          } else {
            if (rs + ra < n) h[k][j][0] = col[ra];
            if (rs + rb < n) h[k][j][1] = col[rb];
          }
        }
      }
    }
    double cs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cw0 + g + j;
      const double xc = xs_w[g + j];
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int rs = r0 + 128 * k;
        double a = h[k][j][0], b = h[k][j][1];
        if (MASK) {                      // the upper triangle is not authoritative (and may hold anything): select, not multiply
          a = (rs + ra >= c) ? a : 0.0;
          b = (rs + rb >= c) ? b : 0.0;
        }
        s += a * xr[k][0] + b * xr[k][1];
        if (MASK) {
          a = (rs + ra > c) ? a : 0.0;
          b = (rs + rb > c) ? b : 0.0;
        }
        yr[k][0] += a * xc;
        yr[k][1] += b * xc;
      }
      cs[j] = s;
    }
    // reduce-scatter over the 64 lanes: lanes [0,32) keep columns 0,1, lanes [32,64) columns 2,3; then by bit 4
    const bool hi5 = (lane & 32) != 0, hi4 = (lane & 16) != 0;
    double k0 = (hi5 ? cs[2] : cs[0]) + shx(hi5 ? cs[0] : cs[2], 32);
    double k1 = (hi5 ? cs[3] : cs[1]) + shx(hi5 ? cs[1] : cs[3], 32);
    double kk = (hi4 ? k1 : k0) + shx(hi4 ? k0 : k1, 16);
    kk += shx(kk, 8);
    kk += shx(kk, 4);
    kk += shx(kk, 2);
    kk += shx(kk, 1);
    if ((lane & 15) == 0) {
      const int c = cw0 + g + 2 * (lane >> 5) + ((lane >> 4) & 1);
      if (c < n) colout[c] = kk;
    }
  }
}

template <int K, bool VEC2>
__global__ __launch_bounds__(256) void symv_lower_tiles_kernel(const double* __restrict__ H, int n,
                                                               const int* __restrict__ idx, const double* __restrict__ x,
                                                               double* __restrict__ colpart, double* __restrict__ rowpart,
                                                               int rank, int world, int shard_bs) {
  constexpr int RB = 128 * K;
  const int J = blockIdx.x, I = blockIdx.y;
  const int r0 = I * RB, c0 = J * 128;
  if (c0 >= r0 + RB || c0 >= n || r0 >= n) return;            // tile entirely above the diagonal / outside
  if (world > 1 && shard_owner(c0 / shard_bs, world) != rank) return;
  __shared__ double xs[128];
  __shared__ double rsum[4][RB];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  if (t < 128) {
    const int cc = c0 + t;
    xs[t] = cc < n ? x[idx ? idx[cc] : cc] : 0.0;
  }
  const int ra = VEC2 ? 2 * lane : lane, rb = VEC2 ? 2 * lane + 1 : lane + 64;
  double xr[K][2], yr[K][2];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int a = r0 + 128 * k + ra, b = r0 + 128 * k + rb;
    xr[k][0] = a < n ? x[idx ? idx[a] : a] : 0.0;
    xr[k][1] = b < n ? x[idx ? idx[b] : b] : 0.0;
    yr[k][0] = 0.0;
    yr[k][1] = 0.0;
  }
  __syncthreads();
  double* colout = colpart + (size_t)I * n;
  if (c0 + 127 >= r0)
    symv_tile_body<K, VEC2, true>(H, n, r0, c0 + 32 * w, lane, xs + 32 * w, xr, yr, colout);
  else
    symv_tile_body<K, VEC2, false>(H, n, r0, c0 + 32 * w, lane, xs + 32 * w, xr, yr, colout);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    rsum[w][128 * k + ra] = yr[k][0];
    rsum[w][128 * k + rb] = yr[k][1];
  }
  __syncthreads();
  double* rowout = rowpart + (size_t)J * n;
  for (int i = t; i < RB; i += 256)
    if (r0 + i < n) rowout[r0 + i] = (rsum[0][i] + rsum[1][i]) + (rsum[2][i] + rsum[3][i]);
}

// y[idx[i]] = sum of the partials of row / column i in a fixed order: 64 outputs per workgroup, the slabs dealt to
// the four waves (slab s to wave s % 4), the four sums added through LDS.  qpart (may be null): per-workgroup partial
// sums of x[idx[i]] y[idx[i]] -- the p'Ap of the CG iteration without another pass over the vectors.
__global__ __launch_bounds__(256) void symv_lower_reduce_kernel(const double* __restrict__ colpart,
                                                                const double* __restrict__ rowpart, int n, int RB,
                                                                const int* __restrict__ idx, const double* __restrict__ x,
                                                                double* __restrict__ y, double* __restrict__ qpart,
                                                                int rank, int world, int shard_bs) {
  __shared__ double sh[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  double s = 0.0;
  if (i < n) {
    const int nrb = (n + RB - 1) / RB;
    const int J = i >> 7;
    const int I0 = (J * 128) / RB;
    const int ncol = (world <= 1 || shard_owner((J * 128) / shard_bs, world) == rank) ? nrb - I0 : 0;
    const int Jmax = min((n - 1) >> 7, ((i / RB) * RB + RB - 1) >> 7);
    // unified slab list: [0, ncol) column slabs I0 + k, then the row slabs 0 .. Jmax
    for (int k = w; k < ncol; k += 4) s += colpart[(size_t)(I0 + k) * n + i];
    for (int k = ((w - ncol) % 4 + 4) % 4; k <= Jmax; k += 4)
      if (world <= 1 || shard_owner((k * 128) / shard_bs, world) == rank) s += rowpart[(size_t)k * n + i];
  }
  sh[w][lane] = s;
  __syncthreads();
  if (w == 0) {
    double v = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
    double q = 0.0;
    if (i < n) {
      const int o = idx ? idx[i] : i;
      y[o] = v;
      q = x[o] * v;
    }
    if (qpart) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) q += __shfl_down(q, off, 64);
      if (lane == 0) qpart[blockIdx.x] = q;
    }
  }
}

static bool hop_shardable(const lrn_ctx* c) {
  return c->pos_space && c->shard_bs > 0 && c->shard_bs % 128 == 0;
}

// y = H x (natural constraint order on both sides; H lives in sigma-position space when nlmi == 1).  world > 1: this
// rank's column chunks only, the caller all-reduces.
// y = A x for a symmetric n x n matrix of which the lower triangle is read (idx: permutation of both sides or null)
int symv_lower(lrn_ctx* c, const double* H, int n, const int* idx, const double* x, double* y, double* qpart, int* nq,
               bool sharded) {
  const bool small = n < 8192;
  const int K = small ? 1 : 4, RB = 128 * K;
  const int nrb = (n + RB - 1) / RB, nch = (n + 127) / 128;
  LRN_TRY(ensure(c, c->hopbuf, (size_t)(nrb + nch) * n * 8));
  double* colpart = c->hopbuf.as<double>();
  double* rowpart = colpart + (size_t)nrb * n;
  const int rank = sharded ? c->rank : 0, world = sharded ? c->world : 1;
  const dim3 grid(nch, nrb);
  const bool vec2 = (n & 1) == 0;
#define LRN_SYMV(KK, VV)                                                                                               \
  hipLaunchKernelGGL((symv_lower_tiles_kernel<KK, VV>), grid, dim3(256), 0, c->stream, H, n, idx, x, colpart, rowpart, \
                     rank, world, c->shard_bs)
  if (small) { if (vec2) LRN_SYMV(1, true); else LRN_SYMV(1, false); }
  else { if (vec2) LRN_SYMV(4, true); else LRN_SYMV(4, false); }
#undef LRN_SYMV
  // (sharded: the partial products x'y would be those of this rank's share -- the caller forms the dot after the all-reduce)
  double* qp = sharded ? nullptr : qpart;
  hipLaunchKernelGGL(symv_lower_reduce_kernel, dim3((n + 63) / 64), dim3(256), 0, c->stream, colpart, rowpart, n, RB,
                     idx, x, y, qp, rank, world, c->shard_bs);
  if (nq) *nq = qp ? (n + 63) / 64 : 0;
  return LRN_OK;
}

int hop_apply(lrn_ctx* c, const double* x, double* y, double* qpart, int* nq) {
  if (!c->have_H) return set_error(c, LRN_ERR_STATE, "no assembled H");
  c->counts["hop_matvec"] += 1;
  return symv_lower(c, c->H.as<double>(), c->nvar, c->pos_space ? c->lmi[0].sigma_d.as<int>() : nullptr, x, y, qpart, nq,
                    c->comm && c->world > 1);
}

// ------------------------------------------------------------------ cost model (static: the choice must not depend on
// measured times, or two runs of one problem would differ at rounding level)
//
// Option "cg_lowrank" (0 never, 1 always, -1 by the terms below): a COVERED block (cg_lowrank_covered: not factored, factors
// for every constraint that has entries) can serve each piece of the CG path from its rank-k factors instead of its
// entries -- the assembly of H in mode 1, the matrix-free operator in factor form, ts of H_alpha (facops.hip::fac_ts_kernel).
// The three terms est_assemble_s(., 1), est_operator_block_s(., ., true) and est_ts_s(., ., ., true) carry rates measured at
// msz 2000 / nvar 4000 / rank 2 (DESIGN.md sections 10, 11, 14).  With world > 1 the option is ignored and the entry routes
// run: the factor routes are not sharded, and no multi-GPU machine was there to test anything else.
static bool cg_lowrank_on(const lrn_ctx* c) { return c->opt.cg_lowrank != 0 && c->world <= 1; }

static double est_operator_block_s(const lrn_ctx* c, const LmiBlock& b, bool factors) {
  const double m = b.msz;
  if (factors) {      // Q = Z Vd (2 m^2 R flop) and the lower triangle of Vs Vd' (m^2 R), the two products of wmw; as many launches
    // as the entry route (section 11: 1.35 + 0.89 ms for 9.6e10 flop).  Option "ragged_ops": both run on the Rc compacted columns
    const double R = ragged_ops_on(c, b) ? (double)b.rg_Rc : (double)c->nvar * b.lr_khat;
    double t = 3.0 * m * m * R / 4.0e13 + 40e-6;
    if (!(b.factored && fac_op_scaled_on(c, b))) t += 4.0 * m * m * m / 5.0e13;      // (Y = W Vd: no W M W product)
    // hybrid block: its stored rows on top, twice (mat(AA' x) and AA vec(.)) -- the sparse tier at the pattern rate, the
    // dense slots as one pass over the slabs each
    if (b.hybrid()) t += 2.0 * ((double)b.nent * 1.43e-12 + (double)b.nd * m * m * 8.0 / 6.0e12) + 20e-6;
    // diagonal parts (option "cg_diag"): the two passes over Ad, dg_n x msz doubles each, three launches.  Section 16 measured
    // them inside aa_times / aat_to_mat only (no difference from the pure block within the spread, 4000 rows included): the
    // rate is the stream rate of the stored rows above, not a new measurement
    if (b.factored && b.dg_n > 0) t += 2.0 * (double)b.dg_n * m * 8.0 / 6.0e12 + 15e-6;
    return t;
  }
  if (use_sparse_matvec(c, b))
    return (b.msz < 1500 ? 30e-6 : 10e-6) + (double)b.ncq * m * 1.43e-12;      // pattern route (C5: 2.58 ms, C3: 36 us)
  return 4.0 * m * m * m / 5.0e13 + (double)b.nd * m * m * 8.0 / 6.0e12 + 40e-6;      // two products + two passes over the column tails
}

bool cg_lowrank_operator(const lrn_ctx* c, const LmiBlock& b) {
  if (!cg_lowrank_on(c) || !cg_lowrank_covered(b)) return false;
  return c->opt.cg_lowrank == 1 || est_operator_block_s(c, b, true) < est_operator_block_s(c, b, false);
}

static double est_operator_s(const lrn_ctx* c) {
  double t = 0.0;
  for (const auto& b : c->lmi) t += est_operator_block_s(c, b, b.factored || cg_lowrank_operator(c, b));
  return t;
}

// Options "fac_op_scaled" and "fac_quadform" (1 on, 0 off, -1 cost model), both inside matvec_dev and under "cg_factored"
// only.  The -1 branches choose a form only where it was MEASURED no slower than the parent's composition on one box
// (msz 320 / nvar 640 / rank 2, msz 2000 / nvar 4000 / rank 2, msz 256 / nvar 32768 / rank 1).
// Scaled factors: faster per application at all three shapes (0.077 -> 0.055, 2.73 -> 2.02, 0.430 -> 0.399 ms); Y = W Vd
// costs 0.02 / 1.27 / 0.09 ms per scaling, the gain of one to three applications -- on from msz 256 (the smallest side
// measured) when the previous scaling saw at least four operator applications (cg_prev_iters, constant within a scaling).
bool fac_op_scaled_on(const lrn_ctx* c, const LmiBlock& b) {
  if (!cg_factored_on(c) || !b.factored || b.hybrid() || b.dg_n > 0) return false;      // (a hybrid block keeps the composition; with
                                                                                          // diagonal parts W M W is not -Y diag Y')
  if (c->opt.fac_op_scaled >= 0) return c->opt.fac_op_scaled == 1;
  return b.msz >= 256 && c->cg_prev_iters >= 4;
}

// Fused quadratic form: slower at msz 320 and 2000, no slower only at msz 256 / R = 32768 -- the regime it was written for
// (m / 16 flop per byte of the Q round trip below the FP64 balance); -1 is on for msz <= 256 and R >= 32768, nothing else
// has been measured
bool fac_quadform_on(const lrn_ctx* c, const LmiBlock& b) {
  if (!cg_factored_on(c) || !b.factored) return false;
  if (c->opt.fac_quadform >= 0) return c->opt.fac_quadform == 1;
  return b.msz <= 256 && (long)c->nvar * b.lr_khat >= 32768;
}

// ts of H_alpha for one block and `erank` eigenvectors.  Entries: per eigenvector one pass over the dense slabs (one
// workgroup per slab, a column-strided walk: 1e12 B/s), the sparse entries, AU zeroed and multiplied by Z (2 nvar m^2 flop).
// Factors: P = L' Vd once (2 m^2 R flop), T = Vd' Um, then per eigenvector one pass over P and one over the block of ts.
static double est_ts_s(const lrn_ctx* c, const LmiBlock& b, int erank, bool factors) {
  const double m = b.msz, n = c->nvar, k = erank;
  if (factors) {
    const double R = ragged_ts_on(c, b) ? (double)b.rg_Rc : n * b.lr_khat;      // option "ragged_ts": on the Rc compacted columns
    return 2.0 * m * m * R / 4.0e13 + 2.0 * m * R * k / 1.0e13 + k * (m * R + m * n) * 8.0 / 3.0e12 + 20e-6;      // three launches in all
  }
  return k * ((double)b.nd * m * m * 8.0 / 1.0e12 + (double)(b.nent) * 2.0e-10 + n * m * 8.0 / 3.0e12 + 2.0 * n * m * m / 4.0e13 + 25e-6);
}

bool cg_lowrank_ts(const lrn_ctx* c, const LmiBlock& b, int erank) {
  if (!cg_lowrank_on(c) || !cg_lowrank_covered(b)) return false;
  return c->opt.cg_lowrank == 1 || est_ts_s(c, b, erank, true) < est_ts_s(c, b, erank, false);
}

static double est_assemble_s(const lrn_ctx* c, int mode) {
  const double n = c->nvar;
  double t = n * n * 8.0 / 4.0e12 + 100e-6;
  for (const auto& b : c->lmi) {
    const double m = b.msz, nd = b.nd;
    // mode 1 of a block with factors for every constraint (covered, or factored); a block beside a factored one that has
    // none takes the general assembly over its entries inside mode 1 (schur.hip): the mode-0 terms below
    if (mode == 1 && (b.factored || cg_lowrank_covered(b))) {
      // U = G' Vd and the blocked square of U' U on its lower triangle (section 10: 1.28e11 flop in 3.78 ms)
      const double R = n * b.lr_khat;
      // option "lowrank_ragged", and every wide block (khat 32 / 64): the two products run on the Rc compacted columns
      // (raggedops.hip); everything below stays on the padded layout
      const double Rp = lowrank_ragged_on(c, b) ? (double)b.rg_Rc : R;
      // option "ragged_cross": Y, the cross terms of a hybrid block and C of the diagonal parts on the compacted columns too
      const double Rx = ragged_cross_on(c, b) ? (double)b.rg_Rc : R;
      t += (2.0 * Rp * m * m + 0.5 * Rp * Rp * m) / 3.4e13;
      if (b.factored && b.dg_n > 0) {
        // diagonal parts (assemble_diag), at the rates section 16 MEASURED at msz 2000 / nvar 4000 / khat 2 / 4000 rows -- those
        // measurements, not new ones: C = Ad' (Y o Y), 2 dg_n m R = 128 GFLOP in 2.8 ms; H_DD = the squared product and the
        // lower tiles of P Ad, 2 dg_n m^2 + dg_n^2 m = 64 GFLOP in 1.6 ms; Y = W Vd of a pure block at the rate of the hybrid
        // term below (a hybrid block pays it there); four launches and the scatters
        const double ns = b.dg_n;
        t += 2.0 * ns * m * Rx / (1.28e11 / 2.8e-3) + (2.0 * ns * m * m + ns * ns * m) / (6.4e10 / 1.6e-3) + 40e-6;
        if (!b.hybrid()) t += 2.0 * Rx * m * m / 3.4e13;
        else t += (double)b.nd * 2.0 * m * m * m / 3.4e13 + 2.0 * (double)b.npos_nz * m * ns / 3.4e13;      // t_s of the dense slots, T Ad
      }
      if (!b.hybrid()) continue;
      // hybrid: Y = W Vd once more when G exists, the cross terms -- nnz(A_s) R multiply-adds per stored constraint at the
      // pair rate below, one product A_s Y per dense slot -- and H_SS over the stored positions by the mode-0 terms
      t += 2.0 * Rx * m * m / 3.4e13 + (double)b.nent * Rx * 4.0e-12 + nd * 2.0 * Rx * m * m / 3.4e13;
    }
    if (b.nd > 0) t += (4.0 / 3.0 * nd * m * m * m + 0.5 * nd * nd * m * m + nd * (n - nd) * m * m * 0.5) / 6.0e13;
    double s1 = 0.0, s2 = 0.0;       // sum over sparse pairs of nnz_i nnz_j = ((sum nnz)^2 + sum nnz^2) / 2
    for (int p = b.nd; p < b.npos_nz; ++p) { s1 += (double)b.nnz[p]; s2 += (double)b.nnz[p] * (double)b.nnz[p]; }
    const double ns = b.npos_nz - b.nd;
    t += std::max(0.5 * (s1 * s1 + s2) * 4.0e-12, 0.5 * ns * (ns + 1.0) * 5.0e-11);      // C5: 2e8 pairs of 9 x 9 in 66 ms
  }
  return t;
}

static bool any_factored(const lrn_ctx* c) {
  for (const auto& b : c->lmi)
    if (b.factored) return true;
  return false;
}

// The mode hop_prepare assembles H in: 1 (from the factors) when every LMI block is covered and the option allows it --
// always under cg_lowrank = 1, where it is estimated cheaper under -1 --, else 0.  And 1 whenever a block is factored
// (option "cg_factored"): mode 0 refuses such a block, mode 1 handles every block kind, the cross terms of a hybrid one included
static int hop_mode(const lrn_ctx* c) {
  if (cg_factored_on(c) && any_factored(c)) return 1;
  if (!cg_lowrank_on(c) || c->lmi.empty()) return 0;
  for (const auto& b : c->lmi)
    if (!cg_lowrank_covered(b)) return 0;
  if (c->opt.cg_lowrank == 1) return 1;
  return est_assemble_s(c, 1) < est_assemble_s(c, 0) ? 1 : 0;
}

static double est_symv_s(const lrn_ctx* c) {
  const double n = c->nvar;
  return n * n * 4.0 / 4.5e12 + 12e-6;
}

// Bytes H may take (option "hop_max_mb"): the option in MiB; -1 = no limit for a model without a factored block (the
// behaviour before the option existed), and for one with a factored block the free device memory plus what H and the
// mode-1 workspaces already hold (they are reused), minus the mode-1 workspace: U (and Y, Q of a hybrid block), msz x R each
static double hop_budget_bytes(const lrn_ctx* c) {
  if (c->opt.hop_max_mb >= 0.0) return c->opt.hop_max_mb * 1048576.0;
  if (!(cg_factored_on(c) && any_factored(c))) return 1e300;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return 1e300;
  double need = 0.0;
  for (const auto& b : c->lmi) {
    const double mr = (double)b.msz * (double)c->nvar * b.lr_khat * 8.0;
    double w = mr * (b.hybrid() ? (b.nd > 0 ? 3.0 : 2.0) : 1.0);
    if (b.factored && b.dg_n > 0) {
      // the mode-1 workspace of assemble_diag (option "cg_diag"): Y of a pure block too, P (dg_n x msz), H_DD (dg_n^2), C (dg_n x
      // nvar), and T, T' Ad of the stored rows
      const double ns = b.dg_n, nst = b.npos_nz;
      if (!b.hybrid()) w += mr;
      w += (ns * b.msz + ns * ns + ns * c->nvar + nst * b.msz + nst * ns) * 8.0;
    }
    need = std::max(need, w);
  }
  double held = (double)c->H.bytes + (double)c->BG.bytes + (double)c->facY.bytes + (double)c->P.bytes;
  for (const auto& b : c->lmi)
    if (b.factored && b.dg_n > 0) {      // (a model without diagonal rows does not reuse these: its budget stays what it was)
      held += (double)c->dgP.bytes + (double)c->dgC.bytes + (double)c->dgH.bytes + (double)c->dgT.bytes + (double)c->dgTA.bytes;
      break;
    }
  return (double)fr + held - need;
}

// Decide, once per NT scaling, whether lrn_pcg / lrn_matvec go through the assembled matrix.  expected_iters: operator
// applications the caller expects under this scaling (the CG iterations of the previous IP iteration).
bool hop_worthwhile(lrn_ctx* c, long expected_iters) {
  if (c->opt.matvec_h == 1 || c->nvar <= 0 || c->nlmi < 1) return false;
  if (c->world > 1 && (!c->comm || !hop_shardable(c))) return false;      // (lrn_set_shard alone: the caller exchanges H itself)
  for (const auto& b : c->lmi)
    if (!b.have_W) return false;
  // option "hop_max_mb": H above the budget is not assembled, whatever else says so -- factored models reach nvar where
  // nvar^2 doubles do not fit, and an automatic choice must not end in an allocation error
  const double hbytes = (double)c->nvar * (double)c->nvar * 8.0;
  if (hbytes > hop_budget_bytes(c)) {
    c->counts["hop_over_budget"] += 1;
    return false;
  }
  if (c->opt.matvec_h == 2) return true;
  const double gain = (double)expected_iters * (est_operator_s(c) - est_symv_s(c));
  return gain > 1.2 * est_assemble_s(c, hop_mode(c));
}

// Make c->H the Schur matrix of the current scaling (general mode: the map MyA applies).  One process per GPU: every
// rank enters the status reduction; column blocks are NOT exchanged (each rank multiplies the columns it assembled),
// partial sums of the factor path are all-reduced as in lrn_schur_assemble.
int hop_prepare(lrn_ctx* c) {
  const int mode = hop_mode(c);      // (a matrix assembled in the other mode is the same map but not the same bits: not reused)
  if (c->have_H && !c->H_shifted && !c->H_partial && c->H_version == c->scal_version && c->H_mode == mode) return LRN_OK;
  const bool sharded = c->comm && c->world > 1;
  int rc;
  if (sharded) {
    LRN_TRY(comm_agree_plan(c, 0));
    rc = schur_assemble(c, 0);
    rc = comm_schur_exchange(c, rc, /*gather_blocks=*/false);
  } else {
    rc = schur_assemble(c, mode);
  }
  if (rc == LRN_OK) c->counts["hop_assemble"] += 1;
  if (rc == LRN_OK && mode == 1) c->counts["hop_assemble_lowrank"] += 1;
  return rc;
}

}  // namespace lrn
