// Rank-class route of the rank-k Schur assembly (option "lowrank_ragged", schur_factored.hip::assemble_lowrank), and below it
// the two data operators in factor form on the same compacted columns (option "ragged_ops", dataops.hip), the cross terms of a
// hybrid block (option "ragged_cross") and ts of H_alpha (option "ragged_ts", cgops.hip) at the end of the file.
//
// The padded route pads every constraint of a block to khat columns, khat from the LARGEST rank, and pays msz R^2 multiply-adds
// for H_FF = blocksum(d d' o (U' V)^2), R = nvar khat.  Here the constraints are grouped by rank class (ragged_plan.h): class c_j
// = the power of two >= the rank of constraint j, classes laid out 16, 8, 4, 2, 1, a constraint of rank 0 left out.  The
// compacted factors Vc (msz x Rc, Rc = sum c_j) are built once per upload, U_c = G' Vc (or W Vc) by the product every route
// uses, and one launch of ragged_blocksum_kernel walks a host-built tile list over T = U_c' B_c (B_c = U_c with G, Vc with W
// only -- the choice of the padded route).
//
// ragged_blocksum_kernel: 256 threads, one workgroup per tile record, tile = at most 64 rows x 64 columns of T inside ONE
// class pair (rows: class A, columns: class B, A at or before B in the layout; all tiles of seg_A x seg_B for A != B, tile row
// >= tile column for A == B).  Tiles are anchored at the segment starts and every class size divides 64, so the ka x kb blocks
// of a tile are uniform and none straddles a tile or a 16 x 16 accumulator block.  K = msz is walked in steps of 16 (tail
// zero-filled).  Both operands are K-contiguous columns:
//   As[i][k] = A[k0 + k, r0 + i]   Bs[j][k] = B[k0 + k, c0 + j]    64 x 16 doubles each, row stride 18
// 2 x 9 216 = 18 432 bytes of LDS.  The global loads of the next step are issued before the MFMAs of the current one.  Wave w
// owns the 32 x 32 block (w >> 1, w & 1) as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64 (A: lane l holds A[l & 15][l >> 4],
// B: B[l >> 4][l & 15], C/D: col = l & 15, row = (l >> 4) + 4 reg).  Fragment reads are ds_read_b64 (bank = dword address mod
// 64, conflicts within a 32-lane half): a half reads rows i .. i + 15 at k and k + 1 -- 36 i mod 64 runs through the sixteen
// multiples of 4, the two dwords of an element and the two k fill the four banks of each: conflict-free (derived from the bank
// rule, as for Vs of facops.hip; not measured).  Staging writes are ds_write_b64 of 16 consecutive k per row.
// Epilogue: each accumulator element is squared and weighted by wc[row] wc[col]; the kb columns of a block are summed over
// neighbouring lanes (xor 1 .. kb / 2), the ka rows over the lane quarters (xor 16, 32) and, from ka = 8 on, over the
// registers first -- the scheme of the blocked epilogue of gemm_f64.hip with independent row and column sizes.  A butterfly
// leaves the same sum in every lane of the group; one lane adds it to H[h_lower(gh[gi], gh[gj])], += because the blocks of a
// model share H.  Rows and columns beyond the segment end carry zero operands and weight 0 and take part in the shuffles, which
// the whole wave executes.  In a diagonal tile of a class with itself the blocks with gi < gj are skipped: every unordered pair
// of constraints has exactly one writer, no atomics -- two assemblies give the same bits.
// A wide block (khat 32 or 64, option "lowrank_wide") adds the classes 64 and 32 in front of the layout and always takes this
// route.  A tile with ka or kb above 16 leaves the K loop for ragged_wide_epilogue below (a branch uniform over the workgroup):
// a class-32 block is one wave's 32 x 32 sub-tile, a class-64 block the whole tile.  A tile with ka, kb <= 16 runs the epilogue
// above, unchanged.
#include "../../include/loraine_hip.h"
#include "ctx.h"
#include "ops.h"
#include "ragged_plan.h"

namespace lrn {

typedef double rg_v4 __attribute__((ext_vector_type(4)));

static constexpr int RG_K = 16;        // K step
static constexpr int RG_LD = 18;       // row stride of As / Bs (doubles)

// Vc[:, h] = factor column src[h] of the CSR by factor column (zero-filled by the caller; padding columns stay zero)
__global__ void ragged_dense_kernel(const long* __restrict__ ptr, const int* __restrict__ col, const double* __restrict__ val,
                                    const long* __restrict__ src, int msz, double* __restrict__ Vc) {
  const long h = blockIdx.x;
  const long s = src[h];
  if (s < 0) return;
  for (long f = ptr[s] + threadIdx.x; f < ptr[s + 1]; f += blockDim.x) Vc[(long)col[f] + h * msz] = val[f];
}

// ---- epilogue of a tile of a wide block (ka or kb in {32, 64}; the other side any class size).  A class-32 block is the 32 x 32
// sub-tile of one wave, a class-64 block the whole tile.  Order of the sum, fixed:
//   1. inside each 16 x 16 accumulator the register / lane butterfly of the narrow epilogue with the sizes capped at 16;
//   2. across the wave's two accumulators in a direction of size >= 32, index 0 + index 1 -- the rows first, then the columns;
//   3. for size 64 across the two waves in that direction through LDS, wave 0 + wave 1 -- again the rows first.
// Step 3 reuses the staging buffer As after a barrier: wave w writes the sums of its (32 / min(ka, 32)) x (32 / min(kb, 32)) <= 32
// blocks to red[32 w + slot] (one lane per block), and after a second barrier the lanes of the wave that is first in every
// 64-direction read their own and the partner sums and add to H.  Both barriers sit in a branch on ka, kb alone and no lane has
// left before them: all 256 threads reach them.  LDS banks of the exchange: the writing lanes of one ds_write_b64 hold
// consecutive slots, i.e. consecutive doubles -- at most 16 of them, distinct bank pairs -- and the reads are the same
// addresses offset by a multiple of 32 doubles, one pass each: conflict-free (derived from the bank rule, not measured).
// One writer per entry of H, no atomics.
__device__ __forceinline__ void ragged_wide_epilogue(const RaggedTile& tl, const rg_v4 (&acc)[2][2], const double* __restrict__ wc,
                                                     const int* __restrict__ gh, double* __restrict__ H, int ldh,
                                                     double* __restrict__ red, int w, int lane) {
  const int ka = tl.ka, kb = tl.kb;
  const int wr = w >> 1, wn = w & 1;
  const int ci = lane & 15, kq = lane >> 4;
  const int ka16 = ka < 16 ? ka : 16, kb16 = kb < 16 ? kb : 16;
  const int rstep = ka16 > 4 ? ka16 / 4 : 1;         // registers per block inside an accumulator
  double v[2][2][4];
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) {
      const int rb = tl.r0 + 32 * wr + 16 * ib;
      const int col = tl.c0 + 32 * wn + 16 * jb + ci;
      const double wcol = col < tl.c1 ? wc[col] : 0.0;
      double s[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rb + kq + 4 * r;
        const double a = acc[ib][jb][r];
        s[r] = a * a * (row < tl.r1 ? wc[row] : 0.0) * wcol;
      }
      if (ka16 >= 8) { s[0] += s[1]; s[2] += s[3]; }
      if (ka16 >= 16) s[0] += s[2];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double x = s[r];
        if (r % rstep == 0) {                        // (uniform: the whole wave executes the shuffles)
          for (int o = 1; o < kb16; o <<= 1) x += __shfl_xor(x, o, 64);
          if (ka16 >= 2) x += __shfl_xor(x, 16, 64);
          if (ka16 >= 4) x += __shfl_xor(x, 32, 64);
        }
        v[ib][jb][r] = x;
      }
    }
  if (ka >= 32) {
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[0][jb][r] += v[1][jb][r];
  }
  if (kb >= 32) {
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[ib][0][r] += v[ib][1][r];
  }
  const int kaw = ka < 32 ? ka : 32, kbw = kb < 32 ? kb : 32;      // extent of a block inside the wave's 32 x 32
  const int ncw = 32 / kbw;
  const bool x64 = ka == 64 || kb == 64;             // (uniform over the workgroup)
  if (x64) {
    __syncthreads();                                 // every wave is done with the last K step's As
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rw = 16 * ib + kq + 4 * r, cw = 16 * jb + ci;
          if (rw % kaw == 0 && cw % kbw == 0) red[32 * w + (rw / kaw) * ncw + cw / kbw] = v[ib][jb][r];
        }
    __syncthreads();
  }
  if ((ka == 64 && wr) || (kb == 64 && wn)) return;  // (whole waves, after the barriers: the partner wave adds)
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rw = 16 * ib + kq + 4 * r, cw = 16 * jb + ci;
        if (rw % kaw || cw % kbw) continue;
        const int row = tl.r0 + 32 * wr + rw, col = tl.c0 + 32 * wn + cw;
        if (row >= tl.r1 || col >= tl.c1) continue;
        const int gi = tl.gi0 + (row - tl.r0) / ka, gj = tl.gj0 + (col - tl.c0) / kb;
        if (tl.diag && gi < gj) continue;
        double x = v[ib][jb][r];
        if (x64) {
          const int slot = (rw / kaw) * ncw + cw / kbw;
          if (ka == 64 && kb == 64) x = (red[slot] + red[64 + slot]) + (red[32 + slot] + red[96 + slot]);
          else if (ka == 64) x = red[32 * w + slot] + red[32 * (w + 2) + slot];
          else x = red[32 * w + slot] + red[32 * (w + 1) + slot];
        }
        H[h_lower(gh[gi], gh[gj], ldh)] += x;
      }
}

__global__ __launch_bounds__(256) void ragged_blocksum_kernel(const double* __restrict__ A, const double* __restrict__ B, int m,
                                                              const RaggedTile* __restrict__ tiles,
                                                              const double* __restrict__ wc, const int* __restrict__ gh,
                                                              double* __restrict__ H, int ldh) {
  __shared__ double As[RG_TILE * RG_LD];
  __shared__ double Bs[RG_TILE * RG_LD];
  const RaggedTile tl = tiles[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = w >> 1, wn = w & 1;
  const int ci = lane & 15, kq = lane >> 4;
  rg_v4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = rg_v4{0.0, 0.0, 0.0, 0.0};
  // staging map of both operands: thread (k = t & 15, column = t >> 4 + 16 pass)
  const int sk = t & 15, sc = t >> 4;
  double areg[4], breg[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int k = k0 + sk;
      const int i = tl.r0 + sc + 16 * ps, j = tl.c0 + sc + 16 * ps;
      areg[ps] = (k < m && i < tl.r1) ? A[(long)k + (long)i * m] : 0.0;
      breg[ps] = (k < m && j < tl.c1) ? B[(long)k + (long)j * m] : 0.0;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < m; k0 += RG_K) {
    __syncthreads();                       // the waves are done with the previous step's tiles
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      As[(sc + 16 * ps) * RG_LD + sk] = areg[ps];
      Bs[(sc + 16 * ps) * RG_LD + sk] = breg[ps];
    }
    __syncthreads();
    if (k0 + RG_K < m) fetch(k0 + RG_K);
#pragma unroll
    for (int ks = 0; ks < RG_K / 4; ++ks) {
      const int k = 4 * ks + kq;
      const double a0 = As[(32 * wr + ci) * RG_LD + k];
      const double a1 = As[(32 * wr + 16 + ci) * RG_LD + k];
      const double b0 = Bs[(32 * wn + ci) * RG_LD + k];
      const double b1 = Bs[(32 * wn + 16 + ci) * RG_LD + k];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  const int ka = tl.ka, kb = tl.kb;
  if (ka > 16 || kb > 16) {                          // a tile of a wide block (uniform over the workgroup): see below
    ragged_wide_epilogue(tl, acc, wc, gh, H, ldh, As, w, lane);
    return;
  }
  // ---- epilogue: ka x kb blocks inside the 16 x 16 accumulator blocks (ka, kb | 16; uniform over the workgroup)
  const int kqr = ka < 4 ? ka : 4;                   // rows of a block among the lane quarters
  const int rstep = ka > 4 ? ka / 4 : 1;             // registers per block
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) {
      const int rb = tl.r0 + 32 * wr + 16 * ib;
      const int col = tl.c0 + 32 * wn + 16 * jb + ci;
      const double wcol = col < tl.c1 ? wc[col] : 0.0;
      double s[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rb + kq + 4 * r;
        const double v = acc[ib][jb][r];
        s[r] = v * v * (row < tl.r1 ? wc[row] : 0.0) * wcol;
      }
      if (ka >= 8) { s[0] += s[1]; s[2] += s[3]; }
      if (ka >= 16) s[0] += s[2];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r % rstep) continue;
        double v = s[r];
        for (int o = 1; o < kb; o <<= 1) v += __shfl_xor(v, o, 64);
        if (ka >= 2) v += __shfl_xor(v, 16, 64);
        if (ka >= 4) v += __shfl_xor(v, 32, 64);
        const int row = rb + kq + 4 * r;
        if ((ci % kb) || (kq % kqr) || row >= tl.r1 || col >= tl.c1) continue;
        const int gi = tl.gi0 + (row - tl.r0) / ka, gj = tl.gj0 + (col - tl.c0) / kb;
        if (tl.diag && gi < gj) continue;
        H[h_lower(gh[gi], gh[gj], ldh)] += v;
      }
    }
}

// the plan of the block and its device copies, Vc among them: once per lrn_upload_lowrank (b.rg_ready), by the first assembly
// or the first data operator that takes a rank-class route
int ragged_setup(lrn_ctx* c, LmiBlock& b) {
  if (b.rg_ready) return LRN_OK;
  const int n = c->nvar, m = b.msz, kh = b.lr_khat;
  const long R = (long)n * kh;
  std::vector<double> w(R);
  LRN_HIP(c, hipMemcpy(w.data(), b.v_w.p, (size_t)R * 8, hipMemcpyDeviceToHost));
  const RaggedPlan p = plan_ragged(w.data(), n, kh);
  if (p.Rc != b.rg_Rc) return set_error(c, LRN_ERR_STATE, "rank-class plan: %ld columns, the upload counted %ld", p.Rc, b.rg_Rc);
  if (p.tiles.size() > 2147483647UL) return set_error(c, LRN_ERR_ARG, "rank-class plan: %zu tiles", p.tiles.size());
  LRN_TRY(ensure(c, b.rg_src, (size_t)p.Rc * 8));
  LRN_TRY(ensure(c, b.rg_wc, (size_t)p.Rc * 8));
  LRN_TRY(ensure(c, b.rg_gh, p.gh.size() * 4));
  LRN_TRY(ensure(c, b.rg_tiles, p.tiles.size() * sizeof(RaggedTile)));
  LRN_TRY(copy_in(c, b.rg_src.p, p.src.data(), (size_t)p.Rc * 8));
  LRN_TRY(copy_in(c, b.rg_wc.p, p.wc.data(), (size_t)p.Rc * 8));
  LRN_TRY(copy_in(c, b.rg_gh.p, p.gh.data(), p.gh.size() * 4));
  LRN_TRY(copy_in(c, b.rg_tiles.p, p.tiles.data(), p.tiles.size() * sizeof(RaggedTile)));
  LRN_TRY(ensure(c, b.rg_cg, (size_t)p.Rc * 4));
  LRN_TRY(copy_in(c, b.rg_cg.p, p.cg.data(), (size_t)p.Rc * 4));
  LRN_TRY(ensure(c, b.rg_hg, (size_t)n * 4));
  LRN_TRY(copy_in(c, b.rg_hg.p, p.hg.data(), (size_t)n * 4));
  for (int ci = 0; ci < RG_NCLS; ++ci) { b.rg_seg0[ci] = p.seg0[ci]; b.rg_grp0[ci] = p.grp0[ci]; }
  b.rg_grp0[RG_NCLS] = (int)p.gh.size();
  LRN_TRY(ensure(c, b.Vc, (size_t)m * p.Rc * 8));
  LRN_HIP(c, hipMemsetAsync(b.Vc.p, 0, (size_t)m * p.Rc * 8, c->stream));
  hipLaunchKernelGGL(ragged_dense_kernel, dim3((unsigned)p.Rc), dim3(64), 0, c->stream, b.v_ptr.as<long>(), b.v_col.as<int>(),
                     b.v_val.as<double>(), b.rg_src.as<long>(), m, b.Vc.as<double>());
  LRN_HIP(c, hipStreamSynchronize(c->stream));      // (the host vectors of the plan go out of scope)
  b.rg_ncls = p.ncls;
  b.rg_ntiles = (long)p.tiles.size();
  b.rg_ready = true;
  return LRN_OK;
}

// H_FF of one block by rank class.  The caller (assemble_lowrank) has checked the factors, the scaling and the route
// conditions: one GPU, 0 < Rc < R -- or a wide block with 0 < Rc <= R
int assemble_ragged(lrn_ctx* c, LmiBlock& b) {
  const int n = c->nvar, m = b.msz;
  const bool fromW = !b.have_G;
  LRN_TRY(ragged_setup(c, b));
  const long Rc = b.rg_Rc;
  LRN_TRY(ensure(c, c->BG, (size_t)m * Rc * 8));
  double* U = c->BG.as<double>();
  tic(c);
  {
    GemmDesc g;     // U_c = G' Vc (or W Vc), msz x Rc
    g.A = fromW ? b.W.as<double>() : b.G.as<double>();
    if (fromW) { g.sAm = 1; g.sAk = m; } else { g.sAm = m; g.sAk = 1; }
    g.B = b.Vc.as<double>(); g.sBk = 1; g.sBn = m;
    g.C = U; g.sCm = 1; g.sCn = m;
    g.M = m; g.N = (int)Rc; g.K = m;
    LRN_TRY(gemm(c->stream, g));
  }
  toc(c, "lowrank_u");     // (U_c alone; "ragged" below: U_c and the tile launch, from the same start)
  if (b.rg_ntiles > 0)
    hipLaunchKernelGGL(ragged_blocksum_kernel, dim3((unsigned)b.rg_ntiles), dim3(256), 0, c->stream, U,
                       fromW ? b.Vc.as<double>() : U, m, b.rg_tiles.as<RaggedTile>(), b.rg_wc.as<double>(), b.rg_gh.as<int>(),
                       c->H.as<double>(), n);
  toc(c, "ragged");
  c->BG_ragged = true;     // (BG holds U_c, not Y = W Vd: factored_y forms its own product -- or, under "ragged_cross" with W
                           // only, hands out this U_c = W Vc as Yc)
  c->counts["schur_ragged"] += 1;
  c->rg_last_cols = Rc;
  c->rg_last_classes = b.rg_ncls;
  c->rg_last_tiles = b.rg_ntiles;
  return LRN_OK;
}

// ================================================================ the data operators on the compacted columns
// Option "ragged_ops" (dataops.hip::aa_times_factored, aat_to_mat_factored decide): the factor form of AA vec(Z) and mat(AA' x)
// of a block of mixed ranks on Vc (msz x Rc) instead of Vd (msz x nvar khat), with the plan the assembly above uses.
//     (AA vec(Z))_j = -sum_{c in group of j} wc_c v_c' Z v_c     Q = Z Vc by the product every route uses (or the fused quadratic
//                                                               form of facops.hip on (Vc, Rc)), then sums by GROUP through gh
//     mat(AA' x)    = -sum_c s_c f_c f_c',  s_c = wc_c x[nat(gh[cg[c]])],  F = Vc or Yc = W Vc (option "fac_op_scaled")
// A constraint of rank 0 has no group and receives nothing.  Every sum has a fixed order and one writer: no atomics.
//
// ragged_syrk_kernel: 256 threads, grid = lower tiles x K-chunks.  Workgroup (t, s): the 64 x 64 tile (ti, tj), ti >= tj, of M
// over the columns of chunk s (ragged_plan.h::ragged_chunk_cols), in steps of 16 columns, the tail zero-filled.  Both panels
// are staged as [k][i], coalesced along the rows of F:
//   Ps[k][i] = s_c F[i0 + i, c]   Qs[k][j] = F[j0 + j, c]   c = chunk start + k0 + k      16 x 64 doubles each, row stride 80
// 2 x 10 240 = 20 480 bytes of LDS.  s_c is computed while staging (thread (i = t & 63, k = t >> 6 + 4 pass): k, hence c and
// s_c, are wave-uniform) -- no scaled copy of the factors is written or read back.  The global loads of the next step are
// issued before the MFMAs of the current one.  Wave w owns the 32 x 32 block (w >> 1, w & 1) as 2 x 2 accumulators of
// v_mfma_f64_16x16x4_f64 with the j side as the A operand and the i side as the B operand: D[row = j][col = i], so the 16
// lanes of a quarter hold 16 consecutive i of one column j of M -- 128-byte stores.  Both fragment reads are the A read of
// fac_quadform_kernel's Zs (rows k, k + 1, sixteen consecutive i, row stride 80): conflict-free by the derivation there --
// derived, not measured.  The tile goes to slab s of c->slabs (ks > 1) or straight to M (ks = 1; the part of a diagonal tile
// above the diagonal is written too and overwritten by the mirror).
// ragged_syrk_reduce_kernel: adds the slabs in the order 0 .. ks - 1 for i >= j and writes M[i, j] and M[j, i] from the one
// sum, by 32 x 32 tile pairs through LDS as mirror_lower_tiled_kernel does: M is exactly symmetric, two calls give equal bits.
struct RaggedSegs { long seg0[RG_NCLS]; int grp0[RG_NCLS + 1]; };

// first column and class size of group g (g < grp0[RG_NCLS])
__device__ __forceinline__ long ragged_group_col(const RaggedSegs& sg, int g, int* cj) {
  int ci = 0;
  while (ci < RG_NCLS - 1 && g >= sg.grp0[ci + 1]) ++ci;
  *cj = ragged_class_size(ci);
  return sg.seg0[ci] + (long)(g - sg.grp0[ci]) * ragged_class_size(ci);
}

// out[nat(gh[g])] -= sum_{p < c_j} wc[col] <Q(:, col), Vc(:, col)>, col = first column of group g + p: one wave per group,
// the rows by the four accumulators and the one shuffle tree of fac_coldot_kernel
__global__ __launch_bounds__(256) void ragged_coldot_kernel(const double* __restrict__ Q, const double* __restrict__ Vc,
                                                            const double* __restrict__ wc, int m, RaggedSegs sg,
                                                            const int* __restrict__ gh, const int* __restrict__ sigma,
                                                            double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= sg.grp0[RG_NCLS]) return;
  int cj;
  const long c0 = ragged_group_col(sg, g, &cj);
  double s = 0.0;
  for (int p = 0; p < cj; ++p) {
    const long col = c0 + p;
    const double wp = wc[col];
    if (wp == 0.0) continue;                       // padding column (wave-uniform)
    const double* __restrict__ q = Q + col * m;
    const double* __restrict__ v = Vc + col * m;
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
  const int h = gh[g];
  out[sigma ? sigma[h] : h] -= s;
}

// the same sums from the partial sums of fac_quadform_kernel on (Vc, Rc): strips in order, then the columns of the group
// (one thread per group; fixed order)
__global__ __launch_bounds__(256) void ragged_quadform_reduce_kernel(const double* __restrict__ part, int nstrip, long Rc,
                                                                     const double* __restrict__ wc, RaggedSegs sg,
                                                                     const int* __restrict__ gh, const int* __restrict__ sigma,
                                                                     double* __restrict__ out) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= sg.grp0[RG_NCLS]) return;
  int cj;
  const long c0 = ragged_group_col(sg, g, &cj);
  double s = 0.0;
  for (int p = 0; p < cj; ++p) {
    const long col = c0 + p;
    const double wp = wc[col];
    if (wp == 0.0) continue;                       // padding column
    double q = 0.0;
    for (int st = 0; st < nstrip; ++st) q += part[(long)st * Rc + col];
    s += wp * q;
  }
  const int h = gh[g];
  out[sigma ? sigma[h] : h] -= s;
}

static constexpr int RS_LD = 80;       // row stride of Ps / Qs (doubles)

__global__ __launch_bounds__(256) void ragged_syrk_kernel(const double* __restrict__ F, int m, long Rc,
                                                          const double* __restrict__ wc, const int* __restrict__ cg,
                                                          const int* __restrict__ gh, const int* __restrict__ sigma,
                                                          const double* __restrict__ x, int ks, double* __restrict__ out,
                                                          long slab_stride) {
  __shared__ double Ps[RG_KSTEP * RS_LD];
  __shared__ double Qs[RG_KSTEP * RS_LD];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = w >> 1, wn = w & 1;
  const int ci = lane & 15, kq = lane >> 4;
  // lower tile (ti, tj) of the workgroup: blockIdx.x = ti (ti + 1) / 2 + tj
  const long tl = blockIdx.x;
  long ti = (long)((sqrt(8.0 * (double)tl + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > tl) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= tl) ++ti;
  const int tj = (int)(tl - ti * (ti + 1) / 2);
  const int i0 = (int)ti * RG_TILE, j0 = tj * RG_TILE;
  long cb, ce;
  ragged_chunk_cols(Rc, ks, blockIdx.y, &cb, &ce);
  rg_v4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = rg_v4{0.0, 0.0, 0.0, 0.0};
  // staging map of both panels: thread (row = t & 63, k = t >> 6 + 4 pass)
  const int zi = t & 63, zk = t >> 6;
  const bool iok = i0 + zi < m, jok = j0 + zi < m;
  double preg[4], qreg[4];
  auto fetch = [&](long k0) {
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const long col = cb + k0 + zk + 4 * ps;
      double sc = 0.0, fi = 0.0, fj = 0.0;
      if (col < ce) {
        const int h = gh[cg[col]];
        sc = -(wc[col] * x[sigma ? sigma[h] : h]);
        if (iok) fi = F[(long)(i0 + zi) + col * m];
        if (jok) fj = F[(long)(j0 + zi) + col * m];
      }
      preg[ps] = sc * fi;
      qreg[ps] = fj;
    }
  };
  fetch(0);
  for (long k0 = 0; cb + k0 < ce; k0 += RG_KSTEP) {
    __syncthreads();                       // the waves are done with the previous step's panels
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      Ps[(zk + 4 * ps) * RS_LD + zi] = preg[ps];
      Qs[(zk + 4 * ps) * RS_LD + zi] = qreg[ps];
    }
    __syncthreads();
    if (cb + k0 + RG_KSTEP < ce) fetch(k0 + RG_KSTEP);
#pragma unroll
    for (int kk = 0; kk < RG_KSTEP / 4; ++kk) {
      const int k = 4 * kk + kq;
      const double a0 = Qs[k * RS_LD + 32 * wn + ci];
      const double a1 = Qs[k * RS_LD + 32 * wn + 16 + ci];
      const double b0 = Ps[k * RS_LD + 32 * wr + ci];
      const double b1 = Ps[k * RS_LD + 32 * wr + 16 + ci];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // acc[jb][ib][r] = M[i0 + 32 wr + 16 ib + ci, j0 + 32 wn + 16 jb + kq + 4 r]
  double* __restrict__ C = out + (long)blockIdx.y * slab_stride;
#pragma unroll
  for (int jb = 0; jb < 2; ++jb)
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) {
      const int i = i0 + 32 * wr + 16 * ib + ci;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + 32 * wn + 16 * jb + kq + 4 * r;
        if (i < m && j < m) C[(long)i + (long)j * m] = acc[jb][ib][r];
      }
    }
}

__global__ void ragged_syrk_reduce_kernel(const double* __restrict__ slabs, long stride, int ks, double* __restrict__ M, int n) {
  __shared__ double tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;      // source tile rows bx.., columns by.. (on or below the diagonal)
  if (bx < by) return;
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int i = bx + threadIdx.x, j = by + r;
    double v = 0.0;
    if (i < n && j < n && i >= j) {
      const long e = (long)i + (long)j * n;
      for (int s = 0; s < ks; ++s) v += slabs[(long)s * stride + e];
      M[e] = v;
    }
    tile[r][threadIdx.x] = v;
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int i = by + threadIdx.x, j = bx + r;              // destination (i, j) = transposed position
    if (i < n && j < n && i < j) M[(long)i + (long)j * n] = tile[threadIdx.x][r];
  }
}

static RaggedSegs ragged_segs(const LmiBlock& b) {
  RaggedSegs sg;
  for (int ci = 0; ci < RG_NCLS; ++ci) sg.seg0[ci] = b.rg_seg0[ci];
  for (int ci = 0; ci <= RG_NCLS; ++ci) sg.grp0[ci] = b.rg_grp0[ci];
  return sg;
}

// Yc = W Vc (msz x Rc) of the current scaling: what fac_scaled_y is on the padded layout
int ragged_scaled_y(lrn_ctx* c, LmiBlock& b) {
  LRN_TRY(ragged_setup(c, b));
  if (b.Yc_version == c->scal_version && b.Yc.p) return LRN_OK;
  const int m = b.msz;
  LRN_TRY(ensure(c, b.Yc, (size_t)m * b.rg_Rc * 8));
  GemmDesc g;
  g.A = b.W.as<double>(); g.sAm = 1; g.sAk = m;
  g.B = b.Vc.as<double>(); g.sBk = 1; g.sBn = m;
  g.C = b.Yc.as<double>(); g.sCm = 1; g.sCn = m;
  g.M = m; g.N = (int)b.rg_Rc; g.K = m;
  LRN_TRY(gemm(c->stream, g));
  b.Yc_version = c->scal_version;
  return LRN_OK;
}

// y += the factor part of AA vec(Z).  The caller has checked the factors and the route (ragged_ops_on)
int aa_times_ragged(lrn_ctx* c, LmiBlock& b, const double* Z, double* y, bool fused) {
  const int m = b.msz;
  LRN_TRY(ragged_setup(c, b));
  const long Rc = b.rg_Rc;
  const RaggedSegs sg = ragged_segs(b);
  const int ngrp = sg.grp0[RG_NCLS];
  const int* sigma = c->pos_space ? b.sigma_d.as<int>() : (const int*)nullptr;
  if (fused) {
    double* part = nullptr;
    int nstrip = 0;
    LRN_TRY(fac_quadform_parts(c, Z, b.Vc.as<double>(), m, Rc, &part, &nstrip));
    hipLaunchKernelGGL(ragged_quadform_reduce_kernel, dim3((ngrp + 255) / 256), dim3(256), 0, c->stream, part, nstrip, Rc,
                       b.rg_wc.as<double>(), sg, b.rg_gh.as<int>(), sigma, y);
    c->counts["op_quadform_fused"] += 1;
  } else {
    LRN_TRY(ensure(c, c->BG, (size_t)m * Rc * 8));
    double* Q = c->BG.as<double>();
    GemmDesc g;     // Q = Z Vc, msz x Rc
    g.A = Z; g.sAm = 1; g.sAk = m;
    g.B = b.Vc.as<double>(); g.sBk = 1; g.sBn = m;
    g.C = Q; g.sCm = 1; g.sCn = m;
    g.M = m; g.N = (int)Rc; g.K = m;
    LRN_TRY(gemm(c->stream, g));
    hipLaunchKernelGGL(ragged_coldot_kernel, dim3((ngrp + 3) / 4), dim3(256), 0, c->stream, Q, b.Vc.as<double>(),
                       b.rg_wc.as<double>(), m, sg, b.rg_gh.as<int>(), sigma, y);
  }
  c->counts["op_factored"] += 1;
  c->counts["op_ragged"] += 1;
  return LRN_OK;
}

// K-chunks of the syrk when the option leaves them open: the smallest ks for which tiles x ks fills the chip FOUR times over at
// the kernel's compiled occupancy (workgroups per CU x CUs, asked of the runtime once), a chunk kept to at least 16 K-steps
// (256 columns).  The first rule -- fill the chip once, ks = 2 at msz 2000 -- had no measurement behind it; the sweep of
// tools/ragged_ops_times.py at msz 2000 / nvar 4000 found ks = 8 the fastest or within 4 % of it at
// Rc = 4015, 6000 and 42 372, which is this rule there.  One matrix side only: a starting point elsewhere
static int ragged_auto_chunks(long tiles, long Rc) {
  static long slots = 0;
  if (slots == 0) {
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, ragged_syrk_kernel, 256, 0) != hipSuccess || cus <= 0 || per <= 0)
      slots = 256;
    else
      slots = (long)cus * per;
  }
  const long want = (4 * slots + tiles - 1) / tiles, cap = ragged_steps(Rc) / 16;
  return (int)std::max<long>(1, std::min(want, cap));
}

// M = -sum_c s_c f_c f_c', F = Vc (null) or Yc.  *ks_out = 1: the lower tiles are in M and the caller mirrors them
// (mirror_lower_tiled_kernel of dataops.hip); > 1: M is complete
int aat_to_mat_ragged(lrn_ctx* c, LmiBlock& b, const double* x, double* M, const double* F, int* ks_out) {
  const int m = b.msz;
  LRN_TRY(ragged_setup(c, b));
  const long Rc = b.rg_Rc, mm = (long)m * m;
  if (!F) F = b.Vc.as<double>();
  const long tm = (m + RG_TILE - 1) / RG_TILE, tiles = tm * (tm + 1) / 2;
  if (tiles > 2147483647L) return set_error(c, LRN_ERR_ARG, "ragged_ops: %ld tiles", tiles);
  const int ks = ragged_clamp_chunks(Rc, c->opt.ragged_ops_split > 0 ? c->opt.ragged_ops_split : ragged_auto_chunks(tiles, Rc));
  double* out = M;
  if (ks > 1) {
    LRN_TRY(ensure(c, c->slabs, (size_t)ks * mm * 8));
    out = c->slabs.as<double>();
  }
  hipLaunchKernelGGL(ragged_syrk_kernel, dim3((unsigned)tiles, (unsigned)ks), dim3(256), 0, c->stream, F, m, Rc,
                     b.rg_wc.as<double>(), b.rg_cg.as<int>(), b.rg_gh.as<int>(),
                     c->pos_space ? b.sigma_d.as<int>() : (const int*)nullptr, x, ks, out, mm);
  if (ks > 1)
    hipLaunchKernelGGL(ragged_syrk_reduce_kernel, dim3((m + 31) / 32, (m + 31) / 32), dim3(32, 8), 0, c->stream,
                       c->slabs.as<double>(), mm, ks, M, m);
  *ks_out = ks;
  c->rg_last_chunks = ks;
  c->counts["op_factored"] += 1;
  c->counts["op_ragged"] += 1;
  return LRN_OK;
}

// ================================================================ cross terms of a hybrid block on the compacted columns
// Option "ragged_cross" (schur_factored.hip::factored_y, assemble_cross decide): H_sj = sum_c wc_c y_c' A_s y_c over the columns
// c of the GROUP of the factored constraint j, y_c the columns of Yc = W Vc (msz x Rc).  A constraint of rank 0 has no group and
// receives nothing (the padded kernel adds + 0 to its entries).
//
// ragged_cross_kernel: fac_cross_kernel of schur_factored.hip with grid.x over the groups instead of the factored positions --
// hj = gh[g], the columns group start .. + class size, weight-0 padding skipped (uniform over the workgroup).  Everything else
// is that kernel's: workgroup (g, y) takes the 32 sparse-tier stored positions s_lo + 32 y .., wave v the positions + 4 t + v,
// t < 8, in eight register sums; a column of Yc is staged in LDS (msz x 8 bytes, dynamic) or read from global memory by the
// same code; lanes stride the entry list of A_s, one shuffle tree in a fixed order, the sum weighted and added over the
// columns in order; lane 0 adds the eight sums to H, one writer per entry, no atomics.  LDS accesses: the staging writes are
// ds_write_b64 of consecutive doubles (lane l -> dwords 2 l, 2 l + 1 of a 256-dword run: conflict-free); the gather reads
// ycol[r], ycol[cc] follow the entry list of A_s, their banks are data-dependent -- an entry list sorted by column reads one
// address for cc (a broadcast) and scattered rows for r, anything from free to a multi-way conflict.  Derived, not measured.
template <bool LDS>
__global__ __launch_bounds__(256) void ragged_cross_kernel(const long* __restrict__ ptr, const int* __restrict__ er,
                                                           const int* __restrict__ ec, const double* __restrict__ ev,
                                                           const double* __restrict__ Yc, const double* __restrict__ wc, int m,
                                                           RaggedSegs sg, int s_lo, int s_hi, const int* __restrict__ gh,
                                                           const int* __restrict__ hidx, double* __restrict__ H, int ldh) {
  extern __shared__ double rg_ycol[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x;
  if (g >= sg.grp0[RG_NCLS]) return;             // (whole workgroup)
  int cj;
  const long c0 = ragged_group_col(sg, g, &cj);
  const int hj = gh[g];
  const int sb = s_lo + blockIdx.y * 32 + wave;
  double acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = 0.0;
  for (int p = 0; p < cj; ++p) {
    const long col = c0 + p;
    const double wp = wc[col];
    if (wp == 0.0) continue;                     // padding column (uniform over the workgroup)
    const double* __restrict__ yg = Yc + col * m;
    if (LDS) {
      __syncthreads();                           // the waves are done with the previous column
      for (int r = threadIdx.x; r < m; r += 256) rg_ycol[r] = yg[r];
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int sp = sb + 4 * t;                 // wave-uniform
      if (sp >= s_hi) continue;
      double q = 0.0;
      for (long e = ptr[sp] + lane; e < ptr[sp + 1]; e += 64) {
        const int r = er[e], cc = ec[e];
        q += ev[e] * (LDS ? rg_ycol[r] * rg_ycol[cc] : yg[r] * yg[cc]);
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
    H[h_lower(hidx[sp], hj, ldh)] += acc[t];
  }
}

// dense slot s: Q = A_s Yc is one product (msz x Rc), H_sj = sum_c wc_c <Q(:, c), Yc(:, c)> one wave per group (the sums of
// fac_cross_coldot_kernel), written once.  No LDS
__global__ __launch_bounds__(256) void ragged_cross_coldot_kernel(const double* __restrict__ Q, const double* __restrict__ Yc,
                                                                  const double* __restrict__ wc, int m, RaggedSegs sg, int s,
                                                                  const int* __restrict__ gh, const int* __restrict__ hidx,
                                                                  double* __restrict__ H, int ldh) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= sg.grp0[RG_NCLS]) return;             // (whole wave)
  int cj;
  const long c0 = ragged_group_col(sg, g, &cj);
  double acc = 0.0;
  for (int p = 0; p < cj; ++p) {
    const long col = c0 + p;
    const double wp = wc[col];
    if (wp == 0.0) continue;
    const double* __restrict__ q = Q + col * m;
    const double* __restrict__ y = Yc + col * m;
    double t = 0.0;
    for (int r = lane; r < m; r += 64) t += q[r] * y[r];
    acc += wp * t;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane != 0) return;
  H[h_lower(hidx[s], gh[g], ldh)] += acc;
}

// the caller (assemble_cross) has checked the route (ragged_cross_on) and that factored positions exist; Yc from factored_y
int assemble_cross_ragged(lrn_ctx* c, LmiBlock& b, const double* Yc) {
  const int n = c->nvar, m = b.msz;
  if (!Yc) return set_error(c, LRN_ERR_STATE, "ragged_cross: Yc = W Vc was not formed");
  LRN_TRY(ragged_setup(c, b));
  const long Rc = b.rg_Rc;
  const RaggedSegs sg = ragged_segs(b);
  const int ngrp = sg.grp0[RG_NCLS];
  if (ngrp <= 0) return LRN_OK;
  tic(c);
  if (b.npos_nz > b.nd) {
    const size_t cap = c->opt.fac_cross_lds == 1 ? 65536 : 32768;      // the rule of assemble_cross
    const bool lds = c->opt.fac_cross_lds != 0 && (size_t)m * 8 <= cap;
    const dim3 grid((unsigned)ngrp, (unsigned)((b.npos_nz - b.nd + 31) / 32));
#define LRN_RCROSS_LAUNCH(L, SH)                                                                                          \
  hipLaunchKernelGGL(ragged_cross_kernel<L>, grid, dim3(256), SH, c->stream, b.ent_ptr.as<long>(), b.ent_r.as<int>(),    \
                     b.ent_c.as<int>(), b.ent_v.as<double>(), Yc, b.rg_wc.as<double>(), m, sg, b.nd, b.npos_nz,           \
                     b.rg_gh.as<int>(), b.hidx.as<int>(), c->H.as<double>(), n)
    if (lds) LRN_RCROSS_LAUNCH(true, (size_t)m * 8);
    else LRN_RCROSS_LAUNCH(false, 0);
#undef LRN_RCROSS_LAUNCH
    c->counts[lds ? "hybrid_cross_lds" : "hybrid_cross_global"] += 1;
  }
  if (b.nd > 0) {
    LRN_TRY(ensure(c, c->P, (size_t)m * Rc * 8));
    double* Q = c->P.as<double>();
    for (int s = 0; s < b.nd; ++s) {
      GemmDesc g;     // Q = A_s Yc
      g.A = b.Adense.as<double>() + (long)s * m * m; g.sAm = 1; g.sAk = m;
      g.B = Yc; g.sBk = 1; g.sBn = m;
      g.C = Q; g.sCm = 1; g.sCn = m;
      g.M = m; g.N = (int)Rc; g.K = m;
      LRN_TRY(gemm(c->stream, g));
      hipLaunchKernelGGL(ragged_cross_coldot_kernel, dim3((ngrp + 3) / 4), dim3(256), 0, c->stream, Q, Yc, b.rg_wc.as<double>(),
                         m, sg, s, b.rg_gh.as<int>(), b.hidx.as<int>(), c->H.as<double>(), n);
    }
    c->counts["hybrid_cross_dense"] += 1;
  }
  toc(c, "hybrid_cross");
  return LRN_OK;
}

// ================================================================ ts of H_alpha on the compacted columns
// Option "ragged_ts" (cgops.hip::prec_setup decides): with Pc = L' Vc (msz x Rc) and Tc = Vc' Um (Rc x erank),
//     ts[j, col0 + a m + r] = -(1 / sqrt(d_j)) sum_{c in group of j} wc_c Tc[c, a] Pc[r, c]
// -- the sum fac_ts_kernel of cgops.hip forms over the khat padded columns of constraint j, over the class-size columns of its
// group instead, in the same order (the weighted columns keep their order in a group), padding skipped.
//
// ragged_ts_kernel keeps that kernel's tiling: workgroup tile = 64 natural rows j x 64 rows r of Pc, eigenvector = blockIdx.z;
// wave w takes the constraints j0 + w, j0 + w + 4, ..: h = ipos ? ipos[j] : j, g = hg[h], the columns group start .. + class
// size; its 64 lanes read 64 consecutive doubles of each column of Pc (512 B per load) with the coefficient wc_c Tc[c, a] as a
// wave-uniform scalar.  hg[h] < 0 (rank 0: a stored row, a purely diagonal row) stores 0, as do rows j >= nvar and r >= msz of
// a partial tile.  The sums go to row jl of an LDS tile of 64 x 65 doubles (33 280 bytes): ds_write_b64, lane l at dwords
// 130 jl + 2 l -- 64 consecutive doubles, conflict-free.  After the barrier lane l of wave w reads tile[l][rr], rr = w, w + 4, ..:
// dword address 130 l + 2 rr, bank (2 l + 2 rr) mod 64 -- the 32 lanes of a half take the 32 even banks and their odd
// neighbours once each: conflict-free, where a row stride of 64 doubles would put all of them on one bank pair.  Derived from
// the bank rule as for fac_ts_kernel, not measured.  The wave then writes 64 consecutive rows j of one column of ts.  Every
// element of the block's part of ts is written exactly once: no memset, no atomics, two setups give the same bits.
static constexpr int RTS_TILE = 64;
__global__ __launch_bounds__(256) void ragged_ts_kernel(const double* __restrict__ Pm, const double* __restrict__ T,
                                                        const double* __restrict__ wc, RaggedSegs sg, const int* __restrict__ hg,
                                                        const int* __restrict__ ipos, const double* __restrict__ d, int m, long Rc,
                                                        int nvar, double* __restrict__ ts) {
  __shared__ double tile[RTS_TILE][RTS_TILE + 1];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j0 = blockIdx.x * RTS_TILE, r0 = blockIdx.y * RTS_TILE, a = blockIdx.z;
  const double* __restrict__ Ta = T + (long)a * Rc;
  const int r = r0 + lane;
  for (int jl = wv; jl < RTS_TILE; jl += 4) {
    const int j = j0 + jl;
    double s = 0.0;
    if (j < nvar) {                                  // (wave-uniform)
      const int g = hg[ipos ? ipos[j] : j];
      if (g >= 0) {                                  // (rank 0: no group, the row stays zero)
        int cj;
        const long c0 = ragged_group_col(sg, g, &cj);
        for (int p = 0; p < cj; ++p) {
          const double wp = wc[c0 + p];
          if (wp == 0.0) continue;                   // padding column
          const double cf = wp * Ta[c0 + p];
          if (r < m) s += cf * Pm[(c0 + p) * m + r];
        }
      }
    }
    tile[jl][lane] = s;
  }
  __syncthreads();
  const int j = j0 + lane;
  if (j >= nvar) return;
  const double sc = -1.0 / sqrt(d[j]);
  double* __restrict__ out = ts + (long)a * m * nvar + j;
  for (int rr = wv; rr < RTS_TILE && r0 + rr < m; rr += 4) out[(long)(r0 + rr) * nvar] = sc * tile[lane][rr];
}

int ragged_ts(lrn_ctx* c, LmiBlock& b, const double* Pc, const double* Tc, const double* d, int erank, double* ts) {
  const int n = c->nvar, m = b.msz;
  LRN_TRY(ragged_setup(c, b));
  const long tx = (n + RTS_TILE - 1) / RTS_TILE, ty = (m + RTS_TILE - 1) / RTS_TILE;
  if (ty > 65535 || erank > 65535) return set_error(c, LRN_ERR_ARG, "ragged_ts: %ld row tiles, erank %d", ty, erank);
  hipLaunchKernelGGL(ragged_ts_kernel, dim3((unsigned)tx, (unsigned)ty, (unsigned)erank), dim3(256), 0, c->stream, Pc, Tc,
                     b.rg_wc.as<double>(), ragged_segs(b), b.rg_hg.as<int>(),
                     c->pos_space ? b.ipos_d.as<int>() : (const int*)nullptr, d, m, b.rg_Rc, n, ts);
  return LRN_OK;
}

}  // namespace lrn
