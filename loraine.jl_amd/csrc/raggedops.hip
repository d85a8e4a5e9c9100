// Rank-class route of the rank-k Schur assembly (option "lowrank_ragged", schur_factored.hip::assemble_lowrank), and below it
// mat(AA' x) in factor form on the same compacted columns (option "ragged_ops", dataops.hip).  What else runs on the compacted
// columns -- AA vec(Z), the cross terms of a hybrid block, ts of H_alpha -- is the padded code on another column layout
// (fac_cols.h) and lives beside it.
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
// of a tile are uniform and none straddles a tile or a 16 x 16 accumulator block.  The product is the tile of mfma_tile.h over
// K = msz (lane maps, LDS banks and the K loop are derived there); both operands are K-contiguous columns, two [row][k] panels:
//   As[i][k] = A[k0 + k, r0 + i]   Bs[j][k] = B[k0 + k, c0 + j]    2 x 9 216 = 18 432 bytes of LDS
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
#include "mfma_tile.h"
#include "ops.h"
#include "ragged_plan.h"

namespace lrn {

static_assert(RG_TILE == MT_T && RG_KSTEP == MT_K, "the plan's tiles and K chunks are those of mfma_tile.h");

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
__device__ __forceinline__ void ragged_wide_epilogue(const RaggedTile& tl, const v4f64 (&acc)[2][2], const double* __restrict__ wc,
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
  __shared__ double As[MtRowK::SIZE];
  __shared__ double Bs[MtRowK::SIZE];
  const RaggedTile tl = tiles[blockIdx.x];
  const MtLane ln = mt_lane();
  const int wr = ln.wr, wn = ln.wc, ci = ln.ci, kq = ln.kq;
  v4f64 acc[2][2];
  double areg[4], breg[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int k = k0 + MtRowK::sk(ln.t, ps);
      const int i = tl.r0 + MtRowK::srow(ln.t, ps), j = tl.c0 + MtRowK::srow(ln.t, ps);
      areg[ps] = (k < m && i < tl.r1) ? A[(long)k + (long)i * m] : 0.0;
      breg[ps] = (k < m && j < tl.c1) ? B[(long)k + (long)j * m] : 0.0;
    }
  };
  auto stage = [&](int ps, double* a, double* b) { *a = areg[ps]; *b = breg[ps]; };
  mt_kloop<MtRowK, MtRowK>(ln, As, Bs, 0, m, fetch, stage, acc);
  const int ka = tl.ka, kb = tl.kb;
  if (ka > 16 || kb > 16) {                          // a tile of a wide block (uniform over the workgroup): see below
    ragged_wide_epilogue(tl, acc, wc, gh, H, ldh, As, 2 * wr + wn, ln.lane);
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
  LRN_TRY(cols_product(c, fromW ? b.W.as<double>() : b.G.as<double>(), !fromW, b.Vc.as<double>(), Rc, m, U));      // U_c = G' Vc (or W Vc)
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

// ================================================================ mat(AA' x) on the compacted columns
// Option "ragged_ops" (dataops.hip::aat_to_mat_factored decides): the factor form of mat(AA' x) of a block of mixed ranks on Vc
// (msz x Rc) instead of Vd (msz x nvar khat), with the plan the assembly above uses.
//     mat(AA' x)    = -sum_c s_c f_c f_c',  s_c = wc_c x[nat(gh[cg[c]])],  F = Vc or Yc = W Vc (option "fac_op_scaled")
// The padded code scales a copy of the factors and runs a lower-triangle product: a different route, which is why this operator
// has a kernel of its own here while AA vec(Z) is dataops.hip::aa_times_factored on either layout.  A constraint of rank 0 has
// no group and contributes nothing.  Every sum has a fixed order and one writer: no atomics.
//
// ragged_syrk_kernel: 256 threads, grid = lower tiles x K-chunks.  Workgroup (t, s): the 64 x 64 tile (ti, tj), ti >= tj, of M
// over the columns of chunk s (ragged_plan.h::ragged_chunk_cols), in steps of 16 columns, the tail zero-filled: the tile of
// mfma_tile.h (lane maps, LDS banks and the order of a K step are derived there) with both panels [k][row], coalesced along the
// rows of F -- WRITTEN OUT here: over mt_kloop its aat_to_mat times came out 0.4 to 1.0 % above the parent's in most figures
// of tools/ragged_ops_times.py, both runs of both sides (profiles/mfma_tile_refactor_ab.txt); as written its code object is
// the one it had.  A change to the loop in mfma_tile.h is to be made here too.
//   Ps[k][i] = s_c F[i0 + i, c]   Qs[k][j] = F[j0 + j, c]   c = chunk start + k0 + k      2 x 10 240 = 20 480 bytes of LDS
// s_c is computed while staging (thread (i = t & 63, k = t >> 6 + 4 pass): k, hence c and s_c, are wave-uniform) -- no scaled
// copy of the factors is written or read back.  Wave w owns the 32 x 32 block (w >> 1, w & 1) with the j side as the A operand
// and the i side as the B operand: D[row = j][col = i], so the 16 lanes of a quarter hold 16 consecutive i of one column j of
// M -- 128-byte stores.  Both fragment reads are conflict-free by the derivation of mfma_tile.h -- derived, not measured.
// The tile goes to slab s of c->slabs (ks > 1) or straight to M (ks = 1; the part of a diagonal tile
// above the diagonal is written too and overwritten by the mirror).
// ragged_syrk_reduce_kernel: adds the slabs in the order 0 .. ks - 1 for i >= j and writes M[i, j] and M[j, i] from the one
// sum, by 32 x 32 tile pairs through LDS as mirror_lower_tiled_kernel does: M is exactly symmetric, two calls give equal bits.
__global__ __launch_bounds__(256) void ragged_syrk_kernel(const double* __restrict__ F, int m, long Rc,
                                                          const double* __restrict__ wc, const int* __restrict__ cg,
                                                          const int* __restrict__ gh, const int* __restrict__ sigma,
                                                          const double* __restrict__ x, int ks, double* __restrict__ out,
                                                          long slab_stride) {
  constexpr int LD = MtKRow::LD;
  __shared__ double Ps[MtKRow::SIZE];
  __shared__ double Qs[MtKRow::SIZE];
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
  v4f64 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};
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
      Ps[(zk + 4 * ps) * LD + zi] = preg[ps];
      Qs[(zk + 4 * ps) * LD + zi] = qreg[ps];
    }
    __syncthreads();
    if (cb + k0 + RG_KSTEP < ce) fetch(k0 + RG_KSTEP);
#pragma unroll
    for (int kk = 0; kk < RG_KSTEP / 4; ++kk) {
      const int k = 4 * kk + kq;
      const double a0 = Qs[k * LD + 32 * wn + ci];
      const double a1 = Qs[k * LD + 32 * wn + 16 + ci];
      const double b0 = Ps[k * LD + 32 * wr + ci];
      const double b1 = Ps[k * LD + 32 * wr + 16 + ci];
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

}  // namespace lrn
