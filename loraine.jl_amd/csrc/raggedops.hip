// Rank-class route of the rank-k Schur assembly (option "lowrank_ragged", schur_factored.hip::assemble_lowrank).
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
  // ---- epilogue: ka x kb blocks inside the 16 x 16 accumulator blocks (ka, kb | 16; uniform over the workgroup)
  const int ka = tl.ka, kb = tl.kb;
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

// the plan of the block and its device copies, Vc among them: once per lrn_upload_lowrank (b.rg_ready)
static int ragged_setup(lrn_ctx* c, LmiBlock& b) {
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
// conditions: one GPU, 0 < Rc < R
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
  c->BG_ragged = true;     // (BG holds U_c, not Y = W Vd: factored_y forms its own product)
  c->counts["schur_ragged"] += 1;
  c->rg_last_cols = Rc;
  c->rg_last_classes = b.rg_ncls;
  c->rg_last_tiles = b.rg_ntiles;
  return LRN_OK;
}

}  // namespace lrn
