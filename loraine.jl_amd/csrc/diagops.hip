// Diagonal parts of a factored block (lrn_upload_diag): constraint A_k = diag(a_k) + V_k D_k V_k' for the dg_n "diagonal rows".
//
// A diagonal part needs no entry list.  With Ad = the diagonals as columns (msz x dg_n, +a as ent_v holds +A and v_w holds +d)
// and Y = W Vd (msz x R), every term it adds to the Schur matrix is a dense product with one operand squared entrywise:
//     tr(diag(a_s) W diag(a_t) W)      = a_s' (W o W) a_t                      H_DD = Ad' (W o W) Ad
//     tr(diag(a_s) W (V_j D_j V_j') W) = sum_p d_jp sum_i a_si Y[i, jp]^2      C = Ad' (Y o Y), weighted and summed over khat
//     tr(diag(a_k) W A_s W), A_s stored = a_k' t_s,  t_s = diag(W A_s W)
//     H over the factored positions    = H_FF + H_DD + C + C'                  (diagonal entries get 2 C_ss)
// and the two data operators get one term each (AA = -A):  y[nat(s)] -= sum_i a_si Z_ii,  M_ii -= sum_s x[nat(s)] a_si.
// Measured times, the crossover between the two forms below and what was not run: DESIGN section 16.
//
// diag_sq, the squared-operand product  D[s, g] = sum_{p < kh} w[g kh + p] sum_i Ad[i, s] B[i, g kh + p]^2, has two forms
// (option "diag_sq_mfma"); B = W with kh = 1 and no weights gives P of H_DD, B = Y with kh = khat and w = v_w gives C -- the
// khat block sum sits in the epilogue, nothing of size dg_n x R reaches HBM.
//   rows form (few rows): one wave per column group g, lanes stride i, eight rows' sums in registers (blockIdx.y picks the
//     eight), weight-0 columns skipped, one shuffle tree per row.  B is read once per eight rows.
//   MFMA form: the 64 x 64 tile of mfma_tile.h (256 threads, K = msz in steps of 16).  Both operands are K-contiguous in
//     memory (column s of Ad, column c of B), so both panels are [row][k]:
//       As[s][k] = Ad[k0 + k, s0 + s],  Bs[c][k] = B[k0 + k, c0 + c]^2
//     (B is squared as it is staged) -- 2 x 9 216 = 18 432 bytes of LDS, eight workgroups per CU by LDS; the compiler reports
//     92 VGPRs + 32 accumulator registers per lane, 124 of the 128 that four waves per SIMD allow (the rows form: 64, eight
//     waves).  Lane maps, LDS banks and the K loop: mfma_tile.h.
//     Epilogue: the accumulator element of column c is multiplied by w[c]; kh (a power of two <= 16) divides 16, so a column
//     group lies on kh neighbouring lanes of one accumulator block and is summed by an xor butterfly of log2 kh steps; the
//     lane with c % kh == 0 writes D[s, c / kh].  kh = 32 and 64 (a wide block, option "wide_diag"): diag_sq_wide_mfma_kernel,
//     the same product with an epilogue that goes on across the wave's two accumulators and, for 64, across two waves.
//   Option "ragged_cross" (DESIGN section 20): C from Yc = W Vc, one launch of either form per rank class, the store going
//     through a group -> H index map (hmap) -- the one change to both kernels, a null map being the code as it was.
// No atomics, fixed order in both forms: two calls give the same bits.  The forms differ from each other in rounding.
//
// The CG path (option "cg_diag"): the operators above carry the diagonal parts; ts of H_alpha gets their
// term from ts_diag_mfma_kernel at the end of this file, a sibling of the MFMA form with a scaled instead of a squared operand.
#include <algorithm>

#include "../../include/loraine_hip.h"
#include "ctx.h"
#include "mfma_tile.h"
#include "ops.h"
#include "ragged_plan.h"

namespace lrn {

static constexpr int DG_ROWS = 8;      // rows per wave of the rows form
static constexpr int DG_MFMA_MIN = 16; // auto: the MFMA form from this many diagonal rows on (measured at msz 2000 / nvar 4000 / khat 2: the rows
                                       // form is 1.8 x faster at 1 row, the MFMA form 1.3 x at 16, 3 x at 64, 13 x at 4000; 2 .. 15 rows not measured).
                                       // At kh 32 / 64 (option "wide_diag") the MFMA form measured faster at every row count: 1.4 x at 1 row,
                                       // 6 x at 16, 19 x at 64, 16 x at 4000 -- the rule was not re-tuned for them

__global__ __launch_bounds__(256) void diag_sq_rows_kernel(const double* __restrict__ Ad, int ns, const double* __restrict__ B,
                                                           long ldb, int m, int ng, int kh, const double* __restrict__ w,
                                                           double* __restrict__ D, long ldd, const int* __restrict__ hmap) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= ng) return;                             // (whole wave)
  const int s0 = blockIdx.y * DG_ROWS;
  double acc[DG_ROWS];
#pragma unroll
  for (int t = 0; t < DG_ROWS; ++t) acc[t] = 0.0;
  for (int p = 0; p < kh; ++p) {
    const long col = (long)g * kh + p;
    const double wp = w ? w[col] : 1.0;
    if (wp == 0.0) continue;                       // padding column, or a constraint without factors (wave-uniform)
    const double* __restrict__ bc = B + col * ldb;
    double q[DG_ROWS];
#pragma unroll
    for (int t = 0; t < DG_ROWS; ++t) q[t] = 0.0;
    for (int i = lane; i < m; i += 64) {
      const double bv = bc[i];
      const double b2 = bv * bv;
#pragma unroll
      for (int t = 0; t < DG_ROWS; ++t)
        if (s0 + t < ns) q[t] += Ad[(long)i + (long)(s0 + t) * m] * b2;
    }
#pragma unroll
    for (int t = 0; t < DG_ROWS; ++t) acc[t] += wp * q[t];
  }
#pragma unroll
  for (int t = 0; t < DG_ROWS; ++t) {
    double v = acc[t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0 && s0 + t < ns) D[(long)(s0 + t) * ldd + (hmap ? hmap[g] : g)] = v;
  }
}

// acc = the tile (rows s0 .., columns c0 ..) of Ad' (B o B): the product of both MFMA kernels below, which differ in the epilogue
__device__ __forceinline__ void diag_sq_tile(const MtLane& ln, const double* __restrict__ Ad, int ns, const double* __restrict__ B,
                                             long ldb, int m, long nc, int s0, long c0, double* __restrict__ As,
                                             double* __restrict__ Bs, v4f64 (&acc)[2][2]) {
  double areg[4], breg[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int k = k0 + MtRowK::sk(ln.t, ps);
      const int s = s0 + MtRowK::srow(ln.t, ps);
      const long cc = c0 + MtRowK::srow(ln.t, ps);
      const bool kin = k < m;
      areg[ps] = (kin && s < ns) ? Ad[(long)k + (long)s * m] : 0.0;
      breg[ps] = (kin && cc < nc) ? B[(long)k + cc * ldb] : 0.0;
    }
  };
  auto stage = [&](int ps, double* a, double* b) { *a = areg[ps]; *b = breg[ps] * breg[ps]; };
  mt_kloop<MtRowK, MtRowK>(ln, As, Bs, 0, m, fetch, stage, acc);
}

__global__ __launch_bounds__(256) void diag_sq_mfma_kernel(const double* __restrict__ Ad, int ns, const double* __restrict__ B,
                                                           long ldb, int m, long nc, int kh, const double* __restrict__ w,
                                                           double* __restrict__ D, long ldd, const int* __restrict__ hmap) {
  __shared__ double As[MtRowK::SIZE];
  __shared__ double Bs[MtRowK::SIZE];
  const MtLane ln = mt_lane();
  const long c0 = (long)blockIdx.x * MT_T;
  const int s0 = blockIdx.y * MT_T;
  v4f64 acc[2][2];
  diag_sq_tile(ln, Ad, ns, B, ldb, m, nc, s0, c0, As, Bs, acc);
  // weight, sum over the kh lanes of the group
#pragma unroll
  for (int jb = 0; jb < 2; ++jb) {
    const long cc = c0 + mt_col(ln, jb);
    const double wcol = cc < nc ? (w ? w[cc] : 1.0) : 0.0;
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double v = acc[ib][jb][r] * wcol;
        for (int off = 1; off < kh; off <<= 1) v += __shfl_xor(v, off, 64);      // (kh is uniform: every lane takes part)
        const int s = s0 + mt_row(ln, ib, r);
        if ((ln.ci & (kh - 1)) == 0 && s < ns && cc < nc) D[(long)s * ldd + (hmap ? (long)hmap[cc / kh] : cc / kh)] = v;
      }
  }
}

// ---- the MFMA form for column groups of 32 and 64 (a wide block with diagonal parts, option "wide_diag").
// A second kernel over the same product (diag_sq_tile), not a branch on kh in the one above: the two epilogues share no code,
// and as two kernels each keeps the registers it had (124 of the 128 that four waves per SIMD allow; mfma_tile.h).
// Geometry: the tile covers the columns c0 .. c0 + 63 with c0 % 64 == 0 and wave (wr, wc) holds the columns
// 32 wc + 16 jb + ci, so a group of 32 is exactly one wave's columns and a group of 64 the columns of the waves wc = 0 and
// wc = 1 of one wr.  Order of the sum, fixed -- the rule of raggedops.hip::ragged_wide_epilogue:
//   1. the accumulator element of column cc is multiplied by w[cc]; a column beyond nc has weight 0 (its operand is zero too);
//   2. inside each accumulator block the xor butterfly over the 16 ci lanes (offsets 1, 2, 4, 8);
//   3. across the wave's two accumulators, jb = 0 + jb = 1;
//   4. kh = 64: across the two waves of the row through LDS, wc = 0 + wc = 1.  The exchange reuses As after a barrier: the
//      lanes ci == 0 of a wave wc = 1 write their eight row sums to red[32 wr + 16 ib + kq + 4 r], and after a second barrier
//      the same lanes of the wave wc = 0 read them.  Both barriers sit in a branch on kh alone, a kernel argument, and no
//      lane has left before them: all 256 threads reach them.  LDS banks of the exchange: one ds_write_b64 has four active
//      lanes (kq = 0 .. 3, ci = 0) on four consecutive doubles, the reads are the same addresses: distinct bank pairs, no
//      conflict (derived from the bank rule, not measured);
//   5. one writer per element: the lane ci == 0 (of the wave wc == 0 for kh = 64) stores D[s ldd + (hmap ? hmap[g] : g)] for
//      s < ns and g < nc / kh.  A half-full last tile of a class-32 segment: the wave wc = 1 holds group nc / 32, no store.
// No atomics: two runs give the same bits.  The compiler's report (registers, LDS, occupancy): DESIGN section 23.
__global__ __launch_bounds__(256) void diag_sq_wide_mfma_kernel(const double* __restrict__ Ad, int ns, const double* __restrict__ B,
                                                                long ldb, int m, long nc, int kh, const double* __restrict__ w,
                                                                double* __restrict__ D, long ldd, const int* __restrict__ hmap) {
  __shared__ double As[MtRowK::SIZE];
  __shared__ double Bs[MtRowK::SIZE];
  const MtLane ln = mt_lane();
  const int wr = ln.wr, wc = ln.wc, ci = ln.ci, kq = ln.kq;
  const long c0 = (long)blockIdx.x * MT_T;
  const int s0 = blockIdx.y * MT_T;
  v4f64 acc[2][2];
  diag_sq_tile(ln, Ad, ns, B, ldb, m, nc, s0, c0, As, Bs, acc);
  // element (row s0 + 32 wr + 16 ib + kq + 4 r, column c0 + 32 wc + 16 jb + ci): steps 1 to 3, v[ib][r] = the wave's 32 columns
  double v[2][4];
  {
    const long cc0 = c0 + 32 * wc + ci, cc1 = cc0 + 16;
    const double w0 = cc0 < nc ? (w ? w[cc0] : 1.0) : 0.0;
    const double w1 = cc1 < nc ? (w ? w[cc1] : 1.0) : 0.0;
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double x0 = acc[ib][0][r] * w0, x1 = acc[ib][1][r] * w1;
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {     // (every lane takes part)
          x0 += __shfl_xor(x0, off, 64);
          x1 += __shfl_xor(x1, off, 64);
        }
        v[ib][r] = x0 + x1;
      }
  }
  const bool x64 = kh == 64;                         // (a kernel argument: uniform over the grid)
  if (x64) {
    double* __restrict__ red = As;                   // 64 of its 1152 doubles
    __syncthreads();                                 // every wave is done with the last K step's As
    if (wc == 1 && ci == 0) {
#pragma unroll
      for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[32 * wr + 16 * ib + kq + 4 * r] = v[ib][r];
    }
    __syncthreads();
    if (wc == 0 && ci == 0) {
#pragma unroll
      for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[ib][r] += red[32 * wr + 16 * ib + kq + 4 * r];
    }
  }
  if (ci != 0 || (x64 && wc != 0)) return;           // (after the barriers)
  const long g = x64 ? c0 / 64 : (c0 + 32 * wc) / 32;
  if (g >= nc / kh) return;
  const long gd = hmap ? (long)hmap[g] : g;
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int s = s0 + 32 * wr + 16 * ib + kq + 4 * r;
      if (s < ns) D[(long)s * ldd + gd] = v[ib][r];
    }
}

// D[s * ldd + g] = sum_{p < kh} w[g kh + p] sum_i Ad[i + s m] B[i + (g kh + p) ldb]^2   (w null: weights 1); s < ns, g < ng.
// hmap (option "ragged_cross": the groups of one rank class, B and w starting at its segment): the sum of group g goes to
// D[s * ldd + hmap[g]] instead -- the store alone differs; null is the code above
static int diag_sq(lrn_ctx* c, const double* Ad, int ns, const double* B, long ldb, int m, int ng, int kh, const double* w,
                   double* D, long ldd, const int* hmap = nullptr) {
  if (ns <= 0 || ng <= 0 || m <= 0 || kh <= 0) return LRN_OK;
  const bool mfma = c->opt.diag_sq_mfma == 1 || (c->opt.diag_sq_mfma < 0 && ns >= DG_MFMA_MIN);
  const long nc = (long)ng * kh;
  if (mfma) {
    // (the butterfly of the epilogue needs a column group on kh neighbouring lanes of one accumulator block)
    // (option "wide_diag": groups of 32 and 64, a wave's columns or the tile's, go to the kernel with the wide epilogue)
    const bool wide = (kh == 32 || kh == 64) && c->opt.wide_diag;
    if (!wide && (kh > 16 || (kh & (kh - 1)))) {
      if (!c->opt.wide_diag) return set_error(c, LRN_ERR_ARG, "diag_sq: the MFMA form needs khat in 1, 2, 4, 8, 16, not %d", kh);
      return set_error(c, LRN_ERR_ARG, "diag_sq: the MFMA form needs khat in 1, 2, 4, 8, 16, or 32 or 64 under option wide_diag, not %d", kh);
    }
    const long tx = (nc + MT_T - 1) / MT_T, ty = (ns + MT_T - 1) / MT_T;
    if (tx > 2147483647L || ty > 65535) return set_error(c, LRN_ERR_ARG, "diag_sq: %ld x %ld tiles", tx, ty);
    if (wide)
      hipLaunchKernelGGL(diag_sq_wide_mfma_kernel, dim3((unsigned)tx, (unsigned)ty), dim3(256), 0, c->stream, Ad, ns, B, ldb, m,
                         nc, kh, w, D, ldd, hmap);
    else
      hipLaunchKernelGGL(diag_sq_mfma_kernel, dim3((unsigned)tx, (unsigned)ty), dim3(256), 0, c->stream, Ad, ns, B, ldb, m, nc,
                         kh, w, D, ldd, hmap);
    c->counts["diag_sq_mfma"] += 1;
  } else {
    const long ty = (ns + DG_ROWS - 1) / DG_ROWS;
    if (ty > 65535) return set_error(c, LRN_ERR_ARG, "diag_sq: %ld row groups (rows form)", ty);
    hipLaunchKernelGGL(diag_sq_rows_kernel, dim3((unsigned)((ng + 3) / 4), (unsigned)ty), dim3(256), 0, c->stream, Ad, ns, B,
                       ldb, m, ng, kh, w, D, ldd, hmap);
    c->counts["diag_sq_rows"] += 1;
  }
  return LRN_OK;
}

// ---------------------------------------------------------------- scatters into the lower triangle of H: one writer per entry
// H_DD: thread (s, t), s >= t, adds HDD[s, t] (the lower triangle of the product; dg_n x dg_n column-major)
__global__ __launch_bounds__(256) void diag_dd_scatter_kernel(const double* __restrict__ HDD, int ns, const int* __restrict__ dgh,
                                                              double* __restrict__ H, int ldh) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= ns) return;
  for (int t = blockIdx.y; t <= s; t += gridDim.y) H[h_lower(dgh[s], dgh[t], ldh)] += HDD[(long)s + (long)t * ns];
}

// C + C' over the factored positions: thread (diagonal row s, position j >= p_f).  j not a diagonal row: the one term C[s, j].
// Both diagonal rows: the thread whose row has the larger H index writes C[s, j] + C[j, s]; s == j: 2 C[s, s].
__global__ __launch_bounds__(256) void diag_cross_scatter_kernel(const double* __restrict__ C, int ns, const int* __restrict__ dgh,
                                                                 const int* __restrict__ dg_of_pos, const int* __restrict__ hidx,
                                                                 int p_f, int p_end, double* __restrict__ H, int ldh) {
  const int j = p_f + blockIdx.x * 256 + threadIdx.x;
  if (j >= p_end) return;
  const int hj = hidx[j], t = dg_of_pos[j];
  for (int s = blockIdx.y; s < ns; s += gridDim.y) {
    const int hs = dgh[s];
    const double csj = C[(long)s * ldh + hj];
    if (t < 0) H[h_lower(hs, hj, ldh)] += csj;
    else if (hs > hj) H[(long)hs + (long)hj * ldh] += csj + C[(long)t * ldh + hs];
    else if (hs == hj) H[(long)hs + (long)hs * ldh] += 2.0 * csj;
  }
}

// stored position s < npos_nz against diagonal row k: TA[s, k] = t_s' a_k
__global__ __launch_bounds__(256) void diag_stored_scatter_kernel(const double* __restrict__ TA, int nst, int ns,
                                                                  const int* __restrict__ hidx, const int* __restrict__ dgh,
                                                                  double* __restrict__ H, int ldh) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nst) return;
  for (int k = blockIdx.y; k < ns; k += gridDim.y) H[h_lower(hidx[s], dgh[k], ldh)] += TA[(long)s + (long)k * nst];
}

// t_s[i] = diag(W A_s W)_i = sum_e ev_e W[i, r_e] W[i, c_e] for the sparse-tier stored position s = s_lo + blockIdx.x; W is
// symmetric, so row i of columns r_e, c_e is read -- coalesced over the threads.  T[s m + i]
__global__ __launch_bounds__(256) void diag_ts_sparse_kernel(const long* __restrict__ ptr, const int* __restrict__ er,
                                                             const int* __restrict__ ec, const double* __restrict__ ev,
                                                             const double* __restrict__ W, int m, int s_lo, double* __restrict__ T) {
  const int s = s_lo + blockIdx.x;
  const long b = ptr[s], e = ptr[s + 1];
  for (int i = blockIdx.y * 256 + threadIdx.x; i < m; i += gridDim.y * 256) {
    double t = 0.0;
    for (long f = b; f < e; ++f) t += ev[f] * W[(long)i + (long)er[f] * m] * W[(long)i + (long)ec[f] * m];
    T[(long)s * m + i] = t;
  }
}

// dense slot: Q = A_s W; t_s[i] = sum_j W[i, j] Q[j, i] = <W(:, i), Q(:, i)> (W symmetric): one wave per column i, lanes stride j
__global__ __launch_bounds__(256) void diag_ts_dense_kernel(const double* __restrict__ Q, const double* __restrict__ W, int m,
                                                            double* __restrict__ Ts) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= m) return;                              // (whole wave)
  const double* __restrict__ q = Q + (long)i * m;
  const double* __restrict__ w = W + (long)i * m;
  double t = 0.0;
  for (int j = lane; j < m; j += 64) t += q[j] * w[j];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  if (lane == 0) Ts[i] = t;
}

int assemble_diag(lrn_ctx* c, LmiBlock& b, const double* Y) {
  const int n = c->nvar, m = b.msz, kh = b.lr_khat, ns = b.dg_n;
  if (ns <= 0) return LRN_OK;
  if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set (call lrn_prepare_w or lrn_set_scaling)");
  if (!Y) return set_error(c, LRN_ERR_STATE, "diagonal parts: Y = W Vd was not formed");
  const double* Ad = b.dg_a.as<double>();
  const int* dgh = b.dg_h.as<int>();
  double* H = c->H.as<double>();
  const unsigned gy = (unsigned)std::min(ns, 65535);      // (the scatters stride the rows by gridDim.y)
  // H_DD = P Ad with P = Ad' (W o W) (dg_n x msz, row s contiguous), lower triangle
  tic(c);
  LRN_TRY(ensure(c, c->dgP, (size_t)ns * m * 8));
  LRN_TRY(ensure(c, c->dgH, (size_t)ns * ns * 8));
  LRN_TRY(diag_sq(c, Ad, ns, b.W.as<double>(), m, m, m, 1, nullptr, c->dgP.as<double>(), m));
  {
    GemmDesc g;
    g.A = c->dgP.as<double>(); g.sAm = m; g.sAk = 1;
    g.B = Ad; g.sBk = 1; g.sBn = m;
    g.C = c->dgH.as<double>(); g.sCm = 1; g.sCn = ns;
    g.M = ns; g.N = ns; g.K = m;
    g.flags = GEMM_TRI_LOWER;
    LRN_TRY(gemm(c->stream, g));
  }
  hipLaunchKernelGGL(diag_dd_scatter_kernel, dim3((ns + 255) / 256, gy), dim3(256), 0, c->stream, c->dgH.as<double>(), ns, dgh,
                     H, n);
  toc(c, "diag_dd");
  // C = Ad' (Y o Y), weighted by d and summed over khat: dg_n x nvar by H index (row s contiguous), then C + C'
  tic(c);
  LRN_TRY(ensure(c, c->dgC, (size_t)ns * n * 8));
  if (ragged_cross_on(c, b)) {
    // option "ragged_cross": Y is Yc = W Vc (factored_y).  Inside one class segment the group size is uniform, so either form
    // runs per class on B = Yc + seg0 msz, w = wc + seg0 and stores through the class's part of gh; a constraint of rank 0 has
    // no writer: C is zeroed first
    LRN_TRY(ragged_setup(c, b));
    LRN_HIP(c, hipMemsetAsync(c->dgC.p, 0, (size_t)ns * n * 8, c->stream));
    for (int ci = 0; ci < RG_NCLS; ++ci) {
      const int ngc = b.rg_grp0[ci + 1] - b.rg_grp0[ci];
      if (ngc <= 0) continue;
      LRN_TRY(diag_sq(c, Ad, ns, Y + b.rg_seg0[ci] * m, m, m, ngc, ragged_class_size(ci), b.rg_wc.as<double>() + b.rg_seg0[ci],
                      c->dgC.as<double>(), n, b.rg_gh.as<int>() + b.rg_grp0[ci]));
    }
  } else
    LRN_TRY(diag_sq(c, Ad, ns, Y, m, m, n, kh, b.v_w.as<double>(), c->dgC.as<double>(), n));
  hipLaunchKernelGGL(diag_cross_scatter_kernel, dim3((n - b.npos_nz + 255) / 256, gy), dim3(256), 0, c->stream,
                     c->dgC.as<double>(), ns, dgh, b.dg_of_pos.as<int>(), b.hidx.as<int>(), b.npos_nz, n, H, n);
  toc(c, "diag_cross");
  if (b.npos_nz > 0) {
    // stored rows of a hybrid block: T (row s = diag(W A_s W)), TA = T Ad, one scatter
    tic(c);
    const int nst = b.npos_nz;
    LRN_TRY(ensure(c, c->dgT, (size_t)nst * m * 8));
    LRN_TRY(ensure(c, c->dgTA, (size_t)nst * ns * 8));
    double* T = c->dgT.as<double>();
    if (b.nd > 0) {
      LRN_TRY(ensure_m(c, m));
      for (int s = 0; s < b.nd; ++s) {
        GemmDesc g;     // Q = A_s W
        g.A = b.Adense.as<double>() + (long)s * m * m; g.sAm = 1; g.sAk = m;
        g.B = b.W.as<double>(); g.sBk = 1; g.sBn = m;
        g.C = c->m0.as<double>(); g.sCm = 1; g.sCn = m;
        g.M = m; g.N = m; g.K = m;
        LRN_TRY(gemm(c->stream, g));
        hipLaunchKernelGGL(diag_ts_dense_kernel, dim3((m + 3) / 4), dim3(256), 0, c->stream, c->m0.as<double>(),
                           b.W.as<double>(), m, T + (long)s * m);
      }
    }
    if (nst > b.nd)
      hipLaunchKernelGGL(diag_ts_sparse_kernel, dim3(nst - b.nd, std::min((m + 255) / 256, 65535)), dim3(256), 0, c->stream, b.ent_ptr.as<long>(),
                         b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(), b.W.as<double>(), m, b.nd, T);
    GemmDesc g;     // TA[s, k] = sum_i T[s m + i] Ad[i, k]
    g.A = T; g.sAm = m; g.sAk = 1;
    g.B = Ad; g.sBk = 1; g.sBn = m;
    g.C = c->dgTA.as<double>(); g.sCm = 1; g.sCn = nst;
    g.M = nst; g.N = ns; g.K = m;
    LRN_TRY(gemm(c->stream, g));
    hipLaunchKernelGGL(diag_stored_scatter_kernel, dim3((nst + 255) / 256, gy), dim3(256), 0, c->stream, c->dgTA.as<double>(),
                       nst, ns, b.hidx.as<int>(), dgh, H, n);
    toc(c, "diag_stored");
    c->counts["diag_stored_cross"] += 1;
  }
  c->counts["schur_diag"] += 1;
  return LRN_OK;
}

// ---------------------------------------------------------------- data operators
// y[nat(s)] -= sum_i a_si Z_ii: one wave per diagonal row, lanes stride i, one shuffle tree
__global__ __launch_bounds__(256) void diag_aa_times_kernel(const double* __restrict__ Ad, const int* __restrict__ nat, int ns,
                                                            const double* __restrict__ Z, int m, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= ns) return;
  double v = 0.0;
  for (int i = lane; i < m; i += 64) v += Ad[(long)i + (long)s * m] * Z[(long)i * (m + 1)];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) y[nat[s]] -= v;
}

// M_ii -= sum_s x[nat(s)] a_si in two steps, so that many rows do not hang on msz threads: workgroup (x, y) takes 64 entries i
// and the 64 rows of chunk y -- wave q the rows 16 q .. 16 q + 15 in order, the four waves added in LDS as (0 + 1) + (2 + 3) --
// and writes part[y m + i]; diag_aat_apply_kernel adds the chunks in order, one thread per i.  Only the diagonal of M changes:
// M stays exactly symmetric.  Fixed order, no atomics
__global__ __launch_bounds__(256) void diag_aat_part_kernel(const double* __restrict__ Ad, const int* __restrict__ nat, int ns,
                                                            const double* __restrict__ x, int m, double* __restrict__ part) {
  __shared__ double red[4][64];
  const int li = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + li;
  const int sb = blockIdx.y * 64 + q * 16;
  double v = 0.0;
  if (i < m)
    for (int t = 0; t < 16; ++t) {
      const int s = sb + t;
      if (s < ns) v += x[nat[s]] * Ad[(long)i + (long)s * m];
    }
  red[q][li] = v;
  __syncthreads();
  if (q == 0 && i < m) part[(long)blockIdx.y * m + i] = (red[0][li] + red[1][li]) + (red[2][li] + red[3][li]);
}

__global__ __launch_bounds__(256) void diag_aat_apply_kernel(const double* __restrict__ part, int nch, int m,
                                                             double* __restrict__ M) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  double v = 0.0;
  for (int ch = 0; ch < nch; ++ch) v += part[(long)ch * m + i];
  M[(long)i * (m + 1)] -= v;
}

int aa_times_diag(lrn_ctx* c, LmiBlock& b, const double* Z, double* y) {
  if (b.dg_n <= 0) return LRN_OK;
  hipLaunchKernelGGL(diag_aa_times_kernel, dim3((b.dg_n + 3) / 4), dim3(256), 0, c->stream, b.dg_a.as<double>(),
                     b.dg_nat.as<int>(), b.dg_n, Z, b.msz, y);
  c->counts["op_diag"] += 1;
  return LRN_OK;
}

int aat_to_mat_diag(lrn_ctx* c, LmiBlock& b, const double* x, double* M) {
  if (b.dg_n <= 0) return LRN_OK;
  const int m = b.msz, nch = (b.dg_n + 63) / 64;
  if (nch > 65535) return set_error(c, LRN_ERR_ARG, "diagonal parts: %d rows", b.dg_n);
  LRN_TRY(ensure(c, c->dgP, (size_t)nch * m * 8));      // (the P workspace of the assembly: at least dg_n x msz there)
  hipLaunchKernelGGL(diag_aat_part_kernel, dim3((m + 63) / 64, nch), dim3(256), 0, c->stream, b.dg_a.as<double>(),
                     b.dg_nat.as<int>(), b.dg_n, x, m, c->dgP.as<double>());
  hipLaunchKernelGGL(diag_aat_apply_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, c->dgP.as<double>(), nch, m, M);
  c->counts["op_diag"] += 1;
  return LRN_OK;
}

// ---------------------------------------------------------------- ts of H_alpha (option "cg_diag", prec.hip::prec_setup)
// The rows of ts that belong to diagonal rows miss  -(L' diag(a_s) u_a)[r] / sqrt(d_j)  after fac_ts_kernel (which holds the
// factor part, a zero for a purely diagonal constraint).  With L the Cholesky factor of 2 W - Um Um' (lower, upper triangle
// zeroed, element (i, r) at L[i + r m]) and u_a column a of Um,
//     ts[nat(s), a m + r] += -(1 / sqrt(d[nat(s)])) sum_{i >= r} Ad[i, s] Um[i, a] L[i, r]
// is a dense product with both operands K-contiguous (column r of L, column s of Ad) -- the tile of mfma_tile.h with two
// [row][k] panels, as in diag_sq_mfma_kernel, but WRITTEN OUT here, the one kernel of the family that is: over mt_kloop it
// compiled to 120 instead of 116 registers with another order of the staging stores and measured 2 to 3 % slower at one
// diagonal row (0.124 against 0.121 ms at msz 2000, both runs of both sides; profiles/mfma_tile_refactor_ab.txt).  As written
// here its code object is the one it had.  A change to the loop in mfma_tile.h is to be made here too.
// What is particular to this kernel:
//   operands: As[r][k] = L[k0 + k, r0 + r],  Bs[s][k] = Ad[k0 + k, s0 + s] Um[k0 + k, a]  (scaled as it is staged, where diag_sq
//     squares; one value of Um per thread and K step, its staging column k is fixed); blockIdx.x picks 64 columns r of L,
//     blockIdx.y 64 diagonal rows s, blockIdx.z the eigenvector a
//   triangular K range: column r of L is zero above row r, so the tile of columns r0 .. r0 + 63 starts at k0 = r0 & ~15 (r0 is a
//     multiple of 64: k0 = r0) and a tile with r0 >= m does not exist; inside the first K steps the zeros of L do the masking
//   transposed store: ts is contiguous along its rows j, so the DIAGONAL ROWS are the B operand -- the sixteen ci lanes of an
//     accumulator block run over s.  A store instruction writes, per register, 4 (kq) x 16 (ci) elements: sixteen lanes one
//     run of ts column a m + r at rows nat(s) .. -- 128 contiguous bytes where the diagonal rows are consecutive constraints --
//     and the four kq groups four neighbouring columns.  No LDS transpose
//   accumulating epilogue: scaled by -1 / sqrt(d[nat(s)]) and ADDED to what fac_ts_kernel left; diagonal rows are no stored
//     rows (lrn_upload_diag), every element of ts has one writer, no atomics: two setups give the same bits
__global__ __launch_bounds__(256) void ts_diag_mfma_kernel(const double* __restrict__ Lf, const double* __restrict__ Ad, int ns,
                                                           const double* __restrict__ Um, const int* __restrict__ nat,
                                                           const double* __restrict__ d, int m, int nvar,
                                                           double* __restrict__ ts) {
  constexpr int LD = MtRowK::LD;
  __shared__ double As[MtRowK::SIZE];
  __shared__ double Bs[MtRowK::SIZE];
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = wv >> 1, wc = wv & 1;
  const int ci = lane & 15, kq = lane >> 4;
  const int r0 = blockIdx.x * MT_T;
  const int s0 = blockIdx.y * MT_T;
  const double* __restrict__ ua = Um + (long)blockIdx.z * m;
  v4f64 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};
  // staging map of both operands: thread (k = t & 15, row = (t >> 4) + 16 pass)
  const int vk = t & 15, vr = t >> 4;
  double areg[4], breg[4], ureg;
  auto fetch = [&](int k0) {
    const bool kin = k0 + vk < m;
    ureg = kin ? ua[k0 + vk] : 0.0;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int r = r0 + vr + 16 * ps;
      const int s = s0 + vr + 16 * ps;
      areg[ps] = (kin && r < m) ? Lf[(long)(k0 + vk) + (long)r * m] : 0.0;
      breg[ps] = (kin && s < ns) ? Ad[(long)(k0 + vk) + (long)s * m] : 0.0;
    }
  };
  const int kbeg = r0 & ~(MT_K - 1);         // rows of L above r0 are zero in every column of the tile
  fetch(kbeg);
  for (int k0 = kbeg; k0 < m; k0 += MT_K) {
    __syncthreads();                       // the waves are done with the previous step's tiles
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      As[(vr + 16 * ps) * LD + vk] = areg[ps];
      Bs[(vr + 16 * ps) * LD + vk] = breg[ps] * ureg;
    }
    __syncthreads();
    if (k0 + MT_K < m) fetch(k0 + MT_K);
#pragma unroll
    for (int ks = 0; ks < MT_K / 4; ++ks) {
      const int k = 4 * ks + kq;
      const double a0 = As[(32 * wr + ci) * LD + k];
      const double a1 = As[(32 * wr + 16 + ci) * LD + k];
      const double b0 = Bs[(32 * wc + ci) * LD + k];
      const double b1 = Bs[(32 * wc + 16 + ci) * LD + k];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // element (column r0 + 32 wr + 16 ib + kq + 4 q of L, diagonal row s0 + 32 wc + 16 jb + ci)
#pragma unroll
  for (int jb = 0; jb < 2; ++jb) {
    const int s = s0 + 32 * wc + 16 * jb + ci;
    if (s >= ns) continue;
    const int j = nat[s];
    const double sc = -1.0 / sqrt(d[j]);
    double* __restrict__ out = ts + ((long)blockIdx.z * m) * nvar + j;
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + 32 * wr + 16 * ib + kq + 4 * q;
        if (r < m) out[(long)r * nvar] += sc * acc[ib][jb][q];
      }
  }
}

// ts (the block's nvar x erank msz part, column 0 = its first) += the diagonal-row term; L = chol(2 W - Um Um') with a zeroed
// upper triangle, Um msz x erank, d the nvar scalings of H_alpha.  One form
int ts_diag(lrn_ctx* c, LmiBlock& b, const double* Lf, const double* Um, int erank, const double* d, double* ts) {
  const int m = b.msz, ns = b.dg_n;
  if (ns <= 0 || erank <= 0) return LRN_OK;
  const long tx = (m + MT_T - 1) / MT_T, ty = (ns + MT_T - 1) / MT_T;
  if (ty > 65535 || erank > 65535) return set_error(c, LRN_ERR_ARG, "ts_diag: %ld row tiles, erank %d", ty, erank);
  hipLaunchKernelGGL(ts_diag_mfma_kernel, dim3((unsigned)tx, (unsigned)ty, (unsigned)erank), dim3(256), 0, c->stream, Lf,
                     b.dg_a.as<double>(), ns, Um, b.dg_nat.as<int>(), d, m, c->nvar, ts);
  c->counts["ts_diag_mfma"] += 1;
  return LRN_OK;
}

}  // namespace lrn
