// Fused quadratic form of the factor-form data operator (option "fac_quadform", dataops.hip::aa_times_factored).
//
// (AA vec(Z))_j = -sum_p w_jp v_jp' Z v_jp over the khat factor columns of constraint j.  The composition of dataops.hip forms
// Q = Z Vd (msz x R, R = nvar khat) by one MFMA product, writes it to HBM and reads it back beside Vd for the column dots:
// 32 m R bytes against 2 m^2 R flop, m / 16 flop per byte -- below the FP64 balance of the machine for m under about 250,
// the regime of kit = 1 (msz in the low hundreds, nvar in the tens of thousands).  Here Q never leaves the registers.
//
// fac_quadform_kernel: 256 threads, workgroup tile = 64 rows of Z (strip blockIdx.y) x 64 factor columns (blockIdx.x).  khat
// is a power of two <= 64 (32 and 64: a wide block), so a column tile holds whole constraints.  The product is the tile of
// mfma_tile.h over K = m (lane maps, LDS banks and the K loop are derived there), one panel of each layout:
//   Zs[k][i] = Z[i0 + i, k0 + k]   the [k][row] panel (Z is symmetric: read down its columns, coalesced)
//   Vs[c][k] = Vd[k0 + k, c0 + c]  the [row][k] panel
// 10 240 + 9 216 bytes, and 1 024 bytes for the sums of the two wave rows: 20 480 bytes of LDS, eight workgroups per CU of
// 160 KiB by LDS; the registers (80 VGPRs + 32 accumulator registers per lane) allow four waves per SIMD, i.e. four
// workgroups per CU.
// Epilogue: every accumulator element is multiplied by the element of Vd it belongs to (row i of column c) and the rows are
// summed per column: registers, then the xor-16 / xor-32 butterfly over the four row groups of a wave, then the two wave
// rows through LDS in the order 0, 1.  One partial per (strip, column) goes to a slab of ceil(m / 64) x R doubles, 1 / 64
// of Q.  fac_quadform_reduce_kernel adds the strips in order and the columns p = 0 .. khat - 1 with their weights, skips
// weight-0 columns and maps through sigma as fac_coldot_kernel does.  No atomics: two applications give the same bits.
// The strip dimension of the grid is what fills the chip when R / 64 is small.
#include "../../include/loraine_hip.h"
#include "ctx.h"
#include "ops.h"
#include "fac_cols.h"
#include "mfma_tile.h"

namespace lrn {

static constexpr int FQ_T = MT_T;      // tile side (rows of Z, factor columns)

__global__ __launch_bounds__(256) void fac_quadform_kernel(const double* __restrict__ Z, const double* __restrict__ Vd, int m,
                                                           long R, double* __restrict__ part) {
  __shared__ double Zs[MtKRow::SIZE];
  __shared__ double Vs[MtRowK::SIZE];
  __shared__ double red[2][FQ_T];
  const MtLane ln = mt_lane();
  const int t = ln.t;
  const long c0 = (long)blockIdx.x * FQ_T;
  const int i0 = blockIdx.y * FQ_T;
  v4f64 acc[2][2];
  double zreg[4], vreg[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int k = k0 + MtKRow::sk(t, ps), i = i0 + MtKRow::srow(t, ps);
      zreg[ps] = (k < m && i < m) ? Z[(long)i + (long)k * m] : 0.0;
      const int kv = k0 + MtRowK::sk(t, ps);
      const long c = c0 + MtRowK::srow(t, ps);
      vreg[ps] = (kv < m && c < R) ? Vd[(long)kv + c * m] : 0.0;
    }
  };
  auto stage = [&](int ps, double* a, double* b) { *a = zreg[ps]; *b = vreg[ps]; };
  mt_kloop<MtKRow, MtRowK>(ln, Zs, Vs, 0, m, fetch, stage, acc);
  // <Q(:, c), Vd(:, c)> over the 32 rows of this wave
#pragma unroll
  for (int jb = 0; jb < 2; ++jb) {
    const long c = c0 + mt_col(ln, jb);
    double s = 0.0;
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + mt_row(ln, ib, r);
        const double v = (i < m && c < R) ? Vd[(long)i + c * m] : 0.0;
        s += acc[ib][jb][r] * v;
      }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (ln.kq == 0) red[ln.wr][mt_col(ln, jb)] = s;
  }
  __syncthreads();
  if (t < FQ_T && c0 + t < R) part[(long)blockIdx.y * R + c0 + t] = red[0][t] + red[1][t];
}

// out[nat(h)] -= sum_p w[col] sum_strips part[strip][col] over the columns col of unit u of the layout, h its H index (one
// thread per unit; the strips in order, then the columns in order)
template <class Cols>
__global__ __launch_bounds__(256) void fac_quadform_reduce_kernel(const double* __restrict__ part, int nstrip, long R,
                                                                  const double* __restrict__ w, Cols lay,
                                                                  const int* __restrict__ sigma, double* __restrict__ out) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  typename Cols::Span span;
  int cnt;
  if (!lay.unit(u, &span, &cnt)) return;
  double s = 0.0;
  for (int p = 0; p < cnt; ++p) {
    const long col = lay.col(span, p);
    const double wp = w[col];
    if (wp == 0.0) continue;                       // padding column
    double q = 0.0;
    for (int st = 0; st < nstrip; ++st) q += part[(long)st * R + col];
    s += wp * q;
  }
  const int h = lay.unit_h(u, span);
  out[sigma ? sigma[h] : h] -= s;
}

// fac_quadform_kernel: *part = nstrip x R partial sums of <(Z V)(:, c), V(:, c)> by row strips, on any column layout V (msz x R)
static int fac_quadform_parts(lrn_ctx* c, const double* Z, const double* V, int m, long R, double** part, int* nstrip_out) {
  const int nstrip = (m + FQ_T - 1) / FQ_T;
  const long ntile = (R + FQ_T - 1) / FQ_T;
  if (ntile > 2147483647L || nstrip > 65535) return set_error(c, LRN_ERR_ARG, "fac_quadform: %ld x %d tiles", ntile, nstrip);
  LRN_TRY(ensure(c, c->slabs, (size_t)nstrip * (size_t)R * 8));
  *part = c->slabs.as<double>();
  *nstrip_out = nstrip;
  hipLaunchKernelGGL(fac_quadform_kernel, dim3((unsigned)ntile, (unsigned)nstrip), dim3(256), 0, c->stream, Z, V, m, R, *part);
  return LRN_OK;
}

int fac_quadform(lrn_ctx* c, const LmiBlock& b, const FacCols& v, const double* Z, const int* sigma, double* out) {
  const int m = b.msz;
  if (m <= 0 || v.R <= 0) return LRN_OK;
  double* part = nullptr;
  int nstrip = 0;
  LRN_TRY(fac_quadform_parts(c, Z, v.V, m, v.R, &part, &nstrip));
  with_layout(c, b, v, [&](auto lay) {
    hipLaunchKernelGGL(fac_quadform_reduce_kernel<decltype(lay)>, dim3((v.nunit + 255) / 256), dim3(256), 0, c->stream, part,
                       nstrip, v.R, v.w, lay, sigma, out);
  });
  c->counts["op_quadform_fused"] += 1;
  return LRN_OK;
}

// ================================================================ ts of H_alpha from the factors
// ts of H_alpha of a block that takes the factor route (a factored block; a covered one under option "cg_lowrank").  With A_j
// = sum_p w_p v_p v_p' over the columns p of constraint j, L the Cholesky factor of 2 W - Um Um' and u_a column a of Um, the
// entry route forms  ts[j, a m + r] = -(L' A_j u_a)[r] / sqrt(d_j)  by one pass over every A_j per eigenvector.  Here
// P = L' V  (m x R, one MFMA product for ALL eigenvectors) and  T = V' Um  (R x erank) come first (prec.hip::prec_setup), and
//     ts[j, col0 + a m + r] = -(1 / sqrt(d_j)) sum_p w[p] T[p, a] P[r, p]
// is what this kernel does: a weighted sum of the columns of P of each constraint, in their order, padding skipped (no atomics:
// two setups give the same bits), written TRANSPOSED -- P is contiguous along r, ts along j.  V is Vd or, under option
// "ragged_ts", the compacted columns Vc of a block of mixed ranks; the weighted columns keep their order in a group, so both
// layouts form the same sum.  A constraint without columns (compacted layout, rank 0: a stored row, a purely diagonal row)
// stores 0, as do rows j >= nvar and r >= msz of a partial tile.
// Workgroup tile: 64 constraints (natural rows j0 .. j0 + 63 of ts) x 64 rows r of P, eigenvector a = blockIdx.z.  Wave w
// takes the constraints j0 + w, j0 + w + 4, .., h = ipos ? ipos[j] : j: its 64 lanes read 64 consecutive doubles of each column
// of P (512 B per load, coalesced whatever the order of h) with the coefficient w T as a wave-uniform scalar, and store the
// sums as row jl of an LDS tile of 64 x 65 doubles (33 280 bytes; ds_write_b64 of consecutive addresses).  After the barrier
// lane l of wave w reads tile[l][rr], rr = w, w + 4, .. -- a stride of 65 doubles = 130 banks, 2 l mod 64 over a 32-lane half:
// conflict-free, where 64 would be a 32-way conflict (derived from the bank rule, not measured) -- and the wave writes 64
// consecutive rows j of one column of ts.  Every element of the block's part of ts is written exactly once: no memset.
static constexpr int FTS_TILE = 64;
template <class Cols>
__global__ __launch_bounds__(256) void fac_ts_kernel(const double* __restrict__ Pm, const double* __restrict__ T,
                                                     const double* __restrict__ w, const int* __restrict__ ipos,
                                                     const double* __restrict__ d, int m, Cols lay, long R, int nvar,
                                                     double* __restrict__ ts) {
  __shared__ double tile[FTS_TILE][FTS_TILE + 1];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j0 = blockIdx.x * FTS_TILE, r0 = blockIdx.y * FTS_TILE, a = blockIdx.z;
  const double* __restrict__ Ta = T + (long)a * R;
  const int r = r0 + lane;
  for (int jl = wv; jl < FTS_TILE; jl += 4) {
    const int j = j0 + jl;
    double s = 0.0;
    if (j < nvar) {                                  // (wave-uniform)
      typename Cols::Span span;
      int cnt;
      if (lay.of_h(ipos ? ipos[j] : j, &span, &cnt)) {  // (no columns: the row stays zero)
        const long c0 = lay.col(span, 0);
        for (int p = 0; p < cnt; ++p) {
          const double wp = w[c0 + p];
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
  for (int rr = wv; rr < FTS_TILE && r0 + rr < m; rr += 4) out[(long)(r0 + rr) * nvar] = sc * tile[lane][rr];
}

// P = L' V (msz x R) and T = V' Um (R x erank) on the columns of the view
int fac_ts(lrn_ctx* c, const LmiBlock& b, const FacCols& v, const double* P, const double* T, const double* d, int erank,
           double* ts) {
  const int n = c->nvar, m = b.msz;
  const long tx = (n + FTS_TILE - 1) / FTS_TILE, ty = (m + FTS_TILE - 1) / FTS_TILE;
  if (ty > 65535 || erank > 65535) return set_error(c, LRN_ERR_ARG, "%s: %ld row tiles, erank %d", v.compact ? "ragged_ts" : "fac_ts", ty, erank);
  with_layout(c, b, v, [&](auto lay) {
    hipLaunchKernelGGL(fac_ts_kernel<decltype(lay)>, dim3((unsigned)tx, (unsigned)ty, (unsigned)erank), dim3(256), 0, c->stream, P,
                       T, v.w, c->pos_space ? b.ipos_d.as<int>() : (const int*)nullptr, d, m, lay, v.R, n, ts);
  });
  return LRN_OK;
}

}  // namespace lrn
