// Host-side launch plan of the Schur assembly (schur.hip, schur_dense.hip, schur_factored.hip): batch sizes, split-K
// factors, the column split of the Cholesky path and the owned column blocks.  Pure functions of sizes and option values --
// no context, no HIP runtime call, no allocator state -- so that what the benchmarked path launches is pinned without a GPU
// (lrn_dbg_schur_chol_plan, tests/test_schur_plan_cpu.py).
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "lrn_common.h"

namespace lrn {

// Workgroup-slot quantisation: the chip holds 256 CUs x 2 workgroups of these GEMMs at once and
// all workgroups of a launch take the same time, so a launch of `wgs` workgroups runs in
// ceil(wgs / 512) rounds.  Pick batch sizes / split-K factors that fill the last round.
static constexpr long WG_SLOTS = 512;
inline double fill_eff(long wgs) { return (double)wgs / (double)(((wgs + WG_SLOTS - 1) / WG_SLOTS) * WG_SLOTS); }

inline int pick_ksplit(long tiles, int max_split) {
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

// split-K of GEMM3 / GEMM3': short workgroups fill the workgroup slots evenly -- measured at C4: GEMM3' 548 / 524 / 509 /
// 505 ms with 8 / 16 / 32 / 64 splits.  Largest factor <= k_top that fills whole rounds of workgroup slots, leaves every
// split >= min_chunks of the `chunks` K-chunks and keeps the slabs (mn elements each) within 9 GB; pick_ksplit otherwise.
inline int pick_ksplit_short(long tiles, int max_split, int k_top, long chunks, long min_chunks, double mn) {
  const int ksplit = pick_ksplit(tiles, max_split);
  for (int k = k_top; k > ksplit; --k) {
    if (chunks / k < min_chunks || (double)k * mn * 8.0 > 9.0e9) continue;
    if (fill_eff(tiles * k) >= 0.97) return k;
  }
  return ksplit;
}

inline long pick_p_batch(int m, long limit) {
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

// Matrices per launch of the triangular-K products: their workgroups differ in length, so every launch ends with a
// drain of about half the longest workgroup -- fewer, larger launches (measured at C4: GEMM1'+GEMM2' 569 / 555 /
// 547 / 545 ms per step with 64 / 128 / 256 / 500 matrices per launch); up to 8.6 GB of P workspace.
// Round 3: with the masked K-steps cheaper the drains show again -- 16 / 8 / 4 / 2 launches per step: GEMM1' 335.8 / 335.3 /
// 333.6 / 334.3, GEMM2' 177.1 / 176.4 / 175.3 / 175.2 ms; `large` = up to 34 GB (1000 matrices at C4) where the memory
// is there (chol_path_applicable).
inline long tri_p_batch(int m, bool large = false) {
  long p = (long)((large ? 34.4e9 : 8.6e9) / ((double)m * m * 8.0));
  return std::max<long>(16, std::min<long>(large ? 1024 : 256, p));
}

// The positions [lo, hi) cut at the Schur column blocks (shard_bs wide) this rank owns -- all of them on one GPU -- and into
// pieces of at most `piece`: the owner ranges of one pair-kernel launch, the owner groups of the dense assembly, the column
// blocks of the rank-one / rank-k products.  The grid of a pair launch is (partners of its FIRST owner) x (owners), so a
// long range launches workgroups that find no partner (half of them for one launch over the whole triangle), and a rank of a
// sharded run would launch the seven eighths it does not own just to return (round 4: C5 at 8 ranks 18.1 -> see
// profiles/r04_shard_balance_c5.txt)
inline std::vector<std::pair<int, int>> owned_ranges(int rank, int world, int shard_bs, int lo, int hi, int piece) {
  std::vector<std::pair<int, int>> out;
  auto cut = [&](int a, int b) {
    for (int x = a; x < b; x += piece) out.push_back({x, std::min(b, x + piece)});
  };
  if (world > 1) {
    for (int c0 = (lo / shard_bs) * shard_bs; c0 < hi; c0 += shard_bs)
      if (shard_owner(c0 / shard_bs, world) == rank) cut(std::max(lo, c0), std::min(hi, c0 + shard_bs));
  } else {
    cut(lo, hi);
  }
  return out;
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
inline double col_range_cost(int m, int nd, int c0, int c1, int S) {
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

// this rank's columns [c0, c1) of the matrix variable; false: a rank left idle (more ranks than 16-column units)
inline bool col_runs(int m, int nd, int rank, int world, int* c0, int* c1) {
  const int S = packed_S(m), nu = S / 16;          // 16-column units
  *c0 = 0;
  *c1 = world <= 1 ? m : 0;
  if (world <= 1) return true;
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
  if (rank >= P) return false;
  *c0 = col(lo[rank]);
  *c1 = col(hi[rank]);
  return true;
}

// weights of the split-K slabs of GEMM3' (1: diagonal 16-blocks, 2: strictly-lower blocks), a kernel argument of the slab
// reduction
struct SlabWeights {
  static constexpr int MAXS = 160;
  float w[MAXS];
};

// the option values the plan of the Cholesky path reads (LrnOptions)
struct CholPlanOpts {
  long p_batch = 0;
  int gemm3_tile = 0, gemm3_ksplit = 0, gemm3_sched = 1, gemm3_strip = 1, gemm_no_skip = 0;
};

// Everything assemble_dense_chol decides before its launches.
struct CholPlan {
  bool idle = false;             // no columns for this rank: no GEMM launch, an empty slab reduction
  int c0 = 0, c1 = 0;            // this rank's columns of the matrix variable (all of them on one GPU), multiples of 16
  // P: a batch of row-major blocks P_k[c0:, c0:c1], (m - c0) rows x ldp.  It holds only the owned columns (leading dimension
  // = their count rounded to 16), so a rank with a narrow range takes many more matrices per launch: the triangular products
  // end every launch with a drain of unequal workgroups, and 8 ranks would otherwise pay 16 of them on a fraction of the work.
  long p_elems = 0, ldp = 0;     // doubles per matrix, leading dimension
  long P_cap = 0;                // matrices per launch of GEMM1'/GEMM2'
  bool t160 = false;             // GEMM3' on the 160 x 160 workgroup tile
  int ncls = 0, cls[2] = {0, 0}; // GemmDesc::tile_class of the GEMM3' launches, in order
  // the splits of GEMM3' go into ONE launch: split s walks chunks [kb[s], ke[s]) with slab weight 1 (diagonal 16-blocks) or
  // 2 (strictly-lower blocks)
  int nslab = 0, kb[64], ke[64];
  SlabWeights sw;
  // this rank's share of the USEFUL work of the three GEMMs (bench.py prices the roofline with them; 1 on one GPU)
  double gemm1_share = 0.0, gemm2_share = 0.0, gemm3_share = 0.0;
};

// pcap_hint: the batch chol_path_applicable found room for
inline CholPlan plan_chol(int m, int nd, int rank, int world, long pcap_hint, const CholPlanOpts& o) {
  CholPlan p;
  const int S = packed_S(m);
  const long Kp = packed_total_elems(m), Kd = packed_diag_elems(m);
  p.idle = !col_runs(m, nd, rank, world, &p.c0, &p.c1);
  const int c0 = p.c0, c1 = p.c1;
  p.P_cap = pcap_hint;
  if (!p.idle) {
    p.ldp = ((c1 - c0) + 15) & ~15;
    p.p_elems = (long)(m - c0) * p.ldp;
  }
  if (p.p_elems > 0) {
    long cap = o.p_batch > 0 ? o.p_batch : std::max<long>(16, (long)(8.6e9 / ((double)p.p_elems * 8.0)));
    // one GPU: 256 matrices per launch, or what chol_path_applicable found room for (up to 1024)
    if (o.p_batch <= 0 && world <= 1) cap = std::max<long>(std::min<long>(cap, 256), std::min<long>(pcap_hint, 1024));
    p.P_cap = std::min<long>(std::min<long>(cap, nd), 32768);
  }
  // workgroup tile of GEMM3': 128 x 128, or 160 x 160 (gemm_f64_kseg_lds_kernel<true, 5>: 0.8 of the panel bytes per
  // flop, 100 MFMAs per wave between barriers) where its grid covers the lower triangle with > 5 % less area -- at
  // C4 (4000 = 25 x 160 = 31.25 x 128) both run within 2 % of each other, 128 ahead on most boxes: the kernel is bound
  // by the MFMA pipe at the clock it is left, not by its panel traffic (option "gemm3_tile": 0 auto, 128, 160)
  auto tri_area = [&](long ts) { const long tt = (nd + ts - 1) / ts; return tt * (tt + 1) / 2 * ts * ts; };
  p.t160 = o.gemm3_tile == 160 || (o.gemm3_tile == 0 && nd >= 320 && (double)tri_area(160) < 0.95 * (double)tri_area(128));
  const int TS3 = p.t160 ? 160 : 128;
  const int tM = (nd + TS3 - 1) / TS3;
  long tiles = (long)tM * (tM + 1) / 2;
  // GEMM3' runs as two launches: the regular tiles -- all equally long, lock-step through K -- and then the tiles
  // with blocks to skip (diagonal tiles: blocks above the diagonal; the last tile row when nd % 128 != 0).  The
  // split-K factor is chosen for the regular launch (the bulk of the work).
  const bool two_launches = !o.gemm_no_skip && tM > 2;
  if (two_launches) tiles -= tM + ((nd % TS3) ? tM - 1 : 0);
  // chunk ranges of the columns: the diagonal chunks [c0, c1) and the strictly-lower ones [o0, o1)
  const long o0 = (Kd + packed_off_base(c0, S)) / 16, o1 = (Kd + packed_off_base(c1, S)) / 16;
  const long nd_ = c1 - c0, no_ = o1 - o0, chunks = nd_ + no_;
  {   // column c of P_k costs 2 (m - c)^2 flop and column c of At_k (m - c)^2, GEMM3' its packed length
    double all = 0.0, own = 0.0;
    for (int cc = 0; cc < m; ++cc) {
      const double w = (double)(m - cc) * (m - cc);
      all += w;
      if (cc >= c0 && cc < c1) own += w;
    }
    p.gemm1_share = p.gemm2_share = own / all;
    p.gemm3_share = (double)chunks / (double)(Kp / 16);
  }
  if (chunks == 0) return p;
  // split-K (pick_ksplit_short): every split >= 256 K-chunks where the range allows; at least two splits, one per weight
  int ksplit = pick_ksplit_short(tiles, (int)std::min<long>(64, std::max<long>(1, chunks / 8)), 64, chunks, 256, (double)nd * nd);
  if (o.gemm3_ksplit > 0) ksplit = std::min(64, o.gemm3_ksplit);
  const int ks = std::max(ksplit, 2);
  int nsd = ks;                  // splits of the diagonal chunks, by their share of the range
  if (no_ > 0) nsd = std::max(1, std::min(ks - 1, (int)((double)ks * (double)nd_ / (double)chunks + 0.5)));
  const int nso = ks - nsd;
  for (int i = 0; i < nsd; ++i, ++p.nslab) {
    p.sw.w[p.nslab] = 1.0f;
    p.kb[p.nslab] = (int)(c0 + nd_ * i / nsd);
    p.ke[p.nslab] = (int)(c0 + nd_ * (i + 1) / nsd);
  }
  for (int i = 0; i < nso; ++i, ++p.nslab) {
    p.sw.w[p.nslab] = 2.0f;
    p.kb[p.nslab] = (int)(o0 + no_ * i / nso);
    p.ke[p.nslab] = (int)(o0 + no_ * (i + 1) / nso);
  }
  // regular tiles of every split first, the tiles with skipped blocks last, in one launch (tile_class 3); measurement
  // (gemm3_sched 0): the two classes as two launches; a last tile row of height 128 + nd % 128 <= 160 instead of a row of
  // edge tiles, as a second launch (gemm_f64.hip, tile_class 4 / 5; option "gemm3_strip")
  if (two_launches && o.gemm3_sched == 0) {
    p.ncls = 2; p.cls[0] = 1; p.cls[1] = 2;
  } else if (two_launches && !p.t160 && o.gemm3_strip && nd >= 288 && nd % 128 > 0 && nd % 128 <= 32) {
    p.ncls = 2; p.cls[0] = 4; p.cls[1] = 5;
  } else {
    p.ncls = 1; p.cls[0] = two_launches ? 3 : 0;
  }
  return p;
}

}  // namespace lrn
