// Host-side plan of the rank-class route of the rank-k Schur assembly (option "lowrank_ragged", raggedops.hip): the constraints
// of a block grouped by rank class, the compacted column layout and the tile list of the one launch.  Pure functions of the
// factor weights -- no context, no HIP runtime call -- in the style of schur_plan.h.  Python specification: model.ragged_plan;
// the column -> group map and the K-chunks of the data operators (option "ragged_ops"): model.ragged_columns, ragged_chunks;
// the H index -> group map of the cross terms and of ts of H_alpha (options "ragged_cross", "ragged_ts"): ragged_columns' hg.
//
// Rank r_j of constraint j = its factor columns of non-zero weight; class c_j = the smallest of {1, 2, 4, 8, 16, 32, 64} >= r_j
// (32 and 64 occur in a wide block only, khat > 16 under option "lowrank_wide").  A constraint of rank 0 (a stored row of a
// hybrid block, a purely diagonal row, an empty constraint) has no group.  Classes are laid out in descending order (64, 32,
// 16, 8, 4, 2, 1), the groups of a class in increasing H index; group g holds the weighted columns of its constraint in their
// original order, then weight-0 padding up to c_j columns.  An empty class has an empty segment and no tile: a block without
// ranks above 16 has the columns, the group order and the tile list it had with five classes.
#pragma once
#include <vector>

namespace lrn {

#if defined(__HIPCC__)
#define RG_HD __host__ __device__
#else
#define RG_HD
#endif
static constexpr int RG_NCLS = 7;                       // classes 64, 32, 16, 8, 4, 2, 1 in layout order
static constexpr int RG_TILE = 64;                      // tile side of ragged_blocksum_kernel: every class size divides it
RG_HD inline int ragged_class_size(int ci) { return 64 >> ci; }

// One workgroup of ragged_blocksum_kernel: rows [r0, r1) x columns [c0, c1) of T = U_c' B_c (at most 64 x 64; r1, c1 = the tile
// end or the segment end), whose ka x kb blocks belong to the groups gi0 + (row - r0) / ka and gj0 + (col - c0) / kb.
// diag: a diagonal tile of a class with itself -- blocks with gi < gj are left to their mirror images
struct RaggedTile {
  int r0, r1, c0, c1;
  int gi0, gj0;
  int ka, kb;
  int diag;
  int pad_[3];
};

struct RaggedPlan {
  long Rc = 0;                                          // compacted columns, sum of c_j
  int ncls = 0;                                         // classes present
  long seg0[RG_NCLS] = {}, seg1[RG_NCLS] = {};          // columns of class ci: [seg0, seg1)
  int grp0[RG_NCLS] = {};                               // first group of class ci
  std::vector<int> gh;                                  // group -> H index
  std::vector<int> hg;                                  // H index -> group, -1 for a constraint of rank 0 (the inverse of gh)
  std::vector<int> cg;                                  // compacted column -> group (option "ragged_ops": the data operators)
  std::vector<long> src;                                // compacted column -> padded column h khat + p, -1 for padding
  std::vector<double> wc;                               // weight of the compacted column (0 in the padding)
  std::vector<RaggedTile> tiles;
};

// class index (0: 64 .. 6: 1) of a rank 1 .. 64
inline int ragged_class_of(int r) {
  int ci = RG_NCLS - 1;
  while (ragged_class_size(ci) < r) --ci;
  return ci;
}

// Rc alone (the cost model and the route decision read it): w = the nvar * khat weights in H index order
inline long ragged_cols(const double* w, int nvar, int khat) {
  long Rc = 0;
  for (long h = 0; h < nvar; ++h) {
    int r = 0;
    for (int p = 0; p < khat; ++p) r += w[h * khat + p] != 0.0;
    if (r > 0) Rc += ragged_class_size(ragged_class_of(r));
  }
  return Rc;
}

// ---- the data operators on the compacted columns (option "ragged_ops", raggedops.hip)
// K-chunks of the column range [0, Rc) walked in steps of RG_KSTEP columns: nsteps = ceil(Rc / 16), ks clamped to
// [1, min(16, nsteps)], chunk s = the steps [s nsteps / ks, (s + 1) nsteps / ks) -- uneven where ks does not divide nsteps,
// the last step a tail where 16 does not divide Rc.  Every step belongs to exactly one chunk.
static constexpr int RG_KSTEP = 16;
static constexpr int RG_MAX_CHUNKS = 16;
RG_HD inline long ragged_steps(long Rc) { return (Rc + RG_KSTEP - 1) / RG_KSTEP; }
inline int ragged_clamp_chunks(long Rc, int ks) {
  const long ns = ragged_steps(Rc), hi = ns < RG_MAX_CHUNKS ? ns : RG_MAX_CHUNKS;
  return ks < 1 || hi < 1 ? 1 : (int)(ks > hi ? hi : ks);
}
// columns [*c0, *c1) of chunk s of ks (ks already clamped)
RG_HD inline void ragged_chunk_cols(long Rc, int ks, int s, long* c0, long* c1) {
  const long ns = ragged_steps(Rc);
  const long s0 = (long)s * ns / ks, s1 = (long)(s + 1) * ns / ks;
  *c0 = s0 * RG_KSTEP;
  *c1 = s1 * RG_KSTEP < Rc ? s1 * RG_KSTEP : Rc;
}

// tiles of the layout: for every class pair (A, B), A at or before B, the 64 x 64 tiles of seg_A x seg_B anchored at the
// segment starts -- all of them for A != B, those with tile row >= tile column for A == B
inline long ragged_tile_count(const long* seg0, const long* seg1) {
  long nt = 0;
  for (int a = 0; a < RG_NCLS; ++a) {
    const long ta = (seg1[a] - seg0[a] + RG_TILE - 1) / RG_TILE;
    nt += ta * (ta + 1) / 2;
    for (int bb = a + 1; bb < RG_NCLS; ++bb) nt += ta * ((seg1[bb] - seg0[bb] + RG_TILE - 1) / RG_TILE);
  }
  return nt;
}

inline RaggedPlan plan_ragged(const double* w, int nvar, int khat, bool with_tiles = true) {
  RaggedPlan p;
  std::vector<int> cls(nvar, -1);
  long cnt[RG_NCLS] = {};
  for (long h = 0; h < nvar; ++h) {
    int r = 0;
    for (int q = 0; q < khat; ++q) r += w[h * khat + q] != 0.0;
    if (r == 0) continue;
    cls[h] = ragged_class_of(r);
    cnt[cls[h]] += 1;
  }
  long col = 0;
  int grp = 0;
  for (int ci = 0; ci < RG_NCLS; ++ci) {
    p.seg0[ci] = col;
    p.grp0[ci] = grp;
    col += cnt[ci] * ragged_class_size(ci);
    grp += (int)cnt[ci];
    p.seg1[ci] = col;
    if (cnt[ci] > 0) p.ncls += 1;
  }
  p.Rc = col;
  p.gh.reserve(grp);
  p.hg.assign(nvar, -1);
  p.src.assign(p.Rc, -1);
  p.wc.assign(p.Rc, 0.0);
  p.cg.assign(p.Rc, 0);
  for (int ci = 0; ci < RG_NCLS; ++ci) {
    long at = p.seg0[ci];
    for (long h = 0; h < nvar; ++h) {
      if (cls[h] != ci) continue;
      for (int q = 0; q < ragged_class_size(ci); ++q) p.cg[at + q] = (int)p.gh.size();
      p.hg[h] = (int)p.gh.size();
      p.gh.push_back((int)h);
      long k = at;
      for (int q = 0; q < khat; ++q)
        if (w[h * khat + q] != 0.0) { p.src[k] = h * khat + q; p.wc[k] = w[h * khat + q]; ++k; }
      at += ragged_class_size(ci);
    }
  }
  if (!with_tiles) return p;
  p.tiles.reserve((size_t)ragged_tile_count(p.seg0, p.seg1));
  for (int a = 0; a < RG_NCLS; ++a)
    for (int bb = a; bb < RG_NCLS; ++bb) {
      const int ka = ragged_class_size(a), kb = ragged_class_size(bb);
      const long ta = (p.seg1[a] - p.seg0[a] + RG_TILE - 1) / RG_TILE, tb = (p.seg1[bb] - p.seg0[bb] + RG_TILE - 1) / RG_TILE;
      for (long ti = 0; ti < ta; ++ti)
        for (long tj = 0; tj < (a == bb ? ti + 1 : tb); ++tj) {
          RaggedTile t;
          t.r0 = (int)(p.seg0[a] + ti * RG_TILE);
          t.r1 = (int)(t.r0 + RG_TILE < p.seg1[a] ? t.r0 + RG_TILE : p.seg1[a]);
          t.c0 = (int)(p.seg0[bb] + tj * RG_TILE);
          t.c1 = (int)(t.c0 + RG_TILE < p.seg1[bb] ? t.c0 + RG_TILE : p.seg1[bb]);
          t.gi0 = p.grp0[a] + (int)(ti * RG_TILE / ka);
          t.gj0 = p.grp0[bb] + (int)(tj * RG_TILE / kb);
          t.ka = ka;
          t.kb = kb;
          t.diag = (a == bb && ti == tj) ? 1 : 0;
          t.pad_[0] = t.pad_[1] = t.pad_[2] = 0;
          p.tiles.push_back(t);
        }
    }
  return p;
}

}  // namespace lrn
