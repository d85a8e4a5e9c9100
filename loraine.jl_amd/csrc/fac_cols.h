// Which columns of the dense factors belong to a constraint: the one question the two column layouts of a factored block answer
// differently.  Every per-constraint kernel of the factor form (fac_coldot_kernel of dataops.hip, fac_quadform_reduce_kernel and
// fac_ts_kernel of facops.hip, fac_cross_kernel and fac_cross_coldot_kernel of schur_factored.hip) is one body, a template on
// the layout, instantiated for both:
//   PaddedCols   Vd (msz x nvar khat): the constraint with H index h owns the columns [h khat, h khat + khat).  Every H index has
//                columns; those beyond its rank -- all khat of a constraint of rank 0 -- have weight 0 and the kernels skip them.
//   CompactCols  Vc (msz x Rc, ragged_plan.h): one group of class-size columns per constraint of rank > 0, the classes laid out
//                64 .. 1; group g belongs to H index gh[g], H index h to group hg[h], none (hg[h] < 0) at rank 0.
// A layout is read in two ways:
//   by unit     grid index u -> (span, count) by unit() -- the data operators -- or pos_unit() -- the cross terms of a hybrid
//               block; the H index of the unit by unit_h().  Padded: unit u is H index u, and for the cross terms the factored
//               position p_f + u, its H index through the position -> H index map hidx the kernel hands in.  Compact: unit u is
//               group u in both.  unit() / pos_unit() return false past the last unit
//   by H index  of_h(): (span, count) of the constraint with H index h, false where it has no columns -- ts of H_alpha
// and col(span, p) is column p < count of a span.
// Both are trivially copyable and travel as one kernel argument.
#pragma once
#include "ctx.h"
#include "ragged_plan.h"

namespace lrn {

struct RaggedSegs { long seg0[RG_NCLS]; int grp0[RG_NCLS + 1]; };

// first column and class size of group g (g < grp0[RG_NCLS])
__device__ __forceinline__ long ragged_group_col(const RaggedSegs& sg, int g, int* cj) {
  int ci = 0;
  while (ci < RG_NCLS - 1 && g >= sg.grp0[ci + 1]) ++ci;
  *cj = ragged_class_size(ci);
  return sg.seg0[ci] + (long)(g - sg.grp0[ci]) * ragged_class_size(ci);
}

struct PaddedCols {
  int kh, nvar, p_f;       // p_f: first factored position (the cross terms)
  typedef int Span;        // the H index h: column p is h kh + p
  __device__ __forceinline__ long col(Span h, int p) const { return (long)h * kh + p; }
  __device__ __forceinline__ bool of_h(int h, Span* s, int* cnt) const {
    *s = h;
    *cnt = kh;
    return true;
  }
  __device__ __forceinline__ bool unit(int u, Span* s, int* cnt) const { return u < nvar && of_h(u, s, cnt); }
  __device__ __forceinline__ int unit_h(int, Span h) const { return h; }
  __device__ __forceinline__ bool pos_unit(int u, const int* hidx, Span* s, int* cnt) const {
    return p_f + u < nvar && of_h(hidx[p_f + u], s, cnt);
  }
};

struct CompactCols {
  RaggedSegs sg;
  const int* gh;           // group -> H index
  const int* hg;           // H index -> group, -1: none
  typedef long Span;       // the first column of the group
  __device__ __forceinline__ long col(Span c0, int p) const { return c0 + p; }
  __device__ __forceinline__ bool unit(int g, Span* s, int* cnt) const {
    if (g >= sg.grp0[RG_NCLS]) return false;
    *s = ragged_group_col(sg, g, cnt);
    return true;
  }
  __device__ __forceinline__ int unit_h(int g, Span) const { return gh[g]; }
  __device__ __forceinline__ bool pos_unit(int g, const int*, Span* s, int* cnt) const { return unit(g, s, cnt); }
  __device__ __forceinline__ bool of_h(int h, Span* s, int* cnt) const {
    const int g = hg[h];
    if (g < 0) return false;
    *s = ragged_group_col(sg, g, cnt);
    return true;
  }
};

// host side: the dense factors of block b in one layout -- V (msz x R), the column weights and the units of a by-unit launch.
// The compact view needs ragged_setup(c, b) first
struct FacCols {
  bool compact;
  const double* V;
  const double* w;
  long R;
  int nunit, npos;         // units of the data operators / of the cross terms
};
inline FacCols fac_cols(const lrn_ctx* c, const LmiBlock& b, bool compact) {
  if (compact) return {true, b.Vc.as<double>(), b.rg_wc.as<double>(), b.rg_Rc, b.rg_grp0[RG_NCLS], b.rg_grp0[RG_NCLS]};
  return {false, b.Vd.as<double>(), b.v_w.as<double>(), (long)c->nvar * b.lr_khat, c->nvar, c->nvar - b.npos_nz};
}
inline PaddedCols padded_cols(const lrn_ctx* c, const LmiBlock& b) {
  return {b.lr_khat, c->nvar, b.npos_nz};
}
inline CompactCols compact_cols(const LmiBlock& b) {
  CompactCols l;
  for (int ci = 0; ci < RG_NCLS; ++ci) l.sg.seg0[ci] = b.rg_seg0[ci];
  for (int ci = 0; ci <= RG_NCLS; ++ci) l.sg.grp0[ci] = b.rg_grp0[ci];
  l.gh = b.rg_gh.as<int>();
  l.hg = b.rg_hg.as<int>();
  return l;
}
// f(layout) with the device-side layout of the view: the one place a driver chooses between the two instantiations of a kernel
template <class F>
inline void with_layout(const lrn_ctx* c, const LmiBlock& b, const FacCols& v, F&& f) {
  if (v.compact) f(compact_cols(b));
  else f(padded_cols(c, b));
}

}  // namespace lrn
