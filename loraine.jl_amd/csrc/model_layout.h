// Host-side layout of an uploaded model (model.hip, model_factored.hip): every array lrn_upload_model, lrn_upload_lowrank and
// lrn_upload_diag put on the device, as plain vectors filled from the caller's CSC arrays, and the argument checks that need
// host data only.  Pure functions -- no context, no HIP header, no allocator state; the one device-dependent input, the free
// memory the dense prefix may use, is an argument -- so that what every kernel reads is pinned without a GPU
// (lrn_dbg_model_layout, lrn_dbg_factor_layout, tests/test_model_layout_cpu.py).  The arrays are described where they are
// kept (ctx.h).
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace lrn {

// a failed check: the code and the message text the entry point hands to set_error (code 0: none)
struct LayoutError {
  int code = 0;
  std::string msg;
  explicit operator bool() const { return code != 0; }
};
constexpr int LAYOUT_ERR_ARG = -1, LAYOUT_ERR_STATE = -3;      // (LRN_ERR_ARG, LRN_ERR_STATE of lrn_common.h)

inline LayoutError layout_error(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return {code, buf};
}

// ---------------------------------------------------------------- one LMI block from AA, sigmaA, qA
struct BlockLayout {
  std::vector<int> sigma, ipos;      // position <-> constraint
  std::vector<long> nnz;             // per position, stored zeros not counted
  int qA = 0, npos_nz = 0, nd = 0, q_wave = 0;
  std::vector<long> ent_ptr;         // entry lists in position order, value = -AA
  std::vector<int> ent_r, ent_c;
  std::vector<double> ent_v;
  std::vector<int> hidx;             // position -> index of the Schur matrix
  std::vector<long> cq_q, cq_ptr;    // stored columns of AA restricted to the non-dense constraints
  std::vector<int> cq_j;
  std::vector<double> cq_v;
  bool sp_ok = false;                // pattern of mat(AA'x): kept when no constraint is dense and the pattern is symmetric
  std::vector<long> pc_ptr;
  std::vector<int> pc_r, pc_t, ent_t, sp_long_cols;
  // local route of the sparse owners (block_local, localops.hip): owners [loc_lo, loc_hi); for the positions p >= loc_lo of a
  // non-empty range the support S_p (ascending) at loc_sup[loc_sptr[p] ..) and A_p[S_p, S_p] (column-major, unpadded, value =
  // ent_v) at loc_a[loc_aptr[p] ..); positions below loc_lo, and every position of an empty range, have empty lists
  int loc_lo = 0, loc_hi = 0;
  std::vector<long> loc_sptr, loc_aptr;
  std::vector<int> loc_sup;
  std::vector<double> loc_a;
  // long route of the sparse owners (block_long, longops.hip): the eligible owners are [nd, lg_hi).  For position nd + k the
  // ascending distinct row indices R at lg_rows[lg_rptr[k] ..), and for the g-th row of lg_rows its entries in ascending column
  // order at lg_ec / lg_ev[lg_eptr[g] ..) (value = ent_v); all five lists are empty when lg_hi == nd
  int lg_hi = 0;
  std::vector<long> lg_rptr, lg_eptr;
  std::vector<int> lg_rows, lg_ec;
  std::vector<double> lg_ev;
  long nent() const { return (long)ent_r.size(); }
  long ncq() const { return (long)cq_q.size(); }
};

constexpr int LOCAL_SUPPORT_MAX = 32;      // side of the largest support the local route takes: two MFMA tiles of 16
constexpr int PAIR_LOCAL_MIN = 36;         // default of option pair_local_min: the measured cross-over, a dense support of 6

// Defaults of the options pair_long_min and pair_long_split, both measured: the smallest diag(a) row from which
// the route beats the pair kernels by more than both spreads beside 400 tiny partners, and the fastest slice size on the identity
// self pair at msz 2000 (2^14 .. 2^16 give 61 .. 64 slices there and lie within each other's spread)
constexpr int PAIR_LONG_MIN = 64;
constexpr long PAIR_LONG_SPLIT = 1L << 15;
constexpr int LONG_SLICES_MAX = 64;

// slices of one pair of the long route's entry kernel: nnz_j * rho_i products above `split` are cut into
// ceil(work / split) slices of `*per` consecutive entries of the partner, at most LONG_SLICES_MAX; a function of (nnz_j, rho_i) alone
inline int long_slices(long nnz_j, long rho_i, long split, long* per) {
  const long work = nnz_j * rho_i;
  long ns = split > 0 ? (work + split - 1) / split : 1;
  ns = std::max(1L, std::min({ns, (long)LONG_SLICES_MAX, nnz_j}));
  *per = (nnz_j + ns - 1) / ns;
  return (int)((nnz_j + *per - 1) / *per);
}

// dense (MFMA) prefix by cost model: pair path cost nnz_p * suffix_nnz vs 3 m^3 GEMM work; dense_threshold >= 0 decides
// instead of the model; at most 0.55 of free_bytes go to the dense copies
inline int dense_prefix(const std::vector<long>& nnz, int qA, int npos_nz, int m, int nvar, double dense_threshold,
                        size_t free_bytes) {
  std::vector<double> suffix(nvar + 1, 0.0);
  for (int p = nvar - 1; p >= 0; --p) suffix[p] = suffix[p + 1] + (double)nnz[p];
  const long max_dense = (long)((double)free_bytes * 0.55 / ((double)m * m * 8.0));
  int nd = 0;
  for (int p = 0; p < qA && p < npos_nz; ++p) {
    bool dense;
    if (dense_threshold >= 0) {
      dense = (double)nnz[p] >= dense_threshold;
    } else {
      double pair_cost = (double)nnz[p] * suffix[p] / 1.0e11;
      double dense_cost = 3.0 * m * (double)m * m / 2.0e13 + (double)(nvar - p) * m * (double)m / 2.0e13 + 2e-5;
      dense = pair_cost > dense_cost;
    }
    if (!dense || nd >= max_dense) break;
    nd = p + 1;
  }
  return nd;
}

// sigma, ipos, nnz, qA, npos_nz and the entry lists.  cp, rv, nz: AA of the block, nvar x m^2 CSC, 1-based; sigma1: the
// block's column of sigmaA, 1-based
inline LayoutError block_entries(int m, int nvar, const int64_t* cp, const int64_t* rv, const double* nz,
                                 const int64_t* sigma1, int64_t qA, BlockLayout& L) {
  const long ncol = (long)m * m;
  std::vector<long> cnt(nvar, 0);
  for (long q = 0; q < ncol; ++q)
    for (long k = cp[q] - 1; k < cp[q + 1] - 1; ++k) {
      long j = rv[k] - 1;
      if (j < 0 || j >= nvar) return layout_error(LAYOUT_ERR_ARG, "AA rowval out of range");
      if (nz[k] != 0.0) cnt[j]++;
    }
  L.sigma.resize(nvar);
  L.ipos.assign(nvar, -1);
  L.nnz.resize(nvar);
  for (int p = 0; p < nvar; ++p) {
    long s = sigma1[p] - 1;
    if (s < 0 || s >= nvar || L.ipos[s] != -1) return layout_error(LAYOUT_ERR_ARG, "sigmaA is not a permutation");
    L.sigma[p] = (int)s;
    L.ipos[s] = p;
    L.nnz[p] = cnt[s];
  }
  for (int p = 1; p < nvar; ++p)
    if (L.nnz[p] > L.nnz[p - 1])
      return layout_error(LAYOUT_ERR_ARG, "sigmaA is not sorted by decreasing nnz (model.jl:159)");
  L.qA = (int)qA;
  if (L.qA < 0) L.qA = 0;
  if (L.qA > nvar) L.qA = nvar;
  L.npos_nz = 0;
  while (L.npos_nz < nvar && L.nnz[L.npos_nz] > 0) L.npos_nz++;
  L.ent_ptr.assign(nvar + 1, 0);
  for (int p = 0; p < nvar; ++p) L.ent_ptr[p + 1] = L.ent_ptr[p] + L.nnz[p];
  const long nent = L.ent_ptr[nvar];
  L.ent_r.resize(nent);
  L.ent_c.resize(nent);
  L.ent_v.resize(nent);
  std::vector<long> fill(L.ent_ptr.begin(), L.ent_ptr.end() - 1);
  for (long q = 0; q < ncol; ++q)
    for (long k = cp[q] - 1; k < cp[q + 1] - 1; ++k) {
      if (nz[k] == 0.0) continue;
      long w = fill[L.ipos[rv[k] - 1]]++;
      L.ent_r[w] = (int)(q % m);
      L.ent_c[w] = (int)(q / m);
      L.ent_v[w] = -nz[k];     // AA = -A  (model.jl:219)
    }
  return {};
}

// stored columns of AA restricted to the non-dense constraints (positions >= nd)
inline void block_stored_columns(int m, const int64_t* cp, const int64_t* rv, const double* nz, BlockLayout& L) {
  const long ncol = (long)m * m;
  L.cq_ptr.assign(1, 0);
  for (long q = 0; q < ncol; ++q) {
    long before = (long)L.cq_j.size();
    for (long k = cp[q] - 1; k < cp[q + 1] - 1; ++k) {
      if (nz[k] == 0.0) continue;
      long j = rv[k] - 1;
      if (L.ipos[j] < L.nd) continue;
      L.cq_j.push_back((int)j);
      L.cq_v.push_back(nz[k]);
    }
    if ((long)L.cq_j.size() > before) { L.cq_q.push_back(q); L.cq_ptr.push_back((long)L.cq_j.size()); }
  }
}

// pattern of mat(AA'x) for the sparse-aware mat-vec: the stored columns by pattern column, the stored column that holds
// the transposed entry, the stored column of every constraint entry
inline void block_pattern(int m, BlockLayout& L) {
  const long nq = L.ncq(), nent = L.nent();
  L.sp_ok = false;
  if (L.nd != 0 || nq <= 0 || nq >= 2000000000L || nent >= 2000000000L) return;
  std::vector<long> pcp(m + 1, 0);
  std::vector<int> pr(nq), pt(nq), et(nent);
  for (long t = 0; t < nq; ++t) {
    pr[t] = (int)(L.cq_q[t] % m);
    pcp[L.cq_q[t] / m + 1]++;
  }
  for (long q = 0; q < m; ++q) pcp[q + 1] += pcp[q];
  auto stored_column = [&](long key, int* out) {
    auto it = std::lower_bound(L.cq_q.begin(), L.cq_q.end(), key);
    if (it == L.cq_q.end() || *it != key) return false;
    *out = (int)(it - L.cq_q.begin());
    return true;
  };
  for (long t = 0; t < nq; ++t)
    if (!stored_column(L.cq_q[t] / m + (L.cq_q[t] % m) * m, &pt[t])) return;       // (col, row) swapped
  for (long e = 0; e < nent; ++e)
    if (!stored_column((long)L.ent_r[e] + (long)L.ent_c[e] * m, &et[e])) return;
  L.sp_ok = true;
  L.pc_ptr.swap(pcp);
  L.pc_r.swap(pr);
  L.pc_t.swap(pt);
  L.ent_t.swap(et);
  // columns of the pattern with many entries (sp_wm_long_kernel, dataops.hip)
  for (long q = 0; q < m; ++q)
    if (L.pc_ptr[q + 1] - L.pc_ptr[q] > 64) L.sp_long_cols.push_back((int)q);
}

// the local range of the sparse owners and its lists (option pair_local, localops.hip): tr(A_i W A_j W) from the dense
// A_p[S_p, S_p] on the supports S_p.  An owner meets every partner j >= i up to npos_nz, so all of them need a support of
// at most LOCAL_SUPPORT_MAX indices.
//   loc_hi: the first position of [nd, q_wave) with fewer than pair_local_min entries -- positions are sorted by decreasing
//           nnz, one scan; below that many entries the pair kernel's nnz_i nnz_j terms are the cheaper route
//   loc_lo: the smallest position >= nd from which every support up to loc_hi fits -- one scan down from loc_hi
// The tail [loc_hi, npos_nz): a symmetric constraint has an entry in every row of its support, so s <= nnz < pair_local_min,
// which is within the bound up to pair_local_min = 33 -- not for the default 36 (35 entries can touch 35 indices), not for an
// unsymmetric entry list (an off-diagonal entry without its twin: s <= 2 nnz), not for a larger setting.  So the tail is
// scanned whatever the option says -- it is linear in its entries -- and one support above the bound behind loc_hi leaves no
// owner whose partners all fit: the range is empty (loc_lo = loc_hi).  Nothing is scanned when no sparse owner reaches pair_local_min entries.
inline void block_local(int m, int pair_local_min, BlockLayout& L) {
  const int nvar = (int)L.nnz.size();
  L.loc_sptr.assign(nvar + 1, 0);
  L.loc_aptr.assign(nvar + 1, 0);
  L.loc_sup.clear();
  L.loc_a.clear();
  int hi = L.nd;
  while (hi < L.q_wave && L.nnz[hi] >= pair_local_min) ++hi;
  L.loc_lo = L.loc_hi = hi;
  if (hi == L.nd) return;
  std::vector<int> mark(m, -1);
  auto fits = [&](int p) {      // at most LOCAL_SUPPORT_MAX distinct indices among the rows and columns of position p
    int s = 0;
    for (long e = L.ent_ptr[p]; e < L.ent_ptr[p + 1] && s <= LOCAL_SUPPORT_MAX; ++e)
      for (int idx : {L.ent_r[e], L.ent_c[e]})
        if (mark[idx] != p) { mark[idx] = p; ++s; }
    return s <= LOCAL_SUPPORT_MAX;
  };
  for (int p = hi; p < L.npos_nz; ++p)
    if (!fits(p)) return;
  int lo = hi;
  while (lo > L.nd && fits(lo - 1)) --lo;
  L.loc_lo = lo;
  if (lo == hi) return;
  std::vector<int> slot(m, 0);
  for (int p = lo; p < L.npos_nz; ++p) {
    const size_t s0 = L.loc_sup.size();
    for (long e = L.ent_ptr[p]; e < L.ent_ptr[p + 1]; ++e)
      for (int idx : {L.ent_r[e], L.ent_c[e]})
        if (mark[idx] != -2 - p) { mark[idx] = -2 - p; L.loc_sup.push_back(idx); }
    std::sort(L.loc_sup.begin() + (long)s0, L.loc_sup.end());
    const int s = (int)(L.loc_sup.size() - s0);
    for (int a = 0; a < s; ++a) slot[L.loc_sup[s0 + a]] = a;
    const size_t a0 = L.loc_a.size();
    L.loc_a.resize(a0 + (size_t)s * s, 0.0);
    for (long e = L.ent_ptr[p]; e < L.ent_ptr[p + 1]; ++e) L.loc_a[a0 + slot[L.ent_r[e]] + (size_t)slot[L.ent_c[e]] * s] = L.ent_v[e];
    L.loc_sptr[p + 1] = (long)L.loc_sup.size();
    L.loc_aptr[p + 1] = (long)L.loc_a.size();
  }
  for (int p = L.npos_nz; p < nvar; ++p) {
    L.loc_sptr[p + 1] = L.loc_sptr[p];
    L.loc_aptr[p + 1] = L.loc_aptr[p];
  }
}

// the eligible owners of the long route and their lists (option pair_long, longops.hip): H_ij from Z_i = (A_i W) on the
// distinct rows R_i of A_i, nnz_i msz flop once per owner and nnz_j |R_i| per pair.  lg_hi: the first position of [nd, q_wave)
// with fewer than pair_long_min entries -- positions are sorted by decreasing nnz, so the owners are a prefix.  The entries of
// a position come ordered by (column, row); a stable sort by row gives every row its entries in ascending column order.
// Nothing is scanned or built when no sparse owner reaches pair_long_min entries.
inline void block_long(int m, int pair_long_min, BlockLayout& L) {
  (void)m;
  int hi = L.nd;
  while (hi < L.q_wave && L.nnz[hi] >= pair_long_min) ++hi;
  L.lg_hi = hi;
  if (hi == L.nd) return;
  L.lg_rptr.assign(1, 0);
  L.lg_eptr.assign(1, 0);
  std::vector<long> order;
  for (int p = L.nd; p < hi; ++p) {
    order.resize((size_t)(L.ent_ptr[p + 1] - L.ent_ptr[p]));
    for (size_t k = 0; k < order.size(); ++k) order[k] = L.ent_ptr[p] + (long)k;
    std::stable_sort(order.begin(), order.end(), [&](long a, long b) { return L.ent_r[a] < L.ent_r[b]; });
    for (size_t k = 0; k < order.size(); ++k) {
      const long e = order[k];
      if (k > 0 && L.ent_r[e] != L.ent_r[order[k - 1]]) L.lg_eptr.push_back((long)L.lg_ec.size());
      if (k == 0 || L.ent_r[e] != L.ent_r[order[k - 1]]) L.lg_rows.push_back(L.ent_r[e]);
      L.lg_ec.push_back(L.ent_c[e]);
      L.lg_ev.push_back(L.ent_v[e]);
    }
    L.lg_eptr.push_back((long)L.lg_ec.size());
    L.lg_rptr.push_back((long)L.lg_rows.size());
  }
}

// the whole block.  pos_space: the Schur matrix is kept in position space (nlmi == 1); free_bytes: the free device memory
inline LayoutError block_layout(int m, int nvar, const int64_t* cp, const int64_t* rv, const double* nz, const int64_t* sigma1,
                                int64_t qA, bool pos_space, double dense_threshold, size_t free_bytes, BlockLayout& L,
                                int pair_local_min = PAIR_LOCAL_MIN, int pair_long_min = PAIR_LONG_MIN) {
  L = BlockLayout();
  if (LayoutError e = block_entries(m, nvar, cp, rv, nz, sigma1, qA, L)) return e;
  L.nd = dense_prefix(L.nnz, L.qA, L.npos_nz, m, nvar, dense_threshold, free_bytes);
  L.q_wave = L.nd;
  while (L.q_wave < L.npos_nz && L.nnz[L.q_wave] > 4) L.q_wave++;
  block_local(m, pair_local_min, L);
  block_long(m, pair_long_min, L);
  block_stored_columns(m, cp, rv, nz, L);
  block_pattern(m, L);
  L.hidx.resize(nvar);
  for (int p = 0; p < nvar; ++p) L.hidx[p] = pos_space ? p : L.sigma[p];
  return {};
}

// ---------------------------------------------------------------- rank-one factors (datarank = -1)
// B (nvar x m CSC, 1-based) as CSR with the rows in H index order
struct RankOneLayout {
  std::vector<long> b_ptr;
  std::vector<int> b_col;
  std::vector<double> b_val;
};

inline void rank_one_layout(int m, int nvar, const int64_t* bc, const int64_t* br, const double* bv, const std::vector<int>& ipos,
                            bool pos_space, RankOneLayout& R) {
  std::vector<long> bcnt(nvar, 0);
  for (long q = 0; q < m; ++q)
    for (long k = bc[q] - 1; k < bc[q + 1] - 1; ++k) bcnt[br[k] - 1]++;
  // row index in H space
  std::vector<int> hrow(nvar);
  for (int j = 0; j < nvar; ++j) hrow[j] = pos_space ? ipos[j] : j;
  std::vector<long> cnt_h(nvar, 0);
  for (int j = 0; j < nvar; ++j) cnt_h[hrow[j]] = bcnt[j];
  R.b_ptr.assign(nvar + 1, 0);
  for (int h = 0; h < nvar; ++h) R.b_ptr[h + 1] = R.b_ptr[h] + cnt_h[h];
  const long bnnz = R.b_ptr[nvar];
  R.b_col.resize(bnnz);
  R.b_val.resize(bnnz);
  std::vector<long> bf(R.b_ptr.begin(), R.b_ptr.end() - 1);
  for (long q = 0; q < m; ++q)
    for (long k = bc[q] - 1; k < bc[q + 1] - 1; ++k) {
      long w = bf[hrow[br[k] - 1]]++;
      R.b_col[w] = (int)q;
      R.b_val[w] = bv[k];
    }
}

// ---------------------------------------------------------------- linear block C_lin (nvar x nlin CSC, 1-based)
struct LinearLayout {
  std::vector<long> cl_ptr;
  std::vector<int> cl_row, cl_rown;          // Schur-matrix index, natural row
  // gather lists: every lower-triangle target (ri >= rj) of C_lin diag(xs) C_lin' with its (l, C_il C_jl)
  std::vector<int> lp_r, lp_c, lp_l;
  std::vector<long> lp_ptr;
  std::vector<double> lp_w;
  // C_lin by natural rows
  std::vector<long> cr_ptr;
  std::vector<int> cr_col;
  std::vector<double> cr_val;
};

// ipos0: constraint -> position of block 0, read when pos_space
inline LayoutError linear_layout(int nvar, int nlin, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                                 const std::vector<int>* ipos0, bool pos_space, LinearLayout& L) {
  const long nn = colptr[nlin] - 1;
  L.cl_ptr.resize(nlin + 1);
  for (int l = 0; l <= nlin; ++l) L.cl_ptr[l] = colptr[l] - 1;
  const std::vector<long>& ptr = L.cl_ptr;
  std::vector<int>&row = L.cl_row, &rown = L.cl_rown;
  row.resize(nn);
  rown.resize(nn);
  for (long k = 0; k < nn; ++k) {
    long i = rowval[k] - 1;
    if (i < 0 || i >= nvar) return layout_error(LAYOUT_ERR_ARG, "C_lin rowval out of range");
    row[k] = pos_space ? (*ipos0)[i] : (int)i;
    rown[k] = (int)i;
  }
  struct Con { int r, c, l; double w; };
  std::vector<Con> cons;
  for (int l = 0; l < nlin; ++l)
    for (long a = ptr[l]; a < ptr[l + 1]; ++a)
      for (long bq = ptr[l]; bq < ptr[l + 1]; ++bq)
        if (row[a] >= row[bq]) cons.push_back({row[a], row[bq], l, nzval[a] * nzval[bq]});
  std::stable_sort(cons.begin(), cons.end(), [](const Con& x, const Con& y) { return x.c != y.c ? x.c < y.c : x.r < y.r; });
  L.lp_l.resize(cons.size());
  L.lp_w.resize(cons.size());
  L.lp_ptr.assign(1, 0);
  for (size_t k = 0; k < cons.size(); ++k) {
    if (k == 0 || cons[k].r != cons[k - 1].r || cons[k].c != cons[k - 1].c) {
      if (k > 0) L.lp_ptr.push_back((long)k);
      L.lp_r.push_back(cons[k].r); L.lp_c.push_back(cons[k].c);
    }
    L.lp_l[k] = cons[k].l; L.lp_w[k] = cons[k].w;
  }
  L.lp_ptr.push_back((long)cons.size());
  L.cr_ptr.assign(nvar + 1, 0);
  for (long k = 0; k < nn; ++k) L.cr_ptr[rown[k] + 1]++;
  for (int i = 0; i < nvar; ++i) L.cr_ptr[i + 1] += L.cr_ptr[i];
  std::vector<long> fill(L.cr_ptr.begin(), L.cr_ptr.end() - 1);
  L.cr_col.resize(nn);
  L.cr_val.resize(nn);
  for (int l = 0; l < nlin; ++l)
    for (long k = ptr[l]; k < ptr[l + 1]; ++k) {
      long w = fill[rown[k]]++;
      L.cr_col[w] = l; L.cr_val[w] = nzval[k];
    }
  return {};
}

// ---------------------------------------------------------------- rank-k factors (lrn_upload_lowrank)
// V: (nvar * khat) x m CSC, 1-based, row k * khat + p = column p of V_k; d[nvar * khat].  Kept as CSR by factor column
// h * khat + p in H index order, the weights in that order
struct LowrankLayout {
  std::vector<long> v_ptr;
  std::vector<int> v_col;
  std::vector<double> v_val, v_w;
};

inline LayoutError lowrank_check_size(int m, int nvar, int khat) {
  const long R = (long)nvar * khat;
  if ((double)R * m >= 9.0e18 / 8.0 || R > 0x7fffffffL) return layout_error(LAYOUT_ERR_ARG, "lrn_upload_lowrank: too many factor columns");
  return {};
}

inline LayoutError lowrank_check_colptr(int m, const int64_t* cp) {
  if (cp[0] != 1 || cp[m] - 1 < 0) return layout_error(LAYOUT_ERR_ARG, "lrn_upload_lowrank: colptr must start at 1 and not decrease");
  for (int q = 0; q < m; ++q)
    if (cp[q + 1] < cp[q]) return layout_error(LAYOUT_ERR_ARG, "lrn_upload_lowrank: colptr decreases at column %d", q);
  return {};
}

// cp has passed lowrank_check_colptr
inline LayoutError lowrank_layout(int m, int nvar, int khat, const int64_t* cp, const int64_t* rv, const double* nz, const double* d,
                                  const std::vector<int>& ipos, bool pos_space, LowrankLayout& L) {
  const long R = (long)nvar * khat, nnz = cp[m] - 1;
  // factor row k * khat + p -> U column hrow(k) * khat + p
  auto hcol = [&](long r) { const long k = r / khat; return (long)(pos_space ? ipos[k] : (int)k) * khat + r % khat; };
  L.v_ptr.assign(R + 1, 0);
  for (long e = 0; e < nnz; ++e) {
    if (rv[e] < 1 || rv[e] > R) return layout_error(LAYOUT_ERR_ARG, "lrn_upload_lowrank: rowval %lld out of range", (long long)rv[e]);
    L.v_ptr[hcol(rv[e] - 1) + 1]++;
  }
  for (long h = 0; h < R; ++h) L.v_ptr[h + 1] += L.v_ptr[h];
  L.v_col.resize(nnz);
  L.v_val.resize(nnz);
  std::vector<long> fill(L.v_ptr.begin(), L.v_ptr.end() - 1);
  for (int q = 0; q < m; ++q)
    for (long e = cp[q] - 1; e < cp[q + 1] - 1; ++e) {
      const long f = fill[hcol(rv[e] - 1)]++;
      L.v_col[f] = q;
      L.v_val[f] = nz[e];
    }
  L.v_w.resize(R);
  for (long r = 0; r < R; ++r) L.v_w[hcol(r)] = d[r];
  return {};
}

// A constraint of a factored block is stored (rows of AA) or factored, never both: the first stored position whose factor
// columns carry a non-zero weight, or -1.  w: the weights in H index order.
inline int stored_and_factored(bool pos_space, const std::vector<int>& sigma, int npos_nz, int khat, const double* w) {
  for (int p = 0; p < npos_nz; ++p) {
    const long h = pos_space ? p : sigma[p];
    for (int q = 0; q < khat; ++q)
      if (w[h * khat + q] != 0.0) return p;
  }
  return -1;
}

// Does a constraint with stored entries have no weighted factor column?  Then the factors do not represent the whole block
// (a materialised block some of whose constraints were given as matrices only): mode 1 assembles it from its entries.
inline bool factors_partial(bool pos_space, const std::vector<int>& sigma, int npos_nz, int khat, const double* w) {
  for (int p = 0; p < npos_nz; ++p) {
    const long h = pos_space ? p : sigma[p];
    bool any = false;
    for (int q = 0; q < khat && !any; ++q) any = w[h * khat + q] != 0.0;
    if (!any) return true;
  }
  return false;
}

// ---------------------------------------------------------------- diagonal rows (lrn_upload_diag)
// rows[s] (0-based constraint numbers): H index, constraint and position -> row (or -1) of every row.  The rows are factored
// positions -- a stored constraint carries its diagonal in its entries
struct DiagRowsLayout {
  std::vector<int> dg_h, dg_nat, dg_of_pos;
};

inline LayoutError diag_rows_layout(int nvar, int ilmi, int ns, const int64_t* rows, const std::vector<int>& ipos, int npos_nz,
                                    bool pos_space, DiagRowsLayout& L) {
  L.dg_h.resize(ns);
  L.dg_nat.resize(ns);
  L.dg_of_pos.assign(nvar, -1);
  for (int s = 0; s < ns; ++s) {
    const int64_t k = rows[s];
    if (k < 0 || k >= nvar) return layout_error(LAYOUT_ERR_ARG, "lrn_upload_diag: row %lld out of range (0 .. %d)", (long long)k, nvar - 1);
    const int pos = ipos[(int)k];
    if (L.dg_of_pos[pos] >= 0) return layout_error(LAYOUT_ERR_ARG, "lrn_upload_diag: row %lld is listed twice", (long long)k);
    if (pos < npos_nz)
      return layout_error(LAYOUT_ERR_STATE, "lrn_upload_diag: constraint %lld of block %d is stored (it has entries): its diagonal "
                                            "belongs into the stored matrix", (long long)k, ilmi);
    L.dg_of_pos[pos] = s;
    L.dg_nat[s] = (int)k;
    L.dg_h[s] = pos_space ? pos : (int)k;
  }
  return {};
}

}  // namespace lrn
