// Factor declarations on an uploaded model: rank-k factors of a block (lrn_upload_lowrank), the factors as the block's
// constraint data (lrn_set_factored), diagonal parts beside them (lrn_upload_diag).  The layouts and the checks on host
// data: model_layout.h.
#include <algorithm>

#include "ctx.h"
#include "model_layout.h"
#include "ops.h"
#include "ragged_plan.h"

using namespace lrn;

static int has_entries_error(lrn_ctx* c, const LmiBlock& b, int ilmi) {
  return set_error(c, LRN_ERR_STATE, "lrn_set_factored: the AA of block %d has entries (%ld): a factored block takes its "
                                     "constraints from the factors alone, or each one from a stored row or from factors, never both", ilmi, b.nent);
}

// Rank-k factors of the constraints of block ilmi (datarank >= 1): A_k = V_k diag(d_k) V_k', V as an (nvar * khat) x msz
// CSC (1-based; row k * khat + p = column p of V_k, the orientation of B in lrn_upload_model), d[nvar * khat].  Stored as
// CSR by factor column in H index order (schur_factored.hip::assemble_lowrank).  Host or device arrays.
extern "C" int lrn_upload_lowrank(lrn_ctx* c, int ilmi, int khat, const int64_t* V_colptr, const int64_t* V_rowval,
                                  const double* V_nzval, const double* d) {
  if (!c) return LRN_ERR_ARG;
  if (ilmi < 0 || ilmi >= c->nlmi) return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: block %d of %d", ilmi, c->nlmi);
  const bool wide = khat == 32 || khat == 64;      // (a wide block: option "lowrank_wide")
  if (khat != 1 && khat != 2 && khat != 4 && khat != 8 && khat != 16 && !(wide && c->opt.lowrank_wide)) {
    if (!c->opt.lowrank_wide) return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: khat = %d (1, 2, 4, 8 or 16)", khat);
    return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: khat = %d (1, 2, 4, 8, 16, or 32 or 64 under option lowrank_wide)", khat);
  }
  if (!V_colptr || !d) return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: null factor array");
  LRN_HIP(c, hipSetDevice(c->device));
  LmiBlock& b = c->lmi[ilmi];
  if (wide && b.dg_n > 0 && !c->opt.wide_diag)      // (option "wide_diag": the rows stay, as under a narrow re-upload)
    return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: khat = %d on block %d, which holds diagonal parts (lrn_upload_diag): a "
                                     "wide block carries none -- store such a constraint as a matrix", khat, ilmi);
  const int m = b.msz, nvar = c->nvar;
  const long R = (long)nvar * khat;
  LRN_LAYOUT(c, lowrank_check_size(m, nvar, khat));
  // the caller's arrays, host or device, on the host
  std::vector<int64_t> cp(m + 1);
  LRN_HIP(c, hipMemcpy(cp.data(), V_colptr, (size_t)(m + 1) * 8, hipMemcpyDefault));
  LRN_LAYOUT(c, lowrank_check_colptr(m, cp.data()));
  const long nnz = cp[m] - 1;
  if (nnz > 0 && (!V_rowval || !V_nzval)) return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: null factor array");
  std::vector<int64_t> rv(nnz);
  std::vector<double> nz(nnz), w(R);
  if (nnz > 0) {
    LRN_HIP(c, hipMemcpy(rv.data(), V_rowval, (size_t)nnz * 8, hipMemcpyDefault));
    LRN_HIP(c, hipMemcpy(nz.data(), V_nzval, (size_t)nnz * 8, hipMemcpyDefault));
  }
  LRN_HIP(c, hipMemcpy(w.data(), d, (size_t)R * 8, hipMemcpyDefault));
  LowrankLayout L;
  LRN_LAYOUT(c, lowrank_layout(m, nvar, khat, cp.data(), rv.data(), nz.data(), w.data(), b.ipos, c->pos_space, L));
  LRN_TRY(upload(c, b.v_ptr, L.v_ptr));
  LRN_TRY(upload(c, b.v_col, L.v_col.data(), (size_t)nnz * 4, (size_t)std::max<long>(nnz, 1) * 4));
  LRN_TRY(upload(c, b.v_val, L.v_val.data(), (size_t)nnz * 8, (size_t)std::max<long>(nnz, 1) * 8));
  LRN_TRY(upload(c, b.v_w, L.v_w));
  release(b.Vd);                 // (the dense copy is rebuilt from these factors on first use)
  b.have_Vd = false;
  b.Ys_version = -1;             // (and Y = W Vd of option "fac_op_scaled" with it)
  drop_rank_classes(b);          // (and the rank-class plan, option "lowrank_ragged": rebuilt on first use)
  b.rg_Rc = ragged_cols(L.v_w.data(), nvar, khat);
  b.lr_khat = khat;
  b.vnnz = nnz;
  b.has_V = true;
  b.v_partial = factors_partial(c->pos_space, b.sigma, b.npos_nz, khat, L.v_w.data());
  if (b.factored && stored_and_factored(c->pos_space, b.sigma, b.npos_nz, khat, L.v_w.data()) >= 0) {      // (new factors that overlap the stored rows of a hybrid block)
    b.factored = false;
    drop_diag(b);
    return has_entries_error(c, b, ilmi);
  }
  if (b.factored) LRN_TRY(lowrank_dense_factors(c, b));      // (new factors of a factored block: its operators read Vd)
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  return LRN_OK;
}

// on = 1: the factors of lrn_upload_lowrank ARE the constraint data of block ilmi (A_k = V_k diag(d_k) V_k', AA = -A as
// everywhere): AA vec(.) and mat(AA' .) of the resident path run in factor form (dataops.hip), the Schur matrix comes from
// mode 1.  The block's AA is without entries, or holds the rows of a few STORED constraints whose factor columns all have
// weight 0 (a hybrid block: stored-entry kernels + factor form, cross terms in schur_factored.hip) -- no constraint may be counted
// twice.  on = 0 takes the declaration back.
extern "C" int lrn_set_factored(lrn_ctx* c, int ilmi, int on) {
  if (!c) return LRN_ERR_ARG;
  if (ilmi < 0 || ilmi >= c->nlmi) return set_error(c, LRN_ERR_ARG, "lrn_set_factored: block %d of %d", ilmi, c->nlmi);
  LRN_HIP(c, hipSetDevice(c->device));
  LmiBlock& b = c->lmi[ilmi];
  if (!on) {
    b.factored = false;
    drop_diag(b);
    return LRN_OK;
  }
  if (!b.has_V)
    return set_error(c, LRN_ERR_STATE, "lrn_set_factored: no factors were uploaded for block %d (lrn_upload_lowrank)", ilmi);
  if (b.npos_nz > 0) {
    std::vector<double> w((size_t)c->nvar * b.lr_khat);
    LRN_HIP(c, hipMemcpy(w.data(), b.v_w.p, w.size() * 8, hipMemcpyDeviceToHost));
    if (stored_and_factored(c->pos_space, b.sigma, b.npos_nz, b.lr_khat, w.data()) >= 0) return has_entries_error(c, b, ilmi);
  }
  LRN_TRY(lowrank_dense_factors(c, b));
  b.factored = true;
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  return LRN_OK;
}

// Diagonal parts of a factored block: constraint rows[s] (0-based) is diag(a_s) + V D V', a_s = column s of a (msz x nrows).
// Host or device arrays; nrows = 0 clears.  The rows are factored positions -- a stored constraint carries its diagonal in its
// entries.  Kept: dg_h (H index per row), dg_nat (constraint per row), dg_of_pos (position -> row or -1), dg_a (diagops.hip)
extern "C" int lrn_upload_diag(lrn_ctx* c, int ilmi, int64_t nrows, const int64_t* rows, const double* a) {
  if (!c) return LRN_ERR_ARG;
  if (ilmi < 0 || ilmi >= c->nlmi) return set_error(c, LRN_ERR_ARG, "lrn_upload_diag: block %d of %d", ilmi, c->nlmi);
  LRN_HIP(c, hipSetDevice(c->device));
  LmiBlock& b = c->lmi[ilmi];
  const int m = b.msz, nvar = c->nvar;
  if (nrows < 0 || nrows > nvar) return set_error(c, LRN_ERR_ARG, "lrn_upload_diag: %lld rows, the model has %d constraints", (long long)nrows, nvar);
  if (!b.factored)
    return set_error(c, LRN_ERR_STATE, "lrn_upload_diag: block %d is not factored (lrn_set_factored): a diagonal part goes with "
                                       "the factors of a factored block", ilmi);
  if (nrows == 0) {
    drop_diag(b);
    return LRN_OK;
  }
  if (lowrank_wide(b) && !c->opt.wide_diag)      // (option "wide_diag": accepted, diagops.hip sums groups of 32 and 64)
    return set_error(c, LRN_ERR_ARG, "lrn_upload_diag: block %d is wide (khat = %d > 16): a wide block carries no diagonal part "
                                     "-- store such a constraint as a matrix", ilmi, b.lr_khat);
  if (!rows || !a) return set_error(c, LRN_ERR_ARG, "lrn_upload_diag: null array");
  const int ns = (int)nrows;
  std::vector<int64_t> rw(ns);
  LRN_HIP(c, hipMemcpy(rw.data(), rows, (size_t)ns * 8, hipMemcpyDefault));
  DiagRowsLayout L;
  LRN_LAYOUT(c, diag_rows_layout(nvar, ilmi, ns, rw.data(), b.ipos, b.npos_nz, c->pos_space, L));
  // staged in buffers of their own and swapped in at the end: an allocation or a copy that fails halfway leaves the parts
  // already uploaded, and their dg_n, as they were
  DBuf th, tn, tp, ta;
  auto stage = [&]() -> int {
    LRN_TRY(upload(c, th, L.dg_h));
    LRN_TRY(upload(c, tn, L.dg_nat));
    LRN_TRY(upload(c, tp, L.dg_of_pos));
    LRN_TRY(upload(c, ta, a, (size_t)ns * m * 8, (size_t)ns * m * 8));
    LRN_HIP(c, hipStreamSynchronize(c->stream));      // (the host vectors above are read by asynchronous copies)
    return LRN_OK;
  };
  const int rc = stage();
  if (rc == LRN_OK) {
    std::swap(b.dg_h, th);
    std::swap(b.dg_nat, tn);
    std::swap(b.dg_of_pos, tp);
    std::swap(b.dg_a, ta);
  }
  for (DBuf* d : {&th, &tn, &tp, &ta}) release(*d);      // (the previous buffers, or the unfinished new ones)
  if (rc != LRN_OK) return rc;
  b.dg_n = ns;
  return LRN_OK;
}
