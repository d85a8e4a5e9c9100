// Model upload (reference MyModel -> device layout): lrn_upload_model lays every block and the linear part out on the host
// (model_layout.h) and copies the arrays over; lrn_free_model, lrn_get_constraint.
#include <algorithm>

#include "ctx.h"
#include "model_layout.h"
#include "ops.h"

namespace lrn {

static_assert(LAYOUT_ERR_ARG == LRN_ERR_ARG && LAYOUT_ERR_STATE == LRN_ERR_STATE, "model_layout.h returns the library's codes");

// ------------------------------------------------------------------ kernels
__global__ void scatter_dense_kernel(const long* __restrict__ ptr, const int* __restrict__ er,
                                     const int* __restrict__ ec, const double* __restrict__ ev,
                                     double* __restrict__ Ad, int msz) {
  int s = blockIdx.y;   // dense slot = position
  long b = ptr[s], e = ptr[s + 1];
  double* A = Ad + (long)s * msz * msz;
  for (long k = b + (long)blockIdx.x * blockDim.x + threadIdx.x; k < e; k += (long)gridDim.x * blockDim.x)
    A[(long)er[k] + (long)ec[k] * msz] = ev[k];
}

__global__ void build_constraint_kernel(const long* __restrict__ ptr, const int* __restrict__ er,
                                        const int* __restrict__ ec, const double* __restrict__ ev,
                                        int pos, double* __restrict__ out, int msz) {
  long b = ptr[pos], e = ptr[pos + 1];
  for (long k = b + (long)blockIdx.x * blockDim.x + threadIdx.x; k < e; k += (long)gridDim.x * blockDim.x)
    out[(long)er[k] + (long)ec[k] * msz] = ev[k];
}

int alloc_common(lrn_ctx* c) {
  size_t n = (size_t)c->nvar;
  LRN_TRY(ensure(c, c->H, n * n * 8, true));
  LRN_TRY(ensure(c, c->info_dev, 64, true));
  for (DBuf* d : {&c->v0, &c->v1, &c->v2, &c->v3}) LRN_TRY(ensure(c, *d, (n + 64) * 8, true));
  for (auto& b : c->lmi) {
    size_t mm = (size_t)b.msz * b.msz * 8;
    for (DBuf* d : {&b.X, &b.S, &b.W, &b.G, &b.Gi, &b.Si}) LRN_TRY(ensure(c, *d, mm, true));
    LRN_TRY(ensure(c, b.D, (size_t)b.msz * 8, true));
    LRN_TRY(ensure(c, b.DDsi, (size_t)b.msz * 8, true));
  }
  return LRN_OK;
}

}  // namespace lrn

using namespace lrn;

static void free_block(LmiBlock& b) {
  for (DBuf* d : b.other_bufs()) release(*d);
  b.tri_nch = 0;
  b.dense_route = LmiBlock::DENSE_SCALAR;
  drop_rank_classes(b);
  drop_diag(b);
}

void lrn_free_model(lrn_ctx* c) {
  for (auto& b : c->lmi) free_block(b);
  c->lmi.clear();
  for (DBuf* d : c->model_bufs()) release(*d);
  c->T_m = 0;
  c->T_owner = nullptr;
  c->T_layout = 0;
  c->have_H = c->have_L = false;
  c->nlmi = c->nvar = c->nlin = 0;
}

// the host fields and the device arrays of one block from its layout
static int upload_block(lrn_ctx* c, LmiBlock& b, BlockLayout& L) {
  b.sigma.swap(L.sigma);
  b.ipos.swap(L.ipos);
  b.nnz.swap(L.nnz);
  b.qA = L.qA;
  b.npos_nz = L.npos_nz;
  b.nd = L.nd;
  b.q_wave = L.q_wave;
  b.nent = L.nent();
  b.ncq = L.ncq();
  b.loc_lo = L.loc_lo;      // (the lists of the local route stay on the host until an assembly takes it: localops.hip)
  b.loc_hi = L.loc_hi;
  b.loc_ready = false;
  b.loc_sptr.swap(L.loc_sptr);
  b.loc_aptr.swap(L.loc_aptr);
  b.loc_sup.swap(L.loc_sup);
  b.loc_a.swap(L.loc_a);
  b.lg_hi = L.lg_hi;        // (the same for the long route: longops.hip)
  b.lg_ready = false;
  b.lg_plan_key.clear();
  b.lg_rho.clear();
  for (size_t k = 0; k + 1 < L.lg_rptr.size(); ++k) b.lg_rho.push_back((int)(L.lg_rptr[k + 1] - L.lg_rptr[k]));
  b.lg_rptr.swap(L.lg_rptr);
  b.lg_eptr.swap(L.lg_eptr);
  b.lg_rows.swap(L.lg_rows);
  b.lg_ec.swap(L.lg_ec);
  b.lg_ev.swap(L.lg_ev);
  LRN_TRY(upload(c, b.cq_q, L.cq_q));
  LRN_TRY(upload(c, b.cq_ptr, L.cq_ptr));
  LRN_TRY(upload(c, b.cq_j, L.cq_j));
  LRN_TRY(upload(c, b.cq_v, L.cq_v));
  b.sp_ok = false;
  if (L.sp_ok) {
    LRN_TRY(upload(c, b.pc_ptr, L.pc_ptr));
    LRN_TRY(upload(c, b.pc_r, L.pc_r));
    LRN_TRY(upload(c, b.pc_t, L.pc_t));
    LRN_TRY(upload(c, b.ent_t, L.ent_t));
    LRN_TRY(ensure(c, b.Mv, (size_t)b.ncq * 8));
    LRN_TRY(ensure(c, b.Zs, (size_t)b.ncq * 8));
    b.sp_long_cols.swap(L.sp_long_cols);
    b.sp_ok = true;
  }
  LRN_TRY(upload(c, b.ent_ptr, L.ent_ptr));
  LRN_TRY(upload(c, b.ent_r, L.ent_r));
  LRN_TRY(upload(c, b.ent_c, L.ent_c));
  LRN_TRY(upload(c, b.ent_v, L.ent_v));
  LRN_TRY(upload(c, b.hidx, L.hidx));
  LRN_TRY(upload(c, b.sigma_d, b.sigma));
  LRN_TRY(upload(c, b.ipos_d, b.ipos));
  return LRN_OK;
}

// positions [0, nd) as dense matrices, and the route of the passes over them
static int scatter_dense_prefix(lrn_ctx* c, LmiBlock& b) {
  if (b.nd > 0) {
    LRN_TRY(ensure(c, b.Adense, (size_t)b.nd * b.msz * b.msz * 8, true));
    hipLaunchKernelGGL(scatter_dense_kernel, dim3(64, b.nd), dim3(256), 0, c->stream,
                       b.ent_ptr.as<long>(), b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(),
                       b.Adense.as<double>(), b.msz);
  }
  return dense_route_setup(c, b, false);
}

// rank-one factors, rows reordered to H index order
static int upload_rank_one(lrn_ctx* c, LmiBlock& b, const int64_t* bc, const int64_t* br, const double* bv) {
  RankOneLayout R;
  rank_one_layout(b.msz, c->nvar, bc, br, bv, b.ipos, c->pos_space, R);
  b.bnnz = (long)R.b_col.size();
  LRN_TRY(upload(c, b.b_ptr, R.b_ptr));
  LRN_TRY(upload(c, b.b_col, R.b_col));
  LRN_TRY(upload(c, b.b_val, R.b_val));
  b.has_B = b.bnnz > 0;
  return LRN_OK;
}

static int upload_linear(lrn_ctx* c, int nlin, const int64_t* colptr, const int64_t* rowval, const double* nzval) {
  LinearLayout L;
  LRN_LAYOUT(c, linear_layout(c->nvar, nlin, colptr, rowval, nzval, c->pos_space ? &c->lmi[0].ipos : nullptr, c->pos_space, L));
  const size_t nn = L.cl_row.size();
  LRN_TRY(upload(c, c->cl_rown, L.cl_rown));
  LRN_TRY(upload(c, c->cl_ptr, L.cl_ptr));
  LRN_TRY(upload(c, c->cl_row, L.cl_row));
  LRN_TRY(upload(c, c->cl_val, nzval, nn * 8, nn * 8));
  LRN_TRY(ensure(c, c->lin_xs, (size_t)nlin * 8, true));
  c->lp_n = (long)L.lp_r.size();
  LRN_TRY(upload(c, c->lp_r, L.lp_r, 4));      // (the paddings: one element each, as these lists always had)
  LRN_TRY(upload(c, c->lp_c, L.lp_c, 4));
  LRN_TRY(upload(c, c->lp_ptr, L.lp_ptr));
  LRN_TRY(upload(c, c->lp_l, L.lp_l, 4));
  LRN_TRY(upload(c, c->lp_w, L.lp_w, 8));
  LRN_TRY(upload(c, c->cr_ptr, L.cr_ptr));
  LRN_TRY(upload(c, c->cr_col, L.cr_col, 4));
  LRN_TRY(upload(c, c->cr_val, L.cr_val, 8));
  return LRN_OK;
}

// the model into a context that holds none; on an error the caller frees what is there
static int upload_model(lrn_ctx* c, int nlmi, int nvar, const int64_t* msizes, const int64_t* const* AA_colptr,
                        const int64_t* const* AA_rowval, const double* const* AA_nzval, const int64_t* const* B_colptr,
                        const int64_t* const* B_rowval, const double* const* B_nzval, const int64_t* sigmaA, const int64_t* qA,
                        int nlin, const int64_t* Clin_colptr, const int64_t* Clin_rowval, const double* Clin_nzval) {
  c->nlmi = nlmi;
  c->nvar = nvar;
  update_shard_bs(c);
  c->nlin = nlin;
  c->pos_space = (nlmi == 1);
  c->lmi.resize(nlmi);
  for (int il = 0; il < nlmi; ++il) {
    LmiBlock& b = c->lmi[il];
    const int m = (int)msizes[il];
    if (m <= 0) return set_error(c, LRN_ERR_ARG, "msizes[%d] = %d", il, m);
    b.msz = m;
    size_t free_b = 0, total_b = 0;      // (what the earlier blocks left: the dense prefix takes at most 0.55 of it)
    (void)hipMemGetInfo(&free_b, &total_b);
    BlockLayout L;
    LRN_LAYOUT(c, block_layout(m, nvar, AA_colptr[il], AA_rowval[il], AA_nzval[il], sigmaA + (long)il * nvar, qA[2 * il],
                               c->pos_space, c->opt.dense_threshold, free_b, L, c->opt.pair_local_min, c->opt.pair_long_min));
    LRN_TRY(upload_block(c, b, L));
    LRN_TRY(scatter_dense_prefix(c, b));
    b.has_B = false;
    if (B_colptr && B_colptr[il] && B_rowval && B_nzval) LRN_TRY(upload_rank_one(c, b, B_colptr[il], B_rowval[il], B_nzval[il]));
  }
  if (nlin > 0) {
    if (!Clin_colptr || !Clin_rowval || !Clin_nzval) return set_error(c, LRN_ERR_ARG, "null C_lin");
    LRN_TRY(upload_linear(c, nlin, Clin_colptr, Clin_rowval, Clin_nzval));
  }
  LRN_TRY(alloc_common(c));
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  return LRN_OK;
}

extern "C" int lrn_upload_model(lrn_ctx* c, int nlmi, int nvar, const int64_t* msizes,
                                const int64_t* const* AA_colptr, const int64_t* const* AA_rowval,
                                const double* const* AA_nzval, const int64_t* const* B_colptr,
                                const int64_t* const* B_rowval, const double* const* B_nzval,
                                const int64_t* sigmaA, const int64_t* qA, int nlin,
                                const int64_t* Clin_colptr, const int64_t* Clin_rowval,
                                const double* Clin_nzval) {
  if (!c) return LRN_ERR_ARG;
  if (nlmi < 0 || nvar <= 0 || nlin < 0) return set_error(c, LRN_ERR_ARG, "bad sizes");
  if (nlmi > 0 && (!msizes || !AA_colptr || !AA_rowval || !AA_nzval || !sigmaA || !qA))
    return set_error(c, LRN_ERR_ARG, "null model array");
  LRN_HIP(c, hipSetDevice(c->device));
  lrn_free_model(c);
  const int rc = upload_model(c, nlmi, nvar, msizes, AA_colptr, AA_rowval, AA_nzval, B_colptr, B_rowval, B_nzval, sigmaA, qA,
                              nlin, Clin_colptr, Clin_rowval, Clin_nzval);
  if (rc != LRN_OK) {      // a failed upload leaves no model, and its message
    const std::string msg = c->err;
    (void)hipStreamSynchronize(c->stream);
    lrn_free_model(c);
    update_shard_bs(c);
    c->err = msg;
  }
  return rc;
}

extern "C" int lrn_get_constraint(lrn_ctx* c, int ilmi, int k, double* A_out) {
  if (!c || ilmi < 0 || ilmi >= c->nlmi || k < 0 || k >= c->nvar || !A_out) return LRN_ERR_ARG;
  LmiBlock& b = c->lmi[ilmi];
  int pos = b.ipos[k];
  if (b.factored && pos >= b.npos_nz)          // (a stored constraint of a hybrid block is returned like any other)
    return set_error(c, LRN_ERR_STATE, "lrn_get_constraint: block %d is factored (lrn_set_factored): no constraint matrix is stored", ilmi);
  size_t mm = (size_t)b.msz * b.msz * 8;
  if (pos < b.nd) return copy_out(c, A_out, b.Adense.as<double>() + (size_t)pos * b.msz * b.msz, mm);
  LRN_TRY(ensure(c, c->scratch, mm));
  LRN_HIP(c, hipMemsetAsync(c->scratch.p, 0, mm, c->stream));
  hipLaunchKernelGGL(build_constraint_kernel, dim3(8), dim3(256), 0, c->stream, b.ent_ptr.as<long>(),
                     b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(), pos,
                     c->scratch.as<double>(), b.msz);
  return copy_out(c, A_out, c->scratch.p, mm);
}
