// Debug entry points of the C ABI (the tests' window on the resident state and on single device routines).
#include <cstring>
#include <new>

#include "../../include/loraine_hip.h"
#include "jacobi.h"
#include "model_layout.h"
#include "ops.h"
#include "options.h"

using namespace lrn;

extern "C" int lrn_dbg_get_block(lrn_ctx* c, int il, const char* name, double* out, int* flag) {
  if (!c || il < 0 || il >= c->nlmi || !name || !out) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  LmiBlock& b = c->lmi[il];
  const size_t mm_ = (size_t)b.msz * b.msz * 8, mv = (size_t)b.msz * 8;
  struct { const char* n; DBuf* d; size_t bytes; } tab[] = {
      {"W", &b.W, mm_}, {"Si", &b.Si, mm_}, {"G", &b.G, mm_}, {"Gi", &b.Gi, mm_}, {"D", &b.D, mv}, {"DDsi", &b.DDsi, mv},
      {"X", &b.X, mm_}, {"S", &b.S, mm_}, {"delX", &b.delX, mm_}, {"delS", &b.delS, mm_}, {"RNT", &b.RNT, mm_},
      {"LX", &b.LXf, mm_}, {"LS", &b.LSf, mm_}, {"Bs", &b.Bs, mm_}, {"TX", &b.TX, mm_}, {"Ki", &b.Ki, mm_}, {"Yh", &b.Yh, mm_},
      {"Zh", &b.Zh, mm_}, {"Qm", &b.Qm, mm_}, {"Rd", &b.Rd, mm_}};
  if (flag) *flag = b.nt_free ? 1 : 0;
  c->timing["ns_c"] = b.ns_c;
  for (auto& t : tab)
    if (!strcmp(name, t.n)) {
      if (!t.d->p || t.d->bytes < t.bytes) return set_error(c, LRN_ERR_STATE, "block array %s not allocated", name);
      return copy_out(c, out, t.d->p, t.bytes);
    }
  return set_error(c, LRN_ERR_ARG, "unknown block array %s", name);
}

extern "C" int lrn_dbg_eigmin(lrn_ctx* c, int n, const double* M, double* lam, int* steps) {
  if (!c || n <= 0 || !M || !lam) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  DBuf d;
  LRN_TRY(ensure(c, d, (size_t)n * n * 8));
  LRN_TRY(copy_in(c, d.p, M, (size_t)n * n * 8));
  int rc = steps ? eigmin_dev(c, d.as<double>(), n, lam, steps) : eigmin_certified(c, d.as<double>(), n, lam);
  release(d);
  return rc;
}

extern "C" int lrn_dbg_svd_jacobi(lrn_ctx* c, int n, const double* A, double* U_sigma, double* V, double* sigma,
                                  int* sweeps) {
  if (!c || n <= 0 || !A || !U_sigma || !sigma) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  DBuf dA, dV, dS;
  size_t mm = (size_t)n * n * 8;
  LRN_TRY(ensure(c, dA, mm));
  if (V) LRN_TRY(ensure(c, dV, mm));          // V == NULL: no accumulation, as every production caller
  LRN_TRY(ensure(c, dS, (size_t)n * 8));
  LRN_TRY(copy_in(c, dA.p, A, mm));
  int sw = 0;
  LRN_TRY(jacobi_svd(c, dA.as<double>(), V ? dV.as<double>() : nullptr, dS.as<double>(), n, &sw));
  if (sweeps) *sweeps = sw;
  LRN_TRY(copy_out(c, U_sigma, dA.p, mm));
  if (V) LRN_TRY(copy_out(c, V, dV.p, mm));
  int rc = copy_out(c, sigma, dS.p, (size_t)n * 8);
  release(dA); release(dV); release(dS);
  return rc;
}

// ---- the layouts of model_layout.h on caller arrays: no context, no device (tests/test_model_layout_cpu.py)
namespace {
// hands the array called `name` back: its length in *count, its elements in iout (integers, widened) or dout (doubles) where given
struct NamedOut {
  const char* name;
  int64_t* count;
  int64_t* iout;
  double* dout;
  bool found = false;
  bool hit(const char* n) { return !strcmp(n, name) && (found = true); }
  template <class T> void ints(const char* n, const std::vector<T>& v) {
    if (!hit(n)) return;
    *count = (int64_t)v.size();
    for (size_t i = 0; iout && i < v.size(); ++i) iout[i] = (int64_t)v[i];
  }
  void scalar(const char* n, long v) { ints(n, std::vector<long>(1, v)); }
  void reals(const char* n, const std::vector<double>& v) {
    if (!hit(n)) return;
    *count = (int64_t)v.size();
    for (size_t i = 0; dout && i < v.size(); ++i) dout[i] = v[i];
  }
};

int layout_result(const LayoutError& e, const NamedOut& o, char* msg, int msg_len) {
  std::string text = e ? e.msg : o.found ? std::string() : std::string("unknown layout array ") + o.name;
  if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", text.c_str());
  return e ? e.code : o.found ? LRN_OK : LRN_ERR_ARG;
}
}  // namespace

extern "C" int lrn_dbg_model_layout(const char* name, int msz, int nvar, const int64_t* AA_colptr, const int64_t* AA_rowval,
                                    const double* AA_nzval, const int64_t* sigma, int64_t qA, int pos_space, double dense_threshold,
                                    int64_t free_bytes, const int64_t* B_colptr, const int64_t* B_rowval, const double* B_nzval, int nlin,
                                    const int64_t* Clin_colptr, const int64_t* Clin_rowval, const double* Clin_nzval, int64_t* count,
                                    int64_t* iout, double* dout, char* msg, int msg_len) {
  if (!name || !count || msz <= 0 || nvar <= 0 || nlin < 0 || free_bytes < 0 || !AA_colptr || !sigma) return LRN_ERR_ARG;
  NamedOut o{name, count, iout, dout};
  *count = 0;
  BlockLayout L;
  LayoutError e = block_layout(msz, nvar, AA_colptr, AA_rowval, AA_nzval, sigma, qA, pos_space != 0, dense_threshold,
                               (size_t)free_bytes, L);
  if (e) return layout_result(e, o, msg, msg_len);
  o.ints("sigma", L.sigma); o.ints("ipos", L.ipos); o.ints("nnz", L.nnz);
  o.scalar("qA", L.qA); o.scalar("npos_nz", L.npos_nz); o.scalar("nd", L.nd); o.scalar("q_wave", L.q_wave);
  o.ints("ent_ptr", L.ent_ptr); o.ints("ent_r", L.ent_r); o.ints("ent_c", L.ent_c); o.reals("ent_v", L.ent_v);
  o.ints("hidx", L.hidx);
  o.ints("cq_q", L.cq_q); o.ints("cq_ptr", L.cq_ptr); o.ints("cq_j", L.cq_j); o.reals("cq_v", L.cq_v);
  o.scalar("sp_ok", L.sp_ok); o.ints("pc_ptr", L.pc_ptr); o.ints("pc_r", L.pc_r); o.ints("pc_t", L.pc_t);
  o.ints("ent_t", L.ent_t); o.ints("sp_long_cols", L.sp_long_cols);
  o.scalar("loc_lo", L.loc_lo); o.scalar("loc_hi", L.loc_hi); o.ints("loc_sptr", L.loc_sptr); o.ints("loc_sup", L.loc_sup);
  o.ints("loc_aptr", L.loc_aptr); o.reals("loc_a", L.loc_a);
  o.scalar("lg_hi", L.lg_hi); o.ints("lg_rptr", L.lg_rptr); o.ints("lg_rows", L.lg_rows); o.ints("lg_eptr", L.lg_eptr);
  o.ints("lg_ec", L.lg_ec); o.reals("lg_ev", L.lg_ev);
  if (!o.found && B_colptr && !strncmp(name, "b_", 2)) {
    RankOneLayout R;
    rank_one_layout(msz, nvar, B_colptr, B_rowval, B_nzval, L.ipos, pos_space != 0, R);
    o.ints("b_ptr", R.b_ptr); o.ints("b_col", R.b_col); o.reals("b_val", R.b_val);
  }
  if (!o.found && nlin > 0 && Clin_colptr) {
    LinearLayout C;
    e = linear_layout(nvar, nlin, Clin_colptr, Clin_rowval, Clin_nzval, &L.ipos, pos_space != 0, C);
    if (e) return layout_result(e, o, msg, msg_len);
    o.ints("cl_ptr", C.cl_ptr); o.ints("cl_row", C.cl_row); o.ints("cl_rown", C.cl_rown);
    o.ints("lp_r", C.lp_r); o.ints("lp_c", C.lp_c); o.ints("lp_ptr", C.lp_ptr); o.ints("lp_l", C.lp_l); o.reals("lp_w", C.lp_w);
    o.ints("cr_ptr", C.cr_ptr); o.ints("cr_col", C.cr_col); o.reals("cr_val", C.cr_val);
  }
  return layout_result(e, o, msg, msg_len);
}

extern "C" int lrn_dbg_factor_layout(const char* name, int msz, int nvar, const int64_t* ipos, int npos_nz, int pos_space, int khat,
                                     const int64_t* V_colptr, const int64_t* V_rowval, const double* V_nzval, const double* d,
                                     int64_t nrows, const int64_t* rows, int64_t* count, int64_t* iout, double* dout, char* msg,
                                     int msg_len) {
  if (!name || !count || msz <= 0 || nvar <= 0 || !ipos || npos_nz < 0 || npos_nz > nvar || nrows < 0 || nrows > nvar)
    return LRN_ERR_ARG;
  NamedOut o{name, count, iout, dout};
  *count = 0;
  std::vector<int> ip(nvar), sg(nvar, 0);
  for (int k = 0; k < nvar; ++k) {
    if (ipos[k] < 0 || ipos[k] >= nvar) return LRN_ERR_ARG;
    ip[k] = (int)ipos[k];
    sg[ip[k]] = k;
  }
  LayoutError e;
  if (V_colptr && d && khat > 0) {
    LowrankLayout L;
    e = lowrank_check_size(msz, nvar, khat);
    if (!e) e = lowrank_check_colptr(msz, V_colptr);
    if (!e) e = lowrank_layout(msz, nvar, khat, V_colptr, V_rowval, V_nzval, d, ip, pos_space != 0, L);
    if (e) return layout_result(e, o, msg, msg_len);
    o.ints("v_ptr", L.v_ptr); o.ints("v_col", L.v_col); o.reals("v_val", L.v_val); o.reals("v_w", L.v_w);
    o.scalar("v_partial", factors_partial(pos_space != 0, sg, npos_nz, khat, L.v_w.data()));
    o.scalar("stored_and_factored", stored_and_factored(pos_space != 0, sg, npos_nz, khat, L.v_w.data()));
  }
  if (!o.found && rows) {
    DiagRowsLayout D;
    e = diag_rows_layout(nvar, 0, (int)nrows, rows, ip, npos_nz, pos_space != 0, D);
    if (e) return layout_result(e, o, msg, msg_len);
    o.ints("dg_h", D.dg_h); o.ints("dg_nat", D.dg_nat); o.ints("dg_of_pos", D.dg_of_pos);
  }
  return layout_result(e, o, msg, msg_len);
}

// ---- lrn_set_option without a device (options.h; tests/test_options_cpu.py)
extern "C" const char* lrn_dbg_option_name(int index) { return option_name(index); }

// Not probed: the keys whose action needs a device or a communicator -- "comm_fail_ensure", "detect_release"
extern "C" int lrn_dbg_option_probe(const char* key, double value, int* rc, char* msg, int msg_len, unsigned char* opt_bytes,
                                    int opt_cap, int* opt_size, int64_t* watched14) {
  if (!rc || !opt_size || !watched14 || opt_cap < 0 || (opt_cap > 0 && !opt_bytes)) return LRN_ERR_ARG;
  if (key && (!strcmp(key, "comm_fail_ensure") || !strcmp(key, "detect_release"))) return LRN_ERR_ARG;
  // a context that exists on the host only: zeroed storage (the padding of LrnOptions compares equal from call to call), no
  // stream, one block; what an option may touch beside LrnOptions starts from values it can be told from
  void* mem = calloc(1, sizeof(lrn_ctx));
  if (!mem) return LRN_ERR_NOMEM;
  lrn_ctx* c = new (mem) lrn_ctx;
  c->hop_version = 7;
  c->lmi.resize(1);
  c->lmi[0].t_cap = 5;
  c->lmi[0].p_cap = 6;
  c->timing["probe"] = 1.0;
  c->counts["probe"] = 1;
  *rc = key ? lrn_set_option(c, key, value) : LRN_OK;      // (no key: the defaults)
  if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", c->err.c_str());
  *opt_size = (int)sizeof(LrnOptions);
  if (opt_cap > 0) memcpy(opt_bytes, &c->opt, std::min((size_t)opt_cap, sizeof(LrnOptions)));
  const int64_t w[14] = {c->hop_version, c->profile ? 1 : 0, c->lz_res_limit, c->lz_wh_left, c->lz_wh_fired, c->lz_wh_run,
                         c->lz_wh_step,  c->lz_wh_wg,        c->shard_bs_opt, c->shard_bs,   c->lmi[0].t_cap, c->lmi[0].p_cap,
                         (int64_t)c->timing.size(), (int64_t)c->counts.size()};
  for (int i = 0; i < 14; ++i) watched14[i] = w[i];
  c->~lrn_ctx();
  free(mem);
  return LRN_OK;
}
