// The value options of lrn_set_option as one table: name, field of LrnOptions, conversion of the double the caller passes, reject
// message, side effects on the context.  Pure host code: no HIP header, no context -- option_apply works on an LrnOptions alone and
// reports the effects as a mask, which lrn_set_option (api.hip) carries out.  LrnOptions (ctx.h) must be complete where this header
// is included.  lrn_dbg_option_name / lrn_dbg_option_probe (dbg.hip) show the table without a device
// (tests/test_options_cpu.py, tests/golden/option_semantics.json).
//
// A new option is one line of kOptions.  Keys that are actions, or live on the context instead of in LrnOptions, are not in the
// table: kContextOptions names them, lrn_set_option holds their code.
#pragma once
#include <cstring>
#include <limits>

namespace lrn {

constexpr int OPT_OK = 0, OPT_ERR_ARG = -1;      // (LRN_OK, LRN_ERR_ARG of lrn_common.h)
constexpr int OPT_NOT_A_VALUE = 1;               // option_apply: the key is not in the table

// what lrn_set_option does to the context after the value is stored
enum : unsigned {
  OPT_INVALIDATES_HOP = 1u,       // the operator choice is taken again, an H of the other setting is not reused (hop_version = -1)
  OPT_RESETS_BATCH_CAPS = 2u,     // t_cap = p_cap = 0 on every block: the T / P workspaces are laid out again
};

// how the double becomes the stored value.  The casts are C casts of the double, taken before any clamp or mask
enum OptRule {
  OPT_CAST,           // (type)value
  OPT_NONZERO,        // value != 0.0 -> 1, else 0
  OPT_CLAMP,          // (type)value moved into [lo, hi]; an open end is -inf / +inf
  OPT_NEG_IS_MINUS1,  // a double: value < 0.0 -> -1.0, else value
  OPT_REJECT,         // !(lo <= value <= hi): OPT_ERR_ARG with `reject`, nothing stored; else (type)value
  OPT_ZERO_OR_ONE,    // any value but 0.0 and 1.0: OPT_ERR_ARG with `reject`, nothing stored
  OPT_MASK,           // (int)value & (int)hi
};

struct OptionDesc {
  const char* name;
  // the field: exactly one of the four is set, and names the kind (int / long / double / flag)
  int LrnOptions::*i;
  long LrnOptions::*l;
  double LrnOptions::*d;
  bool LrnOptions::*flag;
  OptRule rule;
  double lo, hi;
  const char* reject;
  unsigned effects;
};

constexpr double OPT_INF = std::numeric_limits<double>::infinity();

#define LRN_OPT_I(name, rule, lo, hi, reject, fx) {#name, &LrnOptions::name, nullptr, nullptr, nullptr, rule, lo, hi, reject, fx}
#define LRN_OPT_L(name, rule, lo, hi, reject, fx) {#name, nullptr, &LrnOptions::name, nullptr, nullptr, rule, lo, hi, reject, fx}
#define LRN_OPT_D(name, rule, lo, hi, reject, fx) {#name, nullptr, nullptr, &LrnOptions::name, nullptr, rule, lo, hi, reject, fx}
#define LRN_OPT_F(name, fx) {#name, nullptr, nullptr, nullptr, &LrnOptions::name, OPT_NONZERO, 0, 0, nullptr, fx}
// the common shapes
#define LRN_OPT_INT(name) LRN_OPT_I(name, OPT_CAST, 0, 0, nullptr, 0)
#define LRN_OPT_REAL(name) LRN_OPT_D(name, OPT_CAST, 0, 0, nullptr, 0)
#define LRN_OPT_ONOFF(name, fx) LRN_OPT_I(name, OPT_NONZERO, 0, 0, nullptr, fx)
#define LRN_OPT_TRI(name, fx) LRN_OPT_I(name, OPT_CLAMP, -1, 1, nullptr, fx)      // -1 auto / 0 / 1

// state read by the next launch unless marked: "upload" = read by the next lrn_upload_model / lrn_upload_lowrank / lrn_upload_diag
// only, "measurement" = for tools and tests, not for solves
static const OptionDesc kOptions[] = {
    LRN_OPT_REAL(dense_threshold),                                                           // upload
    LRN_OPT_L(t_batch, OPT_CAST, 0, 0, nullptr, OPT_RESETS_BATCH_CAPS),
    LRN_OPT_L(p_batch, OPT_CAST, 0, 0, nullptr, OPT_RESETS_BATCH_CAPS),
    LRN_OPT_INT(prec_eig),
    LRN_OPT_REAL(pivot_boost),
    LRN_OPT_INT(schur_chol),
    LRN_OPT_INT(schur_plan),
    LRN_OPT_INT(gemm3_ksplit),
    LRN_OPT_INT(gemm_no_skip),                                                               // measurement
    LRN_OPT_INT(gemm_dyn_masks),                                                             // measurement
    LRN_OPT_INT(gemm1_diag),
    LRN_OPT_I(gemm_lab, OPT_MASK, 0, 127, nullptr, 0),                                       // measurement
    LRN_OPT_INT(gemm3_sched),
    LRN_OPT_INT(gemm3_tile),
    LRN_OPT_INT(gemm3_strip),
    LRN_OPT_INT(gemm3_stagger),
    LRN_OPT_INT(jacobi_wgs),
    LRN_OPT_INT(jacobi_block),
    LRN_OPT_INT(jacobi_inner),
    LRN_OPT_INT(pair_lanes),
    LRN_OPT_I(pair_local, OPT_ZERO_OR_ONE, 0, 1, "pair_local is 0 or 1", OPT_INVALIDATES_HOP),
    LRN_OPT_I(pair_local_min, OPT_REJECT, 1.0, 1.0e9, "pair_local_min is a count of entries >= 1", 0),      // upload
    LRN_OPT_I(pair_long, OPT_ZERO_OR_ONE, 0, 1, "pair_long is 0 or 1", OPT_INVALIDATES_HOP),
    LRN_OPT_I(pair_long_min, OPT_REJECT, 1.0, 1.0e9, "pair_long_min is a count of entries >= 1", 0),        // upload
    LRN_OPT_L(pair_long_split, OPT_REJECT, 1.0, 1.0e15, "pair_long_split is a count of products >= 1", OPT_INVALIDATES_HOP),
    LRN_OPT_I(pair_long_mfma, OPT_ZERO_OR_ONE, 0, 1, "pair_long_mfma is 0 or 1", OPT_INVALIDATES_HOP),
    LRN_OPT_D(pair_long_scratch_mb, OPT_REJECT, 0.0, OPT_INF, "pair_long_scratch_mb is a size >= 0", OPT_INVALIDATES_HOP),
    LRN_OPT_INT(matvec_sparse),
    LRN_OPT_INT(prec_dense),
    LRN_OPT_I(wmw_pattern_min, OPT_CLAMP, 2, OPT_INF, nullptr, 0),
    LRN_OPT_INT(profile_symv),                                                               // measurement
    LRN_OPT_INT(profile_ops),                                                                // measurement
    LRN_OPT_I(matvec_h, OPT_CAST, 0, 0, nullptr, OPT_INVALIDATES_HOP),
    LRN_OPT_I(pcg_lookahead, OPT_CLAMP, 0, 8, nullptr, 0),
    LRN_OPT_TRI(lowrank_form, 0),
    LRN_OPT_ONOFF(lowrank_ragged, OPT_INVALIDATES_HOP),
    LRN_OPT_ONOFF(lowrank_wide, OPT_INVALIDATES_HOP),                                        // upload
    LRN_OPT_ONOFF(wide_diag, OPT_INVALIDATES_HOP),                                           // upload, and the next launch
    LRN_OPT_ONOFF(ragged_ops, OPT_INVALIDATES_HOP),
    LRN_OPT_ONOFF(ragged_cross, OPT_INVALIDATES_HOP),
    LRN_OPT_ONOFF(ragged_ts, 0),
    LRN_OPT_I(ragged_ops_split, OPT_CLAMP, 0, 16, nullptr, 0),
    LRN_OPT_TRI(cg_lowrank, OPT_INVALIDATES_HOP),
    LRN_OPT_ONOFF(cg_factored, OPT_INVALIDATES_HOP),
    LRN_OPT_ONOFF(cg_diag, OPT_INVALIDATES_HOP),
    LRN_OPT_D(hop_max_mb, OPT_NEG_IS_MINUS1, 0, 0, nullptr, OPT_INVALIDATES_HOP),
    LRN_OPT_TRI(fac_op_scaled, OPT_INVALIDATES_HOP),
    LRN_OPT_TRI(fac_quadform, OPT_INVALIDATES_HOP),
    LRN_OPT_TRI(diag_sq_mfma, 0),
    LRN_OPT_TRI(fac_cross_lds, 0),
    LRN_OPT_INT(jacobi_cross),
    LRN_OPT_REAL(jacobi_early),
    LRN_OPT_INT(eigmin_pair),
    LRN_OPT_INT(lz_resident),
    LRN_OPT_INT(prepw_streams),
    LRN_OPT_F(jacobi_warm, 0),
    LRN_OPT_INT(nt_mode),
    LRN_OPT_INT(prec_inv),
    LRN_OPT_INT(shard_passes),
    LRN_OPT_INT(shard_products),
    LRN_OPT_I(shard_products_min, OPT_CLAMP, 16, OPT_INF, nullptr, 0),
    LRN_OPT_REAL(ns_l0),
    LRN_OPT_INT(ns_maxit),
    LRN_OPT_INT(ns_lanczos),
    LRN_OPT_I(ns_lanczos_min, OPT_CLAMP, 8, OPT_INF, nullptr, 0),
    LRN_OPT_INT(ns_dual),
    LRN_OPT_REAL(lyap_tol),
    LRN_OPT_INT(lyap_maxit),
    LRN_OPT_INT(lyap_form),
};

#undef LRN_OPT_I
#undef LRN_OPT_L
#undef LRN_OPT_D
#undef LRN_OPT_F
#undef LRN_OPT_INT
#undef LRN_OPT_REAL
#undef LRN_OPT_ONOFF
#undef LRN_OPT_TRI

// the keys lrn_set_option serves itself (api.hip): state of the context, actions and test hooks
static const char* const kContextOptions[] = {"profile",          "lz_res_limit",   "lz_test_withhold", "shard_bs",
                                              "comm_fail_ensure", "detect_release", "reset_timing"};

constexpr int kNumOptions = (int)(sizeof(kOptions) / sizeof(kOptions[0]));
constexpr int kNumContextOptions = (int)(sizeof(kContextOptions) / sizeof(kContextOptions[0]));

// the index-th key lrn_set_option accepts -- the table, then kContextOptions -- or nullptr past the end
inline const char* option_name(int index) {
  if (index < 0 || index >= kNumOptions + kNumContextOptions) return nullptr;
  return index < kNumOptions ? kOptions[index].name : kContextOptions[index - kNumOptions];
}

// Stores `value` under `key` as the table says.  OPT_OK: stored, *effects = what the context owes.  OPT_ERR_ARG: rejected, nothing
// stored, *msg = the text.  OPT_NOT_A_VALUE: no such key in the table, nothing touched
inline int option_apply(LrnOptions& o, const char* key, double value, unsigned* effects, const char** msg) {
  const OptionDesc* t = nullptr;
  for (const OptionDesc& e : kOptions)
    if (!strcmp(key, e.name)) { t = &e; break; }
  if (!t) return OPT_NOT_A_VALUE;
  const bool rejected = (t->rule == OPT_REJECT && !(value >= t->lo && value <= t->hi)) ||
                        (t->rule == OPT_ZERO_OR_ONE && value != 0.0 && value != 1.0);
  if (rejected) {
    *msg = t->reject;
    return OPT_ERR_ARG;
  }
  if (t->flag) {
    o.*t->flag = value != 0.0;
  } else if (t->d) {
    o.*t->d = t->rule == OPT_NEG_IS_MINUS1 && value < 0.0 ? -1.0 : value;
  } else if (t->l) {
    o.*t->l = (long)value;
  } else {
    int v = t->rule == OPT_NONZERO ? (value != 0.0 ? 1 : 0) : (int)value;
    if (t->rule == OPT_CLAMP) v = v < t->lo ? (int)t->lo : v > t->hi ? (int)t->hi : v;
    if (t->rule == OPT_MASK) v &= (int)t->hi;
    o.*t->i = v;
  }
  *effects = t->effects;
  return OPT_OK;
}

}  // namespace lrn
