// Debug entry points of the C ABI (the tests' window on the resident state and on single device routines).
#include <cstring>

#include "../../include/loraine_hip.h"
#include "jacobi.h"
#include "ops.h"

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
