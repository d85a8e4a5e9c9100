// The CG recurrence and the device-resident PCG.
// Replaces cg of ConjugateGradients.jl 0.1 (call sites reference src/predictor_corrector.jl:134,235) around MyA and the
// preconditioners of src/Solvers.jl:572-904.
// This file holds: the CG kernels, the operator selection (op_select, op_apply), pcg_dev and the extern "C" entry points
// (lrn_matvec, lrn_matvec_partial, lrn_make_rhs, lrn_prec_*, lrn_pcg).  The preconditioners (none, H_beta, H_alpha: setup,
// apply, dense form) live in prec.hip; the operator itself -- MyA, Ax = AA vec(W mat(AA' x) W) -- and every other pass over the
// constraint data in dataops.hip.
#include <algorithm>
#include <cmath>

#include "../../include/loraine_hip.h"
#include "ctx.h"
#include "ops.h"
#include "prec.h"
#include "reduce.h"

namespace lrn {

// ------------------------------------------------------------------ vector kernels (single workgroup)
// scal: [0]=gamma [1]=pAp [2]=alpha [3]=rr [4]=flag(alpha invalid) [5]=beta [6]=||b|| [7]=zr
__global__ __launch_bounds__(1024) void cg_norm_kernel(const double* __restrict__ b, int n, double* __restrict__ scal, int slot) {
  __shared__ double sh[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) s += b[i] * b[i];
  s = wg_sum<16>(s, sh);
  if (threadIdx.x == 0) scal[slot] = s;
}

// ---- the CG recurrence as two multi-workgroup launches per iteration (round 4; round 3: two single-workgroup kernels of
// 33 + 15 us at nvar 20 000 and a host read between them).
//   cg_b_kernel(it): q = p'Ap (from the partial sums the operator left, or a redundant dot per workgroup), alpha = g / q,
//                    x += alpha p, r -= alpha Ap on the workgroup's slice, z = M^-1 r inline when the preconditioner is
//                    diagonal (none, H_beta), partial sums of r'r and z'r
//   cg_d_kernel(it): r'r -> the convergence test of ConjugateGradients.jl (relative residual <= tol); z'r, beta,
//                    p = z + beta p on the slice
// Every workgroup forms the global scalars itself from the same partials in the same order: no grid barrier, no atomics,
// all workgroups take the same branch.  scal[8] = exit code once the iteration has ended (30 converged, -13 alpha
// invalid), scal[9] = the iteration it ended in, both mirrored to host-mapped words: the host queues iterations ahead of
// the test it has read (option pcg_lookahead); kernels queued beyond the last iteration find the flag set and leave
// x, r, p alone -- count and result are those of the loop that tests after every step.  g = r'z alternates between
// scal[10] and scal[11] (a workgroup of cg_d_kernel must not overwrite the value its neighbours are still reading).
// (not wg_sum<4> of reduce.h: the CG scalars, and so the iteration counts, are pinned to this pairwise order of the waves)
__device__ __forceinline__ double wg_sum256(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

static constexpr int CG_MAXWG = 256;

__global__ __launch_bounds__(256) void cg_b_kernel(const double* __restrict__ p, const double* __restrict__ Ap,
                                                   double* __restrict__ r, double* __restrict__ x, double* __restrict__ z,
                                                   int kind, const double* __restrict__ d, int n, int per,
                                                   double* __restrict__ scal, const double* __restrict__ qpart, int nq,
                                                   double* __restrict__ rrpart, double* __restrict__ zrpart,
                                                   double* __restrict__ hostw, int it) {
  __shared__ double sh[4];
  if (scal[8] != 0.0) return;
  double q = 0.0;
  if (qpart) for (int i = threadIdx.x; i < nq; i += 256) q += qpart[i];
  else for (int i = threadIdx.x; i < n; i += 256) q += p[i] * Ap[i];
  q = wg_sum256(q, sh);
  const double g = scal[10 + ((it - 1) & 1)];
  const double alpha = g / q;
  const bool bad = !(alpha >= 0.0) || isinf(alpha);
  if (blockIdx.x == 0 && threadIdx.x == 0) { scal[1] = q; scal[2] = alpha; scal[4] = bad ? 1.0 : 0.0; }
  if (bad) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      scal[9] = (double)it;
      hostw[1] = (double)it;
      hostw[0] = -13.0;
      __threadfence_system();
      scal[8] = -13.0;
    }
    return;
  }
  const int i0 = blockIdx.x * per, i1 = min(n, i0 + per);
  double rr = 0.0, zr = 0.0;
  for (int i = i0 + threadIdx.x; i < i1; i += 256) {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * Ap[i];
    r[i] = ri;
    rr += ri * ri;
    if (kind == 0) { z[i] = ri; zr += ri * ri; }                       // MyM_no   (Solvers.jl:620-622)
    else if (kind == 2) { const double zi = ri / d[i]; z[i] = zi; zr += zi * ri; }   // MyM_beta (:670-672)
  }
  rr = wg_sum256(rr, sh);
  zr = wg_sum256(zr, sh);
  if (threadIdx.x == 0) { rrpart[blockIdx.x] = rr; zrpart[blockIdx.x] = zr; }
}

// first != 0: the start of the iteration, p = z, g = z'r (no test, no beta)
__global__ __launch_bounds__(256) void cg_d_kernel(const double* __restrict__ z, const double* __restrict__ r,
                                                   double* __restrict__ p, int n, int per, int nwg,
                                                   double* __restrict__ scal, const double* __restrict__ rrpart,
                                                   const double* __restrict__ zrpart, double* __restrict__ hostw, int it,
                                                   double res0, double tol, int first) {
  __shared__ double sh[4];
  if (scal[8] != 0.0) return;
  if (!first) {
    double rr = 0.0;
    for (int i = threadIdx.x; i < nwg; i += 256) rr += rrpart[i];
    rr = wg_sum256(rr, sh);
    if (sqrt(rr) / res0 <= tol) {
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        scal[3] = rr;
        scal[9] = (double)it;
        hostw[1] = (double)it;
        hostw[0] = 30.0;
        __threadfence_system();
        scal[8] = 30.0;
      }
      return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[3] = rr;
  }
  double zr = 0.0;
  if (zrpart) for (int i = threadIdx.x; i < nwg; i += 256) zr += zrpart[i];
  else for (int i = threadIdx.x; i < n; i += 256) zr += z[i] * r[i];
  zr = wg_sum256(zr, sh);
  const double beta = first ? 0.0 : zr / scal[10 + ((it - 1) & 1)];
  const int i0 = blockIdx.x * per, i1 = min(n, i0 + per);
  if (first) for (int i = i0 + threadIdx.x; i < i1; i += 256) p[i] = z[i];
  else for (int i = i0 + threadIdx.x; i < i1; i += 256) p[i] = z[i] + beta * p[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) { scal[10 + (it & 1)] = zr; scal[5] = beta; scal[7] = zr; }
}

// Which operator serves this NT scaling: the assembled Schur matrix (hop.hip) or the matrix-free MyA.  Decided once per
// scaling from the static cost model and the CG iterations of the previous scaling; with a communicator the ranks take
// the decision together (free memory and so the assembly path can differ between them).
int op_select(lrn_ctx* c, bool* use_h) {
  if (c->hop_version != c->scal_version) {
    c->cg_prev_iters = c->cg_cur_iters;
    c->cg_cur_iters = 0;
    bool use = hop_worthwhile(c, c->cg_prev_iters);
    if (c->comm && c->world > 1) {
      double w[1] = {use ? 0.0 : 1.0};
      LRN_TRY(comm_status_max(c, w, 1));
      use = w[0] == 0.0;
    }
    c->hop_use = use;
    c->hop_version = c->scal_version;
  }
  if (c->hop_use) {
    const int rc = hop_prepare(c);
    if (rc != LRN_OK) {
      if (c->comm && c->world > 1) return rc;       // (every rank returns it: the status reduction of the exchange)
      c->hop_use = false;                            // one GPU: the matrix-free operator needs no workspace
      c->counts["hop_fallback"] += 1;
      c->err.clear();
    }
  }
  *use_h = c->hop_use;
  return LRN_OK;
}

// Ap = A p by the selected operator (all-reduced when sharded)
static int op_apply(lrn_ctx* c, bool use_h, const double* p, double* Ap, double* qpart = nullptr, int* nq = nullptr) {
  const bool sharded = c->comm && c->world > 1;
  if (nq) *nq = 0;
  if (use_h) {
    if (c->opt.profile_symv) tic(c);
    LRN_TRY(hop_apply(c, p, Ap, qpart, nq));
    if (c->opt.profile_symv) toc(c, "hop_symv");        // (measurement: this rank's share of H x alone, tools/shard_balance_c5.py)
  } else if (sharded) {
    // one process per GPU: this rank's rows of W M W, then ONE all-reduce of the nvar-vector on this stream -- the
    // recurrence is replicated and stays on the device, as on one GPU
    LRN_TRY(matvec_partial_dev(c, p, Ap, c->rank, c->world));
  } else {
    return matvec_dev(c, p, Ap);
  }
  if (sharded) LRN_TRY(comm_allreduce(c, Ap, c->nvar, 0));
  return LRN_OK;
}

// cg(A, b; tol, maxIter, precon) -- restates ConjugateGradients.jl 0.1 (see oracle.cg)
int pcg_dev(lrn_ctx* c, const double* b, double tol, int maxit, double* x, int* exit_code, int* iters) {
  const int n = c->nvar;
  hipStream_t st = c->stream;
  LRN_TRY(ensure(c, c->cgbuf, (size_t)(6 * (size_t)n + 64) * 8));
  double* r = c->cgbuf.as<double>();
  double* z = r + n;
  double* p = z + n;
  double* Ap = p + n;
  double* tmpv = Ap + n;
  double* scal = tmpv + n;          // 16 doubles
  constexpr int NSLOT = 16;
  if (!c->pin) {
    LRN_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->pin), NSLOT * 16 * 8, hipHostMallocMapped));
    LRN_HIP(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->pin_dev), c->pin, 0));
  }
  if (!c->pcg_ev[0])
    for (int i = 0; i < NSLOT; ++i) LRN_HIP(c, hipEventCreateWithFlags(&c->pcg_ev[i], hipEventDisableTiming));
  volatile double* hs = c->pin;
  // partial sums of the recurrence kernels and of the operator (hop.hip): after the six vectors
  const int nwg = std::max(1, std::min(CG_MAXWG, (n + 255) / 256));
  const int per = (n + nwg - 1) / nwg;
  LRN_TRY(ensure(c, c->cgpart, (size_t)(2 * CG_MAXWG + (n + 63) / 64 + 64) * 8));
  double* rrpart = c->cgpart.as<double>();
  double* zrpart = rrpart + CG_MAXWG;
  double* qpart = zrpart + CG_MAXWG;
  long nmv = 0;
  LRN_HIP(c, hipMemsetAsync(x, 0, (size_t)n * 8, st));
  LRN_HIP(c, hipMemsetAsync(scal, 0, 16 * 8, st));
  hipLaunchKernelGGL(cg_norm_kernel, dim3(1), dim3(1024), 0, st, b, n, scal, 6);
  double bb = 0.0;
  LRN_HIP(c, hipMemcpyAsync(&bb, scal + 6, 8, hipMemcpyDeviceToHost, st));
  LRN_HIP(c, hipStreamSynchronize(st));
  if (std::sqrt(bb) == 0.0) { *exit_code = 1; *iters = 0; return LRN_OK; }
  // r = b - A*0 = b
  LRN_HIP(c, hipMemcpyAsync(r, b, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
  const double residual_0 = std::sqrt(bb);
  if (residual_0 <= tol) { *exit_code = 2; *iters = 0; return LRN_OK; }
  for (int i = 0; i < NSLOT * 16; ++i) hs[i] = 0.0;
  bool use_h = false;
  LRN_TRY(op_select(c, &use_h));
  LRN_TRY(prec_dense_if_worthwhile(c, c->cg_prev_iters));
  const int kind = prec_kind(c);
  const double* dprec = prec_diag(c);
  LRN_TRY(prec_apply_dev(c, r, z, tmpv));
  hipLaunchKernelGGL(cg_d_kernel, dim3(nwg), dim3(256), 0, st, z, r, p, n, per, nwg, scal, rrpart, (const double*)nullptr,
                     c->pin_dev, 0, residual_0, tol, 1);
  // The host runs `ahead` iterations in front of the convergence test it has read: the exit words of iteration `it` are
  // written to host-mapped memory by its kernels and looked at (behind an event) while iteration it + ahead is queued.
  const int ahead = std::max(0, std::min(NSLOT - 2, c->opt.pcg_lookahead));
  int done_code = 0, done_it = 0;
  auto poll = [&](int it) -> int {          // the words of iteration `it`
    const int s = it % NSLOT;
    LRN_HIP(c, hipEventSynchronize(c->pcg_ev[s]));
    if (hs[s * 16] != 0.0) { done_code = (int)hs[s * 16]; done_it = (int)hs[s * 16 + 1]; }
    return LRN_OK;
  };
  int it = 1;
  for (; it <= maxit && done_code == 0; ++it) {
    int nq = 0;
    LRN_TRY(op_apply(c, use_h, p, Ap, qpart, &nq));
    ++nmv;
    const int s = it % NSLOT;
    hipLaunchKernelGGL(cg_b_kernel, dim3(nwg), dim3(256), 0, st, p, Ap, r, x, z, kind, dprec, n, per, scal,
                       nq > 0 ? qpart : (const double*)nullptr, nq, rrpart, zrpart, c->pin_dev + s * 16, it);
    if (kind == 1) LRN_TRY(prec_apply_dev(c, r, z, tmpv));
    hipLaunchKernelGGL(cg_d_kernel, dim3(nwg), dim3(256), 0, st, z, r, p, n, per, nwg, scal, rrpart,
                       kind == 1 ? (const double*)nullptr : zrpart, c->pin_dev + s * 16, it, residual_0, tol, 0);
    LRN_HIP(c, hipEventRecord(c->pcg_ev[s], st));
    if (it - ahead >= 1) LRN_TRY(poll(it - ahead));
  }
  const int last = std::min(it - 1, maxit);
  for (int k = std::max(1, last - ahead + 1); k <= last && done_code == 0; ++k) LRN_TRY(poll(k));
  LRN_HIP(c, hipStreamSynchronize(st));
  LRN_HIP(c, hipGetLastError());
  c->counts["matvec"] += nmv;
  if (done_code != 0) { *exit_code = done_code; *iters = done_it; }
  else { *exit_code = -2; *iters = maxit; }
  c->cg_cur_iters += *iters;
  return LRN_OK;
}

}  // namespace lrn

using namespace lrn;

// the CG side (mat-vec, H_alpha, PCG) reads the entries of AA: not for factored blocks -- unless option "cg_factored" is set:
// then the operator runs in factor form (dataops.hip) or through H assembled in mode 1 (hop.hip) and ts of H_alpha comes from
// the factors.  One GPU only (partial: lrn_matvec_partial; world > 1: any call) -- the factor routes are not sharded
// ... and not for a block with diagonal parts (lrn_upload_diag), whatever cg_factored says: ts of H_alpha is built from the
// factors and the stored rows and would silently miss them
// ... unless option "cg_diag" is set beside cg_factored: then prec_setup adds the diagonal-row term to ts (diagops.hip::ts_diag);
// the operators carry the diagonal parts anyway.  One GPU and not lrn_matvec_partial, as for cg_factored
static int no_diag(lrn_ctx* c, const char* what, bool partial = false) {
  for (size_t il = 0; il < c->lmi.size(); ++il)
    if (c->lmi[il].factored && c->lmi[il].dg_n > 0) {
      if (c->opt.cg_diag != 0 && c->opt.cg_factored != 0 && (partial || c->world > 1))
        return set_error(c, LRN_ERR_STATE, "%s: block %d is factored with diagonal parts (lrn_upload_diag): option cg_diag runs on "
                                           "one GPU (world = %d) and not through lrn_matvec_partial", what, (int)il, c->world);
      if (cg_diag_on(c)) return LRN_OK;
      return set_error(c, LRN_ERR_STATE, "%s: block %d is factored with diagonal parts (lrn_upload_diag): the CG path does not "
                                         "hold them, such a model is solved with kit = 0", what, (int)il);
    }
  return LRN_OK;
}

static int no_factored(lrn_ctx* c, const char* what, bool partial = false) {
  LRN_TRY(no_diag(c, what, partial));
  for (size_t il = 0; il < c->lmi.size(); ++il)
    if (c->lmi[il].factored) {
      if (c->opt.cg_factored != 0 && (partial || c->world > 1))
        return set_error(c, LRN_ERR_STATE, "%s: block %d is factored (lrn_set_factored): option cg_factored runs on one GPU "
                                           "(world = %d) and not through lrn_matvec_partial", what, (int)il, c->world);
      if (c->opt.cg_factored != 0) return LRN_OK;
      return set_error(c, LRN_ERR_STATE, "%s: block %d is factored (lrn_set_factored): the CG path needs the constraint "
                                         "matrices, factored data is solved with kit = 0", what, (int)il);
    }
  return LRN_OK;
}

extern "C" int lrn_matvec(lrn_ctx* c, const double* x, double* Ax) {
  if (!c || !x || !Ax) return LRN_ERR_ARG;
  LRN_TRY(no_factored(c, "lrn_matvec"));
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v0.p, x, (size_t)n * 8));
  // the assembled-matrix operator only when lrn_pcg chose it for this scaling, or when it is forced (option matvec_h = 2)
  bool use_h = false;
  if (c->opt.matvec_h == 2 || (c->hop_use && c->hop_version == c->scal_version)) LRN_TRY(op_select(c, &use_h));
  tic(c);
  LRN_TRY(op_apply(c, use_h, c->v0.as<double>(), c->v1.as<double>()));
  toc(c, "matvec");
  return copy_out(c, Ax, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_matvec_partial(lrn_ctx* c, const double* x, double* Ax_partial) {
  if (!c || !x || !Ax_partial) return LRN_ERR_ARG;
  LRN_TRY(no_factored(c, "lrn_matvec_partial", true));
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v0.p, x, (size_t)n * 8));
  LRN_TRY(matvec_partial_dev(c, c->v0.as<double>(), c->v1.as<double>(), c->rank, c->world));
  return copy_out(c, Ax_partial, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_make_rhs(lrn_ctx* c, const double* Rp, const double* const* RdS, double* h) {
  if (!c || !Rp || !h || (c->nlmi > 0 && !RdS)) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v1.p, Rp, (size_t)n * 8));
  for (int il = 0; il < c->nlmi; ++il) {
    LmiBlock& b = c->lmi[il];
    if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set");
    LRN_TRY(ensure_m(c, b.msz));
    // wmw reads its middle factor transposed (everywhere else it is symmetric): it gets (Rd+S)', so that a Rd+S that is
    // not symmetric still gives W (Rd+S) W -- with constraint matrices that are not symmetric either the two differ
    LRN_TRY(copy_in(c, c->m1.p, RdS[il], (size_t)b.msz * b.msz * 8));
    transpose_mat(c->stream, c->m1.as<double>(), b.msz, c->m0.as<double>());
    LRN_TRY(wmw(c, b, c->m0.as<double>(), c->m1.as<double>(), c->m2.as<double>()));
    LRN_TRY(aa_times(c, b, c->m2.as<double>(), c->v1.as<double>()));
  }
  return copy_out(c, h, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_prec_setup(lrn_ctx* c, int prec, int erank, int aamat, int* info) {
  if (!c) return LRN_ERR_ARG;
  LRN_TRY(no_factored(c, "lrn_prec_setup"));
  LRN_HIP(c, hipSetDevice(c->device));
  return prec_setup(c, prec, erank, aamat, info);
}

extern "C" int lrn_prec_apply(lrn_ctx* c, const double* x, double* Mx) {
  if (!c || !x || !Mx) return LRN_ERR_ARG;
  LRN_TRY(no_diag(c, "lrn_prec_apply"));
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v0.p, x, (size_t)n * 8));
  LRN_TRY(prec_dense_if_worthwhile(c, 0));      // (no application expected: option prec_dense = 2 alone builds it here)
  LRN_TRY(prec_apply_dev(c, c->v0.as<double>(), c->v1.as<double>(), c->v2.as<double>()));
  return copy_out(c, Mx, c->v1.p, (size_t)n * 8);
}

extern "C" int lrn_pcg(lrn_ctx* c, const double* h, double tol, int maxit, double* x, int* exit_code, int* iters) {
  if (!c || !h || !x || !exit_code || !iters) return LRN_ERR_ARG;
  LRN_TRY(no_factored(c, "lrn_pcg"));
  LRN_HIP(c, hipSetDevice(c->device));
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v0.p, h, (size_t)n * 8));
  PhaseTimer timer(c, c->profile);
  LRN_TRY(pcg_dev(c, c->v0.as<double>(), tol, maxit, c->v3.as<double>(), exit_code, iters));
  timer.stop("pcg");
  if (c->profile) c->counts["pcg_iters"] += *iters;
  return copy_out(c, x, c->v3.p, (size_t)n * 8);
}
