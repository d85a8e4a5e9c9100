// Schur-complement assembly  H_ij = tr(A_i W A_j W)  (+ C_lin diag(X_lin/S_lin) C_lin'),
// factorisation and solve.  Replaces makeBBBBs / makeBBBBsi / _dot / makeBBBB_rank1
// (reference src/makeBBBB.jl:1-218) and predictor_corrector.jl:36-39,53-90,199.
//
// Every unordered pair {i,j} is computed once, by the constraint that comes first in the
// reference's nnz-sorted order sigmaA (its "owner"), exactly as makeBBBBsi walks it
// (makeBBBB.jl:77,151,192).  The matrix is kept in sigma-POSITION space when nlmi == 1 so
// that an owner's results form one contiguous column of the lower triangle -- this is what
// makes the multi-GPU exchange an all-gather of column blocks.
//
//   owner dense  (positions < nd):   T_i = W A_i W on the FP64 MFMA GEMM
//        GEMM1  P_i = A_i W                      (batched, 2 msz^3)
//        GEMM2  T_i = W P_i, lower 128-tiles only, strictly-lower tiles scaled by 2 (msz^3)
//        GEMM3  H[j,i] = <A_j, T_i> for dense j >= i: one TN GEMM whose K loop skips the
//               upper tiles (packed-symmetric inner product, nvar^2 msz^2 / 2), split-K slabs
//        gather H[j,i] = sum_e a_e T_i[r_e,c_e] for sparse j
//   owner sparse (positions >= nd):  one WAVEFRONT per entry (i,j), lanes over the
//        nnz_i x nnz_j product terms a_e a_f W[c_e,r_f] W[c_f,r_e]   (the _dot kernel);
//        owners with <= 4 nonzeros use one THREAD per entry (the nnz==1 fast path,
//        makeBBBB.jl:188-209, is its 1x1 case).  Option "pair_local": owners whose partners all have a support of at most
//        32 rows and columns take the dense A[S, S] on the MFMA instead (localops.hip).  Option "pair_long": long sparse
//        owners (a trace row, a band) from Z_i = (A_i W) on their rows, nnz_j |R_i| per pair, sliced (longops.hip).
//   rank-one data (mode -1): BG = B G (sparse x dense), H += (BG BG').^2 with the square
//        fused in the MFMA GEMM epilogue (makeBBBB.jl:7-14).
//   rank-k data (mode 1): U = G' V, H += blocksum(d d' .* (U'U).^2) over khat x khat blocks, again in the
//        epilogue of one MFMA product (assemble_lowrank).  Option "lowrank_ragged": a block of mixed ranks by rank class, on
//        the compacted columns (raggedops.hip).
// This file: the sparse owners, the linear part, the driver schur_assemble, factorisation and solve.  schur_dense.hip: the dense
// owners; localops.hip: sparse owners with a small support; schur_factored.hip: rank-one / rank-k data and hybrid blocks;
// raggedops.hip: rank-k data by rank class; diagops.hip: diagonal parts of factored blocks; schur_plan.h, ragged_plan.h: the
// launch decisions, host only.
#include <algorithm>

#include "ops.h"
#include "schur_plan.h"

namespace lrn {

// ------------------------------------------------------------------ sparse pair kernels
// LANES lanes per entry (pi, pj >= pi), pi in [p_lo, p_hi):
//     H[i,j] = tr(A_i W A_j W) = sum_{(r,c) in A_i} sum_{(p,q) in A_j} a_rc b_pq W[c,p] W[q,r]
// The kernel is bound by the chain of dependent loads of one entry (entry lists -> W gathers -> reduction), not by
// gather bandwidth (rocprofv3, profiles/r02_sparse_*): what raises its throughput is entries in flight.  LANES = 64 for
// long products; 16 (four entries per wavefront) when nnz_i * nnz_j is a few hundred at most.  W is symmetric: both
// factors are fetched from the COLUMNS of the owner's support, W[p + c*msz] and W[q + r*msz] -- consecutive workgroups
// share pi, so at msz = 10^4 (W = 800 MB) the gathers of an owner stay in a few 80 KB columns (L2-miss traffic of the
// C5 assembly 234 GB -> 50 GB).  Staging the block W[supp_i, supp_j] in LDS was tried (one wave per entry, 8 KB each):
// a fifth of the fabric traffic again but 32 KB of LDS per workgroup cost 12 of 32 waves per CU and the kernel got
// slower (tru9 2.25 -> 2.75 ms, C5 110 -> 140 ms; profiles/r02_sparse_pair_lds_staged_summary.csv).
template <int LANES>
__global__ __launch_bounds__(256) void pair_wave_kernel(
    const long* __restrict__ ptr, const int* __restrict__ er, const int* __restrict__ ec,
    const double* __restrict__ ev, const double* __restrict__ W, int msz, int p_lo, int p_hi,
    int p_end, const int* __restrict__ hidx, double* __restrict__ H, int ldh, int rank, int world,
    int bs) {
  constexpr int PER_WG = 256 / LANES;
  const int lane = threadIdx.x & (LANES - 1), grp = threadIdx.x / LANES;
  const int pi = p_lo + blockIdx.y;
  if (pi >= p_hi) return;
  if (world > 1 && shard_owner(pi / bs, world) != rank) return;
  const int pj = pi + blockIdx.x * PER_WG + grp;
  const bool live = pj < p_end;                 // (whole wavefronts stay together for the shuffles below)
  double acc = 0.0;
  if (live) {
    const long ib = ptr[pi], jb = ptr[pj];
    const int ni = (int)(ptr[pi + 1] - ib), nj = (int)(ptr[pj + 1] - jb);
    const int total = ni * nj;
    for (int idx = lane; idx < total; idx += LANES) {
      int e = idx / nj, f = idx - e * nj;
      int r = er[ib + e], c = ec[ib + e];
      int p = er[jb + f], q = ec[jb + f];
      // A_i[r,c] W[c,p] A_j[p,q] W[q,r]
      acc += ev[ib + e] * ev[jb + f] * W[(long)p + (long)c * msz] * W[(long)q + (long)r * msz];
    }
  }
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, LANES);
  if (live && lane == 0) {
    H[h_lower(hidx[pi], hidx[pj], ldh)] += acc;
  }
}

// one thread per entry, owners with <= 4 nonzeros
__global__ __launch_bounds__(256) void pair_thread_kernel(
    const long* __restrict__ ptr, const int* __restrict__ er, const int* __restrict__ ec,
    const double* __restrict__ ev, const double* __restrict__ W, int msz, int p_lo, int p_end,
    const int* __restrict__ hidx, double* __restrict__ H, int ldh, int rank, int world, int bs) {
  const int pi = p_lo + blockIdx.y;
  if (pi >= p_end) return;
  if (world > 1 && shard_owner(pi / bs, world) != rank) return;
  const int pj = pi + blockIdx.x * 256 + threadIdx.x;
  if (pj >= p_end) return;
  const long ib = ptr[pi], jb = ptr[pj];
  const int ni = (int)(ptr[pi + 1] - ib), nj = (int)(ptr[pj + 1] - jb);
  double acc = 0.0;
  for (int e = 0; e < ni; ++e) {
    int r = er[ib + e], c = ec[ib + e];
    double a = ev[ib + e];
    for (int f = 0; f < nj; ++f) {
      int p = er[jb + f], q = ec[jb + f];
      acc += a * ev[jb + f] * W[(long)p + (long)c * msz] * W[(long)q + (long)r * msz];   // both from columns of A_i
    }
  }
  H[h_lower(hidx[pi], hidx[pj], ldh)] += acc;
}

// H += C_lin diag(xs) C_lin'  (lower triangle): one thread per target entry sums its contributions in
// a fixed order (lists built at upload) -- no floating-point atomics, results are reproducible
__global__ void lin_schur_kernel(const int* __restrict__ pr, const int* __restrict__ pc, const long* __restrict__ pp,
                                 const int* __restrict__ pl, const double* __restrict__ pw, long np,
                                 const double* __restrict__ xs, double* __restrict__ H, int ldh, int rank, int world,
                                 int bs) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= np) return;
  const int ri = pr[t], rj = pc[t];
  if (world > 1 && shard_owner(rj / bs, world) != rank) return;
  double s = 0.0;
  for (long k = pp[t]; k < pp[t + 1]; ++k) s += pw[k] * xs[pl[k]];
  H[(long)ri + (long)rj * ldh] += s;
}


__global__ void get_diag_kernel(const double* __restrict__ H, int n, double* __restrict__ d) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = H[(long)i * n + i];
}

__global__ void add_diag_kernel(double* __restrict__ H, int n, double eps) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) H[(long)i * n + i] += eps;
}

// natural-index full symmetric copy of the lower-authoritative H
__global__ void export_h_kernel(const double* __restrict__ H, int n, const int* __restrict__ ipos,
                                double* __restrict__ out) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    out[e] = H[h_lower(ipos ? ipos[i] : i, ipos ? ipos[j] : j, n)];
  }
}

__global__ void gather_vec_kernel(const double* __restrict__ src, const int* __restrict__ idx, double* __restrict__ dst, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[idx ? idx[i] : i];
}
__global__ void scatter_vec_kernel(const double* __restrict__ src, const int* __restrict__ idx, double* __restrict__ dst, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[idx ? idx[i] : i] = src[i];
}

// ------------------------------------------------------------------ host drivers

// lrn_schur_plan: 1 = the next assembly of this rank would take the Cholesky path (partial sums, all-reduce),
// 0 = Schur column blocks (all-gather) -- from this rank's own view
int schur_plan(lrn_ctx* c, int mode) {
  if (mode == -1 || mode == 1 || c->nlmi != 1) return 0;
  LmiBlock& b = c->lmi[0];
  long pcap = 0;
  const int pin = c->opt.schur_plan;
  c->opt.schur_plan = -1;                      // this rank's own view, whatever was pinned before
  const bool ok = b.nd > 0 && c->opt.schur_chol != 2 && chol_path_applicable(c, b, &pcap);
  c->opt.schur_plan = pin;
  return ok ? 1 : 0;
}

static int assemble_sparse(lrn_ctx* c, LmiBlock& b) {
  const int n = c->nvar;
  double* H = c->H.as<double>();
  // option "pair_local": the owners [loc_lo, loc_hi) go to assemble_local (localops.hip) with all their partners, the wave
  // kernel keeps [nd, loc_lo) and [loc_hi, q_wave).  One GPU; with the option off, an empty range or world > 1 the launches
  // below are the ones there always were
  const bool local_on = c->opt.pair_local != 0 && c->world == 1 && b.loc_hi > b.loc_lo;
  if (c->opt.pair_local != 0 && !local_on) c->counts["pair_local_skipped"] += 1;
  // option "pair_long": the long owners [nd, lg_end) go to assemble_long (longops.hip) with all their partners; where both
  // routes could take an owner the local route keeps it.  One GPU, and Zc of every owner within the scratch cap; otherwise
  // "pair_long_skipped" and, again, the launches there always were
  const int lg_end = local_on ? std::min(b.lg_hi, b.loc_lo) : b.lg_hi;
  const bool long_on = c->opt.pair_long != 0 && c->world == 1 && lg_end > b.nd && long_fits(c, b, lg_end);
  if (c->opt.pair_long != 0 && !long_on) c->counts["pair_long_skipped"] += 1;
  const int wave_lo = long_on ? lg_end : b.nd;
  const int wave_parts[2][2] = {{wave_lo, local_on ? b.loc_lo : b.q_wave}, {local_on ? b.loc_hi : b.q_wave, b.q_wave}};
  tic(c);
  if (b.q_wave > b.nd) {
    // entries per wavefront by the typical product length: mean nnz of the sparse owners squared
    double mean_nnz = 0.0;
    for (int p = b.nd; p < b.npos_nz; ++p) mean_nnz += (double)b.nnz[p];
    mean_nnz /= std::max(1, b.npos_nz - b.nd);
    int lanes = c->opt.pair_lanes;
    if (lanes != 4 && lanes != 8 && lanes != 16 && lanes != 64) lanes = mean_nnz * mean_nnz <= 512.0 ? 16 : 64;
    const int per_wg = 256 / lanes;
    std::vector<std::pair<int, int>> ranges;
    for (const auto& part : wave_parts)
      for (const auto& rg : owned_ranges(c->rank, c->world, c->shard_bs, part[0], part[1], 2048)) ranges.push_back(rg);
    for (const auto& rg : ranges) {
      const int a = rg.first, ny = rg.second - rg.first;
      dim3 grid((b.npos_nz - a + per_wg - 1) / per_wg, ny);
#define LRN_PAIR_LAUNCH(L)                                                                                           \
  hipLaunchKernelGGL(pair_wave_kernel<L>, grid, dim3(256), 0, c->stream, b.ent_ptr.as<long>(), b.ent_r.as<int>(),   \
                     b.ent_c.as<int>(), b.ent_v.as<double>(), b.W.as<double>(), b.msz, a, rg.second,                \
                     b.npos_nz, b.hidx.as<int>(), H, n, c->rank, c->world, c->shard_bs)
      if (lanes == 4) LRN_PAIR_LAUNCH(4);
      else if (lanes == 8) LRN_PAIR_LAUNCH(8);
      else if (lanes == 16) LRN_PAIR_LAUNCH(16);
      else LRN_PAIR_LAUNCH(64);
#undef LRN_PAIR_LAUNCH
    }
  }
  if (b.npos_nz > b.q_wave) {
    for (const auto& rg : owned_ranges(c->rank, c->world, c->shard_bs, b.q_wave, b.npos_nz, 4096)) {
      const int a = rg.first, ny = rg.second - rg.first;
      hipLaunchKernelGGL(pair_thread_kernel, dim3((b.npos_nz - a + 255) / 256, ny), dim3(256), 0, c->stream,
                         b.ent_ptr.as<long>(), b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(),
                         b.W.as<double>(), b.msz, a, b.npos_nz, b.hidx.as<int>(), H, n, c->rank,
                         c->world, c->shard_bs);          // (owners a .. a + ny - 1 by the grid, partners up to npos_nz)
    }
  }
  toc(c, "sparse");
  if (local_on) LRN_TRY(assemble_local(c, b));
  if (long_on) LRN_TRY(assemble_long(c, b, lg_end));
  return LRN_OK;
}

// the stored constraints of a block: dense owners, then sparse owners
static int assemble_stored(lrn_ctx* c, LmiBlock& b) {
  if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set (call lrn_prepare_w or lrn_set_scaling)");
  if (b.nd > 0) LRN_TRY(assemble_dense(c, b));
  if (b.npos_nz > b.nd) LRN_TRY(assemble_sparse(c, b));
  return LRN_OK;
}

int schur_assemble(lrn_ctx* c, int mode) {
  const int n = c->nvar;
  if (n <= 0) return set_error(c, LRN_ERR_STATE, "no model uploaded");
  if (c->world > 1 && !c->pos_space)
    return set_error(c, LRN_ERR_STATE, "Schur column sharding needs a single LMI block (sigma-position space)");
  PhaseTimer timer(c, c->profile);
  for (const auto& b : c->lmi)
    if (b.factored && mode != 1)
      return set_error(c, LRN_ERR_STATE, "lrn_schur_assemble: mode %d on a factored block (lrn_set_factored): its constraints "
                                         "exist as factors only, mode 1 assembles from them", mode);
  for (const auto& b : c->lmi)
    if (b.hybrid() && c->world > 1)
      return set_error(c, LRN_ERR_STATE, "lrn_schur_assemble: mode 1 on a factored block with stored constraints runs on one "
                                         "GPU (the cross terms are not sharded)");
  for (const auto& b : c->lmi)
    if (b.factored && b.dg_n > 0 && c->world > 1)
      return set_error(c, LRN_ERR_STATE, "lrn_schur_assemble: mode 1 on a factored block with diagonal parts (lrn_upload_diag) runs "
                                         "on one GPU (their terms are not sharded)");
  for (const auto& b : c->lmi)
    if (mode == 1 && b.has_V && lowrank_wide(b) && c->world > 1)
      return set_error(c, LRN_ERR_ARG, "lrn_schur_assemble: mode 1 on a wide block (khat = %d > 16, option lowrank_wide) runs on one "
                                       "GPU (the rank-class route is not sharded)", b.lr_khat);
  LRN_HIP(c, hipMemsetAsync(c->H.p, 0, (size_t)n * n * 8, c->stream));
  c->H_partial = false;
  c->H_owned_only = false;
  for (auto& b : c->lmi) {
    if (mode == -1) {
      LRN_TRY(assemble_rank1(c, b));
    } else if (mode == 1 && !b.factored && b.has_V && b.v_partial) {
      // factors for some constraints only, and the block is not factored: its AA holds every constraint (a hybrid model the
      // host materialised), the factors do not -- the general assembly over the entries is the exact one
      LRN_TRY(assemble_stored(c, b));
      c->counts["lowrank_from_entries"] += 1;
    } else if (mode == 1 && b.hybrid()) {     // H_SS from the stored entries, then H_FF and the cross terms (see assemble_cross)
      LRN_TRY(assemble_stored(c, b));
      LRN_TRY(assemble_lowrank(c, b));
      const double* Y = nullptr;
      if (n > b.npos_nz) LRN_TRY(factored_y(c, b, &Y));
      LRN_TRY(assemble_cross(c, b, Y));
      if (b.dg_n > 0) LRN_TRY(assemble_diag(c, b, Y));
    } else if (mode == 1 && b.factored && b.dg_n > 0) {     // pure block with diagonal rows (diagops.hip)
      LRN_TRY(assemble_lowrank(c, b));
      const double* Y = nullptr;
      LRN_TRY(factored_y(c, b, &Y));
      LRN_TRY(assemble_diag(c, b, Y));
    } else if (mode == 1) {
      LRN_TRY(assemble_lowrank(c, b));
    } else {
      LRN_TRY(assemble_stored(c, b));
    }
  }
  if (c->nlin > 0) {
    tic(c);
    if (c->lp_n > 0)
      hipLaunchKernelGGL(lin_schur_kernel, dim3((unsigned)((c->lp_n + 255) / 256)), dim3(256), 0, c->stream,
                         c->lp_r.as<int>(), c->lp_c.as<int>(), c->lp_ptr.as<long>(), c->lp_l.as<int>(),
                         c->lp_w.as<double>(), c->lp_n, c->lin_xs.as<double>(), c->H.as<double>(), n, c->rank, c->world,
                         c->shard_bs);
    toc(c, "lin");
  }
  timer.stop("assemble");
  LRN_HIP(c, hipGetLastError());
  c->have_H = true;
  c->H_shifted = false;
  c->have_L = false;
  c->H_version = c->scal_version;
  c->H_mode = mode;
  return LRN_OK;
}

int schur_add_diag(lrn_ctx* c, double eps) {
  if (!c->have_H) return set_error(c, LRN_ERR_STATE, "no assembled H");
  hipLaunchKernelGGL(add_diag_kernel, dim3((c->nvar + 255) / 256), dim3(256), 0, c->stream, c->H.as<double>(),
                     c->nvar, eps);
  c->have_L = false;
  if (eps != 0.0) c->H_shifted = true;
  return LRN_OK;
}

int schur_get(lrn_ctx* c, double* Hout) {
  if (!c->have_H) return set_error(c, LRN_ERR_STATE, "no assembled H");
  const int n = c->nvar;
  size_t bytes = (size_t)n * n * 8;
  LRN_TRY(ensure(c, c->slabs, bytes));     // assembly scratch doubles as staging
  const int* ipos = c->pos_space ? c->lmi[0].ipos_d.as<int>() : nullptr;
  hipLaunchKernelGGL(export_h_kernel, dim3(nb((long)n * n)), dim3(256), 0, c->stream, c->H.as<double>(), n,
                     ipos, c->slabs.as<double>());
  return copy_out(c, Hout, c->slabs.p, bytes);
}

int schur_factor(lrn_ctx* c, int* info) {
  if (!c->have_H) return set_error(c, LRN_ERR_STATE, "no assembled H");
  if (c->H_owned_only) return set_error(c, LRN_ERR_STATE, "H holds only this rank's column blocks (call lrn_schur_assemble)");
  const int n = c->nvar;
  size_t bytes = (size_t)n * n * 8;
  LRN_TRY(ensure(c, c->L, bytes));
  LRN_TRY(ensure(c, c->cholwork, chol_work_doubles(n) * 8));
  PhaseTimer timer(c, c->profile);
  // H is positive semidefinite by construction; late in a solve its smallest eigenvalues sink below the
  // rounding level of the assembly (tru9: lambda_min = -1e-3 at |H| = 4e12).  Pivots at that level are
  // boosted instead of failing the factorisation.  If more than max(8, n/64) pivots are affected the
  // attempt is abandoned and the strict factorisation decides -- this library never fails where a plain
  // Cholesky succeeds --, and once the caller has entered the reference's +1e-4 I loop (:59-85,
  // lrn_schur_add_diag) only the strict factorisation is used, as there.
  LRN_TRY(ensure(c, c->hdiag, (size_t)n * 8));
  int h_two[2] = {0, 0};
  const bool try_boost = c->opt.pivot_boost > 0.0 && !c->H_shifted;
  for (int attempt = try_boost ? 0 : 1; attempt < 2; ++attempt) {
    LRN_HIP(c, hipMemcpyAsync(c->L.p, c->H.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 8, c->stream));
    if (attempt == 0)
      hipLaunchKernelGGL(get_diag_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->H.as<double>(), n,
                         c->hdiag.as<double>());
    LRN_TRY(potrf_lower_boost(c->stream, c->L.as<double>(), n, n, c->cholwork.as<double>(), c->info_dev.as<int>(),
                              attempt == 0 ? c->hdiag.as<double>() : nullptr, c->opt.pivot_boost, std::max(8, n / 64)));
    LRN_HIP(c, hipMemcpyAsync(h_two, c->info_dev.p, 8, hipMemcpyDeviceToHost, c->stream));
    LRN_HIP(c, hipStreamSynchronize(c->stream));
    if (h_two[0] == 0) break;
  }
  timer.stop("factor");
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  const int h_info = h_two[0];
  c->counts["chol_boosted"] = h_two[1];
  if (info) *info = h_info;
  c->have_L = (h_info == 0);
  return LRN_OK;
}

int schur_solve(lrn_ctx* c, const double* h, double* dely) {
  if (!c->have_L) return set_error(c, LRN_ERR_STATE, "no factor (call lrn_schur_factor)");
  const int n = c->nvar;
  LRN_TRY(copy_in(c, c->v0.p, h, (size_t)n * 8));
  PhaseTimer timer(c, c->profile);
  const int* sig = c->pos_space ? c->lmi[0].sigma_d.as<int>() : nullptr;
  const unsigned nvb = (unsigned)((n + 255) / 256);
  // position space: hs[p] = h[sigma[p]]
  hipLaunchKernelGGL(gather_vec_kernel, dim3(nvb), dim3(256), 0, c->stream, c->v0.as<double>(), sig, c->v1.as<double>(), n);
  LRN_TRY(potrs_vec(c->stream, c->L.as<double>(), n, n, c->v1.as<double>(), c->v0.as<double>(), c->v2.as<double>(),
                    c->v3.as<double>()));
  hipLaunchKernelGGL(scatter_vec_kernel, dim3(nvb), dim3(256), 0, c->stream, c->v0.as<double>(), sig, c->v1.as<double>(), n);
  timer.stop("solve");
  return copy_out(c, dely, c->v1.p, (size_t)n * 8);
}

}  // namespace lrn
