// Schur-complement assembly from factors: rank-one data (mode -1), rank-k data (mode 1) and the cross terms of a hybrid
// factored block.  Overview: schur.hip.
#include "ops.h"
#include "fac_cols.h"
#include "schur_plan.h"

namespace lrn {

// BGt[k + h*msz] = sum_e bval_e G[bcol_e + k*msz]     (one workgroup per H-row h)
__global__ __launch_bounds__(256) void bg_kernel(const long* __restrict__ bptr, const int* __restrict__ bcol,
                                                 const double* __restrict__ bval, const double* __restrict__ G,
                                                 int msz, double* __restrict__ BGt) {
  const int h = blockIdx.x;
  const long b = bptr[h], e = bptr[h + 1];
  for (int k = threadIdx.x; k < msz; k += 256) {
    double s = 0.0;
    for (long f = b; f < e; ++f) s += bval[f] * G[(long)bcol[f] + (long)k * msz];
    BGt[(long)k + (long)h * msz] = s;
  }
}

// Bdt[k + h*msz] = B[h, k]  (dense copy of the rank-one factors, zero-filled by the caller)
__global__ void b_dense_kernel(const long* __restrict__ bptr, const int* __restrict__ bcol, const double* __restrict__ bval,
                               int msz, double* __restrict__ Bdt) {
  const int h = blockIdx.x;
  for (long f = bptr[h] + threadIdx.x; f < bptr[h + 1]; f += blockDim.x) Bdt[(long)bcol[f] + (long)h * msz] = bval[f];
}

// U[k + h*msz] = sum_e val_e M[col_e, k]  (one workgroup per factor column h): U = G' V, or U = W V from the symmetric W read
// down its columns (sym, coalesced)
__global__ __launch_bounds__(256) void lowrank_gather_kernel(const long* __restrict__ ptr, const int* __restrict__ col,
                                                             const double* __restrict__ val, const double* __restrict__ M,
                                                             int msz, int sym, double* __restrict__ U) {
  const long h = blockIdx.x;
  const long b = ptr[h], e = ptr[h + 1];
  for (int k = threadIdx.x; k < msz; k += 256) {
    double s = 0.0;
    for (long f = b; f < e; ++f) s += val[f] * (sym ? M[(long)k + (long)col[f] * msz] : M[(long)col[f] + (long)k * msz]);
    U[(long)k + h * msz] = s;
  }
}

// owned column blocks of the lower triangle of H (all of it on one GPU)
static std::vector<std::pair<int, int>> owned_cols(const lrn_ctx* c) {
  return owned_ranges(c->rank, c->world, c->shard_bs, 0, c->nvar, c->nvar);
}

int assemble_rank1(lrn_ctx* c, LmiBlock& b) {
  const int n = c->nvar, m = b.msz;
  if (!b.has_B) return set_error(c, LRN_ERR_STATE, "rank-one mode requested but no B factors were uploaded");
  // with G: H = ((BG)(BG)').^2 as the reference forms it (makeBBBB.jl:7-14); after the eigen-free scaling only W = GG'
  // exists: H = ((BW) B').^2 against a dense copy of B -- the same matrix
  const bool fromW = !b.have_G;
  if (fromW && !b.have_W) return set_error(c, LRN_ERR_STATE, "rank-one mode needs G or W (lrn_prepare_w / lrn_set_scaling)");
  LRN_TRY(ensure(c, c->BG, (size_t)m * n * 8));
  if (fromW && !b.have_Bd) {
    LRN_TRY(ensure(c, b.Bd, (size_t)m * n * 8));
    LRN_HIP(c, hipMemsetAsync(b.Bd.p, 0, (size_t)m * n * 8, c->stream));
    hipLaunchKernelGGL(b_dense_kernel, dim3(n), dim3(64), 0, c->stream, b.b_ptr.as<long>(), b.b_col.as<int>(),
                       b.b_val.as<double>(), m, b.Bd.as<double>());
    b.have_Bd = true;
  }
  tic(c);
  hipLaunchKernelGGL(bg_kernel, dim3(n), dim3(256), 0, c->stream, b.b_ptr.as<long>(), b.b_col.as<int>(),
                     b.b_val.as<double>(), fromW ? b.W.as<double>() : b.G.as<double>(), m, c->BG.as<double>());
  for (const auto& cb : owned_cols(c)) {
    const int c0 = cb.first, c1 = cb.second;
    GemmDesc g;     // H[c0:, c0:c1] += ((BG BG')[c0:, c0:c1]).^2, lower tiles of the sub-block
    g.A = c->BG.as<double>() + (long)c0 * m; g.sAm = m; g.sAk = 1;
    g.B = (fromW ? b.Bd.as<double>() : c->BG.as<double>()) + (long)c0 * m; g.sBk = 1; g.sBn = m;
    g.C = c->H.as<double>() + (long)c0 + (long)c0 * n; g.sCm = 1; g.sCn = n;
    g.M = n - c0; g.N = c1 - c0; g.K = m;
    g.beta = 1.0;
    g.flags = GEMM_TRI_LOWER | GEMM_SQUARE;
    LRN_TRY(gemm(c->stream, g));
  }
  toc(c, "rank1");
  return LRN_OK;
}

// Rank-k data (mode 1): A_k = V_k diag(d_k) V_k' with every constraint padded to khat columns (zero columns of weight 0).
// With U = G' V (or W V against the dense copy of V when only W exists, as assemble_rank1 does) and T = U' U (U' V):
//     H_ij = tr(A_i W A_j W) = sum_{p in i, q in j} d_p d_q (u_p' v_q)^2,
// the entrywise square of T weighted by d d' and summed over khat x khat blocks -- one MFMA product whose epilogue does
// all of that (GEMM_SQUARE_BLOCKSUM), T never stored.  A sign flip of a whole constraint leaves H unchanged, so the sign
// convention of AA (row j = -vec(A_j)) does not matter here.  Blocks accumulate (beta = 1) into the zeroed H.
// the dense copy Vd (msz x nvar khat) of the uploaded factors: built on first use, at lrn_set_factored for a factored block
int lowrank_dense_factors(lrn_ctx* c, LmiBlock& b) {
  if (b.have_Vd) return LRN_OK;
  if (!b.has_V) return set_error(c, LRN_ERR_STATE, "no rank-k factors were uploaded (lrn_upload_lowrank)");
  const int m = b.msz;
  const long R = (long)c->nvar * b.lr_khat;
  LRN_TRY(ensure(c, b.Vd, (size_t)m * R * 8));
  LRN_HIP(c, hipMemsetAsync(b.Vd.p, 0, (size_t)m * R * 8, c->stream));
  hipLaunchKernelGGL(b_dense_kernel, dim3((unsigned)R), dim3(64), 0, c->stream, b.v_ptr.as<long>(), b.v_col.as<int>(),
                     b.v_val.as<double>(), m, b.Vd.as<double>());
  b.have_Vd = true;
  return LRN_OK;
}

int assemble_lowrank(lrn_ctx* c, LmiBlock& b) {
  const int n = c->nvar, m = b.msz;
  if (!b.has_V) return set_error(c, LRN_ERR_STATE, "rank-k mode requested but no factors were uploaded (lrn_upload_lowrank)");
  const bool fromW = !b.have_G;
  if (fromW && !b.have_W) return set_error(c, LRN_ERR_STATE, "rank-k mode needs G or W (lrn_prepare_w / lrn_set_scaling)");
  const int kh = b.lr_khat;
  const long R = (long)n * kh;
  // option "lowrank_ragged": a block of mixed ranks by rank class (raggedops.hip) -- on one GPU and where the compaction drops
  // columns; a uniform block, an empty one and a sharded run keep the padded route below, bit for bit
  // a wide block (khat 32 or 64, option "lowrank_wide") takes that route whatever the option says, a uniform one too: the
  // blocked epilogue of the padded product below sums blocks of at most 16 x 16
  if (lowrank_wide(b)) {
    if (c->world > 1)
      return set_error(c, LRN_ERR_ARG, "rank-k mode on a wide block (khat = %d > 16) runs on one GPU (the rank-class route is not "
                                       "sharded)", kh);
    c->counts["schur_wide"] += 1;
    if (b.rg_Rc <= 0) {      // (no weighted column: nothing to add; BG holds no Y = W Vd -- factored_y forms its own product)
      c->BG_ragged = true;
      return LRN_OK;
    }
    return assemble_ragged(c, b);
  }
  if (c->opt.lowrank_ragged) {
    if (lowrank_ragged_on(c, b)) return assemble_ragged(c, b);
    c->counts["ragged_fallback"] += 1;
  }
  c->BG_ragged = false;
  const double* M = fromW ? b.W.as<double>() : b.G.as<double>();
  // U by one dense product or by a gather over the stored factor entries: the gather reads nnz * msz words of G / W, the
  // product does 2 R msz^2 flop -- the gather wins below a density of about 2 %
  const bool dense = c->opt.lowrank_form == 1 || (c->opt.lowrank_form < 0 && (double)b.vnnz > 0.02 * (double)R * m);
  if (dense || fromW) LRN_TRY(lowrank_dense_factors(c, b));
  LRN_TRY(ensure(c, c->BG, (size_t)m * R * 8));
  double* U = c->BG.as<double>();
  tic(c);
  if (dense) {
    LRN_TRY(cols_product(c, M, !fromW, b.Vd.as<double>(), R, m, U));      // U = G' Vd (or W Vd), msz x R
  } else {
    hipLaunchKernelGGL(lowrank_gather_kernel, dim3((unsigned)R), dim3(256), 0, c->stream, b.v_ptr.as<long>(),
                       b.v_col.as<int>(), b.v_val.as<double>(), M, m, fromW ? 1 : 0, U);
  }
  toc(c, "lowrank_u");     // (U alone; "lowrank" below: U and the blocked product, from the same start)
  for (const auto& cb : owned_cols(c)) {          // H column j <-> U columns j kh .. j kh + kh - 1
    const int c0 = cb.first, c1 = cb.second;
    const long u0 = (long)c0 * kh * m;
    GemmDesc g;     // H[c0:, c0:c1] += blocksum(d d' .* (U' U)[c0 kh:, c0 kh:c1 kh].^2), lower blocks
    g.A = U + u0; g.sAm = m; g.sAk = 1;
    g.B = (fromW ? b.Vd.as<double>() : U) + u0; g.sBk = 1; g.sBn = m;
    g.C = c->H.as<double>() + (long)c0 + (long)c0 * n; g.sCm = 1; g.sCn = n;
    g.M = (n - c0) * kh; g.N = (c1 - c0) * kh; g.K = m;
    g.beta = 1.0;
    g.flags = GEMM_TRI_LOWER | GEMM_SQUARE_BLOCKSUM;
    g.blk_w = b.v_w.as<double>() + (long)c0 * kh;
    g.blk_k = kh;
    LRN_TRY(gemm(c->stream, g));
  }
  toc(c, "lowrank");
  if (!c->profile) c->counts["lowrank"] += 1;     // (the route is counted whether or not the phases are timed)
  return LRN_OK;
}

// C = op(A) V into msz x R columns, op(A) = A' where transA: the one product of every route that multiplies the dense factors
// (or columns laid out like them) from the left -- U = G' V, Y = W V, Q = Z V, Q = A_s Y, P = L' V
int cols_product(lrn_ctx* c, const double* A, bool transA, const double* V, long R, int m, double* C) {
  GemmDesc g;
  g.A = A;
  if (transA) { g.sAm = m; g.sAk = 1; } else { g.sAm = 1; g.sAk = m; }
  g.B = V; g.sBk = 1; g.sBn = m;
  g.C = C; g.sCm = 1; g.sCn = m;
  g.M = m; g.N = (int)R; g.K = m;
  return gemm(c->stream, g);
}

// ---- hybrid factored block: a few constraints S are stored (positions [0, npos_nz)), the others F are factors.  H has three
// parts: H_FF by assemble_lowrank (the stored positions have weight-0 columns and receive + 0), H_SS by assemble_stored
// over the stored positions, and the cross terms, with Y = W V:
//     H_sj = tr(A_s W A_j W) = sum_p d_jp y_jp' A_s y_jp            (A_s from ent_v = +A, d from the weights = +d: the signs agree)
// over the columns p of the factored constraint j, a sparse quadratic form per column of Y, nnz(A_s) R multiply-adds per stored
// constraint.  Y is W Vd (msz x nvar khat) or, under option "ragged_cross", Yc = W Vc (msz x Rc) of a block of mixed ranks: the
// kernels are templates on the column layout (fac_cols.h), a unit the factored position p_f + x or the group x.  A constraint of
// rank 0 has no group and receives nothing (on the padded layout + 0).
//
// fac_cross_kernel: workgroup (x, y) owns unit x and the 32 sparse-tier stored positions s0 + 32 y ..; wave v takes the stored
// positions s0 + 32 y + 4 t + v, t < 8, and keeps their sums in registers.  The columns of Y of the unit are staged in LDS one at
// a time (LDS: msz * 8 bytes, dynamic, up to 32 KiB -- five workgroups per CU) or, for longer columns, gathered from global
// memory by the same code; lanes stride the entry list of A_s, one shuffle tree adds in a fixed order, the sum is weighted by
// d_jp and added over p in order, weight-0 padding skipped (uniform over the workgroup).  Each workgroup writes its 32 entries of
// the lower triangle of H exactly once, += because the blocks of a model share H.  No atomics: two assemblies give the same bits.
// LDS accesses: the staging writes are ds_write_b64 of consecutive doubles (lane l -> dwords 2 l, 2 l + 1 of a 256-dword run:
// conflict-free); the gather reads ycol[r], ycol[cc] follow the entry list of A_s, their banks are data-dependent -- an entry
// list sorted by column reads one address for cc (a broadcast) and scattered rows for r, anything from free to a multi-way
// conflict.  Derived, not measured.
template <class Cols, bool LDS>
__global__ __launch_bounds__(256) void fac_cross_kernel(const long* __restrict__ ptr, const int* __restrict__ er,
                                                        const int* __restrict__ ec, const double* __restrict__ ev,
                                                        const double* __restrict__ Y, const double* __restrict__ w, int m,
                                                        Cols lay, int s_lo, int s_hi, const int* __restrict__ hidx,
                                                        double* __restrict__ H, int ldh) {
  extern __shared__ double ycol[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  typename Cols::Span span;
  int cnt;
  if (!lay.pos_unit(blockIdx.x, hidx, &span, &cnt)) return;      // (whole workgroup)
  const int hj = lay.unit_h(blockIdx.x, span);
  const int sb = s_lo + blockIdx.y * 32 + wave;
  double acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = 0.0;
  for (int p = 0; p < cnt; ++p) {
    const long col = lay.col(span, p);
    const double wp = w[col];
    if (wp == 0.0) continue;                     // padding column (uniform over the workgroup)
    const double* __restrict__ yg = Y + col * m;
    if (LDS) {
      __syncthreads();                           // the waves are done with the previous column
      for (int r = threadIdx.x; r < m; r += 256) ycol[r] = yg[r];
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int sp = sb + 4 * t;                 // wave-uniform
      if (sp >= s_hi) continue;
      double q = 0.0;
      for (long e = ptr[sp] + lane; e < ptr[sp + 1]; e += 64) {
        const int r = er[e], cc = ec[e];
        q += ev[e] * (LDS ? ycol[r] * ycol[cc] : yg[r] * yg[cc]);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) q += __shfl_down(q, off, 64);
      acc[t] += wp * q;
    }
  }
  if (lane != 0) return;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int sp = sb + 4 * t;
    if (sp >= s_hi) continue;
    H[h_lower(hidx[sp], hj, ldh)] += acc[t];
  }
}

// stored constraint in dense slot s: Q = A_s Y is one product, H_sj = sum_p d_jp <Q(:, jp), Y(:, jp)> one wave per unit (the
// column dot of dataops.hip::fac_coldot_kernel with one accumulator), written once.  No LDS
template <class Cols>
__global__ __launch_bounds__(256) void fac_cross_coldot_kernel(const double* __restrict__ Q, const double* __restrict__ Y,
                                                               const double* __restrict__ w, int m, Cols lay, int s,
                                                               const int* __restrict__ hidx, double* __restrict__ H, int ldh) {
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
  typename Cols::Span span;
  int cnt;
  if (!lay.pos_unit(u, hidx, &span, &cnt)) return;       // (whole wave)
  double acc = 0.0;
  for (int p = 0; p < cnt; ++p) {
    const long col = lay.col(span, p);
    const double wp = w[col];
    if (wp == 0.0) continue;
    const double* __restrict__ q = Q + col * m;
    const double* __restrict__ y = Y + col * m;
    double t = 0.0;
    for (int r = lane; r < m; r += 64) t += q[r] * y[r];
    acc += wp * t;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane != 0) return;
  H[h_lower(hidx[s], lay.unit_h(u, span), ldh)] += acc;
}

// Y = W V of the current NT scaling, cached in the block until the scaling changes: Ys = W Vd (msz x nvar khat) or, compact,
// Yc = W Vc (msz x Rc).  Shared by the operator under option "fac_op_scaled" (dataops.hip) and, Yc, by factored_y below
int fac_scaled_y(lrn_ctx* c, LmiBlock& b, bool compact) {
  if (compact) LRN_TRY(ragged_setup(c, b));
  DBuf& Y = compact ? b.Yc : b.Ys;
  long& version = compact ? b.Yc_version : b.Ys_version;
  if (version == c->scal_version && Y.p) return LRN_OK;
  const FacCols v = fac_cols(c, b, compact);
  LRN_TRY(ensure(c, Y, (size_t)b.msz * v.R * 8));
  LRN_TRY(cols_product(c, b.W.as<double>(), false, v.V, v.R, b.msz, Y.as<double>()));
  version = c->scal_version;
  return LRN_OK;
}

// Y = W Vd: what the padded route of assemble_lowrank left in BG when only W exists, one more product into a workspace of its
// own otherwise.
// Formed once per assembly of a block and shared by assemble_cross and diagops.hip::assemble_diag
int factored_y(lrn_ctx* c, LmiBlock& b, const double** Yout) {
  const int n = c->nvar, m = b.msz, kh = b.lr_khat;
  const long R = (long)n * kh;
  if (!b.have_W) return set_error(c, LRN_ERR_STATE, "W not set (call lrn_prepare_w or lrn_set_scaling)");
  // option "ragged_cross": Yc = W Vc (msz x Rc) instead -- what the rank-class route left in BG when only W exists, the product
  // fac_scaled_y caches per scaling otherwise (shared with the operator under "fac_op_scaled").  assemble_cross and
  // assemble_diag ask the same condition and read the compacted layout
  if (c->opt.ragged_cross) {
    if (ragged_cross_on(c, b)) {
      LRN_TRY(ragged_setup(c, b));
      tic(c);
      if (c->BG_ragged && !b.have_G) {
        *Yout = c->BG.as<double>();
        c->counts["ragged_y_reused"] += 1;
      } else {
        LRN_TRY(fac_scaled_y(c, b, true));
        *Yout = b.Yc.as<double>();
      }
      toc(c, "hybrid_y");
      c->counts["schur_cross_ragged"] += 1;
      return LRN_OK;
    }
    c->counts["ragged_cross_fallback"] += 1;
  }
  const double* Y = c->BG.as<double>();
  tic(c);
  if (b.have_G || c->BG_ragged) {      // (after the rank-class route BG holds U_c in the compacted layout)
    LRN_TRY(ensure(c, c->facY, (size_t)m * R * 8));
    LRN_TRY(cols_product(c, b.W.as<double>(), false, b.Vd.as<double>(), R, m, c->facY.as<double>()));
    Y = c->facY.as<double>();
  }
  toc(c, "hybrid_y");
  *Yout = Y;
  return LRN_OK;
}

// the cross terms of a hybrid block from Y of factored_y, in the layout factored_y chose (ragged_cross_on)
int assemble_cross(lrn_ctx* c, LmiBlock& b, const double* Y) {
  const int n = c->nvar, m = b.msz;
  if (n - b.npos_nz <= 0) return LRN_OK;
  const bool rg = ragged_cross_on(c, b);
  if (rg) {
    if (!Y) return set_error(c, LRN_ERR_STATE, "ragged_cross: Yc = W Vc was not formed");
    LRN_TRY(ragged_setup(c, b));
  }
  const FacCols v = fac_cols(c, b, rg);
  if (v.npos <= 0) return LRN_OK;
  tic(c);
  if (b.npos_nz > b.nd) {
    const size_t cap = c->opt.fac_cross_lds == 1 ? 65536 : 32768;      // bytes of one column: forced / by default
    const bool lds = c->opt.fac_cross_lds != 0 && (size_t)m * 8 <= cap;
    const dim3 grid((unsigned)v.npos, (unsigned)((b.npos_nz - b.nd + 31) / 32));
    with_layout(c, b, v, [&](auto lay) {
      using Cols = decltype(lay);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(lds ? fac_cross_kernel<Cols, true> : fac_cross_kernel<Cols, false>), grid, dim3(256),
                         lds ? (size_t)m * 8 : 0, c->stream, b.ent_ptr.as<long>(), b.ent_r.as<int>(), b.ent_c.as<int>(),
                         b.ent_v.as<double>(), Y, v.w, m, lay, b.nd, b.npos_nz, b.hidx.as<int>(), c->H.as<double>(), n);
    });
    c->counts[lds ? "hybrid_cross_lds" : "hybrid_cross_global"] += 1;
  }
  if (b.nd > 0) {
    LRN_TRY(ensure(c, c->P, (size_t)m * v.R * 8));
    double* Q = c->P.as<double>();
    for (int s = 0; s < b.nd; ++s) {
      LRN_TRY(cols_product(c, b.Adense.as<double>() + (long)s * m * m, false, Y, v.R, m, Q));      // Q = A_s Y
      with_layout(c, b, v, [&](auto lay) {
        hipLaunchKernelGGL(fac_cross_coldot_kernel<decltype(lay)>, dim3((v.npos + 3) / 4), dim3(256), 0, c->stream, Q, Y, v.w, m,
                           lay, s, b.hidx.as<int>(), c->H.as<double>(), n);
      });
    }
    c->counts["hybrid_cross_dense"] += 1;
  }
  toc(c, "hybrid_cross");
  return LRN_OK;
}

}  // namespace lrn
