// Schur-complement assembly, dense owners (positions < nd): the Cholesky path H_ij = <L' A_i L, L' A_j L> (GEMM1', GEMM2',
// GEMM3' -- what bench.py times), the W path T_i = W A_i W and its via-L form T_i = L (L' A_i L) L', the slab reduction, the
// gather against sparse partners and the scatter of a multi-block model.  Overview: schur.hip; every launch decision of the
// Cholesky path: schur_plan.h.
#include "ops.h"
#include "schur_plan.h"

namespace lrn {

static constexpr int TS = 128;   // packing tile of the lower-stored T
static constexpr int BK_CHUNK = 16;   // K chunk of the GEMM kernels

// dense owner slot s (T stored lower tiles, strictly-lower x2) x sparse other pj
__global__ __launch_bounds__(256) void dense_sparse_gather_kernel(
    const long* __restrict__ ptr, const int* __restrict__ er, const int* __restrict__ ec,
    const double* __restrict__ ev, const double* __restrict__ T, int msz, int s0, int ns, int p_lo,
    int p_end, const int* __restrict__ hidx, double* __restrict__ H, int ldh) {
  const int s = blockIdx.y;
  if (s >= ns) return;
  const int pj = p_lo + blockIdx.x * 256 + threadIdx.x;
  if (pj >= p_end) return;
  const double* Ts = T + (long)s * msz * msz;
  double acc = 0.0;
  for (long f = ptr[pj]; f < ptr[pj + 1]; ++f) {
    int p = er[f], q = ec[f];
    int tp = p / TS, tq = q / TS;
    double t;
    if (tp == tq) t = Ts[(long)p + (long)q * msz];
    else if (tp > tq) t = 0.5 * Ts[(long)p + (long)q * msz];
    else t = 0.5 * Ts[(long)q + (long)p * msz];
    acc += ev[f] * t;
  }
  H[h_lower(hidx[s0 + s], hidx[pj], ldh)] += acc;
}

// out[i + j*ldo] += sum_s w[s] * slab_s[i + j*M]  for the BLK x BLK blocks on and below the diagonal (the others are not
// computed: lower 128-tiles of the W path, GEMM_DIAG_LOWER 16-blocks of GEMM3'); slabs in ascending order, the weight-1
// slabs (diagonal blocks of the packed operands) and the weight-2 slabs (strictly-lower blocks) summed apart: 1 / 2 are exact
template <int BLK>
__global__ void reduce_slabs_kernel(const double* __restrict__ slabs, long stride, int nslab, SlabWeights sw, int M,
                                    int N, double* __restrict__ out, long ldo) {
  long total = (long)M * N;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % M), j = (int)(e / M);
    if (i / BLK < j / BLK) continue;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < nslab; ++k) {
      const double v = slabs[(long)k * stride + e];
      if (sw.w[k] == 1.0f) s1 += v; else s2 += v;
    }
    out[(long)i + (long)j * ldo] += s1 + 2.0 * s2;
  }
}

// Ut[n + k*m] = L[k + n*m] for k >= n, else 0: the transposed lower Cholesky factor with explicit zeros
__global__ __launch_bounds__(256) void transpose_lower_kernel(const double* __restrict__ L, int m,
                                                              double* __restrict__ Ut) {
  __shared__ double tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;      // bx: rows k of L, by: columns n of L
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8) {
    int k = bx + tx, n = by + j;
    tile[j][tx] = (k < m && n < m && k >= n) ? L[(long)k + (long)n * m] : 0.0;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    int n = by + tx, k = bx + j;
    if (n < m && k < m) Ut[(long)n + (long)k * m] = tile[tx][j];
  }
}

// Hd (nd x nd, slot space, lower) scattered into H through hidx (nlmi > 1)
__global__ void scatter_add_lower_kernel(const double* __restrict__ Hd, int nd, const int* __restrict__ hidx,
                                         double* __restrict__ H, int ldh) {
  long total = (long)nd * nd;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % nd), j = (int)(e / nd);
    if (i < j) continue;
    H[h_lower(hidx[i], hidx[j], ldh)] += Hd[e];
  }
}

// ------------------------------------------------------------------ host drivers

// Where the dense x dense results go: H itself in position space; otherwise (several blocks) a zeroed nd x nd staging
// matrix in slot order, which hd_scatter adds into H through hidx once the block is done
struct HdTarget {
  double* p;
  long ld;
};
static int hd_target(lrn_ctx* c, const LmiBlock& b, HdTarget* t) {
  *t = {c->H.as<double>(), (long)c->nvar};
  if (c->pos_space) return LRN_OK;
  LRN_TRY(ensure(c, c->Hd, (size_t)b.nd * b.nd * 8, true));
  LRN_HIP(c, hipMemsetAsync(c->Hd.p, 0, (size_t)b.nd * b.nd * 8, c->stream));
  *t = {c->Hd.as<double>(), (long)b.nd};
  return LRN_OK;
}
static void hd_scatter(lrn_ctx* c, const LmiBlock& b, const HdTarget& t) {
  if (!c->pos_space)
    hipLaunchKernelGGL(scatter_add_lower_kernel, dim3(nb((long)b.nd * b.nd)), dim3(256), 0, c->stream, t.p, b.nd,
                       b.hidx.as<int>(), c->H.as<double>(), c->nvar);
}

// Claims the T workspace for block b in `layout` (lrn_ctx::T_layout).  Both layouts rely on zeros they never write -- the
// upper tiles of layout 0, the padding rows of the packed layout 1 -- which stay zero between assemblies of the SAME block
// in the same layout; a fresh allocation comes back zeroed (ensure); anything else left its data and is cleared
static int claim_T(lrn_ctx* c, const LmiBlock& b, int layout, size_t bytes) {
  const void* before = c->T.p;
  LRN_TRY(ensure(c, c->T, bytes));
  if (c->T.p == before && (c->T_layout != layout || c->T_m != b.msz || c->T_owner != &b))
    LRN_HIP(c, hipMemsetAsync(c->T.p, 0, bytes, c->stream));
  c->T_layout = layout;
  c->T_m = b.msz;
  c->T_owner = &b;
  return LRN_OK;
}

// ---- Cholesky path of the dense assembly.  With W = L L' (L lower triangular)
//        H_ij = tr(A_i W A_j W) = < L' A_i L , L' A_j L >,
// so the triangular factor replaces the two full products per constraint (3 msz^3 flop) by
//        GEMM1'  P_k  = A_k L,  lower tiles only, K from the tile's column origin   (2/3 msz^3)
//        GEMM2'  At_k = L' P_k, lower tiles only, K from the tile's row origin      (1/3 msz^3)
// and the inner products become a symmetric rank-k update over the packed lower tiles of all At_k
//        GEMM3'  H[j,i] = <At_j, At_i>   (nvar^2 msz^2 / 2, as before).
// The perturbation is that of a backward-stable Cholesky of W (||L L' - W|| <= c msz eps ||W||), the level W
// itself is known to; when the factorisation of W breaks down (W numerically singular late in a solve) the
// T_k = W A_k W path below takes over.  Multi-GPU: the columns of the matrix variable are dealt to the ranks
// (schur_plan.h::col_runs) -- all three GEMMs shard and the ranks' partial Schur matrices are summed by one all-reduce.

bool chol_path_applicable(lrn_ctx* c, LmiBlock& b, long* pcap_out) {
  if (c->opt.schur_chol == 0) return false;
  if (b.npos_nz != b.nd || b.nd < 2 || b.msz < 2) return false;   // sparse partners gather from T_k = W A_k W itself
  if (c->opt.schur_chol < 0 && b.msz < 256) return false;
  if (c->world > 1 && !c->pos_space) return false;
  // the column split deals 16-column units, whole 128-tiles at a time in GEMM1'/2': with fewer tiles than ranks the
  // Schur column blocks (all ranks busy on full tiles) win
  if (c->world > 1 && c->opt.schur_chol < 0 && (b.msz + 127) / 128 < c->world) return false;
  // multi-GPU: the ranks must enter the same collective.  Everything above is the same on every rank; the memory
  // test below is not (allocator state differs), so the host all-reduces lrn_schur_plan over the ranks and pins
  // the result with option "schur_plan" (sharding.SchurExchange) -- a pinned plan is not re-decided here.
  if (c->world > 1 && c->opt.schur_plan == 0) return false;
  const long mm = (long)b.msz * b.msz;
  long pcap = c->opt.p_batch > 0 ? c->opt.p_batch : tri_p_batch(b.msz);
  if (pcap > b.nd) pcap = b.nd;
  *pcap_out = pcap;
  if (c->world > 1 && c->opt.schur_plan == 1) return true;        // (an allocation failure is then a loud error)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  double avail = ((double)free_b + (double)c->T.bytes + (double)c->P.bytes) * 0.92;
  double need = (double)b.nd * packed_total_elems(b.msz) * 8.0 + (double)pcap * mm * 8.0 + 10.0e9;   // + split-K slabs
  if (need > avail) return false;
  if (c->opt.p_batch <= 0 && c->world == 1) {
    // fewer, larger launches of GEMM1'/2' where a tenth of the memory stays free after them
    const long big = std::min<long>(tri_p_batch(b.msz, true), b.nd);
    if (big > pcap && need + (double)(big - pcap) * mm * 8.0 + 0.10 * (double)total_b <= avail / 0.92) *pcap_out = big;
  }
  return true;
}

// W = L L' for the assembly: c->wchol = [ L (col-major, strict upper part zeroed) | Ut = L' with explicit zeros |
// potrf work ].  *ok = false when W is not numerically positive definite.
__global__ void tril_inplace_kernel(double* __restrict__ L, int m) {
  long total = (long)m * m;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % m), j = (int)(e / m);
    if (i < j) L[e] = 0.0;
  }
}

static int factor_w(lrn_ctx* c, LmiBlock& b, bool* ok) {
  const int m = b.msz;
  const long mm = (long)m * m;
  *ok = false;
  LRN_TRY(ensure(c, c->wchol, (2 * (size_t)mm + chol_work_doubles(m)) * 8));
  double* Lw = c->wchol.as<double>();
  double* Ut = Lw + mm;
  double* cw = Ut + mm;
  tic(c);
  LRN_HIP(c, hipMemcpyAsync(Lw, b.W.p, (size_t)mm * 8, hipMemcpyDeviceToDevice, c->stream));
  LRN_HIP(c, hipMemsetAsync(c->info_dev.p, 0, 8, c->stream));
  LRN_TRY(potrf_lower(c->stream, Lw, m, m, cw, c->info_dev.as<int>()));
  int h_info = 0;
  LRN_HIP(c, hipMemcpyAsync(&h_info, c->info_dev.p, 4, hipMemcpyDeviceToHost, c->stream));
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  if (h_info != 0) {
    c->counts["wchol_fail"] += 1;
    return LRN_OK;
  }
  hipLaunchKernelGGL(transpose_lower_kernel, dim3((m + 31) / 32, (m + 31) / 32), dim3(256), 0, c->stream, Lw, m, Ut);
  hipLaunchKernelGGL(tril_inplace_kernel, dim3(nb(mm)), dim3(256), 0, c->stream, Lw, m);
  toc(c, "wchol");
  *ok = true;
  return LRN_OK;
}

// The three products of the Cholesky path for the columns [c0, c1) of the plan and `nbat` matrices from slot a:
// P[c0:, c0:c1] = A[c0:, c0:] L[c0:, c0:c1] and At[c0:, c0:c1] = L[c0:, c0:]' P[c0:, c0:c1] are the same triangular products
// on the trailing blocks (L lower triangular: nothing above row c0 contributes).  Each descriptor takes its measurement-only
// options here and nowhere else.
static int chol_lab12(const LrnOptions& o) {     // GEMM1' and GEMM2' alike
  return (o.gemm_no_skip ? GEMM_NO_SKIP : 0) | (o.gemm_dyn_masks ? GEMM_DYN_MASKS : 0) | ((o.gemm_lab & 15) << 20);
}
// P = A_a L, row-major (P[i][j] at j + i*ldp), tiles i >= j, K from the tile's column origin
static GemmDesc chol_gemm1(const lrn_ctx* c, const CholPlan& pl, int m, const double* Ad, const double* Ut, double* P, int a,
                           int nbat) {
  const long mm = (long)m * m, off = (long)pl.c0 + (long)pl.c0 * m;
  GemmDesc g1;
  g1.A = Ad + (long)a * mm + off; g1.sAm = 1; g1.sAk = m; g1.bA = mm;
  g1.B = Ut + off; g1.sBk = m; g1.sBn = 1; g1.bB = 0;     // op(B)[k][j] = L[k,j] = Ut[j + k*m]
  g1.C = P; g1.sCm = pl.ldp; g1.sCn = 1; g1.bC = pl.p_elems;
  g1.M = g1.K = m - pl.c0; g1.N = pl.c1 - pl.c0; g1.batch = nbat;
  // (round 4: of the diagonal tiles of P_k GEMM2' reads only the blocks on and below the block diagonal -- the
  // others meet the stored zeros of L' -- so GEMM1' leaves them out: 28 of 64 blocks of the 16 longest tiles)
  g1.flags = GEMM_TRI_LOWER | GEMM_KFROM_N | chol_lab12(c->opt) | (c->opt.gemm1_diag ? GEMM_DIAG_LOWER_Z : 0);
  if (c->opt.gemm_lab & 32) g1.bA = 0;                       // (measurement: every batch element reads matrix 0 -- cache-resident)
  if (c->opt.gemm_lab & 16) g1.flags &= ~GEMM_KFROM_N;      // (measurement: every tile walks the whole K range -- stored zeros)
  return g1;
}
// At = L' P, tiles i >= j, K from the tile's row origin, stored packed and chunk-major: chunk q of At_k at q * cstride + 16 k
static GemmDesc chol_gemm2(const lrn_ctx* c, const CholPlan& pl, int m, const double* Ut, const double* P, double* T,
                           long cstride, int a, int nbat) {
  const long off = (long)pl.c0 + (long)pl.c0 * m;
  GemmDesc g2;
  g2.A = Ut + off; g2.sAm = 1; g2.sAk = m; g2.bA = 0;     // op(A)[i][k] = L[k,i] = Ut[i + k*m]
  g2.B = P; g2.sBk = pl.ldp; g2.sBn = 1; g2.bB = pl.p_elems;
  g2.C = T + (long)a * 16; g2.sCm = 1; g2.sCn = m; g2.bC = 16;
  g2.pk_cstride = cstride;
  g2.M = g2.K = m - pl.c0; g2.N = pl.c1 - pl.c0; g2.batch = nbat;
  g2.flags = GEMM_TRI_LOWER | GEMM_KFROM_M | GEMM_C_PACKED | chol_lab12(c->opt);
  if (c->opt.gemm_lab & 32) g2.bB = 0;
  if (c->opt.gemm_lab & 16) g2.flags &= ~GEMM_KFROM_M;
  g2.pk_m = m;
  g2.pk_off = pl.c0;
  return g2;
}
// slabs[s] = <At_j, At_i> over the chunks of split s, lower tiles (tile_class: set per launch)
static GemmDesc chol_gemm3(const lrn_ctx* c, const CholPlan& pl, int m, int nd, const double* T, long cstride, double* slabs) {
  GemmDesc g3;
  g3.A = T; g3.sAm = 16; g3.sAk = 1;
  g3.B = T; g3.sBk = 1; g3.sBn = 16;
  g3.kflat_cstride = cstride;
  g3.C = slabs; g3.sCm = 1; g3.sCn = nd;
  g3.M = nd; g3.N = nd;
  g3.flags = GEMM_TRI_LOWER | GEMM_KFLAT | GEMM_DIAG_LOWER | (c->opt.gemm_no_skip ? GEMM_NO_SKIP : 0) |
             (pl.t160 ? GEMM_TILE160 : 0) | ((c->opt.gemm_lab & 64) ? GEMM_LAB_SAME_CHUNK : 0);
  g3.kflat_total = packed_total_elems(m); g3.kflat_diag = packed_diag_elems(m); g3.kflat_nsd = 1;
  g3.kflat_kb = pl.kb; g3.kflat_ke = pl.ke;
  g3.kstagger = c->opt.gemm3_stagger;
  g3.ksplit = pl.nslab; g3.sCs = (long)nd * nd;
  return g3;
}

// (W = L L' already in c->wchol, factor_w)
static int assemble_dense_chol(lrn_ctx* c, LmiBlock& b, long pcap_hint) {
  const int m = b.msz, nd = b.nd;
  // ---- plan
  CholPlanOpts po;
  po.p_batch = c->opt.p_batch; po.gemm3_tile = c->opt.gemm3_tile; po.gemm3_ksplit = c->opt.gemm3_ksplit;
  po.gemm3_sched = c->opt.gemm3_sched; po.gemm3_strip = c->opt.gemm3_strip; po.gemm_no_skip = c->opt.gemm_no_skip;
  const CholPlan pl = plan_chol(m, nd, c->rank, c->world, pcap_hint, po);
  c->timing["gemm1_share"] = pl.gemm1_share;
  c->timing["gemm2_share"] = pl.gemm2_share;
  c->timing["gemm3_share"] = pl.gemm3_share;
  // ---- workspaces: P (a batch of blocks P_k[c0:, c0:c1]), T (all At_k, packed; its padding rows must be zero), the slabs
  const long cstride = 16L * nd;
  LRN_TRY(ensure(c, c->P, (size_t)pl.P_cap * std::max<long>(pl.p_elems, 1) * 8));
  LRN_TRY(claim_T(c, b, 1, (size_t)(packed_total_elems(m) / 16) * cstride * 8));
  if (pl.nslab > 0) LRN_TRY(ensure(c, c->slabs, (size_t)pl.nslab * nd * nd * 8));
  HdTarget hd;
  LRN_TRY(hd_target(c, b, &hd));
  // ---- launches
  const double* Ut = c->wchol.as<double>() + (long)m * m;
  double* P = c->P.as<double>();
  double* T = c->T.as<double>();
  for (int a = 0; a < nd && !pl.idle; a += (int)pl.P_cap) {
    const int nbat = std::min((int)pl.P_cap, nd - a);
    tic(c);
    LRN_TRY(gemm(c->stream, chol_gemm1(c, pl, m, b.Adense.as<double>(), Ut, P, a, nbat)));
    toc(c, "gemm1");
    tic(c);
    LRN_TRY(gemm(c->stream, chol_gemm2(c, pl, m, Ut, P, T, cstride, a, nbat)));
    toc(c, "gemm2");
  }
  // GEMM3': H (+)= sum over this rank's columns of the packed inner products -- the whole lower triangle of H,
  // a partial sum when world > 1 (the ranks' matrices are added by one all-reduce)
  GemmDesc g3 = chol_gemm3(c, pl, m, nd, T, cstride, c->slabs.as<double>());
  for (int l = 0; l < pl.ncls; ++l) {
    tic(c);
    g3.tile_class = pl.cls[l];
    LRN_TRY(gemm(c->stream, g3));
    toc(c, pl.cls[l] == 5 ? "gemm3s" : "gemm3");
  }
  tic(c);
  hipLaunchKernelGGL(reduce_slabs_kernel<16>, dim3(nb((long)nd * nd)), dim3(256), 0, c->stream, c->slabs.as<double>(),
                     (long)nd * nd, pl.nslab, pl.sw, nd, nd, hd.p, hd.ld);
  toc(c, "reduce3");
  hd_scatter(c, b, hd);
  c->counts["schur_chol"] += 1;
  if (c->world > 1) c->H_partial = true;      // H holds this rank's partial sum: all-reduce, not all-gather
  return LRN_OK;
}

int assemble_dense(lrn_ctx* c, LmiBlock& b) {
  const int m = b.msz, nd = b.nd, n = c->nvar;
  const long mm = (long)m * m;
  // Both fast paths need W = L L'.  via_l: the W path below forms T_k = L (L' A_k L) L' on triangular K ranges
  // (4 products, 2 msz^3 flop) instead of W (A_k W) (2 products, 3 msz^3); this is what blocks that also hold sparse
  // constraints run (on any number of ranks, Schur column blocks).  option schur_chol: -1 auto, 0 never factor W, 1 as auto without the size
  // thresholds, 2 T-via-L only.
  bool via_l = false;
  {
    long pcap = 0;
    const bool want_chol = c->opt.schur_chol != 2 && chol_path_applicable(c, b, &pcap);
    const bool want_via_l = c->opt.schur_chol > 0 || (c->opt.schur_chol < 0 && m >= 256);
    if (want_chol || want_via_l) LRN_TRY(factor_w(c, b, &via_l));
    if (via_l && want_chol) return assemble_dense_chol(c, b, pcap);
  }
  double* W = b.W.as<double>();
  double* Ad = b.Adense.as<double>();
  double* H = c->H.as<double>();
  // capacities, per block: blocks of one problem differ in size (a cache keyed on the context once sized
  // the P / T workspaces for the first block and let a larger later block write past them)
  if (b.t_cap == 0 || b.p_cap == 0) {
    size_t free_b = 0, total_b = 0;
    LRN_HIP(c, hipMemGetInfo(&free_b, &total_b));
    long pcap = c->opt.p_batch > 0 ? c->opt.p_batch : (via_l ? tri_p_batch(m) : pick_p_batch(m, nd));
    if (pcap > nd) pcap = nd;
    // memory that is free now plus what the shared workspaces already hold
    double avail = ((double)free_b + (double)c->T.bytes + (double)c->P.bytes + (double)c->P2.bytes) * 0.80 -
                   2.0 * (double)pcap * mm * 8.0 - 1.5e9;
    long tcap = (long)(avail / ((double)mm * 8.0));
    if (c->opt.t_batch > 0) tcap = c->opt.t_batch;
    if (tcap > nd) tcap = nd;
    if (tcap < 1) return set_error(c, LRN_ERR_NOMEM, "not enough device memory for the T workspace");
    b.p_cap = pcap;
    b.t_cap = tcap;
  }
  const long P_cap = b.p_cap, T_cap = b.t_cap;
  LRN_TRY(ensure(c, c->P, (size_t)P_cap * mm * 8));
  LRN_TRY(claim_T(c, b, 0, (size_t)T_cap * mm * 8));          // upper tiles must be zero
  double* P = c->P.as<double>();
  double* T = c->T.as<double>();
  HdTarget hd;
  LRN_TRY(hd_target(c, b, &hd));
  // owner groups: contiguous slot ranges this rank owns, each at most T_cap long and
  // starting on a 128 boundary (so that the triangular tile mask lines up)
  for (const auto& g : owned_ranges(c->rank, c->world, c->shard_bs, 0, nd, (int)T_cap)) {
    const int s0 = g.first, s1 = g.second, ns = s1 - s0;
    for (int a = s0; a < s1 && via_l; a += (int)P_cap) {
      const int nbat = std::min((int)P_cap, s1 - a);
      double* Lw = c->wchol.as<double>();
      double* Ut = Lw + mm;
      LRN_TRY(ensure(c, c->P2, (size_t)P_cap * mm * 8));
      double* P2 = c->P2.as<double>();
      tic(c);
      GemmDesc g1;   // P = A_a L, row-major, tiles i >= j, K from the tile's column origin
      g1.A = Ad + (long)a * mm; g1.sAm = 1; g1.sAk = m; g1.bA = mm;
      g1.B = Ut; g1.sBk = m; g1.sBn = 1; g1.bB = 0;
      g1.C = P; g1.sCm = m; g1.sCn = 1; g1.bC = mm;
      g1.M = g1.N = g1.K = m; g1.batch = nbat;
      g1.flags = GEMM_TRI_LOWER | GEMM_KFROM_N | (c->opt.gemm_no_skip ? GEMM_NO_SKIP : 0) |
                 (c->opt.gemm_dyn_masks ? GEMM_DYN_MASKS : 0);
      LRN_TRY(gemm(c->stream, g1));
      GemmDesc g2;   // At = L' P, tiles i >= j (K from the tile's row origin), mirrored: full symmetric, col-major
      g2.A = Ut; g2.sAm = 1; g2.sAk = m; g2.bA = 0;
      g2.B = P; g2.sBk = m; g2.sBn = 1; g2.bB = mm;
      g2.C = P2; g2.sCm = 1; g2.sCn = m; g2.bC = mm;
      g2.M = g2.N = g2.K = m; g2.batch = nbat;
      g2.flags = GEMM_TRI_LOWER | GEMM_KFROM_M | GEMM_C_MIRROR;
      LRN_TRY(gemm(c->stream, g2));
      toc(c, "gemm1");
      tic(c);
      GemmDesc g3;   // Q = L At, tiles i >= j, K up to the end of the tile's rows; col-major into P
      g3.A = Lw; g3.sAm = 1; g3.sAk = m; g3.bA = 0;
      g3.B = P2; g3.sBk = m; g3.sBn = 1; g3.bB = mm;            // At symmetric: At[k,n] read as At[n + k*m]
      g3.C = P; g3.sCm = 1; g3.sCn = m; g3.bC = mm;
      g3.M = g3.N = g3.K = m; g3.batch = nbat;
      g3.flags = GEMM_TRI_LOWER | GEMM_KTO_M;
      LRN_TRY(gemm(c->stream, g3));
      GemmDesc g4;   // T = Q L', lower tiles (strictly-lower x2), K up to the end of the tile's columns
      g4.A = P; g4.sAm = 1; g4.sAk = m; g4.bA = mm;
      g4.B = Lw; g4.sBk = m; g4.sBn = 1; g4.bB = 0;             // op(B)[k][j] = L[j,k]
      g4.C = T + (long)(a - s0) * mm; g4.sCm = 1; g4.sCn = m; g4.bC = mm;
      g4.M = g4.N = g4.K = m; g4.batch = nbat;
      g4.flags = GEMM_TRI_LOWER | GEMM_OFFDIAG_X2 | GEMM_KTO_N;
      LRN_TRY(gemm(c->stream, g4));
      toc(c, "gemm2");
      c->counts["schur_via_l"] += 1;
    }
    for (int a = s0; a < s1 && !via_l; a += (int)P_cap) {
      const int nbat = std::min((int)P_cap, s1 - a);
      tic(c);
      GemmDesc g1;   // P = A_a W, stored row-major (P^T) so that GEMM2 reads it n-contiguous;
                     // W is symmetric, so it is read as W[n + k*m]: both operands stream
                     // through the direct-to-LDS path
      g1.A = Ad + (long)a * mm; g1.sAm = 1; g1.sAk = m; g1.bA = mm;
      g1.B = W; g1.sBk = m; g1.sBn = 1; g1.bB = 0;
      g1.C = P; g1.sCm = m; g1.sCn = 1; g1.bC = mm;
      g1.M = g1.N = g1.K = m; g1.batch = nbat;
      LRN_TRY(gemm(c->stream, g1));
      toc(c, "gemm1");
      tic(c);
      GemmDesc g2;   // T = W P, lower tiles, strictly-lower x2
      g2.A = W; g2.sAm = 1; g2.sAk = m; g2.bA = 0;
      g2.B = P; g2.sBk = m; g2.sBn = 1; g2.bB = mm;
      g2.C = T + (long)(a - s0) * mm; g2.sCm = 1; g2.sCn = m; g2.bC = mm;
      g2.M = g2.N = g2.K = m; g2.batch = nbat;
      g2.flags = GEMM_TRI_LOWER | GEMM_OFFDIAG_X2;
      LRN_TRY(gemm(c->stream, g2));
      toc(c, "gemm2");
    }
    // GEMM3: Hd[s0:nd, s0:s1] += A[s0:nd]^T . T   (packed-symmetric dot, lower tiles)
    {
      tic(c);
      const int M = nd - s0, N = ns;
      long tiles = 0;
      int tM = (M + TS - 1) / TS, tN = (N + TS - 1) / TS;
      for (int tn = 0; tn < tN; ++tn) tiles += std::max(0, tM - tn);
      // prefer short workgroups, every split >= 1024 K-chunks (pick_ksplit_short)
      int ksplit = pick_ksplit_short(tiles, std::min(64, std::max(1, m / 8)), std::min(64, m / 8), (long)m * m / 2 / BK_CHUNK,
                                     1024, (double)M * N);
      if (c->opt.gemm3_ksplit > 0) ksplit = std::min(64, c->opt.gemm3_ksplit);
      LRN_TRY(ensure(c, c->slabs, (size_t)ksplit * M * N * 8));
      GemmDesc g3;
      g3.A = Ad + (long)s0 * mm; g3.sAm = mm; g3.sAk = 1;
      g3.B = T; g3.sBk = 1; g3.sBn = mm;
      g3.C = c->slabs.as<double>(); g3.sCm = 1; g3.sCn = M;
      g3.M = M; g3.N = N;
      g3.flags = GEMM_TRI_LOWER | GEMM_KSEG_TRI;
      g3.kseg_ld = m; g3.kseg_cols = m;
      g3.ksplit = ksplit; g3.sCs = (long)M * N;
      LRN_TRY(gemm(c->stream, g3));
      SlabWeights ones;
      for (int k = 0; k < ksplit; ++k) ones.w[k] = 1.0f;
      hipLaunchKernelGGL(reduce_slabs_kernel<TS>, dim3(nb((long)M * N)), dim3(256), 0, c->stream, c->slabs.as<double>(),
                         (long)M * N, ksplit, ones, M, N, hd.p + (long)s0 + (long)s0 * hd.ld, hd.ld);
      toc(c, "gemm3");
    }
    // dense owner x sparse other
    if (b.npos_nz > nd) {
      tic(c);
      int nsp = b.npos_nz - nd;
      for (int y0 = 0; y0 < ns; y0 += 32768) {
        int ny = std::min(32768, ns - y0);
        hipLaunchKernelGGL(dense_sparse_gather_kernel, dim3((nsp + 255) / 256, ny), dim3(256), 0, c->stream,
                           b.ent_ptr.as<long>(), b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(),
                           T + (long)y0 * mm, m, s0 + y0, ny, nd, b.npos_nz, b.hidx.as<int>(), H, n);
      }
      toc(c, "sparse");
    }
  }
  hd_scatter(c, b, hd);
  return LRN_OK;
}

}  // namespace lrn
