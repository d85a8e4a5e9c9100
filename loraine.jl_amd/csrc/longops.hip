// Schur assembly for long sparse stored constraints (option "pair_long"): a trace row, a weighted-trace row
// diag(a), a tridiagonal or arrow matrix -- hundreds to 3 msz entries on up to msz rows.  For an owner i with entries
// (r_e, c_e, a_e), R_i its ascending distinct rows and rho_i = |R_i|,
//     Z_i[a, x] = sum_{e : r_e = R_i[a]} a_e W[c_e, x]                      ((A_i W) on the rows R_i, rho_i x msz)
//     H_ij      = sum_f b_f sum_a Z_i[a, p_f] W[R_i[a], q_f]                (partner j with entries (p_f, q_f, b_f))
// in the convention of pair_wave_kernel (schur.hip): nnz_i msz flop once per owner and nnz_j rho_i per pair instead of
// nnz_i nnz_j gather terms on one wavefront.  Both factors of the inner sum run along a: a column of Zc_i (Z_i stored
// column-major, leading dimension ld_i = rho_i rounded up to 64, the padding rows exact zeros) and a column of W gathered
// at R_i (W is symmetric).  For a partner with local lists (support S_j of s_j <= 32 indices, Ah_j = A_j[S_j, S_j];
// model_layout.h::block_local) the same sum is  sum_{u,v} Ah_j[u, v] M[u, v],  M = Z_i[:, S_j]' W[R_i, S_j]: one s_j x s_j
// product with K = rho_i on the FP64 MFMA, every column loaded once instead of s_j times.
// No kernel here uses atomics; every sum has an order that depends on the lists and on (nnz_j, rho_i) alone.
#include <hip/hip_runtime.h>

#include "model_layout.h"
#include "ops.h"

namespace lrn {

constexpr int LG_TILE = 64;        // long_z_kernel: a 64 x 64 tile of Z through LDS
constexpr int LG_TILE_LD = 65;     //   its leading dimension (rows of x): the transposed reads of 64 lanes fall on 64 distinct bank pairs
constexpr int LG_STRIPES = 8;      // long_entry_kernel: row indices of the first 8 thread stripes (rho <= 2048) live in registers
constexpr int LG_CH = 32;          // long_local_kernel: rows of a K-chunk (ld is a multiple of 64, so chunks tile it)
constexpr int LG_LDA = LG_CH + 2;  //   leading dimension of a staged operand: see the bank rule at the kernel
static_assert(LOCAL_SUPPORT_MAX == 32, "long_local_kernel holds 2 x 2 tiles of 16");

// ---- 1. Zc of one owner batch.  grid (column tiles of msz, row tiles of ld, owners), 256 threads.
// Phase 1, lanes along x: thread (xx = t & 63, ar = t >> 6) forms Z[a0 + ar + 4 pass, x0 + xx] = the fixed-order sum over the
// entries of that row of a_e W[x + c_e msz] -- 64 consecutive addresses a wave and entry, the entry itself wave-uniform -- into
// tile[a_loc LG_TILE_LD + xx].  Phase 2, lanes along a: thread (a_loc = t & 63, xx = t >> 6 + 4 pass) stores 64 consecutive
// addresses of a column of Zc.  Rows a >= rho have no entries: exact zeros.  Bounds: x < msz masks the reads and the stores; a <
// ld always (the grid covers ld / 64 row tiles); tile index <= 63 * 65 + 63 < 64 * 65.
__global__ __launch_bounds__(256) void long_z_kernel(const long* __restrict__ rptr, const long* __restrict__ eptr,
                                                     const int* __restrict__ ec, const double* __restrict__ ev,
                                                     const double* __restrict__ W, int msz, int k0,
                                                     const long* __restrict__ zoff, double* __restrict__ Zc) {
  __shared__ double tile[LG_TILE * LG_TILE_LD];
  const int k = k0 + blockIdx.z;
  const long r0 = rptr[k];
  const int rho = (int)(rptr[k + 1] - r0);
  const long ld = ((long)rho + 63) & ~63L;
  const int a0 = blockIdx.y * LG_TILE, x0 = blockIdx.x * LG_TILE;
  if (a0 >= ld) return;
  const int t = threadIdx.x;
  {
    const int xx = t & 63, x = x0 + xx;
    for (int al = t >> 6; al < LG_TILE; al += 4) {
      const int a = a0 + al;
      double s = 0.0;
      if (a < rho && x < msz) {
        const long e1 = eptr[r0 + a + 1];
        for (long e = eptr[r0 + a]; e < e1; ++e) s += ev[e] * W[(long)x + (long)ec[e] * msz];
      }
      tile[al * LG_TILE_LD + xx] = s;
    }
  }
  __syncthreads();
  {
    const int al = t & 63;
    double* Z = Zc + zoff[k] + a0 + al;
    for (int xx = t >> 6; xx < LG_TILE; xx += 4) {
      const int x = x0 + xx;
      if (x < msz) Z[ld * x] = tile[al * LG_TILE_LD + xx];
    }
  }
}

// ---- 2. the general partner kernel: one 256-thread workgroup per work item (pi, pj, f0, f1) = a slice of consecutive entries of
// the partner.  Thread t accumulates b_f Zc[a + ld p_f] W[R[a] + q_f msz] over f = f0 .. f1 - 1 in list order and, inside,
// a = t, t + 256, ...; then the 64-lane shuffle tree, the four waves through LDS in wave order, one partial per item.
// Bounds: a < rho masks every read; p_f, q_f < msz by the upload's checks.
__global__ __launch_bounds__(256) void long_entry_kernel(const int4* __restrict__ items, long item0, int nd,
                                                         const long* __restrict__ rptr, const int* __restrict__ rows,
                                                         const long* __restrict__ zoff, const double* __restrict__ Zc,
                                                         const long* __restrict__ ptr, const int* __restrict__ er,
                                                         const int* __restrict__ ec, const double* __restrict__ ev,
                                                         const double* __restrict__ W, int msz, double* __restrict__ part) {
  __shared__ double wsum[4];
  const long it = item0 + blockIdx.x;
  const int4 w = items[it];
  const int k = w.x - nd;
  const long r0 = rptr[k];
  const int rho = (int)(rptr[k + 1] - r0);
  const long ld = ((long)rho + 63) & ~63L;
  const double* Z = Zc + zoff[k];
  const int* R = rows + r0;
  const long jb = ptr[w.y];
  const int t = threadIdx.x;
  int ra[LG_STRIPES];
#pragma unroll
  for (int s = 0; s < LG_STRIPES; ++s) {
    const int a = t + 256 * s;
    ra[s] = a < rho ? R[a] : 0;
  }
  double acc = 0.0;
  for (int f = w.z; f < w.w; ++f) {
    const double bv = ev[jb + f];
    const double* zc = Z + ld * er[jb + f];
    const double* wc = W + (long)ec[jb + f] * msz;
#pragma unroll
    for (int s = 0; s < LG_STRIPES; ++s) {
      const int a = t + 256 * s;
      if (a < rho) acc += bv * zc[a] * wc[ra[s]];
    }
    for (int a = t + 256 * LG_STRIPES; a < rho; a += 256) acc += bv * zc[a] * wc[R[a]];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((t & 63) == 0) wsum[t >> 6] = acc;
  __syncthreads();
  if (t == 0) part[it] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// the slices of a pair in ascending order, one thread per pair (pi, pj, first item, slices); the store of pair_wave_kernel
__global__ __launch_bounds__(256) void long_reduce_kernel(const int4* __restrict__ pairs, long pair0, long npairs,
                                                          const double* __restrict__ part, const int* __restrict__ hidx,
                                                          double* __restrict__ H, int ldh) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npairs) return;
  const int4 w = pairs[pair0 + i];
  double s = part[w.z];
  for (int q = 1; q < w.w; ++q) s += part[w.z + q];
  H[h_lower(hidx[w.x], hidx[w.y], ldh)] += s;
}

// ---- 3. partners with local lists: M = Z_i[:, S_j]' W[R_i, S_j] on v_mfma_f64_16x16x4_f64, 2 x 2 output tiles of 16, one
// 256-thread workgroup per pair.  Lane = (ci = lane & 15, kq = lane >> 4): A operand A[row ci][k kq], B operand B[k kq][col ci],
// accumulator register v <-> M[16 ti + kq + 4 v, 16 tj + ci] (the map test_mfma_f64_lane_map pins).
// K runs over a in chunks of LG_CH = 32 rows; wave w takes the chunks w, w + 4, ...  Per chunk the wave stages both operands,
//     ZS[al + LG_LDA u] = Zc[32 ch + al + ld S_j[u]],   WS[al + LG_LDA u] = W[R[32 ch + al] + msz S_j[u]],    u < Rj = s_j rounded up to 16,
// lanes along a (al = lane & 31, two columns a pass): every column is a run of 32 addresses of Zc, and of W where R is a run.
// Exact zeros for u >= s_j, and in WS for a >= rho (there Zc holds its zero padding: the K tail).  Then 8 K-steps of 4 rows:
// A = ZS[4 kk + kq + LG_LDA (16 ti + ci)], B = WS[4 kk + kq + LG_LDA (16 tj + ci)].
// LDS banks, derived from the bank rule (ds_read_b64: bank pair = element index mod 32, conflicts within each half of 32 lanes; not
// measured): a half-wave reads the elements kq + 34 ci, kq in {0, 1} or {2, 3}, ci < 16 -> (kq + 2 ci) mod 32, 32 distinct
// values: conflict-free.  The stores put 32 consecutive elements a half-wave: conflict-free.
// After the loop the per-wave accumulators are added through LDS in wave order (the staging area, reused behind a barrier), wave
// 0 multiplies entrywise by Ah_j in the accumulator layout (zero beyond s_j), sums per lane over (ti, tj, v) in that order,
// runs the shuffle tree, and lane 0 adds to H.
// LDS: 4 waves x 2 operands x 34 x 32 doubles = 69632 bytes.  Bounds: al + 34 u <= 31 + 34 * 31 < 34 * 32; the K-steps read rows
// below 32 and columns below Rj, which the staging has written; global reads under u < s_j and a < rho (W) or a < ld (Zc) only.
__global__ __launch_bounds__(256) void long_local_kernel(const int2* __restrict__ mf, long mf0, int nd,
                                                         const long* __restrict__ rptr, const int* __restrict__ rows,
                                                         const long* __restrict__ zoff, const double* __restrict__ Zc,
                                                         const long* __restrict__ sptr, const int* __restrict__ sup,
                                                         const long* __restrict__ aptr, const double* __restrict__ Ah,
                                                         const double* __restrict__ W, int msz, const int* __restrict__ hidx,
                                                         double* __restrict__ H, int ldh) {
  __shared__ double lds[4 * 2 * LG_LDA * 32];
  const int2 pr = mf[mf0 + blockIdx.x];
  const int k = pr.x - nd;
  const long r0 = rptr[k];
  const int rho = (int)(rptr[k + 1] - r0);
  const long ld = ((long)rho + 63) & ~63L;
  const double* Z = Zc + zoff[k];
  const int* R = rows + r0;
  const long sj0 = sptr[pr.y];
  const int s_j = (int)(sptr[pr.y + 1] - sj0);
  if (s_j <= 0) return;                                 // (an empty partner: no pair below npos_nz is one)
  const int ntj = (s_j + 15) >> 4, Rj = ntj << 4;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ci = lane & 15, kq = lane >> 4;
  const int al = lane & 31, uh = lane >> 5;
  double* ZS = lds + wv * 2 * LG_LDA * 32;
  double* WS = ZS + LG_LDA * 32;
  v4f64 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = v4f64{0.0, 0.0, 0.0, 0.0};
  const int nch = (int)(ld / LG_CH);
  for (int ch = wv; ch < nch; ch += 4) {
    const int a = ch * LG_CH + al;
    const long wrow = a < rho ? (long)R[a] : -1;
    for (int u = uh; u < Rj; u += 2) {
      double zv = 0.0, wvv = 0.0;
      if (u < s_j) {
        const long col = sup[sj0 + u];
        zv = Z[a + ld * col];
        if (wrow >= 0) wvv = W[wrow + col * msz];
      }
      ZS[al + LG_LDA * u] = zv;
      WS[al + LG_LDA * u] = wvv;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int kk = 0; kk < LG_CH / 4; ++kk) {
      double av[2], bv[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        av[tt] = tt < ntj ? ZS[4 * kk + kq + LG_LDA * (16 * tt + ci)] : 0.0;
        bv[tt] = tt < ntj ? WS[4 * kk + kq + LG_LDA * (16 * tt + ci)] : 0.0;
      }
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
          if (ti < ntj && tj < ntj) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ti], bv[tj], acc[ti][tj], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the next chunk's staging overwrites the operands
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();                                      // every wave is done with its staging area: reuse as red[wave][16][64]
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int v = 0; v < 4; ++v) lds[(wv * 16 + (ti * 2 + tj) * 4 + v) * 64 + lane] = acc[ti][tj][v];
  __syncthreads();
  if (wv != 0) return;
  const double* Aj = Ah + aptr[pr.y];
  double sum = 0.0;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int r = (ti * 2 + tj) * 4 + v;
        const double m = ((lds[r * 64 + lane] + lds[(16 + r) * 64 + lane]) + lds[(32 + r) * 64 + lane]) + lds[(48 + r) * 64 + lane];
        const int u = 16 * ti + kq + 4 * v, vv = 16 * tj + ci;
        const double ah = (u < s_j && vv < s_j) ? Aj[u + (long)vv * s_j] : 0.0;
        sum += ah * m;
      }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (lane == 0) H[h_lower(hidx[pr.x], hidx[pr.y], ldh)] += sum;
}

// ------------------------------------------------------------------ host side
static long long_zc_elems(const LmiBlock& b, int k) { return (((long)b.lg_rho[k] + 63) & ~63L) * (long)b.msz; }
static long long_cap_elems(const lrn_ctx* c) { return (long)(c->opt.pair_long_scratch_mb * 1048576.0 / 8.0); }

bool long_fits(const lrn_ctx* c, const LmiBlock& b, int lg_end) {
  const long cap = long_cap_elems(c);
  for (int k = 0; k < lg_end - b.nd; ++k)
    if (long_zc_elems(b, k) > cap) return false;
  return true;
}

// the device copies of the lists, on the first assembly that takes the route
static int long_upload(lrn_ctx* c, LmiBlock& b) {
  if (b.lg_ready) return LRN_OK;
  LRN_TRY(upload(c, b.lg_rptr_d, b.lg_rptr));
  LRN_TRY(upload(c, b.lg_rows_d, b.lg_rows));
  LRN_TRY(upload(c, b.lg_eptr_d, b.lg_eptr));
  LRN_TRY(upload(c, b.lg_ec_d, b.lg_ec));
  LRN_TRY(upload(c, b.lg_ev_d, b.lg_ev));
  for (auto* v : {&b.lg_rptr, &b.lg_eptr}) std::vector<long>().swap(*v);
  for (auto* v : {&b.lg_rows, &b.lg_ec}) std::vector<int>().swap(*v);
  std::vector<double>().swap(b.lg_ev);
  b.lg_ready = true;
  return LRN_OK;
}

// The launch plan of the owners [nd, lg_end): per owner the MFMA pairs (partners pj >= max(pi, loc_lo) when mfma), the pairs of
// the entry kernel with their slices (model_layout.h::long_slices), and the batches of owners whose Zc share the scratch.
// Rebuilt when one of its inputs changes; the tables are small beside the entry lists (16 bytes a work item).
static int long_plan(lrn_ctx* c, LmiBlock& b, int lg_end, bool mfma) {
  const long split = c->opt.pair_long_split, cap = long_cap_elems(c);
  const std::vector<long> key = {(long)lg_end, split, mfma ? 1L : 0L, cap};
  if (key == b.lg_plan_key) return LRN_OK;
  const int nown = lg_end - b.nd;
  std::vector<int4> items, pairs;
  std::vector<int2> mf;
  std::vector<long> zoff(nown, 0);
  b.lg_item_ptr.assign(1, 0);
  b.lg_pair_ptr.assign(1, 0);
  b.lg_mf_ptr.assign(1, 0);
  b.lg_batch.assign(1, 0);
  long used = 0;
  for (int k = 0; k < nown; ++k) {
    const int pi = b.nd + k;
    const long need = long_zc_elems(b, k);
    if (used + need > cap && used > 0) { b.lg_batch.push_back(k); used = 0; }
    zoff[k] = used;
    used += need;
    for (int pj = pi; pj < b.npos_nz; ++pj) {
      if (mfma && pj >= b.loc_lo) { mf.push_back(int2{pi, pj}); continue; }
      long per = 0;
      const int ns = long_slices(b.nnz[pj], b.lg_rho[k], split, &per);
      pairs.push_back(int4{pi, pj, (int)items.size(), ns});
      for (int s = 0; s < ns; ++s)
        items.push_back(int4{pi, pj, (int)(s * per), (int)std::min<long>((s + 1) * per, b.nnz[pj])});
    }
    b.lg_item_ptr.push_back((long)items.size());
    b.lg_pair_ptr.push_back((long)pairs.size());
    b.lg_mf_ptr.push_back((long)mf.size());
  }
  b.lg_batch.push_back(nown);
  if (items.size() >= 2000000000UL) return set_error(c, LRN_ERR_STATE, "pair_long: too many work items");
  LRN_TRY(upload(c, b.lg_items_d, items));
  LRN_TRY(upload(c, b.lg_pairs_d, pairs));
  LRN_TRY(upload(c, b.lg_mf_d, mf));
  LRN_TRY(upload(c, b.lg_zoff_d, zoff));
  LRN_TRY(ensure(c, b.lg_part, items.size() * sizeof(double)));
  b.lg_plan_key = key;
  return LRN_OK;
}

int assemble_long(lrn_ctx* c, LmiBlock& b, int lg_end) {
  const bool mfma = c->opt.pair_long_mfma != 0 && b.loc_hi > b.loc_lo;      // the block's local lists exist
  LRN_TRY(long_upload(c, b));
  if (mfma) LRN_TRY(local_upload(c, b));
  LRN_TRY(long_plan(c, b, lg_end, mfma));
  long zmax = 0;
  for (size_t q = 0; q + 1 < b.lg_batch.size(); ++q) {
    long z = 0;
    for (int k = b.lg_batch[q]; k < b.lg_batch[q + 1]; ++k) z += long_zc_elems(b, k);
    zmax = std::max(zmax, z);
  }
  LRN_TRY(ensure(c, b.lg_z, (size_t)zmax * sizeof(double)));
  tic(c);
  const long* rptr = b.lg_rptr_d.as<long>();
  const int* rows = b.lg_rows_d.as<int>();
  const long* zoff = b.lg_zoff_d.as<long>();
  double* Zc = b.lg_z.as<double>();
  const double* W = b.W.as<double>();
  double* H = c->H.as<double>();
  for (size_t q = 0; q + 1 < b.lg_batch.size(); ++q) {
    const int k0 = b.lg_batch[q], k1 = b.lg_batch[q + 1];
    int rho_max = 0;
    for (int k = k0; k < k1; ++k) rho_max = std::max(rho_max, b.lg_rho[k]);
    for (int ka = k0; ka < k1; ka += 16384) {             // (grid.z is limited to 65535)
      dim3 grid((b.msz + LG_TILE - 1) / LG_TILE, (rho_max + LG_TILE - 1) / LG_TILE, std::min(k1 - ka, 16384));
      hipLaunchKernelGGL(long_z_kernel, grid, dim3(256), 0, c->stream, rptr, b.lg_eptr_d.as<long>(), b.lg_ec_d.as<int>(),
                         b.lg_ev_d.as<double>(), W, b.msz, ka, zoff, Zc);
    }
    const long i0 = b.lg_item_ptr[k0], ni = b.lg_item_ptr[k1] - i0;
    const long p0 = b.lg_pair_ptr[k0], np = b.lg_pair_ptr[k1] - p0;
    const long m0 = b.lg_mf_ptr[k0], nm = b.lg_mf_ptr[k1] - m0;
    if (ni > 0) {
      hipLaunchKernelGGL(long_entry_kernel, dim3((unsigned)ni), dim3(256), 0, c->stream, b.lg_items_d.as<int4>(), i0, b.nd, rptr,
                         rows, zoff, Zc, b.ent_ptr.as<long>(), b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(), W,
                         b.msz, b.lg_part.as<double>());
      hipLaunchKernelGGL(long_reduce_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream,
                         b.lg_pairs_d.as<int4>(), p0, np, b.lg_part.as<double>(), b.hidx.as<int>(), H, c->nvar);
    }
    if (nm > 0)
      hipLaunchKernelGGL(long_local_kernel, dim3((unsigned)nm), dim3(256), 0, c->stream, b.lg_mf_d.as<int2>(), m0, b.nd, rptr, rows,
                         zoff, Zc, b.loc_sptr_d.as<long>(), b.loc_sup_d.as<int>(), b.loc_aptr_d.as<long>(), b.loc_a_d.as<double>(),
                         W, b.msz, b.hidx.as<int>(), H, c->nvar);
  }
  LRN_HIP(c, hipGetLastError());
  toc(c, "long");
  const int nown = lg_end - b.nd;
  c->counts["pair_long_owners"] += nown;
  c->counts["pair_long_pairs"] += b.lg_pair_ptr[nown] + b.lg_mf_ptr[nown];
  c->counts["pair_long_mfma_pairs"] += b.lg_mf_ptr[nown];
  c->counts["pair_long_slices"] += b.lg_item_ptr[nown];
  return LRN_OK;
}

}  // namespace lrn
