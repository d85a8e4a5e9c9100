// Context helpers, model upload (reference MyModel -> device layout), synthetic generator and the synthetic problem on top of it.
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <algorithm>
#include <numeric>

#include "ctx.h"
#include "ops.h"
#include "ragged_plan.h"

namespace lrn {

int set_error(lrn_ctx* c, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  (void)hipGetLastError();
  return code;
}

int ensure(lrn_ctx* c, DBuf& b, size_t bytes, bool zero) {
  if (bytes == 0) bytes = 8;
  if (b.bytes < bytes) {
    if (b.p) (void)hipFree(b.p);
    if (b.acct) *b.acct -= b.bytes;
    b.p = nullptr;
    b.bytes = 0;
    b.acct = nullptr;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess)
      return set_error(c, LRN_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    b.bytes = bytes;
    if (c) {
      b.acct = &c->dev_bytes;
      c->dev_bytes += bytes;
      c->dev_bytes_peak = std::max(c->dev_bytes_peak, c->dev_bytes);
    }
    zero = true;
  }
  if (zero) LRN_HIP(c, hipMemsetAsync(b.p, 0, b.bytes, c->stream));
  return LRN_OK;
}

void release(DBuf& b) {
  if (b.p) (void)hipFree(b.p);
  if (b.p && b.acct) *b.acct -= b.bytes;
  b.p = nullptr;
  b.bytes = 0;
  b.acct = nullptr;
}

bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// Column-block width of the Schur sharding.  Auto: two blocks per rank (the snake map pairs a long early
// block with a short late one, so two are enough to balance the triangle), rounded up to the 128-column
// tile: the owner's GEMM3 then streams the constraint data twice instead of once per 128 columns.
void update_shard_bs(lrn_ctx* c) {
  int bs = 128;
  if (c->shard_bs_opt > 0) bs = c->shard_bs_opt;
  else if (c->world > 1 && c->nvar > 0) {
    int per = (c->nvar + 2 * c->world - 1) / (2 * c->world);
    bs = std::max(128, ((per + 127) / 128) * 128);
  }
  c->shard_bs = bs;
  c->counts["shard_bs"] = bs;
}

int copy_in(lrn_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return LRN_OK;
  if (!src || !dst) return set_error(c, LRN_ERR_ARG, "copy_in: null pointer");
  hipMemcpyKind k = is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  LRN_HIP(c, hipMemcpyAsync(dst, src, bytes, k, c->stream));
  if (k == hipMemcpyHostToDevice) LRN_HIP(c, hipStreamSynchronize(c->stream));
  return LRN_OK;
}

int copy_out(lrn_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return LRN_OK;
  if (!src || !dst) return set_error(c, LRN_ERR_ARG, "copy_out: null pointer");
  hipMemcpyKind k = is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  LRN_HIP(c, hipMemcpyAsync(dst, src, bytes, k, c->stream));
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  return LRN_OK;
}

void tic(lrn_ctx* c) {
  if (c->profile) (void)hipEventRecord(c->ev0, c->stream);
}
void toc(lrn_ctx* c, const char* key) {
  if (!c->profile) return;
  (void)hipEventRecord(c->ev1, c->stream);
  (void)hipEventSynchronize(c->ev1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
  c->timing[key] += ms;
  c->counts[key] += 1;
}

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

// Philox4x32-10 (Salmon et al. 2011), counter = (k, hi, lo, 0), key = seed
__device__ inline void philox4x32(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    uint32_t n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

__device__ inline double synth_entry(uint64_t seed, int k, int r, int cc) {
  int hi = r > cc ? r : cc, lo = r > cc ? cc : r;
  uint32_t c[4] = {(uint32_t)k, (uint32_t)hi, (uint32_t)lo, 0u};
  philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double two32 = 4294967296.0;
  double u1 = ((double)c[0] + 0.5) / two32, u2 = ((double)c[1] + 0.5) / two32;
  double u3 = ((double)c[2] + 0.5) / two32, u4 = ((double)c[3] + 0.5) / two32;
  double z0 = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
  double z1 = sqrt(-2.0 * log(u3)) * cospi(2.0 * u4);
  return hi == lo ? z0 : 0.5 * (z0 + z1);
}

__global__ void synth_dense_kernel(double* __restrict__ Ad, int msz, int k0, int nk, uint64_t seed) {
  long per = (long)msz * msz;
  long total = per * nk;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int kk = (int)(e / per);
    long q = e - (long)kk * per;
    int r = (int)(q % msz), cc = (int)(q / msz);
    Ad[(long)(k0 + kk) * per + q] = synth_entry(seed, k0 + kk, r, cc);
  }
}

// X0 = Q Q' / n + I and out = sgn M + I of the synthetic problem (lrn_synthetic_dense_problem)
__global__ void synth_x0_kernel(double* __restrict__ X, const double* __restrict__ Q, int n, int r) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int i = (int)(e % n), j = (int)(e / n);
    double s = 0.0;
    for (int k = 0; k < r; ++k) s += Q[i + (long)k * n] * Q[j + (long)k * n];
    X[e] = s / n + (i == j ? 1.0 : 0.0);
  }
}
__global__ void eye_add_kernel(double* __restrict__ out, const double* __restrict__ M, double sgn, int n) {
  long total = (long)n * n;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
    out[e] = sgn * M[e] + ((int)(e % n) == (int)(e / n) ? 1.0 : 0.0);
}

__global__ void build_constraint_kernel(const long* __restrict__ ptr, const int* __restrict__ er,
                                        const int* __restrict__ ec, const double* __restrict__ ev,
                                        int pos, double* __restrict__ out, int msz) {
  long b = ptr[pos], e = ptr[pos + 1];
  for (long k = b + (long)blockIdx.x * blockDim.x + threadIdx.x; k < e; k += (long)gridDim.x * blockDim.x)
    out[(long)er[k] + (long)ec[k] * msz] = ev[k];
}

}  // namespace lrn

using namespace lrn;

static void free_block(LmiBlock& b) {
  release(b.tri_tab);
  b.tri_nch = 0;
  b.dense_route = LmiBlock::DENSE_SCALAR;      // (Adense goes below)
  for (DBuf* d : {&b.ent_ptr, &b.ent_r, &b.ent_c, &b.ent_v, &b.Adense, &b.hidx, &b.sigma_d, &b.ipos_d, &b.cq_q, &b.cq_ptr, &b.cq_j, &b.cq_v, &b.pc_ptr, &b.pc_r, &b.pc_t, &b.ent_t, &b.Mv, &b.Zs, &b.b_ptr, &b.b_col,
                  &b.b_val, &b.X, &b.S, &b.W, &b.G, &b.Gi, &b.Si, &b.D, &b.DDsi, &b.Vprev, &b.Cd, &b.Rd, &b.delX, &b.delS, &b.Xn, &b.Sn, &b.RNT,
                  &b.t0, &b.t1, &b.t2, &b.LXf, &b.LXt, &b.LSf, &b.Yh, &b.Zh, &b.Ki, &b.Bs, &b.TX, &b.Qm, &b.lyap, &b.Bd, &b.v_ptr, &b.v_col, &b.v_val, &b.v_w, &b.Vd, &b.Ys,
                  &b.rg_src, &b.rg_wc, &b.rg_gh, &b.rg_hg, &b.rg_tiles, &b.rg_cg, &b.Vc, &b.Yc, &b.dg_h, &b.dg_nat, &b.dg_of_pos, &b.dg_a})
    release(*d);
  b.dg_n = 0;
  b.rg_ready = false;
  b.Yc_version = -1;
  b.rg_Rc = b.rg_ntiles = 0;
}

void lrn_free_model(lrn_ctx* c) {
  for (auto& b : c->lmi) free_block(b);
  c->lmi.clear();
  for (DBuf* d : {&c->cl_ptr, &c->cl_row, &c->cl_val, &c->lin_xs, &c->H, &c->L, &c->cholwork,
                  &c->v0, &c->v1, &c->v2, &c->v3, &c->P, &c->P2, &c->T, &c->slabs, &c->Hd, &c->BG, &c->m0, &c->m1, &c->m2, &c->cgbuf, &c->facY, &c->facM, &c->dgP, &c->dgC, &c->dgH, &c->dgT, &c->dgTA, &c->cl_rown,
                  &c->hdiag, &c->wchol, &c->lp_r, &c->lp_c, &c->lp_ptr, &c->lp_l, &c->lp_w, &c->cr_ptr, &c->cr_col, &c->cr_val})
    release(*d);
  c->T_m = 0;
  c->T_owner = nullptr;
  c->T_layout = 0;
  c->have_H = c->have_L = false;
  c->nlmi = c->nvar = c->nlin = 0;
}


static int alloc_common(lrn_ctx* c) {
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
    const long ncol = (long)m * m;
    const int64_t* cp = AA_colptr[il];
    const int64_t* rv = AA_rowval[il];
    const double* nz = AA_nzval[il];
    // per-constraint counts
    std::vector<long> cnt(nvar, 0);
    long nnz_total = cp[ncol] - cp[0];
    for (long q = 0; q < ncol; ++q)
      for (long k = cp[q] - 1; k < cp[q + 1] - 1; ++k) {
        long j = rv[k] - 1;
        if (j < 0 || j >= nvar) return set_error(c, LRN_ERR_ARG, "AA rowval out of range");
        if (nz[k] != 0.0) cnt[j]++;
      }
    (void)nnz_total;
    b.sigma.resize(nvar);
    b.ipos.assign(nvar, -1);
    b.nnz.resize(nvar);
    for (int p = 0; p < nvar; ++p) {
      long s = sigmaA[(long)il * nvar + p] - 1;
      if (s < 0 || s >= nvar || b.ipos[s] != -1) return set_error(c, LRN_ERR_ARG, "sigmaA is not a permutation");
      b.sigma[p] = (int)s;
      b.ipos[s] = p;
      b.nnz[p] = cnt[s];
    }
    for (int p = 1; p < nvar; ++p)
      if (b.nnz[p] > b.nnz[p - 1])
        return set_error(c, LRN_ERR_ARG, "sigmaA is not sorted by decreasing nnz (model.jl:159)");
    b.qA = (int)qA[2 * il];
    if (b.qA < 0) b.qA = 0;
    if (b.qA > nvar) b.qA = nvar;
    b.npos_nz = 0;
    while (b.npos_nz < nvar && b.nnz[b.npos_nz] > 0) b.npos_nz++;
    // entry lists in position order
    std::vector<long> ptr(nvar + 1, 0);
    for (int p = 0; p < nvar; ++p) ptr[p + 1] = ptr[p] + b.nnz[p];
    b.nent = ptr[nvar];
    std::vector<int> er(b.nent), ec(b.nent);
    std::vector<double> ev(b.nent);
    std::vector<long> fill(ptr.begin(), ptr.end() - 1);
    for (long q = 0; q < ncol; ++q)
      for (long k = cp[q] - 1; k < cp[q + 1] - 1; ++k) {
        if (nz[k] == 0.0) continue;
        int p = b.ipos[rv[k] - 1];
        long w = fill[p]++;
        er[w] = (int)(q % m);
        ec[w] = (int)(q / m);
        ev[w] = -nz[k];     // AA = -A  (model.jl:219)
      }
    // dense (MFMA) prefix by cost model: pair path cost nnz_p * suffix_nnz vs 3 m^3 GEMM work
    {
      std::vector<double> suffix(nvar + 1, 0.0);
      for (int p = nvar - 1; p >= 0; --p) suffix[p] = suffix[p + 1] + (double)b.nnz[p];
      size_t free_b = 0, total_b = 0;
      (void)hipMemGetInfo(&free_b, &total_b);
      long max_dense = (long)((double)free_b * 0.55 / ((double)m * m * 8.0));
      int nd = 0;
      for (int p = 0; p < b.qA && p < b.npos_nz; ++p) {
        bool dense;
        if (c->opt.dense_threshold >= 0) {
          dense = (double)b.nnz[p] >= c->opt.dense_threshold;
        } else {
          double pair_cost = (double)b.nnz[p] * suffix[p] / 1.0e11;
          double dense_cost = 3.0 * m * (double)m * m / 2.0e13 + (double)(nvar - p) * m * (double)m / 2.0e13 + 2e-5;
          dense = pair_cost > dense_cost;
        }
        if (!dense || nd >= max_dense) break;
        nd = p + 1;
      }
      b.nd = nd;
    }
    b.q_wave = b.nd;
    while (b.q_wave < b.npos_nz && b.nnz[b.q_wave] > 4) b.q_wave++;
    {  // stored columns of AA restricted to the non-dense constraints
      std::vector<long> cq_q, cq_ptr(1, 0);
      std::vector<int> cq_j;
      std::vector<double> cq_v;
      for (long q = 0; q < ncol; ++q) {
        long before = (long)cq_j.size();
        for (long k = cp[q] - 1; k < cp[q + 1] - 1; ++k) {
          if (nz[k] == 0.0) continue;
          long j = rv[k] - 1;
          if (b.ipos[j] < b.nd) continue;
          cq_j.push_back((int)j);
          cq_v.push_back(nz[k]);
        }
        if ((long)cq_j.size() > before) { cq_q.push_back(q); cq_ptr.push_back((long)cq_j.size()); }
      }
      b.ncq = (long)cq_q.size();
      LRN_TRY(ensure(c, b.cq_q, (size_t)b.ncq * 8));
      LRN_TRY(ensure(c, b.cq_ptr, (size_t)(b.ncq + 1) * 8));
      LRN_TRY(ensure(c, b.cq_j, cq_j.size() * 4));
      LRN_TRY(ensure(c, b.cq_v, cq_v.size() * 8));
      LRN_TRY(copy_in(c, b.cq_q.p, cq_q.data(), (size_t)b.ncq * 8));
      LRN_TRY(copy_in(c, b.cq_ptr.p, cq_ptr.data(), (size_t)(b.ncq + 1) * 8));
      LRN_TRY(copy_in(c, b.cq_j.p, cq_j.data(), cq_j.size() * 4));
      LRN_TRY(copy_in(c, b.cq_v.p, cq_v.data(), cq_v.size() * 8));
      // pattern of mat(AA'x) for the sparse-aware mat-vec
      b.sp_ok = false;
      if (b.nd == 0 && b.ncq > 0 && b.ncq < 2000000000L && b.nent < 2000000000L) {
        const long nq = b.ncq;
        std::vector<long> pcp(m + 1, 0);
        std::vector<int> pr(nq), pt(nq), et(b.nent);
        for (long t = 0; t < nq; ++t) {
          pr[t] = (int)(cq_q[t] % m);
          pcp[cq_q[t] / m + 1]++;
        }
        for (long q = 0; q < m; ++q) pcp[q + 1] += pcp[q];
        bool sym = true;
        for (long t = 0; t < nq && sym; ++t) {
          long key = cq_q[t] / m + (cq_q[t] % m) * m;       // (col, row) swapped
          auto it = std::lower_bound(cq_q.begin(), cq_q.end(), key);
          if (it == cq_q.end() || *it != key) sym = false;
          else pt[t] = (int)(it - cq_q.begin());
        }
        for (long e = 0; e < b.nent && sym; ++e) {
          long key = (long)er[e] + (long)ec[e] * m;
          auto it = std::lower_bound(cq_q.begin(), cq_q.end(), key);
          if (it == cq_q.end() || *it != key) sym = false;
          else et[e] = (int)(it - cq_q.begin());
        }
        if (sym) {
          LRN_TRY(ensure(c, b.pc_ptr, (size_t)(m + 1) * 8));
          LRN_TRY(ensure(c, b.pc_r, (size_t)nq * 4));
          LRN_TRY(ensure(c, b.pc_t, (size_t)nq * 4));
          LRN_TRY(ensure(c, b.ent_t, (size_t)b.nent * 4));
          LRN_TRY(ensure(c, b.Mv, (size_t)nq * 8));
          LRN_TRY(ensure(c, b.Zs, (size_t)nq * 8));
          LRN_TRY(copy_in(c, b.pc_ptr.p, pcp.data(), (size_t)(m + 1) * 8));
          LRN_TRY(copy_in(c, b.pc_r.p, pr.data(), (size_t)nq * 4));
          LRN_TRY(copy_in(c, b.pc_t.p, pt.data(), (size_t)nq * 4));
          LRN_TRY(copy_in(c, b.ent_t.p, et.data(), (size_t)b.nent * 4));
          b.sp_ok = true;
          // columns of the pattern with many entries (sp_wm_long_kernel, dataops.hip)
          b.sp_long_cols.clear();
          for (long q = 0; q < m; ++q)
            if (pcp[q + 1] - pcp[q] > 64) b.sp_long_cols.push_back((int)q);
        }
      }
    }
    LRN_TRY(ensure(c, b.ent_ptr, (size_t)(nvar + 1) * 8));
    LRN_TRY(ensure(c, b.ent_r, (size_t)b.nent * 4));
    LRN_TRY(ensure(c, b.ent_c, (size_t)b.nent * 4));
    LRN_TRY(ensure(c, b.ent_v, (size_t)b.nent * 8));
    LRN_TRY(copy_in(c, b.ent_ptr.p, ptr.data(), (size_t)(nvar + 1) * 8));
    LRN_TRY(copy_in(c, b.ent_r.p, er.data(), (size_t)b.nent * 4));
    LRN_TRY(copy_in(c, b.ent_c.p, ec.data(), (size_t)b.nent * 4));
    LRN_TRY(copy_in(c, b.ent_v.p, ev.data(), (size_t)b.nent * 8));
    std::vector<int> hidx(nvar);
    for (int p = 0; p < nvar; ++p) hidx[p] = c->pos_space ? p : b.sigma[p];
    LRN_TRY(ensure(c, b.hidx, (size_t)nvar * 4));
    LRN_TRY(copy_in(c, b.hidx.p, hidx.data(), (size_t)nvar * 4));
    LRN_TRY(ensure(c, b.sigma_d, (size_t)nvar * 4));
    LRN_TRY(ensure(c, b.ipos_d, (size_t)nvar * 4));
    LRN_TRY(copy_in(c, b.sigma_d.p, b.sigma.data(), (size_t)nvar * 4));
    LRN_TRY(copy_in(c, b.ipos_d.p, b.ipos.data(), (size_t)nvar * 4));
    if (b.nd > 0) {
      LRN_TRY(ensure(c, b.Adense, (size_t)b.nd * m * m * 8, true));
      hipLaunchKernelGGL(scatter_dense_kernel, dim3(64, b.nd), dim3(256), 0, c->stream,
                         b.ent_ptr.as<long>(), b.ent_r.as<int>(), b.ent_c.as<int>(), b.ent_v.as<double>(),
                         b.Adense.as<double>(), m);
    }
    LRN_TRY(dense_route_setup(c, b, false));
    // rank-one factors, rows reordered to H index order
    b.has_B = false;
    if (B_colptr && B_colptr[il] && B_rowval && B_nzval) {
      const int64_t* bc = B_colptr[il];
      const int64_t* br = B_rowval[il];
      const double* bv = B_nzval[il];
      std::vector<long> bcnt(nvar, 0);
      for (long q = 0; q < m; ++q)
        for (long k = bc[q] - 1; k < bc[q + 1] - 1; ++k) bcnt[br[k] - 1]++;
      // row index in H space
      std::vector<long> bptr(nvar + 1, 0);
      std::vector<int> hrow(nvar);
      for (int j = 0; j < nvar; ++j) hrow[j] = c->pos_space ? b.ipos[j] : j;
      std::vector<long> cnt_h(nvar, 0);
      for (int j = 0; j < nvar; ++j) cnt_h[hrow[j]] = bcnt[j];
      for (int h = 0; h < nvar; ++h) bptr[h + 1] = bptr[h] + cnt_h[h];
      b.bnnz = bptr[nvar];
      std::vector<int> bcol(b.bnnz);
      std::vector<double> bval(b.bnnz);
      std::vector<long> bf(bptr.begin(), bptr.end() - 1);
      for (long q = 0; q < m; ++q)
        for (long k = bc[q] - 1; k < bc[q + 1] - 1; ++k) {
          int h = hrow[br[k] - 1];
          long w = bf[h]++;
          bcol[w] = (int)q;
          bval[w] = bv[k];
        }
      LRN_TRY(ensure(c, b.b_ptr, (size_t)(nvar + 1) * 8));
      LRN_TRY(ensure(c, b.b_col, (size_t)b.bnnz * 4));
      LRN_TRY(ensure(c, b.b_val, (size_t)b.bnnz * 8));
      LRN_TRY(copy_in(c, b.b_ptr.p, bptr.data(), (size_t)(nvar + 1) * 8));
      LRN_TRY(copy_in(c, b.b_col.p, bcol.data(), (size_t)b.bnnz * 4));
      LRN_TRY(copy_in(c, b.b_val.p, bval.data(), (size_t)b.bnnz * 8));
      b.has_B = b.bnnz > 0;
    }
  }
  if (nlin > 0) {
    if (!Clin_colptr || !Clin_rowval || !Clin_nzval) return set_error(c, LRN_ERR_ARG, "null C_lin");
    long nn = Clin_colptr[nlin] - 1;
    std::vector<long> ptr(nlin + 1);
    for (int l = 0; l <= nlin; ++l) ptr[l] = Clin_colptr[l] - 1;
    std::vector<int> row(nn), rown(nn);
    for (long k = 0; k < nn; ++k) {
      long i = Clin_rowval[k] - 1;
      if (i < 0 || i >= nvar) return set_error(c, LRN_ERR_ARG, "C_lin rowval out of range");
      row[k] = c->pos_space ? c->lmi[0].ipos[i] : (int)i;
      rown[k] = (int)i;
    }
    LRN_TRY(ensure(c, c->cl_rown, (size_t)nn * 4));
    LRN_TRY(copy_in(c, c->cl_rown.p, rown.data(), (size_t)nn * 4));
    LRN_TRY(ensure(c, c->cl_ptr, (size_t)(nlin + 1) * 8));
    LRN_TRY(ensure(c, c->cl_row, (size_t)nn * 4));
    LRN_TRY(ensure(c, c->cl_val, (size_t)nn * 8));
    LRN_TRY(copy_in(c, c->cl_ptr.p, ptr.data(), (size_t)(nlin + 1) * 8));
    LRN_TRY(copy_in(c, c->cl_row.p, row.data(), (size_t)nn * 4));
    LRN_TRY(copy_in(c, c->cl_val.p, Clin_nzval, (size_t)nn * 8));
    LRN_TRY(ensure(c, c->lin_xs, (size_t)nlin * 8, true));
    {  // gather lists: every lower-triangle target (ri >= rj) of C_lin diag(xs) C_lin' with its (l, C_il C_jl)
      struct Con { int r, c, l; double w; };
      std::vector<Con> cons;
      for (int l = 0; l < nlin; ++l)
        for (long a = ptr[l]; a < ptr[l + 1]; ++a)
          for (long bq = ptr[l]; bq < ptr[l + 1]; ++bq)
            if (row[a] >= row[bq]) cons.push_back({row[a], row[bq], l, Clin_nzval[a] * Clin_nzval[bq]});
      std::stable_sort(cons.begin(), cons.end(), [](const Con& x, const Con& y) { return x.c != y.c ? x.c < y.c : x.r < y.r; });
      std::vector<int> pr, pc, pl(cons.size());
      std::vector<long> pp(1, 0);
      std::vector<double> pw(cons.size());
      for (size_t k = 0; k < cons.size(); ++k) {
        if (k == 0 || cons[k].r != cons[k - 1].r || cons[k].c != cons[k - 1].c) {
          if (k > 0) pp.push_back((long)k);
          pr.push_back(cons[k].r); pc.push_back(cons[k].c);
        }
        pl[k] = cons[k].l; pw[k] = cons[k].w;
      }
      pp.push_back((long)cons.size());
      c->lp_n = (long)pr.size();
      LRN_TRY(ensure(c, c->lp_r, pr.size() * 4 + 4));
      LRN_TRY(ensure(c, c->lp_c, pc.size() * 4 + 4));
      LRN_TRY(ensure(c, c->lp_ptr, pp.size() * 8));
      LRN_TRY(ensure(c, c->lp_l, pl.size() * 4 + 4));
      LRN_TRY(ensure(c, c->lp_w, pw.size() * 8 + 8));
      LRN_TRY(copy_in(c, c->lp_r.p, pr.data(), pr.size() * 4));
      LRN_TRY(copy_in(c, c->lp_c.p, pc.data(), pc.size() * 4));
      LRN_TRY(copy_in(c, c->lp_ptr.p, pp.data(), pp.size() * 8));
      LRN_TRY(copy_in(c, c->lp_l.p, pl.data(), pl.size() * 4));
      LRN_TRY(copy_in(c, c->lp_w.p, pw.data(), pw.size() * 8));
      // C_lin by natural rows
      std::vector<long> rp(nvar + 1, 0);
      for (long k = 0; k < nn; ++k) rp[rown[k] + 1]++;
      for (int i = 0; i < nvar; ++i) rp[i + 1] += rp[i];
      std::vector<long> fill(rp.begin(), rp.end() - 1);
      std::vector<int> rc(nn);
      std::vector<double> rv(nn);
      for (int l = 0; l < nlin; ++l)
        for (long k = ptr[l]; k < ptr[l + 1]; ++k) {
          long w = fill[rown[k]]++;
          rc[w] = l; rv[w] = Clin_nzval[k];
        }
      LRN_TRY(ensure(c, c->cr_ptr, (size_t)(nvar + 1) * 8));
      LRN_TRY(ensure(c, c->cr_col, (size_t)nn * 4 + 4));
      LRN_TRY(ensure(c, c->cr_val, (size_t)nn * 8 + 8));
      LRN_TRY(copy_in(c, c->cr_ptr.p, rp.data(), (size_t)(nvar + 1) * 8));
      LRN_TRY(copy_in(c, c->cr_col.p, rc.data(), (size_t)nn * 4));
      LRN_TRY(copy_in(c, c->cr_val.p, rv.data(), (size_t)nn * 8));
    }
  }
  LRN_TRY(alloc_common(c));
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  return LRN_OK;
}

extern "C" int lrn_synthetic_dense_model(lrn_ctx* c, int msz, int nvar, uint64_t seed) {
  if (!c || msz <= 0 || nvar <= 0) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  lrn_free_model(c);
  c->nlmi = 1;
  c->nvar = nvar;
  update_shard_bs(c);
  c->nlin = 0;
  c->pos_space = true;
  c->lmi.resize(1);
  LmiBlock& b = c->lmi[0];
  b.msz = msz;
  b.sigma.resize(nvar);
  std::iota(b.sigma.begin(), b.sigma.end(), 0);
  b.ipos = b.sigma;
  b.nnz.assign(nvar, (long)msz * msz);
  b.qA = b.nd = b.q_wave = b.npos_nz = nvar;
  b.sp_ok = false;
  b.nent = 0;
  std::vector<long> ptr(nvar + 1, 0);
  LRN_TRY(ensure(c, b.ent_ptr, (size_t)(nvar + 1) * 8));
  LRN_TRY(copy_in(c, b.ent_ptr.p, ptr.data(), (size_t)(nvar + 1) * 8));
  LRN_TRY(ensure(c, b.ent_r, 8));
  LRN_TRY(ensure(c, b.ent_c, 8));
  LRN_TRY(ensure(c, b.ent_v, 8));
  LRN_TRY(ensure(c, b.hidx, (size_t)nvar * 4));
  LRN_TRY(copy_in(c, b.hidx.p, b.sigma.data(), (size_t)nvar * 4));
  LRN_TRY(ensure(c, b.sigma_d, (size_t)nvar * 4));
  LRN_TRY(ensure(c, b.ipos_d, (size_t)nvar * 4));
  LRN_TRY(copy_in(c, b.sigma_d.p, b.sigma.data(), (size_t)nvar * 4));
  LRN_TRY(copy_in(c, b.ipos_d.p, b.ipos.data(), (size_t)nvar * 4));
  LRN_TRY(ensure(c, b.Adense, (size_t)nvar * msz * msz * 8));
  const int chunk = 64;
  for (int k0 = 0; k0 < nvar; k0 += chunk) {
    int nk = std::min(chunk, nvar - k0);
    hipLaunchKernelGGL(synth_dense_kernel, dim3(4096), dim3(256), 0, c->stream, b.Adense.as<double>(), msz,
                       k0, nk, seed);
  }
  LRN_TRY(dense_route_setup(c, b, true));     // (R_k + R_k')/2 from one Philox draw per unordered index pair: symmetric by construction
  LRN_TRY(alloc_common(c));
  LRN_HIP(c, hipStreamSynchronize(c->stream));
  return LRN_OK;
}

// ---- builder-defined synthetic problem on top of lrn_synthetic_dense_model
extern "C" int lrn_synthetic_dense_problem(lrn_ctx* c, uint64_t seed, double* b_out, double* y0_out, double* normC) {
  if (!c || c->nlmi != 1 || !b_out || !y0_out) return LRN_ERR_ARG;
  LRN_HIP(c, hipSetDevice(c->device));
  LmiBlock& b = c->lmi[0];
  LRN_TRY(ensure_resident(c, b));
  const int m = b.msz, n = c->nvar;
  const long mm_ = (long)m * m;
  // host-side small random factors (deterministic LCG-free: splitmix64 + Box-Muller)
  auto next = [&seed]() {
    seed += 0x9E3779B97F4A7C15ull;
    uint64_t z = seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  auto unif = [&]() { return ((double)(next() >> 11) + 0.5) / 9007199254740992.0; };
  auto gauss = [&]() { return std::sqrt(-2.0 * std::log(unif())) * std::cos(6.283185307179586 * unif()); };
  const int r = 8;
  std::vector<double> Q((size_t)m * r), y0(n);
  for (auto& v : Q) v = gauss();
  for (auto& v : y0) v = gauss() / std::sqrt((double)n);
  LRN_TRY(copy_in(c, b.t1.p, Q.data(), Q.size() * 8));
  hipLaunchKernelGGL(synth_x0_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.t0.as<double>(), b.t1.as<double>(), m, r);
  // b = AA vec(X0)
  LRN_HIP(c, hipMemsetAsync(c->v1.p, 0, (size_t)n * 8, c->stream));
  LRN_TRY(aa_times(c, b, b.t0.as<double>(), c->v1.as<double>()));
  LRN_TRY(copy_out(c, b_out, c->v1.p, (size_t)n * 8));
  // C = I + mat(AA' y0)
  LRN_TRY(copy_in(c, c->v0.p, y0.data(), (size_t)n * 8));
  LRN_TRY(aat_to_mat(c, b, c->v0.as<double>(), b.t0.as<double>()));
  hipLaunchKernelGGL(eye_add_kernel, dim3(nb(mm_)), dim3(256), 0, c->stream, b.Cd.as<double>(), b.t0.as<double>(), 1.0, m);
  if (normC) {
    LRN_TRY(ensure(c, c->redout, 64 * 8));
    LRN_TRY(dot_dev(c, b.Cd.as<double>(), nullptr, mm_, c->redout.as<double>()));
    double s = 0;
    LRN_TRY(copy_out(c, &s, c->redout.p, 8));
    *normC = std::sqrt(s);
  }
  memcpy(y0_out, y0.data(), (size_t)n * 8);
  return LRN_OK;
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

// A constraint of a factored block is stored (rows of AA) or factored, never both: the first stored position whose factor
// columns carry a non-zero weight, or -1.  w: the weights in H index order (host).
static int stored_and_factored(const lrn_ctx* c, const LmiBlock& b, const double* w) {
  for (int p = 0; p < b.npos_nz; ++p) {
    const long h = c->pos_space ? p : b.sigma[p];
    for (int q = 0; q < b.lr_khat; ++q)
      if (w[h * b.lr_khat + q] != 0.0) return p;
  }
  return -1;
}

// Does a constraint with stored entries have no weighted factor column?  Then the factors do not represent the whole block
// (a materialised block some of whose constraints were given as matrices only): mode 1 assembles it from its entries.
static bool factors_partial(const lrn_ctx* c, const LmiBlock& b, const double* w) {
  for (int p = 0; p < b.npos_nz; ++p) {
    const long h = c->pos_space ? p : b.sigma[p];
    bool any = false;
    for (int q = 0; q < b.lr_khat && !any; ++q) any = w[h * b.lr_khat + q] != 0.0;
    if (!any) return true;
  }
  return false;
}

// the diagonal parts belong to the declaration "factored": they go with it
static void drop_diag(LmiBlock& b) {
  for (DBuf* d : {&b.dg_h, &b.dg_nat, &b.dg_of_pos, &b.dg_a}) release(*d);
  b.dg_n = 0;
}

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
  if ((double)R * m >= 9.0e18 / 8.0 || R > 0x7fffffffL) return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: too many factor columns");
  std::vector<int64_t> cp(m + 1);
  LRN_HIP(c, hipMemcpy(cp.data(), V_colptr, (size_t)(m + 1) * 8, hipMemcpyDefault));
  const long nnz = cp[m] - 1;
  if (cp[0] != 1 || nnz < 0) return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: colptr must start at 1 and not decrease");
  for (int q = 0; q < m; ++q)
    if (cp[q + 1] < cp[q]) return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: colptr decreases at column %d", q);
  if (nnz > 0 && (!V_rowval || !V_nzval)) return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: null factor array");
  std::vector<int64_t> rv(nnz);
  std::vector<double> nz(nnz), w(R), wh(R);
  if (nnz > 0) {
    LRN_HIP(c, hipMemcpy(rv.data(), V_rowval, (size_t)nnz * 8, hipMemcpyDefault));
    LRN_HIP(c, hipMemcpy(nz.data(), V_nzval, (size_t)nnz * 8, hipMemcpyDefault));
  }
  LRN_HIP(c, hipMemcpy(w.data(), d, (size_t)R * 8, hipMemcpyDefault));
  // factor row k * khat + p -> U column hrow(k) * khat + p
  auto hcol = [&](long r) { const long k = r / khat; return (long)(c->pos_space ? b.ipos[k] : (int)k) * khat + r % khat; };
  std::vector<long> ptr(R + 1, 0);
  for (long e = 0; e < nnz; ++e) {
    if (rv[e] < 1 || rv[e] > R) return set_error(c, LRN_ERR_ARG, "lrn_upload_lowrank: rowval %lld out of range", (long long)rv[e]);
    ptr[hcol(rv[e] - 1) + 1]++;
  }
  for (long h = 0; h < R; ++h) ptr[h + 1] += ptr[h];
  std::vector<int> col(nnz);
  std::vector<double> val(nnz);
  std::vector<long> fill(ptr.begin(), ptr.end() - 1);
  for (int q = 0; q < m; ++q)
    for (long e = cp[q] - 1; e < cp[q + 1] - 1; ++e) {
      const long f = fill[hcol(rv[e] - 1)]++;
      col[f] = q;
      val[f] = nz[e];
    }
  for (long r = 0; r < R; ++r) wh[hcol(r)] = w[r];
  LRN_TRY(ensure(c, b.v_ptr, (size_t)(R + 1) * 8));
  LRN_TRY(ensure(c, b.v_col, (size_t)std::max<long>(nnz, 1) * 4));
  LRN_TRY(ensure(c, b.v_val, (size_t)std::max<long>(nnz, 1) * 8));
  LRN_TRY(ensure(c, b.v_w, (size_t)R * 8));
  LRN_TRY(copy_in(c, b.v_ptr.p, ptr.data(), (size_t)(R + 1) * 8));
  if (nnz > 0) {
    LRN_TRY(copy_in(c, b.v_col.p, col.data(), (size_t)nnz * 4));
    LRN_TRY(copy_in(c, b.v_val.p, val.data(), (size_t)nnz * 8));
  }
  LRN_TRY(copy_in(c, b.v_w.p, wh.data(), (size_t)R * 8));
  release(b.Vd);                 // (the dense copy is rebuilt from these factors on first use)
  b.have_Vd = false;
  b.Ys_version = -1;             // (and Y = W Vd of option "fac_op_scaled" with it)
  for (DBuf* rg : {&b.rg_src, &b.rg_wc, &b.rg_gh, &b.rg_hg, &b.rg_tiles, &b.rg_cg, &b.Vc, &b.Yc}) release(*rg);      // (and the rank-class plan, option
  b.rg_ready = false;                                                                      // "lowrank_ragged": rebuilt on first use)
  b.Yc_version = -1;
  b.rg_Rc = ragged_cols(wh.data(), nvar, khat);
  b.lr_khat = khat;
  b.vnnz = nnz;
  b.has_V = true;
  b.v_partial = factors_partial(c, b, wh.data());
  if (b.factored && stored_and_factored(c, b, wh.data()) >= 0) {      // (new factors that overlap the stored rows of a hybrid block)
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
    if (stored_and_factored(c, b, w.data()) >= 0) return has_entries_error(c, b, ilmi);
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
  std::vector<int> dgh(ns), nat(ns), of_pos(nvar, -1);
  for (int s = 0; s < ns; ++s) {
    const int64_t k = rw[s];
    if (k < 0 || k >= nvar) return set_error(c, LRN_ERR_ARG, "lrn_upload_diag: row %lld out of range (0 .. %d)", (long long)k, nvar - 1);
    const int pos = b.ipos[(int)k];
    if (of_pos[pos] >= 0) return set_error(c, LRN_ERR_ARG, "lrn_upload_diag: row %lld is listed twice", (long long)k);
    if (pos < b.npos_nz)
      return set_error(c, LRN_ERR_STATE, "lrn_upload_diag: constraint %lld of block %d is stored (it has entries): its diagonal "
                                         "belongs into the stored matrix", (long long)k, ilmi);
    of_pos[pos] = s;
    nat[s] = (int)k;
    dgh[s] = c->pos_space ? pos : (int)k;
  }
  // staged in buffers of their own and swapped in at the end: an allocation or a copy that fails halfway leaves the parts
  // already uploaded, and their dg_n, as they were
  DBuf th, tn, tp, ta;
  auto stage = [&]() -> int {
    LRN_TRY(ensure(c, th, (size_t)ns * 4));
    LRN_TRY(ensure(c, tn, (size_t)ns * 4));
    LRN_TRY(ensure(c, tp, (size_t)nvar * 4));
    LRN_TRY(ensure(c, ta, (size_t)ns * m * 8));
    LRN_TRY(copy_in(c, th.p, dgh.data(), (size_t)ns * 4));
    LRN_TRY(copy_in(c, tn.p, nat.data(), (size_t)ns * 4));
    LRN_TRY(copy_in(c, tp.p, of_pos.data(), (size_t)nvar * 4));
    LRN_TRY(copy_in(c, ta.p, a, (size_t)ns * m * 8));
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
