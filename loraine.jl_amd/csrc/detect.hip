// Low-rank detection (lrn_lowrank_detect): a batched, rank-revealing factorisation A_k = V_k D_k V_k' of dense symmetric
// constraint matrices by the symmetric Nystrom identity.  For A of rank r < l and a sketch matrix Omega (m x l, l = kmax + 8):
//   Y = A Omega,  C = Omega' Y = U Lambda U'   =>   A = (Y U_r) Lambda_r^-1 (Y U_r)',  V = Y U_r |Lambda_r|^-1/2,  d = sign Lambda_r
// -- no orthonormalisation and no eigenproblem larger than l <= 72.  More than kmax eigenvalues of C above the relative cut:
// the constraint is rejected before any factor is formed.  The residual ||A - V D V'||_F, computed from the factor that goes
// back to the caller, is the arbiter: rank = r only if it is <= tol, -1 otherwise -- a constraint the device is unsure of stays
// a stored matrix, it never becomes a wrong factor.
//
// Five launches per chunk of cnt matrices, every one with a fixed summation order and a single writer per element, so the
// result for a constraint depends on A_k and Omega alone (not on cnt, on its place in the chunk, on its neighbours) and two
// calls give the same bits:
//   detect_sketch_kernel   Y_k = A_k Omega on the FP64 MFMA: workgroup = 64 rows of one matrix, wave = 16 rows x all (padded)
//                          columns, K = m walked in order by that one wave.  The pass that reads all of A (HBM-bound)
//   detect_core_kernel     C_k = Omega' Y_k on and below the diagonal, one workgroup per matrix, rows in order
//   detect_eig_kernel      one workgroup per matrix: the triangle of C mirrored into LDS, cyclic two-sided Jacobi with the round-robin
//                          (tournament) ordering -- l / 2 disjoint rotations per step, l - 1 steps per sweep --, C and U in LDS
//                          for the whole run (2 x 72 x 73 x 8 = 84 096 bytes at l = 72: one workgroup per CU of 160 KiB; 9 600
//                          bytes at l = 24).  A pair is rotated while |c_pq| > 2^-60 ||C||_F and > 2^-53 sqrt|c_pp c_qq|; a sweep
//                          without a rotation ends the run, DET_MAX_SWEEPS at the most.  Then T = U_r |Lambda_r|^-1/2 (l x kmax,
//                          zero padded), the signs, and r or the verdict -1
//   detect_factor_kernel   V_k = Y_k T_k, one thread per row, the columns beyond r written as zeros
//   detect_resid_kernel    ||A_k - V_k D_k V_k'||_F^2 over the 64 x 64 tiles on and below the diagonal: V D V' accumulates in
//                          v_mfma_f64_16x16x4_f64 with K = kmax, is subtracted from the tile of A_k and squared; off-diagonal
//                          tiles count twice.  Sums: 16 terms per lane, the xor butterfly of the wave, the four waves in order
//                          (one partial per tile), then detect_verdict_kernel adds the tiles of a matrix in tile-index order
//                          -- the longest addition chain is 16 + 6 + 4 + ntiles, no atomics
// The routine needs a context and its stream only: it does not touch the uploaded model and may run before lrn_upload_model.
#include "../../include/loraine_hip.h"
#include "ctx.h"

namespace lrn {

static constexpr int DET_MAX_SWEEPS = 30;
static constexpr double DET_ROT_FLOOR = 0x1p-60;
static constexpr double DET_ROT_EPS = 0x1p-53;

// Omega (m x l, column-major) -> OmT[k * LP + n] (row-major, LP = l rounded up to 16, zero columns in the padding)
__global__ __launch_bounds__(256) void detect_omega_kernel(const double* __restrict__ Om, int m, int l, int LP,
                                                           double* __restrict__ OmT) {
  const long n = (long)m * LP;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    const int k = (int)(e / LP), c = (int)(e % LP);
    OmT[e] = c < l ? Om[(long)k + (long)c * m] : 0.0;
  }
}

// Y_k[i + n m] = sum_kk A_k[i + kk m] OmT[kk LP + n]   (grid: x = 64-row strips, y = matrix; NB = LP / 16 accumulators per wave.
// A operand: lane holds A[i0 + (lane & 15)][k + (lane >> 4)], B operand: Omega[k + (lane >> 4)][16 nb + (lane & 15)])
template <int NB>
__global__ __launch_bounds__(256) void detect_sketch_kernel(const double* __restrict__ A, const double* __restrict__ OmT, int m,
                                                            double* __restrict__ Y) {
  constexpr int LP = 16 * NB;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i0 = blockIdx.x * 64 + 16 * w;
  if (i0 >= m) return;
  const double* Ak = A + (long)blockIdx.y * m * m;
  double* Yk = Y + (long)blockIdx.y * m * LP;
  const int ci = lane & 15, kq = lane >> 4;
  const int i = i0 + ci;
  const bool iok = i < m;
  v4f64 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int k0 = 0; k0 < m; k0 += 4) {
    const int kk = k0 + kq;
    const bool kok = kk < m;
    const double a = (iok && kok) ? Ak[(long)i + (long)kk * m] : 0.0;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const double b = kok ? OmT[(long)kk * LP + 16 * nb + ci] : 0.0;
      acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[nb], 0, 0, 0);
    }
  }
  // D: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + kq + 4 * r;
      if (row < m) Yk[(long)row + (long)(16 * nb + ci) * m] = acc[nb][r];
    }
}

// C_k[a + b l] = sum_i Omega[i, a] Y_k[i, b] for a >= b, the rows i in order: C is symmetric, so only the l (l + 1) / 2 entries
// on and below the diagonal are formed (half the work of this step) and detect_eig_kernel mirrors them -- the entries above the
// diagonal of C_k are never written and never read.  One workgroup per matrix; thread t owns the entries t, t + 256, ... of
// the triangle, column after column; 16 rows of Omega and Y staged per step
template <int L, int LP>
__global__ __launch_bounds__(256) void detect_core_kernel(const double* __restrict__ OmT, const double* __restrict__ Y, int m,
                                                          double* __restrict__ Cout) {
  constexpr int NT = L * (L + 1) / 2, NE = (NT + 255) / 256;
  __shared__ double Os[16 * LP];
  __shared__ double Ys[16 * LP];
  const int t = threadIdx.x;
  const double* Yk = Y + (long)blockIdx.x * m * LP;
  double acc[NE];
  int ea[NE], eb[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    int idx = t + 256 * e, b = 0;
    acc[e] = 0.0;
    if (idx >= NT) idx = 0;                       // (an idle slot computes entry (0, 0) and stores nothing)
    while (idx >= L - b) { idx -= L - b; ++b; }
    ea[e] = b + idx;
    eb[e] = b;
  }
  for (int r0 = 0; r0 < m; r0 += 16) {
    __syncthreads();
    for (int e = t; e < 16 * LP; e += 256) {
      const int ri = e % 16, c = e / 16;          // (consecutive threads read consecutive rows of a column of Y)
      const int row = r0 + ri;
      Ys[ri * LP + c] = row < m ? Yk[(long)row + (long)c * m] : 0.0;
      const int ro = e / LP, co = e % LP;
      Os[ro * LP + co] = r0 + ro < m ? OmT[(long)(r0 + ro) * LP + co] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int ri = 0; ri < 16; ++ri)
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[e] = fma(Os[ri * LP + ea[e]], Ys[ri * LP + eb[e]], acc[e]);
  }
  double* Ck = Cout + (long)blockIdx.x * L * L;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    if (t + 256 * e < NT) Ck[ea[e] + eb[e] * L] = acc[e];
  }
}

// pair k (0 .. l / 2 - 1) of step s (0 .. l - 2) of the tournament ordering on l players, l even: player l - 1 stays, the others
// turn -- over a sweep every pair meets once, the pairs of a step are disjoint
__device__ __forceinline__ void rr_pair(int l, int s, int k, int* p, int* q) {
  int a, b;
  if (k == 0) { a = l - 1; b = s; }
  else { a = (s + k) % (l - 1); b = (s - k + (l - 1)) % (l - 1); }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}

// one workgroup per matrix; dynamic LDS: Cs, Us (L x LD, LD = L + 1), then the rotation table
template <int L, int KMAX>
__global__ __launch_bounds__(256) void detect_eig_kernel(const double* __restrict__ Cin, double rank_rtol, double* __restrict__ T,
                                                         double* __restrict__ dout, int* __restrict__ rank,
                                                         int* __restrict__ sweeps_out) {
  constexpr int LD = L + 1, H = L / 2;
  extern __shared__ double det_lds[];
  double* Cs = det_lds;
  double* Us = Cs + L * LD;
  double* rc = Us + L * LD;          // [H] cosines
  double* rs = rc + H;               // [H] sines
  double* rowsum = rs + H;           // [L]
  int* rp = reinterpret_cast<int*>(rowsum + L);   // [H], [H]: the pair; [H]: rotated?; [H]: rotations of the sweep
  int* rq = rp + H;
  int* ron = rq + H;
  int* rcnt = ron + H;
  int* sel = rcnt + H;               // [L] selected eigenvalue indices; sel[L] = r; sel[L + 1] = rotations of the sweep
  const int t = threadIdx.x;
  const long k = blockIdx.x;
  const double* Ck = Cin + k * L * L;
  for (int e = t; e < L * L; e += 256) {
    const int a = e % L, b = e / L;
    Cs[a * LD + b] = a >= b ? Ck[a + b * L] : Ck[b + a * L];      // (the triangle detect_core_kernel formed, mirrored)
    Us[a * LD + b] = a == b ? 1.0 : 0.0;
  }
  __syncthreads();
  if (t < L) {
    double s = 0.0;
    for (int b = 0; b < L; ++b) s = fma(Cs[t * LD + b], Cs[t * LD + b], s);
    rowsum[t] = s;
  }
  __syncthreads();
  double nrm2 = 0.0;
  for (int a = 0; a < L; ++a) nrm2 += rowsum[a];      // (every thread: the same order, the same value)
  const double floor_abs = DET_ROT_FLOOR * sqrt(nrm2);
  int sweeps = 0;
  while (sweeps < DET_MAX_SWEEPS) {
    int nrot = 0;
    for (int s = 0; s < L - 1; ++s) {
      if (t < H) {
        int p, q;
        rr_pair(L, s, t, &p, &q);
        const double x = Cs[p * LD + q], cpp = Cs[p * LD + p], cqq = Cs[q * LD + q];
        const bool on = fabs(x) > floor_abs && fabs(x) > DET_ROT_EPS * sqrt(fabs(cpp) * fabs(cqq));
        double cc = 1.0, ss = 0.0;
        if (on) {
          const double tau = (cqq - cpp) / (2.0 * x);
          const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + hypot(1.0, tau));
          cc = 1.0 / sqrt(1.0 + tt * tt);
          ss = tt * cc;
          ++nrot;
        }
        rp[t] = p; rq[t] = q; ron[t] = on ? 1 : 0; rc[t] = cc; rs[t] = ss;
      }
      __syncthreads();
      // columns: C <- C J, U <- U J
      for (int e = t; e < L * H; e += 256) {
        const int kk = e / L, i = e % L;
        if (!ron[kk]) continue;
        const int p = rp[kk], q = rq[kk];
        const double cc = rc[kk], ss = rs[kk];
        const double a = Cs[i * LD + p], b = Cs[i * LD + q];
        Cs[i * LD + p] = cc * a - ss * b;
        Cs[i * LD + q] = ss * a + cc * b;
        const double ua = Us[i * LD + p], ub = Us[i * LD + q];
        Us[i * LD + p] = cc * ua - ss * ub;
        Us[i * LD + q] = ss * ua + cc * ub;
      }
      __syncthreads();
      // rows: C <- J' C
      for (int e = t; e < L * H; e += 256) {
        const int kk = e / L, j = e % L;
        if (!ron[kk]) continue;
        const int p = rp[kk], q = rq[kk];
        const double cc = rc[kk], ss = rs[kk];
        const double a = Cs[p * LD + j], b = Cs[q * LD + j];
        Cs[p * LD + j] = cc * a - ss * b;
        Cs[q * LD + j] = ss * a + cc * b;
      }
      __syncthreads();
      // the annihilated entries are zero by construction (no pair of the next step reads or writes them before its barrier)
      if (t < H && ron[t]) {
        Cs[rp[t] * LD + rq[t]] = 0.0;
        Cs[rq[t] * LD + rp[t]] = 0.0;
      }
    }
    if (t < H) rcnt[t] = nrot;
    __syncthreads();
    if (t == 0) {
      int tot = 0;
      for (int a = 0; a < H; ++a) tot += rcnt[a];
      sel[L + 1] = tot;
    }
    __syncthreads();
    ++sweeps;
    if (sel[L + 1] == 0) break;
    __syncthreads();
  }
  if (t == 0) {
    double mx = 0.0;
    for (int a = 0; a < L; ++a) mx = fmax(mx, fabs(Cs[a * LD + a]));
    int r = 0;
    for (int a = 0; a < L; ++a)
      if (fabs(Cs[a * LD + a]) > rank_rtol * mx) sel[r++] = a;
    sel[L] = r;
    rank[k] = r <= KMAX ? r : -1;
    sweeps_out[k] = sweeps;
  }
  __syncthreads();
  const int r = sel[L] <= KMAX ? sel[L] : 0;      // rejected: no factor is formed
  double* Tk = T + k * L * KMAX;
  for (int e = t; e < L * KMAX; e += 256) {
    const int a = e % L, j = e / L;
    double v = 0.0;
    if (j < r) {
      const int c = sel[j];
      v = Us[a * LD + c] * (1.0 / sqrt(fabs(Cs[c * LD + c])));
    }
    Tk[e] = v;
  }
  if (t < KMAX) {
    double v = 0.0;
    if (t < r) v = Cs[sel[t] * LD + sel[t]] > 0.0 ? 1.0 : -1.0;
    dout[k * KMAX + t] = v;
  }
}

template <int L>
static size_t detect_eig_lds() {
  return (size_t)(2 * L * (L + 1) + 2 * (L / 2) + L) * 8 + (size_t)(4 * (L / 2) + L + 2) * 4;
}

// V_k[i + j m] = sum_a Y_k[i + a m] T_k[a + j L] for j < rank_k, zero beyond (grid: x = 256-row strips, y = matrix)
template <int L, int LP, int KMAX>
__global__ __launch_bounds__(256) void detect_factor_kernel(const double* __restrict__ Y, const double* __restrict__ T,
                                                            const int* __restrict__ rank, int m, double* __restrict__ V) {
  __shared__ double Ts[L * KMAX];
  const long k = blockIdx.y;
  const int t = threadIdx.x;
  const int r = rank[k] > 0 ? rank[k] : 0;
  for (int e = t; e < L * KMAX; e += 256) Ts[e] = T[k * L * KMAX + e];
  __syncthreads();
  const int i = blockIdx.x * 256 + t;
  if (i >= m) return;
  const double* Yk = Y + k * (long)m * LP;
  double y[L];
#pragma unroll
  for (int a = 0; a < L; ++a) y[a] = Yk[(long)i + (long)a * m];
  double* Vk = V + k * (long)m * KMAX;
  for (int j = 0; j < KMAX; ++j) {
    double s = 0.0;
    if (j < r) {
#pragma unroll
      for (int a = 0; a < L; ++a) s = fma(y[a], Ts[j * L + a], s);
    }
    Vk[(long)i + (long)j * m] = s;
  }
}

// part[k ntile + tile] = sum over the 64 x 64 tile (ti, tj), ti >= tj, of (A_k - V_k D_k V_k')^2, twice for ti > tj.
// Wave w owns the 32 x 32 block (w >> 1, w & 1) as 2 x 2 accumulators with the j side as the A operand and the i side as the
// B operand: D[row = j][col = i], so the 16 lanes of a row group read 16 consecutive rows i of one column j of A_k
template <int KMAX>
__global__ __launch_bounds__(256) void detect_resid_kernel(const double* __restrict__ A, const double* __restrict__ V,
                                                           const double* __restrict__ d, int m, int ntile,
                                                           double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long k = blockIdx.y;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
  const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
  const int ci = lane & 15, kq = lane >> 4;
  const int ib0 = 64 * ti + 32 * (w >> 1), jb0 = 64 * tj + 32 * (w & 1);
  const double* Ak = A + k * (long)m * m;
  const double* Vk = V + k * (long)m * KMAX;
  const double* dk = d + k * KMAX;
  v4f64 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int p0 = 0; p0 < KMAX; p0 += 4) {
    const int p = p0 + kq;
    const double dp = dk[p];
    double aj[2], bi[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int jj = jb0 + 16 * h + ci, ii = ib0 + 16 * h + ci;
      aj[h] = jj < m ? Vk[(long)jj + (long)p * m] * dp : 0.0;
      bi[h] = ii < m ? Vk[(long)ii + (long)p * m] : 0.0;
    }
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) acc[jb][ib] = __builtin_amdgcn_mfma_f64_16x16x4f64(aj[jb], bi[ib], acc[jb][ib], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int jb = 0; jb < 2; ++jb)
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ib0 + 16 * ib + ci, j = jb0 + 16 * jb + kq + 4 * r;
        const double e = (i < m && j < m) ? Ak[(long)i + (long)j * m] - acc[jb][ib][r] : 0.0;
        s = fma(e, e, s);
      }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) red[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = ((red[0] + red[1]) + red[2]) + red[3];
    part[k * ntile + blockIdx.x] = ti == tj ? tot : 2.0 * tot;
  }
}

// resid_k = sqrt(sum of the tiles in index order); the residual is the arbiter: a factor that misses tol is no factor
__global__ __launch_bounds__(256) void detect_verdict_kernel(const double* __restrict__ part, int ntile, int cnt, double tol,
                                                             double* __restrict__ resid, int* __restrict__ rank) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= cnt) return;
  double s = 0.0;
  for (int tl = 0; tl < ntile; ++tl) s += part[(long)k * ntile + tl];
  const double r = sqrt(s);
  resid[k] = r;
  if (rank[k] >= 0 && !(r <= tol)) rank[k] = -1;
}

template <int KMAX>
static int detect_run(lrn_ctx* c, int m, int cnt, const double* A_dev, const double* Om_dev, double tol, double rank_rtol) {
  constexpr int L = KMAX + 8, NB = (L + 15) / 16, LP = 16 * NB;
  hipStream_t st = c->stream;
  const int nt1 = (m + 63) / 64, ntile = nt1 * (nt1 + 1) / 2;
  // small buffers in one allocation: OmT | C | T | d | resid | part | rank | sweeps
  const size_t nOm = (size_t)m * LP, nC = (size_t)cnt * L * L, nT = (size_t)cnt * L * KMAX, nd = (size_t)cnt * KMAX,
               nr = (size_t)cnt, np = (size_t)cnt * ntile;
  LRN_TRY(ensure(c, c->det_small, (nOm + nC + nT + nd + nr + np) * 8 + (size_t)cnt * 8));
  LRN_TRY(ensure(c, c->det_Y, (size_t)cnt * m * LP * 8));
  LRN_TRY(ensure(c, c->det_V, (size_t)cnt * m * KMAX * 8));
  double* OmT = c->det_small.as<double>();
  double* Cc = OmT + nOm;
  double* T = Cc + nC;
  double* dd = T + nT;
  double* resid = dd + nd;
  double* part = resid + nr;
  int* rank = reinterpret_cast<int*>(part + np);
  int* sweeps = rank + cnt;
  double* Y = c->det_Y.as<double>();
  double* V = c->det_V.as<double>();
  // dynamic LDS above the 64 KiB default (l = 72) has to be asked for; on every call -- it is cheap, applies to the current
  // device, and keeps no state that two host threads or a device index beyond some table could get wrong
  const size_t sh = detect_eig_lds<L>();
  LRN_HIP(c, hipFuncSetAttribute((const void*)detect_eig_kernel<L, KMAX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
  {
    PhaseTimer pt(c, c->profile);
    hipLaunchKernelGGL(detect_omega_kernel, dim3(nb((long)m * LP)), dim3(256), 0, st, Om_dev, m, L, LP, OmT);
    hipLaunchKernelGGL(detect_sketch_kernel<NB>, dim3(nt1, cnt), dim3(256), 0, st, A_dev, OmT, m, Y);
    pt.stop("detect_sketch");
  }
  {
    PhaseTimer pt(c, c->profile);
    hipLaunchKernelGGL((detect_core_kernel<L, LP>), dim3(cnt), dim3(256), 0, st, OmT, Y, m, Cc);
    pt.stop("detect_core");
  }
  {
    PhaseTimer pt(c, c->profile);
    hipLaunchKernelGGL((detect_eig_kernel<L, KMAX>), dim3(cnt), dim3(256), sh, st, Cc, rank_rtol, T, dd, rank, sweeps);
    pt.stop("detect_eig");
  }
  {
    PhaseTimer pt(c, c->profile);
    hipLaunchKernelGGL((detect_factor_kernel<L, LP, KMAX>), dim3((m + 255) / 256, cnt), dim3(256), 0, st, Y, T, rank, m, V);
    pt.stop("detect_factor");
  }
  {
    PhaseTimer pt(c, c->profile);
    hipLaunchKernelGGL(detect_resid_kernel<KMAX>, dim3(ntile, cnt), dim3(256), 0, st, A_dev, V, dd, m, ntile, part);
    hipLaunchKernelGGL(detect_verdict_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, part, ntile, cnt, tol, resid, rank);
    pt.stop("detect_resid");
  }
  LRN_HIP(c, hipGetLastError());
  return LRN_OK;
}

}  // namespace lrn

using namespace lrn;

extern "C" int lrn_lowrank_detect(lrn_ctx* c, int m, int cnt, const double* A, int kmax, double tol, double rank_rtol,
                                  const double* omega, int32_t* rank_out, double* resid_out, double* V_out, double* d_out) {
  if (!c) return LRN_ERR_ARG;
  if (m < 1 || cnt < 1 || cnt > 65535) return set_error(c, LRN_ERR_ARG, "lrn_lowrank_detect: m = %d, cnt = %d (m >= 1, 1 <= cnt <= 65535)", m, cnt);
  if (kmax != 16 && kmax != 64) return set_error(c, LRN_ERR_ARG, "lrn_lowrank_detect: kmax = %d (16 or 64)", kmax);
  if (!(tol >= 0.0) || !(rank_rtol >= 0.0)) return set_error(c, LRN_ERR_ARG, "lrn_lowrank_detect: tol = %g, rank_rtol = %g", tol, rank_rtol);
  if (!A || !omega || !rank_out || !resid_out || !V_out || !d_out) return set_error(c, LRN_ERR_ARG, "lrn_lowrank_detect: null array");
  LRN_HIP(c, hipSetDevice(c->device));
  PhaseTimer all(c, c->profile);
  const int l = kmax + 8;
  const size_t abytes = (size_t)cnt * m * m * 8;
  const double* A_dev = A;
  if (!is_device_ptr(A)) {
    LRN_TRY(ensure(c, c->det_A, abytes));
    PhaseTimer pt(c, c->profile);
    LRN_TRY(copy_in(c, c->det_A.p, A, abytes));
    pt.stop("detect_upload");
    A_dev = c->det_A.as<double>();
  }
  LRN_TRY(ensure(c, c->det_Om, (size_t)m * l * 8));
  LRN_TRY(copy_in(c, c->det_Om.p, omega, (size_t)m * l * 8));
  LRN_TRY(kmax == 16 ? detect_run<16>(c, m, cnt, A_dev, c->det_Om.as<double>(), tol, rank_rtol)
                     : detect_run<64>(c, m, cnt, A_dev, c->det_Om.as<double>(), tol, rank_rtol));
  // the layout of det_small, as detect_run laid it out
  const int LP = (l + 15) / 16 * 16, nt1 = (m + 63) / 64, ntile = nt1 * (nt1 + 1) / 2;
  const double* dd = c->det_small.as<double>() + (size_t)m * LP + (size_t)cnt * l * l + (size_t)cnt * l * kmax;
  const double* resid = dd + (size_t)cnt * kmax;
  const int* rank = reinterpret_cast<const int*>(resid + cnt + (size_t)cnt * ntile);
  std::vector<int> hr(2 * (size_t)cnt);
  LRN_HIP(c, hipMemcpyAsync(hr.data(), rank, (size_t)cnt * 8, hipMemcpyDeviceToHost, c->stream));
  LRN_TRY(copy_out(c, resid_out, resid, (size_t)cnt * 8));
  LRN_TRY(copy_out(c, d_out, dd, (size_t)cnt * kmax * 8));
  LRN_TRY(copy_out(c, V_out, c->det_V.p, (size_t)cnt * m * kmax * 8));
  long acc = 0, smax = c->counts["detect_sweeps_max"];
  for (int k = 0; k < cnt; ++k) {
    if (hr[k] >= 0) ++acc;
    smax = std::max(smax, (long)hr[cnt + k]);
  }
  if (is_device_ptr(rank_out)) LRN_TRY(copy_in(c, rank_out, hr.data(), (size_t)cnt * 4));
  else memcpy(rank_out, hr.data(), (size_t)cnt * 4);
  c->counts["detect_calls"] += 1;
  c->counts["detect_accepted"] += acc;
  c->counts["detect_rejected"] += cnt - acc;
  c->counts["detect_sweeps_max"] = smax;
  all.stop("detect");
  return LRN_OK;
}

// the workspace of lrn_lowrank_detect goes with the context (lrn_destroy) or on request (lrn_set_option "detect_release")
void lrn_detect_free(lrn_ctx* c) {
  release(c->det_A);
  release(c->det_Om);
  release(c->det_Y);
  release(c->det_V);
  release(c->det_small);
}
