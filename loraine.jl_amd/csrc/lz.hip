// The plain Lanczos recurrence on the device (no re-orthogonalisation): y = M q on all CUs, alpha, the three-term update
// and beta without a host synchronisation inside a batch of steps; the host only bisects the tiny tridiagonal matrix
// (tridiag.h).  It drives every eigmin of the step-length rule (predictor_corrector.jl:272,285; Solvers.jl:503,505), the
// scale of the Newton-Schulz iteration (lanczos_ends) and the k <= 1 H_alpha setup (lanczos.hip).
//
// A step exists in three forms (LzForm, lz.h) that compute the same coefficients; lz_queue_steps is the one place that
// launches them, lz_fetch / lz_record_give_up the one place where a resident launch that gave up is noticed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lz.h"
#include "ops.h"
#include "reduce.h"
#include "tridiag.h"

namespace lrn {

__global__ void lz_init_kernel(double* __restrict__ q, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned h = (unsigned)i * 2654435761u + 12345u;     // fixed pseudo-random start vector
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  q[i] = ((double)h / 4294967296.0) - 0.5;
}

// ypart[chunk][i] = sum_{j in chunk} M[i + j*n] q[j]
__global__ __launch_bounds__(256) void symv_part_kernel(const double* __restrict__ M, int n, int cper,
                                                        const double* __restrict__ q, double* __restrict__ ypart) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int c0 = blockIdx.y * cper, c1 = min(n, c0 + cper);
  double s = 0.0;
  for (int j = c0; j < c1; ++j) s += M[(long)i + (long)j * n] * q[j];
  ypart[(long)blockIdx.y * n + i] = s;
}

// one Lanczos step (no re-orthogonalisation): w = sum ypart; a = q.w; w -= a q + b_prev q_prev;
// b = ||w||; q_next = w / b.   j == -1: just normalise q in place (start vector).
__global__ __launch_bounds__(1024) void lz_step_kernel(const double* __restrict__ ypart, int nchunk, int n, int j,
                                                       double* __restrict__ q, double* __restrict__ qprev,
                                                       double* __restrict__ w, double* __restrict__ ab) {
  __shared__ double sh[16];
  const int t = threadIdx.x;
  if (j < 0) {
    double s = 0.0;
    for (int i = t; i < n; i += 1024) s += q[i] * q[i];
    s = wg_sum<16>(s, sh);
    double r = 1.0 / sqrt(s);
    for (int i = t; i < n; i += 1024) { q[i] *= r; qprev[i] = 0.0; }
    return;
  }
  const double bprev = j > 0 ? ab[2 * (j - 1) + 1] : 0.0;
  double a = 0.0;
  for (int i = t; i < n; i += 1024) {
    double s = 0.0;
    for (int k = 0; k < nchunk; ++k) s += ypart[(long)k * n + i];
    w[i] = s;
    a += q[i] * s;
  }
  a = wg_sum<16>(a, sh);
  double b2 = 0.0;
  for (int i = t; i < n; i += 1024) {
    double v = w[i] - a * q[i] - bprev * qprev[i];
    w[i] = v;
    b2 += v * v;
  }
  b2 = wg_sum<16>(b2, sh);
  double b = sqrt(b2);
  double r = b > 0.0 ? 1.0 / b : 0.0;
  for (int i = t; i < n; i += 1024) {
    double qi = q[i];
    qprev[i] = qi;
    q[i] = w[i] * r;
  }
  if (t == 0) { ab[2 * j] = a; ab[2 * j + 1] = b; }
}

// One Lanczos step in ONE launch (n <= LZ_FUSED_MAX; round 3).  The two-kernel step above costs two dependent launches
// (10 + 7 us at msz 800, rocprofv3) for a few microseconds of work.  Here every workgroup first finishes step j-1 by
// itself -- alpha_{j-1} from the partial dots of the previous launch, w = y_{j-1} - alpha q_{j-1} - beta_{j-2} q_{j-2},
// beta_{j-1} = ||w|| and q_j = w / beta_{j-1} for ALL n entries, redundantly (n <= 4096 flops per thread block, in LDS) --
// and then computes its 16 rows of y_j = M q_j and their share of q_j . y_j.  Vectors rotate through three (q) and two (y)
// buffers so that nothing a workgroup still reads is overwritten inside a launch.  `do_symv` = 0: only finish step j-1
// (last launch of a batch: the host needs alpha, beta of every step it reads).
static constexpr int LZ_FUSED_MAX = 16384;      // (round 4: 4096 -> 16384, q_j in up to 128 KB of LDS: at msz 10^4 the two-kernel
                                                // step costs 0.21 + 0.24 ms -- its single-workgroup half sums 64 partial vectors)
__device__ __forceinline__ void lz_fused_body(const double* __restrict__ M, int n, int nwg, int j, int do_symv, int qmod,
                                              double* Q3, double* Y2, double* PA2, double* ab, double* qs, double* sh) {
  const int t = threadIdx.x;
  double* qj = Q3 + (size_t)(j % qmod) * n;       // qmod = 3: rotating buffers; > number of steps: every q_j is kept
  if (j == 0) {
    for (int i = t; i < n; i += 256) qs[i] = qj[i];
  } else {
    const double* qm1 = Q3 + (size_t)((j - 1) % qmod) * n;  // q_{j-1}
    const double* qm2 = Q3 + (size_t)((j > 1 ? j - 2 : 0) % qmod) * n;   // q_{j-2}
    const double* ym1 = Y2 + (size_t)((j + 1) & 1) * n;     // y_{j-1}
    const double* pa = PA2 + (size_t)((j + 1) & 1) * nwg;
    double a = 0.0;
    for (int e = t; e < nwg; e += 256) a += pa[e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if ((t & 63) == 0) sh[t >> 6] = a;
    __syncthreads();
    const double alpha = sh[0] + sh[1] + sh[2] + sh[3];
    const double bprev = j > 1 ? ab[2 * (j - 2) + 1] : 0.0;
    __syncthreads();
    double b2 = 0.0;
    for (int i = t; i < n; i += 256) {
      const double v = ym1[i] - alpha * qm1[i] - (j > 1 ? bprev * qm2[i] : 0.0);
      qs[i] = v;
      b2 += v * v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) b2 += __shfl_down(b2, off, 64);
    if ((t & 63) == 0) sh[t >> 6] = b2;
    __syncthreads();
    const double beta = sqrt(sh[0] + sh[1] + sh[2] + sh[3]);
    const double r = beta > 0.0 ? 1.0 / beta : 0.0;
    for (int i = t; i < n; i += 256) {
      const double v = qs[i] * r;
      qs[i] = v;
      if (blockIdx.x == 0) qj[i] = v;
    }
    if (blockIdx.x == 0 && t == 0) { ab[2 * (j - 1)] = alpha; ab[2 * (j - 1) + 1] = beta; }
  }
  __syncthreads();
  if (!do_symv) return;
  // rows [16 blockIdx.x, +16) of M q = the same COLUMNS of the symmetric M (contiguous): wave w takes four of them, its
  // lanes run down the columns with the four loads of a step in flight together (round 4; round 3 walked the rows with a
  // stride of n and four loads in flight per thread: 50 dependent rounds of L2 latency at msz 800)
  {
    const int lane = t & 63, w = t >> 6;
    const int c0 = blockIdx.x * 16 + 4 * w;
    const double* m0 = M + (size_t)min(c0 + 0, n - 1) * n;
    const double* m1 = M + (size_t)min(c0 + 1, n - 1) * n;
    const double* m2 = M + (size_t)min(c0 + 2, n - 1) * n;
    const double* m3 = M + (size_t)min(c0 + 3, n - 1) * n;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
    for (int k = lane; k < n; k += 64) {
      const double q = qs[k];
      a0 += m0[k] * q; a1 += m1[k] * q; a2 += m2[k] * q; a3 += m3[k] * q;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      a0 += __shfl_down(a0, off, 64); a1 += __shfl_down(a1, off, 64);
      a2 += __shfl_down(a2, off, 64); a3 += __shfl_down(a3, off, 64);
    }
    if (lane == 0) { sh[4 * w + 0] = a0; sh[4 * w + 1] = a1; sh[4 * w + 2] = a2; sh[4 * w + 3] = a3; }
  }
  __syncthreads();
  if (t < 16) {
    const double y = sh[t];
    const int ii = blockIdx.x * 16 + t;
    double d = 0.0;
    if (ii < n) {
      Y2[(size_t)(j & 1) * n + ii] = y;
      d = qs[ii] * y;
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) d += __shfl_down(d, off, 16);
    if (t == 0) PA2[(size_t)(j & 1) * nwg + blockIdx.x] = d;
  }
}

__global__ __launch_bounds__(256) void lz_fused_kernel(const double* __restrict__ M, int n, int nwg, int j, int do_symv, int qmod,
                                                       double* Q3, double* Y2, double* PA2, double* ab) {
  extern __shared__ double qs[];            // q_j (n doubles)
  __shared__ double sh[16 * 16 + 8];
  lz_fused_body(M, n, nwg, j, do_symv, qmod, Q3, Y2, PA2, ab, qs, sh);
}

// The same step of TWO independent runs on matrices of one size in one launch: blockIdx.y picks the run (round 4, second
// session).  The two eigmin searches of a step-length computation used to live on two streams so that their launch chains
// overlap.  Under rocprofv3's kernel trace they do not (tools/lz_overlap.py on a maxG11 solve: 4 % of the kernel time of the
// two queues overlaps); without the profiler both forms take the same time (same box, profiles/r04_lanczos_pair_ab.txt:
// find_step 4.99 vs 4.96 ms at 480 steps, 0.84 vs 0.90 at 64) -- the chains did overlap, and what a step-length search costs
// is its LONGER chain at 8-10 us per step.  The paired form is the default all the same: half the launches for the host to
// issue, one stream, no events between streams.
struct LzPair {
  const double* M[2];
  double* Q3[2];
  double* Y2[2];
  double* PA2[2];
  double* ab[2];
};
__global__ __launch_bounds__(256) void lz_fused_pair_kernel(LzPair a, int n, int nwg, int j, int do_symv, int qmod) {
  extern __shared__ double qs[];            // q_j (n doubles)
  __shared__ double sh[16 * 16 + 8];
  const int r = blockIdx.y;                 // (uniform: the arrays of the argument block are read with scalar loads)
  lz_fused_body(a.M[r], n, nwg, j, do_symv, qmod, a.Q3[r], a.Y2[r], a.PA2[r], a.ab[r], qs, sh);
}

// more than 64 KB of dynamic LDS need the attribute (once per device); false: the two-kernel step is taken
static bool lz_big_lds_ok() {
  static bool done[64] = {}, ok[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  if (!done[dev]) {
    ok[dev] = hipFuncSetAttribute(reinterpret_cast<const void*>(lz_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  LZ_FUSED_MAX * 8) == hipSuccess &&
              hipFuncSetAttribute(reinterpret_cast<const void*>(lz_fused_pair_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  LZ_FUSED_MAX * 8) == hipSuccess;
    if (!ok[dev]) (void)hipGetLastError();
    done[dev] = true;
  }
  return ok[dev];
}

// ---- RESIDENT steps (option lz_resident): the steps [j0, j1) in ONE launch.  A batch of launched steps is a chain of
// launches of 7-8 us each for 2-3 us of work.  A first resident kernel -- lz_fused_body in a loop, the workgroups meeting at
// a counter barrier with a device-scope fence on either side -- was slower than one launch per step and has been removed
// (DESIGN.md section 8).  Its cost was not the barrier but the two fences (tools/lab/xcd_barrier.hip,
// profiles/r04_xcd_barrier.txt: a barrier of 51 workgroups with an 801-vector exchanged costs 4.7 us per step with
// __threadfence() on both sides and 2.3 us when counter AND payload travel as relaxed agent-scope atomics -- they bypass the
// L1s and meet at the coherent level, nothing has to be written back or invalidated), and that every step still re-read its
// 16 columns of M and three vectors from L2.  Here, for n <= 1024:
//  * a workgroup keeps its 16 columns of M in REGISTERS for the whole launch (wave w: columns 4 w .. 4 w + 3, lane l: rows
//    l, l + 64, ...: the order in which lz_fused_body sums them) and q_j, q_{j-1}, q_{j-2} in LDS;
//  * the only data other workgroups produce -- the 16 entries of y_j and the partial sum of q_j . y_j per workgroup -- are
//    written and read with relaxed agent-scope atomic stores / loads; beta_{j-1} stays in a register;
//  * there is no barrier at all: a word that has not been written yet holds a mark, and a reader polls the 17 words of every
//    workgroup until no mark is left (LZ_MARK_BITS below).
// The kernel can NOT hang: every poll loop is bounded.  A workgroup that waits longer than `limit` ticks of the 100 MHz wall
// clock (its peers were not scheduled -- a GPU shared with another process, an over-subscribed chip) raises the abort word
// flag[1], every workgroup leaves at its next poll, and the host redoes the run with launched steps (lz_fetch).
// The arithmetic, operation by operation, is lz_fused_body's: same coefficients bit for bit
// (test_resident_lanczos_steps_are_the_launched_ones).  blockIdx.y: the run (two runs of a step-length search in lock-step).
struct LzRes {
  const double* M;
  double* Q3;
  double* Y3;            // three n-vectors: y_j in buffer j % 3
  double* PA3;           // three nwg-vectors: the workgroups' shares of q_j . y_j
  double* ab;
  unsigned* flag;        // flag[1]: abort word
};
struct LzResPair { LzRes r[2]; };

__device__ __forceinline__ double lz_ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lz_st(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// "Not written yet": a quiet NaN with a payload no computation produces.  The exchange needs NO counter: a workgroup's
// 17 words of step j go to buffer j % 3, which it has filled with this value at step j - 1 -- at a time when every
// workgroup was done reading the buffer's previous content (that of step j - 3: read in the first phase of step j - 2, and a
// workgroup publishes its words of step j - 2 only after that phase; seeing all of those is what lets step j - 1 begin) --
// and whose reset it has seen acknowledged before it published step j - 1 (s_waitcnt vmcnt(0) between the two).  A reader
// therefore finds either the mark or the word of step j, never an older word, and polls until no mark is left.
static constexpr unsigned long long LZ_MARK_BITS = 0x7ff8a5a5deadbeefULL;
__device__ __forceinline__ bool lz_is_mark(double v) { return (unsigned long long)__double_as_longlong(v) == LZ_MARK_BITS; }

__global__ void lz_mark_kernel(double* __restrict__ p, int cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cnt) p[i] = __longlong_as_double((long long)LZ_MARK_BITS);
}

static constexpr int LZ_RES_MAX = 1024;       // 16 rows per lane and column
// limit: ticks a resident workgroup waits for its peers (option lz_res_limit; 20 ms at 100 MHz by default).  wh_step, wh_wg:
// test hook lz_test_withhold -- workgroup wh_wg (64 blockIdx.y + blockIdx.x) keeps its words of step wh_step to itself, so
// that its peers' wait expires (-1: none)
__global__ __launch_bounds__(256) void lz_resident_kernel(LzResPair args, int n, int nwg, int j0, int j1, int qmod, long long limit,
                                                          int wh_step, int wh_wg) {
  extern __shared__ double ql[];            // three n-vectors: q_j, q_{j-1}, q_{j-2} rotate through them
  __shared__ double sh[16 * 16 + 8];
  __shared__ int ok_s;
  const LzRes& R = args.r[blockIdx.y];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int c0 = blockIdx.x * 16 + 4 * w;
  const double mark = __longlong_as_double((long long)LZ_MARK_BITS);
  const int silent_step = (int)(blockIdx.y * 64 + blockIdx.x) == wh_wg ? wh_step : -1;      // (uniform)
  constexpr int U = LZ_RES_MAX / 64;
  double mreg[4][U];
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) {
    const double* col = R.M + (size_t)min(c0 + cc, n - 1) * n;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = lane + 64 * u;
      mreg[cc][u] = k < n ? col[k] : 0.0;
    }
  }
  // state of the recurrence at entry: q_{j0-1}, q_{j0-2} (the ring of the previous launches), beta_{j0-2}
  double bprev = 0.0;
  if (j0 > 0) {
    const double* g1 = R.Q3 + (size_t)((j0 - 1) % qmod) * n;
    double* l1 = ql + (size_t)((j0 - 1) % 3) * n;
    for (int i = t; i < n; i += 256) l1[i] = g1[i];
    if (j0 > 1) {
      const double* g2 = R.Q3 + (size_t)((j0 - 2) % qmod) * n;
      double* l2 = ql + (size_t)((j0 - 2) % 3) * n;
      for (int i = t; i < n; i += 256) l2[i] = g2[i];
      bprev = R.ab[2 * (j0 - 2) + 1];
    }
  }
  if (t == 0) ok_s = 1;
  __syncthreads();
  double alpha_out = 0.0;
  for (int j = j0; j <= j1; ++j) {
    const bool finish = j == j1;            // (workgroup 0 only: alpha, beta of step j1 - 1 and q_{j1} for the host and the next launch)
    if (finish && blockIdx.x != 0) break;
    double* qs = ql + (size_t)(j % 3) * n;
    double* qj = R.Q3 + (size_t)(j % qmod) * n;
    bool polled = true;
    if (j == 0) {
      for (int i = t; i < n; i += 256) qs[i] = qj[i];
    } else {
      const double* qm1 = ql + (size_t)((j - 1) % 3) * n;
      const double* qm2 = ql + (size_t)((j > 1 ? j - 2 : 0) % 3) * n;
      const double* ym1 = R.Y3 + (size_t)((j - 1) % 3) * n;
      const double* pa = R.PA3 + (size_t)((j - 1) % 3) * nwg;
      // the words of step j - 1 of every workgroup: polled until none is the mark (all requests of a poll in flight together)
      double yv[LZ_RES_MAX / 256];
      double a = 0.0;
      long long t0 = 0;
      for (int tries = 0;; ++tries) {
        int bad = 0;
#pragma unroll
        for (int u = 0; u < LZ_RES_MAX / 256; ++u) {
          const int i = t + 256 * u;
          yv[u] = i < n ? lz_ld(ym1 + i) : 0.0;
        }
        a = t < nwg ? lz_ld(pa + t) : 0.0;            // (nwg <= 64)
#pragma unroll
        for (int u = 0; u < LZ_RES_MAX / 256; ++u) bad |= lz_is_mark(yv[u]) ? 1 : 0;
        bad |= lz_is_mark(a) ? 1 : 0;
        if (tries > 0 && t == 0) {                    // bounded: the wall clock, and the other workgroups' verdict
          if (tries == 1) t0 = wall_clock64();
          if (__hip_atomic_load(R.flag + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) ok_s = 0;
          else if (wall_clock64() - t0 > limit) {
            __hip_atomic_store(R.flag + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok_s = 0;
          }
        }
        if (!__syncthreads_or(bad)) break;
        if (!ok_s) { polled = false; break; }
      }
      if (!polled) return;
      // this workgroup's words of buffer (j + 1) % 3 back to the mark (see LZ_MARK_BITS): issued first thing -- everybody has
      // published step j - 1, so nobody reads that buffer's old content any more --, acknowledged by the time step j is published
      if (!finish && t < 16) {
        const int ii = blockIdx.x * 16 + t;
        if (ii < n) lz_st(R.Y3 + (size_t)((j + 1) % 3) * n + ii, mark);
        if (t == 0) lz_st(R.PA3 + (size_t)((j + 1) % 3) * nwg + blockIdx.x, mark);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
      if ((t & 63) == 0) sh[t >> 6] = a;
      __syncthreads();
      const double alpha = sh[0] + sh[1] + sh[2] + sh[3];
      __syncthreads();
      double b2 = 0.0;
#pragma unroll
      for (int u = 0; u < LZ_RES_MAX / 256; ++u) {
        const int i = t + 256 * u;
        if (i < n) {
          const double v = yv[u] - alpha * qm1[i] - (j > 1 ? bprev * qm2[i] : 0.0);
          qs[i] = v;
          b2 += v * v;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) b2 += __shfl_down(b2, off, 64);
      if ((t & 63) == 0) sh[t >> 6] = b2;
      __syncthreads();
      const double beta = sqrt(sh[0] + sh[1] + sh[2] + sh[3]);
      const double r = beta > 0.0 ? 1.0 / beta : 0.0;
      for (int i = t; i < n; i += 256) qs[i] *= r;
      alpha_out = alpha;
      bprev = beta;
    }
    if (j == 0 && !finish && t < 16) {      // (step 0: the marks of buffer 1; lz_prepare has set them already, kept for symmetry)
      const int ii = blockIdx.x * 16 + t;
      if (ii < n) lz_st(R.Y3 + (size_t)n + ii, mark);
      if (t == 0) lz_st(R.PA3 + (size_t)nwg + blockIdx.x, mark);
    }
    __syncthreads();
    if (finish) {      // (workgroup 0)
      if (j > 0) {
        for (int i = t; i < n; i += 256) qj[i] = qs[i];
        if (t == 0) { R.ab[2 * (j - 1)] = alpha_out; R.ab[2 * (j - 1) + 1] = bprev; }
      }
      break;
    }
    {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = lane + 64 * u;
        if (k < n) {
          const double q = qs[k];
          a0 += mreg[0][u] * q; a1 += mreg[1][u] * q; a2 += mreg[2][u] * q; a3 += mreg[3][u] * q;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        a0 += __shfl_down(a0, off, 64); a1 += __shfl_down(a1, off, 64);
        a2 += __shfl_down(a2, off, 64); a3 += __shfl_down(a3, off, 64);
      }
      if (lane == 0) { sh[4 * w + 0] = a0; sh[4 * w + 1] = a1; sh[4 * w + 2] = a2; sh[4 * w + 3] = a3; }
    }
    __syncthreads();
    if (t < 16 && j != silent_step) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the marks above have been acknowledged
      const double y = sh[t];
      const int ii = blockIdx.x * 16 + t;
      double d = 0.0;
      if (ii < n) {
        lz_st(R.Y3 + (size_t)(j % 3) * n + ii, y);
        d = qs[ii] * y;
      }
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) d += __shfl_down(d, off, 16);
      if (t == 0) lz_st(R.PA3 + (size_t)(j % 3) * nwg + blockIdx.x, d);
    }
    // q_j, alpha_{j-1}, beta_{j-1} for the host and the next launch: plain stores of workgroup 0, BEHIND the publication
    // (the wait for the marks' acknowledgement would otherwise wait for them as well, every step, with everybody waiting)
    if (blockIdx.x == 0 && j > 0) {
      for (int i = t; i < n; i += 256) qj[i] = qs[i];
      if (t == 0) { R.ab[2 * (j - 1)] = alpha_out; R.ab[2 * (j - 1) + 1] = bprev; }
    }
    __syncthreads();      // (sh and the q ring are rewritten by the next step)
  }
}

// ---- the one place that launches steps
// column chunks of the two-kernel mat-vec: ~64 columns per thread keeps the step kernel's reduction short
static void lz_chunks(int n, int* nchunk, int* cper) {
  *nchunk = std::max(1, std::min(64, n / 64));
  *cper = (n + *nchunk - 1) / *nchunk;
  *nchunk = (n + *cper - 1) / *cper;
}

// second half of the two-kernel step j (q_{j-1} in Q + n, w in Y); j = -1: normalise the start vector in Q
static void lz_step(const LzWork& w, int j) {
  int nchunk, cper;
  lz_chunks(w.n, &nchunk, &cper);
  hipLaunchKernelGGL(lz_step_kernel, dim3(1), dim3(1024), 0, w.st, w.PA, nchunk, w.n, j, w.Q, w.Q + w.n, w.Y, w.ab);
}

bool lz_resident_ok(const lrn_ctx* c, int n) {
  return c->opt.lz_resident != 0 && !c->lz_no_persist && n <= LZ_RES_MAX && n >= 32;
}

void lz_prepare(const LzWork& w) {
  if (w.form != LZ_RESIDENT) return;
  hipLaunchKernelGGL(lz_mark_kernel, dim3((3 * w.n + 255) / 256), dim3(256), 0, w.st, w.Y, 3 * w.n);
  hipLaunchKernelGGL(lz_mark_kernel, dim3((3 * w.nwg + 255) / 256), dim3(256), 0, w.st, w.PA, 3 * w.nwg);
  (void)hipMemsetAsync(w.flag, 0, 16, w.st);
}

int lz_queue_steps(const LzWork* const w[], int nruns, int j0, int j1) {
  if (nruns < 1 || nruns > 2) return LRN_ERR_ARG;
  const LzWork &a = *w[0], &b = *w[nruns - 1];
  const int n = a.n, nwg = a.nwg, qmod = a.qmod;
  if (b.n != n || b.qmod != qmod || b.form != a.form || qmod < 3 || (qmod > 3 && j1 + 1 > qmod)) return LRN_ERR_ARG;
  switch (a.form) {
    case LZ_RESIDENT: {
      if (n > LZ_RES_MAX || !a.c) return LRN_ERR_ARG;
      lrn_ctx* c = a.c;
      LzResPair ra;
      ra.r[0] = LzRes{a.M, a.Q, a.Y, a.PA, a.ab, a.flag};
      ra.r[1] = LzRes{b.M, b.Q, b.Y, b.PA, b.ab, b.flag};
      int wh_step = -1, wh_wg = -1;
      if (c->lz_wh_left > 0 && --c->lz_wh_left == 0) {      // test hook lz_test_withhold: this launch is the armed one
        wh_step = c->lz_wh_step == 0 ? j0 : c->lz_wh_step == 1 ? j0 + (j1 - j0) / 2 : j1 - 1;
        wh_wg = 64 * std::min(c->lz_wh_run, nruns - 1) + (c->lz_wh_wg ? nwg - 1 : 0);
        c->lz_wh_fired += 1;
      }
      c->counts["lz_resident_launches"] += 1;
      hipLaunchKernelGGL(lz_resident_kernel, dim3(nwg, nruns), dim3(256), (size_t)3 * n * 8, a.st, ra, n, nwg, j0, j1, qmod,
                         c->lz_res_limit, wh_step, wh_wg);
      break;
    }
    case LZ_FUSED: {
      if (n > LZ_FUSED_MAX) return LRN_ERR_ARG;
      const size_t lds = (size_t)n * 8;
      LzPair p;
      const LzWork* r[2] = {&a, &b};
      for (int k = 0; k < 2; ++k) { p.M[k] = r[k]->M; p.Q3[k] = r[k]->Q; p.Y2[k] = r[k]->Y; p.PA2[k] = r[k]->PA; p.ab[k] = r[k]->ab; }
      for (int j = j0; j <= j1; ++j) {
        // the launch after the last step only finishes it, one workgroup per run (the host needs alpha, beta of every step)
        const int do_symv = j < j1 ? 1 : 0;
        const dim3 grid(do_symv ? nwg : 1, nruns);
        if (nruns == 2) hipLaunchKernelGGL(lz_fused_pair_kernel, grid, dim3(256), lds, a.st, p, n, nwg, j, do_symv, qmod);
        else hipLaunchKernelGGL(lz_fused_kernel, grid, dim3(256), lds, a.st, a.M, n, nwg, j, do_symv, qmod, a.Q, a.Y, a.PA, a.ab);
      }
      break;
    }
    case LZ_TWO_KERNEL: {
      if (nruns != 1) return LRN_ERR_ARG;
      int nchunk, cper;
      lz_chunks(n, &nchunk, &cper);
      for (int j = j0; j < j1; ++j) {
        hipLaunchKernelGGL(symv_part_kernel, dim3((n + 255) / 256, nchunk), dim3(256), 0, a.st, a.M, n, cper, a.Q, a.PA);
        lz_step(a, j);
      }
      break;
    }
  }
  return hipGetLastError() == hipSuccess ? LRN_OK : LRN_ERR_HIP;
}

int lz_fetch(lrn_ctx* c, LzWork* const w[], int nruns, int m, bool* gave_up) {
  unsigned fl[2][2] = {{0u, 0u}, {0u, 0u}};
  for (int k = 0; k < nruns; ++k) {
    w[k]->hab.resize(2 * (size_t)m);
    LRN_HIP(c, hipMemcpyAsync(w[k]->hab.data(), w[k]->ab, (size_t)2 * m * 8, hipMemcpyDeviceToHost, w[0]->st));
    if (w[k]->form == LZ_RESIDENT) LRN_HIP(c, hipMemcpyAsync(fl[k], w[k]->flag, 8, hipMemcpyDeviceToHost, w[0]->st));
  }
  LRN_HIP(c, hipStreamSynchronize(w[0]->st));
  *gave_up = fl[0][1] != 0u || fl[1][1] != 0u;
  return LRN_OK;
}

void lz_record_give_up(lrn_ctx* c) {
  c->lz_no_persist = true;
  c->counts["lz_persist_abort"] += 1;
}

// (the eigenvalues of the tridiagonal matrices: tridiag.h -- bisection on a division-free Sturm count, bracket from the
// previous batch's value)

// |beta_m * s_m| for the Ritz pair (theta, s) of T_m: the residual norm ||M v - theta v|| of the
// Ritz vector, a rigorous bound on the distance from theta to the spectrum.  s by two steps of
// inverse iteration on the tridiagonal matrix (Thomas algorithm with a tiny shift).
static double ritz_residual(const std::vector<double>& a, const std::vector<double>& b, int m, double theta) {
  if (m <= 1) return 0.0;
  std::vector<double> s(m, 1.0 / std::sqrt((double)m)), d(m), u(m), y(m);
  double scale = 0.0;
  for (int i = 0; i < m; ++i) scale = std::max(scale, std::fabs(a[i]) + (i < m - 1 ? std::fabs(b[i]) : 0.0));
  const double shift = theta - 1e-13 * std::max(scale, 1e-300) - 1e-300;
  for (int it = 0; it < 3; ++it) {
    // solve (T - shift I) y = s  (T - shift I is positive definite up to rounding)
    d[0] = a[0] - shift;
    if (d[0] == 0.0) d[0] = 1e-300;
    u[0] = s[0];
    for (int i = 1; i < m; ++i) {
      double l = b[i - 1] / d[i - 1];
      d[i] = a[i] - shift - l * b[i - 1];
      if (d[i] == 0.0) d[i] = 1e-300;
      u[i] = s[i] - l * u[i - 1];
    }
    y[m - 1] = u[m - 1] / d[m - 1];
    for (int i = m - 2; i >= 0; --i) y[i] = (u[i] - b[i] * y[i + 1]) / d[i];
    double nrm = 0.0;
    for (int i = 0; i < m; ++i) nrm += y[i] * y[i];
    nrm = std::sqrt(nrm);
    if (!(nrm > 0.0) || !std::isfinite(nrm)) return std::fabs(b[m - 1]);
    for (int i = 0; i < m; ++i) s[i] = y[i] / nrm;
  }
  return std::fabs(b[m - 1] * s[m - 1]);
}

// One Lanczos iteration as a resumable run: batches of 16 steps are queued on the run's stream, the (alpha, beta)
// pairs come back in one copy per batch and the host decides on the tridiagonal matrix.  The two eigmin calls of a
// step-length search run side by side: in one launch per pair of steps (lz_drive with two runs), or, above LZ_FUSED_MAX,
// as two launch chains on two streams (eigmin_dev_pair).
struct LzRun {
  LzWork w;
  double *Y[2] = {}, *PA[2] = {};           // w.Y, w.PA of the launched forms [0] and of the resident one [1] (lz_set_form)
  int mmax = 0, m = 0, m1 = 0;
  std::vector<double> a, b;
  double theta = 0.0, theta_prev = 0.0, scale = 0.0;
  double last_move = 0.0;                   // |theta - theta_prev| of the last collect: how far the next one is expected to move
  int mc = 0;                               // steps whose coefficients the host holds (lz_collect); a batch [mc, m1) may be queued ahead
  bool ahead = false;
  double err_prev = 0.0, err_last = 0.0;    // residual / (1e-3 x its scale) at the last two looks (0: none): lz_queue_ahead
  bool have_prev = false, conv = false, done = false;
};

static void lz_set_form(LzRun& r, LzForm form) {
  r.w.form = form;
  r.w.Y = r.Y[form == LZ_RESIDENT];
  r.w.PA = r.PA[form == LZ_RESIDENT];
}

static int lz_begin(lrn_ctx* c, LzRun& r, const double* M, int n, hipStream_t st, DBuf& buf) {
  LzWork& w = r.w;
  w.c = c; w.M = M; w.n = n; w.st = st;
  w.nwg = (n + 15) / 16;
  // without re-orthogonalisation the extreme Ritz value may need more than n steps
  r.mmax = std::min(1500, 4 * n + 40);
  int nchunk, cper;
  lz_chunks(n, &nchunk, &cper);
  const size_t npa = (size_t)std::max(nchunk * n, 2 * w.nwg);
  LRN_TRY(ensure(c, buf, ((size_t)5 * n + npa + 2 * (size_t)r.mmax + 64 + 3 * (size_t)n + 3 * (size_t)w.nwg) * 8));
  w.Q = buf.as<double>();                 // fused: three vectors; two-kernel: q, q_prev
  r.Y[0] = w.Q + 3 * (size_t)n;
  r.PA[0] = r.Y[0] + 2 * (size_t)n;
  w.ab = r.PA[0] + npa;
  w.flag = reinterpret_cast<unsigned*>(w.ab + 2 * (size_t)r.mmax + 8);      // (inside the 64 doubles of slack)
  r.Y[1] = w.ab + 2 * (size_t)r.mmax + 64;
  r.PA[1] = r.Y[1] + 3 * (size_t)n;
  static const bool no_fused = getenv("LRN_LZ_UNFUSED") != nullptr;
  const bool fused = !no_fused && n <= LZ_FUSED_MAX && n >= 32 && ((size_t)n * 8 <= 60 * 1024 || lz_big_lds_ok());
  lz_set_form(r, !fused ? LZ_TWO_KERNEL : lz_resident_ok(c, n) ? LZ_RESIDENT : LZ_FUSED);
  return LRN_OK;
}

// start vector (after lz_begin; a fresh workspace is zeroed on c->stream, which w.st must have waited for)
static void lz_start(LzRun& r) {
  lz_prepare(r.w);
  hipLaunchKernelGGL(lz_init_kernel, dim3((r.w.n + 255) / 256), dim3(256), 0, r.w.st, r.w.Q, r.w.n);
  lz_step(r.w, -1);
}

// the next batch of steps of one run, or of two in lock-step (one launch per pair of steps, on r[0]'s stream)
static int lz_launch(LzRun* r, int nr) {
  const int batch = r[0].w.n <= 16 ? r[0].w.n : 16;
  const int m1 = std::min(r[0].mmax, r[0].m + batch);
  const LzWork* w[2] = {&r[0].w, &r[nr - 1].w};
  LRN_TRY(lz_queue_steps(w, nr, r[0].m, m1));
  for (int k = 0; k < nr; ++k) r[k].m1 = m1;
  return LRN_OK;
}

// waits for the batch in flight and brings its coefficients: r.mc steps are on the host afterwards.  *again: a resident
// launch gave up -- from now on launched steps on this context, and these runs are back at their start vector with nothing
// queued: the caller launches and collects again
static int lz_collect(lrn_ctx* c, LzRun* r, int nr, bool* again) {
  LzWork* w[2] = {&r[0].w, &r[nr - 1].w};
  LRN_TRY(lz_fetch(c, w, nr, r[0].m1, again));
  if (*again) lz_record_give_up(c);
  for (int k = 0; k < nr; ++k) {
    if (*again) {
      lz_set_form(r[k], LZ_FUSED);          // (only fused runs are resident)
      r[k].m1 = 0; r[k].have_prev = false; r[k].scale = 0.0;
      r[k].err_prev = r[k].err_last = 0.0;
      lz_start(r[k]);
    }
    r[k].mc = r[k].m = r[k].m1;
    r[k].ahead = false;
  }
  return LRN_OK;
}

// A run that is alone on the GPU (its partner of eigmin_dev_pair has ended, or eigmin_dev) leaves the stream empty while
// the host looks at T: a synchronisation, a bisection, an inverse iteration and the first launch of the next batch, ~50 us
// per 117 us batch (maxG11: 7.3 us per step in runs of 16-30 steps, 12 in runs of 120).  Between lz_collect and lz_decide:
// when the last two looks say that the coming one cannot end the run -- the residual, extrapolated geometrically, stays
// above 1e-2 of its scale, out of reach of every rule of lz_decide (the Kato-Temple rule needs 1e-3, the plain one 1e-11;
// the sign-class rule is excluded by theta < 0) -- the next batch is queued before that look.  Timing only: the looks and
// their verdicts are the same; a batch queued in vain is ignored (eigmin_dev_pair makes c->stream wait for it).
static bool lz_cannot_end_at_next_look(const LzRun& r) {
  static const bool off = getenv("LRN_LZ_NOAHEAD") != nullptr;      // (measurement knob)
  if (off || r.ahead || r.mc >= r.mmax || !(r.err_prev > 0.0) || !(r.err_last > 0.0)) return false;
  if (!(r.theta_prev < 0.0)) return false;
  const double next = r.err_last * std::min(1.0, r.err_last / r.err_prev);
  return next > 10.0;
}

// (runs in lock-step: only when none of them can end)
static int lz_queue_ahead(lrn_ctx* c, LzRun* r, int nr) {
  for (int k = 0; k < nr; ++k)
    if (!lz_cannot_end_at_next_look(r[k])) return LRN_OK;
  LRN_TRY(lz_launch(r, nr));          // (r.m == r.mc: the batch [mc, m1))
  for (int k = 0; k < nr; ++k) r[k].ahead = true;
  c->counts["lanczos_ahead"] += 1;
  return LRN_OK;
}

// the look at T of the fetched steps: r.done when converged, settled or out of steps
static int lz_decide(lrn_ctx* c, LzRun& r) {
  const int m1 = r.mc;
  const int mm_ = std::min(m1, tri_unpack(r.w.hab, m1, 1e-14, r.a, r.b, r.scale) + 1);      // < m1: invariant subspace
  // T of the previous batch is a leading block of this one: its smallest eigenvalue bounds this one from above
  r.theta = tri_eig_kth(r.a, r.b, mm_, 0, r.have_prev ? &r.theta_prev : nullptr, r.last_move);
  if (mm_ < m1) { r.conv = true; r.done = true; return LRN_OK; }
  // stop on the rigorous residual bound; for a clearly non-negative spectrum (theta > 0 is an
  // upper bound of lambda_min) the callers only need the sign class once theta has settled
  const double res = ritz_residual(r.a, r.b, mm_, r.theta);
  r.err_prev = r.err_last;
  r.err_last = res / (1e-3 * std::max(std::max(std::fabs(r.theta), 1e-4 * r.scale), 1e-300));
  if (res <= 1e-11 * std::max(std::fabs(r.theta), 1e-4 * r.scale)) { r.conv = true; r.done = true; return LRN_OK; }
  // Kato-Temple: theta - lambda_min <= res^2 / (lambda_2 - theta).  lambda_2 is bounded below through the second Ritz
  // pair (an eigenvalue lies within res2 of theta2; if that eigenvalue is lambda_min itself -- a ghost copy -- the gap
  // below is <= 0 and the rule does not fire).  The step-length rule consumes lambda_min to ~1e-10 relative.
  static const double kt_tol = getenv("LRN_EIGMIN_KT") ? atof(getenv("LRN_EIGMIN_KT")) : 1e-10;
  if (kt_tol > 0.0 && mm_ >= 8 && r.theta <= -1e-6 && res <= 1e-3 * std::max(std::fabs(r.theta), 1e-4 * r.scale)) {
    const double th2 = tri_eig_kth(r.a, r.b, mm_, 1);
    const double res2 = ritz_residual(r.a, r.b, mm_, th2);
    const double gap = (th2 - res2) - r.theta;
    if (gap > 0.0 && res < 0.25 * gap && res * res / gap <= kt_tol * std::fabs(r.theta)) {
      r.conv = true; r.done = true;
      return LRN_OK;
    }
  }
  if (r.have_prev && r.theta > 0.0 && std::fabs(r.theta - r.theta_prev) <= 1e-3 * r.theta && r.mc >= 64) { r.done = true; return LRN_OK; }
  r.last_move = r.have_prev ? std::fabs(r.theta - r.theta_prev) : 0.0;
  r.theta_prev = r.theta;
  r.have_prev = true;
  if (r.mc >= r.mmax) r.done = true;
  return LRN_OK;
}

// Both ends of the spectrum of a symmetric matrix from `nsteps` plain Lanczos steps: lo = smallest Ritz value (an UPPER
// bound of lambda_min), hi = largest Ritz value, res_hi = residual norm of its Ritz pair (an eigenvalue lies within res_hi
// of hi).  For the scaling of the Newton-Schulz iteration (prepw.hip), where a wrong value costs steps, not correctness.
int lanczos_ends(lrn_ctx* c, const double* M, int n, int nsteps, double* lo, double* hi, double* res_hi) {
  LzRun r;
  LRN_TRY(lz_begin(c, r, M, n, c->stream, c->lzbuf));
  r.mmax = std::min(r.mmax, std::max(4, nsteps));
  lz_start(r);
  for (bool again = true; again;) {          // (all batches queued at once; again: lz_collect)
    while (r.m < r.mmax) {
      LRN_TRY(lz_launch(&r, 1));
      r.m = r.m1;
    }
    LRN_TRY(lz_collect(c, &r, 1, &again));
  }
  const int m = r.m;
  std::vector<double> a, b, an(m);
  double scale = 0.0;
  const int mm_ = std::min(m, tri_unpack(r.w.hab, m, 1e-14, a, b, scale) + 1);      // < m: invariant subspace, the Ritz values are exact
  if (!(scale == scale) || mm_ < 1) return set_error(c, LRN_ERR_STATE, "lanczos_ends: not a finite matrix");
  for (int j = 0; j < mm_; ++j) an[j] = -a[j];
  *lo = tri_eig_kth(a, b, mm_, 0);
  const double top = -tri_eig_kth(an, b, mm_, 0);    // largest eigenvalue of T = - smallest of -T (same off-diagonal)
  *hi = top;
  *res_hi = mm_ < m ? 0.0 : ritz_residual(an, b, mm_, -top);
  c->counts["lanczos_ends_steps"] += m;
  return LRN_OK;
}

// batches of one run, or of two in lock-step, until one of them is done
static int lz_batches(lrn_ctx* c, LzRun* r, int nr) {
  while (!r[0].done && !r[nr - 1].done) {
    bool again = false;
    if (!r[0].ahead) LRN_TRY(lz_launch(r, nr));
    LRN_TRY(lz_collect(c, r, nr, &again));
    if (again) continue;
    LRN_TRY(lz_queue_ahead(c, r, nr));          // (alone on the GPU: see there)
    for (int k = 0; k < nr; ++k) LRN_TRY(lz_decide(c, r[k]));
    if (nr == 2) {
      c->counts["lanczos_pair_batches"] += 1;
      if (r[0].w.form == LZ_RESIDENT) c->counts["lanczos_resident_batches"] += 1;
    }
  }
  return LRN_OK;
}

static int lz_results(lrn_ctx* c, const LzRun* r, int nr, double* lam, bool* conv, double* scale) {
  for (int k = 0; k < nr; ++k) {
    lam[k] = r[k].theta; conv[k] = r[k].conv; scale[k] = r[k].scale;
    c->counts["lanczos_steps"] += r[k].m;
    c->counts["lanczos_runs"] += 1;
  }
  LRN_HIP(c, hipGetLastError());
  return LRN_OK;
}

// Started runs to their end.  Two of them (same n and mmax, both fused, on one stream) go in lock-step, one launch per pair
// of steps (lz_fused_pair_kernel, or both in a resident launch), until the first is done; the longer one goes on alone (a
// pair batch queued ahead carries its steps [mc, m1) already).
static int lz_drive(lrn_ctx* c, LzRun* r, int nr, double* lam, bool* conv, double* scale) {
  LRN_TRY(lz_batches(c, r, nr));
  for (int k = 0; k < nr; ++k) LRN_TRY(lz_batches(c, r + k, 1));
  return lz_results(c, r, nr, lam, conv, scale);
}

int eigmin_dev(lrn_ctx* c, const double* M, int n, double* lam, int* steps_out, bool* converged, double* scale_out) {
  if (converged) *converged = true;
  if (scale_out) *scale_out = 0.0;
  if (n == 1) {
    LRN_TRY(copy_out(c, lam, M, 8));
    if (steps_out) *steps_out = 1;
    return LRN_OK;
  }
  LzRun r;
  LRN_TRY(lz_begin(c, r, M, n, c->stream, c->lzbuf));
  lz_start(r);
  bool conv = false;
  double scale = 0.0;
  LRN_TRY(lz_drive(c, &r, 1, lam, &conv, &scale));
  if (steps_out) *steps_out = r.m;
  if (converged) *converged = conv;
  if (scale_out) *scale_out = scale;
  return LRN_OK;
}

// The Lanczos runs of two matrices of the same size side by side: results as from two eigmin_dev calls.  Option
// eigmin_pair = 2 (default): both runs in one launch per step (lz_drive).  1, or n > LZ_FUSED_MAX or < 32: the second run
// on c->stream2, which first waits for everything queued on c->stream; their batches alternate, each run's next one queued
// as soon as its look is over, so that the other stream's batch keeps the GPU busy during a look.
static int eigmin_dev_pair(lrn_ctx* c, const double* M1, const double* M2, int n, double lam[2], bool conv[2],
                           double scale[2]) {
  LzRun r[2];
  LRN_TRY(lz_begin(c, r[0], M1, n, c->stream, c->lzbuf));
  LRN_TRY(lz_begin(c, r[1], M2, n, c->stream, c->lzbuf2));
  if (c->opt.eigmin_pair >= 2 && r[0].w.form != LZ_TWO_KERNEL && r[1].w.form != LZ_TWO_KERNEL && r[0].mmax == r[1].mmax) {
    lz_start(r[0]);
    lz_start(r[1]);
    return lz_drive(c, r, 2, lam, conv, scale);
  }
  if (!c->stream2) LRN_HIP(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
  r[1].w.st = c->stream2;
  LRN_HIP(c, hipEventRecord(c->ev1, c->stream));             // the matrices, and the zeroing of a fresh workspace
  LRN_HIP(c, hipStreamWaitEvent(c->stream2, c->ev1, 0));
  lz_start(r[0]);
  lz_start(r[1]);
  LRN_TRY(lz_launch(&r[0], 1));
  LRN_TRY(lz_launch(&r[1], 1));
  while (!r[0].done || !r[1].done) {
    for (int k = 0; k < 2; ++k) {
      if (r[k].done) continue;
      bool again = false;
      LRN_TRY(lz_collect(c, &r[k], 1, &again));
      if (!again) {
        if (r[1 - k].done) LRN_TRY(lz_queue_ahead(c, &r[k], 1));      // (otherwise the other run's batch keeps the GPU busy meanwhile)
        LRN_TRY(lz_decide(c, r[k]));
      }
      if (!r[k].done && !r[k].ahead) LRN_TRY(lz_launch(&r[k], 1));
    }
  }
  if (r[1].ahead) {                          // a batch queued in vain on stream2 still reads M2 and its workspace
    LRN_HIP(c, hipEventRecord(c->ev1, c->stream2));
    LRN_HIP(c, hipStreamWaitEvent(c->stream, c->ev1, 0));
  }
  return lz_results(c, r, 2, lam, conv, scale);
}

// ---- certified smallest eigenvalue
// A Ritz value is only an UPPER bound of lambda_min, and plain Lanczos resolves the spectrum relative to
// its spread: lambda_min = -1 next to eigenvalues of 1e6..1e10 (a poor direction after a regularised
// Schur solve) comes back as -0.94 or even +9 -- the step-length rule (predictor_corrector.jl:272-291)
// would then leave the cone.  Every estimate is therefore certified by one Cholesky test
//   M - (theta - delta) I  positive definite  <=>  lambda_min > theta - delta,
// and if the test fails lambda_min is bracketed by bisection over such tests (the reference calls a
// dense `eigmin`; a positive-definiteness test is its GEMM-rich equivalent on this hardware).
static int chol_shift_is_pd(lrn_ctx* c, const double* M, int n, double shift, bool* pd) {
  hipStream_t st = c->stream;
  LRN_TRY(ensure(c, c->info_dev, 64));
  const size_t nn = (size_t)n * n;
  LRN_TRY(ensure(c, c->ezbuf, (nn + chol_work_doubles(n) + 64) * 8));
  double* F = c->ezbuf.as<double>();
  double* work = F + nn;
  int* info = c->info_dev.as<int>() + 8;
  LRN_HIP(c, hipMemcpyAsync(F, M, nn * 8, hipMemcpyDeviceToDevice, st));
  add_diag_mat(st, F, n, shift);
  LRN_HIP(c, hipMemsetAsync(info, 0, 4, st));
  LRN_TRY(potrf_lower(st, F, n, n, work, info));
  int h = 0;
  LRN_TRY(copy_out(c, &h, info, 4));
  *pd = h == 0;
  c->counts["eigmin_chol_tests"] += 1;
  return LRN_OK;
}

static int eigmin_certify(lrn_ctx* c, const double* M, int n, double theta, bool conv, double scale, double* lam);

int eigmin_certified(lrn_ctx* c, const double* M, int n, double* lam) {
  double theta = 0.0, scale = 0.0;
  bool conv = false;
  LRN_TRY(eigmin_dev(c, M, n, &theta, nullptr, &conv, &scale));
  return eigmin_certify(c, M, n, theta, conv, scale, lam);
}

// eigmin_certified of two matrices of the same size: the two Lanczos runs interleaved, then the certificates
int eigmin_certified_pair(lrn_ctx* c, const double* M1, const double* M2, int n, double* lam1, double* lam2) {
  if (n == 1 || !c->opt.eigmin_pair) {
    LRN_TRY(eigmin_certified(c, M1, n, lam1));
    return eigmin_certified(c, M2, n, lam2);
  }
  double th[2], sc[2];
  bool cv[2];
  LRN_TRY(eigmin_dev_pair(c, M1, M2, n, th, cv, sc));
  LRN_TRY(eigmin_certify(c, M1, n, th[0], cv[0], sc[0], lam1));
  return eigmin_certify(c, M2, n, th[1], cv[1], sc[1], lam2);
}

static int eigmin_certify(lrn_ctx* c, const double* M, int n, double theta, bool conv, double scale, double* lam) {
  static const bool trace = getenv("LRN_EIGMIN_TRACE") != nullptr;
  if (trace) fprintf(stderr, "[eigmin n=%d] theta=%.12g conv=%d scale=%.3g\n", n, theta, (int)conv, scale);
  if (n == 1) { *lam = theta; return LRN_OK; }
  // a Ritz value converged to 1e-11 on a spectrum of moderate spread (the usual O(1) scaled directions)
  // needs no certificate: the failures are unconverged runs on spectra spanning 1e6 and more
  if (conv && theta <= -1e-6 && scale <= 1e3 * std::fabs(theta)) { *lam = theta; return LRN_OK; }
  bool pd = false;
  if (theta > -1e-6) {
    // callers only use the class "lambda_min > -1e-6" (step 0.99, DIMACS err2/err4 = 0)
    LRN_TRY(chol_shift_is_pd(c, M, n, 1e-6, &pd));
    if (pd) { *lam = theta; return LRN_OK; }
  } else {
    const double delta = 1e-7 * std::fabs(theta);
    LRN_TRY(chol_shift_is_pd(c, M, n, delta - theta, &pd));
    if (pd) { *lam = theta; return LRN_OK; }
  }
  // the Ritz value was not converged: bracket lambda_min in (lo, hi], hi = theta is an upper bound
  c->counts["eigmin_bisections"] += 1;
  double hi = theta, beta = std::max(2.0 * std::fabs(theta), 1.0);
  for (int it = 0; it < 200; ++it) {
    LRN_TRY(chol_shift_is_pd(c, M, n, beta, &pd));
    if (pd) break;
    hi = std::min(hi, -beta);
    beta *= 4.0;
  }
  if (!pd) return set_error(c, LRN_ERR_STATE, "eigmin: matrix has no finite lower bound (NaN/Inf entries?)");
  double lo = -beta;
  for (int it = 0; it < 100 && hi - lo > 1e-9 * std::max(std::fabs(lo), 1e-6); ++it) {
    const double mid = 0.5 * (lo + hi);
    LRN_TRY(chol_shift_is_pd(c, M, n, -mid, &pd));
    if (trace) fprintf(stderr, "   bisect mid=%.12g pd=%d\n", mid, (int)pd);
    if (pd) lo = mid; else hi = mid;
  }
  *lam = lo;          // the safe side: slightly too negative shortens the step
  return LRN_OK;
}

}  // namespace lrn
