// Schur assembly for stored constraints with a small support (option "pair_local"): finite-element data, where
// A_i touches a handful of degrees of freedom S_i and is dense on them.  With s = |S|, Ah = A[S, S] and Wij = W[S_i, S_j]
//     tr(A_i W A_j W) = <Ah_i Wij Ah_j, Wij>_F = sum_{a,c} (Ah_i Wij)[a,c] (Wij Ah_j')[a,c]
// for every entry list, symmetric or not (W is symmetric): two independent s_i x s_j products of 2 s_i s_j (s_i + s_j) flop
// instead of the s_i^2 s_j^2 gather terms of pair_wave_kernel (schur.hip), and s_i s_j reads of W instead of twice that many
// terms.  Both products land in the same accumulator layout of v_mfma_f64_16x16x4_f64, so their entrywise product needs no
// shuffle.  The lists S_p, Ah_p and the owner range [loc_lo, loc_hi) come from model_layout.h::block_local; every partner
// of such an owner has a support of at most LOCAL_SUPPORT_MAX = 32 indices, two tiles of 16 a side.
#include "model_layout.h"
#include "ops.h"

namespace lrn {

constexpr int LC_LD = 33;          // leading dimension of a wave's W tile in LDS (32 rows + 1: column reads shift by one bank pair)
constexpr int LC_WAVES = 4;        // waves of a workgroup
constexpr int LC_SLICE = 32;       // partners of one workgroup: eight a wave
static_assert(LOCAL_SUPPORT_MAX == 32, "local_pair_kernel holds two 16-tiles a side");

// One workgroup: owner pi = p_lo + blockIdx.y, partners pj = pi + LC_SLICE blockIdx.x + (wave, wave + 4, ...) below p_end; one
// wave works on one pair at a time and on nothing else, so the waves of a workgroup share no data and meet at no barrier.
// The owner's side lives in registers for the life of the wave: its support index S_i[lane % Ri] (Ri = s_i rounded up to 16) and
// the sixteen A-operand fragments of Ah_i (two row tiles x eight K-steps, zero outside s_i x s_i).
// Per pair, with lane = (ci = lane & 15, kq = lane >> 4) -- the operand map test_mfma_f64_lane_map pins: A[ci][kq], B[kq][ci]:
//   1. gather: Wt[a + LC_LD c] = W[S_i[a], S_j[c]] for a < Ri, c < Rj, exact zeros beyond s_i, s_j.  Lanes run along S_i: a run of
//      consecutive degrees of freedom is one run of addresses in a column of W.
//   2. per output tile (ti, tj):  P = Ah_i Wt  (A = the register fragment, B = Wt[4 kk + kq, 16 tj + ci]),
//                                 Q = Wt Ah_j' (A = Wt[16 ti + ci, 4 kk + kq], B = Ah_j[16 tj + ci, 4 kk + kq] from global memory:
//      consecutive ci are consecutive addresses), K-steps up to s_i and s_j; then acc += P[0] Q[0] + ... + P[3] Q[3], tiles in
//      the order (tj, ti).
//   3. shuffle tree over the 64 lanes (offsets 32 .. 1), and lane 0 adds to H as pair_wave_kernel does.
// Every sum has a fixed order that depends on (s_i, s_j) alone: no atomics, the same bits whatever the slicing.
// LDS: 4 x 32 x 33 doubles = 33 KB a workgroup.  Bounds: a + LC_LD c <= 31 + 33 * 31 < 32 * 33; the K-steps read rows / columns below
// Ri / Rj, which step 1 has written; W, sup and Ah are read under the masks a < s_i, c < s_j only.
__global__ __launch_bounds__(64 * LC_WAVES) void local_pair_kernel(
    const long* __restrict__ sptr, const int* __restrict__ sup, const long* __restrict__ aptr, const double* __restrict__ Ah,
    const double* __restrict__ W, int msz, int p_lo, int p_hi, int p_end, const int* __restrict__ hidx, double* __restrict__ H,
    int ldh) {
  __shared__ double Wt_all[LC_WAVES * 32 * LC_LD];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ci = lane & 15, kq = lane >> 4;
  const int pi = p_lo + blockIdx.y;
  if (pi >= p_hi) return;
  const int j0 = pi + blockIdx.x * LC_SLICE;
  if (j0 >= p_end) return;
  const int j1 = min(j0 + LC_SLICE, p_end);
  double* Wt = Wt_all + wv * 32 * LC_LD;

  const long si0 = sptr[pi];
  const int s_i = __builtin_amdgcn_readfirstlane((int)(sptr[pi + 1] - si0));
  if (s_i <= 0) return;                                // (no owner of the range is empty: it has pair_local_min entries)
  const int nti = (s_i + 15) >> 4, Ri = nti << 4;
  const int ga = lane & (Ri - 1);                      // this lane's row of the gather
  const bool ga_in = ga < s_i;
  const long wrow = ga_in ? (long)sup[si0 + ga] : 0;
  const double* Ai = Ah + aptr[pi];
  double ai[2][8];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int r = 16 * ti + ci, k = 4 * kk + kq;
      ai[ti][kk] = (r < s_i && k < s_i) ? Ai[r + k * s_i] : 0.0;
    }
  const int hi = hidx[pi];

  for (int pj = j0 + wv; pj < j1; pj += LC_WAVES) {
    const long sj0 = sptr[pj];
    const int s_j = __builtin_amdgcn_readfirstlane((int)(sptr[pj + 1] - sj0));
    if (s_j <= 0) continue;                            // (nor a partner below npos_nz)
    const int ntj = (s_j + 15) >> 4, Rj = ntj << 4;
    const double* Aj = Ah + aptr[pj];
    // 1. the tile of W
    const int cstep = 64 / Ri, nit = Rj / cstep;        // columns per pass, passes (<= 16)
    const int c_lane = lane / Ri;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      if (it < nit) {
        const int cc = c_lane + it * cstep;
        double v = 0.0;
        if (ga_in && cc < s_j) v = W[wrow + (long)sup[sj0 + cc] * msz];
        Wt[ga + LC_LD * cc] = v;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // 2. the two products, tile by tile
    double acc = 0.0;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      if (tj < ntj) {
        double bj[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          const int r = 16 * tj + ci, k = 4 * kk + kq;
          bj[kk] = (r < s_j && k < s_j) ? Aj[r + k * s_j] : 0.0;
        }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
          if (ti < nti) {
            v4f64 P = {0.0, 0.0, 0.0, 0.0}, Q = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
              if (4 * kk < s_i) P = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[ti][kk], Wt[4 * kk + kq + LC_LD * (16 * tj + ci)], P, 0, 0, 0);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
              if (4 * kk < s_j) Q = __builtin_amdgcn_mfma_f64_16x16x4f64(Wt[16 * ti + ci + LC_LD * (4 * kk + kq)], bj[kk], Q, 0, 0, 0);
            acc += P[0] * Q[0] + P[1] * Q[1] + P[2] * Q[2] + P[3] * Q[3];
          }
        }
      }
    }
    // 3. one sum, one store
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) H[h_lower(hi, hidx[pj], ldh)] += acc;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the next pair's gather overwrites the tile
    __builtin_amdgcn_wave_barrier();
  }
}

// the device copies of the lists, on the first assembly that takes the route (or the long route's MFMA kernel, longops.hip)
int local_upload(lrn_ctx* c, LmiBlock& b) {
  if (b.loc_ready) return LRN_OK;
  LRN_TRY(upload(c, b.loc_sptr_d, b.loc_sptr));
  LRN_TRY(upload(c, b.loc_aptr_d, b.loc_aptr));
  LRN_TRY(upload(c, b.loc_sup_d, b.loc_sup));
  LRN_TRY(upload(c, b.loc_a_d, b.loc_a));
  for (auto* v : {&b.loc_sptr, &b.loc_aptr}) std::vector<long>().swap(*v);
  std::vector<int>().swap(b.loc_sup);
  std::vector<double>().swap(b.loc_a);
  b.loc_ready = true;
  return LRN_OK;
}

int assemble_local(lrn_ctx* c, LmiBlock& b) {
  LRN_TRY(local_upload(c, b));
  tic(c);
  long pairs = 0;
  for (int a = b.loc_lo; a < b.loc_hi; a += 2048) {
    const int e = std::min(b.loc_hi, a + 2048);
    dim3 grid((b.npos_nz - a + LC_SLICE - 1) / LC_SLICE, e - a);
    hipLaunchKernelGGL(local_pair_kernel, grid, dim3(64 * LC_WAVES), 0, c->stream, b.loc_sptr_d.as<long>(), b.loc_sup_d.as<int>(),
                       b.loc_aptr_d.as<long>(), b.loc_a_d.as<double>(), b.W.as<double>(), b.msz, a, e, b.npos_nz,
                       b.hidx.as<int>(), c->H.as<double>(), c->nvar);
    for (int p = a; p < e; ++p) pairs += b.npos_nz - p;
  }
  toc(c, "local");
  c->counts["pair_local_owners"] += b.loc_hi - b.loc_lo;
  c->counts["pair_local_pairs"] += pairs;
  return LRN_OK;
}

}  // namespace lrn
