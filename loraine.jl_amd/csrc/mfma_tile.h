// The 64 x 64 workgroup tile of the small FP64 MFMA products, device-only: geometry, lane maps, the two LDS panel layouts
// and the K loop.  Callers: diag_sq_mfma_kernel, diag_sq_wide_mfma_kernel (diagops.hip),
// ragged_blocksum_kernel (raggedops.hip), fac_quadform_kernel (facops.hip).  Each keeps its own bounds, the one value it
// transforms while staging, its epilogue, grid and LDS declarations.  Two kernels are the same tile WRITTEN OUT, because over
// mt_kloop they measured slower than they were (profiles/mfma_tile_refactor_ab.txt, item 4): ts_diag_mfma_kernel (diagops.hip;
// 120 registers for 116, 2 to 3 % at one diagonal row) and ragged_syrk_kernel (raggedops.hip; 0.4 to 1.0 % in most figures).
// A change to the loop below is to be made in those two as well.
//
// Tile: 256 threads, four waves, D = A B' over 64 rows of A x 64 rows of B, K walked in steps of 16 with the tail zero-filled
// by the caller's fetch.  Wave w owns the 32 x 32 block (wr, wc) = (w >> 1, w & 1) as 2 x 2 accumulators of
// v_mfma_f64_16x16x4_f64 (A: lane l holds A[l & 15][l >> 4], B: B[l >> 4][l & 15], C/D: col = l & 15, row = (l >> 4) + 4 reg),
// so with ci = l & 15, kq = l >> 4 register r of acc[ib][jb] is the element
//     row (A side) 32 wr + 16 ib + kq + 4 r,   column (B side) 32 wc + 16 jb + ci            (mt_row, mt_col)
// of the tile.  Which operand of a product is A and which is B is the caller's choice: the sixteen ci lanes run along B, so the
// side that is contiguous in the result goes there (ts_diag_mfma_kernel, ragged_syrk_kernel: 128-byte stores).
//
// Two LDS panels, one per operand, each 64 rows x 16 k in one of two layouts chosen by how the operand lies in memory:
//   MtRowK  [row][k], row stride 18 doubles, 9 216 bytes -- the operand is K-contiguous (a column of the matrix per tile row).
//           Staged by thread (k = t & 15, row = (t >> 4) + 16 pass): sixteen lanes read 128 contiguous bytes.
//   MtKRow  [k][row], row stride 80 doubles, 10 240 bytes -- the operand is contiguous along the tile rows.
//           Staged by thread (row = t & 63, k = (t >> 6) + 4 pass): a wave reads 512 contiguous bytes, and k is wave-uniform.
// LDS banks.  Fragment reads are ds_read_b64 (bank = dword address mod 64, conflicts within a 32-lane half); a half reads
// sixteen consecutive rows at k and k + 1.
//   MtRowK: 36 row mod 64 runs through the sixteen multiples of 4, the two dwords of an element and the two k fill the four
//           banks of each: conflict-free.
//   MtKRow: the rows k, k + 1 are 160 dwords apart, i.e. 32 mod 64, and sixteen consecutive doubles fill one half of the bank
//           row each: conflict-free.
//   Both derived from the bank rule, not measured.
// Staging writes are ds_write_b64 (bank = dword mod 32).  MtKRow: 32 lanes on consecutive doubles, 2 cycles, the minimum for
// 256 bytes.  MtRowK: 16 consecutive k per row, row stride 36 dwords: free of conflicts if stores are served in groups of 16
// contiguous lanes (one row each), two-way conflicted under a wider grouping (rows start at 0, 4, 8, 12 mod 32) -- not
// measured.
//
// K loop (mt_kloop): the global loads of step k + 1 are issued before the MFMAs of step k and waited for after them, two
// barriers per step.  The compiler's report with this body (registers, instruction counts, beside the written-out loops it
// replaced): profiles/mfma_tile_refactor_ab.txt.  The two diag_sq kernels and ragged_blocksum sit at 124 and fac_quadform at
// 120 of the 128 registers that four waves per SIMD allow: a change here is to be checked against that.
#pragma once
#include "lrn_common.h"

namespace lrn {

static constexpr int MT_T = 64;        // tile side
static constexpr int MT_K = 16;        // K step

// per-thread coordinates; the wave index goes through readfirstlane so that wr, wc are scalars
struct MtLane {
  int t, lane, wr, wc, ci, kq;
};
__device__ __forceinline__ MtLane mt_lane() {
  MtLane ln;
  ln.t = threadIdx.x;
  ln.lane = ln.t & 63;
  const int w = __builtin_amdgcn_readfirstlane(ln.t >> 6);
  ln.wr = w >> 1;
  ln.wc = w & 1;
  ln.ci = ln.lane & 15;
  ln.kq = ln.lane >> 4;
  return ln;
}

// panel layouts: at(row, k) = index of an element, srow / sk = what thread t stages in pass ps = 0 .. 3, SPASS = the index
// step from one pass to the next (mt_kloop stores pass ps at the index of pass 0 + ps SPASS: a constant LDS offset per pass)
struct MtRowK {
  static constexpr int LD = 18, SIZE = MT_T * LD, SPASS = 16 * LD;
  static __device__ __forceinline__ int at(int row, int k) { return row * LD + k; }
  static __device__ __forceinline__ int srow(int t, int ps) { return (t >> 4) + 16 * ps; }
  static __device__ __forceinline__ int sk(int t, int) { return t & 15; }
};
struct MtKRow {
  static constexpr int LD = 80, SIZE = MT_K * LD, SPASS = 4 * LD;
  static __device__ __forceinline__ int at(int row, int k) { return k * LD + row; }
  static __device__ __forceinline__ int srow(int t, int) { return t & 63; }
  static __device__ __forceinline__ int sk(int t, int ps) { return (t >> 6) + 4 * ps; }
};

// accumulator register r of acc[ib][jb] -> tile element
__device__ __forceinline__ int mt_row(const MtLane& ln, int ib, int r) { return 32 * ln.wr + 16 * ib + ln.kq + 4 * r; }
__device__ __forceinline__ int mt_col(const MtLane& ln, int jb) { return 32 * ln.wc + 16 * jb + ln.ci; }

// acc = sum over the K steps k0 = kbeg, kbeg + 16, .. < kend (int or long) of A-panel x B-panel'.
//   fetch(k0)          loads the caller's registers for step k0 (zeros outside its bounds);
//   stage(ps, &a, &b)  hands out what pass ps of this thread puts at (LA::srow, LA::sk) of As and (LB::srow, LB::sk) of Bs --
//                      the place of the one transformed value (b * b, b * u, sc * f).
// Every thread of the workgroup must call it: it holds the barriers.  As, Bs may be reused after one more barrier.
template <class LA, class LB, class KI, class Fetch, class Stage>
__device__ __forceinline__ void mt_kloop(const MtLane& ln, double* As, double* Bs, KI kbeg, KI kend,
                                         Fetch fetch, Stage stage, v4f64 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};
  const int sa = LA::at(LA::srow(ln.t, 0), LA::sk(ln.t, 0)), sb = LB::at(LB::srow(ln.t, 0), LB::sk(ln.t, 0));
  fetch(kbeg);
  for (KI k0 = kbeg; k0 < kend; k0 += MT_K) {
    __syncthreads();                       // the waves are done with the previous step's panels
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      double a, b;
      stage(ps, &a, &b);
      As[sa + ps * LA::SPASS] = a;
      Bs[sb + ps * LB::SPASS] = b;
    }
    __syncthreads();
    if (k0 + MT_K < kend) fetch(k0 + MT_K);
#pragma unroll
    for (int ks = 0; ks < MT_K / 4; ++ks) {
      const int k = 4 * ks + ln.kq;
      const double a0 = As[LA::at(32 * ln.wr + ln.ci, k)];
      const double a1 = As[LA::at(32 * ln.wr + 16 + ln.ci, k)];
      const double b0 = Bs[LB::at(32 * ln.wc + ln.ci, k)];
      const double b1 = Bs[LB::at(32 * ln.wc + 16 + ln.ci, k)];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
}

}  // namespace lrn
