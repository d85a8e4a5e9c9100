// Workgroup reductions (device only): one wave ladder, one combine through LDS.  The order of the operations is fixed -- lanes
// by the shuffle ladder 32 .. 1, waves left to right -- so every caller gets the same bits from the same values.
#pragma once
#include <hip/hip_runtime.h>

namespace lrn {

// v = op(v, the other lanes of the wave) by the ladder 32 .. 1 (valid in lane 0)
template <class Op>
__device__ __forceinline__ double wave_reduce(double v, Op op) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_down(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) { return wave_reduce(v, [](double a, double b) { return a + b; }); }
__device__ __forceinline__ double wave_min(double v) { return wave_reduce(v, [](double a, double b) { return fmin(a, b); }); }
__device__ __forceinline__ double wave_max(double v) { return wave_reduce(v, [](double a, double b) { return fmax(a, b); }); }

// sum over a workgroup of NW waves, in every thread; sh: NW doubles of LDS.  The leading barrier lets a kernel call it
// again on the same sh.  (The ladder is spelled out, not wave_sum(v): the compiler schedules the two differently, and the
// CG and Lanczos kernels are held to the instruction stream they had with their private copies of this function.)
template <int NW>
__device__ __forceinline__ double wg_sum(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < NW; ++i) s += sh[i];
  return s;
}

// part[0] + .. + part[np - 1] in every thread of a workgroup of 256: the second stage of a two-stage sum that every
// workgroup of the consumer takes itself, all in the same order
__device__ __forceinline__ double block_sum_parts(const double* __restrict__ part, int np, double* sh) {
  double s = 0.0;
  for (int e = threadIdx.x; e < np; e += 256) s += part[e];
  return wg_sum<4>(s, sh);
}

}  // namespace lrn
