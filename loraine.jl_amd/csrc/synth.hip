// Synthetic data generated on the device: the dense Philox model (lrn_synthetic_dense_model) and the problem on top of it.
#include <cmath>
#include <cstring>
#include <algorithm>
#include <numeric>

#include "ctx.h"
#include "ops.h"

namespace lrn {

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

}  // namespace lrn

using namespace lrn;

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
  LRN_TRY(upload(c, b.ent_ptr, std::vector<long>(nvar + 1, 0)));
  LRN_TRY(ensure(c, b.ent_r, 8));
  LRN_TRY(ensure(c, b.ent_c, 8));
  LRN_TRY(ensure(c, b.ent_v, 8));
  LRN_TRY(upload(c, b.hidx, b.sigma));
  LRN_TRY(upload(c, b.sigma_d, b.sigma));
  LRN_TRY(upload(c, b.ipos_d, b.ipos));
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
