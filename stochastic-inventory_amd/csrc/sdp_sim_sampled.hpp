// sdp_sim_sampled.hpp -- sample-and-roll on a HANDLE in one launch (sdpgpu_simulate_sampled, sdpgpu_sample_demands;
// sdpgpu_simsample.hip): what `new Simulation(distributions, sampleNum, recursion).simulateSDPGivenSamplNum(initialState)`
// does after a solve (Simulation.java:53-74; CashSimulation.java:85-118; RiskSimulation.java:206-241), and the plain-random
// draws of simulateSDPwithErrorConfidence (Simulation.java:76-107), for every family sdpgpu_simulate serves.
//
//   * one demand path per lane; per period the demand is DRAWN (sim_uniform_lhs / sim_uniform_random and sim_demand of
//     sdp_sampler.hpp: the batch's sampler with the instance position fixed at 0), then sim_period_step of sdp_gather.hpp
//     -- the statements of simulate_kernel -- rolls the path on: a path's sum has the bits sdpgpu_simulate gives on the
//     demands sdpgpu_sample_demands returns;
//   * the period records, the sampler records and the discount weights are the same for every lane (wave-uniform loads);
//     the threshold tables (T of them, a few KB) are read through L1 / L2 as in the batch;
//   * the mean and the second moment are formed in an order fixed by n_paths alone, without floating-point atomics
//     ("Sampled simulation on a handle"): xor-butterfly over the wave (lanes past n_paths hold 0.0), the wave
//     partials then by ONE workgroup of 1024 threads -- thread i adds the C = ceil(W / 1024) consecutive partials
//     i C .. i C + C - 1 in index order, and the 1024 thread sums go through a binary tree in LDS.  The longest chain of
//     additions is L(n) = 6 + C + 10, W = ceil(n / 64): 17 for n <= 65536, 272 at the cap of 2^24 paths.
//
// Global memory is written with ordinary vector stores from plain C++ only.
#pragma once
#include "sdp_gather.hpp"
#include "sdp_sampler.hpp"

namespace sdp {

template <bool RANDOM>
__device__ __forceinline__ double sim_stream_uniform(const SimStream& R, int t, uint32_t p) {
  if constexpr (RANDOM)
    return sim_uniform_random(R.seed_lo, R.seed_hi, t, R.first_path + (uint64_t)p);
  else
    return sim_uniform_lhs(R.n_paths, R.half_bits, R.seed_lo, R.seed_hi, 0, t, p);
}

// counts[0] paths with bit 0 of the flags (valid), counts[1] with bit 1 (a demand was lost): integer atomics, one per wave
template <int FAM, bool RANDOM>
__global__ __launch_bounds__(256) void sim_sampled_kernel(const SimPeriod* __restrict__ per, int T, const int32_t* __restrict__ pol,
                                                          const SimSampler* __restrict__ samp, const double* __restrict__ thr,
                                                          const double* __restrict__ val, const double* __restrict__ disc, SimStream R,
                                                          int64_t idx0, StateT ini, int first_k, double* __restrict__ out_sum,
                                                          uint8_t* __restrict__ out_flags, double* __restrict__ partial,
                                                          unsigned int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const uint32_t gw = blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t p = gw * 64u + (uint32_t)lane;
  if (gw * 64u >= R.n_paths) return;  // no workgroup barrier below: a wave may leave on its own
  double sum = 0.0;
  bool valid = false, lost = false;
  if (p < R.n_paths) {
    int64_t idx = idx0;
    StateT s = ini;
    valid = true;
    for (int t = 0; t < T && valid; ++t) {
      const double u = sim_stream_uniform<RANDOM>(R, t, p);
      const double d = sim_demand(samp[t], thr, val, u);
      sim_period_step<FAM>(per[t], pol, t == 0 && idx0 < 0, first_k, d, disc[t], idx, s, sum, valid, lost);
    }
    out_sum[p] = sum;
    out_flags[p] = (valid ? 1 : 0) | (lost ? 2 : 0);
  }
  const unsigned long long mv = __ballot(valid), ml = __ballot(lost);
  const double tot = sim_wave_sum(sum);
  if (lane == 0) {
    partial[gw] = tot;
    atomicAdd(&counts[0], (unsigned int)__popcll(mv));
    if (ml) atomicAdd(&counts[1], (unsigned int)__popcll(ml));
  }
}

// second pass over the device-resident sums: wave partials of (sum_p - mean)^2, the same order as the first
__global__ __launch_bounds__(256) void sim_dev2_kernel(const double* __restrict__ sums, uint32_t n, const double* __restrict__ mean_ptr,
                                                       double* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const uint32_t gw = blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t p = gw * 64u + (uint32_t)lane;
  if (gw * 64u >= n) return;
  const double mean = *mean_ptr;
  double v = 0.0;
  if (p < n) {
    const double dv = sums[p] - mean;
    v = dv * dv;
  }
  const double tot = sim_wave_sum(v);
  if (lane == 0) partial[gw] = tot;
}

// ONE workgroup of 1024 threads: out[0] = sum of the W partials in the fixed order above, divided by `divisor` when it is not
// 0; NaN when `counts` is given and fewer than n_paths paths were valid (sdpgpu_simulate_sampled: mean and m2 of a run with
// invalid paths)
__global__ __launch_bounds__(1024) void sim_reduce_kernel(const double* __restrict__ partial, uint32_t W, double divisor,
                                                          const unsigned int* __restrict__ counts, uint32_t n_paths,
                                                          double* __restrict__ out) {
  __shared__ double s_v[1024];
  const uint32_t i = threadIdx.x;
  const uint32_t C = (W + 1023u) / 1024u;
  double s = 0.0;
  for (uint32_t k = 0; k < C; ++k) {
    const uint32_t w = i * C + k;
    if (w < W) s += partial[w];
  }
  s_v[i] = s;
  __syncthreads();
  for (uint32_t h = 512; h >= 1; h >>= 1) {
    if (i < h) s_v[i] = s_v[i] + s_v[i + h];
    __syncthreads();
  }
  if (i == 0) {
    double r = s_v[0];
    if (divisor != 0.0) r = r / divisor;
    if (counts && counts[0] < n_paths) r = __builtin_nan("");
    out[0] = r;
  }
}

// the demands (and uniforms) sim_sampled_kernel uses, by the same device functions: out[p * T + t]
template <bool RANDOM>
__global__ __launch_bounds__(256) void sim_sampled_draw_kernel(SimStream R, int T, const SimSampler* __restrict__ samp,
                                                               const double* __restrict__ thr, const double* __restrict__ val,
                                                               double* __restrict__ out_demand, double* __restrict__ out_u) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= R.n_paths) return;
  for (int t = 0; t < T; ++t) {
    const double u = sim_stream_uniform<RANDOM>(R, t, p);
    out_demand[(int64_t)p * T + t] = sim_demand(samp[t], thr, val, u);
    if (out_u) out_u[(int64_t)p * T + t] = u;
  }
}

}  // namespace sdp
