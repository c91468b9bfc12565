// sdp_sampler.hpp -- the device sampler of the simulation kernels ("Batched simulation" and "Sampled simulation on a
// handle"): Philox4x32-10, the keyed bijection sigma of the latin hypercube's shuffle, the two streams of uniforms and the
// demand of a uniform by binary search in a host-made threshold table -- and the wave total every rollout ends with, with the
// wave prologue and epilogue of the rule kernels (sdp_cash_rule_sim.hpp, sdp_xr_sim.hpp, sdp_staff_sim.hpp).  Shared by every
// simulation kernel: records and device functions only, no kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sdp {

// threshold table of one (instance, period) of a batch, [instance * T + t], or of one period of a handle, [t]
struct SimSampler {
  int64_t off;     // element offset of the ascending thresholds in the threshold arena
  int32_t k_lo;    // demand of a u below the first threshold
  int32_t m;       // thresholds
  int32_t strict;  // 1: demand = k_lo + #{c < u} (inverseF of an integer-valued distribution); 0: #{c <= u}
  int32_t pad;
  // >= 0: the demand is the q-th VALUE of a table at this element offset of the value arena (a handle's pmf tile may have
  // gaps and a step other than 1: sdpgpu_simulate_sampled); -1: the demand is k_lo + q (specs, and every table of a batch)
  int64_t val_off;
};

// what identifies the stream of uniforms of one call (host: make_stream, sdpgpu_sim_host.hpp)
struct SimStream {
  uint64_t first_path;  // RANDOM mode: 64-bit index of the call's path 0
  uint32_t n_paths;
  uint32_t seed_lo, seed_hi;
  int32_t half_bits;    // LHS mode: sigma's half width (smallest h >= 1 with 4^h >= n_paths)
};

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
struct Philox4 {
  uint32_t v[4];
};
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the round function of sigma's Feistel network: a 32-bit integer finaliser ("lowbias32")
__device__ __forceinline__ uint32_t sim_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// sigma_{instance, t}: a bijection of [0, n).  Eight Feistel rounds over 2 h bits (4^h >= n), round keys = the eight words
// Philox gives at the counters (0, t, instance, 1) and (1, t, instance, 1); a result >= n is fed through again (cycle walking).
__device__ __forceinline__ uint32_t sim_sigma(uint32_t p, uint32_t n, int h, const uint32_t* rk) {
  const uint32_t mask = (1u << h) - 1u;
  uint32_t x = p;
  do {
    uint32_t l = x >> h, r = x & mask;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint32_t f = sim_mix32(r + rk[q]) & mask;
      const uint32_t nl = r;
      r = l ^ f;
      l = nl;
    }
    x = (l << h) | r;
  } while (x >= n);
  return x;
}

// the latin-hypercube uniform of path p of column (instance, t): stratum j = sigma(p), u = j / n + a / n
__device__ __forceinline__ double sim_uniform_lhs(uint32_t n, int half_bits, uint32_t seed_lo, uint32_t seed_hi, int inst, int t, uint32_t p) {
  const Philox4 ka = philox4x32_10(0u, (uint32_t)t, (uint32_t)inst, 1u, seed_lo, seed_hi);
  const Philox4 kb = philox4x32_10(1u, (uint32_t)t, (uint32_t)inst, 1u, seed_lo, seed_hi);
  const uint32_t rk[8] = {ka.v[0], ka.v[1], ka.v[2], ka.v[3], kb.v[0], kb.v[1], kb.v[2], kb.v[3]};
  const uint32_t j = sim_sigma(p, n, half_bits, rk);
  const Philox4 r = philox4x32_10(j, (uint32_t)t, (uint32_t)inst, 0u, seed_lo, seed_hi);
  const uint64_t bits = (((uint64_t)r.v[0] << 32) | (uint64_t)r.v[1]) >> 11;
  const double a = (double)bits * 0x1p-53;                  // [0, 1), as Math.random()
  return (double)j / (double)n + a / (double)n;             // Sampling.java:94
}

// the plain-random uniform of path P (64 bits) in period index t (Sampling.generateRanSamples, Sampling.java:50-60): word 3
// of the counter (2) keeps the stream apart from the latin hypercube's uniforms (0) and shuffle keys (1)
__device__ __forceinline__ double sim_uniform_random(uint32_t seed_lo, uint32_t seed_hi, int t, uint64_t path) {
  const Philox4 r = philox4x32_10((uint32_t)(path & 0xffffffffu), (uint32_t)t, (uint32_t)(path >> 32), 2u, seed_lo, seed_hi);
  const uint64_t bits = (((uint64_t)r.v[0] << 32) | (uint64_t)r.v[1]) >> 11;
  return (double)bits * 0x1p-53;
}

// demand of a uniform: q = #{thresholds <= u} (or < u) by binary search, then k_lo + q or the q-th value of the table
__device__ __forceinline__ double sim_demand(const SimSampler& S, const double* __restrict__ thr, const double* __restrict__ val, double u) {
  const double* __restrict__ c = thr + S.off;
  int lo = 0, hi = S.m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double cv = c[mid];
    const bool below = S.strict ? cv < u : cv <= u;
    if (below)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (S.val_off >= 0) return val[S.val_off + (lo < S.m ? lo : S.m - 1)];
  return (double)(S.k_lo + lo);
}

// wave total by xor butterfly: every lane ends with the same bits
__device__ __forceinline__ double sim_wave_sum(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// Where a wave of a rule kernel stands (256-thread blocks; the waves of rule r are waves_per_rule * r ..).  A kernel opens with
//   SimWave wv;  if (wv.leaves(n_rules, waves_per_rule)) return;  wv.place(waves_per_rule);
// and has no workgroup barrier below that: a wave past the launch's last one may leave on its own.
struct SimWave {
  int lane;
  int64_t gw;  // the wave's place in the launch
  int ri;      // its rule (wave-uniform)
  uint32_t p;  // the lane's path (or leaf) of that rule
  __device__ __forceinline__ SimWave() {
    lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    gw = (int64_t)blockIdx.x * 4 + wave;
  }
  __device__ __forceinline__ bool leaves(int n_rules, uint32_t waves_per_rule) const { return gw >= (int64_t)n_rules * waves_per_rule; }
  __device__ __forceinline__ void place(uint32_t waves_per_rule) {
    ri = (int)(gw / waves_per_rule);
    const uint32_t w = (uint32_t)(gw - (int64_t)ri * waves_per_rule);
    p = w * 64u + (uint32_t)lane;
  }
};

// what a rule kernel's wave ends with: its total into partial[gw], its valid paths onto counts[2 * ri] (one integer atomic)
template <class RI>
__device__ __forceinline__ void sim_wave_finish(double* __restrict__ partial, unsigned int* __restrict__ counts, int64_t gw, RI ri, bool valid,
                                                double sum) {
  const unsigned long long mv = __ballot(valid);
  const double tot = sim_wave_sum(sum);
  if ((threadIdx.x & 63) == 0) {
    partial[gw] = tot;
    atomicAdd(&counts[2 * ri], (unsigned int)__popcll(mv));
  }
}

}  // namespace sdp
