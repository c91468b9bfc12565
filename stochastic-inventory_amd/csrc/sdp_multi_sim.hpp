// sdp_multi_sim.hpp -- the rollout of a two-product policy on the device (sdpgpu_multi_policy_*, sdpgpu_multisim.hip): what
// CashSimulationMulti.simulateSDPGivenSamplNum[Multi] (CashSimulationMulti.java:71-84, :104-114) and
// CashSimulationMultiXR.simulateSDPGivenSamplNum (CashSimulationMultiXR.java:72-83) do with `recursion.getAction(state)`.
// Definition: DESIGN 4, "Two-product rollout"; tests/multi_sim_twin.py is written from the reference's lines.
//
//   * the states of these families lie on no grid, so getAction is a SEARCH in the memo: an open-addressing hash table over
//     the memo's (period, state tuple) keys.  The memo rows are stored once, as 64-byte aligned records (tuple, period, action
//     pair), and the table itself is an array of 32-bit row indices: a probe reads a slot word and, where it is taken, ONE
//     line.  The hash is the engine's tuple_hash with the period mixed in (sdp_multi_device.hpp);
//   * multi_policy_insert_kernel: a memo row per lane, linear probing, a slot claimed by a 32-bit atomicCAS.  A slot whose
//     record has an equal key is a duplicate (the sort-based forward pass can produce them): with equal actions the lower row
//     index stays, with different ones the two row indices go to the error word and create refuses the memo.  Every probe loop
//     is bounded by the capacity; no lane waits for another;
//   * multi_sim_kernel<MODEL, SOURCE>: a path per lane, the periods serial: probe, read the record, immediate value and
//     successor through the engine's own device functions with is_last set in period T.  A miss ends the path: its sum is NaN
//     and its valid flag 0.  SOURCE: the demand pairs GIVEN by the caller, or drawn -- one uniform per (path, period index) from
//     the streams of sdp_sampler.hpp (instance position 0), which picks a ROW of the period's joint tile by the running sum of
//     its probabilities (multi_draw; multi_sample_kernel writes the same draws out);
//   * reduction as in every other rollout: wave totals by xor butterfly into partial[wave], then sim_reduce_kernel and
//     sim_dev2_kernel in their fixed order (launch_sim_moments).
//
// Global memory is written with ordinary vector stores from plain C++ and integer atomics; no floating-point atomics.
#pragma once
#include "sdp_multi_device.hpp"
#include "sdp_sampler.hpp"

namespace sdp_multi {

constexpr int MS_SOURCE_LHS = 0;
constexpr int MS_SOURCE_RANDOM = 1;
constexpr int MS_SOURCE_GIVEN = 2;

constexpr uint32_t kSlotEmpty = 0xffffffffu;

// one memo row: the key (period, tuple) and the action pair (order-up-to levels for the XR family)
struct alignas(64) PolicyRecord {
  Tuple s;
  int32_t period;
  int32_t a1, a2;
  int32_t pad;
};
static_assert(sizeof(PolicyRecord) == 64, "a probe hit reads one 64-byte line");

struct PolicyTable {
  const PolicyRecord* __restrict__ rec;
  const uint32_t* __restrict__ slots;  // mask + 1 row indices, kSlotEmpty where free
  uint32_t mask;
};

__device__ __forceinline__ unsigned long long policy_hash(int period, const Tuple& t) { return mix64(tuple_hash(t), (double)period); }

__device__ __forceinline__ bool policy_key_eq(const PolicyRecord& r, int period, const Tuple& t) { return r.period == period && tuple_eq(r.s, t); }

// getAction(state): false where the memo holds no such state.  At most mask + 1 slots are read.
__device__ __forceinline__ bool policy_probe(const PolicyTable& H, int period, const Tuple& t, int& a1, int& a2) {
  uint32_t pos = (uint32_t)policy_hash(period, t) & H.mask;
  for (uint32_t k = 0; k <= H.mask; ++k) {
    const uint32_t row = H.slots[pos];
    if (row == kSlotEmpty) return false;
    const PolicyRecord& r = H.rec[row];
    if (policy_key_eq(r, period, t)) {
      a1 = r.a1;
      a2 = r.a2;
      return true;
    }
    pos = (pos + 1u) & H.mask;
  }
  return false;
}

// err[0]: 0, or (lower row + 1) << 32 | (higher row + 1) of the first pair of equal keys with different actions seen
__global__ __launch_bounds__(256) void multi_policy_insert_kernel(const PolicyRecord* __restrict__ rec, uint32_t rows, uint32_t* slots,
                                                                  uint32_t mask, unsigned long long* err) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= rows) return;
  const PolicyRecord me = rec[r];
  uint32_t pos = (uint32_t)policy_hash(me.period, me.s) & mask;
  for (uint32_t k = 0; k <= mask; ++k) {
    uint32_t cur = __atomic_load_n(&slots[pos], __ATOMIC_RELAXED);
    if (cur == kSlotEmpty) {
      cur = atomicCAS(&slots[pos], kSlotEmpty, r);
      if (cur == kSlotEmpty) return;  // claimed
    }
    // the slot belongs to another row (a slot once taken only ever changes to a row of the same key)
    const PolicyRecord o = rec[cur];
    if (policy_key_eq(o, me.period, me.s)) {
      if (o.a1 == me.a1 && o.a2 == me.a2) {
        atomicMin(&slots[pos], r);  // keep the first
      } else {
        const uint32_t lo = r < cur ? r : cur, hi = r < cur ? cur : r;
        atomicCAS(err, 0ull, ((unsigned long long)(lo + 1u) << 32) | (unsigned long long)(hi + 1u));
      }
      return;
    }
    pos = (pos + 1u) & mask;
  }
  // (not reached: the host makes the capacity larger than the row count)
}

// the probe alone, one state per lane
__global__ __launch_bounds__(256) void multi_lookup_kernel(PolicyTable H, int64_t n, const int32_t* __restrict__ period,
                                                           const double* __restrict__ i1, const double* __restrict__ i2,
                                                           const double* __restrict__ q1, const double* __restrict__ q2,
                                                           const double* __restrict__ cash, int32_t* __restrict__ a1,
                                                           int32_t* __restrict__ a2, uint8_t* __restrict__ found) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Tuple t{i1[i], i2[i], q1[i], q2[i], cash[i]};
  int b1 = 0, b2 = 0;
  const bool hit = policy_probe(H, period[i], t, b1, b2);
  a1[i] = b1;
  a2[i] = b2;
  found[i] = hit ? 1 : 0;
}

// a call's wave-uniform constants
struct MultiSimLaunch {
  MLParams P;           // overhead, nd and is_last are set per period by the kernel
  double overhead[16];
  double disc[16];
  int32_t off[17];      // joint tile of period index t: elements [off[t], off[t + 1]) of the pair and threshold arenas
  int32_t T;
  Tuple ini;
};

// The demand pair of (path p, period index t): u from the call's stream, row q = #{c <= u} of the period's tile (sim_demand
// with k_lo 0 on the tile's thresholds, the last of which is +infinity).
template <int SOURCE>
__device__ __forceinline__ double2 multi_draw(const MultiSimLaunch& L, const sdp::SimStream& R, const double* __restrict__ thr,
                                              const double2* __restrict__ dem, int t, uint32_t p, double& u) {
  u = SOURCE == MS_SOURCE_RANDOM ? sdp::sim_uniform_random(R.seed_lo, R.seed_hi, t, R.first_path + (uint64_t)p)
                                 : sdp::sim_uniform_lhs(R.n_paths, R.half_bits, R.seed_lo, R.seed_hi, 0, t, p);
  sdp::SimSampler S{};
  S.off = L.off[t];
  S.k_lo = 0;
  S.m = L.off[t + 1] - L.off[t];
  S.strict = 0;
  S.val_off = -1;
  int q = (int)sdp::sim_demand(S, thr, nullptr, u);
  q = q < S.m ? q : S.m - 1;
  return dem[L.off[t] + q];
}

// one period of one path: the immediate value of (state, action pair, demand pair); before period T the state becomes its
// successor.  a1, a2: the memo's action pair (model 2: order-up-to levels).
template <int MODEL>
__device__ __forceinline__ double multi_step(const MLParams& P, Tuple& s, int a1, int a2, double d1, double d2) {
  double imm;
  if constexpr (MODEL == 1) {
    imm = mc_immediate(P, s, a1, a2, d1, d2);
    if (!P.is_last) s = mc_successor(P, s, a1, a2, d1, d2);
  } else if constexpr (MODEL == 2) {
    const double y1 = (double)a1, y2 = (double)a2;
    imm = xr_immediate(P, s, y1, y2, d1, d2);
    if (!P.is_last) s = xr_successor(P, s, y1, y2, d1, d2);
  } else {
    // cashIncrement (MultiProductLeadtime.java:162-198) as the backward pass forms it: the action-only part, then the demand's
    const double oc = P.vari[0] * (double)a1 + P.vari[1] * (double)a2;
    const double before = s.cash - oc - P.overhead;
    const double bi = before - ml_interest(P, before);
    imm = cash_increment(s, bi, demand_terms(P, s, d1, d2));
    if (!P.is_last) {
      const double2 d = make_double2(d1, d2);
      s = successor(P, s, a1 * P.qb + a2, &d, 0);
    }
  }
  return imm;
}

// counts[0]: valid paths (integer atomics, one per wave) -- what sim_reduce_kernel compares with n_paths
template <int MODEL, int SOURCE>
__global__ __launch_bounds__(256) void multi_sim_kernel(MultiSimLaunch L, sdp::SimStream R, PolicyTable H, const double* __restrict__ thr,
                                                        const double2* __restrict__ dem, const double* __restrict__ given1,
                                                        const double* __restrict__ given2, double* __restrict__ out_sum,
                                                        uint8_t* __restrict__ out_valid, double* __restrict__ partial,
                                                        unsigned int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const uint32_t gw = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (gw * 64u >= R.n_paths) return;  // no workgroup barrier below: a wave may leave on its own
  const uint32_t p = gw * 64u + (uint32_t)lane;
  const bool live = p < R.n_paths;
  double sum = 0.0;
  bool valid = false;
  if (live) {
    MLParams P = L.P;
    Tuple s = L.ini;
    valid = true;
    for (int t = 0; t < L.T && valid; ++t) {
      P.overhead = L.overhead[t];
      P.nd = L.off[t + 1] - L.off[t];
      P.is_last = t == L.T - 1;
      double2 d;
      if constexpr (SOURCE == MS_SOURCE_GIVEN) {
        d = make_double2(given1[(int64_t)p * L.T + t], given2[(int64_t)p * L.T + t]);
      } else {
        double u;
        d = multi_draw<SOURCE>(L, R, thr, dem, t, p, u);
      }
      int a1 = 0, a2 = 0;
      valid = policy_probe(H, t + 1, s, a1, a2);
      if (valid) sum += L.disc[t] * multi_step<MODEL>(P, s, a1, a2, d.x, d.y);
    }
    if (!valid) sum = __builtin_nan("");
    out_sum[p] = sum;
    if (out_valid) out_valid[p] = valid ? 1 : 0;
  }
  const unsigned long long ml = __ballot(valid);
  const double tot = sdp::sim_wave_sum(sum);
  if (lane == 0) {
    partial[gw] = tot;
    atomicAdd(&counts[0], (unsigned int)__popcll(ml));
  }
}

// the draws of the sampled rollout, written out: d1 / d2 / u [p * T + t] (out_u may be null)
template <int SOURCE>
__global__ __launch_bounds__(256) void multi_sample_kernel(MultiSimLaunch L, sdp::SimStream R, const double* __restrict__ thr,
                                                           const double2* __restrict__ dem, double* __restrict__ out_d1,
                                                           double* __restrict__ out_d2, double* __restrict__ out_u) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= R.n_paths) return;
  for (int t = 0; t < L.T; ++t) {
    double u;
    const double2 d = multi_draw<SOURCE>(L, R, thr, dem, t, p, u);
    out_d1[(int64_t)p * L.T + t] = d.x;
    out_d2[(int64_t)p * L.T + t] = d.y;
    if (out_u) out_u[(int64_t)p * L.T + t] = u;
  }
}

}  // namespace sdp_multi
