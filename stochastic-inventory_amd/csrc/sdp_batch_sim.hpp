// sdp_batch_sim.hpp -- forward simulation of ALL instances of a solved batch in one launch (sdpgpu_batch_simulate*,
// sdpgpu_batch.hip): the loop of Simulation.simulateSDPGivenSamplNum (Simulation.java:59-69) on every instance's own
// CLSPTesting lambdas (CLSPTesting.java:89-106), one demand path per lane, with the demand of a (path, period) either read
// from memory or DRAWN here (Sampling.generateLHSamples, Sampling.java:86-103, made reproducible).
//
//   * a wave's 64 paths belong to ONE instance (the paths of an instance are padded to whole waves), so the instance's
//     record -- costs, inventory bounds, order limit, state count, the base of its policy rows --, its sampler records and
//     its policy-row offsets are wave-uniform loads;
//   * ONE kernel rolls the table policy and the (s, S) level rules (sdp_fitss.hpp): batch_sim_kernel is a template over a
//     RULE -- a small struct that picks the period's order and says where the period starts from -- and everything else of
//     a path (demand, f1_sim_period, sums, wave total) is written once.  f1_sim_period is cell<FAM_BACKORDER> of sdp_device.hpp
//     (simulate_kernel of sdp_gather.hpp with discount 1.0: `1.0 * imm` is `imm`), so a path's sum under the table rule has
//     the bits sdpgpu_simulate gives on a handle of the instance;
//   * the sampler ("Batched simulation"): stratum j = sigma(p) of path p, a = 53 bits of Philox4x32-10 at counter
//     (j, t, instance, 0) under the caller's seed, u = j / n + a / n, demand = k_lo + #{thresholds <= u} (or < u for an
//     integer-valued distribution) by binary search in the host-made table of the (instance, period).  The tables are a few
//     KB per instance and shared by every lane of its waves: they are read through L1/L2, not staged in LDS;
//   * the mean of an instance is formed in a fixed order -- xor-butterfly over the wave, then the wave partials of the
//     instance in index order by one thread (batch_sim_mean_kernel): no floating-point atomics, the same bits every call.
//
// Global memory is written with ordinary vector stores from plain C++ only.
#pragma once
#include "sdp_sampler.hpp"

namespace sdp {

// An instance's costs, its OWN grid (the instances of a ragged batch differ in it), its order limit and the base of its policy
// rows; wave-uniform in the rollout.
struct SimInst {
  double h, pi, K, v;
  double min_inventory, max_inventory;
  double maxq;       // order limit (the level rules cap their orders at it)
  int64_t pol_base;  // the instance's policy rows [T][n_states] in the batch's policy arena (the table rule)
  int32_t n_states, pad;
};

struct SimLaunch {
  double step, inv_step;
  int32_t T, n_inst;
  int32_t waves_per_inst;  // ceil(n_paths / 64)
  int64_t demand_stride;   // explicit demands: elements between the demand sets of two instances (0: one shared set)
  SimStream R;             // n_paths, and the latin hypercube's seed and sigma width (first_path is not used: 0)
};

// demand of path p of (instance, t), and the uniform it came from
__device__ __forceinline__ double sim_draw(const SimLaunch& L, const SimSampler& S, const double* __restrict__ thr, int inst, int t,
                                           uint32_t p, double* u_out) {
  const double u = sim_uniform_lhs(L.R.n_paths, L.R.half_bits, L.R.seed_lo, L.R.seed_hi, inst, t, p);
  *u_out = u;
  return sim_demand(S, thr, nullptr, u);
}

// One period of the backorder family from inventory x under order a and demand d: immediateValue and the clamped
// stateTransition (decode_state / action_setup / cell of sdp_device.hpp; CLSP.java:255-272), one operation per statement.
struct F1SimPeriod {
  double imm, level;  // the period's cost, and the next inventory clamped into the instance's bounds
};
__device__ __forceinline__ F1SimPeriod f1_sim_period(const SimInst& I, double x, double a, double d) {
  const double fixed = a > 0 ? I.K : 0.0;
  const double var = I.v * a;
  const double fv = fixed + var;
  const double base = x + a;
  const double level = base - d;
  const double hold = I.h * fmax(level, 0.0);
  const double pen = I.pi * fmax(-level, 0.0);
  const double imm = fv + hold + pen;
  double nx = level;
  nx = nx > I.max_inventory ? I.max_inventory : nx;
  nx = nx < I.min_inventory ? I.min_inventory : nx;
  return F1SimPeriod{imm, nx};
}

// The table rule: the order is the policy row's entry at the state's grid index.  The state is SNAPPED to the grid every
// period -- the index of the carried level truncated toward zero, the period then starts from min + idx * step --, as a
// handle's rollout does.
struct TableRule {
  const int32_t* __restrict__ policy;
  __device__ __forceinline__ const int32_t* rows(const SimLaunch&, const SimInst& I, int) const { return policy + I.pol_base; }
  __device__ __forceinline__ double act(const SimLaunch& L, const SimInst& I, const int32_t* __restrict__ pol, int t, double* x) const {
    int idx = (int)((*x - I.min_inventory) * L.inv_step);  // (inv_step is exact; of a start state: the host's division by step)
    idx = idx < 0 ? 0 : (idx >= I.n_states ? I.n_states - 1 : idx);  // (a NaN demand must not leave the policy row)
    *x = I.min_inventory + (double)idx * L.step;
    return (double)pol[(int64_t)t * I.n_states + idx] * L.step;
  }
};

// One demand path per lane under RULE (TableRule above, LevelRule<1 | 2 | 3> of sdp_fitss.hpp).  The body carries x -- the
// start inventory, then each period's clamped level --; rule.rows gives what the rule reads of instance i, rule.act the
// period's order, and may move x to the inventory the period is evaluated at.
template <class RULE, bool SAMPLED>
__global__ __launch_bounds__(256) void batch_sim_kernel(SimLaunch L, const SimInst* __restrict__ inst, const double* __restrict__ ini_x,
                                                        RULE rule, const double* __restrict__ demand, const SimSampler* __restrict__ samp,
                                                        const double* __restrict__ thr, double* __restrict__ partial,
                                                        double* __restrict__ out_sum) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t gw = (int64_t)blockIdx.x * 4 + wave;
  if (gw >= (int64_t)L.n_inst * L.waves_per_inst) return;  // no workgroup barrier below: a wave may leave on its own
  const int i = (int)(gw / L.waves_per_inst);              // (wave-uniform)
  const int w = (int)(gw - (int64_t)i * L.waves_per_inst);
  const int p = w * 64 + lane;
  const int n_paths = (int)L.R.n_paths;
  const SimInst I = inst[i];
  double sum = 0.0;
  if (p < n_paths) {
    double x = ini_x[i];
    const auto rows = rule.rows(L, I, i);
    const double* __restrict__ dem = SAMPLED ? nullptr : demand + (int64_t)i * L.demand_stride + (int64_t)p * L.T;
    for (int t = 0; t < L.T; ++t) {
      double d;
      if constexpr (SAMPLED) {
        double u;
        d = sim_draw(L, samp[(int64_t)i * L.T + t], thr, i, t, (uint32_t)p, &u);
      } else {
        d = dem[t];
      }
      const double a = rule.act(L, I, rows, t, &x);
      const F1SimPeriod s = f1_sim_period(I, x, a, d);
      sum += s.imm;
      x = s.level;
    }
    if (out_sum) out_sum[(int64_t)i * n_paths + p] = sum;
  }
  // wave total in a fixed order (lanes past n_paths hold 0.0)
  const double tot = sim_wave_sum(sum);
  if (lane == 0) partial[gw] = tot;
}

// mean of every instance: its wave partials in index order, then one division
__global__ __launch_bounds__(256) void batch_sim_mean_kernel(const double* __restrict__ partial, int n_inst, int waves_per_inst, int n_paths,
                                                             double* __restrict__ out_mean) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_inst) return;
  double s = 0.0;
  for (int w = 0; w < waves_per_inst; ++w) s += partial[(int64_t)i * waves_per_inst + w];
  out_mean[i] = s / (double)n_paths;
}

// the demands (and uniforms) batch_sim_kernel<true> uses for ONE instance, by the same sim_draw: out[p * T + t]
__global__ __launch_bounds__(256) void batch_sim_draw_kernel(SimLaunch L, int inst, const SimSampler* __restrict__ samp,
                                                             const double* __restrict__ thr, double* __restrict__ out_demand,
                                                             double* __restrict__ out_u) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)L.R.n_paths) return;
  for (int t = 0; t < L.T; ++t) {
    double u;
    const double d = sim_draw(L, samp[(int64_t)inst * L.T + t], thr, inst, t, (uint32_t)p, &u);
    out_demand[p * L.T + t] = d;
    if (out_u) out_u[p * L.T + t] = u;
  }
}

}  // namespace sdp
