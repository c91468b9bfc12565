// sdp_xr_sim.hpp -- rollouts of the (x, R) state of cash.singleItem.CashConstraintXR (family CASH, cash_formula 2) along demand
// paths (sdpgpu_xr_simulate, sdpgpu_xrsim.hip): what CashSimulationXR.simulateSDPGivenSamplNum (CashSimulationXR.java:91-113),
// the sampling loop of simulateSDPwithErrorConfidence (:115-147) and simulateAStar (:153-173) do, on the device.  Definition:
// DESIGN 4, "(x, R) rollout"; tests/xr_sim_twin.py is written from it.
//
//   * one (rule, path) per lane; the rule index is a dimension of the launch: a wave's 64 paths belong to ONE rule (the paths
//     of a rule are padded to whole waves), so the rule's level of the period is a wave-uniform load;
//   * the RULE is a struct the kernel calls once per period.  XrTableRule: the handle's policy table -- the period's statements
//     are sim_period_step<FAM_CASH> of sdp_gather.hpp (decode_state with xr_state, the policy gather, action_setup, cell): they
//     exist once.  XrLevelRule: Chao's a* levels -- y = R > c a_t ? a_t : R / c (CashSimulationXR.java:162), which is no grid
//     value, so the STATE IS TWO DOUBLES (x, R); the immediate value is cell<FAM_CASH> on the context action_setup_y fills
//     from the level, the transition the family's statements kept as doubles (CashConstraintXR.java:94-110);
//   * the SOURCE of the demands: drawn as sim_sampled_kernel draws them (sdp_sampler.hpp, instance position 0; latin hypercube
//     or plain random), or GIVEN by the caller [path * T + t].  The counters do not carry the rule: every rule of a call sees
//     the same demands, and the waves of rule 0 write them out when the caller asks for them;
//   * the period block, the policy row's place, the sampler record and the discount weight of a period are ONE wave-uniform
//     record (XrPeriod), read where it is used and not held in registers beside the sampler's round keys;
//   * reduction: wave total by xor butterfly (lanes past n_paths hold 0.0) into partial[rule][wave]; sim_reduce_kernel and
//     sim_dev2_kernel of sdp_sim_sampled.hpp then form mean and m2 of every rule in their fixed order.
//
// Global memory is written with ordinary vector stores from plain C++ only; no floating-point atomics.
#pragma once
#include "sdp_gather.hpp"
#include "sdp_sampler.hpp"

namespace sdp {

constexpr int XR_SOURCE_LHS = 0;
constexpr int XR_SOURCE_RANDOM = 1;
constexpr int XR_SOURCE_GIVEN = 2;

struct XrLaunch {
  double ini_x, ini_r;
  double vari_cost;  // the reference's constructor argument variOrderCost (the level rule's cap), not the descriptor's field
  int32_t T, n_rules;
  uint32_t waves_per_rule;
  int32_t pad;
};

// one period of the handle, wave-uniform
struct XrPeriod {
  SimPeriod S;  // the family's parameter block; pol_off / n_states of the policy row (the table rule)
  SimSampler samp;
  double disc;
};

// action_setup<FAM_CASH> for an order-up-to LEVEL that arrives as a double, the sibling of action_setup_q of sdp_device.hpp (the
// level is R / variCost where the working capital does not pay for a*): the statements of CashConstraintXR.java:79-84 on the
// level itself.  The level before demand IS y -- x + (y - x) need not return y once y is no grid value -- and the fixed cost
// tests y > x as the reference does.  s.cash holds initCash (xr_state).
__device__ __forceinline__ void action_setup_y(const DevParams& P, const StateT& s, double y, ActionCtx& c) {
  c.a = y - s.x;
  c.fixed = y > s.x ? P.K : 0.0;
  c.var = P.v * c.a;
  c.fv = c.fixed + c.var;
  c.before = 0;
  c.interest = 0;
  c.next_q_off = 0;
  c.base = y;
  c.deposit = (s.cash - c.fixed - c.var) * P.one_plus_deposit;
}

// the handle's policy table from the period-1 state (ini_x, ini_r): idx0 its flat index, or < 0 for an off-grid state whose
// action first_k comes from sdpgpu_eval_states
struct XrTableRule {
  const int32_t* __restrict__ pol;
  int64_t idx0;
  int32_t first_k;
  struct Path {
    int64_t idx;
    StateT s;
  };
  __device__ __forceinline__ void start(const XrLaunch& L, Path& a) const {
    a.idx = idx0;
    a.s.x = L.ini_x;
    a.s.cash = L.ini_r;
    a.s.preq = 0;
  }
  // false: the path ends here.  Only after period 1 from an off-grid start: an inventory off the grid stays off it unless the
  // period sells out or fills the shelf, and such a successor is no state of the table (the reference re-enters its recursion
  // there; the oracle ends the path, and so does sdpgpu_simulate_sampled's count of valid paths)
  __device__ __forceinline__ bool step(const XrLaunch&, const XrPeriod& Q, int, int t, double d, Path& a, double& sum) const {
    const DevParams& P = Q.S.P;
    const bool off_grid_first = t == 0 && idx0 < 0;
    if (off_grid_first) xr_state<FAM_CASH>(P, a.s, false);  // (the queried "cash" is R: gather_period_kernel's QUERY mode)
    bool valid = true, lost = false;                        // (both clamps are in the transition)
    sim_period_step<FAM_CASH>(Q.S, pol, off_grid_first, first_k, d, Q.disc, a.idx, a.s, sum, valid, lost);
    if (off_grid_first && !P.is_last) {
      double ninv = jmax(0.0, (a.s.x + (double)first_k * P.step) - d);
      ninv = ninv > P.max_inventory ? P.max_inventory : ninv;
      ninv = ninv < P.min_inventory ? P.min_inventory : ninv;
      const double fi = (ninv - P.next.x_lo) * P.inv_step;
      valid = fi == floor(fi);
    }
    return valid;
  }
};

// levels[rule * T + t] = a_t of the rule (RecursionG.getOptY, or any finite level)
struct XrLevelRule {
  const double* __restrict__ levels;
  struct Path {
    double x, r;
  };
  __device__ __forceinline__ void start(const XrLaunch& L, Path& a) const {
    a.x = L.ini_x;
    a.r = L.ini_r;
  }
  __device__ __forceinline__ bool step(const XrLaunch& L, const XrPeriod& Q, int rule, int t, double d, Path& a, double& sum) const {
    const DevParams& P = Q.S.P;
    const double lv = levels[(int64_t)rule * L.T + t];
    const double cap = L.vari_cost * lv;
    const double y = a.r > cap ? lv : a.r / L.vari_cost;  // CashSimulationXR.java:162 (a y below x sells stock back at cost)
    StateT s;
    s.x = a.x;
    s.cash = a.r;
    s.preq = 0;
    xr_state<FAM_CASH>(P, s, false);  // initCash = R - variCost * x (CashConstraintXR.java:83, :99)
    ActionCtx c;
    action_setup_y(P, s, y, c);
    int64_t ni = 0;
    const double imm = cell<FAM_CASH>(P, s, c, d, ni);
    sum += Q.disc * imm;
    if (!P.is_last) {  // the transition of cell<FAM_CASH> (CashConstraintXR.java:98-107), kept as doubles
      double ninv = jmax(0.0, c.base - d);
      ninv = ninv > P.max_inventory ? P.max_inventory : ninv;
      ninv = ninv < P.min_inventory ? P.min_inventory : ninv;
      const double k = (double)((int64_t)cash_index(P, s.cash + imm) + P.next.k_lo);
      const double ncash = P.cash_round_int_div ? k : k / P.round_div;
      const double vx = P.v * ninv;
      a.x = ninv;
      a.r = ncash + vx;
    }
    return true;  // (the state is two doubles: no path ever ends early)
  }
};

// The action of a period-1 state whose INVENTORY is no grid value (the table rule's start): ONE wave, lane = action slot, the
// demand sum serial in the reference's order as in gather_period_kernel, then the lexicographic (value, index) arg-opt over
// the wave.  Such a state's successors max(0, x + k - d) are grid states only where the period sells out or fills the shelf;
// sdpgpu_eval_states' query mode would read V_2 at the truncated inventory index there.  Here a successor that is no grid
// state is worth 0.0, which is what the oracle's rollout takes for it (its dense look-up), so that the action, and with it
// period 1's term of every path, is the oracle's.  v_next: V_2 (nullptr when T == 1).
__global__ __launch_bounds__(64) void xr_first_action_kernel(DevParams P, const double* __restrict__ v_next,
                                                             const double* __restrict__ pmf_d, const double* __restrict__ pmf_p,
                                                             double ini_x, double ini_r, int32_t* __restrict__ out_k) {
  const int lane = threadIdx.x;
  StateT s;
  s.x = ini_x;
  s.cash = ini_r;
  s.preq = 0;
  xr_state<FAM_CASH>(P, s, false);
  const int nA = n_actions<FAM_CASH>(P, s);
  const bool maxdir = P.maxdir != 0;
  double best = maxdir ? -1.7976931348623157e308 : 1.7976931348623157e308;
  int bestk = 0;
  for (int k = lane; k < nA; k += 64) {
    ActionCtx c;
    action_setup<FAM_CASH>(P, s, k, c);
    double acc = 0.0;
    for (int j = 0; j < P.n_demand; ++j) {
      const double d = pmf_d[j], p = pmf_p[j];
      int64_t ni = 0;
      const double imm = cell<FAM_CASH>(P, s, c, d, ni);
      acc += p * imm;
      if (!P.is_last) {
        double ninv = jmax(0.0, c.base - d);
        ninv = ninv > P.max_inventory ? P.max_inventory : ninv;
        ninv = ninv < P.min_inventory ? P.min_inventory : ninv;
        const double fi = (ninv - P.next.x_lo) * P.inv_step;
        const double v = fi == floor(fi) ? v_next[ni] : 0.0;
        acc += (p * P.gamma) * v;
      }
    }
    if (maxdir ? (acc > best) : (acc < best)) {
      best = acc;
      bestk = k;
    }
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double ov = __shfl_xor(best, off, 64);
    const int ok = __shfl_xor(bestk, off, 64);
    if (maxdir ? better<true>(ov, ok, best, bestk) : better<false>(ov, ok, best, bestk)) {
      best = ov;
      bestk = ok;
    }
  }
  if (lane == 0) out_k[0] = bestk;
}

// counts[2 * rule]: valid paths of the rule (integer atomics, one per wave) -- what sim_reduce_kernel compares with n_paths
template <class RULE, int SOURCE>
__global__ __launch_bounds__(256) void xr_sim_kernel(XrLaunch L, SimStream R, const XrPeriod* __restrict__ per,
                                                     const double* __restrict__ thr, const double* __restrict__ val,
                                                     const double* __restrict__ given, RULE rule, double* __restrict__ out_sum,
                                                     double* __restrict__ out_demand, double* __restrict__ partial,
                                                     unsigned int* __restrict__ counts) {
  SimWave wv;
  if (wv.leaves(L.n_rules, L.waves_per_rule)) return;
  wv.place(L.waves_per_rule);
  const int ri = wv.ri;
  const uint32_t p = wv.p;
  const bool live = p < R.n_paths;
  double sum = 0.0;
  bool valid = false;
  if (live) {
    typename RULE::Path a;
    rule.start(L, a);
    const bool writes = out_demand != nullptr && ri == 0;
    valid = true;
    for (int t = 0; t < L.T; ++t) {
      double d;
      if constexpr (SOURCE == XR_SOURCE_GIVEN) {
        d = given[(int64_t)p * L.T + t];
      } else {
        const double u = SOURCE == XR_SOURCE_RANDOM ? sim_uniform_random(R.seed_lo, R.seed_hi, t, R.first_path + (uint64_t)p)
                                                    : sim_uniform_lhs(R.n_paths, R.half_bits, R.seed_lo, R.seed_hi, 0, t, p);
        d = sim_demand(per[t].samp, thr, val, u);
      }
      if (writes) out_demand[(int64_t)p * L.T + t] = d;
      if (valid) valid = rule.step(L, per[t], ri, t, d, a, sum);  // (an ended path still draws: the demands are every rule's)
    }
    out_sum[(int64_t)ri * R.n_paths + p] = sum;
  }
  sim_wave_finish(partial, counts, wv.gw, ri, valid, sum);
}

}  // namespace sdp
