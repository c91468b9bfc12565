// sdp_cash_rule_sim.hpp -- rollout of (s, C, S) ordering rules of the CASH family along sampled demand paths
// (sdpgpu_cash_rule_simulate, sdpgpu_cashrulesim.hip): what CashSimulation.simulatesCS with (s, C1(x), C2(x), S)
// (CashSimulation.java:996-1042), simulatesCS with (s, C1(x), S) (:1050-1093) and simulatesMeanCS (:1101-1134) do after a solve
// -- the four calls of CashConstraintTesting.main (CashConstraintTesting.java:187, 201, 216, 241) as ONE launch.  Definition:
// DESIGN 4, "Cash rule rollout"; tests/cash_rule_twin.py is written from it.
//
//   * one (rule, path) per lane; the rule index is a dimension of the launch: a wave's 64 paths belong to ONE rule (the paths
//     of a rule are padded to whole waves), so the rule's form and its row of the period are wave-uniform loads;
//   * the STATE IS TWO DOUBLES (x, cash), not a grid index: the rule orders (cash - minCashRequired - K) / v units, which is
//     no multiple of the step -- the inventory leaves the grid and stays a double; the cash is the double the family's
//     quantiser yields (the key of cash_index, decoded as decode_state decodes it);
//   * the demand of (t, path) is drawn as sim_sampled_kernel draws it (sdp_sampler.hpp, instance position 0): every rule of a
//     call sees the demands sdpgpu_sample_demands returns.  The counters do not carry the rule;
//   * the period block, the sampler record and the discount weight of a period are ONE wave-uniform record (CashRulePeriod), and
//     the tables' grid is read from that block: fewer values live in scalar registers beside the sampler's round keys;
//   * the period's cash increment is cell<FAM_CASH> of sdp_device.hpp on the context action_setup_q fills from the double q:
//     the family's statements exist once;
//   * the thresholds C1(x), C2(x) are dense tables over the descriptor's inventory grid, NaN = key absent; a lookup hits only
//     where x IS a grid value (TreeMap.get(new State(period, x)) compares doubles exactly);
//   * reduction: wave total by xor butterfly (lanes past n_paths hold 0.0) into partial[rule][wave]; sim_reduce_kernel and
//     sim_dev2_kernel of sdp_sim_sampled.hpp then form mean and m2 of every rule in their fixed order.
//
// Global memory is written with ordinary vector stores from plain C++ only; no floating-point atomics.
#pragma once
#include "sdp_device.hpp"
#include "sdp_sampler.hpp"

namespace sdp {

constexpr int RULE_SC12S = 0;    // (s, C1(x), C2(x), S)
constexpr int RULE_SC1S = 1;     // (s, C1(x), S)
constexpr int RULE_SMEANCS = 2;  // (s, C, S), C the row's own value

struct CashRuleLaunch {
  double ini_x, ini_cash;
  int32_t T, n_rules;
  uint32_t waves_per_rule;
  int32_t pad;
};

// one period of the handle, wave-uniform: the family's parameter block (its `cur` box is the descriptor's inventory grid -- key
// of table entry ix = cur.x_lo + ix * step, cur.nx = NX of the tables), the period's sampler record and discount weight
struct CashRulePeriod {
  DevParams P;
  SimSampler samp;
  double disc;
  double min_cash_required, max_q, fix_order_cost, vari_cost;  // the reference's arguments, not the descriptor's fields (the same in
                                                               // every period: read where they are used, not held in registers)
};

// entry of a dense threshold table at inventory x; `absent` where x is no grid value or the entry is NaN
__device__ __forceinline__ double cash_rule_lookup(const DevParams& P, const double* __restrict__ row, double x, double absent) {
  if (!row) return absent;
  const double fi = rint((x - P.cur.x_lo) * P.inv_step);
  if (!(fi >= 0.0 && fi < (double)P.cur.nx)) return absent;
  const int i = (int)fi;
  if (P.cur.x_lo + (double)i * P.step != x) return absent;
  const double v = row[i];
  return v != v ? absent : v;
}

// the order of rule row (s, c1, c2, S) in period index t at (x, cash)
__device__ __forceinline__ double cash_rule_order(const CashRulePeriod& Q, int form, int t, const double* __restrict__ row,
                                                  const double* __restrict__ c1_row, const double* __restrict__ c2_row, double x,
                                                  double cash) {
  const double s = row[0], S = row[3];
  // the order the cash on hand pays for (CashSimulation.java:1013, :1065, :1069, :1115)
  double m = jmax(0.0, (cash - Q.min_cash_required - Q.fix_order_cost) / Q.vari_cost);
  if (t == 0) {
    double q = x < s ? S - x : 0.0;     // :1011, :1064, :1113
    if (form == RULE_SC1S) q = jmin(q, m);  // :1065-1066
    return q;
  }
  if (form == RULE_SC12S) m = m >= 2147483647.0 ? 2147483647.0 : (double)(int)m;  // `(int)` of :1013 (m >= 0, never NaN)
  m = jmin(m, Q.max_q);
  if (!(x < s)) return 0.0;
  double c1 = row[1], c2 = row[2];
  if (form != RULE_SMEANCS) c1 = cash_rule_lookup(Q.P, c1_row, x, 0.0);      // :1016-1019, :1072-1075
  if (form == RULE_SC12S) c2 = cash_rule_lookup(Q.P, c2_row, x, 10000.0);    // :1020-1023 (M = 10000)
  const bool orders = form == RULE_SC12S ? (cash > c1 && cash < c2) : cash > c1;  // "not include equal"
  return orders ? jmin(m, S - x) : 0.0;
}

// counts[2 * rule]: paths of the rule (integer atomics, one per wave) -- what sim_reduce_kernel compares with n_paths
template <bool RANDOM>
__global__ __launch_bounds__(256) void cash_rule_sim_kernel(CashRuleLaunch L, SimStream R, const CashRulePeriod* __restrict__ per,
                                                            const double* __restrict__ thr, const double* __restrict__ val,
                                                            const int32_t* __restrict__ form, const double* __restrict__ rule,
                                                            const double* __restrict__ c1_tab, const double* __restrict__ c2_tab,
                                                            double* __restrict__ out_sum, double* __restrict__ partial,
                                                            unsigned int* __restrict__ counts) {
  SimWave wv;
  if (wv.leaves(L.n_rules, L.waves_per_rule)) return;
  wv.place(L.waves_per_rule);
  const int ri = wv.ri;
  const uint32_t p = wv.p;
  const bool live = p < R.n_paths;
  double sum = 0.0;
  if (live) {
    const int fm = form[ri];
    double x = L.ini_x, cash = L.ini_cash;
    for (int t = 0; t < L.T; ++t) {
      const DevParams& P = per[t].P;
      const int64_t rt = (int64_t)ri * L.T + t;
      const double u = RANDOM ? sim_uniform_random(R.seed_lo, R.seed_hi, t, R.first_path + (uint64_t)p)
                              : sim_uniform_lhs(R.n_paths, R.half_bits, R.seed_lo, R.seed_hi, 0, t, p);
      const double d = sim_demand(per[t].samp, thr, val, u);
      const double q = cash_rule_order(per[t], fm, t, rule + rt * 4, c1_tab ? c1_tab + rt * P.cur.nx : nullptr,
                                       c2_tab ? c2_tab + rt * P.cur.nx : nullptr, x, cash);
      StateT s;
      s.x = x;
      s.cash = cash;
      s.preq = 0;
      ActionCtx c;
      action_setup_q(P, s, q, c);
      int64_t ni = 0;
      const double imm = cell<FAM_CASH>(P, s, c, d, ni);
      sum += per[t].disc * imm;
      if (!P.is_last) {  // the transition of cell<FAM_CASH> (CashConstraint.java:124-131), kept as doubles
        double ninv = jmax(0.0, c.base - d);
        ninv = ninv > P.max_inventory ? P.max_inventory : ninv;
        ninv = ninv < P.min_inventory ? P.min_inventory : ninv;
        x = ninv;
        const double k = (double)((int64_t)cash_index(P, s.cash + imm) + P.next.k_lo);
        cash = P.cash_round_int_div ? k : k / P.round_div;
      }
    }
    out_sum[(int64_t)ri * R.n_paths + p] = sum;
  }
  sim_wave_finish(partial, counts, wv.gw, ri, live, sum);
}

}  // namespace sdp
