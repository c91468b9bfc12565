// sdp_staff_sim.hpp -- rollout of a hiring rule of the STAFF family on a SAMPLED TREE (sdpgpu_staff_simulate,
// sdpgpu_staffsim.hip): what `new SimulatesS(T, dimissionRate).simulatesS(initialState, sS)` does (SimulatesS.java:33-87 with the
// latin hypercube of Sampling.java:110-124, made reproducible), for the (s, S) level rule of that class and for the handle's own
// policy table.  Definition: DESIGN 4, "Workforce rollout on a sampled tree"; tests/staff_sim_twin.py is written from it.
//
//   * the tree has K[t] children per node of depth t and N = prod K leaves; ONE LEAF PER LANE: a lane walks root to leaf and
//     recomputes the prefixes it shares with its neighbours (they are deterministic), N T period steps in all.  Leaf p passes
//     node n_t = p div stride_t (stride_t = prod_{s > t} K[s]); its child digit is j = n_t mod K[t], its parent i = n_t div K[t]
//     -- the reference's `i * K + j` order;
//   * the uniform of (t, parent i, child j) is sim_uniform_lhs of sdp_sampler.hpp with n = K[t], inst = i, p = j: every node
//     draws its own latin hypercube of K[t] strata.  The counters do not carry the rule: every rule of a call sees the same
//     uniforms;
//   * the turnover is drawn from the row the recursion integrates over, pmfs[t][min(hireTo, rows - 1)] (StaffRecursion.java:92-95):
//     thresholds c_q = p_0 + .. + p_q as a running fp64 sum, turnover = #{q < row_len - 1 : c_q <= u} -- a serial walk down the
//     transposed table, four reads a trip, that stops at the first threshold above u (the sums of non-negative terms never
//     decrease; the host refuses a table with a negative entry).  Its mean length is hireTo x rate;
//   * the period's cost and the next staff number are the statements of staff_period_kernel (sdp_staff.hpp), one fp64
//     operation each.  A leaf's whole period -- rule, hireTo, uniform, turnover, cost, clamp -- is ONE device function,
//     staff_sim_step, which the batch's kernel (sdp_staff_batch_sim.hpp) calls as well: there is no second copy of it;
//   * a RULE is a small struct that picks the period's hires (the idiom of batch_sim_kernel<RULE, SAMPLED>).  A wave's 64 leaves
//     belong to ONE rule (the leaves of a rule are padded to whole waves): the rule's levels and the period records are
//     wave-uniform loads;
//   * reduction: wave total by xor butterfly (lanes past N hold 0.0) into partial[rule][wave]; sim_reduce_kernel and
//     sim_dev2_kernel of sdp_sim_sampled.hpp then form mean and m2 of every rule in their fixed order.
//
// Global memory is written with ordinary vector stores from plain C++ only.
#pragma once
#include "sdp_sampler.hpp"

namespace sdp {

// one period of the handle, wave-uniform
struct StaffSimPeriod {
  const double* pT;        // the period's transposed table, row j = 0: pT[j * n_rows + y]
  const int32_t* row_len;  // entries of row y
  int64_t pol_off;         // the table rule: element offset of the period's policy row (indexed by x - x_lo)
  int32_t n_rows, min_staff;
  int32_t x_lo, nx;        // the period's box of staff numbers
  uint32_t K, stride;      // children per node at this depth, leaves below one child
  int32_t half_bits;       // sigma's half width for n = K
  int32_t pad;
};

// fixCost, unitVariCost, salary, unitPenalty of one instance
struct StaffSimCosts {
  double K, v, salary, pen;
};

struct StaffSimLaunch {
  StaffSimCosts c;           // the handle's costs (a batch reads every instance's own: sdp_staff_batch_sim.hpp)
  int32_t T, n_rules;
  int32_t clamp, min_x, max_x;
  int32_t ini_x;
  uint32_t n_leaves, waves_per_rule;
  uint32_t seed_lo, seed_hi;
};

// (s, S): hire up to S below s, in every period (SimulatesS.java:55).  ss[(rule * T + t) * 2 + {0, 1}], already truncated.
struct StaffLevelRule {
  const int32_t* __restrict__ ss;
  __device__ __forceinline__ bool hires(const StaffSimLaunch& L, const StaffSimPeriod&, int rule, int t, int x, int* a) const {
    const int32_t* r = ss + ((int64_t)rule * L.T + t) * 2;
    const int s = r[0], S = r[1];
    *a = x < s ? S - x : 0;
    return true;
  }
};

// the handle's policy row; a staff number outside the period's box ends the leaf (its valid flag stays clear)
struct StaffTableRule {
  const int32_t* __restrict__ policy;
  __device__ __forceinline__ bool hires(const StaffSimLaunch&, const StaffSimPeriod& P, int, int, int x, int* a) const {
    const int idx = x - P.x_lo;
    if (idx < 0 || idx >= P.nx) return false;
    *a = policy[P.pol_off + idx];
    return true;
  }
};

// turnover of level y > 0 under the uniform u
__device__ __forceinline__ int staff_sim_turnover(const StaffSimPeriod& P, int y, double u) {
  const int r = y >= P.n_rows - 1 ? P.n_rows - 1 : y;
  const int m = P.row_len[r] - 1;  // thresholds that count: the last one is +infinity
  const double* __restrict__ prow = P.pT + r;
  double c = 0.0;
  int k = 0;
  // (a trip's reads past the last threshold that counts repeat the row's last entry: they come after every counted one)
  for (int q0 = 0; q0 < m; q0 += 4) {
    double p[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = prow[(size_t)min(q0 + e, m) * (size_t)P.n_rows];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c += p[e];
      k += (q0 + e < m && c <= u) ? 1 : 0;
    }
    if (!(c <= u)) break;
  }
  return k;
}

// One period of a leaf, the ONE statement of it for the handle's kernel and the batch's (sdp_staff_batch_sim.hpp): rule -> hireTo
// -> the uniform of (t, parent, child) -> turnover -> the cost statements of staff_period_kernel, one fp64 operation each -> the
// clamp.  C: the costs of the instance the leaf belongs to; L: the tree's seed, the clamp; P: the period's table, box, minStaffNum
// and tree level.  false: the rule ended the leaf (nothing is changed).
template <class RULE>
__device__ __forceinline__ bool staff_sim_step(const StaffSimCosts& C, const StaffSimLaunch& L, const StaffSimPeriod& P, const RULE& rule,
                                               int ri, int t, uint32_t p, int* x_io, double* sum_io, int* demand_out) {
  const int x = *x_io;
  int a;
  if (!rule.hires(L, P, ri, t, x, &a)) return false;
  const int hireTo = x + a;
  int demand = 0;
  if (hireTo > 0) {  // (SimulatesS.java:64-67: nobody to leave)
    const uint32_t node = p / P.stride;
    const uint32_t parent = node / P.K, child = node - parent * P.K;
    const double u = sim_uniform_lhs(P.K, P.half_bits, L.seed_lo, L.seed_hi, (int)parent, t, child);
    demand = staff_sim_turnover(P, hireTo, u);
  }
  const double fixHire = a > 0 ? C.K : 0.0;
  const double variHire = C.v * (double)a;
  const double fv = fixHire + variHire;
  const int n = hireTo - demand;  // nextStaffNum
  const double salaryCost = C.salary * (double)n;
  const double penalty = n > P.min_staff ? 0.0 : C.pen * (double)(P.min_staff - n);
  const double imm = fv + salaryCost + penalty;
  *sum_io = t == 0 ? imm : *sum_io + imm;
  int nn = n;
  if (L.clamp) {
    nn = nn > L.max_x ? L.max_x : nn;
    nn = nn < L.min_x ? L.min_x : nn;
  }
  *x_io = nn;
  *demand_out = demand;
  return true;
}

// counts[2 * rule]: valid leaves of the rule (integer atomics, one per wave)
template <class RULE>
__global__ __launch_bounds__(256) void staff_sim_kernel(StaffSimLaunch L, const StaffSimPeriod* __restrict__ per, RULE rule,
                                                        double* __restrict__ out_sum, uint8_t* __restrict__ out_valid,
                                                        int32_t* __restrict__ out_demand, double* __restrict__ partial,
                                                        unsigned int* __restrict__ counts) {
  SimWave wv;
  if (wv.leaves(L.n_rules, L.waves_per_rule)) return;
  wv.place(L.waves_per_rule);
  const int ri = wv.ri;
  const uint32_t p = wv.p;
  double sum = 0.0;
  bool valid = false;
  if (p < L.n_leaves) {
    const int64_t leaf = (int64_t)ri * L.n_leaves + p;
    int x = L.ini_x;
    valid = true;
    int t = 0;
    for (; t < L.T; ++t) {
      const StaffSimPeriod P = per[t];
      int demand;
      if (!staff_sim_step(L.c, L, P, rule, ri, t, p, &x, &sum, &demand)) {
        valid = false;
        break;
      }
      if (out_demand) out_demand[leaf * L.T + t] = demand;
    }
    if (out_demand)
      for (; t < L.T; ++t) out_demand[leaf * L.T + t] = -1;  // (periods an ended leaf never reached)
    out_sum[leaf] = sum;
    if (out_valid) out_valid[leaf] = valid ? 1 : 0;
  }
  sim_wave_finish(partial, counts, wv.gw, ri, valid, sum);
}

}  // namespace sdp
