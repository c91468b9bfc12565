// sdp_staff_batch_sim.hpp -- sdpgpu_staff_simulate (sdp_staff_sim.hpp) for EVERY instance of a STAFF batch in one rollout launch
// (sdpgpu_batch_staff_simulate, sdpgpu_staffbatch.hip): steps 4 and 5 of WorkforceTesting.main's loop body
// (WorkforceTesting.java:112-165) for the whole sweep.  Definition: DESIGN 4, "Workforce batch: fit and rollout".
//
//   * a PAIR is (instance i, rule r), pair = i * rules + r; one leaf per lane, a wave's 64 leaves belong to ONE pair (the leaves
//     of a pair are padded to whole waves), and SimWave places the wave over the n x rules pairs exactly as it places a handle's
//     wave over its rules.  Everything a period needs beyond the lane's own staff number is therefore a wave-uniform load;
//   * what the instances share -- the tree level and the period's box of staff numbers -- is the period record per[t]
//     (StaffSimPeriod with its instance fields empty), the clamp and the seed ride in the kernel argument; what an instance owns
//     comes from the records the solve already keeps on the device: costs, minStaffNum[t], table id and policy row from
//     StaffBatchInst [t][i], the table from StaffBatchTable (the pool: pT[j * n_rows + y], the layout the handle's walk reads);
//   * the period itself is staff_sim_step, the handle kernel's: no statement of it is repeated here.  The uniform's counters
//     carry neither the rule nor the instance: all instances see common random numbers, and instance i, rule r gets the bits of
//     sdpgpu_staff_simulate on a handle of instance i;
//   * the level rule reads ss[(pair * T + t) * 2 ...], the table rule the instance's row of the batch's policy arena;
//   * reduction: sim_wave_finish into partial[pair][wave], then sim_reduce_kernel / sim_dev2_kernel per pair (RolloutFrame).
//
// Global memory is written with ordinary vector stores from plain C++ only.
#pragma once
#include "sdp_staff_batch.hpp"
#include "sdp_staff_sim.hpp"

namespace sdp {

// L.n_rules = the PAIRS of the launch (instances x rules), L.c is not read.  inst: [t * n_inst + i].
template <class RULE>
__global__ __launch_bounds__(256) void staff_batch_sim_kernel(StaffSimLaunch L, int32_t n_inst, int32_t rules,
                                                              const StaffSimPeriod* __restrict__ per,
                                                              const StaffBatchInst* __restrict__ inst,
                                                              const StaffBatchTable* __restrict__ tabs, RULE rule,
                                                              double* __restrict__ out_sum, uint8_t* __restrict__ out_valid,
                                                              int32_t* __restrict__ out_demand, double* __restrict__ partial,
                                                              unsigned int* __restrict__ counts) {
  SimWave wv;
  if (wv.leaves(L.n_rules, L.waves_per_rule)) return;
  wv.place(L.waves_per_rule);
  const int pair = wv.ri;
  const int i = pair / rules;  // (wave-uniform)
  const uint32_t p = wv.p;
  double sum = 0.0;
  bool valid = false;
  if (p < L.n_leaves) {
    const int64_t leaf = (int64_t)pair * L.n_leaves + p;
    int x = L.ini_x;
    valid = true;
    int t = 0;
    for (; t < L.T; ++t) {
      StaffSimPeriod P = per[t];
      const StaffBatchInst I = inst[(int64_t)t * n_inst + i];
      const StaffBatchTable Tb = tabs[I.table];
      P.pT = Tb.pT;
      P.row_len = Tb.row_len;
      P.n_rows = Tb.n_rows;
      P.pol_off = I.pol_off;
      P.min_staff = I.min_staff;
      const StaffSimCosts C{I.K, I.v, I.salary, I.pen};
      int demand;
      if (!staff_sim_step(C, L, P, rule, pair, t, p, &x, &sum, &demand)) {
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
  sim_wave_finish(partial, counts, wv.gw, pair, valid, sum);
}

}  // namespace sdp
