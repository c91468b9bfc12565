// sdpgpu_staffsim.hip -- sdpgpu_staff_simulate: the workforce drivers' rollout of a hiring rule on a sampled tree
// (SimulatesS.java:33-87), for the (s, S) level rule and for the handle's policy table (kernel: sdp_staff_sim.hpp; definition:
// DESIGN 4, "Workforce rollout on a sampled tree").  All validation comes before the first device call; the host frame is
// RolloutFrame (sdpgpu_sim_host.hpp).
#include "sdpgpu_sim_host.hpp"
#include "sdp_staff_sim.hpp"

using namespace sdpgpu_detail;

namespace {

constexpr int32_t kStaffSimMaxRules = 64;

// the walk down a row stops at the first threshold above u: right only when the running sums never decrease
int check_tables(sdpgpu_handle* h, const char* who) {
  for (int t = 0; t < h->T; ++t) {
    const std::vector<double>& p = h->lvl_p[(size_t)t];
    if (t > 0 && p == h->lvl_p[(size_t)t - 1]) continue;
    for (size_t k = 0; k < p.size(); ++k)
      if (!(p[k] >= 0.0))
        return fail(h, SDPGPU_ERR_ARG, "%s: level pmf of period %d holds a negative or NaN probability (level %zu, turnover %zu)", who, t + 1,
                    k % (size_t)h->lvl_rows[(size_t)t], k / (size_t)h->lvl_rows[(size_t)t]);
  }
  return SDPGPU_OK;
}

}  // namespace

extern "C" {

int sdpgpu_staff_simulate(sdpgpu_handle* h, const int32_t* sample_nums, uint64_t seed, double ini_x, const double* ss, int32_t n_rules,
                          sdpgpu_sim_result* results, double* out_sum, uint8_t* out_valid, int32_t* out_demand) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_staff_simulate", [&]() -> int {
    const char* who = "sdpgpu_staff_simulate";
    if (h->d.family != SDPGPU_FAMILY_STAFF)
      return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: only a STAFF handle has a level-dependent pmf to draw from (the other families: sdpgpu_simulate_sampled)", who);
    if (h->d.world_size != 1) return fail(h, SDPGPU_ERR_STATE, "%s needs the whole tables on one GPU (world_size 1)", who);
    if (!sample_nums) return fail(h, SDPGPU_ERR_ARG, "%s: sample_nums is null", who);
    if (!results) return fail(h, SDPGPU_ERR_ARG, "%s: results is null", who);
    if (n_rules < 1 || n_rules > kStaffSimMaxRules) return fail(h, SDPGPU_ERR_ARG, "%s: n_rules = %d (1 .. %d)", who, n_rules, kStaffSimMaxRules);
    if (!ss && n_rules != 1) return fail(h, SDPGPU_ERR_ARG, "%s: n_rules = %d with ss == NULL (the table policy is one rule)", who, n_rules);
    const int T = h->T;
    int64_t N = 1;
    for (int t = 0; t < T; ++t) {
      if (sample_nums[t] < 1) return fail(h, SDPGPU_ERR_ARG, "%s: sample_nums[%d] = %d (at least 1)", who, t, sample_nums[t]);
      N *= sample_nums[t];
      if (N > kSimMaxPaths) return fail(h, SDPGPU_ERR_ARG, "%s: sample_nums gives more than %d leaves (product up to index %d)", who, kSimMaxPaths, t);
    }
    for (int t = 0; t < T; ++t)
      if (!h->pmf_set[(size_t)t]) return fail(h, SDPGPU_ERR_STATE, "%s: level pmf of period %d not set (sdpgpu_set_level_pmf)", who, t + 1);
    if (!(ini_x >= 0 && ini_x <= 1e9) || ini_x != std::floor(ini_x))
      return fail(h, SDPGPU_ERR_ARG, "%s: ini_x = %g (a staff number: an integer in 0 .. 1e9)", who, ini_x);
    std::vector<int32_t> levels;
    if (ss) {
      levels.resize((size_t)n_rules * T * 2);
      for (int r = 0; r < n_rules; ++r)
        for (int t = 0; t < T; ++t) {
          const double s = ss[((size_t)r * T + t) * 2], S = ss[((size_t)r * T + t) * 2 + 1];
          // (int) of a double: toward zero; what it cannot represent is refused
          if (!std::isfinite(s) || !std::isfinite(S) || !(s > -2147483649.0 && s < 2147483648.0) || !(S > -2147483649.0 && S < 2147483648.0))
            return fail(h, SDPGPU_ERR_ARG, "%s: ss[%d][%d] = (%g, %g) is not finite or outside int32", who, r, t, s, S);
          const int32_t si = (int32_t)s, Si = (int32_t)S;
          if ((int64_t)Si < (int64_t)si - 1)
            return fail(h, SDPGPU_ERR_ARG, "%s: ss[%d][%d] = (%g, %g): S < s - 1 would hire a negative number at x = s - 1", who, r, t, s, S);
          levels[((size_t)r * T + t) * 2] = si;
          levels[((size_t)r * T + t) * 2 + 1] = Si;
        }
    }
    int rc = layout(h);  // host arithmetic: the periods' boxes
    if (rc) return rc;
    if (!ss) {
      const double lo = h->per[0].g.x_lo, hi = lo + (double)(h->per[0].g.nx - 1);
      if (ini_x < lo || ini_x > hi) return fail(h, SDPGPU_ERR_ARG, "%s: ini_x = %g outside period 1's staff numbers %g .. %g", who, ini_x, lo, hi);
      rc = check_solved(h, who, "", " (the table policy needs sdpgpu_solve; a level rule does not)");
      if (rc) return rc;
    }
    if (!(h->allocated && h->staff_tables_nonneg)) {  // (looked at once: the tables are frozen once the device copies exist)
      rc = check_tables(h, who);
      if (rc) return rc;
    }

    rc = no_device(h, who);
    if (rc) return rc;
    DeviceScope dev;
    HIP_TRY(h, dev.enter(h->device));
    rc = allocate(h);  // (a level rule needs the device tables, not a solve)
    if (rc) return rc;
    h->staff_tables_nonneg = true;
    rc = flush_api(h);
    if (rc) return rc;
    const uint32_t n = (uint32_t)N;
    std::vector<sdp::StaffSimPeriod> per((size_t)T);
    uint32_t stride = n;
    for (int t = 0; t < T; ++t) {
      sdp::StaffSimPeriod& q = per[(size_t)t];
      stride /= (uint32_t)sample_nums[t];
      q.pT = h->d_lvl_p[(size_t)t];
      q.row_len = h->d_lvl_len[(size_t)t];
      q.pol_off = (int64_t)h->per[t].pol_off - h->per[t].lo;
      q.n_rows = h->lvl_rows[(size_t)t];
      q.min_staff = (int32_t)h->per[t].overhead;
      q.x_lo = (int32_t)h->per[t].g.x_lo;
      q.nx = (int32_t)h->per[t].g.nx;
      q.K = (uint32_t)sample_nums[t];
      q.stride = stride;
      q.half_bits = make_stream(sample_nums[t], 0, 0).half_bits;
      q.pad = 0;
    }
    sdp::StaffSimLaunch L{};
    L.c = sdp::StaffSimCosts{h->d.fixed_order_cost, h->d.unit_order_cost, h->d.holding_cost, h->d.penalty_cost};
    L.T = T;
    L.n_rules = n_rules;
    L.clamp = h->d.clamp_inventory;
    L.min_x = (int32_t)h->d.min_inventory;
    L.max_x = (int32_t)h->d.max_inventory;
    L.ini_x = (int32_t)ini_x;
    L.n_leaves = n;
    L.seed_lo = (uint32_t)(seed & 0xffffffffu);
    L.seed_hi = (uint32_t)(seed >> 32);

    RolloutFrame<sdpgpu_handle> f(h, n, (size_t)n_rules);
    const size_t leaves = f.nr * n;
    const auto p_per = f.put(per.data(), per.size());
    const auto p_ss = f.put(levels.data(), levels.size());
    const auto p_flag = f.take<uint8_t>(out_valid ? leaves : 0);
    const auto p_dem = f.take<int32_t>(out_demand ? leaves * (size_t)T : 0);
    rc = f.begin();
    if (rc) return rc;
    L.waves_per_rule = f.W;
    const dim3 grid((unsigned)((f.nr * f.W + 3) / 4));  // (at most 64 x 2^18 waves)
    rc = f.start();
    if (rc) return rc;
    if (ss)
      hipLaunchKernelGGL((sdp::staff_sim_kernel<sdp::StaffLevelRule>), grid, dim3(256), 0, h->stream, L, f[p_per], sdp::StaffLevelRule{f[p_ss]},
                         f.d_sum, f[p_flag], f[p_dem], f.d_part, f.d_cnt);
    else
      hipLaunchKernelGGL((sdp::staff_sim_kernel<sdp::StaffTableRule>), grid, dim3(256), 0, h->stream, L, f[p_per], sdp::StaffTableRule{h->d_policy},
                         f.d_sum, f[p_flag], f[p_dem], f.d_part, f.d_cnt);
    HIP_TRY(h, hipGetLastError());
    f.download(out_valid, f[p_flag], leaves);
    f.download(out_demand, f[p_dem], leaves * (size_t)T * sizeof(int32_t));
    return f.finish(results, out_sum);
  });
}

}  // extern "C"
