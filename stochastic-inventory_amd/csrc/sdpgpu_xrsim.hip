// sdpgpu_xrsim.hip -- sdpgpu_xr_simulate: the rollouts of cash.singleItem.CashConstraintXR.main on the (x, R) state -- the policy
// table (CashSimulationXR.java:91-147) and Chao's a* levels (:153-173) -- along demand paths (kernel: sdp_xr_sim.hpp;
// definition: DESIGN 4, "(x, R) rollout"); and sdpgpu_xr_opt_levels: the a* levels themselves, RecursionG.getOptY
// (RecursionG.java:80-153), on the host.  All validation comes before the first device call; the draws are
// sdpgpu_simulate_sampled's, the host frame is RolloutFrame (sdpgpu_sim_host.hpp).
#include <map>
#include <utility>

#include "sdpgpu_sim_host.hpp"
#include "sdp_xr_sim.hpp"

using namespace sdpgpu_detail;

namespace {

constexpr int32_t kXrMaxRules = 16;

template <class RULE>
hipError_t launch_xr(int source, dim3 grid, hipStream_t st, const sdp::XrLaunch& L, const sdp::SimStream& R, const sdp::XrPeriod* d_per,
                     const double* d_thr, const double* d_val, const double* d_given, const RULE& rule, double* d_sum, double* d_dem,
                     double* d_part, unsigned int* d_cnt) {
  if (source == sdp::XR_SOURCE_GIVEN)
    hipLaunchKernelGGL((sdp::xr_sim_kernel<RULE, sdp::XR_SOURCE_GIVEN>), grid, dim3(256), 0, st, L, R, d_per, d_thr, d_val, d_given, rule,
                       d_sum, d_dem, d_part, d_cnt);
  else if (source == sdp::XR_SOURCE_RANDOM)
    hipLaunchKernelGGL((sdp::xr_sim_kernel<RULE, sdp::XR_SOURCE_RANDOM>), grid, dim3(256), 0, st, L, R, d_per, d_thr, d_val, d_given, rule,
                       d_sum, d_dem, d_part, d_cnt);
  else
    hipLaunchKernelGGL((sdp::xr_sim_kernel<RULE, sdp::XR_SOURCE_LHS>), grid, dim3(256), 0, st, L, R, d_per, d_thr, d_val, d_given, rule,
                       d_sum, d_dem, d_part, d_cnt);
  return hipGetLastError();
}

// RecursionG: G and getAStar call each other (RecursionG.java:96-153); the memo of G is keyed by (period, y as a double), that
// of getAStar by the period
struct RecursionG {
  int T;
  const int64_t* off;
  const double* dem;
  const double* prob;
  double price, vari_cost, deposit_rate, salvage;
  int32_t max_y;
  std::map<std::pair<int, double>, double> g_memo;
  std::map<int, double> a_memo;

  double G(int n, double y) {
    const std::pair<int, double> key(n, y);
    const auto it = g_memo.find(key);
    if (it != g_memo.end()) return it->second;
    const int64_t lo = off[n - 1], hi = off[n];
    double expectValue = 0;
    if (n == T) {
      for (int64_t j = lo; j < hi; ++j) {  // :105-107
        const double a = (price - vari_cost) * std::fmin(dem[j], y);
        const double b = deposit_rate * vari_cost * y;
        const double c = (salvage - vari_cost) * std::fmax(y - dem[j], 0.0);
        const double thisDValue = a - b + c;
        const double term = prob[j] * thisDValue;
        expectValue += term;
      }
    } else {
      const double nextAStar = a_star(n + 1);
      for (int64_t j = lo; j < hi; ++j) {  // :115-118
        const double ny = std::fmax(nextAStar, std::fmax(y - dem[j], 0.0));
        const double pw = std::pow(1 + deposit_rate, (double)(T - n));
        const double a = (price - vari_cost) * std::fmin(dem[j], y);
        const double b = deposit_rate * vari_cost * y;
        const double inner = a - b;
        const double left = pw * inner;
        const double g = G(n + 1, ny);
        const double thisDValue = left + g;
        const double term = prob[j] * thisDValue;
        expectValue += term;
      }
    }
    g_memo.emplace(key, expectValue);
    return expectValue;
  }

  double a_star(int n) {
    const auto it = a_memo.find(n);
    if (it != a_memo.end()) return it->second;
    double optY = 0;
    double optYValue = -1000;
    for (double y = 0; y < max_y; y = y + 1) {  // :139-150
      const double thisYValue = G(n, y);
      if (thisYValue - optYValue > 0.01) {
        optYValue = thisYValue;
        optY = y;
      }
    }
    a_memo.emplace(n, optY);
    return optY;
  }
};

}  // namespace

extern "C" {

int sdpgpu_xr_opt_levels(int32_t T, const int64_t* tile_off, const double* tile_demand, const double* tile_prob, double price,
                         double vari_cost, double deposit_rate, double salvage, int32_t max_y, double* out_levels) {
  g_create_error.clear();
  return guarded((sdpgpu_batch*)nullptr, "sdpgpu_xr_opt_levels", [&]() -> int {
    const char* who = "sdpgpu_xr_opt_levels";
    if (T < 1) return bfail(nullptr, SDPGPU_ERR_ARG, "%s: T = %d", who, T);
    if (!tile_off || !tile_demand || !tile_prob || !out_levels)
      return bfail(nullptr, SDPGPU_ERR_ARG, "%s: null argument (tile_off, tile_demand, tile_prob, out_levels)", who);
    if (max_y < 1) return bfail(nullptr, SDPGPU_ERR_ARG, "%s: max_y = %d (the scan is y = 0; y < max_y; y += 1: at least 1)", who, max_y);
    if (tile_off[0] != 0) return bfail(nullptr, SDPGPU_ERR_ARG, "%s: tile_off[0] = %lld (the tiles start at element 0)", who, (long long)tile_off[0]);
    for (int t = 0; t < T; ++t)
      if (tile_off[t + 1] <= tile_off[t])
        return bfail(nullptr, SDPGPU_ERR_ARG, "%s: tile_off[%d] = %lld is not above tile_off[%d] = %lld (a period's tile has at least one point)", who,
                     t + 1, (long long)tile_off[t + 1], t, (long long)tile_off[t]);
    for (int64_t j = 0; j < tile_off[T]; ++j) {
      if (!std::isfinite(tile_demand[j])) return bfail(nullptr, SDPGPU_ERR_ARG, "%s: tile_demand[%lld] = %g is not finite", who, (long long)j, tile_demand[j]);
      if (!std::isfinite(tile_prob[j])) return bfail(nullptr, SDPGPU_ERR_ARG, "%s: tile_prob[%lld] = %g is not finite", who, (long long)j, tile_prob[j]);
    }
    const double sc[4] = {price, vari_cost, deposit_rate, salvage};
    const char* names[4] = {"price", "vari_cost", "deposit_rate", "salvage"};
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(sc[k])) return bfail(nullptr, SDPGPU_ERR_ARG, "%s: %s = %g is not finite", who, names[k], sc[k]);
    RecursionG rec{T, tile_off, tile_demand, tile_prob, price, vari_cost, deposit_rate, salvage, max_y, {}, {}};
    for (int t = T - 1; t >= 0; --t) out_levels[t] = rec.a_star(t + 1);  // getOptY, :83-86
    return SDPGPU_OK;
  });
}

int sdpgpu_xr_simulate(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path, const double* demand,
                       const double* discount, double ini_x, double ini_r, int32_t n_rules, const double* levels, double vari_cost,
                       sdpgpu_sim_result* results, double* out_sum, double* out_demand) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_xr_simulate", [&]() -> int {
    const char* who = "sdpgpu_xr_simulate";
    const sdpgpu_desc& d = h->d;
    if (h->custom) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: a user functor's lambdas live on the host; roll the rule forward there", who);
    if (d.family != SDPGPU_FAMILY_CASH || d.cash_formula != 2)
      return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: handle of family %d, cash_formula %d -- the (x, R) rollouts need a CASH handle with cash_formula 2 "
                  "(CashConstraintXR)", who, d.family, d.cash_formula);
    if (d.world_size != 1) return fail(h, SDPGPU_ERR_STATE, "%s needs one GPU (world_size 1), this handle is rank %d of %d", who, d.rank, d.world_size);
    if (!results) return fail(h, SDPGPU_ERR_ARG, "%s: results is null", who);
    if (n_rules < 1 || n_rules > kXrMaxRules) return fail(h, SDPGPU_ERR_ARG, "%s: n_rules = %d (1 .. %d)", who, n_rules, kXrMaxRules);
    if (!levels && n_rules != 1) return fail(h, SDPGPU_ERR_ARG, "%s: n_rules = %d with levels null -- the table rule is one rule", who, n_rules);
    const int T = h->T;
    int rc = SDPGPU_OK;
    if (levels && (rc = check_finite(h, who, "levels", levels, (size_t)n_rules * T, {(size_t)T}))) return rc;
    if (!std::isfinite(ini_x)) return fail(h, SDPGPU_ERR_ARG, "%s: ini_x = %g is not finite", who, ini_x);
    if (!std::isfinite(ini_r)) return fail(h, SDPGPU_ERR_ARG, "%s: ini_r = %g is not finite", who, ini_r);
    if (!std::isfinite(vari_cost) || vari_cost <= 0)
      return fail(h, SDPGPU_ERR_ARG, "%s: vari_cost = %g (finite, above 0: the level is R / vari_cost)", who, vari_cost);
    if (discount && (rc = check_finite(h, who, "discount", discount, (size_t)T))) return rc;
    if (demand) {  // GIVEN: seed, mode and first_path are not read
      rc = check_n_paths(h, who, n_paths);
      if (!rc) rc = check_finite(h, who, "demand", demand, (size_t)n_paths * T, {(size_t)T});
    } else {
      rc = check_stream_args(h, who, n_paths, mode, first_path);
    }
    if (!rc && !levels) rc = check_solved(h, who, "the table rule (levels null): ");
    if (rc) return rc;
    const int source = demand ? sdp::XR_SOURCE_GIVEN : mode == SDPGPU_SAMPLE_RANDOM ? sdp::XR_SOURCE_RANDOM : sdp::XR_SOURCE_LHS;
    HostSamplers samp;
    samp.rec.resize((size_t)T);
    if (!demand) build_samplers(h, &samp);
    const std::vector<double> disc = discounts_or_ones(discount, T);
    int64_t nx = 0;  // NX of the level rule's parameter blocks
    rc = descriptor_nx(h, who, &nx);
    if (rc) return rc;

    rc = no_device(h, who);
    if (rc) return rc;
    DeviceScope dev;
    HIP_TRY(h, dev.enter(h->device));
    sdp::XrTableRule table{};
    if (!levels) {  // the start's index, or its action from sdpgpu_eval_states2, as sdpgpu_simulate
      rc = flush_api(h);
      if (rc) return rc;
      double preq = 0.0, preq2 = 0.0;
      table.idx0 = sdpgpu_state_index2(h, 1, ini_x, ini_r, preq, preq2);
      const double qx = (ini_x - h->per[0].g.x_lo) / d.step;
      const bool x_on_grid = qx >= 0.0 && qx < (double)h->per[0].g.nx && qx == std::floor(qx);
      if (table.idx0 < 0 && x_on_grid) {
        double v;
        rc = sdpgpu_eval_states2(h, 1, 1, &ini_x, &ini_r, &preq, &preq2, &v, &table.first_k);
        if (rc) return rc;
      } else if (table.idx0 < 0) {  // successors off the grid: xr_first_action_kernel values them as the oracle does
        if (T > 1 && !h->period_done[1]) return fail(h, SDPGPU_ERR_STATE, "%s: V_2 has not been computed", who);
        rc = sim_scratch(h, 16);
        if (rc) return rc;
        const PeriodInfo& p0 = h->per[0];
        const double* v_next = T > 1 ? h->d_values + h->per[1].v_off : nullptr;
        const double* pd = h->d_pmf + p0.pmf_off;
        int32_t* d_k = reinterpret_cast<int32_t*>(h->d_sim_scratch);
        hipLaunchKernelGGL(sdp::xr_first_action_kernel, dim3(1), dim3(64), 0, h->stream, make_params(h, 1), v_next, pd, pd + p0.nD, ini_x,
                           ini_r, d_k);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(&table.first_k, d_k, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
      }
      table.pol = h->d_policy;
    }
    std::vector<sdp::XrPeriod> per((size_t)T);
    for (int t = 0; t < T; ++t) {
      sdp::XrPeriod& Q = per[(size_t)t];
      if (levels) {
        Q.S.P = rule_params(h, t, nx);
        Q.S.pol_off = 0;
        Q.S.n_states = 0;
      } else {
        Q.S.P = make_params(h, t + 1);
        Q.S.pol_off = (int64_t)h->per[t].pol_off - h->per[t].lo;
        Q.S.n_states = h->per[t].S;
      }
      Q.samp = samp.rec[(size_t)t];
      Q.disc = disc[(size_t)t];
    }
    RolloutFrame<sdpgpu_handle> f(h, (uint32_t)n_paths, (size_t)n_rules);
    const size_t elems = (size_t)f.n * T;
    const auto p_per = f.put(per.data(), per.size());
    const auto p_samp = f.put_samplers(samp, false);
    const auto p_lev = f.put(levels, f.nr * T), p_giv = f.put(demand, elems);
    const auto p_dem = f.take<double>(out_demand ? elems : 0);
    rc = f.begin();
    if (rc) return rc;
    sdp::XrLaunch L{};
    L.ini_x = ini_x;
    L.ini_r = ini_r;
    L.vari_cost = vari_cost;
    L.T = T;
    L.n_rules = n_rules;
    L.waves_per_rule = f.W;
    const sdp::SimStream R = make_stream(n_paths, seed, demand ? 0 : first_path);
    const dim3 grid((unsigned)((f.nr * f.W + 3) / 4));  // (at most 16 x 2^18 waves)
    rc = f.start();
    if (rc) return rc;
    if (levels)
      HIP_TRY(h, launch_xr(source, grid, h->stream, L, R, f[p_per], f[p_samp.thr], f[p_samp.val], f[p_giv], sdp::XrLevelRule{f[p_lev]}, f.d_sum,
                           f[p_dem], f.d_part, f.d_cnt));
    else
      HIP_TRY(h, launch_xr(source, grid, h->stream, L, R, f[p_per], f[p_samp.thr], f[p_samp.val], f[p_giv], table, f.d_sum, f[p_dem], f.d_part,
                           f.d_cnt));
    f.download(out_demand, f[p_dem], elems * 8);
    return f.finish(results, out_sum);  // (n_valid: every path, but for a table rule's start whose inventory is off the grid)
  });
}

}  // extern "C"
