// sdpgpu_cashrulesim.hip -- sdpgpu_cash_rule_simulate: the cash drivers' rollouts of an (s, C, S) ordering rule along sampled
// demand paths (CashSimulation.java:996-1134; kernel: sdp_cash_rule_sim.hpp; definition: DESIGN 4, "Cash rule rollout").  All
// validation comes before the first device call; the draws are sdpgpu_simulate_sampled's, the host frame is RolloutFrame
// (sdpgpu_sim_host.hpp).
#include "sdpgpu_sim_host.hpp"
#include "sdp_cash_rule_sim.hpp"

using namespace sdpgpu_detail;

namespace {

constexpr int32_t kCashRuleMaxRules = 16;

}  // namespace

extern "C" {

int sdpgpu_cash_rule_simulate(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path, const double* discount,
                              double ini_x, double ini_cash, int32_t n_rules, const int32_t* form, const double* rule, const double* c1_tab,
                              const double* c2_tab, double min_cash_required, double max_q, double fix_order_cost, double vari_cost,
                              sdpgpu_sim_result* results, double* out_sum) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_cash_rule_simulate", [&]() -> int {
    const char* who = "sdpgpu_cash_rule_simulate";
    const sdpgpu_desc& d = h->d;
    if (h->custom) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: a user functor's lambdas live on the host; roll the rule forward there", who);
    if (d.family != SDPGPU_FAMILY_CASH)
      return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: handle of family %d -- the (s, C, S) rules order from the cash on hand of a CASH handle", who, d.family);
    if (d.cash_formula == 2)
      return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: cash_formula 2 -- not built for the (x, R) state of CashConstraintXR", who);
    if (d.world_size != 1) return fail(h, SDPGPU_ERR_STATE, "%s needs one GPU (world_size 1), this handle is rank %d of %d", who, d.rank, d.world_size);
    if (!form) return fail(h, SDPGPU_ERR_ARG, "%s: form is null", who);
    if (!rule) return fail(h, SDPGPU_ERR_ARG, "%s: rule is null", who);
    if (!results) return fail(h, SDPGPU_ERR_ARG, "%s: results is null", who);
    if (n_rules < 1 || n_rules > kCashRuleMaxRules) return fail(h, SDPGPU_ERR_ARG, "%s: n_rules = %d (1 .. %d)", who, n_rules, kCashRuleMaxRules);
    const int T = h->T;
    const size_t nr = (size_t)n_rules;
    for (int r = 0; r < n_rules; ++r)
      if (form[r] < SDPGPU_RULE_SC12S || form[r] > SDPGPU_RULE_SMEANCS)
        return fail(h, SDPGPU_ERR_ARG, "%s: form[%d] = %d (SDPGPU_RULE_SC12S 0, SDPGPU_RULE_SC1S 1, SDPGPU_RULE_SMEANCS 2)", who, r, form[r]);
    int rc = check_finite(h, who, "rule", rule, nr * T * 4, {(size_t)T, 4});
    if (rc) return rc;
    if (!std::isfinite(ini_x)) return fail(h, SDPGPU_ERR_ARG, "%s: ini_x = %g is not finite", who, ini_x);
    if (!std::isfinite(ini_cash)) return fail(h, SDPGPU_ERR_ARG, "%s: ini_cash = %g is not finite", who, ini_cash);
    if (!std::isfinite(min_cash_required)) return fail(h, SDPGPU_ERR_ARG, "%s: min_cash_required = %g is not finite", who, min_cash_required);
    if (!std::isfinite(fix_order_cost)) return fail(h, SDPGPU_ERR_ARG, "%s: fix_order_cost = %g is not finite", who, fix_order_cost);
    if (!std::isfinite(max_q) || max_q < 0) return fail(h, SDPGPU_ERR_ARG, "%s: max_q = %g (finite, at least 0)", who, max_q);
    if (!std::isfinite(vari_cost) || vari_cost <= 0) return fail(h, SDPGPU_ERR_ARG, "%s: vari_cost = %g (finite, above 0: the order is cash / vari_cost)", who, vari_cost);
    int64_t nx = 0;  // NX of the tables
    rc = descriptor_nx(h, who, &nx);
    if (rc) return rc;
    const size_t tab_elems = nr * T * (size_t)nx;
    const double* tabs[2] = {c1_tab, c2_tab};
    for (int w = 0; w < 2; ++w) {
      if (!tabs[w]) continue;
      for (size_t e = 0; e < tab_elems; ++e)
        if (std::isinf(tabs[w][e]))
          return fail(h, SDPGPU_ERR_ARG, "%s: c%d_tab[%zu][%zu][%zu] is infinite (a finite threshold, or NaN for an absent key)", who, w + 1,
                      e / ((size_t)T * nx), e / (size_t)nx % (size_t)T, e % (size_t)nx);
    }
    rc = check_stream_args(h, who, n_paths, mode, first_path);
    if (rc) return rc;
    HostSamplers samp;
    build_samplers(h, &samp);
    const std::vector<double> disc = discounts_or_ones(discount, T);
    std::vector<sdp::CashRulePeriod> per((size_t)T);
    for (int t = 0; t < T; ++t) {
      per[(size_t)t].P = rule_params(h, t, nx);
      per[(size_t)t].samp = samp.rec[(size_t)t];
      per[(size_t)t].disc = disc[(size_t)t];
      per[(size_t)t].min_cash_required = min_cash_required;
      per[(size_t)t].max_q = max_q;
      per[(size_t)t].fix_order_cost = fix_order_cost;
      per[(size_t)t].vari_cost = vari_cost;
    }

    rc = no_device(h, who);
    if (rc) return rc;
    DeviceScope dev;
    HIP_TRY(h, dev.enter(h->device));
    RolloutFrame<sdpgpu_handle> f(h, (uint32_t)n_paths, nr);
    const auto p_per = f.put(per.data(), per.size());
    const auto p_samp = f.put_samplers(samp, false);
    const auto p_form = f.put(form, nr);
    const auto p_rule = f.put(rule, nr * T * 4), p_c1 = f.put(c1_tab, tab_elems), p_c2 = f.put(c2_tab, tab_elems);
    rc = f.begin();
    if (rc) return rc;
    sdp::CashRuleLaunch L{};
    L.ini_x = ini_x;
    L.ini_cash = ini_cash;
    L.T = T;
    L.n_rules = n_rules;
    L.waves_per_rule = f.W;
    const sdp::SimStream R = make_stream(n_paths, seed, first_path);
    const dim3 grid((unsigned)((nr * f.W + 3) / 4));  // (at most 16 x 2^18 waves)
    rc = f.start();
    if (rc) return rc;
    if (mode == SDPGPU_SAMPLE_RANDOM)
      hipLaunchKernelGGL((sdp::cash_rule_sim_kernel<true>), grid, dim3(256), 0, h->stream, L, R, f[p_per], f[p_samp.thr], f[p_samp.val], f[p_form],
                         f[p_rule], f[p_c1], f[p_c2], f.d_sum, f.d_part, f.d_cnt);
    else
      hipLaunchKernelGGL((sdp::cash_rule_sim_kernel<false>), grid, dim3(256), 0, h->stream, L, R, f[p_per], f[p_samp.thr], f[p_samp.val], f[p_form],
                         f[p_rule], f[p_c1], f[p_c2], f.d_sum, f.d_part, f.d_cnt);
    HIP_TRY(h, hipGetLastError());
    return f.finish(results, out_sum);  // (n_valid: every path of a rule -- no path ever becomes invalid)
  });
}

}  // extern "C"
