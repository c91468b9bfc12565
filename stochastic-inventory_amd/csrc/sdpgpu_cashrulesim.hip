// sdpgpu_cashrulesim.hip -- sdpgpu_cash_rule_simulate: the cash drivers' rollouts of an (s, C, S) ordering rule along sampled
// demand paths (CashSimulation.java:996-1134; kernel: sdp_cash_rule_sim.hpp; definition: DESIGN 4, "Cash rule rollout").  All
// validation comes before the first device call; the draws are sdpgpu_simulate_sampled's (check_stream_args, build_samplers and
// make_stream of sdpgpu_sim_host.hpp), the device scratch is carved from the handle's simulation block, the reduction is the
// handle's (launch_sim_moments of sdpgpu_simsample.hip: sim_reduce_kernel, sim_dev2_kernel).
#include "sdpgpu_sim_host.hpp"
#include "sdp_cash_rule_sim.hpp"

using namespace sdpgpu_detail;

namespace {

constexpr int32_t kCashRuleMaxRules = 16;

}  // namespace

namespace sdpgpu_detail {

// the period's parameter block without a layout (the rollout reads no table, so it needs no pmf tile where a spec is set): the
// family's scalars and the handle's overhead from make_params, the boxes from the descriptor as layout() forms them (shared with
// the level rule of sdpgpu_xr_simulate, sdpgpu_xrsim.hip)
DevParams rule_params(const sdpgpu_handle* h, int t, int64_t nx) {
  const sdpgpu_desc& d = h->d;
  DevParams P = make_params(h, t + 1);
  P.overhead = h->per[(size_t)t].overhead_set ? h->per[(size_t)t].overhead : d.overhead_cost;
  Grid g{};
  g.x_lo = d.min_inventory;
  g.nx = nx;
  g.k_lo = cash_key_of_bound(d, d.min_cash);
  g.nc = cash_key_of_bound(d, d.max_cash) - g.k_lo + 1;
  g.nq = g.nq1 = 1;
  P.cur = P.next = g;
  P.counts = nullptr;
  return P;
}

}  // namespace sdpgpu_detail

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
    for (int r = 0; r < n_rules; ++r)
      if (form[r] < SDPGPU_RULE_SC12S || form[r] > SDPGPU_RULE_SMEANCS)
        return fail(h, SDPGPU_ERR_ARG, "%s: form[%d] = %d (SDPGPU_RULE_SC12S 0, SDPGPU_RULE_SC1S 1, SDPGPU_RULE_SMEANCS 2)", who, r, form[r]);
    for (int r = 0; r < n_rules; ++r)
      for (int t = 0; t < T; ++t)
        for (int k = 0; k < 4; ++k) {
          const double v = rule[((size_t)r * T + t) * 4 + k];
          if (!std::isfinite(v)) return fail(h, SDPGPU_ERR_ARG, "%s: rule[%d][%d][%d] = %g is not finite", who, r, t, k, v);
        }
    if (!std::isfinite(ini_x)) return fail(h, SDPGPU_ERR_ARG, "%s: ini_x = %g is not finite", who, ini_x);
    if (!std::isfinite(ini_cash)) return fail(h, SDPGPU_ERR_ARG, "%s: ini_cash = %g is not finite", who, ini_cash);
    if (!std::isfinite(min_cash_required)) return fail(h, SDPGPU_ERR_ARG, "%s: min_cash_required = %g is not finite", who, min_cash_required);
    if (!std::isfinite(fix_order_cost)) return fail(h, SDPGPU_ERR_ARG, "%s: fix_order_cost = %g is not finite", who, fix_order_cost);
    if (!std::isfinite(max_q) || max_q < 0) return fail(h, SDPGPU_ERR_ARG, "%s: max_q = %g (finite, at least 0)", who, max_q);
    if (!std::isfinite(vari_cost) || vari_cost <= 0) return fail(h, SDPGPU_ERR_ARG, "%s: vari_cost = %g (finite, above 0: the order is cash / vari_cost)", who, vari_cost);
    // NX of the tables: the descriptor's inventory points, as layout() counts them (below 2^31: validated at create)
    const int64_t nx = (int64_t)((d.max_inventory - d.min_inventory) / d.step) + 1;
    if (nx < 1 || nx >= 2147483647LL) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: the descriptor's inventory axis has %lld points", who, (long long)nx);
    const size_t tab_elems = (size_t)n_rules * T * (size_t)nx;
    const double* tabs[2] = {c1_tab, c2_tab};
    for (int w = 0; w < 2; ++w) {
      if (!tabs[w]) continue;
      for (size_t e = 0; e < tab_elems; ++e)
        if (std::isinf(tabs[w][e]))
          return fail(h, SDPGPU_ERR_ARG, "%s: c%d_tab[%zu][%zu][%zu] is infinite (a finite threshold, or NaN for an absent key)", who, w + 1,
                      e / ((size_t)T * nx), e / (size_t)nx % (size_t)T, e % (size_t)nx);
    }
    int rc = check_stream_args(h, who, n_paths, mode, first_path);
    if (rc) return rc;
    std::vector<sdp::SimSampler> rec;
    std::vector<double> thr, val;
    build_samplers(h, &rec, &thr, &val);
    std::vector<double> disc((size_t)T, 1.0);  // NULL = all 1.0: the bits of an explicit array of ones
    if (discount) disc.assign(discount, discount + T);
    std::vector<sdp::CashRulePeriod> per((size_t)T);
    for (int t = 0; t < T; ++t) {
      per[(size_t)t].P = rule_params(h, t, nx);
      per[(size_t)t].samp = rec[(size_t)t];
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
    const uint32_t n = (uint32_t)n_paths;
    const uint32_t W = (n + 63u) / 64u;
    sdp::CashRuleLaunch L{};
    L.ini_x = ini_x;
    L.ini_cash = ini_cash;
    L.T = T;
    L.n_rules = n_rules;
    L.waves_per_rule = W;

    const size_t nr = (size_t)n_rules, nn = (size_t)n;
    Carve c;
    const size_t o_per = c.take(per.size() * sizeof(sdp::CashRulePeriod));
    const size_t o_thr = c.take(thr.size() * 8), o_val = c.take(val.size() * 8);
    const size_t o_form = c.take(nr * sizeof(int32_t)), o_rule = c.take(nr * T * 4 * 8);
    const size_t o_c1 = c.take(c1_tab ? tab_elems * 8 : 0), o_c2 = c.take(c2_tab ? tab_elems * 8 : 0);
    const size_t o_cnt = c.take(2 * nr * sizeof(unsigned int)), o_res = c.take(2 * nr * 8), o_part = c.take(nr * W * 8);
    const size_t o_sum = c.take(nr * nn * 8);
    rc = sim_scratch(h, c.at);
    if (rc) return rc;
    if (!h->sim_ev0) {
      HIP_TRY(h, hipEventCreate(&h->sim_ev0));
      HIP_TRY(h, hipEventCreate(&h->sim_ev1));
    }
    char* base = h->d_sim_scratch;
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(base + o_per, per.data(), per.size() * sizeof(sdp::CashRulePeriod), hipMemcpyHostToDevice, st));
    if (!thr.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_thr, thr.data(), thr.size() * 8, hipMemcpyHostToDevice, st));
    if (!val.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_val, val.data(), val.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(base + o_form, form, nr * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(base + o_rule, rule, nr * T * 4 * 8, hipMemcpyHostToDevice, st));
    if (c1_tab) HIP_TRY(h, hipMemcpyAsync(base + o_c1, c1_tab, tab_elems * 8, hipMemcpyHostToDevice, st));
    if (c2_tab) HIP_TRY(h, hipMemcpyAsync(base + o_c2, c2_tab, tab_elems * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemsetAsync(base + o_cnt, 0, 2 * nr * sizeof(unsigned int), st));
    const sdp::CashRulePeriod* d_per = reinterpret_cast<const sdp::CashRulePeriod*>(base + o_per);
    const double* d_thr = reinterpret_cast<const double*>(base + o_thr);
    const double* d_val = reinterpret_cast<const double*>(base + o_val);
    const int32_t* d_form = reinterpret_cast<const int32_t*>(base + o_form);
    const double* d_rule = reinterpret_cast<const double*>(base + o_rule);
    const double* d_c1 = c1_tab ? reinterpret_cast<const double*>(base + o_c1) : nullptr;
    const double* d_c2 = c2_tab ? reinterpret_cast<const double*>(base + o_c2) : nullptr;
    unsigned int* d_cnt = reinterpret_cast<unsigned int*>(base + o_cnt);
    double* d_res = reinterpret_cast<double*>(base + o_res);
    double* d_part = reinterpret_cast<double*>(base + o_part);
    double* d_sum = reinterpret_cast<double*>(base + o_sum);
    const sdp::SimStream R = make_stream(n_paths, seed, first_path);
    const dim3 grid((unsigned)((nr * W + 3) / 4));  // (at most 16 x 2^18 waves)
    HIP_TRY(h, hipEventRecord(h->sim_ev0, st));
    if (mode == SDPGPU_SAMPLE_RANDOM)
      hipLaunchKernelGGL((sdp::cash_rule_sim_kernel<true>), grid, dim3(256), 0, st, L, R, d_per, d_thr, d_val, d_form, d_rule,
                         d_c1, d_c2, d_sum, d_part, d_cnt);
    else
      hipLaunchKernelGGL((sdp::cash_rule_sim_kernel<false>), grid, dim3(256), 0, st, L, R, d_per, d_thr, d_val, d_form, d_rule,
                         d_c1, d_c2, d_sum, d_part, d_cnt);
    HIP_TRY(h, hipGetLastError());
    // per rule, as sdpgpu_simulate_sampled: mean = (partials in the fixed order) / n; m2 = a second pass over the sums
    for (size_t r = 0; r < nr; ++r) HIP_TRY(h, launch_sim_moments(st, d_sum + r * nn, n, d_part + r * W, d_cnt + 2 * r, d_res + 2 * r));
    HIP_TRY(h, hipEventRecord(h->sim_ev1, st));
    std::vector<double> res(2 * nr, 0.0);
    std::vector<unsigned int> cnt(2 * nr, 0u);
    HIP_TRY(h, hipMemcpyAsync(res.data(), d_res, 2 * nr * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(cnt.data(), d_cnt, 2 * nr * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (out_sum) HIP_TRY(h, hipMemcpyAsync(out_sum, d_sum, nr * nn * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->sim_ev0, h->sim_ev1));
    for (size_t r = 0; r < nr; ++r) {
      results[r].n_paths = n_paths;
      results[r].n_valid = (int32_t)cnt[2 * r];  // every path of a rule: no path ever becomes invalid
      results[r].n_lost = 0;
      results[r].reserved = 0;
      results[r].mean = res[2 * r];
      results[r].m2 = res[2 * r + 1];
      results[r].kernel_ms = ms;
    }
    return SDPGPU_OK;
  });
}

}  // extern "C"
