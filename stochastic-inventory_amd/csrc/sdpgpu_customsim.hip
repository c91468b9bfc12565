// sdpgpu_customsim.hip -- sdpgpu_custom_simulate, sdpgpu_custom_simulate_sampled, sdpgpu_custom_rule_simulate: the rollouts of a
// USER-FUNCTOR handle (sdpgpu_create_custom) on the device -- the policy tables along given or sampled demand paths, and the
// overdraft drivers' ordering rules (CashSimulation.java:1142-1250).  Definition: DESIGN 4, "User-functor rollouts"; device
// text: kCustomSim of sdp_custom_src.hpp, compiled by hipRTC around the handle's own text at its first rollout call.  All
// argument validation comes before the compile, the compile before the solve-state and device checks (hipRTC needs no GPU: a
// text that does not compile is reported on a box without one).  The draws are sdpgpu_simulate_sampled's (launch_sim_draw) into a
// device buffer the hipRTC kernel reads; the host frame is RolloutFrame (sdpgpu_sim_host.hpp), which reduces from wave partials
// that a small precompiled pass forms over the sums.
#include <hip/hiprtc.h>

#include "sdpgpu_sim_host.hpp"
#include "sdp_custom_src.hpp"

using namespace sdpgpu_detail;

namespace sdpgpu_detail {
sdp::CustomParams make_custom_params(const sdpgpu_handle* h, int period);  // sdpgpu_generic.hip
}

namespace {

constexpr int32_t kCustomRuleMaxRules = 16;
constexpr int64_t kCustomSimMaxDemands = (int64_t)1 << 27;  // n_paths * T: the demand buffer is resident

// wave partials of n sums in the order of sim_sampled_kernel (xor butterfly, lanes past n hold 0.0) and, with flags, the number
// of paths whose bit 0 is set (without: n) -- what launch_sim_moments reads.  blockIdx.y: the rule.
__global__ __launch_bounds__(256) void custom_partials_kernel(const double* __restrict__ sums, const uint8_t* __restrict__ flags, uint32_t n,
                                                              uint32_t W, double* __restrict__ partial, unsigned int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const uint32_t r = blockIdx.y;
  const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (w >= W) return;  // no workgroup barrier below: a wave may leave on its own
  const uint32_t p = w * 64u + (uint32_t)lane;
  double v = 0.0;
  bool valid = false;
  if (p < n) {
    v = sums[(int64_t)r * n + p];
    valid = flags ? (flags[p] & 1) != 0 : true;
  }
  sdp::sim_wave_finish(partial, counts, (int64_t)r * W + w, r, valid, v);
}

int refuse(sdpgpu_handle* h, const char* who, bool rule) {
  const sdpgpu_desc& d = h->d;
  if (!h->custom)
    return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: not a user-functor handle -- a built-in family has sdpgpu_simulate* / sdpgpu_cash_rule_simulate", who);
  if (d.family == SDPGPU_FAMILY_SURVIVAL)
    return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: state shape SURVIVAL -- the survival loop's rollout (simulateLostSale) is not built for user texts", who);
  if (rule && d.family != SDPGPU_FAMILY_CASH && d.family != SDPGPU_FAMILY_OVERDRAFT)
    return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: handle of family %d -- the rules order from the (x, cash) state: a shape with a cash axis and no pipeline quantity (CASH, OVERDRAFT)", who, d.family);
  if (d.world_size != 1) return fail(h, SDPGPU_ERR_STATE, "%s needs one GPU (world_size 1), this handle is rank %d of %d", who, d.rank, d.world_size);
  return SDPGPU_OK;
}

// the rollout program: compiled once per handle, before anything touches a device
int compile_sim(sdpgpu_handle* h, const char* who) {
  if (!h->custom_sim_code.empty()) return SDPGPU_OK;
  const std::string src = std::string(sdp::kCustomPrelude) + h->custom_source + "\n" + sdp::kCustomCommon + sdp::kCustomSim;
  hiprtcProgram prog = nullptr;
  if (hiprtcCreateProgram(&prog, src.c_str(), "sdp_custom_sim.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    return fail(h, SDPGPU_ERR_DEVICE, "%s: hiprtcCreateProgram failed", who);
  std::vector<const char*> opts;
  for (const std::string& o : h->custom_sim_opts) opts.push_back(o.c_str());
  const hiprtcResult cr = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
  if (cr != HIPRTC_SUCCESS) {
    size_t n = 0;
    (void)hiprtcGetProgramLogSize(prog, &n);
    std::string log(n, '\0');
    if (n) (void)hiprtcGetProgramLog(prog, &log[0]);
    (void)hiprtcDestroyProgram(&prog);
    if (log.size() > 400) log.resize(400);
    return fail(h, SDPGPU_ERR_ARG, "%s: the rollout program does not compile around the user functor: %s", who, log.c_str());
  }
  size_t code_size = 0;
  (void)hiprtcGetCodeSize(prog, &code_size);
  std::vector<char> code(code_size);
  const hiprtcResult gr = hiprtcGetCode(prog, code.data());
  (void)hiprtcDestroyProgram(&prog);
  if (gr != HIPRTC_SUCCESS || code.empty()) return fail(h, SDPGPU_ERR_DEVICE, "%s: hiprtcGetCode failed", who);
  if (const char* dump = std::getenv("SDPGPU_CUSTOM_DUMP")) {  // the rollout object beside the engine's, for llvm-objdump -d
    const std::string path = std::string(dump) + ".sim";
    if (FILE* f = std::fopen(path.c_str(), "wb")) {
      (void)std::fwrite(code.data(), 1, code.size(), f);
      (void)std::fclose(f);
    }
  }
  h->custom_sim_code.swap(code);
  return SDPGPU_OK;
}

int load_sim(sdpgpu_handle* h) {
  if (h->custom_sim_mod) return SDPGPU_OK;
  HIP_TRY(h, hipModuleLoadData(&h->custom_sim_mod, h->custom_sim_code.data()));
  HIP_TRY(h, hipModuleGetFunction(&h->custom_sim, h->custom_sim_mod, "sdp_custom_sim"));
  HIP_TRY(h, hipModuleGetFunction(&h->custom_first, h->custom_sim_mod, "sdp_custom_first"));
  HIP_TRY(h, hipModuleGetFunction(&h->custom_rule_sim, h->custom_sim_mod, "sdp_custom_rule_sim"));
  return SDPGPU_OK;
}

int check_demand_cap(sdpgpu_handle* h, const char* who, int64_t n_paths) {
  if (n_paths * (int64_t)h->T > kCustomSimMaxDemands)
    return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: n_paths * T = %lld exceeds %lld (the demand buffer is resident)", who,
                (long long)(n_paths * (int64_t)h->T), (long long)kCustomSimMaxDemands);
  return SDPGPU_OK;
}

// the table rollout of both entry points.  demand != nullptr: GIVEN paths; else drawn (mode, seed, first_path).
int table_rollout(sdpgpu_handle* h, const char* who, int64_t n_paths, const double* demand, uint64_t seed, int32_t mode, uint64_t first_path,
                  const double* discount, double ini_x, double ini_cash, double ini_preq, sdpgpu_sim_result* result, double* out_sum,
                  uint8_t* out_valid, double* out_demand) {
  const int T = h->T;
  HostSamplers samp;
  if (!demand) build_samplers(h, &samp);
  const std::vector<double> disc = discounts_or_ones(discount, T);
  int rc = compile_sim(h, who);
  if (rc) return rc;
  rc = check_solved(h, who);
  if (rc) return rc;

  DeviceScope dev;
  HIP_TRY(h, dev.enter(h->device));
  rc = flush_api(h);
  if (rc) return rc;
  rc = load_sim(h);
  if (rc) return rc;
  if (!has_cash(h->d.family)) ini_cash = 0;
  if (!has_preq(h->d.family)) ini_preq = 0;
  double ini_preq2 = 0.0;
  long long idx0 = sdpgpu_state_index2(h, 1, ini_x, ini_cash, ini_preq, ini_preq2);
  int32_t first_k = 0;
  if (idx0 < 0) {  // off-grid start: its action as sdpgpu_eval_states forms it, a successor off the grid valued at 0 (sdp_custom_first)
    if (T > 1 && !h->period_done[1]) return fail(h, SDPGPU_ERR_STATE, "%s: V_2 has not been computed", who);
    rc = sim_scratch(h, 16);
    if (rc) return rc;
    sdp::CustomParams C1 = make_custom_params(h, 1);
    const double* v_next = T > 1 ? h->d_values + h->per[1].v_off : nullptr;
    const double* pd = h->d_pmf + h->per[0].pmf_off;
    const double* pp = pd + h->per[0].nD;
    const double* user = h->d_custom_params;
    int* d_k = reinterpret_cast<int*>(h->d_sim_scratch);
    void* args[] = {&C1, &user, &v_next, &pd, &pp, &ini_x, &ini_cash, &ini_preq, &d_k};
    HIP_TRY(h, hipModuleLaunchKernel(h->custom_first, 1, 1, 1, 64, 1, 1, 0, h->stream, args, nullptr));
    HIP_TRY(h, hipMemcpyAsync(&first_k, d_k, sizeof first_k, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  std::vector<sdp::CustomSimPeriod> per((size_t)T);
  for (int t = 0; t < T; ++t) {
    per[(size_t)t].P = make_custom_params(h, t + 1);
    per[(size_t)t].pol_off = (long long)h->per[t].pol_off - h->per[t].lo;
    per[(size_t)t].disc = disc[(size_t)t];
  }
  RolloutFrame<sdpgpu_handle> f(h, (uint32_t)n_paths, 1);
  const size_t elems = (size_t)f.n * T;
  const auto p_per = f.put(per.data(), per.size());
  const auto p_samp = f.put_samplers(samp, true);
  const auto p_user = f.put(h->custom_params.data(), h->custom_params.size(), 1);
  const auto p_flag = f.take<uint8_t>(f.n);
  const auto p_dem = f.put(demand, elems, elems);
  rc = f.begin();
  if (rc) return rc;
  hipStream_t st = h->stream;
  const sdp::CustomSimPeriod* d_per = f[p_per];
  const double *d_user = f[p_user], *d_dem = f[p_dem];
  double* d_sum = f.d_sum;
  uint8_t* d_flag = f[p_flag];
  rc = f.start();
  if (rc) return rc;
  if (!demand)
    HIP_TRY(h, launch_sim_draw(st, mode, make_stream((int32_t)n_paths, seed, first_path), T, f[p_samp.rec], f[p_samp.thr], f[p_samp.val],
                               f[p_dem], nullptr));
  {
    int Ti = T, fk = first_k;
    const int32_t* pol = h->d_policy;
    long long ln = (long long)n_paths;
    void* args[] = {&d_per, &Ti, &pol, &d_user, &d_dem, &ln, &idx0, &ini_x, &ini_cash, &ini_preq, &fk, &d_sum, &d_flag};
    HIP_TRY(h, hipModuleLaunchKernel(h->custom_sim, (unsigned)((n_paths + 255) / 256), 1, 1, 256, 1, 1, 0, st, args, nullptr));
  }
  if (result) {
    hipLaunchKernelGGL(custom_partials_kernel, dim3((f.W + 3) / 4, 1), dim3(256), 0, st, d_sum, d_flag, f.n, f.W, f.d_part, f.d_cnt);
    HIP_TRY(h, hipGetLastError());
  }
  f.download(out_valid, d_flag, f.n);
  f.download(out_demand, d_dem, elems * 8);
  return f.finish(result, out_sum);
}

}  // namespace

extern "C" {

int sdpgpu_custom_simulate(sdpgpu_handle* h, int64_t n_paths, const double* demand, const double* discount, double ini_x, double ini_cash,
                           double ini_preq, double* out_sum, uint8_t* out_valid) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_custom_simulate", [&]() -> int {
    const char* who = "sdpgpu_custom_simulate";
    int rc = refuse(h, who, false);
    if (rc) return rc;
    if (!demand) return fail(h, SDPGPU_ERR_ARG, "%s: demand is null", who);
    if (!discount) return fail(h, SDPGPU_ERR_ARG, "%s: discount is null", who);
    if (!out_sum) return fail(h, SDPGPU_ERR_ARG, "%s: out_sum is null", who);
    if (!out_valid) return fail(h, SDPGPU_ERR_ARG, "%s: out_valid is null", who);
    if (n_paths < 0) return fail(h, SDPGPU_ERR_ARG, "%s: n_paths = %lld (0 .. %d)", who, (long long)n_paths, kSimMaxPaths);
    if (n_paths > kSimMaxPaths) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: n_paths = %lld exceeds %d", who, (long long)n_paths, kSimMaxPaths);
    rc = check_demand_cap(h, who, n_paths);
    if (rc) return rc;
    if (n_paths == 0) {  // (nothing to roll: the solve state is still the caller's business)
      rc = compile_sim(h, who);
      return rc ? rc : check_solved(h, who);
    }
    return table_rollout(h, who, n_paths, demand, 0, 0, 0, discount, ini_x, ini_cash, ini_preq, nullptr, out_sum, out_valid, nullptr);
  });
}

int sdpgpu_custom_simulate_sampled(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path, const double* discount,
                                   double ini_x, double ini_cash, double ini_preq, sdpgpu_sim_result* result, double* out_sum,
                                   uint8_t* out_valid, double* out_demand) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_custom_simulate_sampled", [&]() -> int {
    const char* who = "sdpgpu_custom_simulate_sampled";
    int rc = refuse(h, who, false);
    if (rc) return rc;
    if (!result) return fail(h, SDPGPU_ERR_ARG, "%s: result is null", who);
    rc = check_stream_args(h, who, n_paths, mode, first_path);
    if (rc) return rc;
    rc = check_demand_cap(h, who, n_paths);
    if (rc) return rc;
    return table_rollout(h, who, n_paths, nullptr, seed, mode, first_path, discount, ini_x, ini_cash, ini_preq, result, out_sum, out_valid,
                         out_demand);
  });
}

int sdpgpu_custom_rule_simulate(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path, const double* discount,
                                double ini_x, double ini_cash, int32_t n_rules, const int32_t* form, const double* rule,
                                double min_cash_required, double max_q, double fix_order_cost, double vari_cost, sdpgpu_sim_result* results,
                                double* out_sum, double* out_demand) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_custom_rule_simulate", [&]() -> int {
    const char* who = "sdpgpu_custom_rule_simulate";
    int rc = refuse(h, who, true);
    if (rc) return rc;
    if (!form) return fail(h, SDPGPU_ERR_ARG, "%s: form is null", who);
    if (!rule) return fail(h, SDPGPU_ERR_ARG, "%s: rule is null", who);
    if (!results) return fail(h, SDPGPU_ERR_ARG, "%s: results is null", who);
    if (n_rules < 1 || n_rules > kCustomRuleMaxRules) return fail(h, SDPGPU_ERR_ARG, "%s: n_rules = %d (1 .. %d)", who, n_rules, kCustomRuleMaxRules);
    const int T = h->T;
    bool scalars_read = false;  // (form 2, simulatesSOD2, takes no scalars)
    for (int r = 0; r < n_rules; ++r) {
      if (form[r] < SDPGPU_ORULE_SS || form[r] > SDPGPU_ORULE_SCS1S2)
        return fail(h, SDPGPU_ERR_ARG, "%s: form[%d] = %d (SDPGPU_ORULE_SS 0, SDPGPU_ORULE_SCS 1, SDPGPU_ORULE_SCS1S2 2)", who, r, form[r]);
      scalars_read = scalars_read || form[r] != SDPGPU_ORULE_SCS1S2;
    }
    rc = check_finite(h, who, "rule", rule, (size_t)n_rules * T * 4, {(size_t)T, 4});
    if (rc) return rc;
    if (!std::isfinite(ini_x)) return fail(h, SDPGPU_ERR_ARG, "%s: ini_x = %g is not finite", who, ini_x);
    if (!std::isfinite(ini_cash)) return fail(h, SDPGPU_ERR_ARG, "%s: ini_cash = %g is not finite", who, ini_cash);
    if (discount && (rc = check_finite(h, who, "discount", discount, (size_t)T))) return rc;
    if (scalars_read) {
      if (!std::isfinite(min_cash_required)) return fail(h, SDPGPU_ERR_ARG, "%s: min_cash_required = %g is not finite", who, min_cash_required);
      if (!std::isfinite(fix_order_cost)) return fail(h, SDPGPU_ERR_ARG, "%s: fix_order_cost = %g is not finite", who, fix_order_cost);
      if (!std::isfinite(max_q) || max_q < 0) return fail(h, SDPGPU_ERR_ARG, "%s: max_q = %g (finite, at least 0)", who, max_q);
      if (!std::isfinite(vari_cost) || vari_cost <= 0) return fail(h, SDPGPU_ERR_ARG, "%s: vari_cost = %g (finite, above 0: the order is cash / vari_cost)", who, vari_cost);
    }
    rc = check_stream_args(h, who, n_paths, mode, first_path);
    if (rc) return rc;
    rc = check_demand_cap(h, who, n_paths);
    if (rc) return rc;
    HostSamplers samp;
    build_samplers(h, &samp);
    const std::vector<double> disc = discounts_or_ones(discount, T);
    rc = compile_sim(h, who);
    if (rc) return rc;

    rc = no_device(h, who);
    if (rc) return rc;
    DeviceScope dev;
    HIP_TRY(h, dev.enter(h->device));
    rc = load_sim(h);
    if (rc) return rc;
    const uint32_t n = (uint32_t)n_paths;
    sdp::CustomRuleLaunch L{};
    L.ini_x = ini_x;
    L.ini_cash = ini_cash;
    L.step = h->d.step;
    L.min_cash_required = min_cash_required;
    L.max_q = max_q;
    L.fix_order_cost = fix_order_cost;
    L.vari_cost = vari_cost;
    L.T = T;
    L.n_rules = n_rules;
    L.n_paths = n;

    RolloutFrame<sdpgpu_handle> f(h, n, (size_t)n_rules);
    const size_t elems = (size_t)n * T;
    const auto p_samp = f.put_samplers(samp, true);
    const auto p_user = f.put(h->custom_params.data(), h->custom_params.size(), 1);
    const auto p_disc = f.put(disc.data(), disc.size());
    const auto p_form = f.put(form, f.nr);
    const auto p_rule = f.put(rule, f.nr * T * 4), p_dem = f.take<double>(elems);
    rc = f.begin();
    if (rc) return rc;
    hipStream_t st = h->stream;
    const double *d_user = f[p_user], *d_disc = f[p_disc], *d_rule = f[p_rule], *d_dem = f[p_dem];
    const int32_t* d_form = f[p_form];
    double* d_sum = f.d_sum;
    rc = f.start();
    if (rc) return rc;
    HIP_TRY(h, launch_sim_draw(st, mode, make_stream(n_paths, seed, first_path), T, f[p_samp.rec], f[p_samp.thr], f[p_samp.val], f[p_dem], nullptr));
    {
      void* args[] = {&L, &d_user, &d_disc, &d_dem, &d_form, &d_rule, &d_sum};
      HIP_TRY(h, hipModuleLaunchKernel(h->custom_rule_sim, (n + 255u) / 256u, (unsigned)n_rules, 1, 256, 1, 1, 0, st, args, nullptr));
    }
    const uint8_t* no_flags = nullptr;
    hipLaunchKernelGGL(custom_partials_kernel, dim3((f.W + 3) / 4, (unsigned)n_rules), dim3(256), 0, st, d_sum, no_flags, n, f.W, f.d_part, f.d_cnt);
    HIP_TRY(h, hipGetLastError());
    f.download(out_demand, d_dem, elems * 8);
    return f.finish(results, out_sum);  // (n_valid: every path of a rule -- nothing is tested against a grid)
  });
}

}  // extern "C"
