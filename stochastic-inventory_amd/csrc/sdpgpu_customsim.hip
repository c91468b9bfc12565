// sdpgpu_customsim.hip -- sdpgpu_custom_simulate, sdpgpu_custom_simulate_sampled, sdpgpu_custom_rule_simulate: the rollouts of a
// USER-FUNCTOR handle (sdpgpu_create_custom) on the device -- the policy tables along given or sampled demand paths, and the
// overdraft drivers' ordering rules (CashSimulation.java:1142-1250).  Definition: DESIGN 4, "User-functor rollouts"; device
// text: kCustomSim of sdp_custom_src.hpp, compiled by hipRTC around the handle's own text at its first rollout call.  All
// argument validation comes before the compile, the compile before the solve-state and device checks (hipRTC needs no GPU: a
// text that does not compile is reported on a box without one).  The draws are sdpgpu_simulate_sampled's (check_stream_args,
// build_samplers, make_stream, launch_sim_draw) into a device buffer the hipRTC kernel reads; the reduction is the
// handle's (launch_sim_moments) from wave partials a small precompiled pass forms over the sums with sim_wave_sum.
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
  const unsigned long long mv = __ballot(valid);
  const double tot = sdp::sim_wave_sum(v);
  if (lane == 0) {
    partial[(int64_t)r * W + w] = tot;
    atomicAdd(&counts[2 * r], (unsigned int)__popcll(mv));
  }
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

int check_solved(sdpgpu_handle* h, const char* who) {
  if (!h->allocated) return fail(h, SDPGPU_ERR_STATE, "%s: nothing has been solved", who);
  for (int t = 0; t < h->T; ++t)
    if (!h->policy_done[t]) return fail(h, SDPGPU_ERR_STATE, "%s: period %d has not been computed", who, t + 1);
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
  std::vector<sdp::SimSampler> rec;
  std::vector<double> thr, val;
  if (!demand) build_samplers(h, &rec, &thr, &val);
  std::vector<double> disc((size_t)T, 1.0);  // NULL = all 1.0: the bits of an explicit array of ones
  if (discount) disc.assign(discount, discount + T);
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
  const size_t nn = (size_t)n_paths, np = std::max<size_t>(h->custom_params.size(), 1);
  const uint32_t n = (uint32_t)n_paths;
  const uint32_t W = (n + 63u) / 64u;
  Carve c;
  const size_t o_per = c.take(per.size() * sizeof(sdp::CustomSimPeriod)), o_samp = c.take(rec.size() * sizeof(sdp::SimSampler));
  const size_t o_thr = c.take(thr.size() * 8), o_val = c.take(val.size() * 8), o_user = c.take(np * 8);
  const size_t o_cnt = c.take(2 * sizeof(unsigned int)), o_res = c.take(2 * 8), o_part = c.take((size_t)W * 8);
  const size_t o_sum = c.take(nn * 8), o_flag = c.take(nn), o_dem = c.take(nn * T * 8);
  rc = sim_scratch(h, c.at);
  if (rc) return rc;
  if (!h->sim_ev0) {
    HIP_TRY(h, hipEventCreate(&h->sim_ev0));
    HIP_TRY(h, hipEventCreate(&h->sim_ev1));
  }
  char* base = h->d_sim_scratch;
  hipStream_t st = h->stream;
  HIP_TRY(h, hipMemcpyAsync(base + o_per, per.data(), per.size() * sizeof(sdp::CustomSimPeriod), hipMemcpyHostToDevice, st));
  if (!rec.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_samp, rec.data(), rec.size() * sizeof(sdp::SimSampler), hipMemcpyHostToDevice, st));
  if (!thr.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_thr, thr.data(), thr.size() * 8, hipMemcpyHostToDevice, st));
  if (!val.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_val, val.data(), val.size() * 8, hipMemcpyHostToDevice, st));
  if (!h->custom_params.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_user, h->custom_params.data(), h->custom_params.size() * 8, hipMemcpyHostToDevice, st));
  if (demand) HIP_TRY(h, hipMemcpyAsync(base + o_dem, demand, nn * T * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(h, hipMemsetAsync(base + o_cnt, 0, 2 * sizeof(unsigned int), st));
  const sdp::CustomSimPeriod* d_per = reinterpret_cast<const sdp::CustomSimPeriod*>(base + o_per);
  const sdp::SimSampler* d_samp = reinterpret_cast<const sdp::SimSampler*>(base + o_samp);
  const double* d_thr = reinterpret_cast<const double*>(base + o_thr);
  const double* d_val = reinterpret_cast<const double*>(base + o_val);
  const double* d_user = reinterpret_cast<const double*>(base + o_user);
  unsigned int* d_cnt = reinterpret_cast<unsigned int*>(base + o_cnt);
  double* d_res = reinterpret_cast<double*>(base + o_res);
  double* d_part = reinterpret_cast<double*>(base + o_part);
  double* d_sum = reinterpret_cast<double*>(base + o_sum);
  uint8_t* d_flag = reinterpret_cast<uint8_t*>(base + o_flag);
  double* d_dem = reinterpret_cast<double*>(base + o_dem);
  HIP_TRY(h, hipEventRecord(h->sim_ev0, st));
  if (!demand) HIP_TRY(h, launch_sim_draw(st, mode, make_stream((int32_t)n_paths, seed, first_path), T, d_samp, d_thr, d_val, d_dem, nullptr));
  {
    int Ti = T, fk = first_k;
    const int32_t* pol = h->d_policy;
    const double* dem_c = d_dem;
    long long ln = (long long)n_paths;
    void* args[] = {&d_per, &Ti, &pol, &d_user, &dem_c, &ln, &idx0, &ini_x, &ini_cash, &ini_preq, &fk, &d_sum, &d_flag};
    HIP_TRY(h, hipModuleLaunchKernel(h->custom_sim, (unsigned)((n_paths + 255) / 256), 1, 1, 256, 1, 1, 0, st, args, nullptr));
  }
  if (result) {
    hipLaunchKernelGGL(custom_partials_kernel, dim3((W + 3) / 4, 1), dim3(256), 0, st, d_sum, d_flag, n, W, d_part, d_cnt);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, launch_sim_moments(st, d_sum, n, d_part, d_cnt, d_res));
  }
  HIP_TRY(h, hipEventRecord(h->sim_ev1, st));
  double res[2] = {0, 0};
  unsigned int cnt[2] = {0, 0};
  if (result) {
    HIP_TRY(h, hipMemcpyAsync(res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  }
  if (out_sum) HIP_TRY(h, hipMemcpyAsync(out_sum, d_sum, nn * 8, hipMemcpyDeviceToHost, st));
  if (out_valid) HIP_TRY(h, hipMemcpyAsync(out_valid, d_flag, nn, hipMemcpyDeviceToHost, st));
  if (out_demand) HIP_TRY(h, hipMemcpyAsync(out_demand, d_dem, nn * T * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipStreamSynchronize(st));
  if (result) {
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->sim_ev0, h->sim_ev1));
    result->n_paths = (int32_t)n_paths;
    result->n_valid = (int32_t)cnt[0];
    result->n_lost = 0;
    result->reserved = 0;
    result->mean = res[0];
    result->m2 = res[1];
    result->kernel_ms = ms;
  }
  return SDPGPU_OK;
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
    for (int r = 0; r < n_rules; ++r)
      for (int t = 0; t < T; ++t)
        for (int k = 0; k < 4; ++k) {
          const double v = rule[((size_t)r * T + t) * 4 + k];
          if (!std::isfinite(v)) return fail(h, SDPGPU_ERR_ARG, "%s: rule[%d][%d][%d] = %g is not finite", who, r, t, k, v);
        }
    if (!std::isfinite(ini_x)) return fail(h, SDPGPU_ERR_ARG, "%s: ini_x = %g is not finite", who, ini_x);
    if (!std::isfinite(ini_cash)) return fail(h, SDPGPU_ERR_ARG, "%s: ini_cash = %g is not finite", who, ini_cash);
    if (discount)
      for (int t = 0; t < T; ++t)
        if (!std::isfinite(discount[t])) return fail(h, SDPGPU_ERR_ARG, "%s: discount[%d] = %g is not finite", who, t, discount[t]);
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
    std::vector<sdp::SimSampler> rec;
    std::vector<double> thr, val;
    build_samplers(h, &rec, &thr, &val);
    std::vector<double> disc((size_t)T, 1.0);  // NULL = all 1.0: the bits of an explicit array of ones
    if (discount) disc.assign(discount, discount + T);
    rc = compile_sim(h, who);
    if (rc) return rc;

    rc = no_device(h, who);
    if (rc) return rc;
    DeviceScope dev;
    HIP_TRY(h, dev.enter(h->device));
    rc = load_sim(h);
    if (rc) return rc;
    const uint32_t n = (uint32_t)n_paths;
    const uint32_t W = (n + 63u) / 64u;
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

    const size_t nr = (size_t)n_rules, nn = (size_t)n, np = std::max<size_t>(h->custom_params.size(), 1);
    Carve c;
    const size_t o_samp = c.take(rec.size() * sizeof(sdp::SimSampler)), o_thr = c.take(thr.size() * 8), o_val = c.take(val.size() * 8);
    const size_t o_user = c.take(np * 8), o_disc = c.take((size_t)T * 8);
    const size_t o_form = c.take(nr * sizeof(int32_t)), o_rule = c.take(nr * T * 4 * 8);
    const size_t o_cnt = c.take(2 * nr * sizeof(unsigned int)), o_res = c.take(2 * nr * 8), o_part = c.take(nr * W * 8);
    const size_t o_sum = c.take(nr * nn * 8), o_dem = c.take(nn * T * 8);
    rc = sim_scratch(h, c.at);
    if (rc) return rc;
    if (!h->sim_ev0) {
      HIP_TRY(h, hipEventCreate(&h->sim_ev0));
      HIP_TRY(h, hipEventCreate(&h->sim_ev1));
    }
    char* base = h->d_sim_scratch;
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(base + o_samp, rec.data(), rec.size() * sizeof(sdp::SimSampler), hipMemcpyHostToDevice, st));
    if (!thr.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_thr, thr.data(), thr.size() * 8, hipMemcpyHostToDevice, st));
    if (!val.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_val, val.data(), val.size() * 8, hipMemcpyHostToDevice, st));
    if (!h->custom_params.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_user, h->custom_params.data(), h->custom_params.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(base + o_disc, disc.data(), (size_t)T * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(base + o_form, form, nr * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(base + o_rule, rule, nr * T * 4 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemsetAsync(base + o_cnt, 0, 2 * nr * sizeof(unsigned int), st));
    const sdp::SimSampler* d_samp = reinterpret_cast<const sdp::SimSampler*>(base + o_samp);
    const double* d_thr = reinterpret_cast<const double*>(base + o_thr);
    const double* d_val = reinterpret_cast<const double*>(base + o_val);
    const double* d_user = reinterpret_cast<const double*>(base + o_user);
    const double* d_disc = reinterpret_cast<const double*>(base + o_disc);
    const int32_t* d_form = reinterpret_cast<const int32_t*>(base + o_form);
    const double* d_rule = reinterpret_cast<const double*>(base + o_rule);
    unsigned int* d_cnt = reinterpret_cast<unsigned int*>(base + o_cnt);
    double* d_res = reinterpret_cast<double*>(base + o_res);
    double* d_part = reinterpret_cast<double*>(base + o_part);
    double* d_sum = reinterpret_cast<double*>(base + o_sum);
    double* d_dem = reinterpret_cast<double*>(base + o_dem);
    HIP_TRY(h, hipEventRecord(h->sim_ev0, st));
    HIP_TRY(h, launch_sim_draw(st, mode, make_stream(n_paths, seed, first_path), T, d_samp, d_thr, d_val, d_dem, nullptr));
    {
      const double* dem_c = d_dem;
      void* args[] = {&L, &d_user, &d_disc, &dem_c, &d_form, &d_rule, &d_sum};
      HIP_TRY(h, hipModuleLaunchKernel(h->custom_rule_sim, (n + 255u) / 256u, (unsigned)n_rules, 1, 256, 1, 1, 0, st, args, nullptr));
    }
    const uint8_t* no_flags = nullptr;
    hipLaunchKernelGGL(custom_partials_kernel, dim3((W + 3) / 4, (unsigned)n_rules), dim3(256), 0, st, d_sum, no_flags, n, W, d_part, d_cnt);
    HIP_TRY(h, hipGetLastError());
    // per rule, as sdpgpu_simulate_sampled: mean = (partials in the fixed order) / n; m2 = a second pass over the sums
    for (size_t r = 0; r < nr; ++r) HIP_TRY(h, launch_sim_moments(st, d_sum + r * nn, n, d_part + r * W, d_cnt + 2 * r, d_res + 2 * r));
    HIP_TRY(h, hipEventRecord(h->sim_ev1, st));
    std::vector<double> res(2 * nr, 0.0);
    std::vector<unsigned int> cnt(2 * nr, 0u);
    HIP_TRY(h, hipMemcpyAsync(res.data(), d_res, 2 * nr * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(cnt.data(), d_cnt, 2 * nr * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (out_sum) HIP_TRY(h, hipMemcpyAsync(out_sum, d_sum, nr * nn * 8, hipMemcpyDeviceToHost, st));
    if (out_demand) HIP_TRY(h, hipMemcpyAsync(out_demand, d_dem, nn * T * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->sim_ev0, h->sim_ev1));
    for (size_t r = 0; r < nr; ++r) {
      results[r].n_paths = n_paths;
      results[r].n_valid = (int32_t)cnt[2 * r];  // every path of a rule: nothing is tested against a grid
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
