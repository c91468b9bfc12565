// sdpgpu_simsample.hip -- sdpgpu_set_sampler, sdpgpu_simulate_sampled, sdpgpu_sample_demands: demand paths drawn on the
// device for a handle's policy simulation (kernels: sdp_sim_sampled.hpp; definition: DESIGN 4, "Sampled simulation on a
// handle") -- and what every handle rollout takes from here: the stream refusals, the sampler records, the parameter block
// without a layout, the draws and the fixed-order reduction.  All validation comes before the first device call; the host frame
// is RolloutFrame (sdpgpu_sim_host.hpp), its scratch block is released by sdpgpu_destroy.
#include "sdpgpu_sim_host.hpp"
#include "sdp_sim_sampled.hpp"

using namespace sdpgpu_detail;

namespace {

// the refusals sdpgpu_simulate has, in its order (the solve state is the caller's business)
int refuse(sdpgpu_handle* h, const char* who) {
  if (h->d.cash_formula == 2)
    return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: not built for the (x, R) state of CashConstraintXR (CashSimulationXR is out of scope)", who);
  if (h->d.world_size != 1) return fail(h, SDPGPU_ERR_STATE, "%s needs the whole policy on one GPU (world_size 1)", who);
  if (h->custom) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: a user functor's lambdas live on the host; roll the policy tables forward there", who);
  if (h->d.family == SDPGPU_FAMILY_STAFF)
    return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: the workforce drivers simulate an (s, S) rule with binomial draws (SimulatesS.java), not the table policy along demand paths", who);
  return SDPGPU_OK;
}

template <bool RANDOM>
hipError_t launch_fused(sdpgpu_handle* h, dim3 grid, const sdp::SimPeriod* d_per, const sdp::SimSampler* d_samp, const double* d_thr,
                        const double* d_val, const double* d_disc, const sdp::SimStream& R, int64_t idx0, const sdp::StateT& ini, int first_k,
                        double* d_sum, uint8_t* d_flags, double* d_part, unsigned int* d_counts) {
  const int T = h->T;
#define SDP_SIMS(F)                                                                                                                  \
  case F:                                                                                                                            \
    hipLaunchKernelGGL((sdp::sim_sampled_kernel<F, RANDOM>), grid, dim3(256), 0, h->stream, d_per, T, h->d_policy, d_samp, d_thr, d_val, \
                       d_disc, R, idx0, ini, first_k, d_sum, d_flags, d_part, d_counts);                                             \
    break;
  switch (h->d.family) {
    SDP_SIMS(sdp::FAM_BACKORDER)
    SDP_SIMS(sdp::FAM_LEADTIME)
    SDP_SIMS(sdp::FAM_CASH)
    SDP_SIMS(sdp::FAM_OVERDRAFT)
    SDP_SIMS(sdp::FAM_CASH_LEADTIME)
    SDP_SIMS(sdp::FAM_SURVIVAL)
    default:
      return hipErrorInvalidValue;
  }
#undef SDP_SIMS
  return hipGetLastError();
}

}  // namespace

namespace sdpgpu_detail {

int check_stream_args(sdpgpu_handle* h, const char* who, int32_t n_paths, int32_t mode, uint64_t first_path) {
  if (const int rc = check_n_paths(h, who, n_paths)) return rc;
  if (mode != SDPGPU_SAMPLE_LHS && mode != SDPGPU_SAMPLE_RANDOM)
    return fail(h, SDPGPU_ERR_ARG, "%s: mode = %d (SDPGPU_SAMPLE_LHS 0, SDPGPU_SAMPLE_RANDOM 1)", who, mode);
  if (mode == SDPGPU_SAMPLE_LHS && first_path != 0)
    return fail(h, SDPGPU_ERR_ARG, "%s: first_path = %llu -- a latin hypercube is one whole of n_paths strata, first_path must be 0", who,
                (unsigned long long)first_path);
  for (int t = 0; t < h->T; ++t) {
    const bool spec = h->samp && h->samp->has((size_t)t);
    if (!spec && !h->pmf_set[(size_t)t]) return fail(h, SDPGPU_ERR_STATE, "%s: pmf of period %d not set and no sampler spec given", who, t + 1);
  }
  return SDPGPU_OK;
}

// sampler records and their two arenas: spec tables as set (demand = k_lo + q); tile tables = the running fp64 sum of the
// tile's probabilities in ascending order, the last threshold +infinity, and the tile's demand VALUES (gaps, any step)
void build_samplers(const sdpgpu_handle* h, HostSamplers* s) {
  s->rec.resize((size_t)h->T);
  for (int t = 0; t < h->T; ++t) {
    if (h->samp && h->samp->has((size_t)t)) {
      s->rec[(size_t)t] = h->samp->append((size_t)t, &s->thr);
      continue;
    }
    sdp::SimSampler S{};
    S.off = (int64_t)s->thr.size();
    S.k_lo = 0;
    S.strict = 0;
    S.m = (int32_t)h->pmf_p[(size_t)t].size();
    S.val_off = (int64_t)s->val.size();
    append_tile_thresholds(h->pmf_p[(size_t)t], &s->thr);
    s->val.insert(s->val.end(), h->pmf_d[(size_t)t].begin(), h->pmf_d[(size_t)t].end());
    s->rec[(size_t)t] = S;
  }
}

// the period's parameter block without a layout (the rollout reads no table, so it needs no pmf tile where a spec is set): the
// family's scalars and the handle's overhead from make_params, the boxes from the descriptor as layout() forms them (the rule
// rollouts of sdpgpu_cashrulesim.hip and sdpgpu_xrsim.hip)
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

// the demands of a stream into a device buffer, out[p * T + t] (and the uniforms where d_u is given): sim_sampled_draw_kernel
hipError_t launch_sim_draw(hipStream_t st, int32_t mode, const sdp::SimStream& R, int T, const sdp::SimSampler* d_samp, const double* d_thr,
                           const double* d_val, double* d_dem, double* d_u) {
  const dim3 grid((unsigned)((R.n_paths + 255u) / 256u));
  if (mode == SDPGPU_SAMPLE_RANDOM)
    hipLaunchKernelGGL((sdp::sim_sampled_draw_kernel<true>), grid, dim3(256), 0, st, R, T, d_samp, d_thr, d_val, d_dem, d_u);
  else
    hipLaunchKernelGGL((sdp::sim_sampled_draw_kernel<false>), grid, dim3(256), 0, st, R, T, d_samp, d_thr, d_val, d_dem, d_u);
  return hipGetLastError();
}

// mean = (wave partials in the fixed order) / n; m2 = a second pass over the sums in the same order (which reuses the partials)
hipError_t launch_sim_moments(hipStream_t st, const double* d_sum, uint32_t n, double* d_part, const unsigned int* d_cnt, double* d_res) {
  const uint32_t W = (n + 63u) / 64u;
  hipLaunchKernelGGL(sdp::sim_reduce_kernel, dim3(1), dim3(1024), 0, st, d_part, W, (double)n, d_cnt, n, d_res);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sdp::sim_dev2_kernel, dim3((W + 3) / 4), dim3(256), 0, st, d_sum, n, d_res, d_part);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(sdp::sim_reduce_kernel, dim3(1), dim3(1024), 0, st, d_part, W, 0.0, d_cnt, n, d_res + 1);
  return hipGetLastError();
}

}  // namespace sdpgpu_detail

extern "C" {

int sdpgpu_set_sampler(sdpgpu_handle* h, int32_t t, const sdpgpu_dist_spec* spec) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_set_sampler", [&]() -> int {
    if (t < 0 || t >= h->T) return fail(h, SDPGPU_ERR_ARG, "set_sampler: period index %d outside 0 .. %d", t, h->T - 1);
    if (!h->samp) {  // (a NULL spec at any step creates them too: unlike a batch, whose tables all need step 1)
      h->samp = std::make_shared<SamplerSpecs>();
      h->samp->resize((size_t)h->T);
    }
    if (!spec) {  // back to the pmf tile (any step)
      h->samp->clear((size_t)t);
      return SDPGPU_OK;
    }
    if (h->d.step != 1.0)
      return fail(h, SDPGPU_ERR_UNSUPPORTED, "set_sampler: step %g -- a spec's demands are Math.round's integers (Simulation.java:64), it needs step == 1 "
                  "(the pmf tile samples at any step)", h->d.step);
    std::string why;
    const int rc = h->samp->set((size_t)t, *spec, &why);
    if (rc) return fail(h, rc, "set_sampler: period %d: spec: %s", t + 1, why.c_str());
    return SDPGPU_OK;
  });
}

int sdpgpu_sample_demands(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path, double* out_demand,
                          double* out_u) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_sample_demands", [&]() -> int {
    const char* who = "sdpgpu_sample_demands";
    int rc = refuse(h, who);
    if (rc) return rc;
    if (!out_demand) return fail(h, SDPGPU_ERR_ARG, "%s: out_demand is null", who);
    rc = check_stream_args(h, who, n_paths, mode, first_path);
    if (rc) return rc;
    HostSamplers samp;
    build_samplers(h, &samp);

    rc = no_device(h, who);
    if (rc) return rc;
    DeviceScope dev;
    HIP_TRY(h, dev.enter(h->device));
    const int T = h->T;
    const size_t elems = (size_t)n_paths * T;
    RolloutFrame<sdpgpu_handle> f(h, (uint32_t)n_paths, 0);
    const auto p_samp = f.put_samplers(samp, true);
    const auto p_dem = f.take<double>(elems), p_u = f.take<double>(out_u ? elems : 0);
    rc = f.begin();
    if (rc) return rc;
    HIP_TRY(h, launch_sim_draw(h->stream, mode, make_stream(n_paths, seed, first_path), T, f[p_samp.rec], f[p_samp.thr], f[p_samp.val], f[p_dem], f[p_u]));
    f.download(out_demand, f[p_dem], elems * 8);
    f.download(out_u, f[p_u], elems * 8);
    return f.deliver();
  });
}

int sdpgpu_simulate_sampled(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path, const double* discount,
                            double ini_x, double ini_cash, double ini_preq, sdpgpu_sim_result* result, double* out_sum,
                            uint8_t* out_valid) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_simulate_sampled", [&]() -> int {
    const char* who = "sdpgpu_simulate_sampled";
    int rc = refuse(h, who);
    if (rc) return rc;
    if (!result) return fail(h, SDPGPU_ERR_ARG, "%s: result is null", who);
    rc = check_stream_args(h, who, n_paths, mode, first_path);
    if (rc) return rc;
    rc = check_solved(h, who);
    if (rc) return rc;
    const int T = h->T;
    HostSamplers samp;
    build_samplers(h, &samp);
    const std::vector<double> disc = discounts_or_ones(discount, T);

    DeviceScope dev;
    HIP_TRY(h, dev.enter(h->device));
    rc = flush_api(h);
    if (rc) return rc;
    if (!has_cash(h->d.family)) ini_cash = 0;
    if (!has_preq(h->d.family)) ini_preq = 0;
    double ini_preq2 = h->d.lead_time == 2 ? h->d.ini_preq2 : 0.0;
    const int64_t idx0 = sdpgpu_state_index2(h, 1, ini_x, ini_cash, ini_preq, ini_preq2);
    int32_t first_k = 0;
    if (idx0 < 0) {  // off-grid start: its action from sdpgpu_eval_states2, as sdpgpu_simulate
      double v;
      rc = sdpgpu_eval_states2(h, 1, 1, &ini_x, &ini_cash, &ini_preq, &ini_preq2, &v, &first_k);
      if (rc) return rc;
    }
    std::vector<sdp::SimPeriod> per((size_t)T);
    for (int t = 0; t < T; ++t) {
      per[(size_t)t].P = make_params(h, t + 1);
      per[(size_t)t].pol_off = (int64_t)h->per[t].pol_off - h->per[t].lo;
      per[(size_t)t].n_states = h->per[t].S;
    }
    RolloutFrame<sdpgpu_handle> f(h, (uint32_t)n_paths, 1);
    const auto p_per = f.put(per.data(), per.size());
    const auto p_samp = f.put_samplers(samp, true);
    const auto p_disc = f.put(disc.data(), disc.size());
    const auto p_flag = f.take<uint8_t>(f.n);
    rc = f.begin();
    if (rc) return rc;
    const sdp::SimStream R = make_stream(n_paths, seed, first_path);
    const sdp::StateT ini{ini_x, ini_cash, ini_preq, ini_preq2};
    const dim3 grid((f.W + 3) / 4);
    rc = f.start();
    if (rc) return rc;
    const hipError_t e = mode == SDPGPU_SAMPLE_RANDOM
                             ? launch_fused<true>(h, grid, f[p_per], f[p_samp.rec], f[p_samp.thr], f[p_samp.val], f[p_disc], R, idx0, ini, (int)first_k, f.d_sum, f[p_flag], f.d_part, f.d_cnt)
                             : launch_fused<false>(h, grid, f[p_per], f[p_samp.rec], f[p_samp.thr], f[p_samp.val], f[p_disc], R, idx0, ini, (int)first_k, f.d_sum, f[p_flag], f.d_part, f.d_cnt);
    HIP_TRY(h, e);
    f.download(out_valid, f[p_flag], f.n);
    rc = f.finish(result, out_sum);
    if (rc) return rc;
    if (h->d.family == SDPGPU_FAMILY_SURVIVAL) result->n_lost = (int32_t)f.cnt[1];  // the survival loop's second counter
    return SDPGPU_OK;
  });
}

}  // extern "C"
