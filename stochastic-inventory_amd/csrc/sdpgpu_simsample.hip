// sdpgpu_simsample.hip -- sdpgpu_set_sampler, sdpgpu_simulate_sampled, sdpgpu_sample_demands: demand paths drawn on the
// device for a handle's policy simulation (kernels: sdp_sim_sampled.hpp; definition: DESIGN 4, "Sampled simulation on a
// handle").  All validation comes before the first device call; the device scratch of these entry points is ONE block kept
// on the handle (sim_scratch of sdpgpu_sim_host.hpp, which also holds what this unit shares with the batch's rollouts) and
// released by sdpgpu_destroy.
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
void build_samplers(const sdpgpu_handle* h, std::vector<sdp::SimSampler>* rec, std::vector<double>* thr, std::vector<double>* val) {
  rec->resize((size_t)h->T);
  for (int t = 0; t < h->T; ++t) {
    if (h->samp && h->samp->has((size_t)t)) {
      (*rec)[(size_t)t] = h->samp->append((size_t)t, thr);
      continue;
    }
    sdp::SimSampler S{};
    S.off = (int64_t)thr->size();
    S.k_lo = 0;
    S.strict = 0;
    S.m = (int32_t)h->pmf_p[(size_t)t].size();
    S.val_off = (int64_t)val->size();
    append_tile_thresholds(h->pmf_p[(size_t)t], thr);
    val->insert(val->end(), h->pmf_d[(size_t)t].begin(), h->pmf_d[(size_t)t].end());
    (*rec)[(size_t)t] = S;
  }
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
    std::vector<sdp::SimSampler> rec;
    std::vector<double> thr, val;
    build_samplers(h, &rec, &thr, &val);

    rc = no_device(h, who);
    if (rc) return rc;
    DeviceScope dev;
    HIP_TRY(h, dev.enter(h->device));
    const int T = h->T;
    const size_t elems = (size_t)n_paths * T;
    Carve c;
    const size_t o_samp = c.take(rec.size() * sizeof(sdp::SimSampler)), o_thr = c.take(thr.size() * 8), o_val = c.take(val.size() * 8);
    const size_t o_dem = c.take(elems * 8), o_u = c.take(out_u ? elems * 8 : 0);
    rc = sim_scratch(h, c.at);
    if (rc) return rc;
    char* base = h->d_sim_scratch;
    HIP_TRY(h, hipMemcpyAsync(base + o_samp, rec.data(), rec.size() * sizeof(sdp::SimSampler), hipMemcpyHostToDevice, h->stream));
    if (!thr.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_thr, thr.data(), thr.size() * 8, hipMemcpyHostToDevice, h->stream));
    if (!val.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_val, val.data(), val.size() * 8, hipMemcpyHostToDevice, h->stream));
    const sdp::SimStream R = make_stream(n_paths, seed, first_path);
    const sdp::SimSampler* d_samp = reinterpret_cast<const sdp::SimSampler*>(base + o_samp);
    const double* d_thr = reinterpret_cast<const double*>(base + o_thr);
    const double* d_val = reinterpret_cast<const double*>(base + o_val);
    double* d_dem = reinterpret_cast<double*>(base + o_dem);
    double* d_u = out_u ? reinterpret_cast<double*>(base + o_u) : nullptr;
    HIP_TRY(h, launch_sim_draw(h->stream, mode, R, T, d_samp, d_thr, d_val, d_dem, d_u));
    HIP_TRY(h, hipMemcpyAsync(out_demand, d_dem, elems * 8, hipMemcpyDeviceToHost, h->stream));
    if (out_u) HIP_TRY(h, hipMemcpyAsync(out_u, d_u, elems * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SDPGPU_OK;
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
    if (!h->allocated) return fail(h, SDPGPU_ERR_STATE, "%s: nothing has been solved", who);
    for (int t = 0; t < h->T; ++t)
      if (!h->policy_done[t]) return fail(h, SDPGPU_ERR_STATE, "%s: period %d has not been computed", who, t + 1);
    const int T = h->T;
    std::vector<sdp::SimSampler> rec;
    std::vector<double> thr, val;
    build_samplers(h, &rec, &thr, &val);
    std::vector<double> disc((size_t)T, 1.0);  // NULL = all 1.0: the bits of an explicit array of ones
    if (discount) disc.assign(discount, discount + T);

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
    const size_t nn = (size_t)n_paths;
    const uint32_t W = (uint32_t)((n_paths + 63) / 64);
    Carve c;
    const size_t o_per = c.take(per.size() * sizeof(sdp::SimPeriod)), o_samp = c.take(rec.size() * sizeof(sdp::SimSampler));
    const size_t o_disc = c.take((size_t)T * 8), o_thr = c.take(thr.size() * 8), o_val = c.take(val.size() * 8);
    const size_t o_cnt = c.take(2 * sizeof(unsigned int)), o_res = c.take(2 * 8), o_part = c.take((size_t)W * 8);
    const size_t o_sum = c.take(nn * 8), o_flag = c.take(nn);
    rc = sim_scratch(h, c.at);
    if (rc) return rc;
    if (!h->sim_ev0) {
      HIP_TRY(h, hipEventCreate(&h->sim_ev0));
      HIP_TRY(h, hipEventCreate(&h->sim_ev1));
    }
    char* base = h->d_sim_scratch;
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(base + o_per, per.data(), per.size() * sizeof(sdp::SimPeriod), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(base + o_samp, rec.data(), rec.size() * sizeof(sdp::SimSampler), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(base + o_disc, disc.data(), (size_t)T * 8, hipMemcpyHostToDevice, st));
    if (!thr.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_thr, thr.data(), thr.size() * 8, hipMemcpyHostToDevice, st));
    if (!val.empty()) HIP_TRY(h, hipMemcpyAsync(base + o_val, val.data(), val.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemsetAsync(base + o_cnt, 0, 2 * sizeof(unsigned int), st));
    const sdp::SimPeriod* d_per = reinterpret_cast<const sdp::SimPeriod*>(base + o_per);
    const sdp::SimSampler* d_samp = reinterpret_cast<const sdp::SimSampler*>(base + o_samp);
    const double* d_disc = reinterpret_cast<const double*>(base + o_disc);
    const double* d_thr = reinterpret_cast<const double*>(base + o_thr);
    const double* d_val = reinterpret_cast<const double*>(base + o_val);
    unsigned int* d_cnt = reinterpret_cast<unsigned int*>(base + o_cnt);
    double* d_res = reinterpret_cast<double*>(base + o_res);
    double* d_part = reinterpret_cast<double*>(base + o_part);
    double* d_sum = reinterpret_cast<double*>(base + o_sum);
    uint8_t* d_flag = reinterpret_cast<uint8_t*>(base + o_flag);
    const sdp::SimStream R = make_stream(n_paths, seed, first_path);
    const sdp::StateT ini{ini_x, ini_cash, ini_preq, ini_preq2};
    const dim3 grid((W + 3) / 4);
    HIP_TRY(h, hipEventRecord(h->sim_ev0, st));
    const hipError_t e = mode == SDPGPU_SAMPLE_RANDOM
                             ? launch_fused<true>(h, grid, d_per, d_samp, d_thr, d_val, d_disc, R, idx0, ini, (int)first_k, d_sum, d_flag, d_part, d_cnt)
                             : launch_fused<false>(h, grid, d_per, d_samp, d_thr, d_val, d_disc, R, idx0, ini, (int)first_k, d_sum, d_flag, d_part, d_cnt);
    HIP_TRY(h, e);
    HIP_TRY(h, launch_sim_moments(st, d_sum, (uint32_t)n_paths, d_part, d_cnt, d_res));
    HIP_TRY(h, hipEventRecord(h->sim_ev1, st));
    double res[2] = {0, 0};
    unsigned int cnt[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
    if (out_sum) HIP_TRY(h, hipMemcpyAsync(out_sum, d_sum, nn * 8, hipMemcpyDeviceToHost, st));
    if (out_valid) HIP_TRY(h, hipMemcpyAsync(out_valid, d_flag, nn, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->sim_ev0, h->sim_ev1));
    result->n_paths = n_paths;
    result->n_valid = (int32_t)cnt[0];
    result->n_lost = h->d.family == SDPGPU_FAMILY_SURVIVAL ? (int32_t)cnt[1] : 0;
    result->reserved = 0;
    result->mean = res[0];
    result->m2 = res[1];
    result->kernel_ms = ms;
    return SDPGPU_OK;
  });
}

}  // extern "C"
