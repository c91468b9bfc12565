// sdpgpu_multisim.hip -- sdpgpu_multi_policy_*: a policy object over the memo of a two-product solve (sdpgpu_multilead_solve,
// sdpgpu_multicash_solve, sdpgpu_multixr_solve) and its rollouts on the device -- what CashSimulationMulti and
// CashSimulationMultiXR do with recursion.getAction(state) (kernels and the table: sdp_multi_sim.hpp; definition: DESIGN 4,
// "Two-product rollout").  The descriptor is read by the solver's own checks (multilead_problem / multicash_problem of
// sdpgpu_sparse.hip), errors go through sdpgpu_multilead_last_error and every entry point sits behind ml_guard, as the three
// solves do.  All validation comes before the first device call.  The path-count refusals, the stream record, the threshold
// table of a tile and the host frame (RolloutFrame) are those of the other rollouts (sdpgpu_sim_host.hpp).
#include <cstdarg>

#include "sdpgpu_sim_host.hpp"
#include "sdp_multi_sim.hpp"

using namespace sdpgpu_detail;
using sdp_multi::ml_error;
using sdp_multi::ml_guard;

struct sdpgpu_multi_policy {
  sdp_multi::Problem pb;
  std::vector<double> thr;  // per tile: the running fp64 sum of its probabilities in list order, the last one +infinity
  int device = -1;
  hipStream_t stream = nullptr;  // the null stream, as the solves
  uint32_t rows = 0, mask = 0;
  sdp_multi::PolicyRecord* d_rec = nullptr;
  uint32_t* d_slots = nullptr;
  double2* d_dem = nullptr;
  double* d_thr = nullptr;
  char* d_sim_scratch = nullptr;  // sim_scratch of sdpgpu_sim_host.hpp
  size_t sim_scratch_bytes = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace {

int mfail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  ml_error() = buf;
  return code;
}

}  // namespace

// the error sink of the shared host helpers (check_n_paths, no_device, RolloutFrame) for this owner, and its timing events: the
// pair its create made
template <class... A>
int sim_fail(sdpgpu_multi_policy*, int code, const char* fmt, A... a) {
  return mfail(code, fmt, a...);
}
inline hipError_t sim_events(sdpgpu_multi_policy* p, hipEvent_t* ev0, hipEvent_t* ev1) {
  *ev0 = p->ev0;
  *ev1 = p->ev1;
  return hipSuccess;
}

namespace {

#define MS_TRY(expr)                                                                                  \
  do {                                                                                                \
    const hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return mfail(SDPGPU_ERR_DEVICE, "%s (sdpgpu_multisim.hip:%d): %s", #expr, __LINE__, hipGetErrorString(e_)); \
  } while (0)

void release(sdpgpu_multi_policy* p) {
  if (!p) return;
  DeviceScope dev;
  if (p->device >= 0) (void)dev.enter(p->device);
  if (p->d_rec) (void)hipFree(p->d_rec);
  if (p->d_slots) (void)hipFree(p->d_slots);
  if (p->d_dem) (void)hipFree(p->d_dem);
  if (p->d_thr) (void)hipFree(p->d_thr);
  if (p->d_sim_scratch) (void)hipFree(p->d_sim_scratch);
  if (p->ev0) (void)hipEventDestroy(p->ev0);
  if (p->ev1) (void)hipEventDestroy(p->ev1);
  delete p;
}

// device half of create: the records, the slot array, the insert pass and its error word; the tiles
int build_device(const char* who, sdpgpu_multi_policy* p, const std::vector<sdp_multi::PolicyRecord>& rec) {
  if (const int rc = no_device(p, who)) return rc;
  MS_TRY(hipGetDevice(&p->device));
  const size_t cap = (size_t)p->mask + 1;
  unsigned long long* d_err = nullptr;
  MS_TRY(hipMalloc((void**)&p->d_rec, rec.size() * sizeof(sdp_multi::PolicyRecord)));
  MS_TRY(hipMalloc((void**)&p->d_slots, cap * 4 + 8));  // (the error word behind the slots, 8-byte aligned: cap is even)
  d_err = reinterpret_cast<unsigned long long*>(p->d_slots + cap);
  MS_TRY(hipMalloc((void**)&p->d_dem, p->pb.dem.size() * sizeof(double2)));
  MS_TRY(hipMalloc((void**)&p->d_thr, p->thr.size() * 8));
  MS_TRY(hipEventCreate(&p->ev0));
  MS_TRY(hipEventCreate(&p->ev1));
  MS_TRY(hipMemcpyAsync(p->d_rec, rec.data(), rec.size() * sizeof(sdp_multi::PolicyRecord), hipMemcpyHostToDevice, p->stream));
  MS_TRY(hipMemcpyAsync(p->d_dem, p->pb.dem.data(), p->pb.dem.size() * sizeof(double2), hipMemcpyHostToDevice, p->stream));
  MS_TRY(hipMemcpyAsync(p->d_thr, p->thr.data(), p->thr.size() * 8, hipMemcpyHostToDevice, p->stream));
  MS_TRY(hipMemsetAsync(p->d_slots, 0xff, cap * 4, p->stream));
  MS_TRY(hipMemsetAsync(d_err, 0, 8, p->stream));
  MS_TRY(hipEventRecord(p->ev0, p->stream));
  hipLaunchKernelGGL(sdp_multi::multi_policy_insert_kernel, dim3((p->rows + 255u) / 256u), dim3(256), 0, p->stream, p->d_rec, p->rows, p->d_slots,
                     p->mask, d_err);
  MS_TRY(hipGetLastError());
  MS_TRY(hipEventRecord(p->ev1, p->stream));
  unsigned long long err = 0;
  MS_TRY(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, p->stream));
  MS_TRY(hipStreamSynchronize(p->stream));
  if (err) {
    const size_t a = (size_t)(err >> 32) - 1, b = (size_t)(err & 0xffffffffull) - 1;
    return mfail(SDPGPU_ERR_ARG, "%s: memo rows %zu and %zu hold the same state (period %d: %g, %g, %g, %g, %g) with different actions (%d, %d) and (%d, %d)",
                 who, a, b, rec[a].period, rec[a].s.i1, rec[a].s.i2, rec[a].s.q1, rec[a].s.q2, rec[a].s.cash, rec[a].a1, rec[a].a2, rec[b].a1,
                 rec[b].a2);
  }
  return SDPGPU_OK;
}

// Everything create checks on the host, then the device half.  pb: the descriptor's problem (its own checks passed).
int create_body(const char* who, sdp_multi::Problem&& pb, const sdpgpu_multi_table* memo, int32_t capacity_log2, sdpgpu_multi_policy** out) {
  if (!out) return mfail(SDPGPU_ERR_ARG, "%s: out is null", who);
  *out = nullptr;
  if (!memo) return mfail(SDPGPU_ERR_ARG, "%s: memo is null", who);
  if (memo->rows < 1) return mfail(SDPGPU_ERR_ARG, "%s: memo->rows = %lld (a solved memo has at least the period-1 state)", who, (long long)memo->rows);
  if (memo->rows > memo->capacity)
    return mfail(SDPGPU_ERR_ARG, "%s: memo->rows = %lld exceeds memo->capacity = %lld (the solve wrote nothing: call it again with larger arrays)", who,
                 (long long)memo->rows, (long long)memo->capacity);
  if (!memo->period || !memo->i1 || !memo->i2 || !memo->q1 || !memo->q2 || !memo->cash || !memo->value || !memo->a1 || !memo->a2)
    return mfail(SDPGPU_ERR_ARG, "%s: a column of memo is null (period, i1, i2, q1, q2, cash, value, a1, a2)", who);
  if (memo->rows >= ((int64_t)1 << 31)) return mfail(SDPGPU_ERR_UNSUPPORTED, "%s: memo->rows = %lld (the table holds 32-bit row indices: below 2^31)", who, (long long)memo->rows);
  const int64_t rows = memo->rows;
  if (capacity_log2 < 0 || capacity_log2 > 31)
    return mfail(SDPGPU_ERR_ARG, "%s: capacity_log2 = %d (0 = the smallest power of two >= 2 x rows, else 1 .. 31 with 2^capacity_log2 > rows)", who, capacity_log2);
  int k = capacity_log2;
  if (k == 0) {
    k = 1;
    while (((int64_t)1 << k) < 2 * rows) ++k;
  } else if (((int64_t)1 << k) <= rows) {
    return mfail(SDPGPU_ERR_ARG, "%s: capacity_log2 = %d: 2^%d = %lld slots do not exceed the %lld rows of memo (a probe needs a free slot to end at)", who,
                 capacity_log2, capacity_log2, (long long)((int64_t)1 << k), (long long)rows);
  }
  const int T = pb.T, qb = pb.P.qb, model = pb.P.model;
  int64_t first = -1;
  for (int64_t r = 0; r < rows; ++r) {
    const int32_t per = memo->period[r];
    if (per < 1 || per > T) return mfail(SDPGPU_ERR_ARG, "%s: memo->period[%lld] = %d outside 1 .. %d", who, (long long)r, per, T);
    const double v[5] = {memo->i1[r], memo->i2[r], memo->q1[r], memo->q2[r], memo->cash[r]};
    const char* names[5] = {"i1", "i2", "q1", "q2", "cash"};
    for (int c = 0; c < 5; ++c)
      if (!std::isfinite(v[c])) return mfail(SDPGPU_ERR_ARG, "%s: memo->%s[%lld] = %g is not finite", who, names[c], (long long)r, v[c]);
    // the action pair as the solve reports it: order indices in [0, Qbound), the XR family's levels (int) x + index
    const int64_t b1 = (int64_t)memo->a1[r] - (model == 2 ? (int64_t)(int)v[0] : 0), b2 = (int64_t)memo->a2[r] - (model == 2 ? (int64_t)(int)v[1] : 0);
    if (b1 < 0 || b1 >= qb || b2 < 0 || b2 >= qb)
      return mfail(SDPGPU_ERR_ARG, "%s: memo->a1 / a2[%lld] = (%d, %d) is no action pair of the descriptor (q_bound %d%s)", who, (long long)r, memo->a1[r],
                   memo->a2[r], qb, model == 2 ? ", levels from (int) i1, (int) i2" : "");
    if (per == 1) {
      if (first >= 0) return mfail(SDPGPU_ERR_ARG, "%s: memo->period: rows %lld and %lld are both of period 1 (a solve has ONE period-1 state)", who, (long long)first, (long long)r);
      first = r;
    }
  }
  if (first < 0) return mfail(SDPGPU_ERR_ARG, "%s: memo->period: no row of period 1 (the descriptor's initial state)", who);
  {
    const sdp_multi::Tuple& s = pb.ini;
    const int64_t r = first;
    if (!(memo->i1[r] == s.i1 && memo->i2[r] == s.i2 && memo->q1[r] == s.q1 && memo->q2[r] == s.q2 && memo->cash[r] == s.cash))
      return mfail(SDPGPU_ERR_ARG, "%s: memo row %lld, the period-1 state (%g, %g, %g, %g, %g), is not the descriptor's initial state (%g, %g, %g, %g, %g): "
                   "the memo must come from a solve of the same descriptor", who, (long long)r, memo->i1[r], memo->i2[r], memo->q1[r], memo->q2[r], memo->cash[r],
                   s.i1, s.i2, s.q1, s.q2, s.cash);
  }
  std::vector<sdp_multi::PolicyRecord> rec((size_t)rows);
  for (int64_t r = 0; r < rows; ++r) {
    sdp_multi::PolicyRecord& q = rec[(size_t)r];
    q.s = sdp_multi::Tuple{memo->i1[r], memo->i2[r], memo->q1[r], memo->q2[r], memo->cash[r]};
    q.period = memo->period[r];
    q.a1 = memo->a1[r];
    q.a2 = memo->a2[r];
    q.pad = 0;
  }
  sdpgpu_multi_policy* p = new sdpgpu_multi_policy();
  p->pb = std::move(pb);
  for (int t = 0; t < T; ++t)
    append_tile_thresholds(std::vector<double>(p->pb.prob.begin() + p->pb.off[(size_t)t], p->pb.prob.begin() + p->pb.off[(size_t)t + 1]), &p->thr);
  p->rows = (uint32_t)rows;
  p->mask = (uint32_t)(((uint64_t)1 << k) - 1u);
  int rc = SDPGPU_ERR_INTERNAL;
  try {
    rc = build_device(who, p, rec);
  } catch (...) {
    release(p);
    throw;
  }
  if (rc) {
    release(p);
    return rc;
  }
  *out = p;
  return SDPGPU_OK;
}

sdp_multi::MultiSimLaunch make_launch(const sdpgpu_multi_policy* p, const double* discount) {
  sdp_multi::MultiSimLaunch L{};
  L.P = p->pb.P;
  L.T = p->pb.T;
  L.ini = p->pb.ini;
  for (int t = 0; t < L.T; ++t) {
    L.overhead[t] = p->pb.overhead[t];
    L.disc[t] = discount ? discount[t] : 1.0;  // NULL = all 1.0: the bits of an explicit array of ones
  }
  for (int t = 0; t <= L.T; ++t) L.off[t] = p->pb.off[(size_t)t];
  return L;
}

sdp_multi::PolicyTable table_of(const sdpgpu_multi_policy* p) { return sdp_multi::PolicyTable{p->d_rec, p->d_slots, p->mask}; }

// the refusals of check_stream_args (sdpgpu_simsample.hip) for an owner whose tiles are always set
int check_stream(sdpgpu_multi_policy* p, const char* who, int32_t n_paths, int32_t mode, uint64_t first_path) {
  if (const int rc = check_n_paths(p, who, n_paths)) return rc;
  if (mode != SDPGPU_SAMPLE_LHS && mode != SDPGPU_SAMPLE_RANDOM)
    return mfail(SDPGPU_ERR_ARG, "%s: mode = %d (SDPGPU_SAMPLE_LHS 0, SDPGPU_SAMPLE_RANDOM 1)", who, mode);
  if (mode == SDPGPU_SAMPLE_LHS && first_path != 0)
    return mfail(SDPGPU_ERR_ARG, "%s: first_path = %llu -- a latin hypercube is one whole of n_paths strata, first_path must be 0", who,
                 (unsigned long long)first_path);
  return SDPGPU_OK;
}

template <int MODEL>
hipError_t launch_sim(int source, dim3 grid, hipStream_t st, const sdp_multi::MultiSimLaunch& L, const sdp::SimStream& R, const sdp_multi::PolicyTable& H,
                      const double* d_thr, const double2* d_dem, const double* g1, const double* g2, double* d_sum, uint8_t* d_valid, double* d_part,
                      unsigned int* d_cnt) {
  if (source == sdp_multi::MS_SOURCE_GIVEN)
    hipLaunchKernelGGL((sdp_multi::multi_sim_kernel<MODEL, sdp_multi::MS_SOURCE_GIVEN>), grid, dim3(256), 0, st, L, R, H, d_thr, d_dem, g1, g2, d_sum, d_valid,
                       d_part, d_cnt);
  else if (source == sdp_multi::MS_SOURCE_RANDOM)
    hipLaunchKernelGGL((sdp_multi::multi_sim_kernel<MODEL, sdp_multi::MS_SOURCE_RANDOM>), grid, dim3(256), 0, st, L, R, H, d_thr, d_dem, g1, g2, d_sum, d_valid,
                       d_part, d_cnt);
  else
    hipLaunchKernelGGL((sdp_multi::multi_sim_kernel<MODEL, sdp_multi::MS_SOURCE_LHS>), grid, dim3(256), 0, st, L, R, H, d_thr, d_dem, g1, g2, d_sum, d_valid,
                       d_part, d_cnt);
  return hipGetLastError();
}

// the two rollouts: d1 / d2 given (source GIVEN) or drawn
int simulate_body(const char* who, sdpgpu_multi_policy* p, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path, const double* d1, const double* d2,
                  bool given, const double* discount, sdpgpu_sim_result* result, double* out_sum, uint8_t* out_valid) {
  if (!p) return mfail(SDPGPU_ERR_ARG, "%s: the policy is null", who);
  if (!result) return mfail(SDPGPU_ERR_ARG, "%s: result is null", who);
  const int T = p->pb.T;
  int rc;
  if (given) {
    rc = check_n_paths(p, who, n_paths);
    if (rc) return rc;
    if (!d1 || !d2) return mfail(SDPGPU_ERR_ARG, "%s: null argument (d1, d2)", who);
    // (element by element, d1 before d2)
    const size_t elems = (size_t)n_paths * T, e1 = first_not_finite(d1, elems), e2 = first_not_finite(d2, elems);
    if (e2 < e1) return not_finite(p, who, "d2", d2, e2, {(size_t)T});
    if (e1 < elems) return not_finite(p, who, "d1", d1, e1, {(size_t)T});
  } else {
    rc = check_stream(p, who, n_paths, mode, first_path);
    if (rc) return rc;
  }
  if (discount && (rc = check_finite(p, who, "discount", discount, (size_t)T))) return rc;
  const int source = given ? sdp_multi::MS_SOURCE_GIVEN : mode == SDPGPU_SAMPLE_RANDOM ? sdp_multi::MS_SOURCE_RANDOM : sdp_multi::MS_SOURCE_LHS;
  const sdp_multi::MultiSimLaunch L = make_launch(p, discount);

  rc = no_device(p, who);
  if (rc) return rc;
  DeviceScope dev;
  MS_TRY(dev.enter(p->device));
  RolloutFrame<sdpgpu_multi_policy> f(p, (uint32_t)n_paths, 1);
  const size_t elems = (size_t)f.n * T;
  const auto p_g1 = f.put(given ? d1 : nullptr, elems), p_g2 = f.put(given ? d2 : nullptr, elems);
  const auto p_valid = f.take<uint8_t>(f.n);
  rc = f.begin();
  if (rc) return rc;
  hipStream_t st = p->stream;
  const sdp::SimStream R = make_stream(n_paths, seed, given ? 0 : first_path);
  const sdp_multi::PolicyTable H = table_of(p);
  const dim3 grid((f.W + 3u) / 4u);
  rc = f.start();
  if (rc) return rc;
  if (L.P.model == 1)
    MS_TRY(launch_sim<1>(source, grid, st, L, R, H, p->d_thr, p->d_dem, f[p_g1], f[p_g2], f.d_sum, f[p_valid], f.d_part, f.d_cnt));
  else if (L.P.model == 2)
    MS_TRY(launch_sim<2>(source, grid, st, L, R, H, p->d_thr, p->d_dem, f[p_g1], f[p_g2], f.d_sum, f[p_valid], f.d_part, f.d_cnt));
  else
    MS_TRY(launch_sim<0>(source, grid, st, L, R, H, p->d_thr, p->d_dem, f[p_g1], f[p_g2], f.d_sum, f[p_valid], f.d_part, f.d_cnt));
  f.download(out_valid, f[p_valid], f.n);
  return f.finish(result, out_sum);
}

}  // namespace

extern "C" {

int sdpgpu_multilead_policy_create(const sdpgpu_multilead* k, const sdpgpu_multi_table* memo, int32_t capacity_log2, sdpgpu_multi_policy** out) {
  ml_error().clear();
  return ml_guard("sdpgpu_multilead_policy_create", [&]() -> int {
    sdp_multi::Problem pb;
    if (const int rc = sdp_multi::multilead_problem(k, &pb)) return rc;
    return create_body("sdpgpu_multilead_policy_create", std::move(pb), memo, capacity_log2, out);
  });
}

int sdpgpu_multicash_policy_create(const sdpgpu_multicash* k, int32_t xr, double deposit_rate, const sdpgpu_multi_table* memo, int32_t capacity_log2,
                                   sdpgpu_multi_policy** out) {
  ml_error().clear();
  return ml_guard("sdpgpu_multicash_policy_create", [&]() -> int {
    const char* who = "sdpgpu_multicash_policy_create";
    if (xr != 0 && xr != 1) return mfail(SDPGPU_ERR_ARG, "%s: xr = %d (0: CashRecursionMulti, 1: CashRecursionMultiXR)", who, xr);
    if (!std::isfinite(deposit_rate)) return mfail(SDPGPU_ERR_ARG, "%s: deposit_rate = %g is not finite", who, deposit_rate);
    sdp_multi::Problem pb;
    if (const int rc = sdp_multi::multicash_problem(k, xr ? 2 : 1, xr ? deposit_rate : 0.0, &pb)) return rc;
    return create_body(who, std::move(pb), memo, capacity_log2, out);
  });
}

void sdpgpu_multi_policy_destroy(sdpgpu_multi_policy* p) {
  try {
    release(p);
  } catch (...) {
  }
}

int sdpgpu_multi_policy_lookup(sdpgpu_multi_policy* p, int64_t n, const int32_t* period, const double* i1, const double* i2, const double* q1,
                               const double* q2, const double* cash, int32_t* a1, int32_t* a2, uint8_t* found) {
  ml_error().clear();
  return ml_guard("sdpgpu_multi_policy_lookup", [&]() -> int {
    const char* who = "sdpgpu_multi_policy_lookup";
    if (!p) return mfail(SDPGPU_ERR_ARG, "%s: the policy is null", who);
    if (n < 0 || n > ((int64_t)1 << 28)) return mfail(SDPGPU_ERR_ARG, "%s: n = %lld (0 .. 2^28)", who, (long long)n);
    if (n == 0) return SDPGPU_OK;
    if (!period || !i1 || !i2 || !q1 || !q2 || !cash || !a1 || !a2 || !found)
      return mfail(SDPGPU_ERR_ARG, "%s: null argument (period, i1, i2, q1, q2, cash, a1, a2, found)", who);
    int rc = no_device(p, who);
    if (rc) return rc;
    DeviceScope dev;
    MS_TRY(dev.enter(p->device));
    const size_t nn = (size_t)n;
    RolloutFrame<sdpgpu_multi_policy> f(p, 0, 0);
    const double* src[5] = {i1, i2, q1, q2, cash};
    Part<double> p_d[5];
    for (int j = 0; j < 5; ++j) p_d[j] = f.put(src[j], nn);
    const auto p_per = f.put(period, nn);
    const auto p_a1 = f.take<int32_t>(nn), p_a2 = f.take<int32_t>(nn);
    const auto p_f = f.take<uint8_t>(nn);
    rc = f.begin();
    if (rc) return rc;
    hipLaunchKernelGGL(sdp_multi::multi_lookup_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, p->stream, table_of(p), n, f[p_per], f[p_d[0]],
                       f[p_d[1]], f[p_d[2]], f[p_d[3]], f[p_d[4]], f[p_a1], f[p_a2], f[p_f]);
    MS_TRY(hipGetLastError());
    f.download(a1, f[p_a1], nn * 4);
    f.download(a2, f[p_a2], nn * 4);
    f.download(found, f[p_f], nn);
    return f.deliver();
  });
}

int sdpgpu_multi_policy_simulate(sdpgpu_multi_policy* p, int32_t n_paths, const double* d1, const double* d2, const double* discount,
                                 sdpgpu_sim_result* result, double* out_sum, uint8_t* out_valid) {
  ml_error().clear();
  return ml_guard("sdpgpu_multi_policy_simulate", [&]() -> int {
    return simulate_body("sdpgpu_multi_policy_simulate", p, n_paths, 0, 0, 0, d1, d2, true, discount, result, out_sum, out_valid);
  });
}

int sdpgpu_multi_policy_simulate_sampled(sdpgpu_multi_policy* p, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path,
                                         const double* discount, sdpgpu_sim_result* result, double* out_sum, uint8_t* out_valid) {
  ml_error().clear();
  return ml_guard("sdpgpu_multi_policy_simulate_sampled", [&]() -> int {
    return simulate_body("sdpgpu_multi_policy_simulate_sampled", p, n_paths, seed, mode, first_path, nullptr, nullptr, false, discount, result, out_sum,
                         out_valid);
  });
}

int sdpgpu_multi_policy_sample(sdpgpu_multi_policy* p, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path, double* out_d1,
                               double* out_d2, double* out_u) {
  ml_error().clear();
  return ml_guard("sdpgpu_multi_policy_sample", [&]() -> int {
    const char* who = "sdpgpu_multi_policy_sample";
    if (!p) return mfail(SDPGPU_ERR_ARG, "%s: the policy is null", who);
    if (!out_d1 || !out_d2) return mfail(SDPGPU_ERR_ARG, "%s: null argument (out_d1, out_d2)", who);
    int rc = check_stream(p, who, n_paths, mode, first_path);
    if (rc) return rc;
    const sdp_multi::MultiSimLaunch L = make_launch(p, nullptr);
    rc = no_device(p, who);
    if (rc) return rc;
    DeviceScope dev;
    MS_TRY(dev.enter(p->device));
    const size_t elems = (size_t)n_paths * p->pb.T;
    RolloutFrame<sdpgpu_multi_policy> f(p, (uint32_t)n_paths, 0);
    const auto p_1 = f.take<double>(elems), p_2 = f.take<double>(elems), p_u = f.take<double>(out_u ? elems : 0);
    rc = f.begin();
    if (rc) return rc;
    const sdp::SimStream R = make_stream(n_paths, seed, first_path);
    const dim3 grid(((unsigned)n_paths + 255u) / 256u);
    if (mode == SDPGPU_SAMPLE_RANDOM)
      hipLaunchKernelGGL((sdp_multi::multi_sample_kernel<sdp_multi::MS_SOURCE_RANDOM>), grid, dim3(256), 0, p->stream, L, R, p->d_thr, p->d_dem, f[p_1],
                         f[p_2], f[p_u]);
    else
      hipLaunchKernelGGL((sdp_multi::multi_sample_kernel<sdp_multi::MS_SOURCE_LHS>), grid, dim3(256), 0, p->stream, L, R, p->d_thr, p->d_dem, f[p_1],
                         f[p_2], f[p_u]);
    MS_TRY(hipGetLastError());
    f.download(out_d1, f[p_1], elems * 8);
    f.download(out_d2, f[p_2], elems * 8);
    f.download(out_u, f[p_u], elems * 8);
    return f.deliver();
  });
}

}  // extern "C"
