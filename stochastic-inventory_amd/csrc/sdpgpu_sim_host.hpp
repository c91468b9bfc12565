// sdpgpu_sim_host.hpp -- what the host code of the two simulation translation units shares (sdpgpu_batch.hip: an sdpgpu_batch;
// sdpgpu_simsample.hip: an sdpgpu_handle): the exception barrier, the device scope, the path-count refusals, the stream record,
// the threshold table of a pmf tile, the sampler specs an owner keeps, and the grow-only scratch block with its carving.  The
// templates take the OWNER (handle or batch) and report through its own error sink.  Internal, header only.
#pragma once
#include "sdpgpu_internal.hpp"
#include "sdp_sampler.hpp"

struct sdpgpu_batch;

namespace sdpgpu_detail {

int bfail(sdpgpu_batch* b, int code, const char* fmt, ...);  // sdpgpu_batch.hip (b == nullptr: the create error)

// one name for the two error sinks
template <class... A>
int sim_fail(sdpgpu_handle* h, int code, const char* fmt, A... a) { return fail(h, code, fmt, a...); }
template <class... A>
int sim_fail(sdpgpu_batch* b, int code, const char* fmt, A... a) { return bfail(b, code, fmt, a...); }

// No C++ exception crosses the C ABI: the same barrier as the two-product entry points (sdpgpu_sparse.hip).
template <class Owner, class F>
int guarded(Owner* o, const char* who, F&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return sim_fail(o, SDPGPU_ERR_ALLOC, "%s: host allocation failed (std::bad_alloc)", who);
  } catch (const std::exception& e) {
    return sim_fail(o, SDPGPU_ERR_INTERNAL, "%s: internal error: %s", who, e.what());
  } catch (...) {
    return sim_fail(o, SDPGPU_ERR_INTERNAL, "%s: internal error (unknown exception)", who);
  }
}

// The owner's device for the length of a call; the caller's current device comes back at the end.
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  hipError_t enter(int device) {
    if (device < 0) return hipSuccess;
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return e;
    if (prev == device) return hipSuccess;
    e = hipSetDevice(device);
    switched = e == hipSuccess;
    return e;
  }
  ~DeviceScope() {
    if (switched) (void)hipSetDevice(prev);
  }
};

// `who` == nullptr: the bare sentence (a batch allocating its tables)
template <class Owner>
int no_device(Owner* o, const char* who) {
  int ndev = 0;
  const hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1)
    return sim_fail(o, SDPGPU_ERR_DEVICE, "%s%sno HIP device available (%s); this library has no CPU path", who ? who : "", who ? ": " : "",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  return SDPGPU_OK;
}

constexpr int32_t kSimMaxPaths = 1 << 24;

template <class Owner>
int check_n_paths(Owner* o, const char* who, int32_t n_paths) {
  if (n_paths <= 0) return sim_fail(o, SDPGPU_ERR_ARG, "%s: n_paths = %d (1 .. %d)", who, n_paths, kSimMaxPaths);
  if (n_paths > kSimMaxPaths) return sim_fail(o, SDPGPU_ERR_UNSUPPORTED, "%s: n_paths = %d exceeds %d", who, n_paths, kSimMaxPaths);
  return SDPGPU_OK;
}

inline sdp::SimStream make_stream(int32_t n_paths, uint64_t seed, uint64_t first_path) {
  sdp::SimStream R{};
  R.first_path = first_path;
  R.n_paths = (uint32_t)n_paths;
  R.seed_lo = (uint32_t)(seed & 0xffffffffu);
  R.seed_hi = (uint32_t)(seed >> 32);
  int hb = 1;
  while (((int64_t)1 << (2 * hb)) < (int64_t)n_paths) ++hb;
  R.half_bits = hb;
  return R;
}

// threshold table of a pmf tile: the running fp64 sum of its probabilities in ascending order, the last threshold +infinity
inline void append_tile_thresholds(const std::vector<double>& p, std::vector<double>* thr) {
  double s = 0.0;
  for (size_t j = 0; j < p.size(); ++j) {
    s += p[j];
    thr->push_back(j + 1 == p.size() ? HUGE_VAL : s);
  }
}

// The distribution specs an owner was given (sdpgpu_set_sampler, sdpgpu_batch_set_sampler), by slot: the threshold table of a
// slot that has one; every other slot draws from its pmf tile.  Empty until resized: no slot has a spec.
struct SamplerSpecs {
  std::vector<char> is_set;
  std::vector<int32_t> k_lo, strict;
  std::vector<std::vector<double>> thr;
  void resize(size_t n) {
    is_set.assign(n, 0);
    k_lo.assign(n, 0);
    strict.assign(n, 0);
    thr.assign(n, {});
  }
  bool has(size_t k) const { return k < is_set.size() && is_set[k]; }
  void clear(size_t k) {
    is_set[k] = 0;
    thr[k].clear();
  }
  // the table of `spec` into slot k; a failure leaves the slot as it was, and its reason in *why
  int set(size_t k, const sdpgpu_dist_spec& spec, std::string* why) {
    std::vector<double> t;
    int32_t lo = 0, st = 0;
    const int rc = sample_table_build(spec, &lo, &t, &st, why);
    if (rc) return rc;
    thr[k].swap(t);
    k_lo[k] = lo;
    strict[k] = st;
    is_set[k] = 1;
    return SDPGPU_OK;
  }
  // slot k's record, its thresholds appended to the arena (demand = k_lo + q)
  sdp::SimSampler append(size_t k, std::vector<double>* arena) const {
    sdp::SimSampler S{};
    S.off = (int64_t)arena->size();
    S.k_lo = k_lo[k];
    S.strict = strict[k];
    S.m = (int32_t)thr[k].size();
    S.val_off = -1;
    arena->insert(arena->end(), thr[k].begin(), thr[k].end());
    return S;
  }
};

// The owner's ONE scratch block (d_sim_scratch, sim_scratch_bytes, stream): grow-only, replaced once its stream has drained.
template <class Owner>
int sim_scratch(Owner* o, size_t bytes) {
  if (bytes <= o->sim_scratch_bytes && o->d_sim_scratch) return SDPGPU_OK;
  hipError_t e = hipSuccess;
  if (o->d_sim_scratch) {
    if ((e = hipStreamSynchronize(o->stream)) != hipSuccess) return sim_fail(o, SDPGPU_ERR_DEVICE, "sim_scratch: hipStreamSynchronize: %s", hipGetErrorString(e));
    (void)hipFree(o->d_sim_scratch);
    o->d_sim_scratch = nullptr;
    o->sim_scratch_bytes = 0;
  }
  if ((e = hipMalloc((void**)&o->d_sim_scratch, bytes)) != hipSuccess) return sim_fail(o, SDPGPU_ERR_DEVICE, "sim_scratch: hipMalloc: %s", hipGetErrorString(e));
  o->sim_scratch_bytes = bytes;
  return SDPGPU_OK;
}

// sdpgpu_simsample.hip: the fixed-order reduction of a rollout (sim_reduce_kernel, sim_dev2_kernel of sdp_sim_sampled.hpp) on
// n device-resident sums and their W = ceil(n / 64) wave partials: d_res[0] = mean, d_res[1] = m2, both NaN when d_cnt[0] < n
hipError_t launch_sim_moments(hipStream_t st, const double* d_sum, uint32_t n, double* d_part, const unsigned int* d_cnt, double* d_res);

// sdpgpu_simsample.hip, shared with the user-functor rollouts (sdpgpu_customsim.hip): the draws of sdpgpu_sample_demands into a
// device buffer, d_dem[p * T + t] (d_u: the uniforms, or null)
hipError_t launch_sim_draw(hipStream_t st, int32_t mode, const sdp::SimStream& R, int T, const sdp::SimSampler* d_samp, const double* d_thr,
                           const double* d_val, double* d_dem, double* d_u);

// sdpgpu_simsample.hip, shared with the cash rule rollout (sdpgpu_cashrulesim.hip): the refusals of a call's stream arguments
// (n_paths, mode, first_path, a period without a tile or spec), and the handle's sampler records with their two arenas
int check_stream_args(sdpgpu_handle* h, const char* who, int32_t n_paths, int32_t mode, uint64_t first_path);
void build_samplers(const sdpgpu_handle* h, std::vector<sdp::SimSampler>* rec, std::vector<double>* thr, std::vector<double>* val);

// sdpgpu_cashrulesim.hip, shared with the (x, R) rollout (sdpgpu_xrsim.hip): the parameter block of period index t WITHOUT a
// layout, for rollouts that carry the state as doubles and read no table (nx = the descriptor's inventory points)
sdp::DevParams rule_params(const sdpgpu_handle* h, int t, int64_t nx);

// ---- sdpgpu_staffbatch.hip -------------------------------------------------------------------------------
// A batch of STAFF instances in the separable mode (pool of level tables, groups per (period, table), two launches per period
// for all instances: sdp_staff_batch.hpp): what the sdpgpu_batch_* entry points of sdpgpu_batch.hip forward to when instance 0
// is of that family.  `err` is the batch's error sink (staff_batch_new: the create error).
struct StaffBatch;
int staff_batch_new(const sdpgpu_desc* descs, int32_t n, StaffBatch** out, std::string* why);
void staff_batch_delete(StaffBatch* s);
int staff_batch_add_table(StaffBatch* s, std::string* err, const double* prob, const int32_t* row_len, int32_t n_rows, int32_t row_stride,
                          int32_t* out_table);
int staff_batch_use_table(StaffBatch* s, std::string* err, int32_t instance, int32_t t, int32_t table);
int staff_batch_set_min_staff(StaffBatch* s, std::string* err, int32_t instance, int32_t t, double min_staff);
int staff_batch_grid(const StaffBatch* s, std::string* err, int32_t instance, int32_t period, double* x_lo, int64_t* nx);
int64_t staff_batch_num_states(const StaffBatch* s, int32_t instance);
int32_t staff_batch_num_actions(const StaffBatch* s, int32_t instance);
int staff_batch_plan(StaffBatch* s, std::string* err, int32_t period, sdpgpu_batch_staff_plan* out);
int staff_batch_set_stream(StaffBatch* s, std::string* err, void* hip_stream);
int staff_batch_set_profiling(StaffBatch* s, int32_t on);
int staff_batch_solve(StaffBatch* s, std::string* err, int32_t sync);
int staff_batch_synchronize(StaffBatch* s, std::string* err);
int staff_batch_values(StaffBatch* s, std::string* err, int32_t instance, int32_t period, double* out, int64_t n);
int staff_batch_policy(StaffBatch* s, std::string* err, int32_t instance, int32_t period, int32_t* out, int64_t n);
int staff_batch_initial(StaffBatch* s, std::string* err, double* out_value, int32_t* out_action_index);
int staff_batch_stats(StaffBatch* s, std::string* err, sdpgpu_batch_stats* out);
double staff_batch_period_ms(StaffBatch* s, std::string* err, int32_t period);

// offsets of the scratch block, every part aligned to 16 bytes
struct Carve {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at += (bytes + 15) / 16 * 16;
    return o;
  }
};

}  // namespace sdpgpu_detail
