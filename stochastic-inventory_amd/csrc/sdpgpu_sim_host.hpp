// sdpgpu_sim_host.hpp -- what the host code of the simulation translation units shares.  By every rollout owner (sdpgpu_batch.hip:
// an sdpgpu_batch; the handle rollouts sdpgpu_simsample.hip, sdpgpu_cashrulesim.hip, sdpgpu_xrsim.hip, sdpgpu_staffsim.hip,
// sdpgpu_customsim.hip: an sdpgpu_handle; sdpgpu_multisim.hip: an sdpgpu_multi_policy; sdpgpu_staffbatch.hip: the BatchFrame of a
// staff batch (sdpgpu_batch_frame.hpp), whose pairs (instance, rule) are the frame's rules): the exception barrier, the device scope, the path-count refusals, the stream
// record, the threshold table of a pmf tile and the grow-only scratch block.  By the handle, staff-batch
// and policy rollouts: RolloutFrame, the ONE host frame of a rollout call -- the carving of the scratch block with typed access
// and uploads, the two timing events, the zeroed counters, the fixed-order reduction of every rule, the downloads and the
// sdpgpu_sim_result records -- so that an entry point supplies its validation, its period records and its launch.  By the handle
// rollouts: the sampler records with their arenas (HostSamplers), the discount weights, the flat finiteness check, the
// descriptor's inventory points, the policy-table precondition and the parameter block without a layout.  By handle and batch:
// the sampler specs an owner keeps.  The templates take the OWNER and report through its own error sink.  Internal, header only.
#pragma once
#include "sdpgpu_internal.hpp"
#include "sdp_sampler.hpp"

#include <initializer_list>

struct sdpgpu_batch;
namespace sdp {
struct FitPair;  // sdp_fit_pair.hpp
}

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

// sdpgpu_simsample.hip: the refusals of a call's stream arguments (n_paths, mode, first_path, a period without a tile or spec),
// and the handle's sampler records with their two arenas
int check_stream_args(sdpgpu_handle* h, const char* who, int32_t n_paths, int32_t mode, uint64_t first_path);
struct HostSamplers {
  std::vector<sdp::SimSampler> rec;
  std::vector<double> thr, val;
};
void build_samplers(const sdpgpu_handle* h, HostSamplers* s);

// sdpgpu_simsample.hip: the parameter block of period index t WITHOUT a layout, for rollouts that carry the state as doubles and
// read no table (nx = the descriptor's inventory points: descriptor_nx)
sdp::DevParams rule_params(const sdpgpu_handle* h, int t, int64_t nx);

// the discount weights of a call
inline std::vector<double> discounts_or_ones(const double* discount, int T) {
  std::vector<double> disc((size_t)T, 1.0);  // NULL = all 1.0: the bits of an explicit array of ones
  if (discount) disc.assign(discount, discount + T);
  return disc;
}

// The finiteness refusal of a flat array: element e of `name`, whose trailing dimensions are `inner`, reported with its indices
// ("rule[1][0][3] = inf is not finite").  first_not_finite: the element, or count when every one is finite.
inline size_t first_not_finite(const double* a, size_t count) {
  size_t e = 0;
  while (e < count && std::isfinite(a[e])) ++e;
  return e;
}
template <class Owner>
int not_finite(Owner* o, const char* who, const char* name, const double* a, size_t e, std::initializer_list<size_t> inner) {
  size_t below = 1;
  for (const size_t d : inner) below *= d;
  std::string idx = "[" + std::to_string(e / below) + "]";
  for (const size_t d : inner) {
    below /= d;
    idx += "[" + std::to_string(e / below % d) + "]";
  }
  return sim_fail(o, SDPGPU_ERR_ARG, "%s: %s%s = %g is not finite", who, name, idx.c_str(), a[e]);
}
template <class Owner>
int check_finite(Owner* o, const char* who, const char* name, const double* a, size_t count, std::initializer_list<size_t> inner = {}) {
  const size_t e = first_not_finite(a, count);
  return e == count ? SDPGPU_OK : not_finite(o, who, name, a, e, inner);
}

// NX of a rule's tables and parameter blocks: the descriptor's inventory points, as layout() counts them (below 2^31: validated
// at create)
inline int descriptor_nx(sdpgpu_handle* h, const char* who, int64_t* nx) {
  const sdpgpu_desc& d = h->d;
  *nx = (int64_t)((d.max_inventory - d.min_inventory) / d.step) + 1;
  if (*nx < 1 || *nx >= 2147483647LL) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: the descriptor's inventory axis has %lld points", who, (long long)*nx);
  return SDPGPU_OK;
}

// the precondition of a rollout that reads the policy tables; every caller keeps its own wording (prefix, and what follows the
// first sentence)
inline int check_solved(sdpgpu_handle* h, const char* who, const char* prefix = "", const char* unsolved_tail = "") {
  if (!h->allocated) return fail(h, SDPGPU_ERR_STATE, "%s: %snothing has been solved%s", who, prefix, unsolved_tail);
  for (int t = 0; t < h->T; ++t)
    if (!h->policy_done[(size_t)t]) return fail(h, SDPGPU_ERR_STATE, "%s: %speriod %d has not been computed", who, prefix, t + 1);
  return SDPGPU_OK;
}

// ---- sdpgpu_staffbatch.hip -------------------------------------------------------------------------------
// A batch of STAFF instances in the separable mode (pool of level tables, groups per (period, table), two launches per period
// for all instances: sdp_staff_batch.hpp): what the sdpgpu_batch_* entry points of sdpgpu_batch.hip forward to when instance 0
// is of that family.  It reports through `frame`, the BatchFrame of the sdpgpu_batch that holds it (sdpgpu_batch_frame.hpp), which
// also carries its stream, profiling switch and period times; the create-time refusals go to `why`.
struct StaffBatch;
struct BatchFrame;
int staff_batch_new(const sdpgpu_desc* descs, int32_t n, BatchFrame* frame, StaffBatch** out, std::string* why);
void staff_batch_delete(StaffBatch* s);
int staff_batch_add_table(StaffBatch* s, const double* prob, const int32_t* row_len, int32_t n_rows, int32_t row_stride,
                          int32_t* out_table);
int staff_batch_use_table(StaffBatch* s, int32_t instance, int32_t t, int32_t table);
int staff_batch_set_min_staff(StaffBatch* s, int32_t instance, int32_t t, double min_staff);
int staff_batch_grid(const StaffBatch* s, int32_t instance, int32_t period, double* x_lo, int64_t* nx);
int64_t staff_batch_num_states(const StaffBatch* s, int32_t instance);
int32_t staff_batch_num_actions(const StaffBatch* s, int32_t instance);
int staff_batch_plan(StaffBatch* s, int32_t period, sdpgpu_batch_staff_plan* out);
int staff_batch_solve(StaffBatch* s, int32_t sync);
bool staff_batch_allocated(const StaffBatch* s);  // the device tables exist: a synchronise has something to wait for
int staff_batch_values(StaffBatch* s, int32_t instance, int32_t period, double* out, int64_t n);
int staff_batch_policy(StaffBatch* s, int32_t instance, int32_t period, int32_t* out, int64_t n);
int staff_batch_initial(StaffBatch* s, double* out_value, int32_t* out_action_index);
int staff_batch_stats(StaffBatch* s, sdpgpu_batch_stats* out);
// steps 2-5 of WorkforceTesting.main's loop body for the whole batch ("Workforce batch: fit and rollout")
int staff_batch_reachable(StaffBatch* s, int32_t instance, int32_t period, int64_t* lo, int64_t* hi);
int staff_batch_fit_ss(StaffBatch* s, double max_order_quantity, double* out);
int staff_batch_simulate(StaffBatch* s, const int32_t* sample_nums, uint64_t seed, double ini_x, const double* ss,
                         int32_t n_rules, sdpgpu_sim_result* results, double* out_sum, uint8_t* out_valid, int32_t* out_demand);

// sdpgpu_batch.hip: one launch of batch_fit_ss_kernel<1> (sdp_fitss.hpp) at step 1 over the slices pairs[i * T + t] of a policy
// arena, out[(i * T + t) * 2 + {0, 1}] -- for the staff batch, whose unit fills the slices and owns the buffers
hipError_t launch_fit_singles(hipStream_t st, const sdp::FitPair* d_pairs, int n_pairs, int T, const int32_t* d_policy, double* d_out);

// sdpgpu_batch.hip: CheckKConvexity (sdp_structure.hpp: key fill, convexity_kernel over convexity_tasks, finish) on n_rows rows
// that already lie on the device, all of one kind -- for the staff units, whose rows are V_t or G_t of a handle or of every
// instance of a staff batch.  The launches go to `st` behind whatever wrote the rows; the call returns once the structs are in
// `out`, written only on success.  A failure leaves its reason in *why.
constexpr int32_t kConvexityMaxPoints = 8192;  // sdp::kConvexityMaxRow, for the callers' refusals before any device call
struct ConvexitySpec {
  const double* g;  // device
  double K;
  int32_t n, capacity;
};
int convexity_on_device(hipStream_t st, int32_t kind, const ConvexitySpec* specs, int32_t n_rows, sdpgpu_convexity* out, std::string* why);

// ---- sdpgpu_staffstruct.hip --------------------------------------------------------------------------------
// the G(y) rows of the STAFF family (sdp_staff_structure.hpp) and the checks on them, for a handle; what a staff batch shares
// with it: the one launch of staff_gy_kernel over `n_rows` row records (blocks of 64 levels, highest level first), which
// uploads the records and the block table into `d_rows` / `d_blocks` first
}  // namespace sdpgpu_detail
namespace sdp {
struct StaffGyRow;
struct StaffGyBlock;
}  // namespace sdp
namespace sdpgpu_detail {
int64_t staff_gy_blocks(const sdp::StaffGyRow* rows, int32_t n_rows, std::vector<sdp::StaffGyBlock>* blocks);
hipError_t launch_staff_gy(hipStream_t st, const sdp::StaffGyRow* rows, int32_t n_rows, const std::vector<sdp::StaffGyBlock>& blocks,
                           sdp::StaffGyRow* d_rows, sdp::StaffGyBlock* d_blocks);
int staff_batch_gy(StaffBatch* s, int32_t instance, int32_t period, int32_t y_lo, int32_t n, double* out);
int staff_batch_check_convexity(StaffBatch* s, int32_t kind, int32_t source, int32_t period, const int32_t* lo, const int32_t* hi, const double* K,
                                const int32_t* capacity, sdpgpu_convexity* out);

// ---- the host frame of a rollout --------------------------------------------------------------------------
// offsets of the scratch block, every part aligned to 16 bytes
struct Carve {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at += (bytes + 15) / 16 * 16;
    return o;
  }
};

// `count` elements of T at byte offset `off` of the scratch block
template <class T>
struct Part {
  size_t off = 0, count = 0;
};

// the two timing events of an owner: a handle creates its pair at its first rollout (sdpgpu_destroy releases it), a policy
// created its pair with its table (sim_events of sdpgpu_multisim.hip)
inline hipError_t sim_events(sdpgpu_handle* h, hipEvent_t* ev0, hipEvent_t* ev1) {
  hipError_t e = hipSuccess;
  if (!h->sim_ev0 && (e = hipEventCreate(&h->sim_ev0)) != hipSuccess) return e;
  if (!h->sim_ev1 && (e = hipEventCreate(&h->sim_ev1)) != hipSuccess) return e;
  *ev0 = h->sim_ev0;
  *ev1 = h->sim_ev1;
  return hipSuccess;
}

#define SIM_TRY(o, expr)                                                                                \
  do {                                                                                                  \
    const hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) return sim_fail(o, SDPGPU_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// One call's use of the owner's scratch block and stream, in this order:
//   take / put / put_samplers   reserve the caller's parts (put: with the host range that begin() uploads into it)
//   begin()                     the block (sim_scratch), the events, the uploads, the counters zeroed
//   f[part]                     the typed device pointer of a part (null for an empty part)
//   start()                     ev0; the caller launches its kernels, which leave sums in d_sum, wave partials in d_part and
//                               the valid paths of rule r in d_cnt[2 r] (d_cnt[2 r + 1]: a second counter of the caller's)
//   download(host, dev, bytes)  one more output for finish / deliver to bring back (skipped when host is null)
//   finish(results, out_sum)    mean and m2 of every rule (launch_sim_moments), ev1, the downloads, the synchronise, the results
// The frame's own parts come FIRST in the block, so the counters (one integer atomic per wave) share their 128-byte line with the
// results and the first partials only, never with the tail of a caller's read-only table: behind the sampler's value arena
// they cost sdpgpu_simulate_sampled a fifth of its time at 100 000 paths (profiles/rollout_frame_rows.json).
// n_rules == 0 is a call without sums (the draws alone, a look-up): no reduction parts, no events; it ends with deliver().  An
// early return leaves the owner as it is: the block is grow-only and nothing is freed on an error.
template <class Owner>
class RolloutFrame {
 public:
  const uint32_t n, W;  // paths (or leaves) of a rule, and their waves: ceil(n / 64)
  const size_t nr;      // rules
  unsigned int* d_cnt = nullptr;
  double *d_res = nullptr, *d_part = nullptr, *d_sum = nullptr;
  std::vector<unsigned int> cnt;  // the counters as finish() downloaded them

  RolloutFrame(Owner* owner, uint32_t n_paths, size_t n_rules) : n(n_paths), W((n_paths + 63u) / 64u), nr(n_rules), o(owner) {
    p_cnt = take<unsigned int>(2 * nr);
    p_res = take<double>(2 * nr);
    p_part = take<double>(nr * W);
    p_sum = take<double>(nr * n);
  }

  template <class T>
  Part<T> take(size_t count) {
    return Part<T>{c.take(count * sizeof(T)), count};
  }
  // a part of max(count, reserve) elements whose first `count` are the host range (none where host is null)
  template <class T>
  Part<T> put(const T* host, size_t count, size_t reserve = 0) {
    if (!host) count = 0;
    const Part<T> p = take<T>(std::max(count, reserve));
    if (count) uploads.push_back(Upload{host, p.off, count * sizeof(T)});
    return p;
  }
  struct SamplerParts {
    Part<sdp::SimSampler> rec;
    Part<double> thr, val;
  };
  // the two arenas of build_samplers and, for a kernel that does not carry them in its period records, the records
  SamplerParts put_samplers(const HostSamplers& s, bool with_records) {
    SamplerParts p;
    p.rec = put(s.rec.data(), with_records ? s.rec.size() : 0);
    p.thr = put(s.thr.data(), s.thr.size());
    p.val = put(s.val.data(), s.val.size());
    return p;
  }

  int begin() {
    if (const int rc = sim_scratch(o, c.at)) return rc;
    base = o->d_sim_scratch;
    if (nr) SIM_TRY(o, sim_events(o, &ev0, &ev1));
    for (const Upload& u : uploads) SIM_TRY(o, hipMemcpyAsync(base + u.off, u.host, u.bytes, hipMemcpyHostToDevice, o->stream));
    d_cnt = (*this)[p_cnt];
    d_res = (*this)[p_res];
    d_part = (*this)[p_part];
    d_sum = (*this)[p_sum];
    if (nr) SIM_TRY(o, hipMemsetAsync(d_cnt, 0, 2 * nr * sizeof(unsigned int), o->stream));
    return SDPGPU_OK;
  }
  template <class T>
  T* operator[](Part<T> p) const {
    return p.count ? reinterpret_cast<T*>(base + p.off) : nullptr;
  }

  int start() {
    SIM_TRY(o, hipEventRecord(ev0, o->stream));
    return SDPGPU_OK;
  }
  void download(void* host, const void* dev, size_t bytes) {
    if (host) downloads.push_back(Download{host, dev, bytes});
  }
  // results == nullptr: no moments (the caller formed no partials), the outputs alone
  int finish(sdpgpu_sim_result* results, double* out_sum) {
    hipStream_t st = o->stream;
    // per rule: mean = (partials in the fixed order) / n; m2 = a second pass over the sums
    for (size_t r = 0; results && r < nr; ++r)
      SIM_TRY(o, launch_sim_moments(st, d_sum + r * n, n, d_part + r * W, d_cnt + 2 * r, d_res + 2 * r));
    SIM_TRY(o, hipEventRecord(ev1, st));
    std::vector<double> res(2 * nr, 0.0);
    cnt.assign(2 * nr, 0u);
    if (results) {
      SIM_TRY(o, hipMemcpyAsync(res.data(), d_res, 2 * nr * 8, hipMemcpyDeviceToHost, st));
      SIM_TRY(o, hipMemcpyAsync(cnt.data(), d_cnt, 2 * nr * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    }
    if (out_sum) SIM_TRY(o, hipMemcpyAsync(out_sum, d_sum, nr * n * 8, hipMemcpyDeviceToHost, st));
    if (const int rc = deliver()) return rc;
    if (!results) return SDPGPU_OK;
    float ms = 0;
    SIM_TRY(o, hipEventElapsedTime(&ms, ev0, ev1));
    for (size_t r = 0; r < nr; ++r) {
      results[r].n_paths = (int32_t)n;
      results[r].n_valid = (int32_t)cnt[2 * r];
      results[r].n_lost = 0;
      results[r].reserved = 0;
      results[r].mean = res[2 * r];
      results[r].m2 = res[2 * r + 1];
      results[r].kernel_ms = ms;
    }
    return SDPGPU_OK;
  }
  // the registered downloads and the synchronise
  int deliver() {
    for (const Download& d : downloads) SIM_TRY(o, hipMemcpyAsync(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost, o->stream));
    SIM_TRY(o, hipStreamSynchronize(o->stream));
    return SDPGPU_OK;
  }

 private:
  struct Upload {
    const void* host;
    size_t off, bytes;
  };
  struct Download {
    void* host;
    const void* dev;
    size_t bytes;
  };
  Owner* o;
  Carve c;
  Part<unsigned int> p_cnt;
  Part<double> p_res, p_part, p_sum;
  std::vector<Upload> uploads;
  std::vector<Download> downloads;
  char* base = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

}  // namespace sdpgpu_detail
