// sdpgpu_batch.hip -- a BATCH of backorder-family (F1) instances (include/sdpgpu.h, sdpgpu_batch_*, sdpgpu_fit_*): the parameter sweeps of
// the reference's *Testing mains -- of one grid shape (capacitated.CLSPTesting.main: 540 instances of one grid;
// sdpgpu_batch_create) or with inventory bounds and an order limit of their own (capacitated.fitss.ThreeLevelFitsSTest.main:
// 810 instances with 27 order limits; sdpgpu_batch_create_ragged).  Period t of ALL instances runs in one launch of
// window_f1_batch_kernel (sdp_batch.hpp); this file holds the validation, the host layout with its prefix-sum arenas, the
// plan of a period, the task table, the launcher and the entry points.  Separate from sdpgpu_handle on purpose: a batch has no
// slabs, no exchange, no user functors -- and the handle does not grow.  What a batch of either family needs around a solve --
// error text, stream, the timing events of a sweep, read-outs, the rollouts' scratch block -- is its BatchFrame
// (sdpgpu_batch_frame.hpp).
// A batch whose instance 0 is of the STAFF family (the workforce sweep in the separable mode) lives in sdpgpu_staffbatch.hip:
// sdpgpu_batch_create makes it there, and every entry point below forwards to it or refuses by name.
#include "sdpgpu_batch_frame.hpp"
#include "sdp_batch.hpp"
#include "sdp_batch_sim.hpp"
#include "sdp_fitss.hpp"
#include "sdp_structure.hpp"

namespace sdpgpu_detail {
int validate(const sdpgpu_desc& d);                 // sdpgpu.hip
int32_t full_action_count(const sdpgpu_desc& d);    // sdpgpu.hip
}  // namespace sdpgpu_detail

// (R, S, chunks) of one period for the whole batch
struct BatchPlan {
  int R = 0, S = 0, chunk_blocks = 0, span_max = 0, p_slots_max = 0;
  int n_chunks = 1, min_chunks = 1;  // largest / smallest chunk count of an instance: ceil(its R-blocks / chunk_blocks)
  int64_t n_tasks = 0;               // sum over instances of tiles x chunks
  size_t smem = 0;
};

struct sdpgpu_batch {
  sdpgpu_detail::BatchFrame f;     // error text, stream, events, staging and scratch blocks: of a staff batch too
  std::vector<sdpgpu_desc> d;
  int32_t N = 0, T = 0;
  // instance 0 of the STAFF family: the whole state of the batch lives in sdpgpu_staffbatch.hip, every entry point below forwards
  // to it or refuses by name; N, T and the frame are the only other members in use
  sdpgpu_detail::StaffBatch* staff = nullptr;
  bool ragged = false;             // sdpgpu_batch_create_ragged: bounds and order limit are the instance's own
  std::vector<int32_t> nxs, As;    // [i]: states and actions of instance i
  std::vector<size_t> val_base, pol_base;  // [i]: prefix sums -- instance i's value rows / policy (and key) rows
  int64_t sum_nx = 0;
  std::vector<double> d0;                  // [i * T + t]: first demand value
  std::vector<std::vector<double>> pmf_p;  // [i * T + t]
  std::vector<char> pmf_set;
  int win_r = 0, win_s = 0, win_nch = 0;   // SDPGPU_WIN_R / _S / _NCH, read at create time as for a handle
  bool laid_out = false, allocated = false, solved = false;
  std::vector<BatchPlan> plan;             // [t]
  std::vector<sdp::BatchInst> inst;        // [t * N + rank], longest demand first
  std::vector<size_t> pmf_off;             // [i * T + t]
  std::vector<sdp::BatchTask> tasks;       // the periods' task tables, one after the other
  std::vector<size_t> task_off;            // [t]: first task of period t
  bool any_chunked = false;
  size_t values_elems = 0, policy_elems = 0, pmf_elems = 0, key_elems = 0, chunk_elems = 0;
  int64_t total_final = 0;                 // states the finalize pass resolves
  std::vector<sdp::FinalizeJob> jobs;
  int64_t cells = 0;
  // device
  double* d_values = nullptr;
  int32_t* d_policy = nullptr;
  double* d_pmf = nullptr;
  sdp::BatchInst* d_inst = nullptr;
  sdp::BatchTask* d_tasks = nullptr;
  unsigned long long* d_keys = nullptr;
  double* d_chunk_val = nullptr;
  int32_t* d_chunk_idx = nullptr;
  sdp::FinalizeJob* d_jobs = nullptr;
  int64_t* d_ini_off = nullptr;  // [2 N]: value and policy offsets of every instance's period-1 initial state
  int32_t period_launches = 0, finalize_launches = 0, periods_run = 0;
  // ---- simulation (sdp_batch_sim.hpp) ----
  sdpgpu_detail::SamplerSpecs samp;  // [i * T + t]: a distribution spec, or none = the pmf tile
  bool samp_dirty = true;
  sdp::SimSampler* d_samp = nullptr;
  double* d_thr = nullptr;
  sdp::SimInst* d_sim_inst = nullptr;  // [i], for the table rule and the level rules alike
  bool sim_timed = false;  // (the frame's scratch block: start states, wave partials, means, path sums, an explicit rule, demands)
  // ---- (s, S) level rules (sdp_fitss.hpp) ----
  sdp::FitPair* d_fit_pairs = nullptr;  // [i * T + t]: the reachable slice of every (instance, period)
  double* d_fit = nullptr;              // the last device fit, N x T x 2*levels (sized for three levels)
  // ---- structure checks (sdp_structure.hpp) ----
  double* d_gy = nullptr;               // the G rows, laid out as the policy rows; made on first request after a solve
  sdp::GyPair* d_gy_pairs = nullptr;    // [i * T + t]
  bool gy_valid = false;
};

int sdpgpu_detail::bfail(sdpgpu_batch* b, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfail_to(b ? &b->f.err : &g_create_error, code, fmt, ap);
  va_end(ap);
  return code;
}

namespace {

using namespace sdpgpu_detail;

// a call without a meaning on a STAFF batch (and the staff calls on a backorder batch): refused by name before anything else
#define STAFF_REFUSE(b, who)                                                                                                        \
  if ((b)->staff)                                                                                                                   \
  return bfail(b, SDPGPU_ERR_UNSUPPORTED, who ": not available on a batch of the staff family (SDPGPU_FAMILY_STAFF), which solves, reads " \
                                              "its tables and reports its plan (sdpgpu_batch_staff_plan_period)")
#define STAFF_ONLY(b, who)                                                                                                          \
  if (!(b)->staff)                                                                                                                  \
  return bfail(b, SDPGPU_ERR_UNSUPPORTED, who ": the batch is of the backorder family (SDPGPU_FAMILY_BACKORDER); this call belongs to a " \
                                              "batch of the staff family")
#define STAFF_FORWARD(b, who, call) \
  if ((b)->staff) return guarded(b, who, [&]() -> int { return call; })

#define BHIP_TRY(b, expr) SIM_TRY(b, expr)  // (reports through bfail: sim_fail of an sdpgpu_batch)

inline int rup(int v, int r) { return (v + r - 1) / r * r; }

// The register blocks the planner may choose: R = 4 throughout (A = 501 pads to 504 with R = 4 or 8 alike, and the four
// S cover tiles of 64 .. 512 states); `waves` = waves a SIMD holds within 512 VGPRs (hipcc's resource report).
struct Cand {
  int r, s, waves;
};
// (VGPRs with the future term: 59 / 73 / 123 / 238 for S = 1 / 2 / 4 / 8, no scratch)
constexpr Cand kCand[] = {{4, 1, 8}, {4, 2, 6}, {4, 4, 4}, {4, 8, 2}};

// One plan per period for the whole batch, by the reasoning of the single-handle planner (plan_window_search): a launch
// costs what its busiest SIMD executes.  Tasks differ in length (D, and in a ragged batch the order limit, differ per instance)
// and are dispatched longest first, so the estimate is the larger of the mean load per SIMD and the longest task, at the issue
// rate the resident waves sustain, plus one shortest task for the tail.  An instance's task length comes from its own
// R-blocks and its own D, its tile count from its own states.  Chunking the action axis (key atomics + finalize pass) is
// considered only for a SMALL batch: when 64-state tiles alone give every SIMD four tasks (sum of ceil(nx_i / 64) >= 4096) the
// plan is always one task per (instance, tile) -- no key rows, no finalize launch.  There is ONE chunk_blocks per period:
// instance i has ceil(blocks_i / chunk_blocks) chunks, and a period is chunked as soon as one instance has two.
int plan_period(sdpgpu_batch* b, int t, BatchPlan* out) {
  const int N = b->N, T = b->T;
  int d_max = 0, a_max = 0;
  int64_t tiles64 = 0;
  for (int i = 0; i < N; ++i) {
    const int D = (int)b->pmf_p[(size_t)i * T + t].size();
    d_max = std::max(d_max, D);
    a_max = std::max(a_max, (int)b->As[(size_t)i]);
    tiles64 += (b->nxs[(size_t)i] + 63) / 64;
  }
  const bool may_chunk = b->d[0].store_all_values && tiles64 < 4096;
  BatchPlan best;
  double best_cost = -1;
  bool shape_seen = false;
  size_t lds_least = 0;
  for (const Cand& c : kCand) {
    if (b->win_r && c.r != b->win_r) continue;
    if (b->win_s && c.s != b->win_s) continue;
    shape_seen = true;
    const int r = c.r, sl = c.s, nw = r + sl - 1, ts = 64 * sl;
    const int blocks_total = rup(a_max, r) / r;  // of the instance with the most actions
    const double step_ops = 3.0 * r * sl + r + (r + sl - 1) + 3.0;  // fp64 instructions of one demand step of one R-block
    int forced_nch = 0;
    if (b->win_nch) {
      const int want = std::max(1, std::min(b->win_nch, blocks_total));
      const int bpc_w = (blocks_total + want - 1) / want;
      forced_nch = (blocks_total + bpc_w - 1) / bpc_w;
    }
    for (int nch = 1; nch <= blocks_total; ++nch) {
      if (forced_nch && nch != forced_nch) continue;
      const int bpc = (blocks_total + nch - 1) / nch;
      if ((blocks_total + bpc - 1) / bpc != nch) continue;  // same plan as a smaller nch
      if (nch > 1 && !may_chunk && !forced_nch) break;
      if (nch > 1 && !b->d[0].store_all_values) break;  // chunk rows need every period's rows (as for a handle)
      int span_max = 0, min_chunks = nch;
      int64_t tasks = 0;
      double total = 0, longest = 0, shortest = 0;
      for (int i = 0; i < N; ++i) {
        const int D = (int)b->pmf_p[(size_t)i * T + t].size();
        const int blocks = rup(b->As[(size_t)i], r) / r;
        const int cb = std::min(bpc, blocks);        // R-blocks of one task of this instance
        const int chunks = (blocks + bpc - 1) / bpc;
        const int64_t tiles = (b->nxs[(size_t)i] + ts - 1) / ts;
        const int span = ts + cb * r + rup(D, nw) + sl;
        span_max = std::max(span_max, span);
        min_chunks = std::min(min_chunks, chunks);
        tasks += tiles * chunks;
        const double task = cb * (D * step_ops + 60.0 + 2.0 * (sl - 1) * r) + 400.0 + 4.0 * span;
        total += task * (double)(tiles * chunks);
        longest = std::max(longest, task);
        shortest = shortest == 0 ? task : std::min(shortest, task);
      }
      const int p_slots = sdp::win_p_slots(d_max);
      const size_t smem = sdp::batch_wg_lds(span_max, p_slots);
      const int wg = std::min(c.waves, lds_workgroups(smem));
      if (wg < 1) {
        lds_least = lds_least ? std::min(lds_least, smem) : smem;
        continue;
      }
      const int64_t resident = std::min<int64_t>(wg, (tasks + 1023) / 1024);
      auto eff = [&](int64_t w) { return w >= 8 ? 0.97 : (w >= 4 ? 0.94 : (w >= 3 ? 0.91 : (w >= 2 ? (r * sl >= 32 ? 0.93 : 0.85) : 0.60))); };
      const double cost = std::max(total / 1024.0, longest) / eff(resident) + shortest / 0.60;
      if (best_cost < 0 || cost < best_cost * 0.999) {
        best_cost = cost;
        best.R = r;
        best.S = sl;
        best.n_chunks = nch;
        best.min_chunks = min_chunks;
        best.chunk_blocks = bpc;
        best.n_tasks = tasks;
        best.span_max = span_max;
        best.p_slots_max = p_slots;
        best.smem = smem;
      }
    }
  }
  if (!best.R) {
    if (!shape_seen)
      return bfail(b, SDPGPU_ERR_ARG, "batch kernel: no instantiation for the forced block SDPGPU_WIN_R=%d SDPGPU_WIN_S=%d (have R x S = 4x1 4x2 4x4 4x8)",
                   b->win_r, b->win_s);
    return bfail(b, SDPGPU_ERR_UNSUPPORTED, "batch kernel: %d actions x %d demand steps (period %d) need %zu B of LDS per workgroup, over the %zu B of a "
                 "compute unit", a_max, d_max, t + 1, lds_least, kLdsPerCU);
  }
  if (best.n_tasks > INT32_MAX / 2) return bfail(b, SDPGPU_ERR_UNSUPPORTED, "batch kernel: too many tasks in one launch");
  *out = best;
  return SDPGPU_OK;
}

// rows of instance i in the arenas: the instances follow each other, each with its own row length (prefix sums)
size_t value_row(const sdpgpu_batch* b, int i, int t) {
  const size_t row = b->d[0].store_all_values ? (size_t)t : (size_t)(t & 1);  // (or two ping-pong tables per instance)
  return b->val_base[(size_t)i] + row * (size_t)b->nxs[(size_t)i];
}
size_t policy_row(const sdpgpu_batch* b, int i, int t) { return b->pol_base[(size_t)i] + (size_t)t * (size_t)b->nxs[(size_t)i]; }

// host layout: plans, arena offsets, the per-(period, instance) records in task order, the finalize jobs
int layout(sdpgpu_batch* b) {
  if (b->laid_out) return SDPGPU_OK;
  const int N = b->N, T = b->T;
  for (int i = 0; i < N; ++i)
    for (int t = 0; t < T; ++t)
      if (!b->pmf_set[(size_t)i * T + t]) return bfail(b, SDPGPU_ERR_STATE, "pmf of instance %d, period %d not set", i, t + 1);
  b->plan.assign((size_t)T, BatchPlan());
  b->any_chunked = false;
  for (int t = 0; t < T; ++t) {
    int rc = plan_period(b, t, &b->plan[(size_t)t]);
    if (rc) return rc;
    if (b->plan[(size_t)t].n_chunks > 1) b->any_chunked = true;
  }
  b->values_elems = (size_t)b->sum_nx * (size_t)(b->d[0].store_all_values ? T : 2);
  b->policy_elems = (size_t)b->sum_nx * (size_t)T;
  b->pmf_off.assign((size_t)N * T, 0);
  size_t off = 0;
  b->cells = 0;
  for (int i = 0; i < N; ++i)
    for (int t = 0; t < T; ++t) {
      b->pmf_off[(size_t)i * T + t] = off;
      const size_t D = b->pmf_p[(size_t)i * T + t].size();
      off += D + kPmfPad;  // the probabilities are followed by kPmfPad zeros
      b->cells += (int64_t)b->nxs[(size_t)i] * b->As[(size_t)i] * (int64_t)D;
    }
  b->pmf_elems = off;
  b->key_elems = b->any_chunked ? b->policy_elems : 0;  // (a key row per policy row, at the same offsets)
  b->inst.assign((size_t)T * N, sdp::BatchInst());
  b->jobs.clear();
  size_t chunk_off = 0;
  int64_t first = 0;
  std::vector<int> order((size_t)N);
  std::vector<int64_t> length((size_t)N);
  b->tasks.clear();
  b->task_off.assign((size_t)T, 0);
  for (int t = 0; t < T; ++t) {
    const BatchPlan& pl = b->plan[(size_t)t];
    const int nw = pl.R + pl.S - 1, ts = 64 * pl.S;
    // longest estimated task first: the instance's R-blocks per task x its demand count
    for (int i = 0; i < N; ++i) {
      order[(size_t)i] = i;
      const int blocks = rup(b->As[(size_t)i], pl.R) / pl.R;
      length[(size_t)i] = (int64_t)std::min(pl.chunk_blocks, blocks) * (int64_t)b->pmf_p[(size_t)i * T + t].size();
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return length[(size_t)a] > length[(size_t)c]; });
    b->task_off[(size_t)t] = b->tasks.size();
    for (int rank = 0; rank < N; ++rank) {
      const int i = order[(size_t)rank];
      const sdpgpu_desc& d = b->d[(size_t)i];
      const int D = (int)b->pmf_p[(size_t)i * T + t].size();
      sdp::BatchInst I{};
      const double d0 = b->d0[(size_t)i * T + t];
      I.lev0 = d.min_inventory - d0;
      I.h = d.holding_cost;
      I.pi = d.penalty_cost;
      I.K = d.fixed_order_cost;
      I.v = d.unit_order_cost;
      I.idx_off = (int32_t)((I.lev0 - d.min_inventory) / d.step);
      I.n_demand = D;
      I.d_pad = rup(D, nw);
      I.d_main = D / nw * nw;
      I.pmf_off = (int64_t)b->pmf_off[(size_t)i * T + t];
      I.v_cur_off = (int64_t)value_row(b, i, t);
      I.v_next_off = t + 1 < T ? (int64_t)value_row(b, i, t + 1) : 0;
      I.pol_off = (int64_t)policy_row(b, i, t);
      I.key_cur_off = (int64_t)policy_row(b, i, t);
      I.key_next_off = t + 1 < T ? (int64_t)policy_row(b, i, t + 1) : 0;
      const int32_t nx = b->nxs[(size_t)i];
      const int blocks = rup(b->As[(size_t)i], pl.R) / pl.R;
      I.n_states = nx;
      I.n_actions = b->As[(size_t)i];
      I.n_tiles = (nx + ts - 1) / ts;
      I.n_chunks = (blocks + pl.chunk_blocks - 1) / pl.chunk_blocks;
      I.chunk_blocks = std::min(pl.chunk_blocks, blocks);
      for (int32_t local = 0; local < I.n_tiles * I.n_chunks; ++local) b->tasks.push_back(sdp::BatchTask{rank, local});
      I.chunk_off = 0;
      if (pl.n_chunks > 1) {  // a chunked period: every instance goes through chunk rows and key rows, with its own count
        I.chunk_off = (int64_t)chunk_off;
        chunk_off += (size_t)I.n_chunks * (size_t)nx;
        sdp::FinalizeJob J{};
        J.stride = nx;
        J.lo = J.vlo = 0;
        J.hi = J.vhi = nx;
        J.first = first;
        J.n_chunks = I.n_chunks;
        // (device addresses are filled in at allocation; the offsets travel in the pointer fields until then)
        J.keys = reinterpret_cast<const unsigned long long*>((uintptr_t)I.key_cur_off);
        J.part_val = reinterpret_cast<const double*>((uintptr_t)I.chunk_off);
        J.v_out = reinterpret_cast<double*>((uintptr_t)I.v_cur_off);
        J.pol_out = reinterpret_cast<int32_t*>((uintptr_t)I.pol_off);
        first += nx;
        b->jobs.push_back(J);
      }
      b->inst[(size_t)t * N + rank] = I;
    }
    if ((int64_t)(b->tasks.size() - b->task_off[(size_t)t]) != pl.n_tasks)
      return bfail(b, SDPGPU_ERR_INTERNAL, "batch layout: period %d has %zu tasks, its plan says %lld", t + 1,
                   b->tasks.size() - b->task_off[(size_t)t], (long long)pl.n_tasks);
  }
  b->chunk_elems = chunk_off;
  b->total_final = first;
  b->laid_out = true;
  return SDPGPU_OK;
}

int allocate(sdpgpu_batch* b) {
  if (b->allocated) return SDPGPU_OK;
  int rc = layout(b);
  if (rc) return rc;
  if ((rc = b->f.open(b->N))) return rc;
  const int N = b->N, T = b->T;
  BHIP_TRY(b, hipMalloc((void**)&b->d_values, std::max<size_t>(b->values_elems, 1) * sizeof(double)));
  BHIP_TRY(b, hipMalloc((void**)&b->d_policy, std::max<size_t>(b->policy_elems, 1) * sizeof(int32_t)));
  BHIP_TRY(b, hipMalloc((void**)&b->d_pmf, std::max<size_t>(b->pmf_elems, 1) * sizeof(double)));
  {
    std::vector<double> host(b->pmf_elems, 0.0);
    for (size_t k = 0; k < (size_t)N * T; ++k)
      std::memcpy(&host[b->pmf_off[k]], b->pmf_p[k].data(), b->pmf_p[k].size() * sizeof(double));
    BHIP_TRY(b, hipMemcpy(b->d_pmf, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  BHIP_TRY(b, hipMalloc((void**)&b->d_inst, b->inst.size() * sizeof(sdp::BatchInst)));
  BHIP_TRY(b, hipMemcpy(b->d_inst, b->inst.data(), b->inst.size() * sizeof(sdp::BatchInst), hipMemcpyHostToDevice));
  BHIP_TRY(b, hipMalloc((void**)&b->d_tasks, std::max<size_t>(b->tasks.size(), 1) * sizeof(sdp::BatchTask)));
  BHIP_TRY(b, hipMemcpy(b->d_tasks, b->tasks.data(), b->tasks.size() * sizeof(sdp::BatchTask), hipMemcpyHostToDevice));
  if (b->any_chunked) {
    BHIP_TRY(b, hipMalloc((void**)&b->d_keys, b->key_elems * sizeof(unsigned long long)));
    BHIP_TRY(b, hipMalloc((void**)&b->d_chunk_val, std::max<size_t>(b->chunk_elems, 1) * sizeof(double)));
    BHIP_TRY(b, hipMalloc((void**)&b->d_chunk_idx, std::max<size_t>(b->chunk_elems, 1) * sizeof(int32_t)));
    std::vector<sdp::FinalizeJob> jobs = b->jobs;
    for (sdp::FinalizeJob& J : jobs) {
      const size_t chunk_off = (size_t)(uintptr_t)J.part_val;
      J.keys = b->d_keys + (size_t)(uintptr_t)J.keys;
      J.part_val = b->d_chunk_val + chunk_off;
      J.part_idx = b->d_chunk_idx + chunk_off;
      J.v_out = b->d_values + (size_t)(uintptr_t)J.v_out;
      J.pol_out = b->d_policy + (size_t)(uintptr_t)J.pol_out;
    }
    BHIP_TRY(b, hipMalloc((void**)&b->d_jobs, jobs.size() * sizeof(sdp::FinalizeJob)));
    BHIP_TRY(b, hipMemcpy(b->d_jobs, jobs.data(), jobs.size() * sizeof(sdp::FinalizeJob), hipMemcpyHostToDevice));
  }
  {
    // the period-1 initial state of every instance (validated at create: a grid point)
    std::vector<int64_t> offs((size_t)2 * N);
    for (int i = 0; i < N; ++i) {
      const sdpgpu_desc& d = b->d[(size_t)i];
      const int64_t ix = (int64_t)((d.ini_inventory - d.min_inventory) / d.step);
      offs[(size_t)i] = (int64_t)value_row(b, i, 0) + ix;
      offs[(size_t)N + i] = (int64_t)policy_row(b, i, 0) + ix;
    }
    BHIP_TRY(b, hipMalloc((void**)&b->d_ini_off, offs.size() * sizeof(int64_t)));
    BHIP_TRY(b, hipMemcpy(b->d_ini_off, offs.data(), offs.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  b->allocated = true;
  return SDPGPU_OK;
}

template <int R, int S>
hipError_t launch_rs(sdpgpu_batch* b, const sdp::BatchLaunch& L, const BatchPlan& pl, const sdp::BatchInst* inst,
                     const sdp::BatchTask* tasks, bool future, bool keyed_in) {
  const dim3 grid((unsigned)((L.n_tasks + 3) / 4));
#define SDP_BATCH_GO(FU, KI)                                                                                         \
  do {                                                                                                               \
    static LdsMark mark;                                                                                             \
    hipError_t ea = lds_allow(sdp::window_f1_batch_kernel<R, S, FU, KI>, pl.smem, &mark);                            \
    if (ea != hipSuccess) return ea;                                                                                 \
    hipLaunchKernelGGL((sdp::window_f1_batch_kernel<R, S, FU, KI>), grid, dim3(256), pl.smem, b->f.stream, L, inst,    \
                       tasks, b->d_values, b->d_policy, b->d_pmf, b->d_keys, b->d_chunk_val, b->d_chunk_idx);        \
  } while (0)
  if (!future)
    SDP_BATCH_GO(false, false);
  else if (keyed_in)
    SDP_BATCH_GO(true, true);
  else
    SDP_BATCH_GO(true, false);
#undef SDP_BATCH_GO
  return hipGetLastError();
}

hipError_t launch_period(sdpgpu_batch* b, int t) {
  const BatchPlan& pl = b->plan[(size_t)t];
  sdp::BatchLaunch L{};
  L.step = b->d[0].step;
  L.n_tasks = (int32_t)pl.n_tasks;
  L.chunked = pl.n_chunks > 1;
  L.span_max = pl.span_max;
  L.p_slots_max = pl.p_slots_max;
  L.maxdir = b->d[0].direction == SDPGPU_MAX;
  if (!grid_ok((L.n_tasks + 3) / 4)) return hipErrorInvalidValue;
  const bool future = t + 1 < b->T;
  // V_{t+1} is read from its key row while that period's final rows are still pending (they are written by the one
  // finalize pass at the end of the sweep)
  const bool keyed_in = future && b->plan[(size_t)t + 1].n_chunks > 1;
  const sdp::BatchInst* inst = b->d_inst + (size_t)t * b->N;
  const sdp::BatchTask* tasks = b->d_tasks + b->task_off[(size_t)t];
  if (pl.R == 4 && pl.S == 1) return launch_rs<4, 1>(b, L, pl, inst, tasks, future, keyed_in);
  if (pl.R == 4 && pl.S == 2) return launch_rs<4, 2>(b, L, pl, inst, tasks, future, keyed_in);
  if (pl.R == 4 && pl.S == 4) return launch_rs<4, 4>(b, L, pl, inst, tasks, future, keyed_in);
  if (pl.R == 4 && pl.S == 8) return launch_rs<4, 8>(b, L, pl, inst, tasks, future, keyed_in);
  return hipErrorInvalidValue;
}

// what differs between instance k and instance 0 although the batch needs it shared (nullptr: nothing); a ragged batch
// leaves the inventory bounds and the order limit to the instance
const char* shape_mismatch(const sdpgpu_desc& a, const sdpgpu_desc& c, bool ragged, char* buf, size_t n) {
#define SDP_SAME_I(f) \
  if (a.f != c.f) { std::snprintf(buf, n, #f " %d differs from instance 0's %d", (int)c.f, (int)a.f); return buf; }
#define SDP_SAME_D(f) \
  if (a.f != c.f) { std::snprintf(buf, n, #f " %g differs from instance 0's %g", (double)c.f, (double)a.f); return buf; }
  SDP_SAME_I(direction)
  SDP_SAME_I(periods)
  SDP_SAME_D(step)
  if (!ragged) {
    SDP_SAME_D(min_inventory)
    SDP_SAME_D(max_inventory)
    SDP_SAME_D(max_order_quantity)
  }
  SDP_SAME_I(device)
  SDP_SAME_I(store_all_values)
#undef SDP_SAME_I
#undef SDP_SAME_D
  return nullptr;
}

int batch_create(const sdpgpu_desc* descs, int32_t n, sdpgpu_batch** out, bool ragged) {
  g_create_error.clear();
  if (!descs || !out) return bfail(nullptr, SDPGPU_ERR_ARG, "batch_create: null argument (descs, out)");
  *out = nullptr;
  if (n < 1 || n > 1000000) return bfail(nullptr, SDPGPU_ERR_ARG, "batch_create: n = %d instances (1 .. 1000000)", n);
  return guarded((sdpgpu_batch*)nullptr, "sdpgpu_batch_create", [&]() -> int {
    if (!ragged && descs[0].family == SDPGPU_FAMILY_STAFF) {  // the family of instance 0 selects the kind of batch
      std::string why;
      sdpgpu_batch* b = new sdpgpu_batch();  // (first: the staff batch works on its frame)
      int rc = SDPGPU_OK;
      try {
        rc = staff_batch_new(descs, n, &b->f, &b->staff, &why);
        g_create_error = why;
      } catch (...) {
        delete b;
        throw;
      }
      if (rc) {
        delete b;
        return rc;
      }
      b->N = n;
      b->T = descs[0].periods;
      *out = b;
      return SDPGPU_OK;
    }
    for (int32_t k = 0; k < n; ++k) {
      const sdpgpu_desc& d = descs[k];
      int rc = validate(d);
      if (rc) {
        const std::string why = g_create_error;
        return bfail(nullptr, rc, "instance %d: %s", k, why.c_str());
      }
      if (d.family != SDPGPU_FAMILY_BACKORDER)
        return bfail(nullptr, SDPGPU_ERR_UNSUPPORTED, "instance %d: family %d -- a batch holds the backorder family (SDPGPU_FAMILY_BACKORDER) only", k, d.family);
      if (!d.clamp_inventory)
        return bfail(nullptr, SDPGPU_ERR_UNSUPPORTED, "instance %d: clamp_inventory = 0 -- a batch needs one fixed grid for all periods", k);
      if (d.world_size != 1)
        return bfail(nullptr, SDPGPU_ERR_UNSUPPORTED, "instance %d: world_size %d -- a batch runs on one device (split the instance list per rank on the host)", k, d.world_size);
      if (d.kernel != SDPGPU_KERNEL_AUTO && d.kernel != SDPGPU_KERNEL_WINDOW)
        return bfail(nullptr, SDPGPU_ERR_UNSUPPORTED, "instance %d: kernel %d -- a batch runs the window kernel (SDPGPU_KERNEL_AUTO or _WINDOW)", k, d.kernel);
      char buf[160];
      if (const char* why = shape_mismatch(descs[0], d, ragged, buf, sizeof buf))
        return bfail(nullptr, SDPGPU_ERR_ARG, "instance %d: %s (%s)", k, why,
                     ragged ? "the instances of a ragged batch share direction, horizon, step, device and table storage"
                            : "the instances of a batch share one grid shape");
      if (std::fmod(d.ini_inventory, d.step) != 0 || d.ini_inventory < d.min_inventory || d.ini_inventory > d.max_inventory)
        return bfail(nullptr, SDPGPU_ERR_ARG, "instance %d: ini_inventory %g is not a point of the grid [%g, %g]", k, d.ini_inventory, d.min_inventory, d.max_inventory);
    }
    const sdpgpu_desc& d = descs[0];
    // states and actions per instance; the size refusals count the SUM of the instances' states
    std::vector<int32_t> nxs((size_t)n), As((size_t)n);
    double sum_nx = 0;
    for (int32_t k = 0; k < n; ++k) {
      const sdpgpu_desc& dk = descs[k];
      const int64_t nx = (int64_t)((dk.max_inventory - dk.min_inventory) / dk.step) + 1;
      const int32_t A = full_action_count(dk);
      if (nx >= 2147483647LL - 4096 || (int64_t)A + nx > 2000000000LL) return bfail(nullptr, SDPGPU_ERR_UNSUPPORTED, "axis longer than 2^31");
      nxs[(size_t)k] = (int32_t)nx;
      As[(size_t)k] = A;
      sum_nx += (double)nx;
    }
    if (sum_nx * d.periods > 4.0e9) {
      if (ragged)
        return bfail(nullptr, SDPGPU_ERR_UNSUPPORTED, "batch tables of %d periods x %.0f states (the sum over %d instances) are too large", d.periods, sum_nx, n);
      return bfail(nullptr, SDPGPU_ERR_UNSUPPORTED, "batch tables of %d x %d x %lld states are too large", n, d.periods, (long long)nxs[0]);
    }
    sdpgpu_batch* b = new sdpgpu_batch();
    try {
      b->d.assign(descs, descs + n);
      b->N = n;
      b->T = d.periods;
      b->ragged = ragged;
      b->nxs.swap(nxs);
      b->As.swap(As);
      b->val_base.assign((size_t)n, 0);
      b->pol_base.assign((size_t)n, 0);
      size_t vb = 0, pb = 0;
      for (int32_t k = 0; k < n; ++k) {
        b->val_base[(size_t)k] = vb;
        b->pol_base[(size_t)k] = pb;
        vb += (size_t)b->nxs[(size_t)k] * (size_t)(d.store_all_values ? d.periods : 2);
        pb += (size_t)b->nxs[(size_t)k] * (size_t)d.periods;
      }
      b->sum_nx = (int64_t)sum_nx;
      b->f.device = d.device;
      b->f.T = d.periods;
      b->d0.assign((size_t)n * b->T, 0.0);
      b->pmf_p.resize((size_t)n * b->T);
      b->pmf_set.assign((size_t)n * b->T, 0);
      b->samp.resize((size_t)n * b->T);
      if (const char* e = std::getenv("SDPGPU_WIN_R")) b->win_r = std::atoi(e);
      if (const char* e = std::getenv("SDPGPU_WIN_NCH")) b->win_nch = std::atoi(e);
      if (const char* e = std::getenv("SDPGPU_WIN_S")) b->win_s = std::atoi(e);
    } catch (...) {
      delete b;
      throw;
    }
    *out = b;
    return SDPGPU_OK;
  });
}

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int sdpgpu_batch_create(const sdpgpu_desc* descs, int32_t n, sdpgpu_batch** out) { return batch_create(descs, n, out, false); }

int sdpgpu_batch_create_ragged(const sdpgpu_desc* descs, int32_t n, sdpgpu_batch** out) { return batch_create(descs, n, out, true); }

int64_t sdpgpu_batch_num_states(const sdpgpu_batch* b, int32_t instance) {
  if (b && b->staff) return staff_batch_num_states(b->staff, instance);
  return b && instance >= 0 && instance < b->N ? (int64_t)b->nxs[(size_t)instance] : -1;
}

int32_t sdpgpu_batch_num_actions(const sdpgpu_batch* b, int32_t instance) {
  if (b && b->staff) return staff_batch_num_actions(b->staff, instance);
  return b && instance >= 0 && instance < b->N ? b->As[(size_t)instance] : -1;
}

int sdpgpu_batch_plan_period(sdpgpu_batch* b, int32_t period, sdpgpu_batch_plan* out) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_REFUSE(b, "sdpgpu_batch_plan_period");
  if (!out) return bfail(b, SDPGPU_ERR_ARG, "sdpgpu_batch_plan_period: out is null");
  if (period < 1 || period > b->T) return bfail(b, SDPGPU_ERR_ARG, "sdpgpu_batch_plan_period: period %d outside 1 .. %d", period, b->T);
  return guarded(b, "sdpgpu_batch_plan_period", [&]() -> int {
    std::memset(out, 0, sizeof *out);
    int rc = layout(b);  // (host arithmetic only; names the first pmf that is missing)
    if (rc) return rc;
    const BatchPlan& p = b->plan[(size_t)period - 1];
    out->r = p.R;
    out->s = p.S;
    out->chunk_blocks = p.chunk_blocks;
    out->chunked = p.n_chunks > 1;
    out->max_chunks = p.n_chunks;
    out->min_chunks = p.min_chunks;
    out->tasks = p.n_tasks;
    out->lds_bytes = (int64_t)p.smem;
    return SDPGPU_OK;
  });
}

void sdpgpu_batch_destroy(sdpgpu_batch* b) {
  if (!b) return;
  if (b->staff) {
    staff_batch_delete(b->staff);
    delete b;
    return;
  }
  b->f.close(b->allocated || b->d_values || b->d_pmf,
             {b->d_values, b->d_policy, b->d_pmf, b->d_inst, b->d_tasks, b->d_keys, b->d_chunk_val, b->d_chunk_idx, b->d_jobs, b->d_ini_off,
              b->d_samp, b->d_thr, b->d_sim_inst, b->d_fit_pairs, b->d_fit, b->d_gy, b->d_gy_pairs});
  delete b;
}

const char* sdpgpu_batch_last_error(const sdpgpu_batch* b) { return b ? b->f.err.c_str() : g_create_error.c_str(); }

int sdpgpu_batch_set_pmf(sdpgpu_batch* b, int32_t instance, int32_t t, const double* demand, const double* prob, int32_t n) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_REFUSE(b, "sdpgpu_batch_set_pmf");
  return guarded(b, "sdpgpu_batch_set_pmf", [&]() -> int {
    if (instance < 0 || instance >= b->N) return bfail(b, SDPGPU_ERR_ARG, "batch_set_pmf: instance %d outside 0 .. %d", instance, b->N - 1);
    if (t < 0 || t >= b->T) return bfail(b, SDPGPU_ERR_ARG, "batch_set_pmf: period index %d outside 0 .. %d", t, b->T - 1);
    if (!demand || !prob || n < 1) return bfail(b, SDPGPU_ERR_ARG, "batch_set_pmf: bad argument (instance %d, t=%d, n=%d)", instance, t, n);
    if (b->allocated) return bfail(b, SDPGPU_ERR_STATE, "pmf is frozen once the device tables exist");
    const double step = b->d[0].step;
    for (int32_t j = 0; j < n; ++j) {
      if (std::fmod(demand[j], step) != 0)
        return bfail(b, SDPGPU_ERR_ARG, "demand %g of instance %d, period %d is not a multiple of step", demand[j], instance, t + 1);
      if (j && !(demand[j] > demand[j - 1]))
        return bfail(b, SDPGPU_ERR_ARG, "demands of instance %d, period %d must be strictly ascending", instance, t + 1);
      if (j && demand[j] - demand[j - 1] != step)
        return bfail(b, SDPGPU_ERR_ARG, "demands of instance %d, period %d: spacing %g between points %d and %d, the batch kernel needs "
                     "spacing = step (%g)", instance, t + 1, demand[j] - demand[j - 1], j - 1, j, step);
    }
    const int32_t A = b->As[(size_t)instance];
    if (std::fabs(demand[0]) > 1.0e9 || n > 3000 || (int64_t)A + n > 3500)
      return bfail(b, SDPGPU_ERR_UNSUPPORTED, "instance %d, period %d: %d actions + %d demand points exceed the window kernel's 3500", instance, t + 1, A, n);
    const size_t k = (size_t)instance * b->T + t;
    b->pmf_p[k].assign(prob, prob + n);
    b->d0[k] = demand[0];
    b->pmf_set[k] = 1;
    b->laid_out = false;
    return SDPGPU_OK;
  });
}

int sdpgpu_batch_set_stream(sdpgpu_batch* b, void* hip_stream) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  return b->f.set_stream(hip_stream);
}

int sdpgpu_batch_set_profiling(sdpgpu_batch* b, int32_t on) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  b->f.profiling = on != 0;
  return SDPGPU_OK;
}

int sdpgpu_batch_solve(sdpgpu_batch* b, int32_t sync) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_FORWARD(b, "sdpgpu_batch_solve", staff_batch_solve(b->staff, sync));
  return guarded(b, "sdpgpu_batch_solve", [&]() -> int {
    int rc = layout(b);  // (argument and state errors before the device is touched)
    if (rc) return rc;
    DeviceScope dev;
    BHIP_TRY(b, dev.enter(b->f.device));
    rc = allocate(b);
    if (rc) return rc;
    b->period_launches = b->finalize_launches = b->periods_run = 0;
    b->gy_valid = false;  // (the G rows are those of the tables about to be replaced)
    if ((rc = b->f.sweep_begin())) return rc;
    if (b->any_chunked) {  // key rows back to the reduction identity
      const int64_t nk = (int64_t)b->key_elems;
      if (!grid_ok((nk + 255) / 256)) return bfail(b, SDPGPU_ERR_UNSUPPORTED, "key rows too long for one launch");
      BHIP_TRY(b, launch_key_fill(b->d_keys, nk, (int)(b->d[0].direction == SDPGPU_MAX), b->f.stream));
      b->finalize_launches++;
    }
    for (int t = b->T - 1; t >= 0; --t) {
      if ((rc = b->f.period_mark(t))) return rc;
      hipError_t e = launch_period(b, t);
      if (e != hipSuccess) return bfail(b, SDPGPU_ERR_DEVICE, "batch period %d: %s", t + 1, hipGetErrorString(e));
      b->period_launches++;
      b->periods_run++;
    }
    if ((rc = b->f.period_mark(-1))) return rc;
    if (b->any_chunked && b->total_final > 0) {  // V_t = unkey(K_t), policy = action of the lowest chunk that attains it: one launch
      if (!grid_ok((b->total_final + 255) / 256)) return bfail(b, SDPGPU_ERR_UNSUPPORTED, "finalize pass too long for one launch");
      BHIP_TRY(b, launch_finalize(b->d_jobs, (int)b->jobs.size(), b->total_final, b->f.stream));
      b->finalize_launches++;
    }
    b->solved = true;
    return b->f.sweep_end(sync != 0);
  });
}

int sdpgpu_batch_synchronize(sdpgpu_batch* b) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  return b->f.synchronize(b->staff ? staff_batch_allocated(b->staff) : b->allocated);
}

static int read_check(sdpgpu_batch* b, const char* who, int32_t instance, int32_t period, const void* out, int64_t n, bool is_values) {
  const int32_t nx = instance >= 0 && instance < b->N ? b->nxs[(size_t)instance] : 0;  // the instance's own count
  char states[64];
  std::snprintf(states, sizeof states, "the grid has %d states", nx);
  return read_check(&b->f, who, instance, b->N, period, out, n, nx, states, b->solved, false, is_values && !b->d[0].store_all_values);
}

int sdpgpu_batch_values(sdpgpu_batch* b, int32_t instance, int32_t period, double* out, int64_t n) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_FORWARD(b, "sdpgpu_batch_values", staff_batch_values(b->staff, instance, period, out, n));
  int rc = read_check(b, "sdpgpu_batch_values", instance, period, out, n, true);
  if (rc) return rc;
  return b->f.read_row(out, b->d_values + value_row(b, instance, period - 1), (size_t)n * sizeof(double));
}

int sdpgpu_batch_policy(sdpgpu_batch* b, int32_t instance, int32_t period, int32_t* out, int64_t n) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_FORWARD(b, "sdpgpu_batch_policy", staff_batch_policy(b->staff, instance, period, out, n));
  int rc = read_check(b, "sdpgpu_batch_policy", instance, period, out, n, false);
  if (rc) return rc;
  return b->f.read_row(out, b->d_policy + policy_row(b, instance, period - 1), (size_t)n * sizeof(int32_t));
}

int sdpgpu_batch_initial(sdpgpu_batch* b, double* out_value, int32_t* out_action_index) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_FORWARD(b, "sdpgpu_batch_initial", staff_batch_initial(b->staff, out_value, out_action_index));
  if (!out_value || !out_action_index) return bfail(b, SDPGPU_ERR_ARG, "sdpgpu_batch_initial: null output");
  if (!b->solved) return bfail(b, SDPGPU_ERR_STATE, "sdpgpu_batch_initial before sdpgpu_batch_solve");
  return guarded(b, "sdpgpu_batch_initial", [&]() -> int {
    DeviceScope dev;
    BHIP_TRY(b, dev.enter(b->f.device));
    const int N = b->N;
    hipLaunchKernelGGL(sdp::batch_initial_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, b->f.stream, b->d_values, b->d_policy,
                       b->d_ini_off, b->d_ini_off + N, N, b->f.ini_value(), b->f.ini_action(N));
    BHIP_TRY(b, hipGetLastError());
    return b->f.initial_download(out_value, out_action_index, N);
  });
}

int sdpgpu_batch_stats_get(sdpgpu_batch* b, sdpgpu_batch_stats* out) {
  if (!b || !out) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_FORWARD(b, "sdpgpu_batch_stats_get", staff_batch_stats(b->staff, out));
  return guarded(b, "sdpgpu_batch_stats_get", [&]() -> int {
    std::memset(out, 0, sizeof *out);
    out->instances = b->N;
    out->periods_run = b->periods_run;
    out->period_launches = b->period_launches;
    out->finalize_launches = b->finalize_launches;
    bool all_set = true;
    for (char c : b->pmf_set) all_set = all_set && c;
    if (all_set) {  // the plan is host arithmetic: available before anything has run
      int rc = layout(b);
      if (rc) return rc;
      out->window_r = b->plan[0].R;
      out->window_s = b->plan[0].S;
      for (const BatchPlan& p : b->plan) {
        out->window_chunks = std::max(out->window_chunks, p.n_chunks);
        out->lds_bytes = std::max<int64_t>(out->lds_bytes, (int64_t)p.smem);
      }
      out->cells_evaluated = b->solved ? b->cells : 0;
    }
    return b->f.solve_ms(&out->solve_ms);
  });
}

double sdpgpu_batch_period_ms(sdpgpu_batch* b, int32_t period) {
  if (!b) return -1.0;
  b->f.err.clear();
  return b->f.period_ms(period);
}

// ---- the staff batch's own calls (sdpgpu_staffbatch.hip) ----
int sdpgpu_batch_add_level_pmf(sdpgpu_batch* b, const double* prob, const int32_t* row_len, int32_t n_rows, int32_t row_stride,
                               int32_t* out_table) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_ONLY(b, "sdpgpu_batch_add_level_pmf");
  return guarded(b, "sdpgpu_batch_add_level_pmf",
                 [&]() -> int { return staff_batch_add_table(b->staff, prob, row_len, n_rows, row_stride, out_table); });
}

int sdpgpu_batch_use_level_pmf(sdpgpu_batch* b, int32_t instance, int32_t t, int32_t table) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_ONLY(b, "sdpgpu_batch_use_level_pmf");
  return guarded(b, "sdpgpu_batch_use_level_pmf", [&]() -> int { return staff_batch_use_table(b->staff, instance, t, table); });
}

int sdpgpu_batch_set_overhead(sdpgpu_batch* b, int32_t instance, int32_t t, double min_staff) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_ONLY(b, "sdpgpu_batch_set_overhead");
  return guarded(b, "sdpgpu_batch_set_overhead", [&]() -> int { return staff_batch_set_min_staff(b->staff, instance, t, min_staff); });
}

int sdpgpu_batch_grid(sdpgpu_batch* b, int32_t instance, int32_t period, double* x_lo, int64_t* nx) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_FORWARD(b, "sdpgpu_batch_grid", staff_batch_grid(b->staff, instance, period, x_lo, nx));
  if (instance < 0 || instance >= b->N) return bfail(b, SDPGPU_ERR_ARG, "sdpgpu_batch_grid: instance %d outside 0 .. %d", instance, b->N - 1);
  if (period < 1 || period > b->T) return bfail(b, SDPGPU_ERR_ARG, "sdpgpu_batch_grid: period %d outside 1 .. %d", period, b->T);
  if (!x_lo || !nx) return bfail(b, SDPGPU_ERR_ARG, "sdpgpu_batch_grid: null output");
  *x_lo = b->d[(size_t)instance].min_inventory;  // (one fixed grid for all periods)
  *nx = b->nxs[(size_t)instance];
  return SDPGPU_OK;
}

int sdpgpu_batch_staff_plan_period(sdpgpu_batch* b, int32_t period, sdpgpu_batch_staff_plan* out) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_ONLY(b, "sdpgpu_batch_staff_plan_period");
  return guarded(b, "sdpgpu_batch_staff_plan_period", [&]() -> int { return staff_batch_plan(b->staff, period, out); });
}

int sdpgpu_batch_staff_reachable(sdpgpu_batch* b, int32_t instance, int32_t period, int64_t* lo, int64_t* hi) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_ONLY(b, "sdpgpu_batch_staff_reachable");
  return guarded(b, "sdpgpu_batch_staff_reachable", [&]() -> int { return staff_batch_reachable(b->staff, instance, period, lo, hi); });
}

int sdpgpu_batch_staff_fit_ss(sdpgpu_batch* b, double max_order_quantity, double* out) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_ONLY(b, "sdpgpu_batch_staff_fit_ss");
  return guarded(b, "sdpgpu_batch_staff_fit_ss", [&]() -> int { return staff_batch_fit_ss(b->staff, max_order_quantity, out); });
}

int sdpgpu_batch_staff_simulate(sdpgpu_batch* b, const int32_t* sample_nums, uint64_t seed, double ini_x, const double* ss, int32_t n_rules,
                                sdpgpu_sim_result* results, double* out_sum, uint8_t* out_valid, int32_t* out_demand) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_ONLY(b, "sdpgpu_batch_staff_simulate");
  return guarded(b, "sdpgpu_batch_staff_simulate", [&]() -> int {
    return staff_batch_simulate(b->staff, sample_nums, seed, ini_x, ss, n_rules, results, out_sum, out_valid, out_demand);
  });
}

int sdpgpu_batch_staff_gy(sdpgpu_batch* b, int32_t instance, int32_t period, int32_t y_lo, int32_t n, double* out) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_ONLY(b, "sdpgpu_batch_staff_gy");
  return guarded(b, "sdpgpu_batch_staff_gy", [&]() -> int { return staff_batch_gy(b->staff, instance, period, y_lo, n, out); });
}

int sdpgpu_batch_staff_check_convexity(sdpgpu_batch* b, int32_t kind, int32_t source, int32_t period, const int32_t* lo, const int32_t* hi,
                                       const double* K, const int32_t* capacity, sdpgpu_convexity* out) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_ONLY(b, "sdpgpu_batch_staff_check_convexity");
  return guarded(b, "sdpgpu_batch_staff_check_convexity",
                 [&]() -> int { return staff_batch_check_convexity(b->staff, kind, source, period, lo, hi, K, capacity, out); });
}

}  // extern "C"

// =================================================================================================
// Batched simulation (sdp_batch_sim.hpp): the samplers and what every rollout checks (the rollouts end the file)
// =================================================================================================
namespace {

// sampler records + threshold arena on the device (spec tables as set; tile tables = the running sum of the tile)
int sim_upload_samplers(sdpgpu_batch* b) {
  if (!b->samp_dirty && b->d_samp) return SDPGPU_OK;
  const size_t NT = (size_t)b->N * b->T;
  std::vector<sdp::SimSampler> rec(NT);
  std::vector<double> arena;
  for (size_t k = 0; k < NT; ++k) {
    if (b->samp.has(k)) {
      rec[k] = b->samp.append(k, &arena);
      continue;
    }
    sdp::SimSampler S{};
    S.off = (int64_t)arena.size();
    S.val_off = -1;  // demand = k_lo + q (validate: step 1 and a gapless tile)
    S.k_lo = (int32_t)b->d0[k];
    S.strict = 0;
    S.m = (int32_t)b->pmf_p[k].size();
    append_tile_thresholds(b->pmf_p[k], &arena);
    rec[k] = S;
  }
  if (b->d_samp) (void)hipFree(b->d_samp);
  if (b->d_thr) (void)hipFree(b->d_thr);
  b->d_samp = nullptr;
  b->d_thr = nullptr;
  BHIP_TRY(b, hipMalloc((void**)&b->d_samp, NT * sizeof(sdp::SimSampler)));
  BHIP_TRY(b, hipMalloc((void**)&b->d_thr, std::max<size_t>(arena.size(), 1) * sizeof(double)));
  BHIP_TRY(b, hipMemcpy(b->d_samp, rec.data(), NT * sizeof(sdp::SimSampler), hipMemcpyHostToDevice));
  if (!arena.empty()) BHIP_TRY(b, hipMemcpy(b->d_thr, arena.data(), arena.size() * sizeof(double), hipMemcpyHostToDevice));
  b->samp_dirty = false;
  return SDPGPU_OK;
}

sdp::SimLaunch sim_launch_params(const sdpgpu_batch* b, int32_t n_paths, uint64_t seed, int64_t stride) {
  sdp::SimLaunch L{};
  const sdpgpu_desc& d = b->d[0];
  L.step = d.step;
  L.inv_step = 1.0 / d.step;  // exact: step is a power of two (validate)
  L.T = b->T;
  L.n_inst = b->N;
  L.waves_per_inst = (n_paths + 63) / 64;
  L.demand_stride = stride;
  L.R = make_stream(n_paths, seed, 0);
  return L;
}

int sim_needs_unit_step(sdpgpu_batch* b, const char* who) {
  if (b->d[0].step != 1.0)
    return bfail(b, SDPGPU_ERR_UNSUPPORTED, "%s: step %g -- sampled demands are Math.round's integers (Simulation.java:64), the sampler needs step == 1",
                 who, b->d[0].step);
  return SDPGPU_OK;
}

// What every rollout of a batch takes -- of the table policy and of a level rule alike: the outputs, the path count, the
// explicit demands, the start states (ini[i]: the inventory instance i starts from) and, when sampled, the unit step.
int sim_check_args(sdpgpu_batch* b, const char* who, int32_t n_paths, const double* demand, int64_t stride, bool sampled, const double* ini_x,
                   const double* out_mean, std::vector<double>* ini) {
  const int N = b->N, T = b->T;
  if (!out_mean) return bfail(b, SDPGPU_ERR_ARG, "%s: out_mean is null", who);
  if (const int rc = check_n_paths(b, who, n_paths)) return rc;
  if (!sampled) {
    if (!demand) return bfail(b, SDPGPU_ERR_ARG, "%s: demand is null", who);
    if (stride != 0 && stride < (int64_t)n_paths * T)
      return bfail(b, SDPGPU_ERR_ARG, "%s: instance_stride %lld is neither 0 (one shared set) nor >= n_paths * T = %lld", who, (long long)stride,
                   (long long)n_paths * T);
  }
  ini->assign((size_t)N, 0.0);
  for (int i = 0; i < N; ++i) {
    const sdpgpu_desc& di = b->d[(size_t)i];  // the instance's OWN grid
    const double x = ini_x ? ini_x[i] : di.ini_inventory;
    if (!(x >= di.min_inventory && x <= di.max_inventory) || std::fmod(x, di.step) != 0)
      return bfail(b, SDPGPU_ERR_ARG, "%s: instance %d: ini_x %g is not a point of the grid [%g, %g]", who, i, x, di.min_inventory, di.max_inventory);
    (*ini)[(size_t)i] = x;
  }
  return sampled ? sim_needs_unit_step(b, who) : SDPGPU_OK;
}

}  // namespace

extern "C" {

int sdpgpu_batch_set_sampler(sdpgpu_batch* b, int32_t instance, int32_t t, const sdpgpu_dist_spec* spec) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_REFUSE(b, "sdpgpu_batch_set_sampler");
  return guarded(b, "sdpgpu_batch_set_sampler", [&]() -> int {
    if (instance < 0 || instance >= b->N) return bfail(b, SDPGPU_ERR_ARG, "batch_set_sampler: instance %d outside 0 .. %d", instance, b->N - 1);
    if (t < 0 || t >= b->T) return bfail(b, SDPGPU_ERR_ARG, "batch_set_sampler: period index %d outside 0 .. %d", t, b->T - 1);
    int rc = sim_needs_unit_step(b, "batch_set_sampler");
    if (rc) return rc;
    const size_t k = (size_t)instance * b->T + t;
    if (!spec) {
      b->samp.clear(k);
    } else {
      std::string why;
      rc = b->samp.set(k, *spec, &why);
      if (rc) return bfail(b, rc, "batch_set_sampler: instance %d, period %d: spec: %s", instance, t + 1, why.c_str());
    }
    b->samp_dirty = true;
    return SDPGPU_OK;
  });
}

int sdpgpu_batch_sample_demands(sdpgpu_batch* b, int32_t instance, int32_t n_paths, uint64_t seed, double* out_demand, double* out_u) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_REFUSE(b, "sdpgpu_batch_sample_demands");
  return guarded(b, "sdpgpu_batch_sample_demands", [&]() -> int {
    const char* who = "sdpgpu_batch_sample_demands";
    if (instance < 0 || instance >= b->N) return bfail(b, SDPGPU_ERR_ARG, "%s: instance %d outside 0 .. %d", who, instance, b->N - 1);
    if (!out_demand) return bfail(b, SDPGPU_ERR_ARG, "%s: out_demand is null", who);
    int rc = check_n_paths(b, who, n_paths);
    if (rc) return rc;
    rc = sim_needs_unit_step(b, who);
    if (rc) return rc;
    rc = layout(b);  // (every pmf set: the tile samplers read them)
    if (rc) return rc;
    DeviceScope dev;
    BHIP_TRY(b, dev.enter(b->f.device));
    rc = allocate(b);
    if (rc) return rc;
    rc = sim_upload_samplers(b);
    if (rc) return rc;
    const size_t elems = (size_t)n_paths * b->T;
    Carve c;
    const size_t o_dem = c.take(elems * 8), o_u = c.take(out_u ? elems * 8 : 0);
    rc = sim_scratch(&b->f, c.at);
    if (rc) return rc;
    double* d_dem = reinterpret_cast<double*>(b->f.d_sim_scratch + o_dem);
    double* d_u = out_u ? reinterpret_cast<double*>(b->f.d_sim_scratch + o_u) : nullptr;
    const sdp::SimLaunch L = sim_launch_params(b, n_paths, seed, 0);
    hipLaunchKernelGGL(sdp::batch_sim_draw_kernel, dim3((unsigned)((n_paths + 255) / 256)), dim3(256), 0, b->f.stream, L, (int)instance, b->d_samp,
                       b->d_thr, d_dem, d_u);
    BHIP_TRY(b, hipGetLastError());
    BHIP_TRY(b, hipMemcpyAsync(out_demand, d_dem, elems * 8, hipMemcpyDeviceToHost, b->f.stream));
    if (out_u) BHIP_TRY(b, hipMemcpyAsync(out_u, d_u, elems * 8, hipMemcpyDeviceToHost, b->f.stream));
    BHIP_TRY(b, hipStreamSynchronize(b->f.stream));
    return SDPGPU_OK;
  });
}

double sdpgpu_batch_simulate_ms(sdpgpu_batch* b) {
  if (!b) return -1.0;
  b->f.err.clear();
  if (b->staff) {
    (void)bfail(b, SDPGPU_ERR_UNSUPPORTED, "sdpgpu_batch_simulate_ms: not available on a batch of the staff family (SDPGPU_FAMILY_STAFF)");
    return -1.0;
  }
  if (!b->sim_timed) {
    (void)bfail(b, SDPGPU_ERR_STATE, "sdpgpu_batch_simulate_ms: no simulation has run");
    return -1.0;
  }
  DeviceScope dev;
  if (dev.enter(b->f.device) != hipSuccess) return -1.0;
  if (hipEventSynchronize(b->f.sim_ev1) != hipSuccess) return -1.0;
  float ms = 0;
  if (hipEventElapsedTime(&ms, b->f.sim_ev0, b->f.sim_ev1) != hipSuccess) return -1.0;
  return ms;
}

}  // extern "C"

// =================================================================================================
// (s, S) level rules: fit from the policy tables (sdp_fitss.hpp)
// =================================================================================================
namespace {

// rows [period, x, Q] of one period of an opt table, in table order
struct FitTableRows {
  const double* tab;
  const int64_t* idx;
  double x(int j) const { return tab[3 * idx[j] + 1]; }
  double q(int j) const { return tab[3 * idx[j] + 2]; }
};

// two parallel columns (sdpgpu_fit_level_index, sdpgpu_fit_min_square)
struct FitColumnRows {
  const double* xs;
  const double* qs;
  double x(int j) const { return xs[j]; }
  double q(int j) const { return qs[j]; }
};

template <int LEVELS>
int fit_table(int32_t T, double maxq, const double* tab, int64_t n_rows, double* out) {
  sdp::fit_first_period<LEVELS>(tab[1], tab[2], out);  // (optimalTable[0], whatever its period: FitsS.java:102-103)
  std::vector<int64_t> idx;
  for (int32_t t = 1; t < T; ++t) {
    idx.clear();
    for (int64_t k = 0; k < n_rows; ++k)
      if (tab[3 * k] == (double)(t + 1)) idx.push_back(k);
    if (idx.empty() || idx.size() > (size_t)INT32_MAX)
      return bfail(nullptr, SDPGPU_ERR_ARG, "sdpgpu_fit_ss: the table has %zu rows of period %d (the reference indexes an empty array there)", idx.size(), t + 1);
    sdp::fit_period<LEVELS>(FitTableRows{tab, idx.data()}, (int)idx.size(), maxq, out + (size_t)t * 2 * LEVELS);
  }
  return SDPGPU_OK;
}

// lo / hi of the reachable interval of (instance, period); needs the instance's pmfs of the periods before
int reachable_interval(sdpgpu_batch* b, const char* who, int32_t instance, int32_t period, int32_t* lo_out, int32_t* hi_out) {
  const sdpgpu_desc& d = b->d[(size_t)instance];
  const int64_t nx = b->nxs[(size_t)instance], A = b->As[(size_t)instance];
  int64_t lo = (int64_t)((d.ini_inventory - d.min_inventory) / d.step), hi = lo;
  auto clampidx = [&](int64_t v) { return v < 0 ? (int64_t)0 : (v > nx - 1 ? nx - 1 : v); };
  for (int32_t t = 0; t + 1 < period; ++t) {
    const size_t k = (size_t)instance * b->T + t;
    if (!b->pmf_set[k]) return bfail(b, SDPGPU_ERR_STATE, "%s: pmf of instance %d, period %d not set", who, instance, t + 1);
    const int64_t d0 = (int64_t)(b->d0[k] / d.step), D = (int64_t)b->pmf_p[k].size();
    lo = clampidx(lo - (d0 + D - 1));
    hi = clampidx(hi + (A - 1) - d0);
  }
  *lo_out = (int32_t)lo;
  *hi_out = (int32_t)hi;
  return SDPGPU_OK;
}

int fit_needs_unit_step(sdpgpu_batch* b, const char* who) {
  if (b->d[0].step != 1.0)
    return bfail(b, SDPGPU_ERR_UNSUPPORTED, "%s: step %g -- the fit's `s = x + 1` (FitsS.java:102) and the exact min-square sum need step == 1", who,
                 b->d[0].step);
  return SDPGPU_OK;
}

// the (instance, period) slices on the device, once
int fit_upload_pairs(sdpgpu_batch* b, const char* who) {
  if (b->d_fit_pairs) return SDPGPU_OK;
  const int N = b->N, T = b->T;
  std::vector<sdp::FitPair> pairs((size_t)N * T);
  for (int i = 0; i < N; ++i)
    for (int t = 0; t < T; ++t) {
      int32_t lo = 0, hi = 0;
      int rc = reachable_interval(b, who, i, t + 1, &lo, &hi);
      if (rc) return rc;
      pairs[(size_t)i * T + t] = sdp::FitPair{(int64_t)policy_row(b, i, t), b->d[(size_t)i].min_inventory, b->d[(size_t)i].max_order_quantity, lo, hi - lo + 1};
    }
  BHIP_TRY(b, hipMalloc((void**)&b->d_fit_pairs, pairs.size() * sizeof(sdp::FitPair)));
  BHIP_TRY(b, hipMemcpy(b->d_fit_pairs, pairs.data(), pairs.size() * sizeof(sdp::FitPair), hipMemcpyHostToDevice));
  return SDPGPU_OK;
}

// launch the fit of the whole batch into b->d_fit (n x T x 2*levels doubles, kept on the device)
int fit_launch(sdpgpu_batch* b, const char* who, int32_t levels) {
  int rc = fit_upload_pairs(b, who);
  if (rc) return rc;
  const int n_pairs = b->N * b->T;
  if (!b->d_fit) BHIP_TRY(b, hipMalloc((void**)&b->d_fit, (size_t)n_pairs * 6 * sizeof(double)));  // (room for three levels)
  const dim3 grid((unsigned)((n_pairs + 255) / 256));
  const double step = b->d[0].step;
  if (levels == 1)
    hipLaunchKernelGGL((sdp::batch_fit_ss_kernel<1>), grid, dim3(256), 0, b->f.stream, b->d_fit_pairs, n_pairs, b->T, step, b->d_policy, b->d_fit);
  else if (levels == 2)
    hipLaunchKernelGGL((sdp::batch_fit_ss_kernel<2>), grid, dim3(256), 0, b->f.stream, b->d_fit_pairs, n_pairs, b->T, step, b->d_policy, b->d_fit);
  else
    hipLaunchKernelGGL((sdp::batch_fit_ss_kernel<3>), grid, dim3(256), 0, b->f.stream, b->d_fit_pairs, n_pairs, b->T, step, b->d_policy, b->d_fit);
  BHIP_TRY(b, hipGetLastError());
  return SDPGPU_OK;
}

}  // namespace

hipError_t sdpgpu_detail::launch_fit_singles(hipStream_t st, const sdp::FitPair* d_pairs, int n_pairs, int T, const int32_t* d_policy, double* d_out) {
  hipLaunchKernelGGL((sdp::batch_fit_ss_kernel<1>), dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, d_pairs, n_pairs, T, 1.0, d_policy,
                     d_out);
  return hipGetLastError();
}

extern "C" {

int sdpgpu_batch_reachable(sdpgpu_batch* b, int32_t instance, int32_t period, int32_t* lo, int32_t* hi) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_REFUSE(b, "sdpgpu_batch_reachable");
  const char* who = "sdpgpu_batch_reachable";
  if (instance < 0 || instance >= b->N) return bfail(b, SDPGPU_ERR_ARG, "%s: instance %d outside 0 .. %d", who, instance, b->N - 1);
  if (period < 1 || period > b->T) return bfail(b, SDPGPU_ERR_ARG, "%s: period %d outside 1 .. %d", who, period, b->T);
  if (!lo || !hi) return bfail(b, SDPGPU_ERR_ARG, "%s: null output (lo, hi)", who);
  return reachable_interval(b, who, instance, period, lo, hi);
}

int sdpgpu_fit_ss(int32_t levels, int32_t T, double max_order_quantity, const double* opt_table, int64_t n_rows, double* out) {
  g_create_error.clear();
  return guarded((sdpgpu_batch*)nullptr, "sdpgpu_fit_ss", [&]() -> int {
    if (levels < 1 || levels > 3) return bfail(nullptr, SDPGPU_ERR_ARG, "sdpgpu_fit_ss: levels = %d (1, 2 or 3: getSinglesS, getTwosS, getThreesS)", levels);
    if (T < 1) return bfail(nullptr, SDPGPU_ERR_ARG, "sdpgpu_fit_ss: T = %d", T);
    if (!opt_table || !out) return bfail(nullptr, SDPGPU_ERR_ARG, "sdpgpu_fit_ss: null argument (opt_table, out)");
    if (n_rows < 1) return bfail(nullptr, SDPGPU_ERR_ARG, "sdpgpu_fit_ss: n_rows = %lld (the table holds at least the initial state's row)", (long long)n_rows);
    if (levels == 1) return fit_table<1>(T, max_order_quantity, opt_table, n_rows, out);
    if (levels == 2) return fit_table<2>(T, max_order_quantity, opt_table, n_rows, out);
    return fit_table<3>(T, max_order_quantity, opt_table, n_rows, out);
  });
}

int sdpgpu_fit_level_index(double max_order_quantity, const double* q, int32_t n, int32_t* out_index, int32_t* n_out) {
  g_create_error.clear();
  if (!q || !out_index || !n_out || n < 0) return bfail(nullptr, SDPGPU_ERR_ARG, "sdpgpu_fit_level_index: bad argument (q, out_index, n_out, n = %d)", n);
  struct {
    int32_t* out;
    int32_t count;
    void add(int j) { out[count++] = j; }
  } sink{out_index, 0};
  sdp::fit_level_walk(FitColumnRows{q, q}, n, max_order_quantity, sink);
  *n_out = sink.count;
  return SDPGPU_OK;
}

int sdpgpu_fit_min_square(double max_order_quantity, double lb, int32_t up_index, const double* x, const double* q, int32_t n, double* out) {
  g_create_error.clear();
  if (!x || !q || !out || n < 1) return bfail(nullptr, SDPGPU_ERR_ARG, "sdpgpu_fit_min_square: bad argument (x, q, out, n = %d)", n);
  if (up_index < 0 || up_index >= n) return bfail(nullptr, SDPGPU_ERR_ARG, "sdpgpu_fit_min_square: up_index %d outside 0 .. %d", up_index, n - 1);
  *out = sdp::fit_min_square(FitColumnRows{x, q}, n, max_order_quantity, lb, up_index);
  return SDPGPU_OK;
}

int sdpgpu_batch_fit_ss(sdpgpu_batch* b, int32_t levels, double* out) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_REFUSE(b, "sdpgpu_batch_fit_ss");
  return guarded(b, "sdpgpu_batch_fit_ss", [&]() -> int {
    const char* who = "sdpgpu_batch_fit_ss";
    if (levels < 1 || levels > 3) return bfail(b, SDPGPU_ERR_ARG, "%s: levels = %d (1, 2 or 3: getSinglesS, getTwosS, getThreesS)", who, levels);
    if (!out) return bfail(b, SDPGPU_ERR_ARG, "%s: out is null", who);
    int rc = fit_needs_unit_step(b, who);
    if (rc) return rc;
    if (!b->solved) return bfail(b, SDPGPU_ERR_STATE, "%s before sdpgpu_batch_solve", who);
    DeviceScope dev;
    BHIP_TRY(b, dev.enter(b->f.device));
    rc = fit_launch(b, who, levels);
    if (rc) return rc;
    BHIP_TRY(b, hipMemcpyAsync(out, b->d_fit, (size_t)b->N * b->T * 2 * levels * sizeof(double), hipMemcpyDeviceToHost, b->f.stream));
    BHIP_TRY(b, hipStreamSynchronize(b->f.stream));
    return SDPGPU_OK;
  });
}

}  // extern "C"

// =================================================================================================
// The rollouts: the table policy or a level rule along given or drawn demand paths (batch_sim_kernel, sdp_batch_sim.hpp)
// =================================================================================================
namespace {

// What a call rolls: the solved policy tables, or a rule of `levels` (s, S) pairs -- the caller's `ss`, or with ss == NULL the
// fit of the tables, made on the device inside the call.
struct SimRule {
  bool table;
  int32_t levels;
  const double* ss;
};

template <class RULE>
void sim_launch(sdpgpu_batch* b, bool sampled, dim3 grid, const sdp::SimLaunch& L, const double* d_ini, RULE rule, const double* d_dem,
                double* d_part, double* d_sum) {
  if (sampled)
    hipLaunchKernelGGL((sdp::batch_sim_kernel<RULE, true>), grid, dim3(256), 0, b->f.stream, L, b->d_sim_inst, d_ini, rule, nullptr, b->d_samp,
                       b->d_thr, d_part, d_sum);
  else
    hipLaunchKernelGGL((sdp::batch_sim_kernel<RULE, false>), grid, dim3(256), 0, b->f.stream, L, b->d_sim_inst, d_ini, rule, d_dem, nullptr,
                       nullptr, d_part, d_sum);
}

int sim_run(sdpgpu_batch* b, const char* who, SimRule rule, int32_t n_paths, const double* demand, int64_t stride, bool sampled, uint64_t seed,
            const double* ini_x, double* out_mean, double* out_sum) {
  const int N = b->N, T = b->T;
  const int32_t levels = rule.levels;
  if (!rule.table && (levels < 1 || levels > 3))
    return bfail(b, SDPGPU_ERR_ARG, "%s: levels = %d (1, 2 or 3: simulateSinglesS, simulateTwosS, simulateThreesS)", who, levels);
  std::vector<double> ini;
  int rc = sim_check_args(b, who, n_paths, demand, stride, sampled, ini_x, out_mean, &ini);
  if (rc) return rc;
  // The tables must exist for the table policy and for a fit; an explicit rule may be rolled on an unsolved batch, whose
  // tables layout() and allocate() below then make (after a solve both return at once).
  if (rule.table) {
    if (!b->solved) return bfail(b, SDPGPU_ERR_STATE, "%s before sdpgpu_batch_solve", who);
  } else if (!rule.ss) {  // fit first, in this call
    if ((rc = fit_needs_unit_step(b, who))) return rc;
    if (!b->solved) return bfail(b, SDPGPU_ERR_STATE, "%s: ss = NULL fits the rule from the policy tables: before sdpgpu_batch_solve", who);
  }
  rc = layout(b);  // (every pmf set)
  if (rc) return rc;
  const int64_t wpi = (n_paths + 63) / 64;
  const int64_t waves = (int64_t)N * wpi;
  if (!grid_ok((waves + 3) / 4) || (double)N * n_paths > 2.0e9)
    return bfail(b, SDPGPU_ERR_UNSUPPORTED, "%s: %d instances x %d paths are too many for one launch", who, N, n_paths);

  DeviceScope dev;
  BHIP_TRY(b, dev.enter(b->f.device));
  rc = allocate(b);
  if (rc) return rc;
  if (!b->d_sim_inst) {
    std::vector<sdp::SimInst> inst((size_t)N);
    for (int i = 0; i < N; ++i) {
      const sdpgpu_desc& d = b->d[(size_t)i];
      inst[(size_t)i] = sdp::SimInst{d.holding_cost, d.penalty_cost, d.fixed_order_cost, d.unit_order_cost, d.min_inventory, d.max_inventory,
                                     d.max_order_quantity, (int64_t)policy_row(b, i, 0), b->nxs[(size_t)i], 0};
    }
    BHIP_TRY(b, hipMalloc((void**)&b->d_sim_inst, inst.size() * sizeof(sdp::SimInst)));
    BHIP_TRY(b, hipMemcpy(b->d_sim_inst, inst.data(), inst.size() * sizeof(sdp::SimInst), hipMemcpyHostToDevice));
  }
  if (!b->f.sim_ev0) {
    BHIP_TRY(b, hipEventCreate(&b->f.sim_ev0));
    BHIP_TRY(b, hipEventCreate(&b->f.sim_ev1));
  }
  if (sampled && (rc = sim_upload_samplers(b))) return rc;
  const size_t ss_elems = rule.ss ? (size_t)N * T * 2 * levels : 0;
  const size_t sum_bytes = out_sum ? (size_t)N * n_paths * 8 : 0;
  const size_t dem_elems = sampled ? 0 : (stride == 0 ? (size_t)n_paths * T : (size_t)(N - 1) * (size_t)stride + (size_t)n_paths * T);
  Carve c;
  const size_t o_ini = c.take((size_t)N * 8), o_part = c.take((size_t)waves * 8), o_mean = c.take((size_t)N * 8);
  const size_t o_sum = c.take(sum_bytes), o_ss = c.take(ss_elems * 8), o_dem = c.take(dem_elems * 8);
  rc = sim_scratch(&b->f, c.at);
  if (rc) return rc;
  char* base = b->f.d_sim_scratch;
  double* d_ini = reinterpret_cast<double*>(base + o_ini);
  double* d_part = reinterpret_cast<double*>(base + o_part);
  double* d_mean = reinterpret_cast<double*>(base + o_mean);
  double* d_sum = out_sum ? reinterpret_cast<double*>(base + o_sum) : nullptr;
  const double* d_rule = reinterpret_cast<double*>(base + o_ss);
  double* d_dem = sampled ? nullptr : reinterpret_cast<double*>(base + o_dem);
  BHIP_TRY(b, hipMemcpyAsync(d_ini, ini.data(), (size_t)N * 8, hipMemcpyHostToDevice, b->f.stream));
  if (rule.ss) BHIP_TRY(b, hipMemcpyAsync(base + o_ss, rule.ss, ss_elems * 8, hipMemcpyHostToDevice, b->f.stream));
  if (!sampled) BHIP_TRY(b, hipMemcpyAsync(d_dem, demand, dem_elems * 8, hipMemcpyHostToDevice, b->f.stream));
  const sdp::SimLaunch L = sim_launch_params(b, n_paths, seed, stride);
  const dim3 grid((unsigned)((waves + 3) / 4));
  BHIP_TRY(b, hipEventRecord(b->f.sim_ev0, b->f.stream));
  if (!rule.table && !rule.ss) {
    rc = fit_launch(b, who, levels);
    if (rc) return rc;
    d_rule = b->d_fit;
  }
  if (rule.table)
    sim_launch(b, sampled, grid, L, d_ini, sdp::TableRule{b->d_policy}, d_dem, d_part, d_sum);
  else if (levels == 1)
    sim_launch(b, sampled, grid, L, d_ini, sdp::LevelRule<1>{d_rule}, d_dem, d_part, d_sum);
  else if (levels == 2)
    sim_launch(b, sampled, grid, L, d_ini, sdp::LevelRule<2>{d_rule}, d_dem, d_part, d_sum);
  else
    sim_launch(b, sampled, grid, L, d_ini, sdp::LevelRule<3>{d_rule}, d_dem, d_part, d_sum);
  BHIP_TRY(b, hipGetLastError());
  hipLaunchKernelGGL(sdp::batch_sim_mean_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, b->f.stream, d_part, N, (int)wpi, n_paths, d_mean);
  BHIP_TRY(b, hipGetLastError());
  BHIP_TRY(b, hipEventRecord(b->f.sim_ev1, b->f.stream));
  b->sim_timed = true;
  BHIP_TRY(b, hipMemcpyAsync(out_mean, d_mean, (size_t)N * 8, hipMemcpyDeviceToHost, b->f.stream));
  if (out_sum) BHIP_TRY(b, hipMemcpyAsync(out_sum, d_sum, sum_bytes, hipMemcpyDeviceToHost, b->f.stream));
  BHIP_TRY(b, hipStreamSynchronize(b->f.stream));
  return SDPGPU_OK;
}

// the four entry points differ in the rule and in where the demands come from
int sim_entry(sdpgpu_batch* b, const char* who, SimRule rule, int32_t n_paths, const double* demand, int64_t stride, bool sampled, uint64_t seed,
              const double* ini_x, double* out_mean, double* out_sum) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  if (b->staff)
    return bfail(b, SDPGPU_ERR_UNSUPPORTED, "%s: not available on a batch of the staff family (SDPGPU_FAMILY_STAFF): a hiring rule is rolled out on a "
                 "sampled tree (sdpgpu_batch_staff_simulate)", who);
  return guarded(b, who, [&]() -> int { return sim_run(b, who, rule, n_paths, demand, stride, sampled, seed, ini_x, out_mean, out_sum); });
}

}  // namespace

extern "C" {

int sdpgpu_batch_simulate(sdpgpu_batch* b, int32_t n_paths, const double* demand, int64_t instance_stride, const double* ini_x,
                          double* out_mean, double* out_sum) {
  return sim_entry(b, "sdpgpu_batch_simulate", SimRule{true, 0, nullptr}, n_paths, demand, instance_stride, false, 0, ini_x, out_mean, out_sum);
}

int sdpgpu_batch_simulate_sampled(sdpgpu_batch* b, int32_t n_paths, uint64_t seed, const double* ini_x, double* out_mean, double* out_sum) {
  return sim_entry(b, "sdpgpu_batch_simulate_sampled", SimRule{true, 0, nullptr}, n_paths, nullptr, 0, true, seed, ini_x, out_mean, out_sum);
}

int sdpgpu_batch_simulate_ss(sdpgpu_batch* b, int32_t levels, const double* ss, int32_t n_paths, const double* demand, int64_t instance_stride,
                             const double* ini_x, double* out_mean, double* out_sum) {
  return sim_entry(b, "sdpgpu_batch_simulate_ss", SimRule{false, levels, ss}, n_paths, demand, instance_stride, false, 0, ini_x, out_mean, out_sum);
}

int sdpgpu_batch_simulate_ss_sampled(sdpgpu_batch* b, int32_t levels, const double* ss, int32_t n_paths, uint64_t seed, const double* ini_x,
                                     double* out_mean, double* out_sum) {
  return sim_entry(b, "sdpgpu_batch_simulate_ss_sampled", SimRule{false, levels, ss}, n_paths, nullptr, 0, true, seed, ini_x, out_mean, out_sum);
}

}  // extern "C"

// =================================================================================================
// Structure checks: the G rows of a solved batch, K- and CK-convexity of its rows (sdp_structure.hpp)
// =================================================================================================
namespace {

static_assert(sizeof(sdp::ConvexityOut) == sizeof(sdpgpu_convexity) && offsetof(sdp::ConvexityOut, lhs) == offsetof(sdpgpu_convexity, lhs) &&
                  offsetof(sdp::ConvexityOut, rhs) == offsetof(sdpgpu_convexity, rhs) && offsetof(sdp::ConvexityOut, i2) == offsetof(sdpgpu_convexity, i2),
              "sdp::ConvexityOut is sdpgpu_convexity field for field");

// G_period exists when V_{period+1} does: every period with store_all_values, else period 1 (V_2 survives) and period T
bool gy_period_kept(const sdpgpu_batch* b, int32_t period) { return b->d[0].store_all_values || period == b->T || period == 1; }

// the G rows of every (instance, period) on the device, once per solve
int gy_fill(sdpgpu_batch* b) {
  if (b->gy_valid) return SDPGPU_OK;
  const int N = b->N, T = b->T;
  if (!b->d_gy_pairs) {
    std::vector<sdp::GyPair> pairs((size_t)N * T);
    for (int i = 0; i < N; ++i)
      for (int t = 0; t < T; ++t) {
        const sdpgpu_desc& d = b->d[(size_t)i];
        const size_t k = (size_t)i * T + t;
        sdp::GyPair P{};
        P.pmf_off = (int64_t)b->pmf_off[k];
        P.v_next_off = t + 1 < T ? (int64_t)value_row(b, i, t + 1) : -1;
        P.out_off = (int64_t)policy_row(b, i, t);
        P.x_min = d.min_inventory;
        P.x_max = d.max_inventory;
        P.d0 = b->d0[k];
        P.h = d.holding_cost;
        P.pi = d.penalty_cost;
        P.v = d.unit_order_cost;
        P.nx = gy_period_kept(b, t + 1) ? b->nxs[(size_t)i] : 0;  // (a row whose V_{t+1} is gone is not made)
        P.n_demand = (int32_t)b->pmf_p[k].size();
        pairs[k] = P;
      }
    BHIP_TRY(b, hipMalloc((void**)&b->d_gy_pairs, pairs.size() * sizeof(sdp::GyPair)));
    BHIP_TRY(b, hipMemcpy(b->d_gy_pairs, pairs.data(), pairs.size() * sizeof(sdp::GyPair), hipMemcpyHostToDevice));
  }
  if (!b->d_gy) BHIP_TRY(b, hipMalloc((void**)&b->d_gy, std::max<size_t>(b->policy_elems, 1) * sizeof(double)));
  if (!grid_ok((int64_t)N * T)) return bfail(b, SDPGPU_ERR_UNSUPPORTED, "G rows: %d instances x %d periods are too many for one launch", N, T);
  const double step = b->d[0].step;
  hipLaunchKernelGGL(sdp::gy_kernel, dim3((unsigned)(N * T)), dim3(256), 0, b->f.stream, b->d_gy_pairs, step, 1.0 / step, b->d_pmf, b->d_values,
                     b->d_gy);
  BHIP_TRY(b, hipGetLastError());
  b->gy_valid = true;
  return SDPGPU_OK;
}

int convexity_kind_check(sdpgpu_batch* b, const char* who, int32_t kind) {
  if (kind != sdp::kConvexityCheck && kind != sdp::kConvexityCheckCK)
    return bfail(b, SDPGPU_ERR_ARG, "%s: kind = %d (0: CheckKConvexity.check, 1: CheckKConvexity.checkCK)", who, kind);
  return SDPGPU_OK;
}

// The device part of a check, for the rows of a batch and (convexity_on_device) of a staff handle: the tasks of the rows, the
// carving of ONE scratch block, and the launches behind its uploads.
struct ConvexityWork {
  std::vector<sdp::ConvexityTask> tasks;
  int n_max = 1;
  size_t o_rows = 0, o_tasks = 0, o_keys = 0, o_out = 0, bytes = 0;
};

double convexity_triples(const sdp::ConvexityRow& R) {
  double triples = 0;
  for (int o = 0; o < R.n; ++o)
    triples += (double)(R.kind == sdp::kConvexityCheck ? sdp::convexity_count<sdp::kConvexityCheck>(R.n, R.capacity, o)
                                                       : sdp::convexity_count<sdp::kConvexityCheckCK>(R.n, R.capacity, o));
  return triples;
}

void convexity_plan(int kind, const std::vector<sdp::ConvexityRow>& rows, double triples, ConvexityWork* w) {
  // tiles of about equal triple counts: enough of them to fill the device several times over, none below what pays for
  // staging its row
  const int64_t target = (int64_t)std::min(std::max(triples / 16384.0, 16384.0), 4194304.0);
  for (size_t i = 0; i < rows.size(); ++i) {
    sdp::convexity_tasks((int32_t)i, kind, rows[i].n, rows[i].capacity, target, &w->tasks);
    w->n_max = std::max(w->n_max, (int)rows[i].n);
  }
  Carve c;
  w->o_rows = c.take(rows.size() * sizeof(sdp::ConvexityRow));
  w->o_tasks = c.take(std::max<size_t>(w->tasks.size(), 1) * sizeof(sdp::ConvexityTask));
  w->o_keys = c.take(rows.size() * 8);
  w->o_out = c.take(rows.size() * sizeof(sdp::ConvexityOut));
  w->bytes = c.at;
}

// rows (their g set) and tasks go up, the key fill, the check and the finish run, the structs come down: all on `st`, which the
// caller synchronises before it reads host_out.  sb: w.bytes of device memory.
hipError_t convexity_launch(hipStream_t st, const std::vector<sdp::ConvexityRow>& rows, const ConvexityWork& w, char* sb, sdp::ConvexityOut* host_out) {
  const int N = (int)rows.size();
  sdp::ConvexityRow* d_rows = reinterpret_cast<sdp::ConvexityRow*>(sb + w.o_rows);
  sdp::ConvexityTask* d_tasks = reinterpret_cast<sdp::ConvexityTask*>(sb + w.o_tasks);
  unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(sb + w.o_keys);
  sdp::ConvexityOut* d_out = reinterpret_cast<sdp::ConvexityOut*>(sb + w.o_out);
  hipError_t e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(sdp::ConvexityRow), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  if (!w.tasks.empty() && (e = hipMemcpyAsync(d_tasks, w.tasks.data(), w.tasks.size() * sizeof(sdp::ConvexityTask), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  const dim3 per_row((unsigned)((N + 255) / 256));
  hipLaunchKernelGGL(sdp::convexity_key_fill_kernel, per_row, dim3(256), 0, st, d_keys, N);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (!w.tasks.empty()) {
    static LdsMark mark;
    const size_t smem = sdp::convexity_lds(w.n_max);
    if ((e = lds_allow(sdp::convexity_kernel, smem, &mark)) != hipSuccess) return e;
    hipLaunchKernelGGL(sdp::convexity_kernel, dim3((unsigned)w.tasks.size()), dim3(256), smem, st, d_rows, d_tasks, d_keys);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(sdp::convexity_finish_kernel, per_row, dim3(256), 0, st, d_rows, d_keys, N, d_out);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipMemcpyAsync(host_out, d_out, (size_t)N * sizeof(sdp::ConvexityOut), hipMemcpyDeviceToHost, st);
}

int batch_check_convexity(sdpgpu_batch* b, int32_t kind, int32_t source, int32_t period, const double* x_lo, const double* x_hi, const double* K,
                          const int32_t* capacity, sdpgpu_convexity* out) {
  const char* who = "sdpgpu_batch_check_convexity";
  const int N = b->N;
  int rc = convexity_kind_check(b, who, kind);
  if (rc) return rc;
  if (source != 0 && source != 1) return bfail(b, SDPGPU_ERR_ARG, "%s: source = %d (0: the value rows V_period, 1: the rows G_period)", who, source);
  if (period < 1 || period > b->T) return bfail(b, SDPGPU_ERR_ARG, "%s: period %d outside 1 .. %d", who, period, b->T);
  if (!out) return bfail(b, SDPGPU_ERR_ARG, "%s: out is null", who);
  if ((x_lo == nullptr) != (x_hi == nullptr)) return bfail(b, SDPGPU_ERR_ARG, "%s: x_lo and x_hi are given together, or both NULL (the whole grid)", who);
  const double step = b->d[0].step;
  if (kind == sdp::kConvexityCheckCK && !capacity && step != 1.0)
    return bfail(b, SDPGPU_ERR_ARG, "%s: capacity = NULL means (int)max_order_quantity grid points, which holds with step == 1 only (step %g): pass "
                 "the capacities explicitly", who, step);
  if (!b->solved) return bfail(b, SDPGPU_ERR_STATE, "%s before sdpgpu_batch_solve", who);
  if (source == 0 && !b->d[0].store_all_values && period > 2)
    return bfail(b, SDPGPU_ERR_STATE, "%s: V_%d was overwritten (store_all_values = 0 keeps two ping-pong tables: periods 1 and 2 survive)", who, period);
  if (source == 1 && !gy_period_kept(b, period))
    return bfail(b, SDPGPU_ERR_STATE, "%s: G_%d needs V_%d, which was overwritten (store_all_values = 0 keeps G_1 and G_%d)", who, period, period + 1, b->T);
  // the rows: a window of every instance's row, its K, its capacity
  std::vector<int64_t> row_off((size_t)N);
  std::vector<sdp::ConvexityRow> rows((size_t)N);
  double triples = 0;
  for (int i = 0; i < N; ++i) {
    const sdpgpu_desc& d = b->d[(size_t)i];
    const int64_t nx = b->nxs[(size_t)i];
    int64_t lo = 0, hi = nx - 1;
    if (x_lo) {
      const double a = x_lo[i], c = x_hi[i];
      if (!(a >= d.min_inventory && c <= d.max_inventory && a <= c) || std::fmod(a, step) != 0 || std::fmod(c, step) != 0)
        return bfail(b, SDPGPU_ERR_ARG, "%s: instance %d: the window [%g, %g] is not a run of points of its grid [%g, %g]", who, i, a, c,
                     d.min_inventory, d.max_inventory);
      lo = (int64_t)((a - d.min_inventory) / step);
      hi = (int64_t)((c - d.min_inventory) / step);
    }
    const int64_t n = hi - lo + 1;
    if (n > sdp::kConvexityMaxRow)
      return bfail(b, SDPGPU_ERR_UNSUPPORTED, "%s: instance %d: a row of %lld points exceeds the kernel's %d (a workgroup keeps the row in LDS): "
                   "narrow the window", who, i, (long long)n, sdp::kConvexityMaxRow);
    sdp::ConvexityRow R{};
    row_off[(size_t)i] = (int64_t)(source == 0 ? value_row(b, i, period - 1) : policy_row(b, i, period - 1)) + lo;
    R.K = K ? K[i] : d.fixed_order_cost;
    R.n = (int32_t)n;
    R.capacity = capacity ? capacity[i] : (int32_t)d.max_order_quantity;
    R.kind = kind;
    rows[(size_t)i] = R;
    triples += convexity_triples(R);
  }
  ConvexityWork w;
  convexity_plan(kind, rows, triples, &w);
  if (w.tasks.size() > (size_t)INT32_MAX / 2) return bfail(b, SDPGPU_ERR_UNSUPPORTED, "%s: too many tasks in one launch", who);

  DeviceScope dev;
  BHIP_TRY(b, dev.enter(b->f.device));
  if (source == 1 && (rc = gy_fill(b))) return rc;
  const double* base = source == 0 ? b->d_values : b->d_gy;
  for (int i = 0; i < N; ++i) rows[(size_t)i].g = base + row_off[(size_t)i];
  rc = sim_scratch(&b->f, w.bytes);
  if (rc) return rc;
  std::vector<sdp::ConvexityOut> host((size_t)N);  // (out is written only once everything has succeeded)
  BHIP_TRY(b, convexity_launch(b->f.stream, rows, w, b->f.d_sim_scratch, host.data()));
  BHIP_TRY(b, hipStreamSynchronize(b->f.stream));
  std::memcpy(out, host.data(), host.size() * sizeof(sdp::ConvexityOut));
  return SDPGPU_OK;
}

}  // namespace

static_assert(sdpgpu_detail::kConvexityMaxPoints == sdp::kConvexityMaxRow, "the limit the staff units refuse by is the kernel's");

// sdpgpu_sim_host.hpp: the check on rows that already lie on the device, for the staff units
int sdpgpu_detail::convexity_on_device(hipStream_t st, int32_t kind, const ConvexitySpec* specs, int32_t n_rows, sdpgpu_convexity* out, std::string* why) {
  std::vector<sdp::ConvexityRow> rows((size_t)n_rows);
  double triples = 0;
  for (int i = 0; i < n_rows; ++i) {
    if (specs[i].n > sdp::kConvexityMaxRow)
      return fail_to(why, SDPGPU_ERR_UNSUPPORTED, "row %d: %d points exceed the kernel's %d (a workgroup keeps the row in LDS): narrow the window", i,
                     specs[i].n, sdp::kConvexityMaxRow);
    sdp::ConvexityRow R{};
    R.g = specs[i].g;
    R.K = specs[i].K;
    R.n = specs[i].n;
    R.capacity = specs[i].capacity;
    R.kind = kind;
    rows[(size_t)i] = R;
    triples += convexity_triples(R);
  }
  ConvexityWork w;
  convexity_plan(kind, rows, triples, &w);
  if (w.tasks.size() > (size_t)INT32_MAX / 2) return fail_to(why, SDPGPU_ERR_UNSUPPORTED, "too many tasks in one launch");
  struct Block {
    char* p = nullptr;
    ~Block() {
      if (p) (void)hipFree(p);
    }
  } blk;
  hipError_t e = hipMalloc((void**)&blk.p, w.bytes);
  std::vector<sdp::ConvexityOut> host((size_t)n_rows);  // (out is written only once everything has succeeded)
  if (e == hipSuccess) e = convexity_launch(st, rows, w, blk.p, host.data());
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail_to(why, SDPGPU_ERR_DEVICE, "convexity check: %s", hipGetErrorString(e));
  std::memcpy(out, host.data(), host.size() * sizeof(sdp::ConvexityOut));
  return SDPGPU_OK;
}

extern "C" {

int sdpgpu_check_convexity(int32_t kind, const double* g, int64_t n, double K, int32_t capacity, sdpgpu_convexity* out) {
  g_create_error.clear();
  return guarded((sdpgpu_batch*)nullptr, "sdpgpu_check_convexity", [&]() -> int {
    const char* who = "sdpgpu_check_convexity";
    int rc = convexity_kind_check(nullptr, who, kind);
    if (rc) return rc;
    if (!out || n < 0 || (n > 0 && !g)) return bfail(nullptr, SDPGPU_ERR_ARG, "%s: bad argument (g, out, n = %lld)", who, (long long)n);
    if (n >= (1 << 21)) return bfail(nullptr, SDPGPU_ERR_UNSUPPORTED, "%s: a row of %lld points (below %d)", who, (long long)n, 1 << 21);
    sdp::ConvexityOut r;
    sdp::convexity_host(kind, g, (int)n, K, capacity, &r);
    std::memcpy(out, &r, sizeof r);
    return SDPGPU_OK;
  });
}

int sdpgpu_batch_gy(sdpgpu_batch* b, int32_t instance, int32_t period, double* out, int64_t n) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_REFUSE(b, "sdpgpu_batch_gy");
  return guarded(b, "sdpgpu_batch_gy", [&]() -> int {
    const char* who = "sdpgpu_batch_gy";
    int rc = read_check(b, who, instance, period, out, n, false);
    if (rc) return rc;
    if (!gy_period_kept(b, period))
      return bfail(b, SDPGPU_ERR_STATE, "%s: G_%d needs V_%d, which was overwritten (store_all_values = 0 keeps G_1 and G_%d)", who, period, period + 1, b->T);
    DeviceScope dev;
    BHIP_TRY(b, dev.enter(b->f.device));
    rc = gy_fill(b);
    if (rc) return rc;
    BHIP_TRY(b, hipStreamSynchronize(b->f.stream));
    BHIP_TRY(b, hipMemcpy(out, b->d_gy + policy_row(b, instance, period - 1), (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return SDPGPU_OK;
  });
}

int sdpgpu_batch_check_convexity(sdpgpu_batch* b, int32_t kind, int32_t source, int32_t period, const double* x_lo, const double* x_hi,
                                 const double* K, const int32_t* capacity, sdpgpu_convexity* out) {
  if (!b) return SDPGPU_ERR_ARG;
  b->f.err.clear();
  STAFF_REFUSE(b, "sdpgpu_batch_check_convexity");
  return guarded(b, "sdpgpu_batch_check_convexity",
                 [&]() -> int { return batch_check_convexity(b, kind, source, period, x_lo, x_hi, K, capacity, out); });
}

}  // extern "C"
