// sdpgpu_staffbatch.hip -- a BATCH of STAFF-family instances of one shape in the opt-in separable mode (include/sdpgpu.h,
// "batched workforce solve"): the sweep of workforce.WorkforceTesting.main -- 216 instances of T = 8, hires 0..1000, no clamp,
// two turnover tables.  Period t of ALL instances runs in two launches (sdp_staff_batch.hpp): the rows G and P of every
// instance, then the scan.  This unit holds the pool of level tables, the validation, the host layout (per-period boxes,
// groups of instances per (period, table), instance blocks), the plan, the launcher and what the entry points of
// sdpgpu_batch.hip forward to on a batch whose instance 0 is of the STAFF family -- and, at the end, the rest of the sweep's loop
// body for all instances: the visited staff numbers, the (s, S) fit on the device and the rollout of hiring rules on a sampled
// tree (sdp_staff_batch_sim.hpp) on the shared host frame.  Stream, events, staging block and error text are the BatchFrame of
// the sdpgpu_batch that holds this batch (sdpgpu_batch_frame.hpp); only the create-time refusals go to the caller's string.
#include "sdpgpu_batch_frame.hpp"
#include "sdp_fit_pair.hpp"
#include "sdp_staff_batch.hpp"
#include "sdp_staff_batch_sim.hpp"
#include "sdp_staff_structure.hpp"

#include <map>

namespace sdpgpu_detail {

int validate(const sdpgpu_desc& d);               // sdpgpu.hip
int32_t full_action_count(const sdpgpu_desc& d);  // sdpgpu.hip

namespace {

// launch of one period for the whole batch
struct PeriodPlan {
  int tables = 0;          // distinct tables = groups of instances
  int R = 1, U = sdp::kStaffBatchU1;
  int64_t blocks = 0;      // instance blocks: sum over groups of ceil(size / R)
  int64_t g_blocks = 0;    // waves of 64 levels per block
  int64_t tiles = 0;       // workgroups of 64 states per instance
  int longest_row = 0;
};

struct Table {
  std::vector<double> p;  // transposed: p[j * rows + y], zero behind a row's length
  std::vector<int32_t> len;
  int32_t rows = 0, maxj = 0;
  bool nonneg = false;    // staff_batch_simulate has looked at the table and found no negative or NaN entry
};

}  // namespace

struct StaffBatch {
  BatchFrame* f = nullptr;         // of the sdpgpu_batch that holds this batch
  std::vector<sdpgpu_desc> d;
  int32_t N = 0, T = 0, A = 0;
  std::vector<Table> pool;
  std::vector<int32_t> use;        // [i * T + t]: pool id, -1 = none yet
  std::vector<double> min_staff;   // [i * T + t]
  std::vector<char> min_set;
  bool laid_out = false, allocated = false, solved = false;
  std::vector<int64_t> x_lo, nx, row_pre;  // [t]: the period's box (shared by the instances), prefix sums of nx
  int64_t sum_nx = 0, nx_max = 0, lev_max = 0;
  std::vector<PeriodPlan> plan;            // [t]
  std::vector<sdp::StaffBatchInst> inst;   // [t * N + i]
  std::vector<int32_t> blk;                // the periods' instance blocks, one after the other (R entries a block)
  std::vector<size_t> blk_off;             // [t]
  int64_t cells = 0;
  // device
  std::vector<void*> owned;                // pool tables and row lengths
  sdp::StaffBatchTable* d_tabs = nullptr;
  sdp::StaffBatchInst* d_inst = nullptr;
  int32_t* d_blk = nullptr;
  double* d_values = nullptr;
  int32_t* d_policy = nullptr;
  double* d_gp = nullptr;                  // [N][2][lev_max]
  int32_t period_launches = 0, periods_run = 0;
  // ---- fit and rollout (staff_batch_fit_ss, staff_batch_simulate) ----
  std::vector<int64_t> reach_lo, reach_hi;  // [i * T + t]: the reachable intervals, made once the tables are frozen
  sdp::FitPair* d_fit_pairs = nullptr;      // [i * T + t]
  double* d_fit = nullptr;                  // N x T x 2
  // ---- structure rows (staff_batch_gy, staff_batch_check_convexity; sdp_staff_structure.hpp) ----
  bool inst_stale = false;                  // minStaffNum changed behind the device copy of `inst`: the next solve uploads it again
  bool gy_valid = false;                    // the G rows below are those of the tables the last solve left
  std::vector<size_t> gy_off;               // [i * T + t]: the row of (instance, period) in d_gy, one entry per table row
  std::vector<int32_t> gy_lo, gy_hi;        // [i * T + t]: the levels made -- the first run that is not off the grid (lo > hi: none)
  std::vector<sdp::StaffGyRow> gy_rows;     // the upload sources of the one launch, kept while the stream may read them
  std::vector<sdp::StaffGyBlock> gy_blocks;
  char* d_gy = nullptr;                     // [the rows' doubles][the records][the blocks]
};

namespace {

size_t value_row(const StaffBatch* s, int i, int t) {
  if (s->d[0].store_all_values) return (size_t)i * (size_t)s->sum_nx + (size_t)s->row_pre[(size_t)t];
  return ((size_t)i * 2 + (size_t)(t & 1)) * (size_t)s->nx_max;  // two ping-pong tables per instance: V_1 and V_2 survive
}
size_t policy_row(const StaffBatch* s, int i, int t) { return (size_t)i * (size_t)s->sum_nx + (size_t)s->row_pre[(size_t)t]; }

// The box of every period.  Clamped: [minX, maxX] throughout.  Unclamped: as a handle lays it out (layout, sdpgpu.hip) -- from
// [ini, ini], lower end down by the longest row of the period's table less one (never below 0), upper end up by the hire limit.
// The lower end reads instance i's tables of the periods before `upto`; -1 in *missing_t: all were there.
void boxes_of(const StaffBatch* s, int i, int upto, std::vector<int64_t>* lo_out, std::vector<int64_t>* nx_out, int* missing_t) {
  const sdpgpu_desc& d = s->d[0];
  *missing_t = -1;
  lo_out->assign((size_t)upto, 0);
  nx_out->assign((size_t)upto, 0);
  int64_t lo = (int64_t)d.min_inventory, hi = (int64_t)d.max_inventory;
  if (!d.clamp_inventory) lo = hi = (int64_t)d.ini_inventory;
  for (int t = 0; t < upto; ++t) {
    (*lo_out)[(size_t)t] = lo;
    (*nx_out)[(size_t)t] = hi - lo + 1;
    if (d.clamp_inventory || t + 1 == upto) continue;
    const int32_t id = s->use[(size_t)i * s->T + t];
    if (id < 0) {
      *missing_t = t;
      return;
    }
    lo = std::max<int64_t>(0, lo - (s->pool[(size_t)id].maxj - 1));
    hi += s->A - 1;
  }
}

// sum over the states of a period and the actions of pmfs[t][min(x + a, rows - 1)].length (staff_cells, sdpgpu_staff.hip)
int64_t cells_of(const Table& tb, int64_t x0, int64_t nx, int64_t nA) {
  const int64_t rows = tb.rows;
  std::vector<int64_t> pre((size_t)rows + 1, 0);
  for (int64_t y = 0; y < rows; ++y) pre[(size_t)y + 1] = pre[(size_t)y] + tb.len[(size_t)y];
  auto upto = [&](int64_t y) { return y <= rows ? pre[(size_t)y] : pre[(size_t)rows] + (y - rows) * (int64_t)tb.len[(size_t)rows - 1]; };
  int64_t cells = 0;
  for (int64_t i = 0; i < nx; ++i) cells += upto(x0 + i + nA) - upto(x0 + i);
  return cells;
}

int layout(StaffBatch* s) {
  if (s->laid_out) return SDPGPU_OK;
  const int N = s->N, T = s->T;
  const sdpgpu_desc& d0 = s->d[0];
  for (int i = 0; i < N; ++i)
    for (int t = 0; t < T; ++t)
      if (s->use[(size_t)i * T + t] < 0)
        return s->f->fail(SDPGPU_ERR_STATE, "level table of instance %d, period %d not set (sdpgpu_batch_use_level_pmf)", i, t + 1);
  for (int i = 0; i < N; ++i)
    for (int t = 0; t < T; ++t) {
      const size_t k = (size_t)i * T + t;
      if (!s->min_set[k]) s->min_staff[k] = s->d[(size_t)i].overhead_cost;
      const double m = s->min_staff[k];
      if (m != std::floor(m) || std::fabs(m) > 1e9)
        return s->f->fail(SDPGPU_ERR_ARG, "minStaffNum of instance %d, period %d (sdpgpu_batch_set_overhead) must be an integer", i, t + 1);
    }
  int missing = -1;
  boxes_of(s, 0, T, &s->x_lo, &s->nx, &missing);
  if (!d0.clamp_inventory) {  // the boxes are common to the batch: every instance's tables must grow the same ones
    std::vector<int64_t> lo, nx;
    for (int i = 1; i < N; ++i) {
      boxes_of(s, i, T, &lo, &nx, &missing);
      for (int t = 0; t < T; ++t)
        if (lo[(size_t)t] != s->x_lo[(size_t)t])
          return s->f->fail(SDPGPU_ERR_UNSUPPORTED, "instance %d: its level tables put the staff range of period %d at %lld .., instance 0's at %lld .. "
                       "(clamp_inventory = 0: the longest rows of the tables of a period must leave the instances one staff range)",
                       i, t + 1, (long long)lo[(size_t)t], (long long)s->x_lo[(size_t)t]);
    }
  }
  s->row_pre.assign((size_t)T, 0);
  s->sum_nx = s->nx_max = s->lev_max = 0;
  for (int t = 0; t < T; ++t) {
    const int64_t nx = s->nx[(size_t)t], levels = nx + s->A - 1;
    // (levels and staff numbers are 32-bit in the kernels, V_{t+1} is addressed by 32-bit byte offsets)
    if (nx >= 2147483647LL || levels >= 2147483647LL || s->x_lo[(size_t)t] + levels >= 2147483647LL)
      return s->f->fail(SDPGPU_ERR_UNSUPPORTED, "period %d: %lld states + %d actions reach 2^31 levels", t + 1, (long long)nx, s->A);
    if (nx * 8 >= 2147483647LL)
      return s->f->fail(SDPGPU_ERR_UNSUPPORTED, "period %d: a value table of %lld states reaches 2 GiB (the G kernel uses 32-bit byte offsets)", t + 1, (long long)nx);
    s->row_pre[(size_t)t] = (size_t)s->sum_nx;
    s->sum_nx += nx;
    s->nx_max = std::max(s->nx_max, nx);
    s->lev_max = std::max(s->lev_max, levels);
  }
  if ((double)s->sum_nx * N > 4.0e9 || (double)s->lev_max * 2 * N > 4.0e9)
    return s->f->fail(SDPGPU_ERR_UNSUPPORTED, "batch tables of %d instances x %lld states (all periods) are too large", N, (long long)s->sum_nx);
  s->plan.assign((size_t)T, PeriodPlan());
  s->inst.assign((size_t)T * N, sdp::StaffBatchInst());
  s->blk.clear();
  s->blk_off.assign((size_t)T, 0);
  s->cells = 0;
  std::vector<int> order((size_t)N);
  for (int t = 0; t < T; ++t) {
    PeriodPlan& pl = s->plan[(size_t)t];
    // groups: the instances of one table, in ascending table id and, inside a group, in the caller's order
    for (int i = 0; i < N; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return s->use[(size_t)a * T + t] < s->use[(size_t)c * T + t]; });
    int largest = 0;
    for (int a = 0; a < N;) {
      int e = a;
      while (e < N && s->use[(size_t)order[(size_t)e] * T + t] == s->use[(size_t)order[(size_t)a] * T + t]) ++e;
      pl.tables++;
      largest = std::max(largest, e - a);
      const Table& tb = s->pool[(size_t)s->use[(size_t)order[(size_t)a] * T + t]];
      pl.longest_row = std::max(pl.longest_row, (int)tb.maxj);
      s->cells += cells_of(tb, s->x_lo[(size_t)t], s->nx[(size_t)t], s->A) * (int64_t)(e - a);
      a = e;
    }
    // R from the group sizes alone: the instance block where some group fills one, else single instances
    pl.R = sdp::kStaffBatchR > 1 && largest >= sdp::kStaffBatchR ? sdp::kStaffBatchR : 1;
    pl.U = pl.R > 1 ? sdp::kStaffBatchUR : sdp::kStaffBatchU1;
    s->blk_off[(size_t)t] = s->blk.size();
    for (int a = 0; a < N;) {
      int e = a;
      while (e < N && s->use[(size_t)order[(size_t)e] * T + t] == s->use[(size_t)order[(size_t)a] * T + t]) ++e;
      for (int b0 = a; b0 < e; b0 += pl.R) {
        for (int r = 0; r < pl.R; ++r) s->blk.push_back(order[(size_t)std::min(b0 + r, e - 1)]);  // (spare slots repeat the last instance)
        pl.blocks++;
      }
      a = e;
    }
    const int64_t levels = s->nx[(size_t)t] + s->A - 1;
    pl.g_blocks = (levels + 63) / 64;
    pl.tiles = (s->nx[(size_t)t] + 63) / 64;
    // (a dispatch carries at most 2^32 - 1 work-items)
    if (pl.blocks * pl.g_blocks * 64 >= 4294967296LL || !grid_ok((int64_t)N * pl.tiles) || pl.blocks * pl.R >= 2147483647LL)
      return s->f->fail(SDPGPU_ERR_UNSUPPORTED, "period %d: %lld G tasks / %lld scan workgroups do not fit one launch", t + 1,
                   (long long)(pl.blocks * pl.g_blocks), (long long)((int64_t)N * pl.tiles));
    for (int i = 0; i < N; ++i) {
      const sdpgpu_desc& d = s->d[(size_t)i];
      sdp::StaffBatchInst I{};
      I.K = d.fixed_order_cost;
      I.v = d.unit_order_cost;
      I.salary = d.holding_cost;
      I.pen = d.penalty_cost;
      I.min_staff = (int32_t)s->min_staff[(size_t)i * T + t];
      I.table = s->use[(size_t)i * T + t];
      I.v_cur_off = (int64_t)value_row(s, i, t);
      I.v_next_off = t + 1 < T ? (int64_t)value_row(s, i, t + 1) : 0;
      I.pol_off = (int64_t)policy_row(s, i, t);
      s->inst[(size_t)t * N + i] = I;
    }
  }
  s->laid_out = true;
  return SDPGPU_OK;
}

// sdpgpu_batch_set_overhead since the instance records went up: the records laid out again (same size, new minStaffNum) replace
// the device copy.  Every user of d_inst comes through allocate(), so none of them launches on the old values.
int refresh_inst(StaffBatch* s) {
  if (!s->inst_stale) return SDPGPU_OK;
  int rc = layout(s);
  if (rc) return rc;
  SIM_TRY(s->f, hipStreamSynchronize(s->f->stream));  // (an earlier launch may still be reading the old records)
  SIM_TRY(s->f, hipMemcpy(s->d_inst, s->inst.data(), s->inst.size() * sizeof(sdp::StaffBatchInst), hipMemcpyHostToDevice));
  s->inst_stale = false;
  return SDPGPU_OK;
}

int allocate(StaffBatch* s) {
  if (s->allocated) return refresh_inst(s);
  int rc = layout(s);
  if (rc) return rc;
  if ((rc = s->f->open(s->N))) return rc;
  const int N = s->N;
  std::vector<sdp::StaffBatchTable> tabs(s->pool.size());
  for (size_t k = 0; k < s->pool.size(); ++k) {
    const Table& tb = s->pool[k];
    double* p = nullptr;
    int32_t* len = nullptr;
    SIM_TRY(s->f, hipMalloc((void**)&p, tb.p.size() * sizeof(double)));
    s->owned.push_back(p);
    SIM_TRY(s->f, hipMalloc((void**)&len, tb.len.size() * sizeof(int32_t)));
    s->owned.push_back(len);
    SIM_TRY(s->f, hipMemcpy(p, tb.p.data(), tb.p.size() * sizeof(double), hipMemcpyHostToDevice));
    SIM_TRY(s->f, hipMemcpy(len, tb.len.data(), tb.len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    tabs[k] = sdp::StaffBatchTable{p, len, tb.rows, tb.maxj};
  }
  SIM_TRY(s->f, hipMalloc((void**)&s->d_tabs, std::max<size_t>(tabs.size(), 1) * sizeof(sdp::StaffBatchTable)));
  SIM_TRY(s->f, hipMemcpy(s->d_tabs, tabs.data(), tabs.size() * sizeof(sdp::StaffBatchTable), hipMemcpyHostToDevice));
  SIM_TRY(s->f, hipMalloc((void**)&s->d_inst, s->inst.size() * sizeof(sdp::StaffBatchInst)));
  SIM_TRY(s->f, hipMemcpy(s->d_inst, s->inst.data(), s->inst.size() * sizeof(sdp::StaffBatchInst), hipMemcpyHostToDevice));
  SIM_TRY(s->f, hipMalloc((void**)&s->d_blk, std::max<size_t>(s->blk.size(), 1) * sizeof(int32_t)));
  SIM_TRY(s->f, hipMemcpy(s->d_blk, s->blk.data(), s->blk.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  const size_t v_elems = s->d[0].store_all_values ? (size_t)N * (size_t)s->sum_nx : (size_t)N * 2 * (size_t)s->nx_max;
  SIM_TRY(s->f, hipMalloc((void**)&s->d_values, v_elems * sizeof(double)));
  SIM_TRY(s->f, hipMalloc((void**)&s->d_policy, (size_t)N * (size_t)s->sum_nx * sizeof(int32_t)));
  SIM_TRY(s->f, hipMalloc((void**)&s->d_gp, (size_t)N * 2 * (size_t)s->lev_max * sizeof(double)));
  s->allocated = true;
  return SDPGPU_OK;
}

template <int R, int U>
hipError_t launch_g(StaffBatch* s, const sdp::StaffBatchLaunch& L, const PeriodPlan& pl, int t) {
  const dim3 grid((unsigned)(pl.blocks * pl.g_blocks));
  const sdp::StaffBatchInst* inst = s->d_inst + (size_t)t * s->N;
  const int32_t* blk = s->d_blk + s->blk_off[(size_t)t];
  if (t + 1 < s->T)
    hipLaunchKernelGGL((sdp::staff_batch_g_kernel<R, U, true>), grid, dim3(64), 0, s->f->stream, L, inst, s->d_tabs, blk, s->d_values, s->d_gp);
  else
    hipLaunchKernelGGL((sdp::staff_batch_g_kernel<R, U, false>), grid, dim3(64), 0, s->f->stream, L, inst, s->d_tabs, blk, s->d_values, s->d_gp);
  return hipGetLastError();
}

hipError_t launch_period(StaffBatch* s, int t) {
  const PeriodPlan& pl = s->plan[(size_t)t];
  const sdpgpu_desc& d = s->d[0];
  sdp::StaffBatchLaunch L{};
  L.n_actions = s->A;
  L.y0 = (int32_t)s->x_lo[(size_t)t];
  L.n_states = (int32_t)s->nx[(size_t)t];
  L.n_levels = L.n_states + s->A - 1;
  // bounds of the next staff number: [minX, maxX] when clamped, else the next period's box (staff_next_bounds, sdpgpu_staff.hip)
  L.next_x_lo = t + 1 < s->T ? (int32_t)s->x_lo[(size_t)t + 1] : 0;
  if (d.clamp_inventory) {
    L.nn_lo = (int32_t)d.min_inventory;
    L.nn_hi = (int32_t)d.max_inventory;
  } else {
    L.nn_lo = L.next_x_lo;
    L.nn_hi = t + 1 < s->T ? L.next_x_lo + (int32_t)s->nx[(size_t)t + 1] - 1 : 0;
  }
  L.g_blocks = (int32_t)pl.g_blocks;
  L.tiles = (int32_t)pl.tiles;
  L.lev_stride = s->lev_max;
  hipError_t e = pl.R == 1 ? launch_g<1, sdp::kStaffBatchU1>(s, L, pl, t) : launch_g<sdp::kStaffBatchR, sdp::kStaffBatchUR>(s, L, pl, t);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sdp::staff_batch_min_kernel, dim3((unsigned)((int64_t)s->N * pl.tiles)), dim3(256), 0, s->f->stream, L,
                     s->d_inst + (size_t)t * s->N, s->d_gp, s->d_values, s->d_policy);
  return hipGetLastError();
}

// what differs between instance k and instance 0 although the batch needs it shared (nullptr: nothing)
const char* shape_mismatch(const sdpgpu_desc& a, const sdpgpu_desc& c, char* buf, size_t n) {
#define SDP_SAME_I(f) \
  if (a.f != c.f) { std::snprintf(buf, n, #f " %d differs from instance 0's %d", (int)c.f, (int)a.f); return buf; }
#define SDP_SAME_D(f) \
  if (a.f != c.f) { std::snprintf(buf, n, #f " %g differs from instance 0's %g", (double)c.f, (double)a.f); return buf; }
  SDP_SAME_I(periods)
  SDP_SAME_D(step)
  SDP_SAME_D(min_inventory)
  SDP_SAME_D(max_inventory)
  SDP_SAME_D(max_order_quantity)
  SDP_SAME_I(clamp_inventory)
  SDP_SAME_D(ini_inventory)
  SDP_SAME_I(device)
  SDP_SAME_I(store_all_values)
#undef SDP_SAME_I
#undef SDP_SAME_D
  return nullptr;
}

int read_check(StaffBatch* s, const char* who, int32_t instance, int32_t period, const void* out, int64_t n, bool is_values) {
  // the period's own count (the boxes exist once a solve has laid them out: `solved` is looked at first)
  const int64_t nx = s->solved && period >= 1 && period <= s->T ? s->nx[(size_t)period - 1] : 0;
  char states[64];
  std::snprintf(states, sizeof states, "period %d has %lld states", period, (long long)nx);
  return read_check(s->f, who, instance, s->N, period, out, n, nx, states, s->solved, true, is_values && !s->d[0].store_all_values);
}

}  // namespace

int staff_batch_new(const sdpgpu_desc* descs, int32_t n, BatchFrame* frame, StaffBatch** out, std::string* why) {
  for (int32_t k = 0; k < n; ++k) {
    const sdpgpu_desc& d = descs[k];
    g_create_error.clear();
    int rc = validate(d);
    if (rc) {
      const std::string inner = g_create_error;
      return fail_to(why, rc, "instance %d: %s", k, inner.c_str());
    }
    if (d.family != SDPGPU_FAMILY_STAFF)
      return fail_to(why, SDPGPU_ERR_UNSUPPORTED, "instance %d: family %d -- instance 0 makes this a batch of the staff family (SDPGPU_FAMILY_STAFF); a batch holds one family", k, d.family);
    if (d.world_size != 1)
      return fail_to(why, SDPGPU_ERR_UNSUPPORTED, "instance %d: world_size %d -- a batch runs on one device (split the instance list per rank on the host)", k, d.world_size);
    if (d.kernel != SDPGPU_KERNEL_SEPARABLE)
      return fail_to(why, SDPGPU_ERR_UNSUPPORTED, "instance %d: kernel %d -- a staff batch runs the separable mode only (SDPGPU_KERNEL_SEPARABLE, never chosen "
                   "automatically); the exact cell-by-cell tables come from one handle per instance", k, d.kernel);
    char buf[160];
    if (const char* mis = shape_mismatch(descs[0], d, buf, sizeof buf))
      return fail_to(why, SDPGPU_ERR_ARG, "instance %d: %s (the instances of a staff batch share one shape and iniStaffNum)", k, mis);
  }
  const sdpgpu_desc& d = descs[0];
  const int32_t A = full_action_count(d);
  StaffBatch* s = new StaffBatch();
  try {
    s->d.assign(descs, descs + n);
    s->N = n;
    s->T = d.periods;
    s->A = A;
    s->f = frame;
    frame->device = d.device;
    frame->T = d.periods;
    s->use.assign((size_t)n * s->T, -1);
    s->min_staff.assign((size_t)n * s->T, 0.0);
    s->min_set.assign((size_t)n * s->T, 0);
  } catch (...) {
    delete s;
    throw;
  }
  *out = s;
  return SDPGPU_OK;
}

void staff_batch_delete(StaffBatch* s) {
  if (!s) return;
  s->f->close(s->allocated || s->d_tabs || !s->owned.empty() || s->f->d_sim_scratch,
              {s->d_tabs, s->d_inst, s->d_blk, s->d_values, s->d_policy, s->d_gp, s->d_fit_pairs, s->d_fit, s->d_gy}, s->owned);
  delete s;
}

int staff_batch_add_table(StaffBatch* s, const double* prob, const int32_t* row_len, int32_t n_rows, int32_t row_stride,
                          int32_t* out_table) {
  if (!prob || !out_table || n_rows < 1 || row_stride < 1)
    return s->f->fail(SDPGPU_ERR_ARG, "batch_add_level_pmf: bad argument (prob %s, out_table %s, rows=%d stride=%d)", prob ? "set" : "null",
                 out_table ? "set" : "null", n_rows, row_stride);
  if (s->allocated) return s->f->fail(SDPGPU_ERR_STATE, "level tables are frozen once the device tables exist");
  Table tb;
  tb.len.resize((size_t)n_rows);
  int32_t maxj = 1;
  for (int32_t y = 0; y < n_rows; ++y) {
    const int32_t n = row_len ? row_len[y] : y + 1;
    if (n < 1 || n > y + 1 || n > row_stride)
      return s->f->fail(SDPGPU_ERR_ARG, "batch_add_level_pmf: row %d has %d entries (1 .. min(y + 1, row_stride) allowed)", y, n);
    tb.len[(size_t)y] = n;
    maxj = std::max(maxj, n);
  }
  if ((int64_t)n_rows * maxj * 8 >= 2147483647LL)
    return s->f->fail(SDPGPU_ERR_UNSUPPORTED, "batch_add_level_pmf: a table of %d x %d entries reaches 2 GiB (the G kernel uses 32-bit byte offsets)", n_rows, maxj);
  tb.p.assign((size_t)n_rows * (size_t)maxj, 0.0);
  for (int32_t y = 0; y < n_rows; ++y)
    for (int32_t j = 0; j < tb.len[(size_t)y]; ++j) tb.p[(size_t)j * (size_t)n_rows + (size_t)y] = prob[(size_t)y * (size_t)row_stride + (size_t)j];
  tb.rows = n_rows;
  tb.maxj = maxj;
  s->pool.push_back(std::move(tb));
  *out_table = (int32_t)s->pool.size() - 1;
  return SDPGPU_OK;
}

int staff_batch_use_table(StaffBatch* s, int32_t instance, int32_t t, int32_t table) {
  if (instance < -1 || instance >= s->N) return s->f->fail(SDPGPU_ERR_ARG, "batch_use_level_pmf: instance %d outside 0 .. %d (-1: every instance)", instance, s->N - 1);
  if (t < -1 || t >= s->T) return s->f->fail(SDPGPU_ERR_ARG, "batch_use_level_pmf: period index %d outside 0 .. %d (-1: every period)", t, s->T - 1);
  if (table < 0 || table >= (int32_t)s->pool.size())
    return s->f->fail(SDPGPU_ERR_ARG, "batch_use_level_pmf: table %d is not in the pool (%d tables, sdpgpu_batch_add_level_pmf)", table, (int)s->pool.size());
  if (s->allocated) return s->f->fail(SDPGPU_ERR_STATE, "level tables are frozen once the device tables exist");
  for (int i = instance < 0 ? 0 : instance; i < (instance < 0 ? s->N : instance + 1); ++i)
    for (int u = t < 0 ? 0 : t; u < (t < 0 ? s->T : t + 1); ++u) s->use[(size_t)i * s->T + u] = table;
  s->laid_out = false;
  return SDPGPU_OK;
}

int staff_batch_set_min_staff(StaffBatch* s, int32_t instance, int32_t t, double min_staff) {
  if (instance < 0 || instance >= s->N) return s->f->fail(SDPGPU_ERR_ARG, "batch_set_overhead: instance %d outside 0 .. %d", instance, s->N - 1);
  if (t < 0 || t >= s->T) return s->f->fail(SDPGPU_ERR_ARG, "batch_set_overhead: period index %d outside 0 .. %d", t, s->T - 1);
  if (!(min_staff == std::floor(min_staff)) || std::fabs(min_staff) > 1e9)
    return s->f->fail(SDPGPU_ERR_ARG, "batch_set_overhead: minStaffNum %g of instance %d, period %d must be an integer", min_staff, instance, t + 1);
  // (the staff ranges, plans and arenas do not depend on minStaffNum: once the device tables exist, whatever uses the instance
  // records next -- a solve, a level-rule rollout -- lays them out again and uploads them over the old ones: refresh_inst)
  s->min_staff[(size_t)instance * s->T + t] = min_staff;
  s->min_set[(size_t)instance * s->T + t] = 1;
  s->laid_out = false;
  if (s->allocated) {  // (the value and policy tables answer the old value: the batch is unsolved until the next solve)
    s->inst_stale = true;
    s->solved = false;
    s->gy_valid = false;
  }
  return SDPGPU_OK;
}

int staff_batch_grid(const StaffBatch* s, int32_t instance, int32_t period, double* x_lo, int64_t* nx) {
  if (instance < 0 || instance >= s->N) return s->f->fail(SDPGPU_ERR_ARG, "sdpgpu_batch_grid: instance %d outside 0 .. %d", instance, s->N - 1);
  if (period < 1 || period > s->T) return s->f->fail(SDPGPU_ERR_ARG, "sdpgpu_batch_grid: period %d outside 1 .. %d", period, s->T);
  if (!x_lo || !nx) return s->f->fail(SDPGPU_ERR_ARG, "sdpgpu_batch_grid: null output");
  std::vector<int64_t> lo, n;
  int missing = -1;
  boxes_of(s, instance, period, &lo, &n, &missing);
  if (missing >= 0)
    return s->f->fail(SDPGPU_ERR_STATE, "sdpgpu_batch_grid: level table of instance %d, period %d not set (clamp_inventory = 0: the staff range of period %d "
                 "grows from the tables before it)", instance, missing + 1, period);
  *x_lo = (double)lo[(size_t)period - 1];
  *nx = n[(size_t)period - 1];
  return SDPGPU_OK;
}

int64_t staff_batch_num_states(const StaffBatch* s, int32_t instance) {
  if (instance < 0 || instance >= s->N) return -1;
  std::vector<int64_t> lo, n;
  int missing = -1;
  boxes_of(s, instance, s->T, &lo, &n, &missing);
  return missing >= 0 ? -1 : n[(size_t)s->T - 1];
}

int32_t staff_batch_num_actions(const StaffBatch* s, int32_t instance) { return instance >= 0 && instance < s->N ? s->A : -1; }

int staff_batch_plan(StaffBatch* s, int32_t period, sdpgpu_batch_staff_plan* out) {
  if (!out) return s->f->fail(SDPGPU_ERR_ARG, "sdpgpu_batch_staff_plan_period: out is null");
  if (period < 1 || period > s->T) return s->f->fail(SDPGPU_ERR_ARG, "sdpgpu_batch_staff_plan_period: period %d outside 1 .. %d", period, s->T);
  std::memset(out, 0, sizeof *out);
  int rc = layout(s);
  if (rc) return rc;
  const PeriodPlan& pl = s->plan[(size_t)period - 1];
  out->tables = pl.tables;
  out->groups = pl.tables;
  out->r = pl.R;
  out->u = pl.U;
  out->longest_row = pl.longest_row;
  out->blocks = pl.blocks;
  out->g_tasks = pl.blocks * pl.g_blocks;
  out->scan_workgroups = (int64_t)s->N * pl.tiles;
  out->states = s->nx[(size_t)period - 1];
  out->levels = out->states + s->A - 1;
  return SDPGPU_OK;
}

int staff_batch_solve(StaffBatch* s, int32_t sync) {
  int rc = layout(s);  // (argument and state errors before the device is touched)
  if (rc) return rc;
  DeviceScope dev;
  SIM_TRY(s->f, dev.enter(s->f->device));
  rc = allocate(s);
  if (rc) return rc;
  s->gy_valid = false;  // (the G rows are those of the tables about to be replaced)
  s->period_launches = s->periods_run = 0;
  if ((rc = s->f->sweep_begin())) return rc;
  for (int t = s->T - 1; t >= 0; --t) {
    if ((rc = s->f->period_mark(t))) return rc;
    const hipError_t e = launch_period(s, t);
    if (e != hipSuccess) return s->f->fail(SDPGPU_ERR_DEVICE, "staff batch period %d: %s", t + 1, hipGetErrorString(e));
    s->period_launches += 2;
    s->periods_run++;
  }
  if ((rc = s->f->period_mark(-1))) return rc;
  s->solved = true;
  return s->f->sweep_end(sync != 0);
}

bool staff_batch_allocated(const StaffBatch* s) { return s->allocated; }

int staff_batch_values(StaffBatch* s, int32_t instance, int32_t period, double* out, int64_t n) {
  int rc = read_check(s, "sdpgpu_batch_values", instance, period, out, n, true);
  if (rc) return rc;
  return s->f->read_row(out, s->d_values + value_row(s, instance, period - 1), (size_t)n * sizeof(double));
}

int staff_batch_policy(StaffBatch* s, int32_t instance, int32_t period, int32_t* out, int64_t n) {
  int rc = read_check(s, "sdpgpu_batch_policy", instance, period, out, n, false);
  if (rc) return rc;
  return s->f->read_row(out, s->d_policy + policy_row(s, instance, period - 1), (size_t)n * sizeof(int32_t));
}

int staff_batch_initial(StaffBatch* s, double* out_value, int32_t* out_action_index) {
  if (!out_value || !out_action_index) return s->f->fail(SDPGPU_ERR_ARG, "sdpgpu_batch_initial: null output");
  if (!s->solved) return s->f->fail(SDPGPU_ERR_STATE, "sdpgpu_batch_initial before sdpgpu_batch_solve");
  DeviceScope dev;
  SIM_TRY(s->f, dev.enter(s->f->device));
  const int N = s->N;
  const int ini_idx = (int)((int64_t)s->d[0].ini_inventory - s->x_lo[0]);  // (validated at create: inside period 1's box)
  hipLaunchKernelGGL(sdp::staff_batch_initial_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->f->stream, s->d_inst, N, ini_idx,
                     s->d_values, s->d_policy, s->f->ini_value(), s->f->ini_action(N));
  SIM_TRY(s->f, hipGetLastError());
  return s->f->initial_download(out_value, out_action_index, N);
}

int staff_batch_stats(StaffBatch* s, sdpgpu_batch_stats* out) {
  std::memset(out, 0, sizeof *out);
  out->instances = s->N;
  out->periods_run = s->periods_run;
  out->period_launches = s->period_launches;
  out->cells_evaluated = s->solved ? s->cells : 0;
  return s->f->solve_ms(&out->solve_ms);
}

// =================================================================================================
// Fit and rollout: getOptTable's intervals, FitsS.getSinglesS and SimulatesS.simulatesS for every instance ("Workforce
// batch: fit and rollout").  The rollout's host frame is RolloutFrame with the batch's frame as its owner.
// =================================================================================================

namespace {

constexpr int32_t kStaffBatchSimMaxRules = 64;
constexpr int64_t kStaffBatchSimMaxSums = (int64_t)1 << 28;  // leaf sums of a call: 2 GiB

// staff_reach_intervals (sdpgpu_staff.hip) for instance i over the pool's tables, periods 1 .. upto; reads the tables of the
// periods before `upto`.  -1 in *missing_t: all were there.
void reach_of(const StaffBatch* s, int i, int upto, std::vector<int64_t>* lo_out, std::vector<int64_t>* hi_out, int* missing_t) {
  const sdpgpu_desc& d = s->d[0];
  *missing_t = -1;
  int64_t L = (int64_t)d.ini_inventory, H = L;
  lo_out->assign((size_t)upto, 0);
  hi_out->assign((size_t)upto, -1);
  for (int t = 0; t < upto; ++t) {
    (*lo_out)[(size_t)t] = L;
    (*hi_out)[(size_t)t] = H;
    if (t + 1 == upto) break;
    const int32_t id = s->use[(size_t)i * s->T + t];
    if (id < 0) {
      *missing_t = t;
      return;
    }
    const Table& tb = s->pool[(size_t)id];
    const int64_t rows = tb.rows;
    int64_t low = INT64_MAX;
    const int64_t top = H + (s->A - 1);
    for (int64_t y = L; y <= std::min(top, rows - 1); ++y) low = std::min(low, y - tb.len[(size_t)y] + 1);
    if (top > rows - 1) low = std::min(low, std::max(L, rows) - tb.len[(size_t)rows - 1] + 1);
    L = low;
    H = top;
    if (d.clamp_inventory) {
      auto cl = [&](int64_t v) {
        v = v > (int64_t)d.max_inventory ? (int64_t)d.max_inventory : v;
        return v < (int64_t)d.min_inventory ? (int64_t)d.min_inventory : v;
      };
      L = cl(L);
      H = cl(H);
    }
  }
}

// the intervals of every (instance, period), once (the tables are frozen: the device tables exist); instances that walk the same
// tables share one computation
void reach_all(StaffBatch* s) {
  if (!s->reach_lo.empty()) return;
  const int N = s->N, T = s->T;
  s->reach_lo.assign((size_t)N * T, 0);
  s->reach_hi.assign((size_t)N * T, -1);
  std::map<std::vector<int32_t>, int> seen;
  std::vector<int64_t> lo, hi;
  for (int i = 0; i < N; ++i) {
    const std::vector<int32_t> key(s->use.begin() + (size_t)i * T, s->use.begin() + (size_t)(i + 1) * T);
    const auto at = seen.find(key);
    if (at != seen.end()) {
      std::copy_n(s->reach_lo.begin() + (size_t)at->second * T, T, s->reach_lo.begin() + (size_t)i * T);
      std::copy_n(s->reach_hi.begin() + (size_t)at->second * T, T, s->reach_hi.begin() + (size_t)i * T);
      continue;
    }
    int missing = -1;
    reach_of(s, i, T, &lo, &hi, &missing);  // (laid out: no table is missing)
    std::copy_n(lo.begin(), T, s->reach_lo.begin() + (size_t)i * T);
    std::copy_n(hi.begin(), T, s->reach_hi.begin() + (size_t)i * T);
    seen.emplace(key, i);
  }
}

// the walk down a row stops at the first threshold above u: right only when the running sums never decrease.  Every table an
// (instance, period) uses is looked at once.
int check_tables(StaffBatch* s, const char* who) {
  for (size_t k = 0; k < s->use.size(); ++k) {
    Table& tb = s->pool[(size_t)s->use[k]];
    if (tb.nonneg) continue;
    for (size_t e = 0; e < tb.p.size(); ++e)
      if (!(tb.p[e] >= 0.0))
        return s->f->fail(SDPGPU_ERR_ARG, "%s: table %d of the pool holds a negative or NaN probability (level %zu, turnover %zu)", who, (int)s->use[k],
                     e % (size_t)tb.rows, e / (size_t)tb.rows);
    tb.nonneg = true;
  }
  return SDPGPU_OK;
}

}  // namespace

int staff_batch_reachable(StaffBatch* s, int32_t instance, int32_t period, int64_t* lo, int64_t* hi) {
  const char* who = "sdpgpu_batch_staff_reachable";
  if (instance < 0 || instance >= s->N) return s->f->fail(SDPGPU_ERR_ARG, "%s: instance %d outside 0 .. %d", who, instance, s->N - 1);
  if (period < 1 || period > s->T) return s->f->fail(SDPGPU_ERR_ARG, "%s: period %d outside 1 .. %d", who, period, s->T);
  if (!lo || !hi) return s->f->fail(SDPGPU_ERR_ARG, "%s: null output (lo, hi)", who);
  std::vector<int64_t> l, h;
  int missing = -1;
  reach_of(s, instance, period, &l, &h, &missing);
  if (missing >= 0)
    return s->f->fail(SDPGPU_ERR_STATE, "%s: level table of instance %d, period %d not set (the staff numbers of period %d follow from the tables "
                 "before it)", who, instance, missing + 1, period);
  *lo = l[(size_t)period - 1];
  *hi = h[(size_t)period - 1];
  return SDPGPU_OK;
}

int staff_batch_fit_ss(StaffBatch* s, double max_order_quantity, double* out) {
  const char* who = "sdpgpu_batch_staff_fit_ss";
  if (!out) return s->f->fail(SDPGPU_ERR_ARG, "%s: out is null", who);
  if (!std::isfinite(max_order_quantity) || max_order_quantity < 0)
    return s->f->fail(SDPGPU_ERR_ARG, "%s: max_order_quantity = %g (a finite limit >= 0; the drivers pass Integer.MAX_VALUE)", who, max_order_quantity);
  if (!s->solved) return s->f->fail(SDPGPU_ERR_STATE, "%s before sdpgpu_batch_solve", who);
  const int N = s->N, T = s->T;
  reach_all(s);
  std::vector<sdp::FitPair> pairs((size_t)N * T);
  for (int i = 0; i < N; ++i)
    for (int t = 0; t < T; ++t) {
      const int64_t L = s->reach_lo[(size_t)i * T + t], H = s->reach_hi[(size_t)i * T + t], x0 = s->x_lo[(size_t)t];
      if (L < x0 || H < L || H - x0 >= s->nx[(size_t)t])  // (the visited numbers lie inside the period's box by construction)
        return s->f->fail(SDPGPU_ERR_INTERNAL, "%s: instance %d, period %d: staff numbers %lld .. %lld outside the box %lld .. %lld", who, i, t + 1,
                     (long long)L, (long long)H, (long long)x0, (long long)(x0 + s->nx[(size_t)t] - 1));
      pairs[(size_t)i * T + t] = sdp::FitPair{(int64_t)policy_row(s, i, t), (double)x0, max_order_quantity, (int32_t)(L - x0), (int32_t)(H - L + 1)};
    }
  DeviceScope dev;
  SIM_TRY(s->f, dev.enter(s->f->device));
  if (!s->d_fit_pairs) SIM_TRY(s->f, hipMalloc((void**)&s->d_fit_pairs, pairs.size() * sizeof(sdp::FitPair)));
  if (!s->d_fit) SIM_TRY(s->f, hipMalloc((void**)&s->d_fit, pairs.size() * 2 * sizeof(double)));
  SIM_TRY(s->f, hipMemcpyAsync(s->d_fit_pairs, pairs.data(), pairs.size() * sizeof(sdp::FitPair), hipMemcpyHostToDevice, s->f->stream));
  SIM_TRY(s->f, launch_fit_singles(s->f->stream, s->d_fit_pairs, N * T, T, s->d_policy, s->d_fit));
  SIM_TRY(s->f, hipMemcpyAsync(out, s->d_fit, pairs.size() * 2 * sizeof(double), hipMemcpyDeviceToHost, s->f->stream));
  SIM_TRY(s->f, hipStreamSynchronize(s->f->stream));
  return SDPGPU_OK;
}

int staff_batch_simulate(StaffBatch* s, const int32_t* sample_nums, uint64_t seed, double ini_x, const double* ss,
                         int32_t n_rules, sdpgpu_sim_result* results, double* out_sum, uint8_t* out_valid, int32_t* out_demand) {
  const char* who = "sdpgpu_batch_staff_simulate";
  const int N = s->N, T = s->T;
  if (!sample_nums) return s->f->fail(SDPGPU_ERR_ARG, "%s: sample_nums is null", who);
  if (!results) return s->f->fail(SDPGPU_ERR_ARG, "%s: results is null", who);
  if (n_rules < 1 || n_rules > kStaffBatchSimMaxRules) return s->f->fail(SDPGPU_ERR_ARG, "%s: n_rules = %d (1 .. %d)", who, n_rules, kStaffBatchSimMaxRules);
  if (!ss && n_rules != 1) return s->f->fail(SDPGPU_ERR_ARG, "%s: n_rules = %d with ss == NULL (the table policy is one rule)", who, n_rules);
  int64_t leaves = 1;
  for (int t = 0; t < T; ++t) {
    if (sample_nums[t] < 1) return s->f->fail(SDPGPU_ERR_ARG, "%s: sample_nums[%d] = %d (at least 1)", who, t, sample_nums[t]);
    leaves *= sample_nums[t];
    if (leaves > kSimMaxPaths) return s->f->fail(SDPGPU_ERR_ARG, "%s: sample_nums gives more than %d leaves (product up to index %d)", who, kSimMaxPaths, t);
  }
  const int64_t n_pairs = (int64_t)N * n_rules;
  if (n_pairs * leaves > kStaffBatchSimMaxSums)
    return s->f->fail(SDPGPU_ERR_ARG, "%s: %d instances x n_rules %d x %lld leaves (sample_nums) exceed %lld leaf sums (2 GiB)", who, N, n_rules,
                 (long long)leaves, (long long)kStaffBatchSimMaxSums);
  for (int i = 0; i < N; ++i)
    for (int t = 0; t < T; ++t)
      if (s->use[(size_t)i * T + t] < 0)
        return s->f->fail(SDPGPU_ERR_STATE, "%s: level table of instance %d, period %d not set (sdpgpu_batch_use_level_pmf)", who, i, t + 1);
  if (!(ini_x >= 0 && ini_x <= 1e9) || ini_x != std::floor(ini_x))
    return s->f->fail(SDPGPU_ERR_ARG, "%s: ini_x = %g (a staff number: an integer in 0 .. 1e9)", who, ini_x);
  std::vector<int32_t> levels;
  if (ss) {
    levels.resize((size_t)n_pairs * T * 2);
    for (int i = 0; i < N; ++i)
      for (int r = 0; r < n_rules; ++r)
        for (int t = 0; t < T; ++t) {
          const size_t k = (((size_t)i * n_rules + r) * T + t) * 2;
          const double lo = ss[k], up = ss[k + 1];
          // (int) of a double: toward zero; what it cannot represent is refused
          if (!std::isfinite(lo) || !std::isfinite(up) || !(lo > -2147483649.0 && lo < 2147483648.0) || !(up > -2147483649.0 && up < 2147483648.0))
            return s->f->fail(SDPGPU_ERR_ARG, "%s: ss[%d][%d][%d] = (%g, %g) is not finite or outside int32", who, i, r, t, lo, up);
          const int32_t si = (int32_t)lo, Si = (int32_t)up;
          if ((int64_t)Si < (int64_t)si - 1)
            return s->f->fail(SDPGPU_ERR_ARG, "%s: ss[%d][%d][%d] = (%g, %g): S < s - 1 would hire a negative number at x = s - 1", who, i, r, t, lo, up);
          levels[k] = si;
          levels[k + 1] = Si;
        }
  }
  int rc = layout(s);  // host arithmetic: the periods' boxes
  if (rc) return rc;
  if (!ss) {
    const double lo = (double)s->x_lo[0], hi = lo + (double)(s->nx[0] - 1);
    if (ini_x < lo || ini_x > hi) return s->f->fail(SDPGPU_ERR_ARG, "%s: ini_x = %g outside period 1's staff numbers %g .. %g", who, ini_x, lo, hi);
    if (!s->solved) return s->f->fail(SDPGPU_ERR_STATE, "%s: nothing has been solved (the table policy needs sdpgpu_batch_solve; a level rule does not)", who);
  }
  rc = check_tables(s, who);
  if (rc) return rc;

  rc = no_device(s->f, who);
  if (rc) return rc;
  DeviceScope dev;
  SIM_TRY(s->f, dev.enter(s->f->device));
  rc = allocate(s);  // (a level rule needs the device tables, not a solve)
  if (rc) return rc;
  const uint32_t n = (uint32_t)leaves;
  // what the instances share of a period: the tree level and the box (the instance's fields are filled in by the kernel)
  std::vector<sdp::StaffSimPeriod> per((size_t)T);
  uint32_t stride = n;
  for (int t = 0; t < T; ++t) {
    sdp::StaffSimPeriod& q = per[(size_t)t];
    std::memset(&q, 0, sizeof q);
    stride /= (uint32_t)sample_nums[t];
    q.x_lo = (int32_t)s->x_lo[(size_t)t];
    q.nx = (int32_t)s->nx[(size_t)t];
    q.K = (uint32_t)sample_nums[t];
    q.stride = stride;
    q.half_bits = make_stream(sample_nums[t], 0, 0).half_bits;
  }
  const sdpgpu_desc& d = s->d[0];
  sdp::StaffSimLaunch L{};
  L.T = T;
  L.n_rules = (int32_t)n_pairs;
  L.clamp = d.clamp_inventory;
  L.min_x = (int32_t)d.min_inventory;
  L.max_x = (int32_t)d.max_inventory;
  L.ini_x = (int32_t)ini_x;
  L.n_leaves = n;
  L.seed_lo = (uint32_t)(seed & 0xffffffffu);
  L.seed_hi = (uint32_t)(seed >> 32);

  RolloutFrame<BatchFrame> f(s->f, n, (size_t)n_pairs);
  const size_t sums = f.nr * n;
  const auto p_per = f.put(per.data(), per.size());
  const auto p_ss = f.put(levels.data(), levels.size());
  const auto p_flag = f.take<uint8_t>(out_valid ? sums : 0);
  const auto p_dem = f.take<int32_t>(out_demand ? sums * (size_t)T : 0);
  rc = f.begin();
  if (rc) return rc;
  L.waves_per_rule = f.W;
  const dim3 grid((unsigned)((f.nr * f.W + 3) / 4));  // (at most 2^28 / 64 + n x rules waves)
  rc = f.start();
  if (rc) return rc;
  if (ss)
    hipLaunchKernelGGL((sdp::staff_batch_sim_kernel<sdp::StaffLevelRule>), grid, dim3(256), 0, s->f->stream, L, (int32_t)N, n_rules, f[p_per], s->d_inst,
                       s->d_tabs, sdp::StaffLevelRule{f[p_ss]}, f.d_sum, f[p_flag], f[p_dem], f.d_part, f.d_cnt);
  else
    hipLaunchKernelGGL((sdp::staff_batch_sim_kernel<sdp::StaffTableRule>), grid, dim3(256), 0, s->f->stream, L, (int32_t)N, n_rules, f[p_per], s->d_inst,
                       s->d_tabs, sdp::StaffTableRule{s->d_policy}, f.d_sum, f[p_flag], f[p_dem], f.d_part, f.d_cnt);
  SIM_TRY(s->f, hipGetLastError());
  f.download(out_valid, f[p_flag], sums);
  f.download(out_demand, f[p_dem], sums * (size_t)T * sizeof(int32_t));
  return f.finish(results, out_sum);
}

// =================================================================================================
// Structure rows: G_t(y) of every (instance, period) in ONE launch, kept until the next solve, and CheckKConvexity on a row of
// every instance ("Workforce structure rows"; sdp_staff_structure.hpp)
// =================================================================================================
namespace {

sdp::StaffGyCost gy_cost(const StaffBatch* s, int i, int t) {
  const sdpgpu_desc& d = s->d[(size_t)i];
  sdp::StaffGyCost c{};
  c.v = d.unit_order_cost;
  c.salary = d.holding_cost;
  c.pen = d.penalty_cost;
  c.min_staff = (int32_t)s->min_staff[(size_t)i * s->T + t];
  c.clamp = d.clamp_inventory;
  c.min_x = (int32_t)d.min_inventory;
  c.max_x = (int32_t)d.max_inventory;
  return c;
}

// G of period index t exists when V of t + 1 does: every period with store_all_values, else t = 0 (V_2 survives) and t = T - 1
bool gy_kept(const StaffBatch* s, int t) { return s->d[0].store_all_values || t == 0 || t == s->T - 1; }

const Table& gy_table(const StaffBatch* s, int i, int t) { return s->pool[(size_t)s->use[(size_t)i * s->T + t]]; }

// level y of (i, t) is off the grid of period index t + 1
bool gy_off_grid(const StaffBatch* s, int i, int t, int y, int* bad_j, int* bad_nn) {
  if (t + 1 >= s->T) return false;
  return sdp::staff_gy_first_off_grid(gy_cost(s, i, t), y, gy_table(s, i, t).len[(size_t)y], s->x_lo[(size_t)t + 1], s->nx[(size_t)t + 1], bad_j, bad_nn);
}

// where the rows lie and which levels of each are made: host arithmetic, once per batch (the tables are frozen by then)
void gy_layout(StaffBatch* s) {
  if (!s->gy_off.empty()) return;
  const int N = s->N, T = s->T;
  s->gy_off.assign((size_t)N * T + 1, 0);
  s->gy_lo.assign((size_t)N * T, 0);
  s->gy_hi.assign((size_t)N * T, -1);
  for (int i = 0; i < N; ++i)
    for (int t = 0; t < T; ++t) {
      const size_t k = (size_t)i * T + t;
      const int32_t rows = gy_table(s, i, t).rows;
      s->gy_off[k + 1] = s->gy_off[k] + (size_t)rows;
      int bj, bn;
      int32_t y = 0;
      while (y < rows && gy_off_grid(s, i, t, y, &bj, &bn)) ++y;
      if (y >= rows) continue;
      s->gy_lo[k] = y;
      while (y < rows && !gy_off_grid(s, i, t, y, &bj, &bn)) ++y;
      s->gy_hi[k] = y - 1;
    }
}

// the G rows of every (instance, period) on the device, once per solve
int gy_fill(StaffBatch* s) {
  if (s->gy_valid) return SDPGPU_OK;
  const int N = s->N, T = s->T;
  gy_layout(s);
  Carve c;
  const size_t o_g = c.take(std::max<size_t>(s->gy_off.back(), 1) * sizeof(double));
  const size_t o_rows = c.take(std::max<size_t>((size_t)N * T, 1) * sizeof(sdp::StaffGyRow));
  // (blocks of 64 levels: no more than one per 64 entries of a row, plus one per row)
  const size_t o_blk = c.take((s->gy_off.back() / 64 + (size_t)N * T + 1) * sizeof(sdp::StaffGyBlock));
  if (!s->d_gy) SIM_TRY(s->f, hipMalloc((void**)&s->d_gy, c.at));
  double* d_g = reinterpret_cast<double*>(s->d_gy + o_g);
  SIM_TRY(s->f, hipStreamSynchronize(s->f->stream));  // (an earlier launch may still be reading the records below)
  s->gy_rows.clear();
  for (int i = 0; i < N; ++i)
    for (int t = 0; t < T; ++t) {
      const size_t k = (size_t)i * T + t;
      if (!gy_kept(s, t) || s->gy_hi[k] < s->gy_lo[k]) continue;  // (a row whose V_{t+1} is gone is not made)
      const int32_t id = s->use[k];
      sdp::StaffGyRow R{};
      R.pT = static_cast<const double*>(s->owned[(size_t)id * 2]);
      R.row_len = static_cast<const int32_t*>(s->owned[(size_t)id * 2 + 1]);
      R.v_next = t + 1 < T ? s->d_values + value_row(s, i, t + 1) : nullptr;
      R.c = gy_cost(s, i, t);
      R.n_rows = s->pool[(size_t)id].rows;
      R.y_lo = s->gy_lo[k];
      R.n = s->gy_hi[k] - s->gy_lo[k] + 1;
      R.next_x_lo = t + 1 < T ? (int32_t)s->x_lo[(size_t)t + 1] : 0;
      R.out = d_g + s->gy_off[k] + (size_t)R.y_lo;
      s->gy_rows.push_back(R);
    }
  staff_gy_blocks(s->gy_rows.data(), (int32_t)s->gy_rows.size(), &s->gy_blocks);
  SIM_TRY(s->f, launch_staff_gy(s->f->stream, s->gy_rows.data(), (int32_t)s->gy_rows.size(), s->gy_blocks, reinterpret_cast<sdp::StaffGyRow*>(s->d_gy + o_rows),
                                reinterpret_cast<sdp::StaffGyBlock*>(s->d_gy + o_blk)));
  s->gy_valid = true;
  return SDPGPU_OK;
}

// the refusals of a level window of (i, period): rows of the table, V_{period+1} held, none off the grid
int gy_check_window(StaffBatch* s, const char* who, int i, int32_t period, int32_t y_lo, int64_t n) {
  const int t = period - 1;
  const int32_t rows = gy_table(s, i, t).rows;
  if (n < 0) return s->f->fail(SDPGPU_ERR_ARG, "%s: n = %lld (at least 0)", who, (long long)n);
  if (y_lo < 0) return s->f->fail(SDPGPU_ERR_ARG, "%s: y_lo = %d (levels start at 0)", who, y_lo);
  if ((int64_t)y_lo + n > rows)
    return s->f->fail(SDPGPU_ERR_ARG, "%s: instance %d: level %d is not a row of period %d's table (n_rows = %d: levels 0 .. %d)", who, i, std::max(y_lo, rows),
                      period, rows, rows - 1);
  if (!gy_kept(s, t))
    return s->f->fail(SDPGPU_ERR_STATE, "%s: G_%d needs V_%d, which was overwritten (store_all_values = 0 keeps G_1 and G_%d)", who, period, period + 1, s->T);
  gy_layout(s);
  const size_t k = (size_t)i * s->T + t;
  for (int64_t y = y_lo; y < y_lo + n; ++y) {
    if (y >= s->gy_lo[k] && y <= s->gy_hi[k]) continue;
    int bj = 0, bn = 0;
    if (gy_off_grid(s, i, t, (int)y, &bj, &bn))
      return s->f->fail(SDPGPU_ERR_ARG, "%s: instance %d: level %d of period %d is off the grid: its successor %d (j = %d) lies outside period %d's staff numbers "
                        "%lld .. %lld", who, i, (int)y, period, bn, bj, period + 1, (long long)s->x_lo[(size_t)t + 1],
                        (long long)(s->x_lo[(size_t)t + 1] + s->nx[(size_t)t + 1] - 1));
    return s->f->fail(SDPGPU_ERR_ARG, "%s: instance %d: level %d of period %d lies behind an off-grid level: the rows kept are the first run %d .. %d", who, i,
                      (int)y, period, s->gy_lo[k], s->gy_hi[k]);
  }
  return SDPGPU_OK;
}

}  // namespace

int staff_batch_gy(StaffBatch* s, int32_t instance, int32_t period, int32_t y_lo, int32_t n, double* out) {
  const char* who = "sdpgpu_batch_staff_gy";
  if (instance < 0 || instance >= s->N) return s->f->fail(SDPGPU_ERR_ARG, "%s: instance %d outside 0 .. %d", who, instance, s->N - 1);
  if (period < 1 || period > s->T) return s->f->fail(SDPGPU_ERR_ARG, "%s: period %d outside 1 .. %d", who, period, s->T);
  if (!s->solved) return s->f->fail(SDPGPU_ERR_STATE, "%s before sdpgpu_batch_solve", who);
  if (!out) return s->f->fail(SDPGPU_ERR_ARG, "%s: out is null", who);
  int rc = gy_check_window(s, who, instance, period, y_lo, n);
  if (rc || n == 0) return rc;
  DeviceScope dev;
  SIM_TRY(s->f, dev.enter(s->f->device));
  if ((rc = gy_fill(s))) return rc;
  const double* d_g = reinterpret_cast<const double*>(s->d_gy);
  return s->f->read_row(out, d_g + s->gy_off[(size_t)instance * s->T + (period - 1)] + y_lo, (size_t)n * sizeof(double));
}

int staff_batch_check_convexity(StaffBatch* s, int32_t kind, int32_t source, int32_t period, const int32_t* lo, const int32_t* hi, const double* K,
                                const int32_t* capacity, sdpgpu_convexity* out) {
  const char* who = "sdpgpu_batch_staff_check_convexity";
  const int N = s->N;
  if (kind != 0 && kind != 1) return s->f->fail(SDPGPU_ERR_ARG, "%s: kind = %d (0: CheckKConvexity.check, 1: CheckKConvexity.checkCK)", who, kind);
  if (source != 0 && source != 1) return s->f->fail(SDPGPU_ERR_ARG, "%s: source = %d (0: the value rows V_period, 1: the rows G_period)", who, source);
  if (period < 1 || period > s->T) return s->f->fail(SDPGPU_ERR_ARG, "%s: period %d outside 1 .. %d", who, period, s->T);
  if (!out) return s->f->fail(SDPGPU_ERR_ARG, "%s: out is null", who);
  if ((lo == nullptr) != (hi == nullptr)) return s->f->fail(SDPGPU_ERR_ARG, "%s: lo and hi are given together, or both NULL (the whole row)", who);
  if (!s->solved) return s->f->fail(SDPGPU_ERR_STATE, "%s before sdpgpu_batch_solve", who);
  const int t = period - 1;
  if (source == 0 && !s->d[0].store_all_values && period > 2)
    return s->f->fail(SDPGPU_ERR_STATE, "%s: V_%d was overwritten (store_all_values = 0 keeps two ping-pong tables: periods 1 and 2 survive)", who, period);
  if (source == 1) gy_layout(s);
  std::vector<ConvexitySpec> specs((size_t)N);
  std::vector<int64_t> row_off((size_t)N);
  for (int i = 0; i < N; ++i) {
    const size_t k = (size_t)i * s->T + t;
    int64_t a, c;
    if (source == 0) {
      const int64_t x0 = s->x_lo[(size_t)t], x1 = x0 + s->nx[(size_t)t] - 1;
      a = lo ? lo[i] : x0;
      c = hi ? hi[i] : x1;
      if (a > c || a < x0 || c > x1)
        return s->f->fail(SDPGPU_ERR_ARG, "%s: instance %d: the window %lld .. %lld is not a run of period %d's staff numbers %lld .. %lld", who, i, (long long)a,
                          (long long)c, period, (long long)x0, (long long)x1);
      row_off[(size_t)i] = (int64_t)value_row(s, i, t) + (a - x0);
    } else {
      a = lo ? lo[i] : s->gy_lo[k];
      c = hi ? hi[i] : s->gy_hi[k];
      if (a > c) return s->f->fail(SDPGPU_ERR_ARG, "%s: instance %d: the window %lld .. %lld is empty", who, i, (long long)a, (long long)c);
      const int rc = gy_check_window(s, who, i, period, (int32_t)a, c - a + 1);
      if (rc) return rc;
      row_off[(size_t)i] = (int64_t)s->gy_off[k] + a;
    }
    if (c - a + 1 > kConvexityMaxPoints)
      return s->f->fail(SDPGPU_ERR_UNSUPPORTED, "%s: instance %d: a row of %lld points exceeds the kernel's %d (a workgroup keeps the row in LDS): narrow "
                        "the window", who, i, (long long)(c - a + 1), kConvexityMaxPoints);
    specs[(size_t)i].K = K ? K[i] : s->d[(size_t)i].fixed_order_cost;
    specs[(size_t)i].n = (int32_t)(c - a + 1);
    specs[(size_t)i].capacity = capacity ? capacity[i] : (int32_t)s->d[(size_t)i].max_order_quantity;
  }
  DeviceScope dev;
  SIM_TRY(s->f, dev.enter(s->f->device));
  int rc = SDPGPU_OK;
  if (source == 1 && (rc = gy_fill(s))) return rc;
  const double* base = source == 0 ? s->d_values : reinterpret_cast<const double*>(s->d_gy);
  for (int i = 0; i < N; ++i) specs[(size_t)i].g = base + row_off[(size_t)i];
  std::string why;
  rc = convexity_on_device(s->f->stream, kind, specs.data(), N, out, &why);
  if (rc) return s->f->fail(rc, "%s: %s", who, why.c_str());
  return SDPGPU_OK;
}

}  // namespace sdpgpu_detail
