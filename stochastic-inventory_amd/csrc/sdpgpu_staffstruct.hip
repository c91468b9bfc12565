// sdpgpu_staffstruct.hip -- sdpgpu_staff_gy_host, sdpgpu_staff_gy, sdpgpu_staff_gy_range, sdpgpu_staff_check_convexity: the G(y)
// rows of the STAFF family and CheckKConvexity on them, for a solved handle (the sum of one level and the kernel:
// sdp_staff_structure.hpp; definition: DESIGN 4, "Workforce structure rows"), and the launch a staff batch shares with it
// (sdpgpu_staffbatch.hip holds the batch's own part).  All validation comes before the first device call.
#include "sdpgpu_sim_host.hpp"
#include "sdp_staff_structure.hpp"

using namespace sdpgpu_detail;

// Blocks of 64 levels over the rows of a call, highest level first (those walk the longest rows); returns their number.
int64_t sdpgpu_detail::staff_gy_blocks(const sdp::StaffGyRow* rows, int32_t n_rows, std::vector<sdp::StaffGyBlock>* blocks) {
  blocks->clear();
  for (int32_t r = 0; r < n_rows; ++r)
    for (int32_t e0 = 0; e0 < rows[r].n; e0 += 64) blocks->push_back(sdp::StaffGyBlock{r, e0});
  std::stable_sort(blocks->begin(), blocks->end(), [&](const sdp::StaffGyBlock& a, const sdp::StaffGyBlock& c) {
    return rows[a.row].y_lo + a.e0 > rows[c.row].y_lo + c.e0;
  });
  return (int64_t)blocks->size();
}

hipError_t sdpgpu_detail::launch_staff_gy(hipStream_t st, const sdp::StaffGyRow* rows, int32_t n_rows, const std::vector<sdp::StaffGyBlock>& blocks,
                                          sdp::StaffGyRow* d_rows, sdp::StaffGyBlock* d_blocks) {
  if (blocks.empty()) return hipSuccess;
  if ((int64_t)blocks.size() * 64 >= 4294967296LL) return hipErrorInvalidValue;  // (a dispatch carries at most 2^32 - 1 work-items)
  hipError_t e = hipMemcpyAsync(d_rows, rows, (size_t)n_rows * sizeof(sdp::StaffGyRow), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  if ((e = hipMemcpyAsync(d_blocks, blocks.data(), blocks.size() * sizeof(sdp::StaffGyBlock), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  hipLaunchKernelGGL((sdp::staff_gy_kernel<sdp::kStaffGyU>), dim3((unsigned)blocks.size()), dim3(64), 0, st, d_rows, d_blocks);
  return hipGetLastError();
}

namespace {

// the scope of a handle, naming the field
int check_scope(sdpgpu_handle* h, const char* who) {
  const sdpgpu_desc& d = h->d;
  if (h->custom) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: a user functor's lambdas are not the closed-form staff cell the rows are defined on", who);
  if (d.family != SDPGPU_FAMILY_STAFF) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: family = %d -- the G(y) rows are those of a STAFF handle (SDPGPU_FAMILY_STAFF)", who, d.family);
  if (d.world_size != 1) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: world_size = %d -- needs the whole value table on one GPU", who, d.world_size);
  return SDPGPU_OK;
}

sdp::StaffGyCost cost_of(const sdpgpu_handle* h, int period) {
  const sdpgpu_desc& d = h->d;
  sdp::StaffGyCost c{};
  c.v = d.unit_order_cost;
  c.salary = d.holding_cost;
  c.pen = d.penalty_cost;
  c.min_staff = (int32_t)h->per[(size_t)period - 1].overhead;
  c.clamp = d.clamp_inventory;
  c.min_x = (int32_t)d.min_inventory;
  c.max_x = (int32_t)d.max_inventory;
  return c;
}

// the stored grid of period + 1 (nothing to leave in period T)
void next_grid(const sdpgpu_handle* h, int period, int64_t* x_lo, int64_t* nx) {
  *x_lo = 0;
  *nx = 0;
  if (period < h->T) {
    *x_lo = (int64_t)h->per[(size_t)period].g.x_lo;
    *nx = h->per[(size_t)period].g.nx;
  }
}

// the levels y_lo .. y_lo + n - 1 of `period` are rows of its table and none of them is off the grid
int check_levels(sdpgpu_handle* h, const char* who, int period, int32_t y_lo, int32_t n) {
  const int32_t n_rows = h->lvl_rows[(size_t)period - 1];
  if (n < 0) return fail(h, SDPGPU_ERR_ARG, "%s: n = %d (at least 0)", who, n);
  if (y_lo < 0) return fail(h, SDPGPU_ERR_ARG, "%s: y_lo = %d (levels start at 0)", who, y_lo);
  if ((int64_t)y_lo + n > n_rows)
    return fail(h, SDPGPU_ERR_ARG, "%s: level %d is not a row of period %d's table (n_rows = %d: levels 0 .. %d)", who, std::max(y_lo, n_rows), period, n_rows,
                n_rows - 1);
  if (period == h->T) return SDPGPU_OK;
  const sdp::StaffGyCost c = cost_of(h, period);
  int64_t x_lo, nx;
  next_grid(h, period, &x_lo, &nx);
  const std::vector<int32_t>& len = h->lvl_len[(size_t)period - 1];
  for (int32_t y = y_lo; y < y_lo + n; ++y) {
    int bj, bn;
    if (sdp::staff_gy_first_off_grid(c, y, len[(size_t)y], x_lo, nx, &bj, &bn))
      return fail(h, SDPGPU_ERR_ARG, "%s: level %d of period %d is off the grid: its successor %d (j = %d) lies outside period %d's staff numbers %lld .. %lld", who,
                  y, period, bn, bj, period + 1, (long long)x_lo, (long long)(x_lo + nx - 1));
  }
  return SDPGPU_OK;
}

// what G of `period` needs from the solve
int check_solved_for(sdpgpu_handle* h, const char* who, int period, bool need_g, bool need_v) {
  if (!h->allocated || !h->policy_done[(size_t)period - 1]) return fail(h, SDPGPU_ERR_STATE, "%s: period %d has not been solved", who, period);
  if (need_g && period < h->T && !h->period_done[(size_t)period])
    return fail(h, SDPGPU_ERR_STATE, "%s: G of period %d needs V_%d, which has not been computed or was overwritten (store_all_values = 0 keeps two tables)", who,
                period, period + 1);
  if (need_v && !h->period_done[(size_t)period - 1])
    return fail(h, SDPGPU_ERR_STATE, "%s: V_%d has not been computed or was overwritten (store_all_values = 0 keeps two tables)", who, period);
  return SDPGPU_OK;
}

// one device block per call, released on every path
struct DeviceBlock {
  char* base = nullptr;
  ~DeviceBlock() {
    if (base) (void)hipFree(base);
  }
};

// the record of one G row of the handle over a level window, its values going to d_out
sdp::StaffGyRow row_of(const sdpgpu_handle* h, int period, int32_t y_lo, int32_t n, double* d_out) {
  sdp::StaffGyRow R{};
  R.pT = h->d_lvl_p[(size_t)period - 1];
  R.row_len = h->d_lvl_len[(size_t)period - 1];
  R.v_next = period < h->T ? h->d_values + h->per[(size_t)period].v_off : nullptr;
  R.out = d_out;
  R.c = cost_of(h, period);
  R.n_rows = h->lvl_rows[(size_t)period - 1];
  R.y_lo = y_lo;
  R.n = n;
  R.next_x_lo = period < h->T ? (int32_t)h->per[(size_t)period].g.x_lo : 0;
  return R;
}

// G of `period` over a window, made on the handle's stream: ONE device block [n doubles][the record][the blocks].  The call
// object outlives the stream's work, because the uploads read `row` and `blocks`.
struct GyCall {
  DeviceBlock blk;
  sdp::StaffGyRow row{};
  std::vector<sdp::StaffGyBlock> blocks;
  double* d_g = nullptr;
};

int launch_window(sdpgpu_handle* h, int period, int32_t y_lo, int32_t n, GyCall* call) {
  Carve c;
  const size_t o_g = c.take(std::max<size_t>((size_t)n, 1) * sizeof(double)), o_row = c.take(sizeof(sdp::StaffGyRow));
  const size_t o_blk = c.take(((size_t)n + 63) / 64 * sizeof(sdp::StaffGyBlock) + 16);
  HIP_TRY(h, hipMalloc((void**)&call->blk.base, c.at));
  call->d_g = reinterpret_cast<double*>(call->blk.base + o_g);
  call->row = row_of(h, period, y_lo, n, call->d_g);
  staff_gy_blocks(&call->row, 1, &call->blocks);
  HIP_TRY(h, launch_staff_gy(h->stream, &call->row, 1, call->blocks, reinterpret_cast<sdp::StaffGyRow*>(call->blk.base + o_row),
                             reinterpret_cast<sdp::StaffGyBlock*>(call->blk.base + o_blk)));
  return SDPGPU_OK;
}

// the first maximal run of levels of `period` that are not off the grid; *lo > *hi: none
void range_of(const sdpgpu_handle* h, int period, int32_t* lo, int32_t* hi) {
  const int32_t n_rows = h->lvl_rows[(size_t)period - 1];
  *lo = 0;
  *hi = n_rows - 1;
  if (period == h->T) return;
  const sdp::StaffGyCost c = cost_of(h, period);
  int64_t x_lo, nx;
  next_grid(h, period, &x_lo, &nx);
  const std::vector<int32_t>& len = h->lvl_len[(size_t)period - 1];
  int bj, bn;
  int32_t y = 0;
  while (y < n_rows && sdp::staff_gy_first_off_grid(c, y, len[(size_t)y], x_lo, nx, &bj, &bn)) ++y;
  *lo = y;
  while (y < n_rows && !sdp::staff_gy_first_off_grid(c, y, len[(size_t)y], x_lo, nx, &bj, &bn)) ++y;
  *hi = y - 1;
  if (*lo >= n_rows) {
    *lo = 0;
    *hi = -1;
  }
}

}  // namespace

extern "C" {

int sdpgpu_staff_gy_host(double unit_vari_cost, double salary, double unit_penalty, int32_t min_staff, const double* prob, const int32_t* row_len,
                         int32_t n_rows, int32_t row_stride, const double* v_next, int32_t v_x_lo, int64_t v_nx, int32_t clamp, int32_t min_x,
                         int32_t max_x, int32_t y_lo, int32_t n, double* out) {
  g_create_error.clear();
  sdpgpu_handle* const none = nullptr;  // (the text goes to sdpgpu_batch_last_error(NULL))
  return guarded(none, "sdpgpu_staff_gy_host", [&]() -> int {
    const char* who = "sdpgpu_staff_gy_host";
    if (!out) return fail(none, SDPGPU_ERR_ARG, "%s: out is null", who);
    if (n < 0) return fail(none, SDPGPU_ERR_ARG, "%s: n = %d (at least 0)", who, n);
    if (!prob || n_rows < 1 || row_stride < 1)
      return fail(none, SDPGPU_ERR_ARG, "%s: bad table (prob %s, n_rows = %d, row_stride = %d)", who, prob ? "set" : "null", n_rows, row_stride);
    if (y_lo < 0) return fail(none, SDPGPU_ERR_ARG, "%s: y_lo = %d (levels start at 0)", who, y_lo);
    if ((int64_t)y_lo + n > n_rows)
      return fail(none, SDPGPU_ERR_ARG, "%s: level %d is not a row of the table (n_rows = %d: levels 0 .. %d)", who, std::max(y_lo, n_rows), n_rows, n_rows - 1);
    if (v_next && v_nx < 1) return fail(none, SDPGPU_ERR_ARG, "%s: v_next holds v_nx = %lld values (at least 1)", who, (long long)v_nx);
    sdp::StaffGyCost c{};
    c.v = unit_vari_cost;
    c.salary = salary;
    c.pen = unit_penalty;
    c.min_staff = min_staff;
    c.clamp = clamp;
    c.min_x = min_x;
    c.max_x = max_x;
    auto len_of = [&](int32_t y) { return row_len ? row_len[y] : y + 1; };
    for (int32_t y = y_lo; y < y_lo + n; ++y) {
      const int32_t nj = len_of(y);
      if (nj < 1 || nj > y + 1 || nj > row_stride)
        return fail(none, SDPGPU_ERR_ARG, "%s: row %d has %d entries (1 .. min(y + 1, row_stride) allowed)", who, y, nj);
      int bj, bn;
      if (v_next && sdp::staff_gy_first_off_grid(c, y, nj, v_x_lo, v_nx, &bj, &bn))
        return fail(none, SDPGPU_ERR_ARG, "%s: level %d is off the grid: its successor %d (j = %d) lies outside v_next's staff numbers %d .. %lld", who, y, bn,
                    bj, v_x_lo, (long long)v_x_lo + v_nx - 1);
    }
    for (int32_t y = y_lo; y < y_lo + n; ++y)
      out[y - y_lo] = sdp::staff_gy_level(c, y, prob + (size_t)y * (size_t)row_stride, 1, len_of(y), v_next, v_x_lo);
    return SDPGPU_OK;
  });
}

int sdpgpu_staff_gy_range(sdpgpu_handle* h, int32_t period, int32_t* y_lo, int32_t* y_hi) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_staff_gy_range", [&]() -> int {
    const char* who = "sdpgpu_staff_gy_range";
    int rc = check_scope(h, who);
    if (rc) return rc;
    if (period < 1 || period > h->T) return fail(h, SDPGPU_ERR_ARG, "%s: period = %d (1 .. %d)", who, period, h->T);
    if (!y_lo || !y_hi) return fail(h, SDPGPU_ERR_ARG, "%s: null output", who);
    rc = layout(h);
    if (rc) return rc;
    range_of(h, period, y_lo, y_hi);
    return SDPGPU_OK;
  });
}

int sdpgpu_staff_gy(sdpgpu_handle* h, int32_t period, int32_t y_lo, int32_t n, double* out) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_staff_gy", [&]() -> int {
    const char* who = "sdpgpu_staff_gy";
    int rc = check_scope(h, who);
    if (rc) return rc;
    if (period < 1 || period > h->T) return fail(h, SDPGPU_ERR_ARG, "%s: period = %d (1 .. %d)", who, period, h->T);
    if (!out) return fail(h, SDPGPU_ERR_ARG, "%s: out is null", who);
    rc = layout(h);  // (the refusals of the levels are host arithmetic on the layout: they come before the state of the solve)
    if (rc) return rc;
    rc = check_levels(h, who, period, y_lo, n);
    if (rc) return rc;
    rc = check_solved_for(h, who, period, true, false);
    if (rc || n == 0) return rc;
    rc = ensure_device(h);
    if (rc) return rc;
    rc = flush_api(h);
    if (rc) return rc;
    GyCall call;
    rc = launch_window(h, period, y_lo, n, &call);
    if (rc) return rc;
    std::vector<double> host((size_t)n);  // (out is written only once everything has succeeded)
    HIP_TRY(h, hipMemcpyAsync(host.data(), call.d_g, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::memcpy(out, host.data(), (size_t)n * sizeof(double));
    return SDPGPU_OK;
  });
}

int sdpgpu_staff_check_convexity(sdpgpu_handle* h, int32_t kind, int32_t source, int32_t period, int32_t lo, int32_t hi, double K, int32_t capacity,
                                 sdpgpu_convexity* out) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_staff_check_convexity", [&]() -> int {
    const char* who = "sdpgpu_staff_check_convexity";
    int rc = check_scope(h, who);
    if (rc) return rc;
    if (kind != 0 && kind != 1) return fail(h, SDPGPU_ERR_ARG, "%s: kind = %d (0: CheckKConvexity.check, 1: CheckKConvexity.checkCK)", who, kind);
    if (source != 0 && source != 1) return fail(h, SDPGPU_ERR_ARG, "%s: source = %d (0: the row V_period, 1: the row G_period)", who, source);
    if (period < 1 || period > h->T) return fail(h, SDPGPU_ERR_ARG, "%s: period = %d (1 .. %d)", who, period, h->T);
    if (!out) return fail(h, SDPGPU_ERR_ARG, "%s: out is null", who);
    if (lo > hi) return fail(h, SDPGPU_ERR_ARG, "%s: the window %d .. %d is empty", who, lo, hi);
    rc = layout(h);
    if (rc) return rc;
    const int64_t n = (int64_t)hi - lo + 1;
    if (n > kConvexityMaxPoints)
      return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: a row of %lld points exceeds the kernel's %d (a workgroup keeps the row in LDS): narrow the window", who,
                  (long long)n, kConvexityMaxPoints);
    const PeriodInfo& p = h->per[(size_t)period - 1];
    if (source == 0) {
      const int64_t x_lo = (int64_t)p.g.x_lo;
      if (lo < x_lo || hi > x_lo + p.g.nx - 1)
        return fail(h, SDPGPU_ERR_ARG, "%s: the window %d .. %d is not inside period %d's staff numbers %lld .. %lld", who, lo, hi, period, (long long)x_lo,
                    (long long)(x_lo + p.g.nx - 1));
    } else {
      rc = check_levels(h, who, period, lo, (int32_t)std::min<int64_t>(n, INT32_MAX));
      if (rc) return rc;
    }
    rc = check_solved_for(h, who, period, source == 1, source == 0);
    if (rc) return rc;
    rc = ensure_device(h);
    if (rc) return rc;
    rc = flush_api(h);
    if (rc) return rc;
    GyCall call;
    ConvexitySpec spec{};
    spec.K = K;
    spec.n = (int32_t)n;
    spec.capacity = capacity;
    if (source == 0) {
      spec.g = h->d_values + p.v_off + (lo - (int64_t)p.g.x_lo);
    } else {
      rc = launch_window(h, period, lo, (int32_t)n, &call);
      if (rc) return rc;
      spec.g = call.d_g;
    }
    std::string why;
    rc = convexity_on_device(h->stream, kind, &spec, 1, out, &why);
    if (rc) return fail(h, rc, "%s: %s", who, why.c_str());
    return SDPGPU_OK;
  });
}

}  // extern "C"
