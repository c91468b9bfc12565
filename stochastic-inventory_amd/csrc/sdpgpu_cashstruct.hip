// sdpgpu_cashstruct.hip -- sdpgpu_cash_g_table, sdpgpu_cash_structure, sdpgpu_cash_structure_host: the structure tables of the cash
// drivers and their checks (kernels and the shared per-element functions: sdp_cash_structure.hpp; definition: DESIGN 4, "Cash
// structure tables").  All validation comes before the first device call.
#include "sdpgpu_sim_host.hpp"
#include "sdp_cash_structure.hpp"

using namespace sdpgpu_detail;

namespace {

static_assert(sizeof(sdp::CsVerdict) == sizeof(sdpgpu_cash_verdict), "CsVerdict mirrors sdpgpu_cash_verdict");

// table slots of a call
enum { T_G, T_GA, T_GB, T_F, T_H, T_GAGB, T_FG, T_COUNT };

struct Needs {
  bool src[4];    // G, GA, GB, F are read
  bool tab[3];    // H, GB - GA - K, F - G - v j take part in the call
  bool given[3];  // ... as the caller's own table (source 1): not formed
  bool cross, noninc[3], nondec[3];
  bool formed(int s) const { return tab[s] && !given[s]; }
};

Needs needs_of(const sdpgpu_cash_structure_in* in) {
  const int32_t mask = in->mask;
  const double* own[3] = {in->h, in->gagb, in->fg};
  Needs n{};
  n.cross = mask & SDPGPU_CSTRUCT_SINGLE_CROSS;
  for (int s = 0; s < 3; ++s) {
    n.noninc[s] = mask & SDPGPU_CSTRUCT_NONINC(s);
    n.nondec[s] = mask & SDPGPU_CSTRUCT_NONDEC(s);
    n.tab[s] = (mask & (1 << s)) || n.noninc[s] || n.nondec[s];
  }
  n.tab[0] = n.tab[0] || n.cross;
  for (int s = 0; s < 3; ++s) n.given[s] = n.tab[s] && in->source == 1 && own[s];
  n.src[T_G] = n.formed(0) || n.formed(2);
  n.src[T_GA] = n.src[T_GB] = n.formed(1);
  n.src[T_F] = n.formed(2);
  return n;
}

const char* kSrcName[4] = {"g", "ga", "gb", "f"};

// the refusals both entry points share; h only receives the text
int check_request(sdpgpu_handle* h, const char* who, const sdpgpu_cash_structure_in* in, const sdpgpu_cash_structure_out* out) {
  if (!in) return fail(h, SDPGPU_ERR_ARG, "%s: in is null", who);
  if (!out) return fail(h, SDPGPU_ERR_ARG, "%s: out is null", who);
  if (in->source != 0 && in->source != 1) return fail(h, SDPGPU_ERR_ARG, "%s: source = %d (0: the handle's tables, 1: the caller's)", who, in->source);
  if (in->mask < 1 || in->mask > SDPGPU_CSTRUCT_ALL) return fail(h, SDPGPU_ERR_ARG, "%s: mask = 0x%x (SDPGPU_CSTRUCT_* bits, 1 .. 0x%x)", who, in->mask, SDPGPU_CSTRUCT_ALL);
  if (in->n_r < 1) return fail(h, SDPGPU_ERR_ARG, "%s: n_r = %d (at least 1)", who, in->n_r);
  if (in->n_x < 1) return fail(h, SDPGPU_ERR_ARG, "%s: n_x = %d (at least 1)", who, in->n_x);
  return SDPGPU_OK;
}

int check_limits(sdpgpu_handle* h, const char* who, const sdpgpu_cash_structure_in* in) {
  if (in->n_r > SDPGPU_CSTRUCT_MAX_AXIS) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: n_r = %d exceeds %d points", who, in->n_r, SDPGPU_CSTRUCT_MAX_AXIS);
  if (in->n_x > SDPGPU_CSTRUCT_MAX_AXIS) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: n_x = %d exceeds %d points", who, in->n_x, SDPGPU_CSTRUCT_MAX_AXIS);
  if ((int64_t)in->n_r * in->n_x > SDPGPU_CSTRUCT_MAX_POINTS)
    return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: n_r * n_x = %lld exceeds %d points", who, (long long)in->n_r * in->n_x, SDPGPU_CSTRUCT_MAX_POINTS);
  return SDPGPU_OK;
}

int check_caller_tables(sdpgpu_handle* h, const char* who, const sdpgpu_cash_structure_in* in, const Needs& nd) {
  const double* src[4] = {in->g, in->ga, in->gb, in->f};
  for (int s = 0; s < 4; ++s)
    if (nd.src[s] && !src[s]) return fail(h, SDPGPU_ERR_ARG, "%s: mask 0x%x reads table %s, which is null", who, in->mask, kSrcName[s]);
  return SDPGPU_OK;
}

// getH's index check (where Java would throw), before any table is written
int check_h_index(sdpgpu_handle* h, const char* who, const sdpgpu_cash_structure_in* in) {
  int bi, bk;
  sdp::cs_h_first_overflow(in->n_r, in->n_x, in->min_cash, in->fix_cost, in->vari_cost, &bi, &bk);
  if (bi < 0) return SDPGPU_OK;
  const double cash = sdp::cs_cash(in->min_cash, bi);
  return fail(h, SDPGPU_ERR_ARG, "%s: getH at (i, j, k) = (%d, 0, %d): cashIndex = (int)(%g - %g - %g * %d) = %d is not a row of the table (n_r = %d)", who,
              bi, bk, cash, in->fix_cost, in->vari_cost, bk, sdp::cs_cash_index(cash, in->fix_cost, in->vari_cost, bk), in->n_r);
}

// the scope of a handle, naming the field
int check_scope(sdpgpu_handle* h, const char* who) {
  const sdpgpu_desc& d = h->d;
  if (h->custom) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: a user functor's lambdas are not the closed-form cash cell the tables are defined on", who);
  if (d.family != SDPGPU_FAMILY_CASH) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: family = %d -- the structure tables are those of a CASH handle", who, d.family);
  if (d.cash_formula != 1) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: cash_formula = %d -- built for formula 1 (CashConstraintTesting's lambdas)", who, d.cash_formula);
  if (d.step != 1.0) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: step = %g -- the tables index levels by unit steps", who, d.step);
  if (d.cash_round_mult != 1.0 || d.cash_round_div != 1.0)
    return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: cash_round_mult = %g, cash_round_div = %g -- rows are whole units of cash (an integer cash grid)", who,
                d.cash_round_mult, d.cash_round_div);
  if (d.world_size != 1) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: world_size = %d -- needs the whole value table on one GPU", who, d.world_size);
  if (!d.clamp_inventory) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: clamp_inventory = 0 -- the levels come from the grid [min_inventory, max_inventory]", who);
  return SDPGPU_OK;
}

// the window of a handle: whole numbers inside the grid
int check_window(sdpgpu_handle* h, const char* who, double x_lo, int32_t n_x, double cash_lo, int32_t n_r, const char* cash_name) {
  const sdpgpu_desc& d = h->d;
  if (n_x < 1) return fail(h, SDPGPU_ERR_ARG, "%s: n_x = %d (at least 1)", who, n_x);
  if (n_r < 1) return fail(h, SDPGPU_ERR_ARG, "%s: n_r = %d (at least 1)", who, n_r);
  if (!std::isfinite(x_lo) || x_lo != std::floor(x_lo)) return fail(h, SDPGPU_ERR_ARG, "%s: x_lo = %g is not a whole number", who, x_lo);
  if (!std::isfinite(cash_lo) || cash_lo != std::floor(cash_lo)) return fail(h, SDPGPU_ERR_ARG, "%s: %s = %g is not a whole number", who, cash_name, cash_lo);
  if (x_lo < d.min_inventory || x_lo + (double)(n_x - 1) > d.max_inventory)
    return fail(h, SDPGPU_ERR_ARG, "%s: x_lo = %g, n_x = %d -- levels %g .. %g outside [min_inventory, max_inventory] = [%g, %g]", who, x_lo, n_x, x_lo,
                x_lo + (double)(n_x - 1), d.min_inventory, d.max_inventory);
  if (cash_lo < d.min_cash || cash_lo + (double)(n_r - 1) > d.max_cash)
    return fail(h, SDPGPU_ERR_ARG, "%s: %s = %g, n_r = %d -- cash %g .. %g outside [min_cash, max_cash] = [%g, %g]", who, cash_name, cash_lo, n_r, cash_lo,
                cash_lo + (double)(n_r - 1), d.min_cash, d.max_cash);
  return SDPGPU_OK;
}

// what a G table of `period` needs from the solve (need_f: V_period itself too)
int check_solved_for(sdpgpu_handle* h, const char* who, int period, bool need_g, bool need_f) {
  if (!h->allocated || !h->policy_done[(size_t)period - 1]) return fail(h, SDPGPU_ERR_STATE, "%s: period %d has not been solved", who, period);
  if (need_g && period < h->T && !h->period_done[(size_t)period])
    return fail(h, SDPGPU_ERR_STATE, "%s: G of period %d needs V_%d, which has not been computed or was overwritten (store_all_values = 0 keeps two tables)", who,
                period, period + 1);
  if (need_f && !h->period_done[(size_t)period - 1])
    return fail(h, SDPGPU_ERR_STATE, "%s: F of period %d is V_%d, which has not been computed or was overwritten (store_all_values = 0 keeps two tables)", who,
                period, period);
  return SDPGPU_OK;
}

// the G launch of `n_kinds` kinds into d_out (kind z at element offset off[z])
hipError_t launch_g(sdpgpu_handle* h, int period, double x_lo, int n_x, double cash_lo, int n_r, int n_kinds, const int32_t* kinds, const int64_t* off,
                    double* d_out) {
  const DevParams P = make_params(h, period);
  const PeriodInfo& p = h->per[(size_t)period - 1];
  sdp::CashGLaunch L{};
  L.x_lo = x_lo;
  L.cash_lo = cash_lo;
  L.n_x = n_x;
  L.n_r = n_r;
  for (int z = 0; z < n_kinds; ++z) {
    L.kinds[z] = kinds[z];
    L.out_off[z] = off[z];
  }
  const bool last = period == h->T;
  L.next_states = last ? 0 : h->per[(size_t)period].S;
  const double* v_next = last ? nullptr : h->d_values + h->per[(size_t)period].v_off;
  const double* pd = h->d_pmf + p.pmf_off;
  const dim3 grid((unsigned)((n_r + 63) / 64), (unsigned)((n_x + 3) / 4), (unsigned)n_kinds);
  if (last)
    hipLaunchKernelGGL((sdp::cash_g_kernel<true>), grid, dim3(256), 0, h->stream, P, L, pd, pd + p.nD, v_next, d_out);
  else
    hipLaunchKernelGGL((sdp::cash_g_kernel<false>), grid, dim3(256), 0, h->stream, P, L, pd, pd + p.nD, v_next, d_out);
  return hipGetLastError();
}

// one device block per call, released on every path
struct DeviceBlock {
  char* base = nullptr;
  ~DeviceBlock() {
    if (base) (void)hipFree(base);
  }
};
struct Events {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~Events() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

void write_verdict(sdpgpu_cash_verdict* dst, const sdp::CsVerdict& v) { std::memcpy(dst, &v, sizeof v); }

void reset_verdicts(sdpgpu_cash_structure_out* out) {
  const sdp::CsVerdict hold = sdp::cs_holds();
  write_verdict(&out->single_crossing, hold);
  for (int s = 0; s < 3; ++s) {
    write_verdict(&out->non_increasing[s], hold);
    write_verdict(&out->non_decreasing[s], hold);
  }
  out->kernel_ms = 0.0;
}

}  // namespace

extern "C" {

int sdpgpu_cash_g_table(sdpgpu_handle* h, int32_t kind, int32_t period, double x_lo, int32_t n_x, double cash_lo, int32_t n_r, double* out) {
  if (!h) return SDPGPU_ERR_ARG;
  h->err.clear();
  return guarded(h, "sdpgpu_cash_g_table", [&]() -> int {
    const char* who = "sdpgpu_cash_g_table";
    int rc = check_scope(h, who);
    if (rc) return rc;
    if (kind < SDPGPU_CASH_G || kind > SDPGPU_CASH_GB) return fail(h, SDPGPU_ERR_ARG, "%s: kind = %d (SDPGPU_CASH_G 0, SDPGPU_CASH_GA 1, SDPGPU_CASH_GB 2)", who, kind);
    if (period < 1 || period > h->T) return fail(h, SDPGPU_ERR_ARG, "%s: period = %d (1 .. %d)", who, period, h->T);
    if (!out) return fail(h, SDPGPU_ERR_ARG, "%s: out is null", who);
    rc = check_window(h, who, x_lo, n_x, cash_lo, n_r, "cash_lo");
    if (rc) return rc;
    if (n_x > SDPGPU_CASH_G_MAX_AXIS) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: n_x = %d exceeds %d points", who, n_x, SDPGPU_CASH_G_MAX_AXIS);
    if (n_r > SDPGPU_CASH_G_MAX_AXIS) return fail(h, SDPGPU_ERR_UNSUPPORTED, "%s: n_r = %d exceeds %d points", who, n_r, SDPGPU_CASH_G_MAX_AXIS);
    rc = check_solved_for(h, who, period, true, false);
    if (rc) return rc;
    rc = ensure_device(h);
    if (rc) return rc;
    rc = flush_api(h);
    if (rc) return rc;
    const size_t elems = (size_t)n_r * (size_t)n_x;
    DeviceBlock blk;
    HIP_TRY(h, hipMalloc((void**)&blk.base, elems * sizeof(double)));
    const int64_t off0 = 0;
    HIP_TRY(h, launch_g(h, period, x_lo, n_x, cash_lo, n_r, 1, &kind, &off0, reinterpret_cast<double*>(blk.base)));
    HIP_TRY(h, hipMemcpyAsync(out, blk.base, elems * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SDPGPU_OK;
  });
}

int sdpgpu_cash_structure_host(const sdpgpu_cash_structure_in* in, sdpgpu_cash_structure_out* out) {
  g_create_error.clear();
  return guarded((sdpgpu_handle*)nullptr, "sdpgpu_cash_structure_host", [&]() -> int {
    const char* who = "sdpgpu_cash_structure_host";
    int rc = check_request(nullptr, who, in, out);
    if (rc) return rc;
    if (in->source != 1) return fail(nullptr, SDPGPU_ERR_ARG, "%s: source = %d -- the host entry point reads the caller's tables (source 1)", who, in->source);
    const Needs nd = needs_of(in);
    rc = check_caller_tables(nullptr, who, in, nd);
    if (rc) return rc;
    rc = check_limits(nullptr, who, in);
    if (rc) return rc;
    if (nd.formed(0) && (rc = check_h_index(nullptr, who, in))) return rc;
    const int n_r = in->n_r, n_x = in->n_x;
    const size_t elems = (size_t)n_r * (size_t)n_x;
    reset_verdicts(out);
    std::vector<double> made[3];
    std::vector<int32_t> opt;
    const double* tab[3] = {in->h, in->gagb, in->fg};  // the caller's own, or the one formed here
    for (int s = 0; s < 3; ++s)
      if (nd.formed(s)) {
        made[s].resize(elems);
        tab[s] = made[s].data();
      }
    if (nd.formed(0)) {
      opt.resize(elems);
      sdp::cash_structure_host_h(in->g, n_r, n_x, in->min_cash, in->fix_cost, in->vari_cost, made[0].data(), opt.data());
    }
    if (nd.formed(1)) sdp::cash_structure_host_gagb(in->ga, in->gb, n_r, n_x, in->min_cash, in->fix_cost, in->vari_cost, made[1].data());
    if (nd.formed(2)) sdp::cash_structure_host_fg(in->g, in->f, n_r, n_x, in->vari_cost, made[2].data());
    if (nd.cross) write_verdict(&out->single_crossing, sdp::cash_structure_host_cross(tab[0], n_r, n_x));
    for (int s = 0; s < 3; ++s) {
      if (nd.noninc[s]) write_verdict(&out->non_increasing[s], sdp::cash_structure_host_noninc(tab[s], n_r, n_x));
      if (nd.nondec[s]) write_verdict(&out->non_decreasing[s], sdp::cash_structure_host_nondec(tab[s], n_r, n_x));
    }
    const double* src[4] = {in->g, in->ga, in->gb, in->f};
    double* src_out[4] = {out->g, out->ga, out->gb, out->f};
    for (int s = 0; s < 4; ++s)
      if (nd.src[s] && src_out[s] && src_out[s] != src[s]) std::memcpy(src_out[s], src[s], elems * sizeof(double));
    double* tab_out[3] = {out->h, out->gagb, out->fg};
    for (int s = 0; s < 3; ++s)
      if (nd.tab[s] && tab_out[s] && tab_out[s] != tab[s]) std::memcpy(tab_out[s], tab[s], elems * sizeof(double));
    if (nd.formed(0) && out->opt_y) std::memcpy(out->opt_y, opt.data(), elems * sizeof(int32_t));
    return SDPGPU_OK;
  });
}

int sdpgpu_cash_structure(sdpgpu_handle* h, const sdpgpu_cash_structure_in* in, sdpgpu_cash_structure_out* out) {
  if (h)
    h->err.clear();
  else
    g_create_error.clear();
  return guarded(h, "sdpgpu_cash_structure", [&]() -> int {
    const char* who = "sdpgpu_cash_structure";
    int rc = check_request(h, who, in, out);
    if (rc) return rc;
    const Needs nd = needs_of(in);
    const int n_r = in->n_r, n_x = in->n_x;
    if (in->source == 0) {
      if (!h) return fail(nullptr, SDPGPU_ERR_ARG, "%s: source 0 reads a solved handle, h is null", who);
      rc = check_scope(h, who);
      if (rc) return rc;
      if (in->period < 1 || in->period > h->T) return fail(h, SDPGPU_ERR_ARG, "%s: period = %d (1 .. %d)", who, in->period, h->T);
      rc = check_window(h, who, in->x_lo, n_x, in->min_cash, n_r, "min_cash");
      if (rc) return rc;
    } else {
      rc = check_caller_tables(h, who, in, nd);
      if (rc) return rc;
    }
    rc = check_limits(h, who, in);
    if (rc) return rc;
    if (nd.formed(0) && (rc = check_h_index(h, who, in))) return rc;
    if (in->source == 0) {
      rc = check_solved_for(h, who, in->period, nd.src[T_G] || nd.src[T_GA] || nd.src[T_GB], nd.src[T_F]);
      if (rc) return rc;
    }

    rc = no_device(h, who);
    if (rc) return rc;
    DeviceScope dev;
    HIP_TRY(h, dev.enter(h ? h->device : in->device));
    hipStream_t st = h ? h->stream : nullptr;
    if (h && h->allocated && (rc = flush_api(h))) return rc;

    // the block: seven tables, optyIndex, next_fail, two rows, seven keys and verdicts
    const size_t elems = (size_t)n_r * (size_t)n_x;
    Carve c;
    size_t o_tab[T_COUNT];
    const bool have[T_COUNT] = {nd.src[T_G], nd.src[T_GA], nd.src[T_GB], nd.src[T_F], nd.tab[0], nd.tab[1], nd.tab[2]};
    for (int t = 0; t < T_COUNT; ++t) o_tab[t] = have[t] ? c.take(elems * sizeof(double)) : 0;
    const size_t o_opt = nd.formed(0) ? c.take(elems * sizeof(int32_t)) : 0;
    const size_t o_nf = nd.cross ? c.take(elems * sizeof(int32_t)) : 0;
    const size_t o_last = c.take((size_t)n_r * sizeof(int32_t)), o_end = c.take((size_t)n_r * sizeof(int32_t));
    const size_t o_keys = c.take(8 * sizeof(unsigned long long)), o_ver = c.take(7 * sizeof(sdp::CsVerdict));
    DeviceBlock blk;
    HIP_TRY(h, hipMalloc((void**)&blk.base, c.at));
    auto dtab = [&](int t) { return have[t] ? reinterpret_cast<double*>(blk.base + o_tab[t]) : nullptr; };
    int32_t* d_opt = reinterpret_cast<int32_t*>(blk.base + o_opt);
    int32_t* d_nf = reinterpret_cast<int32_t*>(blk.base + o_nf);
    int32_t* d_last = reinterpret_cast<int32_t*>(blk.base + o_last);
    int32_t* d_end = reinterpret_cast<int32_t*>(blk.base + o_end);
    unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(blk.base + o_keys);
    sdp::CsVerdict* d_ver = reinterpret_cast<sdp::CsVerdict*>(blk.base + o_ver);
    Events ev;
    HIP_TRY(h, hipEventCreate(&ev.e0));
    HIP_TRY(h, hipEventCreate(&ev.e1));

    const double* src[4] = {in->g, in->ga, in->gb, in->f};
    if (in->source == 1)
      for (int s = 0; s < 4; ++s)
        if (nd.src[s]) HIP_TRY(h, hipMemcpyAsync(dtab(s), src[s], elems * sizeof(double), hipMemcpyHostToDevice, st));
    const double* own[3] = {in->h, in->gagb, in->fg};
    for (int s = 0; s < 3; ++s)
      if (nd.given[s]) HIP_TRY(h, hipMemcpyAsync(dtab(T_H + s), own[s], elems * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipEventRecord(ev.e0, st));
    if (in->source == 0) {
      int32_t kinds[3];
      int64_t off[3];
      int nk = 0;
      for (int s = 0; s < 3; ++s)
        if (nd.src[s]) kinds[nk++] = s;  // (T_G, T_GA, T_GB are the kinds' numbers)
      if (nk) {
        double* first = dtab(kinds[0]);  // (the lowest of the block: the slots are carved in this order)
        for (int z = 0; z < nk; ++z) off[z] = dtab(kinds[z]) - first;
        HIP_TRY(h, launch_g(h, in->period, in->x_lo, n_x, in->min_cash, n_r, nk, kinds, off, first));
      }
      if (nd.src[T_F]) {
        const PeriodInfo& p = h->per[(size_t)in->period - 1];
        const int64_t ix0 = (int64_t)(in->x_lo - p.g.x_lo), ic0 = (int64_t)in->min_cash - p.g.k_lo;
        hipLaunchKernelGGL(sdp::cash_f_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, h->d_values + p.v_off, p.g.nc, ix0, ic0, n_r, n_x,
                           dtab(T_F));
        HIP_TRY(h, hipGetLastError());
      }
    }
    const dim3 per_elem((unsigned)((elems + 255) / 256)), per_wave((unsigned)((elems + 3) / 4));
    const double K = in->fix_cost, v = in->vari_cost;
    if (nd.formed(0)) hipLaunchKernelGGL(sdp::cash_h_kernel, per_wave, dim3(256), 0, st, dtab(T_G), n_r, n_x, in->min_cash, K, v, dtab(T_H), d_opt);
    if (nd.formed(1)) hipLaunchKernelGGL(sdp::cash_gagb_kernel, per_elem, dim3(256), 0, st, dtab(T_GA), dtab(T_GB), n_r, n_x, in->min_cash, K, v, dtab(T_GAGB));
    if (nd.formed(2)) hipLaunchKernelGGL(sdp::cash_fg_kernel, per_elem, dim3(256), 0, st, dtab(T_G), dtab(T_F), n_r, n_x, v, dtab(T_FG));
    HIP_TRY(h, hipGetLastError());
    const bool any_check = nd.cross || nd.noninc[0] || nd.noninc[1] || nd.noninc[2] || nd.nondec[0] || nd.nondec[1] || nd.nondec[2];
    if (any_check) {
      hipLaunchKernelGGL(sdp::cs_key_fill_kernel, dim3(1), dim3(64), 0, st, d_keys, 8);
      sdp::CsFinish F{};
      F.n_r = n_r;
      F.n_x = n_x;
      F.last = d_last;
      for (int s = 0; s < 3; ++s) F.tab[s] = dtab(T_H + s);
      if (nd.cross) {
        F.checks |= 1u;
        hipLaunchKernelGGL(sdp::cs_last_pass_kernel, dim3((unsigned)((n_r + 3) / 4)), dim3(256), 0, st, dtab(T_H), n_r, n_x, d_last);
        hipLaunchKernelGGL(sdp::cs_col_suffix_kernel, dim3((unsigned)((n_x + 255) / 256)), dim3(256), 0, st, dtab(T_H), n_r, n_x, d_nf);
        hipLaunchKernelGGL(sdp::cs_row_scan_kernel, dim3(1), dim3(64), 0, st, d_last, n_r, d_end);
        hipLaunchKernelGGL(sdp::cs_cross_kernel, per_elem, dim3(256), 0, st, d_last, d_end, d_nf, n_r, n_x, d_keys + 0);
      }
      for (int s = 0; s < 3; ++s) {
        if (nd.noninc[s]) {
          F.checks |= 1u << (1 + s);
          hipLaunchKernelGGL((sdp::cs_monotone_kernel<false>), per_elem, dim3(256), 0, st, dtab(T_H + s), n_r, n_x, d_keys + 1 + s);
        }
        if (nd.nondec[s]) {
          F.checks |= 1u << (4 + s);
          hipLaunchKernelGGL((sdp::cs_monotone_kernel<true>), per_elem, dim3(256), 0, st, dtab(T_H + s), n_r, n_x, d_keys + 4 + s);
        }
      }
      hipLaunchKernelGGL(sdp::cs_finish_kernel, dim3(1), dim3(64), 0, st, F, d_keys, d_ver);
      HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(ev.e1, st));

    sdp::CsVerdict ver[7];
    if (any_check) HIP_TRY(h, hipMemcpyAsync(ver, d_ver, sizeof ver, hipMemcpyDeviceToHost, st));
    double* host_out[T_COUNT] = {out->g, out->ga, out->gb, out->f, out->h, out->gagb, out->fg};
    for (int t = 0; t < T_COUNT; ++t)
      if (have[t] && host_out[t]) HIP_TRY(h, hipMemcpyAsync(host_out[t], dtab(t), elems * sizeof(double), hipMemcpyDeviceToHost, st));
    if (nd.formed(0) && out->opt_y) HIP_TRY(h, hipMemcpyAsync(out->opt_y, d_opt, elems * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    reset_verdicts(out);
    out->kernel_ms = ms;
    if (nd.cross) write_verdict(&out->single_crossing, ver[0]);
    for (int s = 0; s < 3; ++s) {
      if (nd.noninc[s]) write_verdict(&out->non_increasing[s], ver[1 + s]);
      if (nd.nondec[s]) write_verdict(&out->non_decreasing[s], ver[4 + s]);
    }
    return SDPGPU_OK;
  });
}

}  // extern "C"
