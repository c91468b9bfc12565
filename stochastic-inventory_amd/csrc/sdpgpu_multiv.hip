// sdpgpu_multiv.hip -- sdpgpu_multiv_solve: sdp.cash.multiItem.CashRecursionV (CashRecursionV.java:83-194) on the
// reachable-set engine, for the lambdas of cash.multiItem.MultiItemYR.main (MultiItemYR.java:104-158) and MultiItemYRTesting.main
// (MultiItemYRTesting.java:100-101, 163-165).  The kernels are in sdp_multiv.hpp; this file checks the descriptor (before any
// device call), bounds the integer lattice the V states of periods 2 .. T live on, and runs the two passes:
//
//   forward  t = 1 .. T  : distinct R of S_t by bit pattern (radix sort + unique), the Pi entries E_t as flags over the dense
//                          (R, y1, y2) table, compacted to a list; for t < T the successors of E_t and of the alpha line of
//                          every R are marked on the lattice and the marks compacted to S_{t+1}.
//   backward t = T .. 1  : Pi over E_t and the alpha lines (V_{t+1} dense on the lattice), then the V, y* and alpha scans.
//
// The reference computes alpha(t, R) only where y*(t, R) is not affordable, which depends on values; the engine evaluates the
// alpha line of every (t, R), so its memo is a superset of the reference's (V is a pure function of the state) and the counts
// it reports are its own.  The error text, the exception barrier and the V-state table are those of the other two-product
// solvers (sdp_multi_device.hpp).
#include "sdp_multi_device.hpp"
#include "sdp_multiv.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

using namespace sdp_multiv;
using sdp_multi::ml_error;

thread_local sdpgpu_multiv_rtable* g_rtable = nullptr;

constexpr long long kMaxLattice = 1LL << 27;  // points of the dense V_{t+1} (1 GiB of values)
constexpr long long kMaxPiTable = 1LL << 28;  // entries of one period's dense Pi table

struct DeviceError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct Unsupported : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define MV_TRY(expr)                                                                          \
  do {                                                                                        \
    const hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) throw DeviceError(std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <class T>
struct Buf {
  T* p = nullptr;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  void alloc(long long n) {
    release();
    MV_TRY(hipMalloc((void**)&p, (size_t)std::max<long long>(n, 1) * sizeof(T)));
  }
  void swap(Buf& o) { std::swap(p, o.p); }
};

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

// what the descriptor describes, as the passes read it
struct Plan {
  int T = 0;
  VParams P{};
  State ini{};
  std::vector<int> off;
  std::vector<double2> dem;
  std::vector<double> prob;
  long long lattice = 1;
};

bool whole(double v) { return std::isfinite(v) && std::fabs(v) < 2147483648.0 && v == std::floor(v); }

int refuse(int rc, const std::string& text) {
  ml_error() = "multiv: " + text;
  return rc;
}

int multiv_plan(const sdpgpu_multiv* k, Plan& pl) {
  if (!k) return refuse(SDPGPU_ERR_ARG, "NULL descriptor");
  if (k->T < 1 || k->T > 16) return refuse(SDPGPU_ERR_ARG, "T must be 1 .. 16");
  for (int i = 0; i < 2; ++i) {
    if (k->q_bound[i] < 1 || k->q_bound[i] > 1024) return refuse(SDPGPU_ERR_ARG, "q_bound must be 1 .. 1024 for both products");
    if (!(k->vari_cost[i] > 0) || !std::isfinite(k->vari_cost[i]))
      return refuse(SDPGPU_ERR_ARG, "vari_cost must be > 0 (the alpha line divides by it)");
    if (!std::isfinite(k->price[i]) || !std::isfinite(k->sal_price[i])) return refuse(SDPGPU_ERR_ARG, "price and sal_price must be finite");
  }
  if (k->rounding != SDPGPU_MULTIV_TRUNC10 && k->rounding != SDPGPU_MULTIV_ROUND)
    return refuse(SDPGPU_ERR_ARG, "rounding must be SDPGPU_MULTIV_TRUNC10 or SDPGPU_MULTIV_ROUND");
  if (!std::isfinite(k->deposit_rate)) return refuse(SDPGPU_ERR_ARG, "deposit_rate must be finite");
  if (!whole(k->min_cash) || !whole(k->max_cash) || !whole(k->min_inventory) || !whole(k->max_inventory))
    return refuse(SDPGPU_ERR_ARG, "min_cash, max_cash, min_inventory and max_inventory must be integers (the states of periods 2 .. T "
                                  "live on an integer lattice)");
  if (k->min_cash < 0)
    return refuse(SDPGPU_ERR_ARG, "min_cash < 0: a state without an affordable level would return -Double.MAX_VALUE");
  if (!std::isfinite(k->ini_cash) || k->ini_cash < 0)
    return refuse(SDPGPU_ERR_ARG, "ini_cash < 0: a state without an affordable level would return -Double.MAX_VALUE");
  if (k->max_cash < k->min_cash) return refuse(SDPGPU_ERR_ARG, "max_cash < min_cash");
  if (k->max_inventory < 0) return refuse(SDPGPU_ERR_ARG, "max_inventory < 0");
  if (!whole(k->ini_i1) || !whole(k->ini_i2) || k->ini_i1 < 0 || k->ini_i2 < 0)
    return refuse(SDPGPU_ERR_ARG, "ini_i1 and ini_i2 must be non-negative integers (the V box starts at (int) x)");
  if (!k->pmf_off || !k->d1 || !k->d2 || !k->p) return refuse(SDPGPU_ERR_ARG, "pmf_off, d1, d2 and p must not be NULL");
  pl.T = k->T;
  for (int t = 0; t <= k->T; ++t) {
    if (k->pmf_off[t] < 0 || (t && (k->pmf_off[t] <= k->pmf_off[t - 1] || k->pmf_off[t] - k->pmf_off[t - 1] > 65536)))
      return refuse(SDPGPU_ERR_ARG, "pmf_off must ascend, with 1 .. 65536 demand pairs per period");
    pl.off.push_back(k->pmf_off[t] - k->pmf_off[0]);
  }
  for (int32_t j = k->pmf_off[0]; j < k->pmf_off[k->T]; ++j) {
    if (!std::isfinite(k->d1[j]) || !std::isfinite(k->d2[j]) || k->d1[j] < 0 || k->d2[j] < 0 || !std::isfinite(k->p[j]))
      return refuse(SDPGPU_ERR_ARG, "d1 / d2 must be finite and >= 0, p finite");
    pl.dem.push_back(make_double2(k->d1[j], k->d2[j]));  // CashRecursionV.java:89 keeps the doubles
    pl.prob.push_back(k->p[j]);
  }
  VParams& P = pl.P;
  for (int i = 0; i < 2; ++i) {
    P.price[i] = k->price[i];
    P.vari[i] = k->vari_cost[i];
    P.sal[i] = k->sal_price[i];
  }
  P.one_plus_dep = 1 + k->deposit_rate;
  P.min_inventory = k->min_inventory; P.max_inventory = k->max_inventory;
  P.min_cash = k->min_cash; P.max_cash = k->max_cash;
  P.q1 = k->q_bound[0]; P.q2 = k->q_bound[1];
  P.rounding = k->rounding;
  pl.ini = State{k->ini_i1, k->ini_i2, k->ini_cash};
  // The box of the rounded successors, period by period: e1 <= min(max_inventory, the largest level), e2 <= the largest level
  // (it has no upper clamp, MultiItemYR.java:155) or min_inventory, w' <= min(max_cash, the largest revenue + (1 + dep) R).  A
  // level is at most x + Q - 1 (V box), Q - 1 (y* box) or R / c (alpha line); rounding adds less than 1.
  double x1 = k->ini_i1, x2 = k->ini_i2, w = k->ini_cash;
  double n1 = 0, n2 = 0, nw = k->min_cash;
  for (int t = 1; t < k->T; ++t) {
    const double R = w + P.vari[0] * x1 + P.vari[1] * x2;
    const double y1 = std::max(x1 + P.q1 - 1, R / P.vari[0]), y2 = std::max(x2 + P.q2 - 1, R / P.vari[1]);
    x1 = std::min(k->max_inventory, std::ceil(y1) + 1);
    x2 = std::max(k->min_inventory, std::ceil(y2) + 1);
    w = std::ceil(std::fabs(P.price[0]) * y1 + std::fabs(P.price[1]) * y2 + std::fabs(P.one_plus_dep) * R) + 1;
    w = std::max(k->min_cash, std::min(k->max_cash, w));
    n1 = std::max(n1, x1); n2 = std::max(n2, x2); nw = std::max(nw, w);
    if (!(n1 < 1e9 && n2 < 1e9 && nw < 2e9)) break;
  }
  const double points = (n1 + 1) * (n2 + 1) * (nw - k->min_cash + 1);
  if (!(points <= (double)kMaxLattice))
    return refuse(SDPGPU_ERR_UNSUPPORTED, "the lattice (x1, x2, w) the bounds max_inventory / max_cash, q_bound and T allow has more than 2^27 "
                                          "points (V_{t+1} is laid out dense on it)");
  P.n1 = (int)n1 + 1; P.n2 = (int)n2 + 1; P.nw = (int)(nw - k->min_cash) + 1;
  P.w0 = (int)k->min_cash;
  pl.lattice = (long long)P.n1 * P.n2 * P.nw;
  const double Y1 = std::max(n1, k->ini_i1) + P.q1, Y2 = std::max(n2, k->ini_i2) + P.q2;
  if (!(Y1 * Y2 <= (double)kMaxPiTable))
    return refuse(SDPGPU_ERR_UNSUPPORTED, "the levels the bounds and q_bound allow make one R's Pi table larger than 2^28 entries");
  P.Y1 = (int)Y1; P.Y2 = (int)Y2;
  return SDPGPU_OK;
}

// the set flags of `flags[0, n)` as ascending indices: -> how many; `out` is sized to them
long long compact(const unsigned char* flags, long long n, Buf<long long>& out) {
  Buf<long long> all, count;
  Buf<char> tmp;
  all.alloc(n);
  count.alloc(1);
  size_t bytes = 0;
  hipcub::CountingInputIterator<long long> first(0);
  MV_TRY(hipcub::DeviceSelect::Flagged(nullptr, bytes, first, flags, all.p, count.p, (int)n));
  tmp.alloc((long long)bytes);
  MV_TRY(hipcub::DeviceSelect::Flagged(tmp.p, bytes, first, flags, all.p, count.p, (int)n));
  long long m = 0;
  MV_TRY(hipMemcpy(&m, count.p, 8, hipMemcpyDeviceToHost));
  out.alloc(m);
  if (m) MV_TRY(hipMemcpy(out.p, all.p, (size_t)m * 8, hipMemcpyDeviceToDevice));
  return m;
}

struct Period {
  long long n = 0, nE = 0;
  int nR = 0;
  Buf<State> states;
  Buf<int> ridx;
  Buf<unsigned long long> rb;
  Buf<long long> entries;
};

struct Side {
  Buf<int> e1, e2;
  Buf<double> r1, r2;
  void build(const VParams& P, const double2* dem) {
    e1.alloc((long long)P.nd * P.Y1); r1.alloc((long long)P.nd * P.Y1);
    e2.alloc((long long)P.nd * P.Y2); r2.alloc((long long)P.nd * P.Y2);
    const long long n = (long long)P.nd * std::max(P.Y1, P.Y2);
    hipLaunchKernelGGL(side_kernel, dim3(blocks_of(n)), dim3(256), 0, 0, P, dem, e1.p, r1.p, e2.p, r2.p);
    MV_TRY(hipGetLastError());
  }
};

void check_oob(const Buf<int>& oob, const char* where) {
  int h = 0;
  MV_TRY(hipMemcpy(&h, oob.p, 4, hipMemcpyDeviceToHost));
  if (h) throw std::runtime_error(std::string(where) + " left the box the descriptor's bounds allow");
}

int multiv_run(const Plan& pl, sdpgpu_multiv_result* out, int64_t* states_per_period, int64_t* r_per_period,
               int64_t* entries_per_period) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    ml_error() = "no HIP device available; this library has no CPU path";
    return SDPGPU_ERR_DEVICE;
  }
  const int T = pl.T;
  VParams P = pl.P;
  // the alpha list, by the reference's own loop (CashRecursionV.java:180)
  std::vector<double> h_alpha;
  for (double alpha = 0; alpha <= 1; alpha = alpha + 0.01) h_alpha.push_back(alpha);
  if ((int)h_alpha.size() != kAlpha) throw std::runtime_error("the alpha loop did not run 100 times");

  std::vector<Period> per((size_t)T);
  Buf<double2> d_dem;
  Buf<double> d_prob, d_alpha, vnext, vcur;
  Buf<int> oob;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  struct Events {
    hipEvent_t &a, &b;
    ~Events() {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } events{ev0, ev1};
  MV_TRY(hipEventCreate(&ev0));
  MV_TRY(hipEventCreate(&ev1));
  const long long nd_all = pl.off[(size_t)T];
  d_dem.alloc(nd_all);
  d_prob.alloc(nd_all);
  d_alpha.alloc(kAlpha);
  oob.alloc(1);
  MV_TRY(hipMemcpy(d_dem.p, pl.dem.data(), (size_t)nd_all * sizeof(double2), hipMemcpyHostToDevice));
  MV_TRY(hipMemcpy(d_prob.p, pl.prob.data(), (size_t)nd_all * 8, hipMemcpyHostToDevice));
  MV_TRY(hipMemcpy(d_alpha.p, h_alpha.data(), kAlpha * 8, hipMemcpyHostToDevice));
  MV_TRY(hipMemset(oob.p, 0, 4));
  per[0].n = 1;
  per[0].states.alloc(1);
  MV_TRY(hipMemcpy(per[0].states.p, &pl.ini, sizeof(State), hipMemcpyHostToDevice));
  MV_TRY(hipEventRecord(ev0, 0));

  // ---- forward ----
  for (int t = 0; t < T; ++t) {
    Period& p = per[(size_t)t];
    P.nd = pl.off[(size_t)t + 1] - pl.off[(size_t)t];
    const double2* dem_t = d_dem.p + pl.off[(size_t)t];
    {
      // distinct R by bit pattern; period 1 also holds the driver's getYStar(1, iniCash) (MultiItemYR.java:179-180)
      const long long m = p.n + (t == 0 ? 1 : 0);
      Buf<unsigned long long> raw, sorted, uniq;
      Buf<long long> count;
      Buf<char> tmp;
      raw.alloc(m); sorted.alloc(m); uniq.alloc(m); count.alloc(1);
      hipLaunchKernelGGL(state_r_kernel, dim3(blocks_of(p.n)), dim3(256), 0, 0, P, p.states.p, p.n, raw.p);
      MV_TRY(hipGetLastError());
      if (t == 0) {
        double c = pl.ini.w + 0.0;
        unsigned long long bits;
        std::memcpy(&bits, &c, 8);
        MV_TRY(hipMemcpy(raw.p + p.n, &bits, 8, hipMemcpyHostToDevice));
      }
      size_t bytes = 0;
      MV_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, raw.p, sorted.p, (int)m));
      tmp.alloc((long long)bytes);
      MV_TRY(hipcub::DeviceRadixSort::SortKeys(tmp.p, bytes, raw.p, sorted.p, (int)m));
      bytes = 0;
      MV_TRY(hipcub::DeviceSelect::Unique(nullptr, bytes, sorted.p, uniq.p, count.p, (int)m));
      tmp.alloc((long long)bytes);
      MV_TRY(hipcub::DeviceSelect::Unique(tmp.p, bytes, sorted.p, uniq.p, count.p, (int)m));
      long long nR = 0;
      MV_TRY(hipMemcpy(&nR, count.p, 8, hipMemcpyDeviceToHost));
      p.nR = (int)nR;
      p.rb.alloc(nR);
      MV_TRY(hipMemcpy(p.rb.p, uniq.p, (size_t)nR * 8, hipMemcpyDeviceToDevice));
    }
    p.ridx.alloc(p.n);
    hipLaunchKernelGGL(state_ridx_kernel, dim3(blocks_of(p.n)), dim3(256), 0, 0, P, p.states.p, p.n, p.rb.p, p.nR, p.ridx.p);
    MV_TRY(hipGetLastError());
    const double dense_d = (double)p.nR * P.Y1 * P.Y2;
    if (!(dense_d <= (double)kMaxPiTable))
      throw Unsupported("period " + std::to_string(t + 1) + ": " + std::to_string(p.nR) + " distinct R x " + std::to_string(P.Y1) + " x " +
                        std::to_string(P.Y2) + " levels exceed the 2^28 entries of a period's Pi table");
    const long long dense = (long long)p.nR * P.Y1 * P.Y2;
    {
      Buf<unsigned char> flags;
      flags.alloc(dense);
      MV_TRY(hipMemset(flags.p, 0, (size_t)dense));
      const long long box = (long long)P.q1 * P.q2;
      hipLaunchKernelGGL(entry_mark_states_kernel, dim3(blocks_of(p.n * box)), dim3(256), 0, 0, P, p.states.p, p.n, p.ridx.p, flags.p,
                         oob.p);
      MV_TRY(hipGetLastError());
      hipLaunchKernelGGL(entry_mark_ystar_kernel, dim3(blocks_of(p.nR * box)), dim3(256), 0, 0, P, p.nR, flags.p);
      MV_TRY(hipGetLastError());
      check_oob(oob, "a level of a state's box");
      p.nE = compact(flags.p, dense, p.entries);
    }
    if (t + 1 < T) {
      Side side;
      side.build(P, dem_t);
      Buf<unsigned char> marks;
      marks.alloc(pl.lattice);
      MV_TRY(hipMemset(marks.p, 0, (size_t)pl.lattice));
      hipLaunchKernelGGL((pi_kernel<true, 0>), dim3(blocks_of(p.nE)), dim3(256), 0, 0, P, p.entries.p, p.nE, p.rb.p, d_alpha.p, dem_t,
                         (const double*)nullptr, side.e1.p, side.r1.p, side.e2.p, side.r2.p, (const double*)nullptr, marks.p,
                         (double*)nullptr, oob.p);
      MV_TRY(hipGetLastError());
      const long long na = (long long)p.nR * kAlpha;
      hipLaunchKernelGGL((pi_kernel<false, 0>), dim3(blocks_of(na)), dim3(256), 0, 0, P, (const long long*)nullptr, na, p.rb.p, d_alpha.p,
                         dem_t, (const double*)nullptr, (const int*)nullptr, (const double*)nullptr, (const int*)nullptr,
                         (const double*)nullptr, (const double*)nullptr, marks.p, (double*)nullptr, oob.p);
      MV_TRY(hipGetLastError());
      check_oob(oob, "a successor");
      Buf<long long> idx;
      Period& q = per[(size_t)t + 1];
      q.n = compact(marks.p, pl.lattice, idx);
      q.states.alloc(q.n);
      hipLaunchKernelGGL(lattice_states_kernel, dim3(blocks_of(q.n)), dim3(256), 0, 0, P, idx.p, q.n, q.states.p);
      MV_TRY(hipGetLastError());
    }
  }

  // ---- the tables asked for ----
  long long rows_v = 0, rows_r = 0;
  for (const Period& p : per) {
    rows_v += p.n;
    rows_r += p.nR;
  }
  sdpgpu_multi_table* vt = sdp_multi::ml_table();
  sdpgpu_multiv_rtable* rt = g_rtable;
  const bool fill_v = vt && rows_v <= vt->capacity, fill_r = rt && rows_r <= rt->capacity;
  if (vt) vt->rows = rows_v;
  if (rt) rt->rows = rows_r;

  // ---- backward ----
  int64_t cells = 0;
  double v1 = 0, alpha1 = 0;
  int a1_1 = 0, a2_1 = 0, ys1 = 0, ys2 = 0, cons1 = 0;
  std::vector<State> h_states;
  std::vector<double> h_val, h_alpha_out;
  std::vector<int> h_a1, h_a2, h_y1, h_y2, h_cons;
  std::vector<unsigned long long> h_rb;
  long long at_v = rows_v, at_r = rows_r;
  for (int t = T - 1; t >= 0; --t) {
    Period& p = per[(size_t)t];
    P.nd = pl.off[(size_t)t + 1] - pl.off[(size_t)t];
    const double2* dem_t = d_dem.p + pl.off[(size_t)t];
    const double* prob_t = d_prob.p + pl.off[(size_t)t];
    const bool last = t == T - 1;
    Side side;
    side.build(P, dem_t);
    const long long dense = (long long)p.nR * P.Y1 * P.Y2, na = (long long)p.nR * kAlpha;
    Buf<double> pi, pia, value, alpha_out;
    Buf<int> a1, a2, y1s, y2s, cons;
    pi.alloc(dense);
    pia.alloc(na);
    MV_TRY(hipMemset(pi.p, 0xFF, (size_t)dense * 8));  // (NaN: an entry that was not flagged is never read)
    if (last) {
      hipLaunchKernelGGL((pi_kernel<true, 2>), dim3(blocks_of(p.nE)), dim3(256), 0, 0, P, p.entries.p, p.nE, p.rb.p, d_alpha.p, dem_t, prob_t,
                         side.e1.p, side.r1.p, side.e2.p, side.r2.p, (const double*)nullptr, (unsigned char*)nullptr, pi.p, oob.p);
      MV_TRY(hipGetLastError());
      hipLaunchKernelGGL((pi_kernel<false, 2>), dim3(blocks_of(na)), dim3(256), 0, 0, P, (const long long*)nullptr, na, p.rb.p, d_alpha.p,
                         dem_t, prob_t, (const int*)nullptr, (const double*)nullptr, (const int*)nullptr, (const double*)nullptr,
                         (const double*)nullptr, (unsigned char*)nullptr, pia.p, oob.p);
    } else {
      hipLaunchKernelGGL((pi_kernel<true, 1>), dim3(blocks_of(p.nE)), dim3(256), 0, 0, P, p.entries.p, p.nE, p.rb.p, d_alpha.p, dem_t, prob_t,
                         side.e1.p, side.r1.p, side.e2.p, side.r2.p, vnext.p, (unsigned char*)nullptr, pi.p, oob.p);
      MV_TRY(hipGetLastError());
      hipLaunchKernelGGL((pi_kernel<false, 1>), dim3(blocks_of(na)), dim3(256), 0, 0, P, (const long long*)nullptr, na, p.rb.p, d_alpha.p,
                         dem_t, prob_t, (const int*)nullptr, (const double*)nullptr, (const int*)nullptr, (const double*)nullptr, vnext.p,
                         (unsigned char*)nullptr, pia.p, oob.p);
    }
    MV_TRY(hipGetLastError());
    cells += (int64_t)(p.nE + na) * P.nd;
    value.alloc(p.n); a1.alloc(p.n); a2.alloc(p.n);
    if (t > 0) {
      vcur.alloc(pl.lattice);
      MV_TRY(hipMemset(vcur.p, 0xFF, (size_t)pl.lattice * 8));
      hipLaunchKernelGGL(v_scan_kernel<true>, dim3(blocks_of(p.n)), dim3(256), 0, 0, P, p.states.p, p.n, p.ridx.p, pi.p, vcur.p, value.p,
                         a1.p, a2.p);
    } else {
      hipLaunchKernelGGL(v_scan_kernel<false>, dim3(blocks_of(p.n)), dim3(256), 0, 0, P, p.states.p, p.n, p.ridx.p, pi.p, (double*)nullptr,
                         value.p, a1.p, a2.p);
    }
    MV_TRY(hipGetLastError());
    y1s.alloc(p.nR); y2s.alloc(p.nR); cons.alloc(p.nR); alpha_out.alloc(p.nR);
    hipLaunchKernelGGL(ystar_kernel, dim3(blocks_of(p.nR)), dim3(256), 0, 0, P, p.rb.p, p.nR, pi.p, pia.p, d_alpha.p, y1s.p, y2s.p, cons.p,
                       alpha_out.p);
    MV_TRY(hipGetLastError());
    if (fill_v || t == 0) {
      h_states.resize((size_t)p.n); h_val.resize((size_t)p.n); h_a1.resize((size_t)p.n); h_a2.resize((size_t)p.n);
      MV_TRY(hipMemcpy(h_states.data(), p.states.p, (size_t)p.n * sizeof(State), hipMemcpyDeviceToHost));
      MV_TRY(hipMemcpy(h_val.data(), value.p, (size_t)p.n * 8, hipMemcpyDeviceToHost));
      MV_TRY(hipMemcpy(h_a1.data(), a1.p, (size_t)p.n * 4, hipMemcpyDeviceToHost));
      MV_TRY(hipMemcpy(h_a2.data(), a2.p, (size_t)p.n * 4, hipMemcpyDeviceToHost));
      at_v -= p.n;
      if (fill_v)
        for (long long i = 0; i < p.n; ++i) {
          vt->period[at_v + i] = t + 1;
          vt->i1[at_v + i] = h_states[(size_t)i].x1;
          vt->i2[at_v + i] = h_states[(size_t)i].x2;
          vt->q1[at_v + i] = 0.0;
          vt->q2[at_v + i] = 0.0;
          vt->cash[at_v + i] = h_states[(size_t)i].w;
          vt->value[at_v + i] = h_val[(size_t)i];
          vt->a1[at_v + i] = h_a1[(size_t)i];
          vt->a2[at_v + i] = h_a2[(size_t)i];
        }
      if (t == 0) {
        v1 = h_val[0];
        a1_1 = h_a1[0];
        a2_1 = h_a2[0];
      }
    }
    if (fill_r || t == 0) {
      const size_t n = (size_t)p.nR;
      h_rb.resize(n); h_y1.resize(n); h_y2.resize(n); h_cons.resize(n); h_alpha_out.resize(n);
      MV_TRY(hipMemcpy(h_rb.data(), p.rb.p, n * 8, hipMemcpyDeviceToHost));
      MV_TRY(hipMemcpy(h_y1.data(), y1s.p, n * 4, hipMemcpyDeviceToHost));
      MV_TRY(hipMemcpy(h_y2.data(), y2s.p, n * 4, hipMemcpyDeviceToHost));
      MV_TRY(hipMemcpy(h_cons.data(), cons.p, n * 4, hipMemcpyDeviceToHost));
      MV_TRY(hipMemcpy(h_alpha_out.data(), alpha_out.p, n * 8, hipMemcpyDeviceToHost));
      at_r -= p.nR;
      if (fill_r)
        for (size_t i = 0; i < n; ++i) {
          double R;
          std::memcpy(&R, &h_rb[i], 8);
          rt->period[at_r + (long long)i] = t + 1;
          rt->R[at_r + (long long)i] = R;
          rt->y1[at_r + (long long)i] = h_y1[i];
          rt->y2[at_r + (long long)i] = h_y2[i];
          rt->constrained[at_r + (long long)i] = h_cons[i];
          rt->alpha[at_r + (long long)i] = h_alpha_out[i];
        }
      if (t == 0) {
        const double c = pl.ini.w + 0.0;
        unsigned long long bits;
        std::memcpy(&bits, &c, 8);
        const size_t i = (size_t)(std::lower_bound(h_rb.begin(), h_rb.end(), bits) - h_rb.begin());
        if (i >= n || h_rb[i] != bits) throw std::runtime_error("the row (1, ini_cash) is missing");
        ys1 = h_y1[i]; ys2 = h_y2[i]; cons1 = h_cons[i]; alpha1 = h_alpha_out[i];
      }
    }
    vnext.swap(vcur);
    vcur.release();
  }
  MV_TRY(hipEventRecord(ev1, 0));
  MV_TRY(hipEventSynchronize(ev1));
  check_oob(oob, "a successor");
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ev0, ev1);
  if (out) {
    out->value = v1;
    out->y1 = (double)a1_1; out->y2 = (double)a2_1;
    out->ystar1 = (double)ys1; out->ystar2 = (double)ys2;
    out->constrained = cons1;
    out->forms = (int32_t)(SDPGPU_MULTIV_FORM_SIDE | SDPGPU_MULTIV_FORM_GENERIC);
    out->alpha = alpha1;
    out->cells = cells;
    out->gpu_ms = ms;
  }
  for (int t = 0; t < T; ++t) {
    if (states_per_period) states_per_period[t] = per[(size_t)t].n;
    if (r_per_period) r_per_period[t] = per[(size_t)t].nR;
    if (entries_per_period) entries_per_period[t] = per[(size_t)t].nE + (long long)per[(size_t)t].nR * kAlpha;
  }
  return SDPGPU_OK;
}

}  // namespace

extern "C" {

void sdpgpu_multiv_set_rtable(sdpgpu_multiv_rtable* table) { g_rtable = table; }

int sdpgpu_multiv_solve(const sdpgpu_multiv* k, sdpgpu_multiv_result* out, int64_t* states_per_period, int64_t* r_per_period,
                        int64_t* entries_per_period) {
  ml_error().clear();
  return sdp_multi::ml_guard("multiv", [&] {
    Plan pl;
    if (const int rc = multiv_plan(k, pl)) return rc;
    try {
      return multiv_run(pl, out, states_per_period, r_per_period, entries_per_period);
    } catch (const DeviceError& e) {
      ml_error() = std::string("multiv: ") + e.what();
      return (int)SDPGPU_ERR_DEVICE;
    } catch (const Unsupported& e) {
      ml_error() = std::string("multiv: ") + e.what();
      return (int)SDPGPU_ERR_UNSUPPORTED;
    }
  });
}

}  // extern "C"
