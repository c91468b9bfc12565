// sdp_cash_structure.hpp -- the structure tables of the cash drivers and their checks ("Cash structure tables"):
// G / GA / GB over a window of (cash R, level y) start states of a solved CASH handle (the second and third CashRecursion of
// CashConstraintDraw.main :187-297, CheckFG.main :100-198, SingleCrossTesting.main :85-178, whose drawn period ignores the
// action), and sdp.cash.CashRecursion's post-processing of them (CashRecursion.java:227-404): getH, getMinusGAGB, getMinusFG,
// checkSingleCrossing, checkNonIncreasing, checkNonDecreasing.
//
//   * Per-element arithmetic and predicates are the cs_* functions below, __host__ __device__, fp64, left to right, no FMA
//     (-ffp-contract=off): the plain loops of cash_structure_host_* and the kernels call the same ones, so the device path is
//     bit for bit the host path.  (int) is Java's narrowing (cs_d2i: NaN -> 0, saturating), int sums wrap (cs_iadd).
//   * cash_g_kernel: blockIdx.z = requested kind, blockIdx.y = four levels y (one per wave), blockIdx.x = 64 cash points: the
//     lanes of a wave run along the CASH axis of the window -- successors of neighbouring R are neighbouring cash keys of one
//     V_{t+1} row until a clamp, so the gather coalesces.  One lane = one (R, y) point, the demand loop serial and ascending
//     (CashRecursion.java:110-122), the (demand, probability) tile staged in LDS in pieces of kCashGTile.
//   * cash_h_kernel: a wave per (i, j); the lanes take the candidates k = j + 1 + lane, + 64, ... each with the serial scan's
//     strict compare, then the wave reduces (value, k) lexicographically -- largest value, lowest k.  That equals the serial
//     scan: a NaN candidate never passes the strict compare (so no lane ever holds one unless -K itself is NaN, and then every
//     lane holds (-K, j) and lane 0's is kept), and -0.0 == 0.0 leaves the earlier candidate in place, as the scan does.
//   * checkSingleCrossing without the reference's O(R^2 X) rectangles: cs_last_pass_kernel finds each row's last passing
//     column, cs_col_suffix_kernel each column's next failing row at or below every row, cs_row_scan_kernel carries
//     lastColumnEnd down the rows, cs_cross_kernel turns (row i, column c in [lastColumnEnd_i, last_i]) whose suffix is finite
//     into the key i << 42 | i1 << 21 | c, which sorts like the loops (i, then i1, then j1) visit them.  lastColumnEnd_i
//     depends on the rows above alone, so up to the first violating row it is the reference's.
//   * Every check reduces its first violation as an integer key: minimum inside the wave, one atomicMin per wave that found
//     one.  A minimum does not depend on the order of its operands.
//
// Global memory is written with ordinary vector stores and integer atomics from plain C++ only.
#pragma once
#include "sdp_device.hpp"

namespace sdp {

constexpr int kCashG = 0, kCashGA = 1, kCashGB = 2;
constexpr int kCashGTile = 512;  // (demand, probability) pairs of a staged piece: 8 KiB of LDS
constexpr unsigned long long kCsNoKey = ~0ull;

// ---- shared arithmetic ----
__host__ __device__ __forceinline__ int32_t cs_d2i(double x) {  // Java (int) of a double
  if (x != x) return 0;
  if (x >= 2147483647.0) return 2147483647;
  if (x <= -2147483648.0) return (int32_t)(-2147483647 - 1);
  return (int32_t)x;
}
// A NaN that is STORED (a table entry formed here, a verdict's double) is the one NaN of Double.doubleToLongBits,
// 0x7ff8000000000000: which NaN an operation yields is the processor's choice (inf - inf is negative on the host and positive
// on the device), and Java defines none.  Comparisons never see the difference.
__host__ __device__ __forceinline__ double cs_canon(double x) {
  if (x == x) return x;
  const unsigned long long bits = 0x7ff8000000000000ull;
  double r;
  __builtin_memcpy(&r, &bits, sizeof r);
  return r;
}
__host__ __device__ __forceinline__ int32_t cs_iadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__host__ __device__ __forceinline__ int32_t cs_imax(int32_t a, int32_t b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ int32_t cs_imin(int32_t a, int32_t b) { return a < b ? a : b; }
// `double cash = minCash + i` (CashRecursion.java:232, :275)
__host__ __device__ __forceinline__ double cs_cash(double min_cash, int i) { return min_cash + (double)i; }
// Math.max(0, (int) ((cash - fixCost) / variCost)) (:233, :277)
__host__ __device__ __forceinline__ int32_t cs_qbound(double cash, double K, double v) { return cs_imax(0, cs_d2i((cash - K) / v)); }
// ybound of getH (:277)
__host__ __device__ __forceinline__ int32_t cs_ybound(int n_x, int j, int32_t qbound) { return cs_imin(n_x - 1, cs_iadd(j, qbound)); }
// (int) (cash - fixCost - variCost * (k - j)) (:281)
__host__ __device__ __forceinline__ int32_t cs_cash_index(double cash, double K, double v, int m) { return cs_d2i(cash - K - v * (double)m); }
// resultG[cashIndex][k] - resultG[i][j] - fixCost (:285)
__host__ __device__ __forceinline__ double cs_h_candidate(double g_ck, double g_ij, double K) { return g_ck - g_ij - K; }
// exclusive end of getMinusGAGB's k loop (:236)
__host__ __device__ __forceinline__ int32_t cs_gagb_end(int n_x, int j, int32_t qbound) { return cs_imin(cs_iadd(cs_iadd(j, qbound), 1), n_x); }
// optimalGB - resultGA[i][j] - fixCost (:240)
__host__ __device__ __forceinline__ double cs_gagb_value(double opt_gb, double ga, double K) { return cs_canon(opt_gb - ga - K); }
// resultF[i][j] - resultG[i][j] - variCost * j (:258)
__host__ __device__ __forceinline__ double cs_fg_value(double f, double g, double v, int j) { return cs_canon(f - g - v * (double)j); }
// resultH[..] > -0.1 (:304, :307)
__host__ __device__ __forceinline__ bool cs_cross_pass(double h) { return h > -0.1; }
// arr[i][j + 1] - arr[i][j] < 0.1 (:370)
__host__ __device__ __forceinline__ bool cs_noninc_pass(double next, double cur, double* diff) {
  *diff = cs_canon(next - cur);
  return *diff < 0.1;
}
// arr[i + 1][j] - arr[i][j] > -0.1 (:395)
__host__ __device__ __forceinline__ bool cs_nondec_pass(double next, double cur, double* diff) {
  *diff = cs_canon(next - cur);
  return *diff > -0.1;
}
__host__ __device__ __forceinline__ unsigned long long cs_cross_key(int i, int i1, int j1) {
  return ((unsigned long long)i << 42) | ((unsigned long long)i1 << 21) | (unsigned long long)j1;
}

// what sdpgpu_cash_verdict holds (include/sdpgpu.h), field for field
struct CsVerdict {
  int32_t holds, i, j, i1, j1, reserved;
  double value;
};
__host__ __device__ __forceinline__ CsVerdict cs_holds() { return CsVerdict{1, -1, -1, -1, -1, 0, 0.0}; }

// the first row of getH whose candidates leave the table: for a row the index depends on k - j alone and j = 0 reaches every
// k - j any j reaches, in ascending order -- so the first offender in loop order sits at j = 0.  -> (i, k) or i = -1
inline void cs_h_first_overflow(int n_r, int n_x, double min_cash, double K, double v, int* bad_i, int* bad_k) {
  *bad_i = -1;
  *bad_k = -1;
  for (int i = 0; i < n_r; ++i) {
    const double cash = cs_cash(min_cash, i);
    const int32_t yb = cs_ybound(n_x, 0, cs_qbound(cash, K, v));
    for (int k = 1; k <= yb; ++k)
      if (cs_cash_index(cash, K, v, k) >= n_r) {
        *bad_i = i;
        *bad_k = k;
        return;
      }
  }
}

// ---- host: the reference's loops as they stand ----
inline void cash_structure_host_h(const double* g, int n_r, int n_x, double min_cash, double K, double v, double* values, int32_t* opt_y) {
  for (int i = 0; i < n_r; ++i) {
    const double cash = cs_cash(min_cash, i);
    for (int j = 0; j < n_x; ++j) {
      const int32_t ybound = cs_ybound(n_x, j, cs_qbound(cash, K, v));
      double optimalIncre = -K;
      int32_t optyIndex = j;
      for (int k = j + 1; k <= ybound; ++k) {
        const int32_t cashIndex = cs_cash_index(cash, K, v, k - j);
        if (cashIndex < 0) continue;
        const double c = cs_h_candidate(g[(size_t)cashIndex * n_x + k], g[(size_t)i * n_x + j], K);
        if (c > optimalIncre) {
          optimalIncre = c;
          optyIndex = k;
        }
      }
      values[(size_t)i * n_x + j] = cs_canon(optimalIncre);
      opt_y[(size_t)i * n_x + j] = optyIndex;
    }
  }
}

inline void cash_structure_host_gagb(const double* ga, const double* gb, int n_r, int n_x, double min_cash, double K, double v, double* values) {
  for (int i = 0; i < n_r; ++i) {
    const double cash = cs_cash(min_cash, i);
    const int32_t Qbound = cs_qbound(cash, K, v);
    for (int j = 0; j < n_x; ++j) {
      double optimalGB = gb[(size_t)i * n_x + j];
      const int32_t end = cs_gagb_end(n_x, j, Qbound);
      for (int k = j; k < end; ++k)
        if (gb[(size_t)i * n_x + k] > optimalGB) optimalGB = gb[(size_t)i * n_x + k];
      values[(size_t)i * n_x + j] = cs_gagb_value(optimalGB, ga[(size_t)i * n_x + j], K);
    }
  }
}

inline void cash_structure_host_fg(const double* g, const double* f, int n_r, int n_x, double v, double* values) {
  for (int i = 0; i < n_r; ++i)
    for (int j = 0; j < n_x; ++j) values[(size_t)i * n_x + j] = cs_fg_value(f[(size_t)i * n_x + j], g[(size_t)i * n_x + j], v, j);
}

inline CsVerdict cash_structure_host_cross(const double* H, int n_r, int n_x) {
  int lastColumnEnd = 0;
  for (int i = 0; i < n_r; ++i)
    for (int j = n_x - 1; j >= 0; --j)
      if (cs_cross_pass(H[(size_t)i * n_x + j])) {
        for (int i1 = i; i1 < n_r; ++i1)
          for (int j1 = lastColumnEnd; j1 <= j; ++j1)
            if (!cs_cross_pass(H[(size_t)i1 * n_x + j1])) return CsVerdict{0, i, j, i1, j1, 0, cs_canon(H[(size_t)i1 * n_x + j1])};
        lastColumnEnd = j + 1;
        break;
      }
  return cs_holds();
}

inline CsVerdict cash_structure_host_noninc(const double* a, int n_r, int n_x) {
  for (int i = 0; i < n_r; ++i)
    for (int j = 0; j < n_x - 1; ++j) {
      double diff;
      if (!cs_noninc_pass(a[(size_t)i * n_x + j + 1], a[(size_t)i * n_x + j], &diff)) return CsVerdict{0, i, j, i, j + 1, 0, diff};
    }
  return cs_holds();
}

inline CsVerdict cash_structure_host_nondec(const double* a, int n_r, int n_x) {
  for (int j = 0; j < n_x; ++j)
    for (int i = 0; i < n_r - 1; ++i) {
      double diff;
      if (!cs_nondec_pass(a[(size_t)(i + 1) * n_x + j], a[(size_t)i * n_x + j], &diff)) return CsVerdict{0, i, j, i + 1, j, 0, diff};
    }
  return cs_holds();
}

// ---- device: the G tables ----

struct CashGLaunch {
  double x_lo, cash_lo;   // level of column 0, cash of row 0
  int32_t n_x, n_r;
  int32_t kinds[3];       // blockIdx.z -> kind
  int64_t out_off[3];     // blockIdx.z -> element offset of that kind's table in `out`
  int64_t next_states;    // states of V_{t+1} (the gather's last line of defence: an index is clamped into the table)
};

// One (R, y) point of one kind: CashRecursion.java:110-122 over the statements of cell<FAM_CASH> (sdp_device.hpp) with
// cash_formula 1, base = y, fixed = 0.0, var by kind, and for GB `ncash = ncash - K` before the clamps.
template <int KIND, bool LAST>
__device__ __forceinline__ void cash_g_steps(const DevParams& P, double R, double y, double var, const double2* s_pmf, int n, const double* __restrict__ v_next,
                                             int64_t next_states, double& acc) {
  const double fixed = 0.0;
  for (int jj = 0; jj < n; ++jj) {
    const double2 dp = s_pmf[jj];
    const double d = dp.x;
    double revenue = P.price * jmin(y, d);
    double level = y - d;
    double hold = P.h * jmax(level, 0.0);
    double inc = revenue - fixed - var - hold - P.overhead;
    double sal = LAST ? P.salvage * jmax(level, 0.0) : 0.0;
    inc += sal;
    double end_cash = R + inc;
    if (end_cash < 0) inc += P.pi * end_cash;
    acc += dp.y * inc;
    if (!LAST) {
      double ninv = jmax(0.0, level);
      double ncash = R + inc;
      if (KIND == kCashGB) ncash = ncash - P.K;
      ninv = ninv > P.max_inventory ? P.max_inventory : ninv;
      ninv = ninv < P.min_inventory ? P.min_inventory : ninv;
      int64_t ni = (int64_t)inv_index(P, ninv) * P.next.nc + cash_index(P, ncash);
      ni = ni < 0 ? 0 : (ni >= next_states ? next_states - 1 : ni);  // (never taken for finite inputs)
      acc += (dp.y * P.gamma) * v_next[ni];
    }
  }
}

template <bool LAST>
__global__ __launch_bounds__(256) void cash_g_kernel(DevParams P, CashGLaunch L, const double* __restrict__ pmf_d, const double* __restrict__ pmf_p,
                                                     const double* __restrict__ v_next, double* __restrict__ out) {
  __shared__ double2 s_pmf[kCashGTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = (int)blockIdx.x * 64 + lane, j = (int)blockIdx.y * 4 + wave;
  const bool live = i < L.n_r && j < L.n_x;
  const int kind = L.kinds[blockIdx.z];
  // (an idle lane repeats the window's first point: no read outside the tables, every lane reaches the barriers)
  const double R = L.cash_lo + (double)(live ? i : 0), y = L.x_lo + (double)(live ? j : 0);
  const double vy = P.v * y;
  const double var = kind == kCashG ? 0.0 : vy;
  double acc = 0.0;
  for (int base = 0; base < P.n_demand; base += kCashGTile) {
    const int n = min(kCashGTile, P.n_demand - base);
    __syncthreads();
    for (int q = threadIdx.x; q < n; q += 256) s_pmf[q] = make_double2(pmf_d[base + q], pmf_p[base + q]);
    __syncthreads();
    if (kind == kCashGB)
      cash_g_steps<kCashGB, LAST>(P, R, y, var, s_pmf, n, v_next, L.next_states, acc);
    else
      cash_g_steps<kCashGA, LAST>(P, R, y, var, s_pmf, n, v_next, L.next_states, acc);
  }
  if (live) out[L.out_off[blockIdx.z] + (int64_t)i * L.n_x + j] = kind == kCashG ? acc - vy : acc;
}

// F = V_period on the window: out[i * n_x + j] = V(ix0 + j, ic0 + i)
__global__ __launch_bounds__(256) void cash_f_kernel(const double* __restrict__ v_cur, int64_t nc, int64_t ix0, int64_t ic0, int n_r, int n_x,
                                                     double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n_r * n_x) return;
  const int i = (int)(e / n_x), j = (int)(e % n_x);
  out[e] = v_cur[(ix0 + j) * nc + (ic0 + i)];
}

// ---- device: the derived tables ----

// grid = ceil(n_r n_x / 4) workgroups of four waves, a wave per (i, j).  The caller has made sure no cashIndex reaches n_r.
__global__ __launch_bounds__(256) void cash_h_kernel(const double* __restrict__ g, int n_r, int n_x, double min_cash, double K, double v,
                                                     double* __restrict__ values, int32_t* __restrict__ opt_y) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= (int64_t)n_r * n_x) return;  // (wave-uniform)
  const int i = (int)(e / n_x), j = (int)(e % n_x);
  const double cash = cs_cash(min_cash, i);
  const int32_t ybound = cs_ybound(n_x, j, cs_qbound(cash, K, v));
  const double g_ij = g[e];
  double best = -K;
  int32_t best_k = j;
  for (int k = j + 1 + lane; k <= ybound; k += 64) {
    const int32_t cashIndex = cs_cash_index(cash, K, v, k - j);
    if (cashIndex < 0 || cashIndex >= n_r) continue;  // (>= n_r: refused on the host before the launch)
    const double c = cs_h_candidate(g[(int64_t)cashIndex * n_x + k], g_ij, K);
    if (c > best) {
      best = c;
      best_k = k;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ob = __shfl_down(best, off);
    const int32_t ok = __shfl_down(best_k, off);
    if (ob > best || (ob == best && ok < best_k)) {
      best = ob;
      best_k = ok;
    }
  }
  if (lane == 0) {
    values[e] = cs_canon(best);
    opt_y[e] = best_k;
  }
}

// one thread per (i, j), the lanes along j: the running maximum of the reference, k ascending
__global__ __launch_bounds__(256) void cash_gagb_kernel(const double* __restrict__ ga, const double* __restrict__ gb, int n_r, int n_x, double min_cash,
                                                        double K, double v, double* __restrict__ values) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n_r * n_x) return;
  const int i = (int)(e / n_x), j = (int)(e % n_x);
  const double cash = cs_cash(min_cash, i);
  const int32_t end = cs_gagb_end(n_x, j, cs_qbound(cash, K, v));
  const double* __restrict__ row = gb + (int64_t)i * n_x;
  double optimalGB = row[j];
  for (int k = j; k < end; ++k) {
    const double c = row[k];
    if (c > optimalGB) optimalGB = c;
  }
  values[e] = cs_gagb_value(optimalGB, ga[e], K);
}

__global__ __launch_bounds__(256) void cash_fg_kernel(const double* __restrict__ g, const double* __restrict__ f, int n_r, int n_x, double v,
                                                      double* __restrict__ values) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n_r * n_x) return;
  values[e] = cs_fg_value(f[e], g[e], v, (int)(e % n_x));
}

// ---- device: the checks ----

__device__ __forceinline__ unsigned long long cs_wave_min(unsigned long long key) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_down(key, off);
    key = o < key ? o : key;
  }
  return key;  // (lane 0 holds the wave's minimum)
}

__global__ __launch_bounds__(64) void cs_key_fill_kernel(unsigned long long* __restrict__ keys, int n) {
  if ((int)threadIdx.x < n) keys[threadIdx.x] = kCsNoKey;
}

// checkNonIncreasing (DEC = false: key i * n_x + j) / checkNonDecreasing (DEC = true: key j * n_r + i), a thread per element
template <bool DEC>
__global__ __launch_bounds__(256) void cs_monotone_kernel(const double* __restrict__ a, int n_r, int n_x, unsigned long long* __restrict__ key) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long mine = kCsNoKey;
  if (e < (int64_t)n_r * n_x) {
    const int i = (int)(e / n_x), j = (int)(e % n_x);
    double diff;
    if (DEC) {
      if (i + 1 < n_r && !cs_nondec_pass(a[e + n_x], a[e], &diff)) mine = (unsigned long long)j * (unsigned)n_r + (unsigned)i;
    } else {
      if (j + 1 < n_x && !cs_noninc_pass(a[e + 1], a[e], &diff)) mine = (unsigned long long)i * (unsigned)n_x + (unsigned)j;
    }
  }
  mine = cs_wave_min(mine);
  if ((threadIdx.x & 63) == 0 && mine != kCsNoKey) atomicMin(key, mine);
}

// a wave per row: the largest passing column, -1 when none (:303-304)
__global__ __launch_bounds__(256) void cs_last_pass_kernel(const double* __restrict__ H, int n_r, int n_x, int32_t* __restrict__ last) {
  const int lane = threadIdx.x & 63;
  const int i = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_r) return;  // (wave-uniform)
  int best = -1;
  for (int j = lane; j < n_x; j += 64)
    if (cs_cross_pass(H[(int64_t)i * n_x + j])) best = j;  // (ascending: the last one stays)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_down(best, off);
    best = o > best ? o : best;
  }
  if (lane == 0) last[i] = best;
}

// a thread per column, rows from the bottom up: next_fail[i][c] = the smallest i1 >= i whose entry in column c fails, n_r: none
__global__ __launch_bounds__(256) void cs_col_suffix_kernel(const double* __restrict__ H, int n_r, int n_x, int32_t* __restrict__ next_fail) {
  const int c = (int)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_x) return;
  int32_t nf = n_r;
  for (int i = n_r - 1; i >= 0; --i) {
    if (!cs_cross_pass(H[(int64_t)i * n_x + c])) nf = i;
    next_fail[(int64_t)i * n_x + c] = nf;
  }
}

// one thread: lastColumnEnd at the entry of every row (:301, :312) -- a row without a passing entry leaves it unchanged
__global__ __launch_bounds__(64) void cs_row_scan_kernel(const int32_t* __restrict__ last, int n_r, int32_t* __restrict__ col_end) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int32_t lastColumnEnd = 0;
  for (int i = 0; i < n_r; ++i) {
    col_end[i] = lastColumnEnd;
    if (last[i] >= 0) lastColumnEnd = last[i] + 1;
  }
}

__global__ __launch_bounds__(256) void cs_cross_kernel(const int32_t* __restrict__ last, const int32_t* __restrict__ col_end, const int32_t* __restrict__ next_fail,
                                                       int n_r, int n_x, unsigned long long* __restrict__ key) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long mine = kCsNoKey;
  if (e < (int64_t)n_r * n_x) {
    const int i = (int)(e / n_x), c = (int)(e % n_x);
    if (last[i] >= 0 && c >= col_end[i] && c <= last[i]) {
      const int32_t i1 = next_fail[e];
      if (i1 < n_r) mine = cs_cross_key(i, i1, c);
    }
  }
  mine = cs_wave_min(mine);
  if ((threadIdx.x & 63) == 0 && mine != kCsNoKey) atomicMin(key, mine);
}

// What a call's checks read and write: slot 0 the single crossing on H, slots 1-3 checkNonIncreasing on table 0 / 1 / 2, slots
// 4-6 checkNonDecreasing; a table that is nullptr was not requested.
struct CsFinish {
  const double* tab[3];
  const int32_t* last;
  int32_t n_r, n_x;
  uint32_t checks;  // bit s: slot s was run
};

// thread s: the verdict of slot s from its key, the offending double recomputed with the shared predicate
__global__ __launch_bounds__(64) void cs_finish_kernel(CsFinish F, const unsigned long long* __restrict__ keys, CsVerdict* __restrict__ out) {
  const int s = threadIdx.x;
  if (s >= 7) return;
  CsVerdict r = cs_holds();
  const unsigned long long key = keys[s];
  if (((F.checks >> s) & 1u) && key != kCsNoKey) {
    r.holds = 0;
    if (s == 0) {
      r.i = (int32_t)(key >> 42);
      r.i1 = (int32_t)((key >> 21) & 0x1fffff);
      r.j1 = (int32_t)(key & 0x1fffff);
      r.j = F.last[r.i];
      r.value = cs_canon(F.tab[0][(int64_t)r.i1 * F.n_x + r.j1]);
    } else if (s <= 3) {
      const double* a = F.tab[s - 1];
      r.i = (int32_t)(key / (unsigned)F.n_x);
      r.j = (int32_t)(key % (unsigned)F.n_x);
      r.i1 = r.i;
      r.j1 = r.j + 1;
      (void)cs_noninc_pass(a[(int64_t)r.i * F.n_x + r.j + 1], a[(int64_t)r.i * F.n_x + r.j], &r.value);
    } else {
      const double* a = F.tab[s - 4];
      r.j = (int32_t)(key / (unsigned)F.n_r);
      r.i = (int32_t)(key % (unsigned)F.n_r);
      r.i1 = r.i + 1;
      r.j1 = r.j;
      (void)cs_nondec_pass(a[(int64_t)(r.i + 1) * F.n_x + r.j], a[(int64_t)r.i * F.n_x + r.j], &r.value);
    }
  }
  out[s] = r;
}

}  // namespace sdp
