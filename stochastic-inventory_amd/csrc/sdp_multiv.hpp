// sdp_multiv.hpp -- device side of sdpgpu_multiv_solve: sdp.cash.multiItem.CashRecursionV (CashRecursionV.java:83-194) over the
// lambdas of cash.multiItem.MultiItemYR.main (MultiItemYR.java:104-158; rounding and order bounds of MultiItemYRTesting.main,
// MultiItemYRTesting.java:100-101, 163-165).  The statements of the transition exist once (v_successor / the side tables built
// from the same expressions); the kernels around them form, per period,
//   forward : the distinct R of the V states, the Pi entries E_t (affordable boxes of the states + the y* box of every R, as
//             flags over the dense (R, y1, y2) table; the alpha line of every R beside it), and the marks of their successors
//             on the integer lattice (x1, x2, w) -> S_{t+1};
//   backward: Pi over E_t (pi_kernel: a lane per entry, the demand pairs serially in list order, V_{t+1} read DENSE from the
//             lattice), then the reference's sequential scans -- V per state (`> val + 0.01`), y* and alpha per R (`> val + 0.1`).
// Compile with -ffp-contract=off: every sum below is the Java expression, operation for operation.  Internal, header only.
#pragma once
#include "../../include/sdpgpu.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

namespace sdp_multiv {

constexpr int kAlpha = 100;  // `for (alpha = 0; alpha <= 1; alpha = alpha + 0.01)` runs 100 times (CashRecursionV.java:180)

struct VParams {
  double price[2], vari[2], sal[2];
  double one_plus_dep;  // 1 + depositeRate (MultiItemYR.java:146)
  double min_inventory, max_inventory, min_cash, max_cash;
  int32_t q1, q2;    // the order bounds
  int32_t rounding;  // SDPGPU_MULTIV_TRUNC10 / _ROUND
  int32_t nd;        // demand pairs of the period being processed
  int32_t Y1, Y2;    // the dense Pi table of one R: levels [0, Y1) x [0, Y2), index (r * Y1 + y1) * Y2 + y2
  int32_t n1, n2, nw;  // the lattice of V_{t+1}: index (x1 * n2 + x2) * nw + (w - w0)
  int32_t w0;
};

struct State {
  double x1, x2, w;
};

// java.lang.Math.round(double) as an integer-valued double: nearest, ties toward +infinity (as sdp_device.hpp's jround_d)
__device__ __forceinline__ double v_jround(double x) {
  const double f = floor(x);
  const double diff = x - f;  // exact
  return diff >= 0.5 ? f + 1.0 : f;
}

// MultiItemYR.java:149-151 `Math.round(v * 10) / 10` (long / int: truncates toward zero) or MultiItemYRTesting.java:163-165
__device__ __forceinline__ double v_round(int mode, double v) {
  if (mode == SDPGPU_MULTIV_ROUND) return v_jround(v);
  return (double)((long long)v_jround(v * 10) / 10);
}

// the per-product halves of the transition (MultiItemYR.java:140-145, 149-150, 154-155)
__device__ __forceinline__ double v_end1(const VParams& P, double y1, double d1) {
  double e = y1 - d1;
  e = fmax(0.0, e);
  e = v_round(P.rounding, e);
  return e > P.max_inventory ? P.max_inventory : e;  // clamped above only
}
__device__ __forceinline__ double v_end2(const VParams& P, double y2, double d2) {
  double e = y2 - d2;
  e = fmax(0.0, e);
  e = v_round(P.rounding, e);
  return e < P.min_inventory ? P.min_inventory : e;  // clamped below only
}
__device__ __forceinline__ double v_revenue(double price, double y, double d) { return price * fmin(y, d); }

// (1 + depositeRate) * (R - v1 y1 - v2 y2), :146-147
__device__ __forceinline__ double v_base(const VParams& P, double y1, double y2, double R) {
  return P.one_plus_dep * (R - P.vari[0] * y1 - P.vari[1] * y2);
}

// nextW of :146-153 from the two revenues and the base
__device__ __forceinline__ double v_next_w(const VParams& P, double rev1, double rev2, double base) {
  double w = rev1 + rev2 + base;
  w = v_round(P.rounding, w);
  w = w > P.max_cash ? P.max_cash : w;
  w = w < P.min_cash ? P.min_cash : w;
  return w;
}

// lattice index of an integer state, -1 outside the box (never written or read then; the host reports it)
__device__ __forceinline__ long long v_lattice(const VParams& P, double e1, double e2, double w) {
  const long long a = (long long)e1, b = (long long)e2, c = (long long)w - P.w0;
  if (a < 0 || a >= P.n1 || b < 0 || b >= P.n2 || c < 0 || c >= P.nw) return -1;
  return (a * P.n2 + b) * (long long)P.nw + c;
}

__device__ __forceinline__ unsigned long long v_bits(double v) {
  v += 0.0;  // -0.0 -> +0.0 (the reference's comparators use == and >)
  return (unsigned long long)__double_as_longlong(v);
}

// R of a V state, CashRecursionV.java:108
__device__ __forceinline__ double v_state_R(const VParams& P, const State& s) {
  return s.w + P.vari[0] * s.x1 + P.vari[1] * s.x2;
}

// index of `key` in the sorted distinct R of the period (it is there: the list was formed from the same expression)
__device__ __forceinline__ int v_find(const unsigned long long* __restrict__ rb, int n, unsigned long long key) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rb[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void state_r_kernel(VParams P, const State* __restrict__ states, long long n,
                                                      unsigned long long* __restrict__ rbits) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s < n) rbits[s] = v_bits(v_state_R(P, states[s]));
}

__global__ __launch_bounds__(256) void state_ridx_kernel(VParams P, const State* __restrict__ states, long long n,
                                                         const unsigned long long* __restrict__ rb, int nR,
                                                         int* __restrict__ ridx) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s < n) ridx[s] = v_find(rb, nR, v_bits(v_state_R(P, states[s])));
}

// buildActionListV (MultiItemYR.java:116-129): a thread per (state, box cell); the affordable cells are flagged
__global__ __launch_bounds__(256) void entry_mark_states_kernel(VParams P, const State* __restrict__ states, long long n,
                                                                const int* __restrict__ ridx,
                                                                unsigned char* __restrict__ flags, int* __restrict__ oob) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
  const int box = P.q1 * P.q2;
  if (tid >= n * box) return;
  const long long s = tid / box;
  const int c = (int)(tid - s * box);
  const State st = states[s];
  const int i = (int)st.x1 + c / P.q2, j = (int)st.x2 + c % P.q2;
  const double R = v_state_R(P, st);
  if (!(P.vari[0] * (double)i + P.vari[1] * (double)j < R + 0.1)) return;
  if (i < 0 || i >= P.Y1 || j < 0 || j >= P.Y2) {
    *oob = 1;
    return;
  }
  flags[((long long)ridx[s] * P.Y1 + i) * P.Y2 + j] = 1;
}

// buildActionListPai (:104-113): the unshifted box of every R, every cell
__global__ __launch_bounds__(256) void entry_mark_ystar_kernel(VParams P, int nR, unsigned char* __restrict__ flags) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
  const int box = P.q1 * P.q2;
  if (tid >= (long long)nR * box) return;
  const long long r = tid / box;
  const int c = (int)(tid - r * box);
  flags[(r * P.Y1 + c / P.q2) * P.Y2 + c % P.q2] = 1;
}

// per-product side tables of the integer levels: row j (demand pair), column y -- the rounded, clamped end inventory and the
// revenue of (y, d_j), the same statements v_successor's generic form evaluates per cell
__global__ __launch_bounds__(256) void side_kernel(VParams P, const double2* __restrict__ dem, int* __restrict__ se1,
                                                   double* __restrict__ sr1, int* __restrict__ se2, double* __restrict__ sr2) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
  const int Ym = P.Y1 > P.Y2 ? P.Y1 : P.Y2;
  if (tid >= (long long)P.nd * Ym) return;
  const int j = (int)(tid / Ym), y = (int)(tid - (long long)j * Ym);
  const double2 d = dem[j];
  if (y < P.Y1) {
    se1[(long long)j * P.Y1 + y] = (int)v_end1(P, (double)y, d.x);
    sr1[(long long)j * P.Y1 + y] = v_revenue(P.price[0], (double)y, d.x);
  }
  if (y < P.Y2) {
    se2[(long long)j * P.Y2 + y] = (int)v_end2(P, (double)y, d.y);
    sr2[(long long)j * P.Y2 + y] = v_revenue(P.price[1], (double)y, d.y);
  }
}

// ---- Pi --------------------------------------------------------------------------------------------------------------------
// One lane per entry (y1, y2, R), the demand pairs serially in list order (CashRecursionV.java:88-94).
//   SIDE : the entry is a flagged cell of the dense table (integer levels; e_i and revenue_i from the side tables);
//          else it is point k of the alpha line of R number r (fractional levels, the transition evaluated per cell).
//   MODE 0: forward -- mark the successors on the lattice of period t + 1.
//   MODE 1: Pi from V_{t+1} on the lattice.   MODE 2: period T, V_{T+1} = w + sal1 x1 + sal2 x2 (MultiItemYR.java:132-135).
template <bool SIDE, int MODE>
__global__ __launch_bounds__(256) void pi_kernel(VParams P, const long long* __restrict__ entries, long long n_entries,
                                                 const unsigned long long* __restrict__ rb, const double* __restrict__ alphas,
                                                 const double2* __restrict__ dem, const double* __restrict__ prob,
                                                 const int* __restrict__ se1, const double* __restrict__ sr1,
                                                 const int* __restrict__ se2, const double* __restrict__ sr2,
                                                 const double* __restrict__ vnext, unsigned char* __restrict__ marks,
                                                 double* __restrict__ pi_out, int* __restrict__ oob) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_entries) return;
  long long out_at;
  int iy1 = 0, iy2 = 0;
  double y1, y2, R;
  if constexpr (SIDE) {
    out_at = entries[e];
    iy2 = (int)(out_at % P.Y2);
    const long long q = out_at / P.Y2;
    iy1 = (int)(q % P.Y1);
    R = __longlong_as_double((long long)rb[q / P.Y1]);
    y1 = (double)iy1;
    y2 = (double)iy2;
  } else {
    out_at = e;
    const long long r = e / kAlpha;
    const double alpha = alphas[e - r * kAlpha];
    R = __longlong_as_double((long long)rb[r]);
    y1 = alpha * R / P.vari[0];        // CashRecursionV.java:183
    y2 = (1 - alpha) * R / P.vari[1];  // :184
  }
  const double base = v_base(P, y1, y2, R);
  double ev = 0;
#pragma unroll 4
  for (int j = 0; j < P.nd; ++j) {
    double e1, e2, rev1, rev2;
    if constexpr (SIDE) {
      e1 = (double)se1[(long long)j * P.Y1 + iy1];
      e2 = (double)se2[(long long)j * P.Y2 + iy2];
      rev1 = sr1[(long long)j * P.Y1 + iy1];
      rev2 = sr2[(long long)j * P.Y2 + iy2];
    } else {
      const double2 d = dem[j];
      e1 = v_end1(P, y1, d.x);
      e2 = v_end2(P, y2, d.y);
      rev1 = v_revenue(P.price[0], y1, d.x);
      rev2 = v_revenue(P.price[1], y2, d.y);
    }
    const double w = v_next_w(P, rev1, rev2, base);
    if constexpr (MODE == 2) {
      ev += prob[j] * (w + P.sal[0] * e1 + P.sal[1] * e2);
    } else {
      const long long at = v_lattice(P, e1, e2, w);
      if (at < 0) {
        *oob = 1;
        continue;
      }
      if constexpr (MODE == 0)
        marks[at] = 1;
      else
        ev += prob[j] * vnext[at];
    }
  }
  if constexpr (MODE != 0) pi_out[out_at] = ev;
}

// ---- the lattice's marks as states ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lattice_states_kernel(VParams P, const long long* __restrict__ idx, long long n,
                                                             State* __restrict__ states) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const long long at = idx[s];
  const long long c = at % P.nw, q = at / P.nw;
  State st;
  st.x1 = (double)(q / P.n2);
  st.x2 = (double)(q % P.n2);
  st.w = (double)(c + P.w0);
  states[s] = st;
}

// ---- the scans --------------------------------------------------------------------------------------------------------------
// getExpectedValueV (CashRecursionV.java:100-131) of one state per lane: the affordable levels of its box, row-major,
// `> val + 0.01`.  ON_LATTICE: the state is a lattice point and its value goes to the dense V of its period.
template <bool ON_LATTICE>
__global__ __launch_bounds__(256) void v_scan_kernel(VParams P, const State* __restrict__ states, long long n,
                                                     const int* __restrict__ ridx, const double* __restrict__ pi,
                                                     double* __restrict__ vdense, double* __restrict__ value,
                                                     int* __restrict__ a1, int* __restrict__ a2) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const State st = states[s];
  const double R = v_state_R(P, st);
  const double* row = pi + (long long)ridx[s] * P.Y1 * P.Y2;
  double val = -DBL_MAX;
  int b1 = (int)st.x1, b2 = (int)st.x2;
  const int i0 = (int)st.x1, j0 = (int)st.x2;
  for (int i = i0; i < i0 + P.q1; ++i)
    for (int j = j0; j < j0 + P.q2; ++j) {
      if (!(P.vari[0] * (double)i + P.vari[1] * (double)j < R + 0.1)) continue;
      if (i >= P.Y1 || j >= P.Y2) continue;  // (never flagged either: entry_mark_states_kernel reported it)
      const double v = row[(long long)i * P.Y2 + j];
      if (v > val + 0.01) {
        val = v;
        b1 = i;
        b2 = j;
      }
    }
  value[s] = val;
  a1[s] = b1;
  a2[s] = b2;
  if constexpr (ON_LATTICE) {
    const long long at = v_lattice(P, st.x1, st.x2, st.w);
    if (at >= 0) vdense[at] = val;
  }
}

// getYStar (:149-173) and, where y* is not affordable, getAlpha (:176-194), one R per lane
__global__ __launch_bounds__(256) void ystar_kernel(VParams P, const unsigned long long* __restrict__ rb, int nR,
                                                    const double* __restrict__ pi, const double* __restrict__ pi_alpha,
                                                    const double* __restrict__ alphas, int* __restrict__ y1s,
                                                    int* __restrict__ y2s, int* __restrict__ constrained,
                                                    double* __restrict__ alpha_out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= nR) return;
  const double R = __longlong_as_double((long long)rb[r]);
  const double* row = pi + (long long)r * P.Y1 * P.Y2;
  double val = -DBL_MAX;
  int b1 = 0, b2 = 0;
  for (int i = 0; i < P.q1; ++i)
    for (int j = 0; j < P.q2; ++j) {
      const double v = row[(long long)i * P.Y2 + j];
      if (v > val + 0.1) {
        val = v;
        b1 = i;
        b2 = j;
      }
    }
  y1s[r] = b1;
  y2s[r] = b2;
  const bool cons = P.vari[0] * (double)b1 + P.vari[1] * (double)b2 >= R + 0.1;
  double best_alpha = 0;
  if (cons) {
    double best = -DBL_MAX;
    for (int k = 0; k < kAlpha; ++k) {
      const double v = pi_alpha[(long long)r * kAlpha + k];
      if (v > best + 0.1) {
        best = v;
        best_alpha = alphas[k];
      }
    }
  }
  constrained[r] = cons ? 1 : 0;
  alpha_out[r] = best_alpha;
}

}  // namespace sdp_multiv
