// sdp_fitss.hpp -- the (s, S) level rules of the reference's capacitated.fitss drivers (OneLevelFitsSTest, TwoLevelFitsSTest,
// ThreeLevelFitsSTest): the FIT of a one-, two- or three-level rule to the optimal table (sdp.inventory.FitsS,
// FitsS.java:39-291) and the ROLLOUT of such a rule along demand paths (capacitated.fitss.SimulateFitsS,
// SimulateFitsS.java:32-130), for all instances of a batch (sdpgpu_fit_ss, sdpgpu_batch_fit_ss, sdpgpu_batch_simulate_ss*;
// sdpgpu_batch.hip).
//
//   * the fit is ONE set of functions, compiled for the host (sdpgpu_fit_ss on rows [period, x, Q]) and for the device
//     (batch_fit_ss_kernel on the reachable slice of a policy row): `Rows` gives x(j) and q(j) of row j of one period, the
//     statements are those of FitsS word for word -- levelIndex (:39-59), the branches of getSinglesS / getTwosS /
//     getThreesS (:100-291) with the "last row still at the limit" corrections and the copies of the upper bands.  The
//     device fit of a (instance, period) pair is one thread walking its slice: the walk carries `mark` from row to row and
//     stops at the first zero, there are n x T pairs of a few hundred rows, and the host twin of the walk is then the same
//     code (bit-for-bit equality is by construction, not by care);
//   * minSquare (:69-98) is the closed form of the one-variable problem the reference hands to CPLEX: the mean of
//     the terms x_i + Q_i, clamped to [lb, 10000].  With step 1 every term is an integer far below 2^53, the fp64 sum exact;
//   * the rollout is batch_sim_kernel (sdp_batch_sim.hpp) under LevelRule below: the state stays the DOUBLE it is (a fitted S
//     may be fractional), the rule needs no policy row and gathers nothing per step; everything else of a path is the table
//     rollout's, so the same (seed, position, n) rolls the rule along the SAME demand paths as the table policy.
//
// Global memory is written with ordinary vector stores from plain C++ only.
#pragma once
#include "sdp_batch_sim.hpp"
#include "sdp_fit_pair.hpp"

namespace sdp {

// FitsS.levelIndex (FitsS.java:39-59) on the n rows of one period: sink.add(j) for every index the reference appends.
template <class Rows, class Sink>
__host__ __device__ __forceinline__ void fit_level_walk(const Rows& r, int n, double maxq, Sink& sink) {
  bool mark = false;
  for (int j = 0; j < n; ++j) {
    const double q = r.q(j);
    if (q < maxq && !mark) {
      mark = true;
    } else if (q == maxq && mark && j != n - 1) {
      mark = false;
      sink.add(j);
    }
    if (q == 0) {
      sink.add(j);
      break;
    }
    if (j == n - 1) sink.add(j);
  }
}

// FitsS.minSquare (FitsS.java:69-98) in closed form: argmin over [lb, 10000] of the sum of (x - realS_i)^2.
template <class Rows>
__host__ __device__ __forceinline__ double fit_min_square(const Rows& r, int n, double maxq, double lb, int up) {
  int low = 0;
  for (int i = 0; i < n; ++i)
    if (r.q(i) != maxq) {
      low = i;
      break;
    }
  double sum = r.x(low) + r.q(low);
  int count = 1;
  for (int i = low + 1; i <= up; ++i)
    if (r.q(i) != maxq) {
      sum += r.x(i) + r.q(i);
      ++count;
    }
  double m = sum / (double)count;
  m = m < lb ? lb : m;
  return m > 10000.0 ? 10000.0 : m;
}

// what the three get*sS methods read of a levelIndex list: its length, its first three and its last three entries
struct FitLevels {
  int n = 0;
  int f0 = 0, f1 = 0, f2 = 0;  // the first three entries
  int l0 = 0, l1 = 0, l2 = 0;  // l0: the final entry, l1 the one before, l2 the one before that
  __host__ __device__ __forceinline__ void add(int j) {  // (scalars, not arrays: nothing here may end up in scratch memory)
    f0 = n == 0 ? j : f0;
    f1 = n == 1 ? j : f1;
    f2 = n == 2 ? j : f2;
    l2 = l1;
    l1 = l0;
    l0 = j;
    ++n;
  }
};

// the S of the band that ends below row k: x_{k-1} + Q_{k-1}
template <class Rows>
__host__ __device__ __forceinline__ double fit_up_to(const Rows& r, int k) { return r.x(k - 1) + r.q(k - 1); }

// One period t >= 2 of getSinglesS (levels 1, FitsS.java:105-127), getTwosS (2, :162-207) or getThreesS (3, :222-288):
// o[0 .. 2 * levels) = s1, S1 (, s2, S2 (, s3, S3)).  n >= 1 rows.
template <int LEVELS, class Rows>
__host__ __device__ __forceinline__ void fit_period(const Rows& r, int n, double maxq, double* o) {
  FitLevels L;
  fit_level_walk(r, n, maxq, L);
  constexpr int bands = LEVELS;
  if (L.n == 1 && L.f0 != 0) {
    const int k = L.f0;
    o[0] = r.x(k);
    o[1] = fit_up_to(r, k);
    if (k == n - 1 && r.q(k) == maxq) {  // the last row still orders the limit
      o[0] = r.x(k) + 1;
      o[1] = r.x(k) + r.q(k);
    }
    for (int b = 1; b < bands; ++b) {
      o[2 * b] = o[0];
      o[2 * b + 1] = o[1];
    }
  } else if (L.n == 1 && L.f0 == 0) {  // s, S are both the first row's inventory
    for (int b = 0; b < 2 * bands; ++b) o[b] = r.x(0);
  } else if (L.n == 0) {  // "order at max" (:120-123; levelIndex never returns an empty list: kept for fidelity)
    for (int b = 0; b < bands; ++b) {
      o[2 * b] = r.x(n - 1);
      o[2 * b + 1] = maxq * 10;
    }
  } else if constexpr (LEVELS == 1) {  // fit the remnant S values to one (:124-126)
    const int k = L.l0;
    o[0] = r.x(k);
    o[1] = fit_min_square(r, n, maxq, o[0], k);
  } else if (L.n == 2) {
    const int k0 = L.f0, k1 = L.f1;
    o[0] = r.x(k0);
    o[1] = fit_up_to(r, k0);
    o[2] = r.x(k1);
    o[3] = fit_up_to(r, k1);
    if (k1 == n - 1 && r.q(k1) == maxq) {
      o[2] = r.x(k1) + 1;
      o[3] = r.x(k1) + r.q(k1);
    }
    if constexpr (LEVELS == 3) {
      o[4] = o[2];
      o[5] = o[3];
    }
  } else if constexpr (LEVELS == 2) {  // three or more entries (:200-207)
    const int k2 = L.l0, k1 = L.l1;
    o[2] = r.x(k2);
    o[3] = fit_up_to(r, k2);
    o[0] = r.x(k1);
    o[1] = fit_min_square(r, n, maxq, o[0], k1);
  } else if (L.n == 3) {
    const int k0 = L.f0, k1 = L.f1, k2 = L.f2;
    o[0] = r.x(k0);
    o[1] = fit_up_to(r, k0);
    o[2] = r.x(k1);
    o[3] = fit_up_to(r, k1);
    o[4] = r.x(k2);
    o[5] = fit_up_to(r, k2);
    if (k2 == n - 1 && r.q(k2) == maxq) {
      o[4] = r.x(k2) + 1;
      o[5] = r.x(k2) + r.q(k2);
    }
  } else {  // four or more entries (:278-288)
    const int k3 = L.l0, k2 = L.l1, k1 = L.l2;
    o[4] = r.x(k3);
    o[5] = fit_up_to(r, k3);
    o[2] = r.x(k2);
    o[3] = fit_up_to(r, k2);
    o[0] = r.x(k1);
    o[1] = fit_min_square(r, n, maxq, o[0], k1);
  }
}

// Period 1 (:101-103, :157-160, :215-220): s = x_0 + 1 (the literal 1), S = x_0 + Q_0, the pair repeated for every level.
template <int LEVELS>
__host__ __device__ __forceinline__ void fit_first_period(double x0, double q0, double* o) {
#pragma unroll
  for (int b = 0; b < LEVELS; ++b) {
    o[2 * b] = x0 + 1;
    o[2 * b + 1] = x0 + q0;
  }
}

// ---- device: the fit of every (instance, period) of a solved batch ----

struct FitSliceRows {
  const int32_t* __restrict__ pol;  // the policy row
  double x_min, step;
  int lo;
  __device__ double x(int j) const { return x_min + (double)(lo + j) * step; }  // (as the read-back rows are formed)
  __device__ double q(int j) const { return (double)pol[lo + j] * step; }
};

// One thread per (instance, period): out[(i * T + t) * 2 * levels ...].
template <int LEVELS>
__global__ __launch_bounds__(256) void batch_fit_ss_kernel(const FitPair* __restrict__ pairs, int n_pairs, int T, double step,
                                                           const int32_t* __restrict__ policy, double* __restrict__ out) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n_pairs) return;
  const FitPair P = pairs[g];
  const FitSliceRows rows{policy + P.pol_off, P.x_min, step, P.lo};
  double o[2 * LEVELS];
  if (g % T == 0)
    fit_first_period<LEVELS>(rows.x(0), rows.q(0), o);
  else
    fit_period<LEVELS>(rows, P.n, P.maxq, o);
#pragma unroll
  for (int k = 0; k < 2 * LEVELS; ++k) out[(int64_t)g * (2 * LEVELS) + k] = o[k];
}

// ---- device: the rollout of a level rule ----

__device__ __forceinline__ double ss_capped(double maxq, double want) { return maxq <= want ? maxq : want; }  // Math.min

// SimulateFitsS.simulateSinglesS / TwosS / ThreesS (SimulateFitsS.java:32-130): ss[(i * T + t) * 2 * LEVELS ...].  The period
// starts from the carried level itself, NOT snapped to the grid.
template <int LEVELS>
struct LevelRule {
  const double* __restrict__ ss;
  __device__ __forceinline__ const double* rows(const SimLaunch& L, const SimInst&, int i) const { return ss + (int64_t)i * L.T * (2 * LEVELS); }
  __device__ __forceinline__ double act(const SimLaunch&, const SimInst& I, const double* __restrict__ rule, int t, double* x_kept) const {
    const double* __restrict__ o = rule + (int64_t)t * (2 * LEVELS);
    const double x = *x_kept;
    if (t == 0) return o[1] - x;  // (x is the start state; not capped: SimulateFitsS.java:43)
    if constexpr (LEVELS == 1) {
      return x >= o[0] ? 0.0 : ss_capped(I.maxq, o[1] - x);
    } else {
      if (x < o[0]) return ss_capped(I.maxq, o[1] - x);
      if (o[0] <= x && x < o[2]) return ss_capped(I.maxq, o[3] - x);
      if constexpr (LEVELS == 3)
        if (o[2] <= x && x < o[4]) return ss_capped(I.maxq, o[5] - x);
      return 0.0;
    }
  }
};

}  // namespace sdp
