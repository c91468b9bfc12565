// sdp_staff_structure.hpp -- the G(y) rows of the STAFF family: what WorkforcePlanning.main draws and hands to
// CheckKConvexity.check(yG, fixCost) (WorkforcePlanning.java:165-211), for any period of a solved handle or batch instance.
//
//   G_t(y), t in 1 .. T, y in 0 .. n_rows_t - 1, row = pmfs[t - 1][y] with len(y) entries:
//       g = 0.0
//       for j = 0 .. len(y) - 1, ascending:
//           n   = y - j
//           pen = n > minStaff_t ? 0.0 : unitPenalty * (double)(minStaff_t - n)
//           g  += p_row[j] * (((0.0 + unitVariCost * (double)y) + salary * (double)n) + pen)
//           if t < T:  g += p_row[j] * V_{t+1}(nn)
//   the lambda pair of WorkforcePlanning.java:171-195 inside the loop of StaffRecursion.java:153-163: fp64, no FMA
//   (-ffp-contract=off), the two additions of a step in that order.  nn = n, pushed through the family's clamp when
//   clamp_inventory = 1 (upper bound first, then lower: StaffFunctor.stateTransition), untouched otherwise.  Period T reads no V.
//   hireUpStaffNum is not an input: the reference never reads it.
//
//   * No second recursion is built: an entry is ONE serial sum against the V_{t+1} the handle or batch already holds.  G_1(y)
//     equals the loop of StaffRecursion.java:127-172, run at every period over the second lambdas, bit for bit when no state x of
//     periods 2 .. T that those sums reach has x + policy(x) > n_rows - 1: that loop SKIPS such actions (:148-149), the solved
//     recursion integrates them over the table's last row (:93-94).  tests/staff_gy_twin.py restates the loop and the condition.
//     (The Java's inner call at :161 has one argument and so resolves to the method of :81-118, over lambdas that differ from the
//     solved ones in periods 2 .. T only by the missing clamp.)
//   * A level is OFF THE GRID when one of its successors nn, j < len(y), lies outside the stored grid [x_lo, x_lo + nx) of
//     period t + 1 (zero-probability entries count): the host refuses it before anything is launched (staff_gy_first_off_grid),
//     so every read of the kernel below is one the host has checked.
//   * The sum of one level is ONE function, staff_gy_level, compiled for the host (sdpgpu_staff_gy_host) and for the device
//     (staff_gy_kernel).  Its chain is two dependent fp64 adds a step and its reads do not depend on it, so the reads of the next
//     kStaffGyU steps are issued before the current ones are added (two register sets in turn, as staff_g_kernel does); reads
//     past the row's end are folded onto its last entry and their steps not taken.
//   * staff_gy_kernel: ONE launch for every row of a call (any set of periods and a level window per period; for a batch, of
//     every instance).  A workgroup is one wave: 64 consecutive levels of one row, so a step reads one line of the transposed
//     table pT[j * n_rows + y] and one of V_{t+1}.  The host orders the blocks highest level first: those walk the longest rows.
//     No LDS, no atomics, results leave through ordinary vector stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdp {

constexpr int kStaffGyU = 8;  // steps per register set of staff_gy_level

struct StaffGyCost {
  double v, salary, pen;  // unitVariCost, salary, unitPenalty
  int32_t min_staff;      // minStaffNum[t]
  int32_t clamp, min_x, max_x;
};

// the next staff number as V_{t+1} is indexed by it (StaffFunctor.stateTransition)
__host__ __device__ __forceinline__ int staff_gy_next(const StaffGyCost& c, int n) {
  if (c.clamp) {
    n = n > c.max_x ? c.max_x : n;
    n = n < c.min_x ? c.min_x : n;
  }
  return n;
}

// G(y): p[j * p_stride] is entry j of the level's row, nj >= 1 its length; v_next (null: period T) holds V_{t+1} of the staff
// numbers next_x_lo ...
__host__ __device__ __forceinline__ double staff_gy_level(const StaffGyCost& c, int y, const double* __restrict__ p, int64_t p_stride, int nj,
                                                          const double* __restrict__ v_next, int next_x_lo) {
  constexpr int U = kStaffGyU;
  const double fv = 0.0 + c.v * (double)y;  // fixHireCost + variHireCost of the drawn period: the same for every step
  const bool future = v_next != nullptr;
  auto fetch = [&](int j0, double (&pp)[U], double (&vv)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u < nj ? j0 + u : nj - 1;
      pp[u] = p[(int64_t)j * p_stride];
      vv[u] = future ? v_next[staff_gy_next(c, y - j) - next_x_lo] : 0.0;
    }
  };
  double g = 0.0;
  auto steps = [&](int j0, const double (&pp)[U], const double (&vv)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u;
      if (j < nj) {
        const int n = y - j;  // nextStaffNum
        const double pen = n > c.min_staff ? 0.0 : c.pen * (double)(c.min_staff - n);
        const double imm = (fv + c.salary * (double)n) + pen;
        g += pp[u] * imm;
        if (future) g += pp[u] * vv[u];
      }
    }
  };
  double pa[U], va[U], pb[U], vb[U];
  fetch(0, pa, va);
  for (int j0 = 0; j0 < nj; j0 += 2 * U) {
    fetch(j0 + U, pb, vb);
    steps(j0, pa, va);
    fetch(j0 + 2 * U, pa, va);
    steps(j0 + U, pb, vb);
  }
  return g;
}

// The first successor of level y outside the grid [next_x_lo, next_x_lo + next_nx) of period t + 1, in ascending j: true and
// *bad_j, *bad_nn when there is one.  (The successors of a level are an interval, clamped or not: its two ends decide.)
inline bool staff_gy_first_off_grid(const StaffGyCost& c, int y, int nj, int64_t next_x_lo, int64_t next_nx, int* bad_j, int* bad_nn) {
  auto off = [&](int j) {
    const int64_t nn = staff_gy_next(c, y - j);
    return nn < next_x_lo || nn >= next_x_lo + next_nx;
  };
  if (!off(0) && !off(nj - 1)) return false;
  for (int j = 0; j < nj; ++j)
    if (off(j)) {
      *bad_j = j;
      *bad_nn = staff_gy_next(c, y - j);
      return true;
    }
  return false;
}

// ---- device ----

struct StaffGyRow {  // one G row of a call: the levels y_lo .. y_lo + n - 1 of one (instance, period)
  const double* pT;        // the period's table, transposed: pT[j * n_rows + y]
  const int32_t* row_len;  // [n_rows]
  const double* v_next;    // V_{t+1} of the staff numbers next_x_lo ..; null: period T
  double* out;             // [n]
  StaffGyCost c;
  int32_t n_rows, y_lo, n, next_x_lo;
};

struct StaffGyBlock {  // 64 levels of a row, from entry e0
  int32_t row, e0;
};

// grid = blocks, 64 threads.  (A template so that every translation unit that launches it may include this header.)
template <int U>
__global__ __launch_bounds__(64) void staff_gy_kernel(const StaffGyRow* __restrict__ rows, const StaffGyBlock* __restrict__ blocks) {
  static_assert(U == kStaffGyU, "the register sets of staff_gy_level");
  const StaffGyBlock B = blocks[blockIdx.x];
  const StaffGyRow& R = rows[B.row];
  const int e = B.e0 + (int)threadIdx.x;
  if (e >= R.n) return;
  const int y = R.y_lo + e;  // < n_rows: the host refuses anything else
  R.out[e] = staff_gy_level(R.c, y, R.pT + y, (int64_t)R.n_rows, R.row_len[y], R.v_next, R.next_x_lo);
}

}  // namespace sdp
