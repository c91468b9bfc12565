// sdp_staff_sep.hpp -- OPT-IN separable mode of the STAFF family (SDPGPU_KERNEL_SEPARABLE on a workforce handle).
//
// The lambdas of the workforce drivers read the staff number x and the hire a only through the hire-up-to level y = x + a:
// the pmf is pmfs[t][min(y, rows - 1)] (StaffRecursion.java:92-95), and salary, penalty and the transition read the staff
// left, y - j (WorkforceTesting.java:92-107, WorkforcePlanning.java:84-101).  In real arithmetic
//     Q_t(x, a) = c(a) P_t(y) + G_t(y),     c(a) = (a > 0 ? fixCost : 0) + unitVariCost a,
//     G_t(y)    = sum_{j < len(row)} p_row(j) w_t(y - j) + p_row(j) V_{t+1}(clamp(y - j)),   row = min(y, rows - 1),
//     w_t(n)    = salary n + (n > minStaff_t ? 0 : unitPenalty (minStaff_t - n)),            P_t(y) = sum_{j < len(row)} p_row(j),
// so a period costs sum over the levels of len(row) steps for the rows G and P (staff_g_kernel) and S A steps for the scan
// (staff_sep_min_kernel) instead of the S A D cells of the kernels in sdp_staff.hpp.
//
// This REASSOCIATES the reference's sum (the hiring cost leaves every term and multiplies the row's weight once): values agree
// with the cell-by-cell kernels to rounding (1e-9 relative), the hire count may differ where two actions tie to that
// rounding.  With fixCost = unitVariCost = salary = 0 nothing is reassociated (c(a) = 0, w the bare penalty) and the tables
// are the oracle's bit for bit.  tests/staff_separable_twin.py restates both kernels bit for bit.
#pragma once
#include "sdp_device.hpp"
#include "sdp_staff.hpp"

namespace sdp {

constexpr int kStaffSepU = 16;  // realisations a trip of staff_g_kernel, the next trip's reads issued ahead

// One lane per level y = y0 + e, e < n_levels: the lanes of a wave are 64 consecutive levels, so a step reads one line of the
// transposed table and one of V_{t+1}; the levels on or beyond the table's last row read one address.  A lane walks its row
// SERIALLY in ascending j -- g += p w; g += p V -- and adds the row's weights in the same loop.  Its chain is two dependent
// fp64 adds a step and its reads do not depend on it, so the reads of the next kStaffSepU steps are issued before the
// current ones are added (two register sets in turn).
// With some 1e3 - 1e4 levels a SIMD holds one wave, and what a step costs is the instructions that wave issues.  So the step
// counter is the WAVE's: the loop runs to the longest row among the wave's levels, which makes the table row of a step a scalar
// address (plus the lane's constant level offset) and the staff left y - j one fp64 subtraction from a scalar; (double)n and
// (double)(minStaff - n) are formed as y - j and minStaff - n in fp64, exact on integers below 2^53 and hence the conversions'
// bits.  A lane whose own row is shorter does NOT TAKE the steps past its end (the reads there stay inside the table, whose
// device copy holds zeros behind a row's length; whatever the caller's array held there never reaches G or P); the trips
// that lie inside every row of the wave run without that test.  Reads ahead of the longest row are folded onto its last step.
// Addresses are a scalar base + a 32-bit byte offset: the launcher refuses tables beyond 2 GiB.
template <bool FUTURE>
__global__ __launch_bounds__(64) void staff_g_kernel(StaffParams P, const double* __restrict__ pT,
                                                     const int32_t* __restrict__ row_len,
                                                     const double* __restrict__ v_next, double* __restrict__ g_out,
                                                     double* __restrict__ p_out, int y0, int n_levels) {
  constexpr int U = kStaffSepU;
  const int e_own = (int)blockIdx.x * 64 + (int)threadIdx.x;
  const int e = e_own < n_levels ? e_own : n_levels - 1;  // (lanes past the last level repeat it and store nothing)
  const int y = y0 + e;
  const int row = y >= P.n_rows - 1 ? P.n_rows - 1 : y;  // :93-94
  const int nj = row_len[row];                           // >= 1 (sdpgpu_set_level_pmf)
  int kmax = nj, kmin = nj;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    kmax = max(kmax, __shfl_xor(kmax, off, 64));
    kmin = min(kmin, __shfl_xor(kmin, off, 64));
  }
  kmax = __builtin_amdgcn_readfirstlane(kmax);
  kmin = __builtin_amdgcn_readfirstlane(kmin);
  const char* pb = reinterpret_cast<const char*>(pT);
  const char* vb = reinterpret_cast<const char*>(v_next);
  const uint32_t row_bytes = (uint32_t)P.n_rows * 8u;
  const uint32_t row_off = (uint32_t)row * 8u;
  // index into V_{t+1} of the staff left n: clamp(n, nn_lo, nn_hi) - next_x_lo ([minX, maxX] when clamped, else the next
  // period's box, never binding inside a row)
  const int yv = y - P.next_x_lo, v_lo = P.nn_lo - P.next_x_lo, v_hi = P.nn_hi - P.next_x_lo;
  const double yd = (double)y, msd = (double)P.min_staff;
  auto fetch = [&](int j0, double (&p)[U], double (&vn)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u < kmax ? j0 + u : kmax - 1;  // (scalar)
      p[u] = *reinterpret_cast<const double*>(pb + ((uint32_t)j * row_bytes + row_off));
      if constexpr (FUTURE) {
        int i = yv - j;
        i = i > v_hi ? v_hi : i;
        i = i < v_lo ? v_lo : i;
        vn[u] = *reinterpret_cast<const double*>(vb + (uint32_t)(i * 8));
      } else {
        vn[u] = 0.0;
      }
    }
  };
  double g = 0.0, ps = 0.0;
  auto steps = [&](auto guard_tag, int j0, const double (&p)[U], const double (&vn)[U]) {
    constexpr bool GUARD = decltype(guard_tag)::value;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u;
      if (!GUARD || j < nj) {
        const double nd = yd - (double)j;  // (double)nextStaffNum
        const double penalty = nd > msd ? 0.0 : P.pen * (msd - nd);
        const double w = P.salary * nd + penalty;
        g += p[u] * w;
        if constexpr (FUTURE) g += p[u] * vn[u];
        ps += p[u];
      }
    }
  };
  double pa[U], va[U], pb2[U], vb2[U];
  fetch(0, pa, va);
  int j0 = 0;
  for (; j0 + 2 * U <= kmin; j0 += 2 * U) {  // inside every row of the wave
    fetch(j0 + U, pb2, vb2);
    steps(std::false_type{}, j0, pa, va);
    fetch(j0 + 2 * U, pa, va);
    steps(std::false_type{}, j0 + U, pb2, vb2);
  }
  for (; j0 < kmax; j0 += 2 * U) {
    fetch(j0 + U, pb2, vb2);
    steps(std::true_type{}, j0, pa, va);
    fetch(j0 + 2 * U, pa, va);
    steps(std::true_type{}, j0 + U, pb2, vb2);
  }
  if (e_own < n_levels) {
    g_out[e_own] = g;
    p_out[e_own] = ps;
  }
}

// V_t and the policy of the slab [lo, hi) from the rows G and P over its levels (entry 0 = level x_lo + lo): a workgroup takes
// 64 states x 4 action strides, as phase 2 of separable_f1_kernel does; each stride scans its actions in ascending order with
// the reference's strict compare from (Double.MAX_VALUE, 0) (StaffRecursion.java:87-89, 110-113), the four are combined in
// (value, action) order -- the lowest action wins among equals.  G and P are read from global memory: the lanes are
// consecutive states, hence consecutive entries, and the rows (some 1e3 - 1e4 doubles) stay in L2.
constexpr size_t kStaffSepMinLds = 256 * (sizeof(double) + sizeof(int));

__global__ __launch_bounds__(256) void staff_sep_min_kernel(StaffParams P, const double* __restrict__ g,
                                                            const double* __restrict__ ps, double* __restrict__ v_cur,
                                                            int32_t* __restrict__ pol, int64_t lo, int64_t hi) {
  __shared__ double s_val[256];
  __shared__ int s_k[256];
  static_assert(sizeof(double) * 256 + sizeof(int) * 256 == kStaffSepMinLds, "the LDS the launch plan reports");
  const int tid = threadIdx.x;
  const int sx = tid & 63, as = tid >> 6;
  const int64_t i0 = lo + (int64_t)blockIdx.x * 64;
  double best = 1.7976931348623157e308;
  int bestk = 0;
  if (i0 + sx < hi) {
    const double* gs = g + (i0 - lo) + sx;  // level of (state, action k): entry (state - lo) + k
    const double* pp = ps + (i0 - lo) + sx;
#pragma unroll 4
    for (int k = as; k < P.n_actions; k += 4) {
      const double q = ((k > 0 ? P.K : 0.0) + P.v * (double)k) * pp[k] + gs[k];
      if (q < best) {
        best = q;
        bestk = k;
      }
    }
  }
  s_val[tid] = best;
  s_k[tid] = bestk;
  __syncthreads();
  const int64_t idx = i0 + tid;
  if (tid < 64 && idx < hi) {
    double bv = s_val[tid];
    int bk = s_k[tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const double ov = s_val[w * 64 + tid];
      const int ok = s_k[w * 64 + tid];
      if (better<false>(ov, ok, bv, bk)) {
        bv = ov;
        bk = ok;
      }
    }
    v_cur[idx] = bv;
    pol[idx] = bk;
  }
}

}  // namespace sdp
