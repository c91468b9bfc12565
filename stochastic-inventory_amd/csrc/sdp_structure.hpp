// sdp_structure.hpp -- the reference's structure checks on the rows of a solved batch: sdp.inventory.CheckKConvexity.check
// (CheckKConvexity.java:39-68, K-convexity) and checkCK (:6-36, CK-convexity of Gallego and Scheller-Wolf 2000), and the G(y)
// rows they are run on (the second Recursion of capacitated.CLSPforDraw.main, CLSPforDraw.java:147-170, for any period).
//
//   * A row is g[0 .. n): fp64 values at CONSECUTIVE grid points.  The reference takes xLength from the first and the last
//     abscissa ((int) (max - min + 1), :9 / :42); for the unit-spaced rows every caller builds that is the row's length, so
//     here xLength = n and the abscissae are not passed.
//   * The predicate of one triple is ONE function, convexity_triple below, compiled for the host (sdpgpu_check_convexity, the
//     plain loops of convexity_host) and for the device (convexity_kernel): fp64, left to right, no FMA (-ffp-contract=off),
//     an IEEE division.  A triple VIOLATES when !(lhs > rhs0 - 0.1) -- the Java `if (... > ...) continue; else`: a NaN on
//     either side and equality both violate.  Both checks return at the FIRST violation in loop order.
//   * The device reduces to that first violation with integers only: a violating triple becomes a 64-bit key that sorts like
//     the loop order (outer << 42 | middle << 21 | inner), the minimum is taken inside the wave, inside the workgroup (an LDS
//     atomic) and with ONE global atomicMin per workgroup on the row's key.  A minimum does not depend on the order of its
//     operands, so the result is reproducible; convexity_finish_kernel recomputes lhs and rhs0 of the winning triple with the
//     same predicate and writes the struct.  A workgroup stops early once the row's key is already below everything it could
//     still find -- that only skips triples which cannot win.
//   * convexity_kernel: one launch for every row of a call.  A task is (row, a run of outer indices) with roughly equal triple
//     counts (the loops are triangular; convexity_tasks); its workgroup stages the row in LDS once, a wave takes an
//     (outer, middle) pair, the lanes run the innermost index: g[c] (g[y - b]) is one contiguous ds_read_b64, g[a] and g[b]
//     (g[y + z] and g[y]) are wave-uniform.
//   * gy_kernel: one thread per (instance, period, y), the demand loop serial and in the reference's order, with jmax of
//     sdp_device.hpp and the family's clamp (upper bound first, then lower: CLSPforDraw.java:150-151).
//
// Global memory is written with ordinary vector stores and integer atomics from plain C++ only.
#pragma once
#include "sdp_device.hpp"

#include <vector>

namespace sdp {

constexpr int kConvexityCheck = 0;    // CheckKConvexity.check
constexpr int kConvexityCheckCK = 1;  // CheckKConvexity.checkCK
constexpr int kConvexityMaxRow = 8192;  // points of a row: 64 KiB of LDS (two workgroups to a CU), and three indices of 21 bits in a key
constexpr unsigned long long kConvexityNoKey = ~0ull;

// One triple of either check (:16 / :48).  check: far = g[a], mid = g[b], near = g[c], mult = a - b, div = b - c;
// checkCK: far = g[y + z], mid = g[y], near = g[y - b], mult = z, div = b.  True iff the triple PASSES; *lhs and *rhs0 are the
// two numbers the reference prints at a violation (:19-20 / :51-52).
__host__ __device__ __forceinline__ bool convexity_triple(double g_far, double g_mid, double g_near, int mult, int div, double K,
                                                          double* lhs, double* rhs0) {
  double t = g_mid - g_near;
  t = (double)mult * t;
  t = t / (double)div;
  *rhs0 = g_mid + t;
  *lhs = g_far + K;
  return *lhs > *rhs0 - 0.1;
}

// The loops of a row by kind, as (outer o, middle m, inner i):  check: o = a, m = b in [1, a) (b = 0 has no c), i = c in
// [0, b);  checkCK: o = y, m = z in [0, min(capacity, n - y)), i = b in [1, min(capacity, y)) -- the reference's two skips
// (y - b <= 0, y + z >= xLength) as loop bounds.
template <int KIND>
__host__ __device__ __forceinline__ int convexity_mid_lo() { return KIND == kConvexityCheck ? 1 : 0; }
template <int KIND>
__host__ __device__ __forceinline__ int convexity_mid_hi(int n, int capacity, int o) {
  if (KIND == kConvexityCheck) return o;
  const int room = n - o;
  return capacity < room ? capacity : room;
}
template <int KIND>
__host__ __device__ __forceinline__ int convexity_in_lo() { return KIND == kConvexityCheck ? 0 : 1; }
template <int KIND>
__host__ __device__ __forceinline__ int convexity_in_hi(int capacity, int o, int m) {
  if (KIND == kConvexityCheck) return m;
  return capacity < o ? capacity : o;
}
// where triple (o, m, i) of a row reads, and its two integers (the comment of convexity_triple); far and mid depend on the
// (outer, middle) pair alone
template <int KIND>
__host__ __device__ __forceinline__ int convexity_far(int o, int m) { return KIND == kConvexityCheck ? o : o + m; }
template <int KIND>
__host__ __device__ __forceinline__ int convexity_mid(int o, int m) { return KIND == kConvexityCheck ? m : o; }
template <int KIND>
__host__ __device__ __forceinline__ int convexity_near(int o, int i) { return KIND == kConvexityCheck ? i : o - i; }
template <int KIND>
__host__ __device__ __forceinline__ int convexity_mult(int o, int m) { return KIND == kConvexityCheck ? o - m : m; }
template <int KIND>
__host__ __device__ __forceinline__ int convexity_div(int m, int i) { return KIND == kConvexityCheck ? m - i : i; }
// the predicate on triple (o, m, i) of a row
template <int KIND>
__host__ __device__ __forceinline__ bool convexity_at(const double* g, int o, int m, int i, double K, double* lhs, double* rhs0) {
  return convexity_triple(g[convexity_far<KIND>(o, m)], g[convexity_mid<KIND>(o, m)], g[convexity_near<KIND>(o, i)], convexity_mult<KIND>(o, m),
                          convexity_div<KIND>(m, i), K, lhs, rhs0);
}
// triples of outer index o
template <int KIND>
inline int64_t convexity_count(int n, int capacity, int o) {
  if (KIND == kConvexityCheck) return (int64_t)o * (o - 1) / 2;
  const int64_t nm = convexity_mid_hi<KIND>(n, capacity, o), ni = (int64_t)convexity_in_hi<KIND>(capacity, o, 0) - 1;
  return nm > 0 && ni > 0 ? nm * ni : 0;
}

__host__ __device__ __forceinline__ unsigned long long convexity_key(int o, int m, int i) {
  return ((unsigned long long)o << 42) | ((unsigned long long)m << 21) | (unsigned long long)i;
}

// what sdpgpu_convexity holds (include/sdpgpu.h), field for field
struct ConvexityOut {
  int32_t holds, i0, i1, i2;
  double lhs, rhs;
};

__host__ __device__ __forceinline__ void convexity_write(ConvexityOut* out, const double* g, int kind, double K, unsigned long long key) {
  ConvexityOut r{1, -1, -1, -1, 0.0, 0.0};
  if (key != kConvexityNoKey) {
    r.holds = 0;
    r.i0 = (int32_t)(key >> 42);
    r.i1 = (int32_t)((key >> 21) & 0x1fffff);
    r.i2 = (int32_t)(key & 0x1fffff);
    if (kind == kConvexityCheck)
      (void)convexity_at<kConvexityCheck>(g, r.i0, r.i1, r.i2, K, &r.lhs, &r.rhs);
    else
      (void)convexity_at<kConvexityCheckCK>(g, r.i0, r.i1, r.i2, K, &r.lhs, &r.rhs);
  }
  *out = r;
}

// ---- host: the reference's loops as they stand ----
template <int KIND>
inline unsigned long long convexity_host_kind(const double* g, int n, double K, int capacity) {
  for (int o = 0; o < n; ++o) {
    const int m_hi = convexity_mid_hi<KIND>(n, capacity, o);
    for (int m = convexity_mid_lo<KIND>(); m < m_hi; ++m) {
      const int i_hi = convexity_in_hi<KIND>(capacity, o, m);
      for (int i = convexity_in_lo<KIND>(); i < i_hi; ++i) {
        double lhs, rhs0;
        if (!convexity_at<KIND>(g, o, m, i, K, &lhs, &rhs0)) return convexity_key(o, m, i);
      }
    }
  }
  return kConvexityNoKey;
}

inline void convexity_host(int kind, const double* g, int n, double K, int capacity, ConvexityOut* out) {
  const unsigned long long key = kind == kConvexityCheck ? convexity_host_kind<kConvexityCheck>(g, n, K, capacity)
                                                         : convexity_host_kind<kConvexityCheckCK>(g, n, K, capacity);
  convexity_write(out, g, kind, K, key);
}

// ---- device ----

struct ConvexityRow {
  const double* g;  // device
  double K;
  int32_t n, capacity, kind, pad;
};

struct ConvexityTask {
  int32_t row, o_lo, o_hi;  // outer indices o_lo .. o_hi - 1 of the row
};

// The tasks of one row, appended: runs of outer indices of about `target` triples each, in ascending order (the tiles that can
// hold the first violation come first, so the later ones may find the row's key already below theirs).
inline void convexity_tasks(int32_t row, int kind, int n, int capacity, int64_t target, std::vector<ConvexityTask>* tasks) {
  int lo = -1;
  int64_t have = 0;
  for (int o = 0; o < n; ++o) {
    const int64_t c = kind == kConvexityCheck ? convexity_count<kConvexityCheck>(n, capacity, o) : convexity_count<kConvexityCheckCK>(n, capacity, o);
    if (c == 0 && lo < 0) continue;
    if (lo < 0) lo = o;
    have += c;
    if (have >= target) {
      tasks->push_back(ConvexityTask{row, lo, o + 1});
      lo = -1;
      have = 0;
    }
  }
  if (lo >= 0 && have > 0) tasks->push_back(ConvexityTask{row, lo, n});
}

// One task of one kind: s_g holds the row, s_key the workgroup's smallest key so far.
template <int KIND>
__device__ __forceinline__ void convexity_run(const ConvexityRow& R, const ConvexityTask& T, const double* s_g, unsigned long long* s_key,
                                              const unsigned long long* row_key, int wave, int lane) {
  const int n = R.n, cap = R.capacity;
  const double K = R.K;
  for (int o = T.o_lo; o < T.o_hi; ++o) {
    // nothing from outer index o on can win any more (wave-uniform; relaxed reads: a stale value only costs work).  The
    // workgroup's own key is an LDS read per outer index, the row's key a trip to L2 on every 16th.
    const unsigned long long floor_key = convexity_key(o, 0, 0);
    if (*(volatile unsigned long long*)s_key < floor_key) return;
    if (((o - T.o_lo) & 15) == 15 && __hip_atomic_load(row_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < floor_key) return;
    const int m_hi = convexity_mid_hi<KIND>(n, cap, o);
    for (int m = convexity_mid_lo<KIND>() + wave; m < m_hi; m += 4) {
      const int i_lo = convexity_in_lo<KIND>(), i_hi = convexity_in_hi<KIND>(cap, o, m);
      // the pair's two wave-uniform values, read once (the LDS atomic below keeps the compiler from hoisting them itself)
      const double g_far = s_g[convexity_far<KIND>(o, m)], g_mid = s_g[convexity_mid<KIND>(o, m)];
      const int mult = convexity_mult<KIND>(o, m);
      for (int base = i_lo; base < i_hi; base += 64) {
        const int i = base + lane;
        const bool live = i < i_hi;
        const int ii = live ? i : i_lo;  // (an idle lane repeats a triple of the row: no read outside it)
        double lhs, rhs0;
        const bool bad = live && !convexity_triple(g_far, g_mid, s_g[convexity_near<KIND>(o, ii)], mult, convexity_div<KIND>(m, ii), K, &lhs, &rhs0);
        const unsigned long long mask = __ballot(bad);
        if (mask) {
          // the wave's first violation in loop order: every triple it would still visit sorts after this one
          if (lane == 0) atomicMin(s_key, convexity_key(o, m, base + (int)__builtin_ctzll(mask)));
          return;
        }
      }
    }
  }
}

// grid = tasks, 256 threads, dynamic LDS = convexity_lds(the longest row of the launch): the workgroup's key and its skip
// flag in the first 16 bytes, then the row (ONE LDS object).  keys[row] starts at kConvexityNoKey.
__host__ __device__ inline size_t convexity_lds(int n_max) { return 16 + (size_t)n_max * sizeof(double); }

__global__ __launch_bounds__(256) void convexity_kernel(const ConvexityRow* __restrict__ rows, const ConvexityTask* __restrict__ tasks,
                                                        unsigned long long* __restrict__ keys) {
  extern __shared__ unsigned long long s_lds[];
  unsigned long long* s_key = s_lds;
  int* s_skip = reinterpret_cast<int*>(s_lds + 1);
  double* s_g = reinterpret_cast<double*>(s_lds + 2);
  const ConvexityTask T = tasks[blockIdx.x];
  const ConvexityRow R = rows[T.row];
  unsigned long long* row_key = keys + T.row;
  if (threadIdx.x == 0) {  // (one read for the whole workgroup, so that it leaves as one)
    *s_key = kConvexityNoKey;
    *s_skip = __hip_atomic_load(row_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < convexity_key(T.o_lo, 0, 0);
  }
  __syncthreads();
  if (*s_skip) return;
  for (int q = threadIdx.x; q < R.n; q += 256) s_g[q] = R.g[q];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (R.kind == kConvexityCheck)
    convexity_run<kConvexityCheck>(R, T, s_g, s_key, row_key, wave, lane);
  else
    convexity_run<kConvexityCheckCK>(R, T, s_g, s_key, row_key, wave, lane);
  __syncthreads();
  if (threadIdx.x == 0 && *s_key != kConvexityNoKey) atomicMin(row_key, *s_key);
}

__global__ __launch_bounds__(256) void convexity_key_fill_kernel(unsigned long long* __restrict__ keys, int n_rows) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < n_rows) keys[r] = kConvexityNoKey;
}

// one thread per row: the struct of the winning triple
__global__ __launch_bounds__(256) void convexity_finish_kernel(const ConvexityRow* __restrict__ rows, const unsigned long long* __restrict__ keys,
                                                               int n_rows, ConvexityOut* __restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  const ConvexityRow R = rows[r];
  convexity_write(out + r, R.g, R.kind, R.K, keys[r]);
}

// ---- G(y) of every (instance, period) of a solved batch ----

struct GyPair {
  int64_t pmf_off;     // the period's probabilities in the batch's pmf arena
  int64_t v_next_off;  // V_{t+1} in the value arena; -1: period T, no future term (Recursion.java:140)
  int64_t out_off;     // the G row in the batch's G arena
  double x_min, x_max, d0, h, pi, v;
  int32_t nx, n_demand;
};

// One workgroup per (instance, period), a thread per level y; the demand index ascends as in Recursion.java:138-143 with the
// lambdas of CLSPforDraw.java:147-170 for the drawn period: fixedCost = 0, variableCost = v * y, level = y - d.
__global__ __launch_bounds__(256) void gy_kernel(const GyPair* __restrict__ pairs, double step, double inv_step, const double* __restrict__ pmf,
                                                 const double* __restrict__ values, double* __restrict__ gy) {
  const GyPair P = pairs[blockIdx.x];
  const double* __restrict__ p = pmf + P.pmf_off;
  const double* __restrict__ v_next = P.v_next_off >= 0 ? values + P.v_next_off : nullptr;
  for (int iy = threadIdx.x; iy < P.nx; iy += 256) {
    const double y = P.x_min + (double)iy * step;
    const double fv = 0.0 + P.v * y;  // fixedCost + variableCost
    double acc = 0.0;
    for (int j = 0; j < P.n_demand; ++j) {
      const double d = P.d0 + (double)j * step;
      const double lev = y - d;
      const double imm = (fv + P.h * jmax(lev, 0.0)) + P.pi * jmax(-lev, 0.0);
      acc += p[j] * imm;
      if (v_next) {
        double nx = lev;
        nx = nx > P.x_max ? P.x_max : nx;
        nx = nx < P.x_min ? P.x_min : nx;
        acc += p[j] * v_next[(int)((nx - P.x_min) * inv_step)];
      }
    }
    gy[P.out_off + iy] = acc;
  }
}

}  // namespace sdp
