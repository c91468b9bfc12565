// sdp_batch.hpp -- period kernel of a BATCH of backorder-family (F1) instances of one grid shape: period t of all N
// instances in ONE launch (sdpgpu_batch_solve, sdpgpu_batch.hip).
//
// The per-cell arithmetic is window_f1_kernel's (sdp_window.hpp), operation for operation: a lane owns S adjacent states
// and R actions in registers and walks the demand index j = 0..D-1 serially,
//     imm = c0[r] + W.x;  t = p_j*imm;  acc += t;  u = p_j*W.y;  acc += u;
// separate multiplies and adds, strict compare in ascending action order -- so every instance's tables are bit for bit
// those of a single handle.  New is what surrounds it:
//
//   * a TASK (one wave) is (instance, state tile, action chunk); tasks are packed four to a workgroup regardless of the
//     instance, so a workgroup may hold four different instances.  Everything an instance owns -- its cost constants, the
//     level of m = 0, its demand count and the places of its probabilities and tables in the batch's arenas -- comes
//     from a small per-(period, instance) record (BatchInst) read with wave-uniform loads; the probabilities are staged in
//     LDS per WAVE (window_f1_kernel keeps one copy per workgroup, which all four waves write alike).
//   * the records of a period are sorted by demand count, longest first (stable): D differs between instances by up to
//     ~30x (NormalDist(3, 0.3): 4 points, NormalDist(54, 16.2): 121), tasks are dispatched in index order, and the
//     tail of the launch is then made of short tasks.
//   * the LDS of a launch is sized for the period's widest instance; a narrower one uses the front of its wave's region.
//
// Global memory is written with ordinary vector stores from plain C++ only.
#pragma once
// sdp_window.hpp defines three non-template kernels, which a second translation unit cannot define again under the same
// names.  This unit takes its own copies under batch_* names (it launches two of them: the key reset and the finalize
// pass); the header itself stays as it is, its digest pins the stored counter summaries of the bench workloads.
#define key_fill_kernel batch_key_fill_kernel
#define finalize_kernel batch_finalize_kernel
#define separable_f2_expand_kernel batch_unused_f2_expand_kernel
#include "sdp_window.hpp"
#undef key_fill_kernel
#undef finalize_kernel
#undef separable_f2_expand_kernel

namespace sdp {

// One instance in one period, in task order.  Offsets are ELEMENT offsets into the batch's arenas.
struct BatchInst {
  double lev0;         // level of m = 0: min_inventory - d_0 (d_0 may be negative: GetPmf truncates a negative quantile toward 0)
  double h, pi, K, v;
  int32_t idx_off;     // m -> index into V_{t+1}: -d_0 / step
  int32_t n_demand;    // D of this (instance, period)
  int32_t d_pad;       // D rounded up to R + S - 1 (padded steps carry p = 0)
  int32_t d_main;      // floor(D / (R + S - 1)) * (R + S - 1)
  int64_t pmf_off;     // probabilities p_0 .. p_{D-1}, followed by kPmfPad zeros
  int64_t v_cur_off;   // V_t row of the instance (fp64 arena)
  int64_t v_next_off;  // V_{t+1} row (unused in the last period)
  int64_t pol_off;     // policy row (int32 arena)
  int64_t key_cur_off, key_next_off;  // key rows of V_t / V_{t+1} (chunked plans)
  int64_t chunk_off;   // chunk rows [n_chunks][n_states] of this (instance, period) (chunked plans)
};

struct BatchLaunch {
  double step;
  int32_t n_states;       // states of the shared grid
  int32_t n_actions;      // A
  int32_t n_tiles;        // state tiles of 64 S states per instance
  int32_t n_chunks;       // tasks per state tile
  int32_t chunk_blocks;   // R-blocks per task
  int32_t tasks_per_inst; // n_tiles * n_chunks; task = rank * tasks_per_inst + chunk * n_tiles + tile
  int32_t n_tasks;
  int32_t span_max;       // window entries of a wave's LDS region (the period's widest instance)
  int32_t p_slots_max;    // doubles of a wave's probability copy
  int32_t maxdir;
};

// LDS of a workgroup: four windows and four probability copies
__host__ __device__ inline size_t batch_wg_lds(int span_max, int p_slots_max) {
  return (size_t)4 * span_max * 16 + (size_t)4 * p_slots_max * 8;
}

template <int R, int S, bool FUTURE, bool KEYED_IN>
__global__ __launch_bounds__(256) void window_f1_batch_kernel(BatchLaunch L, const BatchInst* __restrict__ inst,
                                                              double* __restrict__ values, int32_t* __restrict__ policy,
                                                              const double* __restrict__ pmf,
                                                              unsigned long long* __restrict__ keys,
                                                              double* __restrict__ chunk_val, int32_t* __restrict__ chunk_idx) {
  constexpr int NW = R + S - 1;  // register window entries = demand steps per unrolled block
  constexpr int TS = 64 * S;     // states per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int task = blockIdx.x * 4 + wave;
  if (task >= L.n_tasks) return;  // no workgroup barrier below: a wave may leave on its own
  const int rank = task / L.tasks_per_inst;
  const int local = task - rank * L.tasks_per_inst;
  const int chunk = local / L.n_tiles;
  const int tile = local - chunk * L.n_tiles;
  const BatchInst& I = inst[rank];  // (wave-uniform)
  // the instance's constants in the shape window_entry takes them
  WinParams W{};
  W.lev0 = I.lev0;
  W.step = L.step;
  W.h = I.h;
  W.pi = I.pi;
  W.K = I.K;
  W.v = I.v;
  W.idx_off = I.idx_off;
  W.next_last = L.n_states - 1;
  W.n_actions = L.n_actions;
  W.d_pad = I.d_pad;
  W.d_main = I.d_main;
  W.n_demand = I.n_demand;
  W.chunk_blocks = L.chunk_blocks;
  const bool MAXDIR = L.maxdir != 0;
  const double* __restrict__ v_next = FUTURE && !KEYED_IN ? values + I.v_next_off : nullptr;
  const unsigned long long* __restrict__ k_next = KEYED_IN ? keys + I.key_next_off : nullptr;
  const double* __restrict__ pmf_p = pmf + I.pmf_off;
  const int hi = L.n_states;

  const int chunk_actions = W.chunk_blocks * R;
  const int span = TS + chunk_actions + W.d_pad + S;  // entries [0, span): slot 0 is a spare; span <= L.span_max
  double2* s_win = reinterpret_cast<double2*>(smem) + (size_t)wave * L.span_max;
  double* s_p = reinterpret_cast<double*>(smem + (size_t)4 * L.span_max * 16) + (size_t)wave * L.p_slots_max;
  const int i0 = tile * TS;
  const int kA = chunk * chunk_actions;

  // stage this wave's window: slot q holds m = m_lo + q (four entries per pass, their loads in flight together; slots past
  // the span are computed from clamped indices and land in the spare slot 0 -- see window_f1_kernel)
  const int m_lo = i0 + kA - W.d_pad;
  for (int q0 = lane; q0 < span; q0 += 256) {
    double2 e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = window_entry<FUTURE, KEYED_IN>(W, v_next, k_next, m_lo + q0 + 64 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u) s_win[q0 + 64 * u < span ? q0 + 64 * u : 0] = e[u];
  }
  {
    const int p_cnt = win_p_slots(W.n_demand) - 2;  // (the array ends in kPmfPad = 16 zeros: D + 3 stays inside)
    for (int q0 = lane; q0 < p_cnt; q0 += 256) {
      double pv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) pv[u] = pmf_p[q0 + 64 * u < p_cnt ? q0 + 64 * u : p_cnt - 1];
#pragma unroll
      for (int u = 0; u < 4; ++u) s_p[q0 + 64 * u < p_cnt ? q0 + 64 * u : p_cnt] = pv[u];
    }
  }
  __builtin_amdgcn_wave_barrier();

  double best[S];
  int bestk[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    best[s] = MAXDIR ? -1.7976931348623157e308 : 1.7976931348623157e308;
    bestk[s] = 0;
  }
  for (int rb = 0; rb < W.chunk_blocks; ++rb) {
    const int k0 = kA + rb * R;
    if (k0 >= W.n_actions) break;
    double c0[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double a = (double)(k0 + r) * W.step;
      c0[r] = (a > 0 ? W.K : 0.0) + W.v * a;  // fixedCost + variableCost (wave-uniform)
    }
    // slot of (lane, s, r, j):  S*lane + s + (k0 - kA) + r - j + d_pad;  window entry q at step j: base - j + q
    const int base = S * lane + (k0 - kA) + W.d_pad;
    double2 win[NW];
    double acc[S][R];
    double immc[S][R];  // immc[s][r], s >= 1: immediate cost of (state s, action r) at the current demand step
#pragma unroll
    for (int q = 0; q < NW; ++q) win[q] = s_win[base + q];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        acc[s][r] = 0.0;
        immc[s][r] = c0[r] + win[r + s].x;  // (s = 0 unused)
      }
    }
    double p_cur = s_p[0];  // p_j of the step at hand; every step requests the next one's
#pragma unroll 1
    for (int jb = 0; jb < W.d_main; jb += NW) {
      {
        // priority by progress, as in window_f1_kernel: the resident waves of a SIMD -- here tasks of different lengths
        // -- advance by the same FRACTION of their work, so a short task does not wait behind a long one's age
        const unsigned done = (unsigned)(rb * W.d_main + jb);
        const unsigned pr = 3u - (4u * done) / (unsigned)(W.chunk_blocks * W.d_main + 1);
        if (pr == 0) __builtin_amdgcn_s_setprio(0);
        else if (pr == 1) __builtin_amdgcn_s_setprio(1);
        else if (pr == 2) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(3);
      }
      const double2* nxt = s_win + (base - jb - NW);  // slots base-jb-NW ... base-jb-1
      const double* pq = s_p + jb + 1;
#pragma unroll
      for (int t = 0; t < NW; ++t) {
        const double p = p_cur;
        // the cell (s = S-1, r = R-1) goes first: it alone reads the window's top entry, so the slide is requested at
        // the start of the step (see window_f1_kernel); every accumulator still sees its two adds in the reference's order
        if constexpr (S > 1) {
          acc[S - 1][R - 1] += p * immc[S - 1][R - 1];
          if constexpr (FUTURE) acc[S - 1][R - 1] += p * win[(R + S - 2 - t + NW) % NW].y;
        } else {
          const double2 wt = win[(R - 1 - t + NW) % NW];
          acc[0][R - 1] += p * (c0[R - 1] + wt.x);
          if constexpr (FUTURE) acc[0][R - 1] += p * wt.y;
        }
        win[(NW - 1 - t) % NW] = nxt[NW - 1 - t];
        p_cur = pq[t];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (S == 1 && r == R - 1) continue;
          const double2 w0 = win[(r - t + NW) % NW];
          const double imm0 = c0[r] + w0.x;
          acc[0][r] += p * imm0;
          if constexpr (FUTURE) acc[0][r] += p * w0.y;
#pragma unroll
          for (int s = 1; s < S; ++s) {
            if (r == R - 1 && s == S - 1) continue;
            acc[s][r] += p * immc[s][r];
            // (cells with the same r + s read the same entry: the product p * V is formed once for them)
            if constexpr (FUTURE) acc[s][r] += p * win[(r + s - t + NW) % NW].y;
          }
#pragma unroll
          for (int s = S - 1; s > 1; --s) immc[s][r] = immc[s - 1][r];
          if constexpr (S > 1) immc[1][r] = imm0;
        }
      }
    }
    // the last D mod NW demand steps: the same unrolled body under wave-uniform guards
    if (W.d_main < W.n_demand) {
      const int jb = W.d_main;
      const int rem = W.n_demand - W.d_main;
      const double2* nxt = s_win + (base - jb - NW);
#pragma unroll
      for (int t = 0; t < NW - 1; ++t) {
        if (t < rem) {
          const double p = p_cur;
          p_cur = s_p[jb + t + 1];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const double2 w0 = win[(r - t + NW) % NW];
            const double imm0 = c0[r] + w0.x;
            acc[0][r] += p * imm0;
            if constexpr (FUTURE) acc[0][r] += p * w0.y;
#pragma unroll
            for (int s = 1; s < S; ++s) {
              acc[s][r] += p * immc[s][r];
              if constexpr (FUTURE) acc[s][r] += p * win[(r + s - t + NW) % NW].y;
            }
#pragma unroll
            for (int s = S - 1; s > 1; --s) immc[s][r] = immc[s - 1][r];
            if constexpr (S > 1) immc[1][r] = imm0;
          }
          win[(NW - 1 - t) % NW] = nxt[NW - 1 - t];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = k0 + r;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        if (k < W.n_actions && (MAXDIR ? (acc[s][r] > best[s]) : (acc[s][r] < best[s]))) {
          best[s] = acc[s][r];
          bestk[s] = k;
        }
      }
    }
  }

  // results leave through the wave's own LDS region (its window is dead by now) so that every store instruction writes 64
  // CONSECUTIVE states: lane l owns states S*l .. S*l+S-1, but stores state 64*u + l
  if constexpr (S > 1) {
    __builtin_amdgcn_wave_barrier();
    double* t_val = reinterpret_cast<double*>(s_win);
    int* t_idx = reinterpret_cast<int*>(t_val + TS);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      t_val[S * lane + s] = best[s];
      t_idx[S * lane + s] = bestk[s];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < S; ++u) {
      best[u] = t_val[64 * u + lane];
      bestk[u] = t_idx[64 * u + lane];
    }
  }
  const bool chunked = L.n_chunks > 1;
  double* __restrict__ out_val = chunked ? chunk_val + I.chunk_off + (int64_t)chunk * L.n_states : values + I.v_cur_off;
  int32_t* __restrict__ out_idx = chunked ? chunk_idx + I.chunk_off + (int64_t)chunk * L.n_states : policy + I.pol_off;
  unsigned long long* __restrict__ k_cur = chunked ? keys + I.key_cur_off : nullptr;
#pragma unroll
  for (int u = 0; u < S; ++u) {
    const int idx = i0 + (S > 1 ? 64 * u + lane : lane);
    if (idx < hi) {
      out_val[idx] = best[u];
      out_idx[idx] = bestk[u];
      if (chunked) {
        if (MAXDIR)
          atomicMax(k_cur + idx, f64_key(best[u]));
        else
          atomicMin(k_cur + idx, f64_key(best[u]));
      }
    }
  }
}

// V_1(ini_inventory_i) and its action index for every instance: what a sweep main records (CLSPTesting.java:115-118).
// The two arrays share one buffer -- n doubles, then n int32 -- so that the host needs one copy.
__global__ __launch_bounds__(256) void batch_initial_kernel(const double* __restrict__ values, const int32_t* __restrict__ policy,
                                                            const int64_t* __restrict__ v_off, const int64_t* __restrict__ pol_off,
                                                            int n, double* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out_val[i] = values[v_off[i]];
  out_idx[i] = policy[pol_off[i]];
}

}  // namespace sdp
