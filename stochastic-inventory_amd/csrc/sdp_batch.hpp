// sdp_batch.hpp -- period kernel of a BATCH of backorder-family (F1) instances: period t of all N instances in ONE launch
// (sdpgpu_batch_solve, sdpgpu_batch.hip).  The instances may share one grid shape (sdpgpu_batch_create) or each have its
// own inventory bounds and order limit (sdpgpu_batch_create_ragged): a uniform batch is the ragged one with equal records.
//
// What a wave does with its task is window_f1_kernel's, by the very same code: f1_stage_window and f1_cells
// (sdp_f1_cells.hpp) -- so every instance's tables are bit for bit those of a single handle.  New is what surrounds it:
//
//   * a TASK (one wave) is (instance, state tile, action chunk); tasks are packed four to a workgroup regardless of the
//     instance, so a workgroup may hold four different instances.  Everything an instance owns -- its cost constants, the
//     level of m = 0, its demand count, its numbers of states, actions, tiles and chunks and the places of its
//     probabilities and tables in the batch's arenas -- comes from a small per-(period, instance) record (BatchInst) read
//     with wave-uniform loads; the probabilities are staged in LDS per WAVE (window_f1_kernel keeps one copy per workgroup,
//     which all four waves write alike).
//   * which record a task belongs to comes from the period's TASK TABLE (BatchTask, 8 bytes per task, made on the host once
//     per layout): instances have different numbers of tasks, so `task / tasks_per_instance` does not find the instance.
//     One wave-uniform 8-byte load replaces that division; a prefix array would cost a binary search of dependent loads.
//   * the records of a period are sorted by estimated task length -- R-blocks per task x demand count --, longest first
//     (stable): D differs between instances by up to ~30x (NormalDist(3, 0.3): 4 points, NormalDist(54, 16.2): 121) and
//     the order limit by 10x (ThreeLevelFitsSTest: 26 .. 288), tasks are dispatched in index order, and the tail of the
//     launch is then made of short tasks.
//   * the LDS of a launch is sized for the period's widest instance; a narrower one uses the front of its wave's region.
//
// Global memory is written with ordinary vector stores from plain C++ only.
#pragma once
#include "sdp_f1_cells.hpp"

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
  int32_t n_states;    // states of the instance's own grid
  int32_t n_actions;   // A of the instance
  int32_t n_tiles;     // its state tiles of 64 S states
  int32_t n_chunks;    // its tasks per state tile: ceil(its R-blocks / the period's chunk_blocks)
  int32_t chunk_blocks;  // R-blocks per task: the period's, or all of the instance's when it has fewer
  int32_t pad;
};

// One task of a period, in dispatch order: the record it belongs to and chunk * n_tiles + tile within that instance.
struct BatchTask {
  int32_t rank, local;
};

struct BatchLaunch {
  double step;
  int32_t n_tasks;
  int32_t span_max;       // window entries of a wave's LDS region (the period's widest instance)
  int32_t p_slots_max;    // doubles of a wave's probability copy
  int32_t maxdir;
  int32_t chunked;        // some instance has several chunks: EVERY instance writes chunk rows and key rows
  int32_t pad;
};

// LDS of a workgroup: four windows and four probability copies
__host__ __device__ inline size_t batch_wg_lds(int span_max, int p_slots_max) {
  return (size_t)4 * span_max * 16 + (size_t)4 * p_slots_max * 8;
}

template <int R, int S, bool FUTURE, bool KEYED_IN>
__global__ __launch_bounds__(256) void window_f1_batch_kernel(BatchLaunch L, const BatchInst* __restrict__ inst,
                                                              const BatchTask* __restrict__ tasks,
                                                              double* __restrict__ values, int32_t* __restrict__ policy,
                                                              const double* __restrict__ pmf,
                                                              unsigned long long* __restrict__ keys,
                                                              double* __restrict__ chunk_val, int32_t* __restrict__ chunk_idx) {
  constexpr int TS = 64 * S;     // states per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int task = blockIdx.x * 4 + wave;
  if (task >= L.n_tasks) return;  // no workgroup barrier below: a wave may leave on its own
  const BatchTask tk = tasks[task];     // (wave-uniform, as everything derived from it)
  const BatchInst& I = inst[tk.rank];
  const int chunk = tk.local / I.n_tiles;
  const int tile = tk.local - chunk * I.n_tiles;
  // the instance's constants in the shape the shared F1 code takes them (m_tab / c_tab null: the built-in CLSP costs)
  WinParams W{};
  W.lev0 = I.lev0;
  W.step = L.step;
  W.h = I.h;
  W.pi = I.pi;
  W.K = I.K;
  W.v = I.v;
  W.idx_off = I.idx_off;
  W.next_last = I.n_states - 1;
  W.n_actions = I.n_actions;
  W.d_pad = I.d_pad;
  W.d_main = I.d_main;
  W.n_demand = I.n_demand;
  W.chunk_blocks = I.chunk_blocks;
  W.prio_fair = 1;  // (always: the resident waves of a SIMD are tasks of different lengths here)
  W.maxdir = L.maxdir;
  const bool MAXDIR = L.maxdir != 0;
  const double* __restrict__ v_next = FUTURE && !KEYED_IN ? values + I.v_next_off : nullptr;
  const unsigned long long* __restrict__ k_next = KEYED_IN ? keys + I.key_next_off : nullptr;
  const double* __restrict__ pmf_p = pmf + I.pmf_off;
  const int hi = I.n_states;

  const int chunk_actions = W.chunk_blocks * R;
  const int span = TS + chunk_actions + W.d_pad + S;  // entries [0, span): slot 0 is a spare; span <= L.span_max
  double2* s_win = reinterpret_cast<double2*>(smem) + (size_t)wave * L.span_max;
  double* s_p = reinterpret_cast<double*>(smem + (size_t)4 * L.span_max * 16) + (size_t)wave * L.p_slots_max;
  const int i0 = tile * TS;
  const int kA = chunk * chunk_actions;

  // stage this wave's window: slot q holds m = m_lo + q
  const int m_lo = i0 + kA - W.d_pad;
  f1_stage_window<FUTURE, KEYED_IN>(W, v_next, k_next, pmf_p, s_win, s_p, span, m_lo, lane);

  double best[S];
  int bestk[S];
  f1_cells<R, S, FUTURE>(W, s_win, s_p, lane, kA, best, bestk);  // (best[u]: state 64*u + lane of the tile)
  const bool chunked = L.chunked != 0;
  double* __restrict__ out_val = chunked ? chunk_val + I.chunk_off + (int64_t)chunk * I.n_states : values + I.v_cur_off;
  int32_t* __restrict__ out_idx = chunked ? chunk_idx + I.chunk_off + (int64_t)chunk * I.n_states : policy + I.pol_off;
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
