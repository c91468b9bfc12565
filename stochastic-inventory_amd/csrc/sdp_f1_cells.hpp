// sdp_f1_cells.hpp -- the state-major cell loop of the backorder family F1 (CLSP.java:251-272): what ONE WAVE does with
// one task, from "LDS region and m_lo known" to "best[u] / bestk[u] hold the results in store order".
//
// window_f1_kernel (sdp_window.hpp: one handle, one period) and window_f1_batch_kernel (sdp_batch.hpp: N instances of one
// grid shape, one period) both call f1_stage_window and f1_cells below; what a kernel keeps for itself is how a task number
// becomes (chunk, tile) or (instance, chunk, tile), where its LDS regions lie and where the results go.  The arithmetic of
// a cell -- its operations, their operands and their order -- exists here and nowhere else, so the tables of a batch
// instance are bit for bit those of a single handle by construction.
//
// Also here, because both units need them: WinParams, the order-preserving keys of chunked periods and FinalizeJob.
#pragma once
#include "sdp_device.hpp"

namespace sdp {

struct WinParams {
  double lev0;   // level value of m = 0: x_lo(cur) - d_0
  double step;
  double h, pi, K, v;
  int32_t idx_off;    // m -> next-grid index offset: (lev0 - x_lo(next)) / step
  int32_t next_last;  // nx(next) - 1
  int32_t n_actions;  // A
  int32_t d_pad;      // demand steps rounded up to a multiple of NW = R + S - 1 (sizes the LDS window)
  int32_t d_main;     // demand steps handled by full blocks of NW: floor(D / NW) * NW
  int32_t n_demand;   // D
  int32_t n_chunks;   // tasks per state tile: the action range is cut into n_chunks runs of R-blocks
  int32_t chunk_blocks;   // R-blocks per task
  int32_t n_tiles;        // state tiles (64 * S states each) covered by THIS launch
  int32_t n_tasks;        // n_tiles * n_chunks (one task per wave)
  int32_t tile_first;     // launch tile u maps to slab tile tile_first + u (+ tile_gap when u >= tile_gap_at):
  int32_t tile_gap_at;    // lets one launch cover the interior run of tiles, or the two boundary runs
  int32_t tile_gap;
  int32_t prio_fair;      // s_setprio by progress: resident waves of a SIMD advance together
  int32_t maxdir;         // OptDirection.MAX
  int32_t pad0;
  int64_t partial_stride; // elements between chunk rows of the partial tables
  int64_t pol_lo, pol_hi; // states whose action index may be stored (all of them when the rows are chunk rows)
  // USER LAMBDAS OF THE LEVEL SHAPE (sdpgpu_create_custom with SDP_SHAPE_LEVEL; nullptr: the built-in CLSP costs above).
  // The driver declared its immediate value as  sdp_action_cost(action) + sdp_level_cost(x + action - demand)  and its
  // transition as the (clamped) level: everything this kernel needs from the lambdas is one number per level m and one per
  // action, tabulated for the period by the user's own compiled functions (sdp_custom_tabulate):
  // M(m) = m_tab[m - m_tab_min], c(a) = c_tab[a].  An index outside a table is a padded cell (probability 0, or a lane
  // beyond the tile): clamped onto the table so that what it multiplies by zero is finite.
  const double* m_tab;
  const double* c_tab;
  int32_t m_tab_min, m_tab_n;
};

// Doubles of a staged copy of the probabilities p_0 .. p_D (the step after the last is requested but not used): an even
// count plus a slot for the staging loop's overshoot.
__host__ __device__ inline int win_p_slots(int n_demand) { return ((n_demand + 3) & ~1) + 2; }

// Order-preserving map double -> uint64 (and back): lets a 64-bit atomic min/max reduce fp64 values
// exactly.  Used for V_t when several tasks share a state tile.
__device__ __forceinline__ unsigned long long f64_key(double v) {
  unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double f64_unkey(unsigned long long k) {
  unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// Deferred read-out for chunked periods (finalize_kernel, sdp_window.hpp): V_t = unkey(K_t); policy = action of the
// lowest chunk whose best value equals V_t.  One launch covers every pending period (jobs sorted by first state).
struct FinalizeJob {
  const unsigned long long* keys;  // indexed by flat state index
  const double* part_val;          // [n_chunks][stride], indexed by flat state index
  const int32_t* part_idx;
  double* v_out;
  int32_t* pol_out;
  int64_t stride;
  int64_t lo, hi;    // states whose policy this job resolves (this rank's slab)
  int64_t vlo, vhi;  // states whose value it decodes (the whole row when sharded)
  int64_t first;     // prefix sum of (vhi - vlo) over earlier jobs
  int32_t n_chunks;
  int32_t pad;
};

// V_{t+1}(clamp m).  CLSP.java:257-258: upper clamp, then lower clamp.  In the unclamped variant every real cell
// is inside the next box by construction; the clamp then only keeps padded (p = 0) demand
// steps, padded actions and tail lanes from reading outside the table.
// In two halves -- the load of the stored word, and its decoding -- for a caller that issues the load long before it uses
// the value (the level kernel's prefetch slot): decoding a key is arithmetic on the loaded word, and would wait for it.
template <bool KEYED_IN>
__device__ __forceinline__ unsigned long long level_v_word(const WinParams& W, const double* __restrict__ v_next,
                                                           const unsigned long long* __restrict__ k_next, int m) {
  int idx = m + W.idx_off;
  idx = idx > W.next_last ? W.next_last : idx;
  idx = idx < 0 ? 0 : idx;
  if constexpr (KEYED_IN)
    return k_next[idx];
  else
    return (unsigned long long)__double_as_longlong(v_next[idx]);
}
template <bool KEYED_IN>
__device__ __forceinline__ double level_v_decode(unsigned long long word) {
  if constexpr (KEYED_IN)
    return f64_unkey(word);
  else
    return __longlong_as_double((long long)word);
}
template <bool KEYED_IN>
__device__ __forceinline__ double level_v(const WinParams& W, const double* __restrict__ v_next,
                                          const unsigned long long* __restrict__ k_next, int m) {
  return level_v_decode<KEYED_IN>(level_v_word<KEYED_IN>(W, v_next, k_next, m));
}

// W[m] for one m: the immediate-cost part that depends on the level, and the future value.
template <bool FUTURE, bool KEYED_IN>
__device__ __forceinline__ double2 window_entry(const WinParams& W, const double* __restrict__ v_next,
                                                const unsigned long long* __restrict__ k_next, int m) {
  double2 e;
  if (W.m_tab) {  // (wave-uniform; staging only: once per window entry, not per cell)
    int i = m - W.m_tab_min;
    i = i < 0 ? 0 : (i >= W.m_tab_n ? W.m_tab_n - 1 : i);
    e.x = W.m_tab[i];
  } else {
    double l = W.lev0 + (double)m * W.step;
    double hold = W.h * jmax(l, 0.0);
    double pen = W.pi * jmax(-l, 0.0);
    e.x = hold + pen;  // one of the two is +-0: c0 + e.x == (c0 + hold) + pen bit for bit
  }
  e.y = 0.0;
  if constexpr (FUTURE) e.y = level_v<KEYED_IN>(W, v_next, k_next, m);
  return e;
}

// Priority by progress -- the further behind, the higher: the SIMD issues by priority, then age, so left alone the
// oldest resident wave runs ahead and the last task of a SIMD ends up alone.  (s_setprio takes an immediate.)
__device__ __forceinline__ void prio_by_progress(unsigned done, unsigned total) {
  const unsigned pr = 3u - (4u * done) / (total + 1u);
  if (pr == 0) __builtin_amdgcn_s_setprio(0);
  else if (pr == 1) __builtin_amdgcn_s_setprio(1);
  else if (pr == 2) __builtin_amdgcn_s_setprio(2);
  else __builtin_amdgcn_s_setprio(3);
}

// Stage the wave's window -- slot q of s_win holds W[m_lo + q], q in [0, span), slot 0 a spare -- and a copy of the
// probabilities in s_p (win_p_slots(D) doubles).  Ends with the wave's writes ordered before its reads: no workgroup
// barrier, a region is read only by waves that wrote every slot of it themselves.
template <bool FUTURE, bool KEYED_IN>
__device__ __forceinline__ void f1_stage_window(const WinParams& W, const double* __restrict__ v_next,
                                                const unsigned long long* __restrict__ k_next,
                                                const double* __restrict__ pmf_p, double2* s_win, double* s_p, int span,
                                                int m_lo, int lane) {
  // (four entries per pass, their loads in flight together: one round trip to L2 per 256 slots instead of four -- on
  // configs[1] the whole window is one pass, and nothing else runs on the SIMD while its two waves stage.  Slots past
  // the span are computed from clamped indices and land in the spare slot 0, which no cell reads: stores without a
  // guard, so that the compiler does not sink a load under its guard and serialise it again.)
  for (int q0 = lane; q0 < span; q0 += 256) {
    double2 e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = window_entry<FUTURE, KEYED_IN>(W, v_next, k_next, m_lo + q0 + 64 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u) s_win[q0 + 64 * u < span ? q0 + 64 * u : 0] = e[u];
  }
  // The probabilities go through LDS as well (one broadcast read per demand step): as scalar loads they shared the
  // wave's lgkm counter with the window reads, and a scalar load in flight turns every wait for an LDS read into a
  // wait for everything -- the slide of f1_cells could not stay in flight across a step.
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
}

// The cells of one task: 64 * S states (lane l owns states S*l .. S*l+S-1 of the tile) x the R-blocks
// kA, kA + R, ... of the task's action run x all demand steps, from the staged window; on return best[u] / bestk[u] are
// the arg-opt of state 64*u + lane of the tile over the task's actions (lowest action index on ties).
//
// S ADJACENT STATES PER LANE.  The cells (state s, action r,
// demand j) and (s+1, r, j+1) have the same m AND the same action, hence the same immediate cost
// c0[r] + M(m) -- the identical fp64 add on identical operands.  It is computed once, for state 0 of the
// lane, and handed down the lane's states one demand step at a time (immc[s][r]); only p_j * imm and the
// two accumulations are per cell.  Operations per cell: (5 + 4*(S-1)) / S = 5, 4.5, 4.25 for S = 1, 2, 4,
// every one of them an operation the reference performs, in its order.  The register window has
// R + S - 1 entries (state s, action r reads entry r + s) and still slides by ONE ds_read_b128 per
// demand step: LDS traffic is 16 + 8 B per R*S cells.
template <int R, int S, bool FUTURE>
__device__ __forceinline__ void f1_cells(const WinParams& W, double2* s_win, const double* s_p, int lane, int kA,
                                         double (&best)[S], int (&bestk)[S]) {
  constexpr int NW = R + S - 1;  // register window entries = demand steps per unrolled block
  constexpr int TS = 64 * S;     // states per tile
  const bool MAXDIR = W.maxdir != 0;
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
      if (W.c_tab)  // (user lambdas of the level shape: the action's own cost, tabulated; a padded action reads the last entry)
        c0[r] = W.c_tab[k0 + r < W.n_actions ? k0 + r : W.n_actions - 1];
      else
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
      // Priority by progress keeps the resident waves of a SIMD level, so they finish together (one wave alone sustains
      // 76 % of the fp64 issue rate, four 94 %: +4 % on configs[1]; nothing to gain on grids with many rounds).  In a
      // batch the resident waves are tasks of different lengths: they advance by the same FRACTION of their work, so
      // a short task does not wait behind a long one's age.
      if (W.prio_fair) prio_by_progress((unsigned)(rb * W.d_main + jb), (unsigned)(W.chunk_blocks * W.d_main));
      const double2* nxt = s_win + (base - jb - NW);  // slots base-jb-NW ... base-jb-1
      const double* pq = s_p + jb + 1;
#pragma unroll
      for (int t = 0; t < NW; ++t) {
        const double p = p_cur;
        // The cell (s = S-1, r = R-1) goes FIRST: it alone reads the window's top entry, so the slide -- the entry for
        // (s = 0, r = 0, j + 1) replaces that one -- is requested at the start of the step and has the rest of the step
        // (60 fp64 instructions) to arrive.  (Left to the scheduler the read sat five instructions before its use; a
        // wave alone on its SIMD then ran at 0.76 of the issue rate.)  Every accumulator still sees its own two adds
        // per step in the reference's order.
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
    // the last D mod NW demand steps: the same cells, in plain order, under wave-uniform guards (the register
    // window is back in its canonical rotation after every full block)
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

  // Results leave through the wave's own LDS region (its window is dead by now) so that every store
  // instruction writes 64 CONSECUTIVE states: lane l owns states S*l .. S*l+S-1, but stores state 64*u + l.
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
}

}  // namespace sdp
