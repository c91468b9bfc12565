// sdp_window.hpp -- LDS-window period kernel for the backorder family F1 (CLSP.java:251-272).
//
// Why a second kernel: in F1 everything a cell needs depends on ONE integer, m = i + k - j
// (state index + action index - demand index):
//     level      l(m) = (x_lo - d_0) + m*step                       (exact integer arithmetic)
//     imm        = (fixed + var)(k) + M(m),   M(m) = h*max(l,0) + pi*max(-l,0)
//     next state = clamp(l(m))  ->  V_{t+1}[clampidx(m)]
// so a workgroup that owns 64 consecutive states and a run of actions touches only a
// contiguous span of 62 + A_chunk + D entries of the pair table W[m] = {M(m), V_{t+1}(clamp m)}.
// The span is staged ONCE in LDS (16 B per entry); HBM/L2 sees each V_{t+1} element once per
// workgroup instead of once per cell.
//
// Thread mapping (wave64): a lane owns S adjacent states and carries R consecutive actions in registers; it
// walks the demand index j = 0..D-1 serially, in the reference's order (Recursion.java:138-144): per cell
//     imm = c0[r] + W.x;  t = p_j*imm;  acc += t;  u = p_j*W.y;  acc += u;
// with separate multiplies and adds (no FMA).  Neighbouring cells repeat some of these operations on the
// very same operands (see f1_cells, sdp_f1_cells.hpp), and those are executed once: 3 + 1/S + (R+S-1)/(RS) operations
// per cell instead of 5.  The register window of R + S - 1 entries slides by ONE new ds_read_b128 per demand
// step: LDS traffic is 16 B per R*S cells, plus 8 B for p_j (wave-uniform: one broadcast read of the workgroup's LDS copy
// per step -- not a scalar load, see the staging code).
// The kernel is bound by fp64 VALU issue (4 cycles per wave64 instruction per SIMD), not by memory.
//
// Small grids (configs[1] has only 79 tiles of 128 states) do not fill 1024 SIMDs with whole-action tasks,
// so the action range of a tile is cut into chunks handled by different waves (see window_f1_kernel).
#pragma once
#include "sdp_f1_cells.hpp"

namespace sdp {

// LDS of a workgroup of window_f1_kernel: one window per wave (span entries of 16 B) and ONE copy of the probabilities
// (win_p_slots doubles).  Every wave writes the whole copy itself (the same values to the same slots as its neighbours)
// and reads it after its own writes have landed: no workgroup barrier, and a one-task-per-tile plan of the 500-action,
// 200-demand grid (R = 4, S = 4: 61.6 KB of windows) still fits the 64 KB a launch may ask for.
__host__ __device__ inline size_t win_wg_lds(int span, int n_demand) { return (size_t)4 * span * 16 + (size_t)win_p_slots(n_demand) * 8; }

// One TASK per wave: (state tile of 64*S, run of R-blocks of the action axis).  Tasks are numbered
// chunk-major (task = chunk * n_tiles + tile) and packed four to a workgroup regardless of tile, so
// every workgroup carries four equal tasks -- one per SIMD -- and a launch of n_tasks/4 workgroups
// loads the 1024 SIMDs evenly (the measured timeline of one SIMD is strictly task after task).  Each
// wave stages its OWN window in its own LDS region: there is no workgroup barrier in this kernel.
//
// What the wave then does with its task -- S adjacent states per lane, R actions in registers, the demand steps walked
// serially -- is f1_stage_window and f1_cells (sdp_f1_cells.hpp), shared with window_f1_batch_kernel.
//
// When a tile is shared by several tasks (n_chunks > 1, small grids) a task publishes its best value
// with a 64-bit atomic min/max on the order-preserving key of V_t (exact), and stores its
// (value, action) pair in its chunk row; the arg-opt ACTION is resolved later, off the critical
// path, by finalize_kernel: the lowest chunk whose value equals V_t holds the lowest optimal action
// index (chunks are ascending action ranges), which is the reference's tie rule.
template <int R, int S, bool FUTURE, bool KEYED_IN>
__global__ __launch_bounds__(256) void window_f1_kernel(WinParams W, const double* __restrict__ v_next,
                                                        const unsigned long long* __restrict__ k_next,
                                                        double* __restrict__ out_val, int32_t* __restrict__ out_idx,
                                                        unsigned long long* __restrict__ k_cur,
                                                        const double* __restrict__ pmf_p, int64_t lo, int64_t hi
#ifdef SDP_STAMPS
                                                        , unsigned long long* stamps
#endif
) {
  constexpr int TS = 64 * S;     // states per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int task = blockIdx.x * 4 + wave;
  if (task >= W.n_tasks) return;  // no barriers below: a wave may leave on its own
  const bool MAXDIR = W.maxdir != 0;
  const int chunk = task / W.n_tiles;
  int tile = task - chunk * W.n_tiles;
  tile = W.tile_first + tile + (tile >= W.tile_gap_at ? W.tile_gap : 0);
  const int chunk_actions = W.chunk_blocks * R;
  const int span = TS + chunk_actions + W.d_pad + S;  // entries [0, span): slot 0 is a spare
  double2* s_win = reinterpret_cast<double2*>(smem) + (size_t)wave * span;
  double* s_p = reinterpret_cast<double*>(smem + (size_t)4 * span * 16);  // (shared: see win_wg_lds)
  const int64_t i0 = lo + (int64_t)tile * TS;
  const int kA = chunk * chunk_actions;
#ifdef SDP_STAMPS  // diagnostic build only (tools/stamp_window.py): per-wave timeline, never in the product
  unsigned long long st_t0 = __builtin_amdgcn_s_memrealtime();
#endif

  // stage this wave's window: slot q holds m = m_lo + q, m_lo = i0 + kA - d_pad
  const int m_lo = (int)i0 + kA - W.d_pad;
  f1_stage_window<FUTURE, KEYED_IN>(W, v_next, k_next, pmf_p, s_win, s_p, span, m_lo, lane);
#ifdef SDP_STAMPS
  unsigned long long st_t1 = __builtin_amdgcn_s_memrealtime();
#endif

  double best[S];
  int bestk[S];
  f1_cells<R, S, FUTURE>(W, s_win, s_p, lane, kA, best, bestk);  // (best[u]: state 64*u + lane of the tile)
#pragma unroll
  for (int u = 0; u < S; ++u) {
    const int64_t idx = i0 + (S > 1 ? 64 * u + lane : lane);
    if (idx < hi) {
      const int64_t o = (int64_t)chunk * W.partial_stride + idx;
      out_val[o] = best[u];
      if (idx >= W.pol_lo && idx < W.pol_hi) out_idx[o] = bestk[u];
      if (W.n_chunks > 1) {
        if (MAXDIR)
          atomicMax(k_cur + idx, f64_key(best[u]));
        else
          atomicMin(k_cur + idx, f64_key(best[u]));
      }
    }
  }
#ifdef SDP_STAMPS
  if (stamps && lane == 0) {
    unsigned long long st_t2 = __builtin_amdgcn_s_memrealtime();
    unsigned hwid = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));  // HW_REG_HW_ID
    unsigned xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11));  // HW_REG_XCC_ID
    unsigned long long* o = stamps + (size_t)task * 5;
    o[0] = st_t0; o[1] = st_t1; o[2] = st_t2; o[3] = hwid; o[4] = xcc;
  }
#endif
}

// ---------------------------------------------------------------------------------------------
// ACTION-MAJOR LEVEL KERNEL for F1 (window_f1_level_kernel).  In window_f1_kernel a lane owns states, and the product
// p_j * V(m) that every (state, action) pair of post-order level y = i + k needs at step j (m = y - j) is formed again by
// every lane and every R-block that meets it.  Here a lane owns ACTIONS k = kb + lane + 64 r (r < R) and walks the levels
// y in blocks of S consecutive levels y0 + s: the cell (lane, r, s) is the pair (state y0 + s - k, action k), and at
// step j its level m = y0 + s - j is the same in all 64 lanes.  So p_j, M(m) and p_j * V(m) are wave-uniform: the wave
// forms the S products of 64 steps lane-parallel (one v_mul_f64 gives 64 of them) into a table in its own LDS region,
// and the step loop reads them back as broadcasts.  The immediate cost c0[k] + M(m) of level s at step j is that of level
// s - 1 at step j - 1 (a ring of S registers per action): R new adds per step.  Operations per cell:
//     p * imm, acc += , acc += p V                3
//     c0 + M, once per (action, m)                R / (R S)
//     p * V, once per (step, m) and wave          S / 64 / (R S)
// each of them an operation the reference performs on the same operands, in its order (j ascending, += p imm then += p V,
// from +0.0).  Padded cells -- actions >= A, levels whose state lies outside the slab, demand steps past D (p = 0) -- read
// clamped, finite table entries.
//
// A task (one wave) is (band of `band` levels, block of 64 R actions).  A state's cells are spread over lanes, over the
// level blocks of the band and, near the band's ends and across action blocks, over tasks:
//   * within a task they meet in a per-state (value, action) slot in LDS, updated after every level block in R S passes;
//     one pass (r, s) touches 64 distinct states, and the passes go s ascending, which for any one state is action
//     ascending -- so a strict < / > keeps the lowest action of a tie, the reference's rule (Recursion.java:146-157);
//   * across tasks through the chunk rows, the key atomics and finalize_kernel: the piece of state i held by task
//     (band b, action block a) goes to chunk row (b - band(i)) + a, band(i) = the band of level i.  Along the action axis
//     of one state both b and a are non-decreasing, so a lower row always holds lower actions; where a band boundary and
//     an action-block boundary fall on the same action, the row skipped in between gets a NaN value, which the finalize
//     never takes.  Rows above a state's last piece are never reached: the value it looks for is in one below.
//
// THE CUT-OFF (CUT; the host turns it on per period, f1_cutoff_on in sdpgpu_window.hip: MIN, the built-in costs, K, v, h,
// pi >= 0, every probability >= 0, V_{t+1} >= 0).  Every addend of a cell is then >= 0, and under round-to-nearest
// a + b >= a for b >= 0: the running sum of a cell never exceeds its final value.  A cell whose running sum is already
// STRICTLY greater than a value some action of the same state has reached can neither win nor tie, and its remaining
// steps change no value, no action index and no tie-break.  So
//   * a state's slot does not start at the reduction identity but at U(i) = Q(i, 0), action 0: the exact value of the
//     state's lowest action, the same operations in the same order (a pre-pass of window_f1_kernel with one action writes
//     the row u_row).  Every piece then reports min(U(i), its own cells) under the strict <, a tie still goes to action 0,
//     and the lowest chunk row whose value equals V_t still carries the lowest optimal action: chunk rows, key atomics and
//     finalize_kernel are untouched;
//   * every S steps from a scheduled step on (where the imm ring is in its canonical rotation) the wave tests its R S
//     cells against their slots -- R S per-lane LDS reads and compares, about 0.7 of a step -- and when every real
//     cell other than action 0 itself is beaten (one ballot, a scalar branch) it drops the rest of the level block and its
//     epilogue.  A NaN compares false: such a block runs in full.
// A stopped block skips (d_pad - stop) of its d_pad steps: 3 + 1/S + 1/(64 R) operations per cell and step, as above, over
// the steps that ran (counted per wave into cut_count[0], the tests into cut_count[1]) plus one compare per cell and test.
// With CUT off the kernel is the one above, instruction for instruction.
//
// THE SCREEN (CUT only; LevelParams::screen_start, a multiple of S, 0 = off; the host: f1_screen_start / f1_screen_on in
// sdpgpu_window.hip).  The steps in front of the pmf's mass prove nothing about a block that loses; they are walked only
// because a winner's value is summed from step 0.  Under the cut-off's gate every addend is >= 0, round-to-nearest addition
// is monotone in both operands and fl(x + 0) = x: replace any addends of a cell by +0.0, in the reference's order, and by
// induction over the steps the sum is <= the cell's fp64 value.  So the sum over the steps j >= screen_start alone, in
// order from +0.0, is a lower bound of Q(i, k), and a cell whose bound is STRICTLY greater than its slot can neither win
// nor tie -- the cut-off's own condition.  A level block is therefore either exact (walked from step 0, as above) or
// SCREENED: the imm ring set up for step screen_start (its canonical rotation), the sums from +0.0, the product tables
// from j0 = screen_start (tables and prefetch tags at screen_start + n DB), the tests on their schedule but not before
// screen_start + S.  A screened block that stops is done, like any stopped block.  One that reaches d_pad has learned
// nothing: the block is walked again as an exact block, by a second turn of the loop around the table loop (there is one
// step loop).  A NaN sum compares false, so such a block fails its screen and is walked exactly.
//   The mode (wave-uniform, scalar registers): a task's first block is exact; a block is screened only while the task's
// last `need` blocks all stopped, in either mode; a failed screen doubles `need` (up to 8) and starts the count again
// (the exact walk of the same block counts if it stops), a screen that stopped sets it back to 1.  Where nothing ever
// stops, no block is screened and the steps are the cut-off's; a run of stopped blocks pays for few failed screens.
//   The prefetch guess for the next block's first table starts at the step that block is expected to start at.
//   cut_count[0] counts the steps walked (a failed screen: its own and the exact walk's), cut_count[2..4] the blocks
// screened and stopped, the screens that failed and the exact walks, cut_count[5] the steps walked in screened passes
// (stopped or failed; part of cut_count[0]).
//   The host screens where the planner chose this kernel by itself.  Under a forced plan (SDPGPU_WIN_LEVEL=1) it does so
// only with SDPGPU_F1_SCREEN=1: screen_start is 0 there otherwise and the kernel walks the cut-off's schedule step for
// step, which the device tests of the cut-off count against a CPU twin.  SDPGPU_F1_SCREEN=0 turns it off everywhere.
//
// THE SCREEN ROWS (RS, a divisor of R; the host: SDPGPU_F1_SCREEN_ROWS / kF1ScreenRows, sdpgpu_internal.hpp).  A screened
// pass proves "beaten" and nothing else, and it does not need all R action rows of a lane for that.  At step j every cell
// of level y0 + s has the same m = y0 + s - j whatever its action: for one lane and one level the R cells differ in ONE
// operand, c0[r].  Under the cut-off's gate c0[k] = (a > 0 ? K : 0) + v a with K, v >= 0 and a = k step, step > 0, is
// non-decreasing in k (fl(v a) and fl(K + .) are monotone), and fl(c0 + M), fl(p x) for p >= 0 and fl(acc + x) are monotone in
// each operand under round-to-nearest: by induction over the steps, in the reference's order, acc[r'][s] >= acc[r][s]
// whenever r' >= r -- termwise, in fp64 as executed, no error analysis.  So the sum of row r, started at the same step, is
// a lower bound of the sums of the rows above it as well, and cell (r', s) is beaten as soon as a LOWER row's sum is strictly
// greater than cell (r', s)'s OWN threshold.  (Against the lower row's threshold alone it would be wrong: in the ordering
// region the states of the higher rows, 64 below, have far higher thresholds.)  The gate suffices because it already excludes
// what would break the order of c0: a c_tab (user tables of the level shape) and custom costs; MAX; negative K or v.
//   A screened pass of an RS < R instantiation therefore walks RS screen rows: row q stands for rows q G .. (q + 1) G - 1
// (G = R / RS) and carries the c0 of the lowest live action among them (c0s: the base row; lane 0 of action block 0 skips
// action 0; a lane whose base row is a padded action has nothing live in the group).  Ring set-up, step loop and the imm
// hand-over run over RS rows -- the pass is ONE text, sdp_window_level_pass.hpp, included for R and for RS rows: the same
// operations on the same operands in the same order -- and the test reads the R thresholds of a level as before, compares
// each covered row's threshold with its screen row's sum and ANDs without a short cut (a NaN compares false and fails the
// screen).  Where the thresholds U(i) do not fall with the state over the block -- everywhere but the ordering region near
// level 0 -- that is the test of the row group's hardest cell and stops at the same step.  A screen that fails is walked
// again exactly with all R rows; the exact pass, the epilogue, the product table, the prefetch slot, the test schedule, the
// mode rule and stop_at know nothing of RS, and no table can change.  With RS = R the kernel is the one before, instruction
// for instruction.  A screened step costs RS S 3 + RS fp64 operations per lane (period T: RS S 2 + RS) instead of
// R S 3 + R: sdpgpu_stats prices cut_count[5] steps so (f1_level_ops_per_cell).
//
// THE STEP GROUPS (SG; the host: SDPGPU_F1_STEP_GROUP / kF1StepGroup, sdpgpu_internal.hpp).  A cell's step is three fp64
// instructions, each waiting on the one before: t = p imm, t' = acc + t, acc = t' + p V.  Written cell after cell, two of
// every three instructions of a collapsed pass follow their own operand directly, and a wave that runs alone on its SIMD --
// while the other builds a table, tests or waits for LDS -- issues at the rate of that chain.  With SG > 1 a step takes its
// RW S cells (level-major: the rows of a level together) in groups of SG: the group's SG products, then its SG `acc +=`,
// then its SG `+= p V`, fenced so that the order holds; dependent instructions are SG apart.  Per cell these are the same
// operations on the same operands in the same order, and no sum meets another before the test or the epilogue: tables,
// counters, tests and stop steps know nothing of SG.  With SG = 1 the kernel is the one before, instruction for instruction.
// ---------------------------------------------------------------------------------------------
struct LevelParams {
  int32_t band;       // levels per task (a multiple of S)
  int32_t n_ablocks;  // action blocks of 64 R
  int32_t n_tasks;    // bands x action blocks; task = band * n_ablocks + block
  int32_t d_pad;      // demand steps rounded up to S; the padded steps carry p = 0
  int32_t lo;         // first state of the slab = first level (state lo, action 0)
  int32_t n_states;   // hi - lo
  int32_t y_hi;       // one past the last level: hi + A - 1
  int32_t n_chunks;   // chunk rows: ceil((A - 1) / band) + n_ablocks
  int32_t cut_start;  // CUT: the step of a task's first cut-off test (a multiple of S, >= S)
  int32_t screen_start;  // CUT: the step a screened level block starts at (a multiple of S; 0: no block is screened)
  int32_t form;       // THE LAUNCH FORMS: 0 = four tasks per workgroup, 1 = one wave per workgroup, 2 = waves claim tasks
};

template <int S>
struct LevelShape {
  static constexpr int DB = (64 / S) * S;  // demand steps per product table (a whole number of S-step rotations)
  static constexpr int ROW = S + 2;        // doubles per table row: p_j, M(y0 - j - 1), p_j * V(y0 + s - j) for s < S
};
// LDS of one wave: its product table, then (band + 64 R) slots of {value, action}
__host__ __device__ inline size_t level_wave_lds(int band, int R, int S) {
  const int db = (64 / S) * S;
  return (((size_t)db * (S + 2) * 8 + (size_t)(band + 64 * R) * 12) + 15) & ~(size_t)15;
}
__host__ __device__ inline int level_chunks(int n_actions, int band, int n_ablocks) {
  return (n_actions - 1 + band - 1) / band + n_ablocks;
}

// THE LAUNCH FORMS (LevelParams::form; the host: SDPGPU_F1_LEVEL_FORM / kF1LevelForm, sdpgpu_internal.hpp).  The waves of a
// workgroup are independent tasks -- there is no workgroup barrier -- but a workgroup gives its LDS and its wave slots back
// only when its slowest wave ends, and tasks differ in length (the cut-off stops the blocks of high bands later).  Which
// wave runs which task, and when, is all that a form decides:
//   0  four tasks per 256-thread workgroup, task = blockIdx.x * 4 + wave, in index order;
//   1  the same instantiation launched with ONE wave per workgroup (64 threads, level_wave_lds bytes, n_tasks workgroups): a
//      slot and its LDS are free the moment the wave ends;
//   2  resident waves that claim tasks (CLAIM): each wave, on its own, takes the next index from the word `claim` (lane 0,
//      one vector atomic; zeroed on the stream before the launch), runs that task in its own LDS region and leaves when the
//      index reaches n_tasks.  No wave waits for another, and nothing depends on how many workgroups are resident: one that
//      starts late finds the queue empty.  Everything a task keeps -- slot fill, prefetch slot, c0, test schedule, the
//      screen's mode rule, the tallies -- is set up again for every task, as at kernel entry.
// Forms 1 and 2 take the longest tasks first: band 0, then from the last band down (index c, q = c / n_ablocks: band 0 for
// q = 0, else band n_bands - q; action block c % n_ablocks).  The cut-off stops the blocks of higher bands later, so length
// grows with the band -- except band 0, the ordering region near level 0, where screens fail and blocks are walked exactly:
// its first action block is the longest task of a launch by half (profiles/f1_level_forms_ab.txt, the timeline).  No result
// can see the order or the form: chunk rows are per (task, state), the NaN row goes where no other task writes, key and
// counter atomics commute, and the counters are added per task.
//   Forms 0 and 1 are one instantiation (CLAIM = false: the form is a wave-uniform field, the loop below is left after one
// turn) with the registers of the kernel that knew no forms; the claim loop is an instantiation of its own, because as a
// run-time branch it costs every instantiation registers and the period-T ones their third wave per SIMD
// (profiles/f1_level_forms_resources.txt).
__device__ __forceinline__ int level_task_of(const LevelParams& L, int c) {
  const int q = c / L.n_ablocks;  // 0: band 0; q >= 1: band n_bands - q
  return q == 0 ? c : L.n_tasks - L.n_ablocks * q + c % L.n_ablocks;
}

template <int R, int S, bool FUTURE, bool KEYED_IN, bool CUT, int RS = R, int SG = 1, bool CLAIM = false>
__global__ __launch_bounds__(256) void window_f1_level_kernel(WinParams W, LevelParams L, const double* __restrict__ v_next,
                                                              const unsigned long long* __restrict__ k_next,
                                                              double* __restrict__ out_val, int32_t* __restrict__ out_idx,
                                                              unsigned long long* __restrict__ k_cur,
                                                              const double* __restrict__ pmf_p,
                                                              const double* __restrict__ u_row,
                                                              unsigned long long* __restrict__ cut_count,
                                                              unsigned* __restrict__ claim) {
  constexpr int DB = LevelShape<S>::DB, ROW = LevelShape<S>::ROW, NA = 64 * R;
  static_assert(RS >= 1 && R % RS == 0 && (CUT || RS == R), "screen rows divide R; only the cut-off screens");
  static_assert(SG >= 1 && (RS * S) % SG == 0, "a step's cells, RW S of them in either pass, fall into whole groups of SG");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (;;) {  // (CLAIM: one turn per task claimed; else one turn)
    int task;
    if constexpr (CLAIM) {
      unsigned got = 0;
      if (lane == 0) got = atomicAdd(claim, 1u);
      got = __builtin_amdgcn_readfirstlane(got);
      if (got >= (unsigned)L.n_tasks) return;
      task = level_task_of(L, (int)got);
    } else {
      // (the workgroup's own wave count: 4, or 1 in form 1)
      task = (int)(blockIdx.x * (blockDim.x >> 6)) + wave;
      if (task >= L.n_tasks) return;  // no workgroup barrier below
      if (L.form != 0) task = level_task_of(L, task);
    }
    const bool MAXDIR = W.maxdir != 0;
    const double ident = MAXDIR ? -1.7976931348623157e308 : 1.7976931348623157e308;
    const int ab = task % L.n_ablocks;
    const int b = task / L.n_ablocks;
    const int kb = ab * NA;
    const int yb = L.lo + b * L.band;
    const int ye = min(yb + L.band, L.y_hi);
    const int i_min = yb - kb - NA + 1;  // slot q holds state i_min + q; states i_min .. ye - 1 - kb
    const int n_slot = ye - yb + NA - 1;
    char* mine = smem + (size_t)wave * level_wave_lds(L.band, R, S);
    double* s_row = reinterpret_cast<double*>(mine);
    double* s_val = s_row + DB * ROW;
    int* s_idx = reinterpret_cast<int*>(s_val + L.band + NA);
    // THE PREFETCH SLOT: what the build of ONE table reads from memory, loaded while the table before it is walked.  The
    // table of block y and steps j .. j + DB - 1 needs V(clamp(y + s - j')) for s < S and DB steps j': the DB + S - 1
    // consecutive entries w[q] = V(clamp(y - j - (DB - 1) + q)), of which row t, level s takes w[DB - 1 - t + s].  Lane t holds
    // w[t] and w[64 + t] (as stored: a key is decoded where it is used, so that nothing waits for the load here) and its
    // row's p_j; the tag (pf_y, pf_j) says whose they are.  A table whose tag does not match is built from direct loads.
    // Period T (no future term) has only p_j to fetch, and holding it costs its CUT instantiation the third wave per SIMD
    // (166 -> 189 VGPRs): it stays as it was.
    constexpr bool PF = FUTURE;
    static_assert(DB + S - 1 > 64 && DB + S - 1 <= 128, "two window entries per lane");
    [[maybe_unused]] unsigned long long pf_w0 = 0, pf_w1 = 0;
    [[maybe_unused]] double pf_p = 0.0;
    [[maybe_unused]] int pf_y = INT32_MIN, pf_j = 0;
    [[maybe_unused]] int pf_stop = INT32_MAX;  // CUT: the step the block before stopped at (a guess at where this one will)
    [[maybe_unused]] auto prefetch = [&](int y, int j) {
      const int m = y - j - (DB - 1);
      pf_p = pmf_p[j + min(lane, min(DB, L.d_pad - j) - 1)];
      pf_w0 = level_v_word<KEYED_IN>(W, v_next, k_next, m + lane);
      pf_w1 = level_v_word<KEYED_IN>(W, v_next, k_next, m + 64 + min(lane, DB + S - 2 - 64));
      pf_y = y;
      pf_j = j;
    };
    if constexpr (PF) prefetch(yb, 0);  // (the slot fill below covers it)
    if constexpr (CUT) {
      // every slot starts at U(i) = Q(i, 0) with action 0 (see THE CUT-OFF above); a slot of no state of the slab -- the
      // ends of the range, and the slots past n_slot that the last, ragged band's level blocks still address -- at a value
      // every sum exceeds, so that it never holds a block back (it is never written out)
      for (int q = lane; q < L.band + NA; q += 64) {
        const int i = i_min + q;
        const bool in = i >= L.lo && i - L.lo < L.n_states;
        s_val[q] = in ? u_row[i] : -__builtin_huge_val();
        s_idx[q] = 0;
      }
    } else {
      for (int q = lane; q < n_slot; q += 64) {
        s_val[q] = ident;
        s_idx[q] = 0;
      }
    }
    double c0[R];
    bool kreal[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = kb + lane + 64 * r;
      kreal[r] = k < W.n_actions;
      const double a = (double)k * W.step;
      if (W.c_tab)  // (a padded action reads the last entry: finite, never selected)
        c0[r] = W.c_tab[k < W.n_actions ? k : W.n_actions - 1];
      else
        c0[r] = (a > 0 ? W.K : 0.0) + W.v * a;
    }
    // SCREEN ROWS: screen row q carries the c0 of the lowest live action of rows q G .. (q + 1) G - 1 -- its base row, except
    // that lane 0 of action block 0 skips action 0 (a group whose base row is padded has nothing live: any finite c0 will do)
    [[maybe_unused]] double c0s[RS];
    if constexpr (RS < R) {
#pragma unroll
      for (int q = 0; q < RS; ++q) c0s[q] = q == 0 && kb + lane == 0 ? c0[1] : c0[q * (R / RS)];
    }
    // CUT: the test schedule (wave-uniform, scalar registers).  A block's first test comes `dec` steps before the step its
    // predecessor stopped at, then one every S steps; a block that passes its first test moves the next block's twice as
    // far down, and after a block that ran to the end the next one is tested once, S steps before the end (a sum only grows,
    // so a block that could have stopped earlier still passes there): where nothing ever stops, one test per block.
    [[maybe_unused]] int cut_first = L.cut_start, cut_dec = S, cut_once = 0;
    [[maybe_unused]] unsigned cut_steps = 0, cut_tests = 0;
    // CUT: the screen's mode rule (wave-uniform, scalar registers; THE SCREEN above).  scr_run counts the stopped blocks since
    // the last one that ran to the end or failed its screen; a block is screened when scr_run >= scr_need.
    [[maybe_unused]] int scr_run = 0, scr_need = 1;
    [[maybe_unused]] unsigned scr_hit = 0, scr_miss = 0, scr_exact = 0, scr_steps = 0;

    for (int y0 = yb; y0 < ye; y0 += S) {
      // Priority by progress, as in f1_cells: the four waves of a workgroup free its LDS only together, and a plan
      // of two rounds of equal tasks loses a tenth of the issue rate when the resident waves of a SIMD drift apart by age
      // (the one left behind then runs alone, at 0.6 of the rate, while the slot of the finished one stays empty).
      if (W.prio_fair) prio_by_progress((unsigned)(y0 - yb), (unsigned)(ye - yb));
      double acc[R][S];
      [[maybe_unused]] int cut_fail = 0;
      int stop_at = -1;  // CUT: the step the block stopped at
      // CUT: the step this pass over the block starts at -- L.screen_start for a screened block, 0 for an exact one (and for
      // the second pass over a block whose screen failed)
      [[maybe_unused]] int scr_from = 0;
      if constexpr (CUT) scr_from = scr_run >= scr_need ? L.screen_start : 0;
      [[maybe_unused]] bool again = false;
      // ONE PASS over the block from step j_first is the text of sdp_window_level_pass.hpp.  A collapsed instantiation (RS < R)
      // walks a screened pass here, over the RS screen rows, and leaves the loop below to the exact walks: the screen stopped
      // the block (done), or it failed and the block is walked from step 0.  (In front of the loop and not a branch inside it:
      // there the R S sums of the exact walk stay live through the screened pass, 279 VGPRs and one wave per SIMD.)
      if constexpr (RS < R) {
        if (scr_from > 0) {
          const int j_first = scr_from;
          double acs[RS][S];
#define SDP_LEVEL_PASS_ROWS RS
#define SDP_LEVEL_PASS_C0 c0s
#define SDP_LEVEL_PASS_ACC acs
#include "sdp_window_level_pass.hpp"
#undef SDP_LEVEL_PASS_ROWS
#undef SDP_LEVEL_PASS_C0
#undef SDP_LEVEL_PASS_ACC
          const unsigned walked = (unsigned)((stop_at < 0 ? L.d_pad : stop_at) - j_first);
          cut_steps += walked;
          scr_steps += walked;
          if (stop_at >= 0) {
            ++scr_hit;
            scr_need = 1;
          } else {  // the screen has failed, as below
            ++scr_miss;
            scr_need = min(2 * scr_need, 8);
            scr_run = 0;
            scr_from = 0;
          }
        }
      }
      if (RS == R || stop_at < 0) do {
        const int j_first = CUT ? scr_from : 0;
#define SDP_LEVEL_PASS_ROWS R
#define SDP_LEVEL_PASS_C0 c0
#define SDP_LEVEL_PASS_ACC acc
#include "sdp_window_level_pass.hpp"
#undef SDP_LEVEL_PASS_ROWS
#undef SDP_LEVEL_PASS_C0
#undef SDP_LEVEL_PASS_ACC
        if constexpr (CUT) {
          again = false;
          cut_steps += (unsigned)((stop_at < 0 ? L.d_pad : stop_at) - j_first);
          if (j_first > 0) scr_steps += (unsigned)((stop_at < 0 ? L.d_pad : stop_at) - j_first);  // (RS = R: screened here)
          if (j_first == 0) {
            ++scr_exact;
          } else if (stop_at >= 0) {
            ++scr_hit;
            scr_need = 1;
          } else {  // the screen has failed: nothing is known about the block, walk it again from step 0
            ++scr_miss;
            scr_need = min(2 * scr_need, 8);
            scr_run = 0;
            scr_from = 0;
            again = true;
          }
        }
      } while (CUT && again);
      if constexpr (CUT) {
        scr_run = stop_at >= 0 ? scr_run + 1 : 0;
        if constexpr (PF) pf_stop = stop_at < 0 ? INT32_MAX : stop_at;
        if (stop_at >= 0) {  // no cell of the block can win or tie: nothing to put into the slots
          cut_dec = cut_fail == 0 ? min(2 * cut_dec, 8 * S) : S;
          cut_first = max(S, stop_at - cut_dec);
          cut_once = 0;
          continue;
        }
        cut_first = max(S, L.d_pad - S);
        cut_dec = S;
        cut_once = 1;
      }
      // into the per-state slots: cell (r, s) is state y0 + s - k, slot (y0 - yb) + s - lane - 64 r + NA - 1
      const int sb = (y0 - yb) - lane + NA - 1;
      const int ib = y0 - kb - lane - L.lo;  // state - lo of cell (0, 0)
#pragma unroll
      for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int rel = ib + s - 64 * r;
          if (kreal[r] && rel >= 0 && rel < L.n_states) {
            const int q = sb + s - 64 * r;
            const double cur = s_val[q];
            if (MAXDIR ? (acc[r][s] > cur) : (acc[r][s] < cur)) {
              s_val[q] = acc[r][s];
              s_idx[q] = kb + lane + 64 * r;
            }
          }
        }
      }
    }

    // every state of the task's range that has a real action here: its piece, in chunk row (b - band(i)) + ab
    __builtin_amdgcn_wave_barrier();
    for (int q = lane; q < n_slot; q += 64) {
      const int i = i_min + q;
      const int rel = i - L.lo;
      if (rel < 0 || rel >= L.n_states) continue;
      const int kf = max(kb, yb - i);  // lowest action of the piece
      if (kf >= W.n_actions) continue;
      const int c = (b - rel / L.band) + ab;
      const double v = s_val[q];
      const int64_t o = (int64_t)c * W.partial_stride + i;
      out_val[o] = v;
      out_idx[o] = s_idx[q];
      if (kb > 0 && yb - i == kb) {  // both boundaries at action kf: row c - 1 holds no piece of this state
        out_val[o - W.partial_stride] = __builtin_nan("");
        out_idx[o - W.partial_stride] = 0;
      }
      if (MAXDIR)
        atomicMax(k_cur + i, f64_key(v));
      else
        atomicMin(k_cur + i, f64_key(v));
    }
    if constexpr (CUT) {  // what ran, for sdpgpu_stats: demand steps of level blocks, and cut-off tests
      if (lane == 0) {
        atomicAdd(cut_count, (unsigned long long)cut_steps);
        atomicAdd(cut_count + 1, (unsigned long long)cut_tests);
        if (L.screen_start > 0) {
          atomicAdd(cut_count + 2, (unsigned long long)scr_hit);
          atomicAdd(cut_count + 3, (unsigned long long)scr_miss);
          atomicAdd(cut_count + 5, (unsigned long long)scr_steps);
        }
        atomicAdd(cut_count + 4, (unsigned long long)scr_exact);
      }
    }
    if constexpr (!CLAIM) return;
    __builtin_amdgcn_wave_barrier();  // (the next task's slot fill stays behind this task's read-out)
  }
}

// Fill the key rows with the reduction identity (+-Double.MAX_VALUE, the `val` initialiser of
// Recursion.java:132-133).
__global__ __launch_bounds__(256) void key_fill_kernel(unsigned long long* __restrict__ keys, int64_t n, int maxdir) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = f64_key(maxdir ? -1.7976931348623157e308 : 1.7976931348623157e308);
}

// Deferred read-out for chunked periods (FinalizeJob, sdp_f1_cells.hpp): V_t = unkey(K_t); policy = action of the lowest
// chunk whose best value equals V_t.  One launch covers every pending period (jobs sorted by first state).
__global__ __launch_bounds__(256) void finalize_kernel(const FinalizeJob* __restrict__ jobs, int n_jobs, int64_t total) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  int a = 0, b = n_jobs - 1;
  while (a < b) {  // last job with first <= g
    int mid = (a + b + 1) >> 1;
    if (jobs[mid].first <= g) a = mid; else b = mid - 1;
  }
  const FinalizeJob& J = jobs[a];
  const int64_t idx = J.vlo + (g - J.first);
  const double v = f64_unkey(J.keys[idx]);
  J.v_out[idx] = v;
  if (idx < J.lo || idx >= J.hi) return;
  int k = 0;
  for (int c = 0; c < J.n_chunks; ++c) {
    if (J.part_val[(int64_t)c * J.stride + idx] == v) {
      k = J.part_idx[(int64_t)c * J.stride + idx];
      break;
    }
  }
  J.pol_out[idx] = k;
}

// ---------------------------------------------------------------------------------------------
// F2 (Leadtime.java:50-81): state (x, preQ), level l = x + preQ - d does not depend on the action;
// the action only selects the PLANE of V_{t+1} (next preQ = action) and the ordering cost:
//     imm = (fixed + var)(k) + M(m),  next = V_{t+1}[k][clamp(m)],   m = ix + iq - j.
// A workgroup owns 64 consecutive x of one preQ row and a chunk of actions; it stages M(m) and,
// per action of the chunk, the row segment V_{t+1}[k][clamp(m)] of 64 + D entries in LDS.  A lane
// (= state) carries R actions in registers; per demand step it reads M once and one V entry per
// action (ds_read_b64, consecutive lanes -> conflict-free).  Same five fp64 ops per cell.
// ---------------------------------------------------------------------------------------------
struct RowParams {
  double lev0;  // level of m = 0: x_lo(cur) - d_0   (preQ enters through m)
  double step;
  double h, pi, K, v;
  int32_t idx_off;      // m -> next-grid inventory index offset
  int32_t next_last;    // nx(next) - 1
  int32_t next_nx;      // nx(next): plane stride of V_{t+1}
  int32_t cur_nx;       // nx(cur)
  int32_t tiles_per_row;
  int32_t n_actions;
  int32_t d_pad;
  int32_t n_chunks;
  int32_t chunk_actions;
  int32_t waves_active; // waves of a workgroup that take action blocks (4 unless the LDS budget for 4 x R row segments says fewer)
  int32_t n_tiles;      // tiles launched (a contiguous run of row tiles)
  int32_t tile0;        // first tile of the run (tile = iq * tiles_per_row + ix / 64)
  int32_t nq1;          // inner pipeline axis: iq = iq2 * nq1 + iq1 (lead time 1: nq1 = nq, iq2 = 0)
  int64_t plane_stride; // V_{t+1} elements between the planes of consecutive actions: nx(next), or nq1 * nx(next)
                        // with lead time 2, where the plane of action k is row (k * nq1 + iq2)
  int64_t partial_stride;
};

// S ADJACENT STATES PER LANE, as in the F1 kernel: the cell (state s+1, action r, demand j+1) has the level AND
// the plane of (s, r, j), i.e. the same immediate cost c0[r] + M(m) and the same V_{t+1} entry.  Both are
// formed / read once, for state 0 of the lane, and reused by state s at step j + s (a ring of S register
// sets, the demand loop unrolled by S so that the ring needs no moves): 4 + 1/S fp64 operations and
// 8(R+1)/(R S) B of LDS per cell.
#ifndef SDP_F2_WAVES_ATTR
#define SDP_F2_WAVES_ATTR
#endif
template <int R, int S, bool MAXDIR, bool FUTURE>
__global__ __launch_bounds__(256) SDP_F2_WAVES_ATTR void window_f2_kernel(RowParams W, const double* __restrict__ v_next,
                                                        double* __restrict__ out_val, int32_t* __restrict__ out_idx,
                                                        const double* __restrict__ pmf_p, int64_t lo, int64_t hi) {
  constexpr int TS = 64 * S;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int span = TS + W.d_pad + 2;                   // slots per row segment (slots 0, 1 spare; even: rows stay 16-byte aligned)
  double* s_m = reinterpret_cast<double*>(smem);       // M(m)
  double* s_v = s_m + span;                            // [waves_active][R][span]: every wave stages the rows of its own block
  // read-out scratch of wave w ({best value, best action} of its TS states): inside the wave's own row region, which it has
  // finished reading by then (R rows of span doubles >= 12 TS bytes for every R >= 2); waves without a region get one behind
  char* s_extra = reinterpret_cast<char*>(s_v + (size_t)(FUTURE ? W.waves_active * R : 0) * span);
  auto scratch = [&](int w) -> char* {
    if (FUTURE && w < W.waves_active) return reinterpret_cast<char*>(s_v + (size_t)(w * R) * span);
    return s_extra + (size_t)(w - (FUTURE ? W.waves_active : 0)) * (TS * 12);
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int chunk = blockIdx.x / W.n_tiles;
  const int tile = W.tile0 + (blockIdx.x - chunk * W.n_tiles);
  const int iq = tile / W.tiles_per_row;
  const int ix0 = (tile - iq * W.tiles_per_row) * TS;
  const int kA = chunk * W.chunk_actions;
  const int iq2 = iq / W.nq1;
  const int iq1 = iq - iq2 * W.nq1;     // the quantity arriving this period
  const int m_lo = ix0 + iq1 - W.d_pad - 1;  // slot q <-> m = m_lo + q
  const int64_t row_off = (int64_t)iq2 * W.next_nx;

  for (int q = tid; q < span; q += 256) {
    double l = W.lev0 + (double)(m_lo + q) * W.step;
    s_m[q] = W.h * jmax(l, 0.0) + W.pi * jmax(-l, 0.0);
  }
  __syncthreads();  // the only workgroup barrier before the read-out: the V rows below are wave-private

  double best[S];
  int bestk[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    best[s] = MAXDIR ? -1.7976931348623157e308 : 1.7976931348623157e308;
    bestk[s] = 0;
  }
  const int blocks_in_chunk = W.chunk_actions / R;
  // slot of (lane, s, j): base + s - j.  With S >= 2 the slots of two consecutive steps (base - j - 1, base - j), j even, start on an
  // even slot: ONE 16-byte read per row and two steps, consecutive lanes reading consecutive 16-byte pieces -- no bank conflicts
  // (an 8-byte read with the lanes 8 S bytes apart is 2- or 4-way conflicted, and the LDS pipe was 84 % busy with those).
  const int base = S * lane + W.d_pad + 1;
  double* my_rows = s_v + (size_t)(wave * R) * span;
  for (int rb = wave; rb < blocks_in_chunk && wave < W.waves_active; rb += W.waves_active) {
    const int k0 = kA + rb * R;
    if (k0 >= W.n_actions) break;
    if constexpr (FUTURE) {
      // the block's R row segments V_{t+1}[plane(k0 + r)][clamp(m)], m = m_lo + q: one scalar base per row, R loads in
      // flight per pass over q (the wave does not wait for the other waves of the workgroup, nor they for it)
      __builtin_amdgcn_wave_barrier();
      const double* src[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        int k = k0 + r;
        k = k < W.n_actions ? k : W.n_actions - 1;  // padded actions read a valid plane, never selected
        src[r] = v_next + ((int64_t)k * W.plane_stride + row_off);
      }
      // (three passes over q per trip: 3 R loads in flight, two round trips to L2 for the 358 slots of S = 4 instead of six;
      // slots past the span land in the spare slot 0 -- stores without a guard, see window_f1_kernel)
      for (int q0 = lane; q0 < span; q0 += 192) {
        double tmp[3][R];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          int idx = m_lo + q0 + 64 * u + W.idx_off;
          idx = idx > W.next_last ? W.next_last : idx;
          idx = idx < 0 ? 0 : idx;
#pragma unroll
          for (int r = 0; r < R; ++r) tmp[u][r] = src[r][idx];
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const int slot = q0 + 64 * u < span ? q0 + 64 * u : 0;
#pragma unroll
          for (int r = 0; r < R; ++r) my_rows[r * span + slot] = tmp[u][r];
        }
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the wave's own LDS writes have landed
    }
    double c0[R], acc[S][R];
    // ring[u][r]: {imm, V} of state 0 at the step j with j mod S == u; state s at step j uses ring[(j - s) mod S]
    double ring_i[S][R], ring_v[S][R];
    const double* rows = my_rows + base;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double a = (double)(k0 + r) * W.step;
      c0[r] = (a > 0 ? W.K : 0.0) + W.v * a;
#pragma unroll
      for (int s = 0; s < S; ++s) acc[s][r] = 0.0;
      // what state s needs at step 0 is "state 0 at step -s": the entry at slot base + s
#pragma unroll
      for (int s = 1; s < S; ++s) {
        ring_i[(S - s) % S][r] = c0[r] + s_m[base + s];
        ring_v[(S - s) % S][r] = FUTURE ? rows[r * span + s] : 0.0;
      }
    }
    // (four demand steps per trip -- d_pad is a multiple of 4, S divides 4 -- so that the loop control and the
    // LDS address updates are paid once per four steps)
    for (int jb = 0; jb < W.d_pad; jb += 4) {
      if constexpr (S >= 2) {
#pragma unroll
        for (int t2 = 0; t2 < 4; t2 += 2) {
          const int j = jb + t2;
          const double2 mm = *reinterpret_cast<const double2*>(s_m + base - j - 1);  // {M of step j + 1, M of step j}
          double2 vv[R];
          if constexpr (FUTURE) {
#pragma unroll
            for (int r = 0; r < R; ++r) vv[r] = *reinterpret_cast<const double2*>(rows + r * span - j - 1);
          }
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) {
            const int u = (t2 + tt) % S;
            const double p = pmf_p[j + tt];
            const double mj = tt ? mm.x : mm.y;
#pragma unroll
            for (int r = 0; r < R; ++r) {
              ring_i[u][r] = c0[r] + mj;
              if constexpr (FUTURE) ring_v[u][r] = tt ? vv[r].x : vv[r].y;
#pragma unroll
              for (int s = 0; s < S; ++s) {
                acc[s][r] += p * ring_i[(u - s + S) % S][r];
                if constexpr (FUTURE) acc[s][r] += p * ring_v[(u - s + S) % S][r];
              }
            }
          }
        }
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int u = t % S;
          const int j = jb + t;
          const double p = pmf_p[j];
          const double mj = s_m[base - j];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            ring_i[u][r] = c0[r] + mj;
            if constexpr (FUTURE) ring_v[u][r] = rows[r * span - j];
#pragma unroll
            for (int s = 0; s < S; ++s) {
              acc[s][r] += p * ring_i[(u - s + S) % S][r];
              if constexpr (FUTURE) acc[s][r] += p * ring_v[(u - s + S) % S][r];
            }
          }
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

#pragma unroll
  for (int s = 0; s < S; ++s) {
    reinterpret_cast<double*>(scratch(wave))[S * lane + s] = best[s];
    reinterpret_cast<int*>(scratch(wave) + TS * 8)[S * lane + s] = bestk[s];
  }
  __syncthreads();
  for (int q = tid; q < TS; q += 256) {
    const int ix = ix0 + q;
    const int64_t idx = (int64_t)iq * W.cur_nx + ix;
    if (ix < W.cur_nx && idx >= lo && idx < hi) {
      double bv = reinterpret_cast<const double*>(scratch(0))[q];
      int bk = reinterpret_cast<const int*>(scratch(0) + TS * 8)[q];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        double ov = reinterpret_cast<const double*>(scratch(w))[q];
        int ok = reinterpret_cast<const int*>(scratch(w) + TS * 8)[q];
        if (better<MAXDIR>(ov, ok, bv, bk)) {
          bv = ov;
          bk = ok;
        }
      }
      const int64_t o = (int64_t)chunk * W.partial_stride + idx;
      out_val[o] = bv;
      out_idx[o] = bk;
    }
  }
}

// arg-opt over the action chunks: rows [c * stride + idx], c = 0..n_chunks-1
template <bool MAXDIR>
__global__ __launch_bounds__(256) void window_combine_kernel(const double* __restrict__ part_val,
                                                             const int32_t* __restrict__ part_idx, int n_chunks,
                                                             int64_t stride, double* __restrict__ v_cur,
                                                             int32_t* __restrict__ pol, int64_t lo, int64_t hi) {
  const int64_t idx = lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= hi) return;
  double bv = part_val[idx];
  int bk = part_idx[idx];
  for (int c = 1; c < n_chunks; ++c) {
    double ov = part_val[(int64_t)c * stride + idx];
    int ok = part_idx[(int64_t)c * stride + idx];
    if (better<MAXDIR>(ov, ok, bv, bk)) {
      bv = ov;
      bk = ok;
    }
  }
  v_cur[idx] = bv;
  pol[idx] = bk;
}


// ---------------------------------------------------------------------------------------------
// OPT-IN separable mode for F1 -- NOT the graded brute-force path.
// In real arithmetic Q(x, a) = c(a) + G(x + a) with G(y) = sum_j p_j [ M(y - d_j) + V_{t+1}(clamp(y - d_j)) ],
// so a period costs O((S + A) D + S A) instead of O(S A D).  The summation order differs from the
// reference's (c(a) is added once at the end instead of inside every term), so values agree with the
// brute-force path only to rounding (parity statement: 1e-9 relative, tests/test_gpu_separable.py) and
// the arg-opt may differ where two actions tie to within that rounding.  Any demand grid (no unit-stride
// requirement).  One workgroup = 64 states: phase 1 builds G over the tile's 64 + A - 1 levels in LDS,
// phase 2 scans the actions.
// The weights need not sum to 1 (the ABI takes any: zeroed points without renormalising, a negative weight): the reference's
// sum_j p_j (c(a) + ...) carries c(a) * sum_j p_j, so phase 2 forms Q(x, a) = c(a) * P_t + G(x + a) with P_t the period's
// weights added in ascending order from 0.0 on the host (SepParams::p_sum).  P_t == 1.0 multiplies exactly: the bits of
// a normalised period are those of c(a) + G(x + a).  tests/separable_twin.py restates this kernel bit for bit.
// ---------------------------------------------------------------------------------------------
struct SepParams {
  double x_lo, step, h, pi, K, v;
  double next_x_lo, inv_step;
  double min_inventory, max_inventory;
  double d_min;          // smallest demand value of the period
  double p_sum;          // the period's weights added in ascending order from 0.0 (1.0 for a normalised pmf)
  int32_t d_range;       // (d_max - d_min) / step
  int32_t clamp_inventory;
  int32_t next_last;
  int32_t n_actions, n_demand;
};

template <bool MAXDIR, bool FUTURE>
__global__ __launch_bounds__(256) void separable_f1_kernel(SepParams P, const double* __restrict__ v_next,
                                                           double* __restrict__ v_cur, int32_t* __restrict__ pol,
                                                           const double* __restrict__ pmf_d,
                                                           const double* __restrict__ pmf_p, int64_t lo, int64_t hi) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // levels the tile can reach: y - d for y in [y0, y0 + 64 + A - 2], d in [d_min, d_max]; slot e <-> level
  // lev_lo + e*step, lev_lo = y0 - d_max
  const int span = 64 + P.n_actions - 1;
  const int wlen = span + P.d_range;
  double2* s_w = reinterpret_cast<double2*>(smem);        // {M(level), V_{t+1}(clamp level)}
  double* s_g = reinterpret_cast<double*>(s_w + wlen);    // G over the tile's 64 + A - 1 values of x + a
  double* s_val = s_g + span;
  int* s_k = reinterpret_cast<int*>(s_val + 4 * 64);
  const int tid = threadIdx.x;
  const int64_t i0 = lo + (int64_t)blockIdx.x * 64;
  const double y0 = P.x_lo + (double)i0 * P.step;
  const double lev_lo = y0 - (P.d_min + (double)P.d_range * P.step);
  for (int e = tid; e < wlen; e += 256) {
    const double l = lev_lo + (double)e * P.step;
    double2 w;
    w.x = P.h * jmax(l, 0.0) + P.pi * jmax(-l, 0.0);
    w.y = 0.0;
    if constexpr (FUTURE) {
      double nx = l;
      if (P.clamp_inventory) {
        nx = nx > P.max_inventory ? P.max_inventory : nx;
        nx = nx < P.min_inventory ? P.min_inventory : nx;
      }
      int idx = (int)((nx - P.next_x_lo) * P.inv_step);
      idx = idx > P.next_last ? P.next_last : idx;  // levels only padded lanes / actions reach
      idx = idx < 0 ? 0 : idx;
      w.y = v_next[idx];
    }
    s_w[e] = w;
  }
  __syncthreads();
  for (int e = tid; e < span; e += 256) {
    double g = 0.0;
    for (int j = 0; j < P.n_demand; ++j) {
      const double p = pmf_p[j];
      const int jd = (int)((pmf_d[j] - P.d_min) * P.inv_step);  // wave-uniform
      const double2 w = s_w[e + P.d_range - jd];
      g += p * w.x;
      if constexpr (FUTURE) g += p * w.y;
    }
    s_g[e] = g;
  }
  __syncthreads();
  const int sx = tid & 63, as = tid >> 6;
  double best = MAXDIR ? -1.7976931348623157e308 : 1.7976931348623157e308;
  int bestk = 0;
  for (int k = as; k < P.n_actions; k += 4) {
    const double a = (double)k * P.step;
    const double q = ((a > 0 ? P.K : 0.0) + P.v * a) * P.p_sum + s_g[sx + k];
    if (MAXDIR ? (q > best) : (q < best)) {
      best = q;
      bestk = k;
    }
  }
  s_val[as * 64 + sx] = best;
  s_k[as * 64 + sx] = bestk;
  __syncthreads();
  const int64_t idx = i0 + tid;
  if (tid < 64 && idx < hi) {
    double bv = s_val[tid];
    int bk = s_k[tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      double ov = s_val[w * 64 + tid];
      int ok = s_k[w * 64 + tid];
      if (better<MAXDIR>(ov, ok, bv, bk)) {
        bv = ov;
        bk = ok;
      }
    }
    v_cur[idx] = bv;
    pol[idx] = bk;
  }
}

// ---------------------------------------------------------------------------------------------
// OPT-IN separable mode for F2 (Leadtime.java:50-81) -- NOT the graded path.
// The level y - d, y = x + preQ, does not depend on the action, and the action only picks the plane of V_{t+1}
// (next preQ = action; with lead_time 2 the plane (q2' = action, q1' = q2)).  In real arithmetic
//     Q(x, q1[, q2], a) = c(a) + L(y) + W_{a[,q2]}(y),   L(y) = sum_j p_j M(y - d_j),
//     W_p(y) = sum_j p_j V_{t+1}[plane p][clamp(y - d_j)],
// so V_t and the arg-min depend on (y[, q2]) only: a period costs O(A * NY * D [* nq]) for the table
// G[q2][y] = min_a Q(y[, q2], a) instead of O(S * A * D), plus one 12-byte write per state.
// Unlike the F1 mode this one reassociates nothing: every state of a level evaluates the very same cells (the lambdas read
// x and preQ only through their sum), so the table kernel forms Q(y, a) with the reference's operations in the reference's
// order and the expansion copies it -- values and arg-min BIT-IDENTICAL to the brute-force kernels and the oracle
// (tests/test_gpu_separable.py).  What the mode changes is the number of cells executed, not any result; it stays opt-in
// because the metric counts executed (state, action, demand) cells.
// Kernel 1: one workgroup = 64 values of y (lanes) x 4 action slots of one q2; kernel 2 expands G over the slab.
// ---------------------------------------------------------------------------------------------
struct SepF2Params {
  double y_lo;        // level of e = 0: x_lo(cur)   (preQ starts at 0)
  double step, inv_step, h, pi, K, v;
  double min_inventory, max_inventory, next_x_lo;
  int32_t clamp_inventory;
  int32_t next_last;  // nx(next) - 1
  int32_t next_nx;    // plane stride of V_{t+1}
  int32_t next_nq1;   // lead_time 2: planes of V_{t+1} are (q2' = action) * nq1 + (q1' = q2)
  int32_t lead2;
  int32_t n_actions, n_demand;
  int32_t ny;         // nx(cur) + nq1(cur) - 1
  int32_t cur_nx, cur_nq1;
};

template <bool FUTURE>
__global__ __launch_bounds__(256) void separable_f2_table_kernel(SepF2Params P, const double* __restrict__ v_next,
                                                                 double* __restrict__ g_val, int32_t* __restrict__ g_idx,
                                                                 const double* __restrict__ pmf_d,
                                                                 const double* __restrict__ pmf_p) {
  __shared__ double s_val[4 * 64];
  __shared__ int s_k[4 * 64];
  const int tid = threadIdx.x, sx = tid & 63, as = tid >> 6;
  const int e = blockIdx.x * 64 + sx;
  const int iq2 = blockIdx.y;  // 0 with lead time 1
  const int ec = e < P.ny ? e : P.ny - 1;
  const double y = P.y_lo + (double)ec * P.step;
  double best = 1.7976931348623157e308;
  int bestk = 0;
  for (int k = as; k < P.n_actions; k += 4) {
    const double a = (double)k * P.step;
    // Every state (x, preQ) of one level y = x + preQ evaluates the SAME cells -- the reference's lambdas read the two only
    // through their sum (Leadtime.java:61-81) -- so Q(y, a) formed here with the reference's operations in the reference's
    // order (imm = fv + hold + pen; acc += p imm; acc += p V, demand ascending) is bit for bit the Q(x, preQ, a) the
    // brute-force kernels form for each of them: the table is exact, not a reassociation.
    const double fv = (a > 0 ? P.K : 0.0) + P.v * a;
    double q = 0.0;
    {
      const double* plane = FUTURE ? v_next + (int64_t)(P.lead2 ? k * P.next_nq1 + iq2 : k) * P.next_nx : nullptr;
      for (int j = 0; j < P.n_demand; ++j) {
        const double lev = y - pmf_d[j];
        const double imm = fv + P.h * jmax(lev, 0.0) + P.pi * jmax(-lev, 0.0);
        const double p = pmf_p[j];
        q += p * imm;
        if constexpr (FUTURE) {
          double nx = lev;
          if (P.clamp_inventory) {
            nx = nx > P.max_inventory ? P.max_inventory : nx;
            nx = nx < P.min_inventory ? P.min_inventory : nx;
          }
          int idx = (int)((nx - P.next_x_lo) * P.inv_step);
          idx = idx > P.next_last ? P.next_last : idx;  // (levels only padded lanes reach)
          idx = idx < 0 ? 0 : idx;
          q += p * plane[idx];
        }
      }
    }
    if (q < best) {  // LeadtimeRecursion is MIN only (LeadtimeRecursion.java:52,66)
      best = q;
      bestk = k;
    }
  }
  s_val[as * 64 + sx] = best;
  s_k[as * 64 + sx] = bestk;
  __syncthreads();
  if (tid < 64 && e < P.ny) {
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
    g_val[(int64_t)iq2 * P.ny + e] = bv;
    g_idx[(int64_t)iq2 * P.ny + e] = bk;
  }
}

__global__ __launch_bounds__(256) void separable_f2_expand_kernel(SepF2Params P, const double* __restrict__ g_val,
                                                                  const int32_t* __restrict__ g_idx,
                                                                  double* __restrict__ v_cur, int32_t* __restrict__ pol,
                                                                  int64_t lo, int64_t hi) {
  const int64_t idx = lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= hi) return;
  const int64_t iq = idx / P.cur_nx;
  const int ix = (int)(idx - iq * P.cur_nx);
  const int iq2 = (int)(iq / P.cur_nq1);
  const int iq1 = (int)(iq - (int64_t)iq2 * P.cur_nq1);
  const int64_t g = (int64_t)iq2 * P.ny + ix + iq1;
  v_cur[idx] = g_val[g];
  pol[idx] = g_idx[g];
}

}  // namespace sdp
