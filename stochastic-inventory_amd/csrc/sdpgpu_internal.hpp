// sdpgpu_internal.hpp -- what the translation units of libsdpgpu.so share: the handle, the per-period layout
// record, small host helpers and the functions one unit offers the others.  Not installed, not part of the ABI.
//
//   sdpgpu.hip          descriptor validation, grid layout, device tables, period dispatch, the C ABI
//   sdpgpu_generic.hip  generic per-cell kernel (every family), reachable set, rollout, user-defined functors
//   sdpgpu_window.hip   F1 window kernel (plan, chunk/key bookkeeping, finalize) and F2 row-window kernel
//   sdpgpu_cash.hip     F3 uniform-shift kernel and the cash row kernel (F3-F6)
//   sdpgpu_staff.hip    STAFF family (workforce.StaffRecursion): level-dependent pmf tables, its period kernel
//   sdpgpu_sparse.hip   reachable-set engine of the two-product lead-time family (own entry point)
//   sdpgpu_pmf.hip      GetPmf.getpmf / CLSP.main's inline pmf (host arithmetic) behind the ABI
//   sdpgpu_batch.hip    a batch of F1 instances (own entry points): batched solve, batched rollout of the table policy and of
//                       (s, S) level rules (ONE kernel over a rule: sdp_batch_sim.hpp, sdp_fitss.hpp), the level-rule fit
//   sdpgpu_simsample.hip  demand paths drawn on the device for a handle's policy simulation (sampler, fused rollout, reduction)
//   sdpgpu_staffsim.hip   STAFF family: a hiring rule rolled out on a sampled tree
//   sdpgpu_cashrulesim.hip  CASH family: (s, C, S) ordering rules rolled out along sampled demand paths, the state kept as doubles
//   sdpgpu_xrsim.hip      CASH family, cash_formula 2: the policy table and Chao's a* levels rolled out on the (x, R) state; a* itself
//   sdpgpu_sim_host.hpp   host helpers of those units: exception barrier, device scope, stream record, sampler specs, scratch
//   sdpgpu_comm.hip     multi-GPU: RCCL communicators (loaded on first use), per-period all-gather, sharded sweeps
#pragma once
#include "../../include/sdpgpu.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <new>
#include <mutex>
#include <string>
#include <vector>

#include "sdp_device.hpp"

namespace sdp {
struct FinalizeJob;
struct QueryStates;
struct SimPeriod;
}  // namespace sdp

namespace sdpgpu_detail {
struct SamplerSpecs;  // sdpgpu_sim_host.hpp
}

using sdp::DevParams;
using sdp::Grid;



// THE SCREEN of the F1 level kernel (sdp_window.hpp): a screened level block skips the leading demand steps that carry at
// most this share of the period's probability (screen_start, f1_screen_start in sdpgpu_window.hip).  Any bound is exact; a
// larger one skips more steps and may fail more screens.  2^-16 was taken from the sweep of 2^-16, 2^-24, 2^-32 in
// profiles/f1_screen_ab.txt (same failed screens, one more block of S steps skipped than 2^-24); SDPGPU_F1_SCREEN_LOG2=<e>
// (diagnostic) uses 2^-e.
constexpr double kF1ScreenMass = 0x1p-16;
// per period: steps run, tests made, blocks screened and stopped, screens failed, exact walks, steps of screened passes
constexpr int kCutCounters = 6;
// THE SCREEN ROWS of the F1 level kernel (sdp_window.hpp): the action rows RS a screened pass walks, of the block's R = 4.
// SDPGPU_F1_SCREEN_ROWS=<1|2|4> at create time; 4 is the kernel without the collapse, instruction for instruction.
constexpr int kF1ScreenRows = 2;
// THE STEP GROUPS of the F1 level kernel (sdp_window.hpp): the cells SG a step of a pass takes together -- their products,
// then their `acc +=`, then their `+= p V` -- so that no fp64 instruction waits on the one directly before it.  Per cell the
// same operations on the same operands in the same order: no table, counter or stop step depends on SG.
// SDPGPU_F1_STEP_GROUP=<1|2|4> at create time; 1 is the kernel without the groups, instruction for instruction.  The default
// is the fastest SG under which the bench contract holds on the full line with 3 % to spare (profiles/f1_step_groups_ab.txt).
constexpr int kF1StepGroup = 4;
// THE LAUNCH FORMS of the F1 level kernel (sdp_window.hpp): which wave runs which task, and when -- 0 = four tasks per
// 256-thread workgroup in index order, 1 = one wave per workgroup, 2 = resident waves that claim tasks; 1 and 2 start band 0
// and then the last bands first.  No table, counter or plan depends on the form.  SDPGPU_F1_LEVEL_FORM=<0|1|2> at create
// time.  The default is the fastest form under which the bench contract holds on the full line with 3 % to spare
// (profiles/f1_level_forms_ab.txt: 13.45 ms against the 16.49 ms of form 0 on the target grid).  Where form 2 would cost an
// instantiation its third wave per SIMD (period T without the cut-off or with all rows screened) the launcher takes form 1.
constexpr int kF1LevelForm = 2;
// the wave slots the level planner sizes its rounds against (two waves per SIMD), and the workgroups of four waves that fill
// them: form 2 launches no more than these (SDPGPU_F1_LEVEL_WGS=<n> caps its grid elsewhere: tests, measurements)
constexpr int kLevelWaveSlots = 2048;
constexpr int kLevelResidentWgs = kLevelWaveSlots / 4;
// Executed fp64 operations per nominal cell of a level period that counted its steps (sdpgpu_stats_get): an exact step costs
// ops_cell per cell; a screened step walks RS of the R rows -- RS S (3 or 2) + RS operations per lane and the table's S / 64
// products, spread over the R S nominal cells (RS = R: ops_cell itself) --; a test is one compare per cell.  `screened` of the
// `steps` walked belong to screened passes; both are in units of `planned`.
inline double f1_level_ops_per_cell(double ops_cell, bool future, int R, int S, int RS, double planned, double steps,
                                    double screened, double tests) {
  const double ops_scr = (RS * S * (future ? 3.0 : 2.0) + RS + (future ? S / 64.0 : 0.0)) / (double)(R * S);
  const double ratio = RS == R ? 1.0 : ops_scr / ops_cell;
  return ops_cell * (((steps - screened) + screened * ratio) / planned) + tests / planned;
}
constexpr size_t kPmfPad = 16;  // zero-probability tail: demand loop in blocks of R <= 8, one block of prefetch

// register block / chunking of the F1 window kernel for one period (sdpgpu_window.hip)
struct WinPlan {
  int R = 0, S = 1, d_pad = 0, n_chunks = 1, chunk_blocks = 0, n_tiles = 0, n_tasks = 0;
  size_t smem = 0;
  // window_f1_level_kernel (action-major lanes): tasks = n_tiles level bands of `band` levels x n_ablocks blocks of 64 R
  // actions; d_pad, n_chunks and smem are then its own
  bool level = false;
  int band = 0, n_ablocks = 0;
  // THE DECIDED SPLIT (f1_decided_start, sdpgpu_window.hip): >= 0: the level launch covers the live states [lo, dec_c) only
  // -- band, n_tiles, n_tasks, n_chunks and smem are that launch's -- and the states [dec_c, hi) take action 0 from one
  // one-action launch of window_f1_kernel<1, 8>; -1: no split
  int64_t dec_c = -1;
  int tile_states() const { return 64 * S; }
};

// the launch of the F2 row-window kernel for one period and slab (plan_row_window, sdpgpu_window.hip): what launch_row_window
// launches and sdpgpu_plan_period reports.  R = 0: no plan (the reason is in `why`).
struct RowPlan {
  int R = 0, S = 0;        // window_f2_kernel<R, S>: actions x adjacent states per lane
  int d_pad = 0, span = 0; // demand steps padded to a multiple of 4; slots of a staged row segment
  int waves = 0;           // waves of a workgroup that take action blocks
  int chunk_blocks = 0, n_chunks = 0;     // R-blocks per chunk; chunks per tile (> 1: chunk rows + window_combine_kernel)
  int tiles_per_row = 0, tile0 = 0, n_tiles = 0;  // row tiles of 64 S states: per inventory row, first of the slab, of the slab
  size_t smem = 0;         // dynamic LDS per workgroup
};

// the launch of the staff family for one period and slab (plan_staff, sdpgpu_staff.hip): what launch_staff launches and
// sdpgpu_plan_period reports
enum StaffForm { STAFF_ACTION, STAFF_WINDOW, STAFF_PAIR, STAFF_PLAIN, STAFF_BLOCK };
struct StaffPlan {
  StaffForm form = STAFF_BLOCK;
  int r = 4;              // actions per register block: 64 for staff_action_kernel (a wave's lanes), 1 for staff_period_kernel
  int s = 1;              // adjacent states per lane: 2 for the pair kernel, 2 / 4 for the window kernel
  int tile_states = 64;   // states per workgroup (1: lanes are actions)
  int n_groups = 1, group_actions = 0;  // action groups per state tile; actions per group, a multiple of r
  int64_t tiles = 0;      // state tiles of the slab; the launch has tiles * n_groups workgroups
  size_t lds = 0;         // static LDS of the window form (sdp::staff_window_lds_bytes), 0 otherwise
};

// the separable mode of the staff family (plan_staff_separable): two launches, the rows G and P over the slab's levels
// (staff_g_kernel, one lane per level) and the scan of 64-state workgroups over them (staff_sep_min_kernel)
struct StaffSepPlan {
  int64_t levels = 0;     // hire-up-to levels the slab reaches: states + actions - 1
  int64_t g_blocks = 0;   // workgroups of 64 levels of the G launch
  int64_t tiles = 0;      // workgroups of 64 states of the min launch
  size_t lds = 0;         // static LDS of the min launch (sdp::kStaffSepMinLds)
};

// plan_window's answer for one period, kept per (slab, forced block): the search walks 8 block shapes x up to blocks_total
// chunk counts on the issuing thread, and launch_window, run_period_impl's pre-check and sdpgpu_plan_period all ask for it
// (at 30 us per period the second search sat on the critical path).  Dropped by layout().
struct WinPlanCache {
  bool valid = false;
  int64_t lo = 0, hi = 0;
  int win_r = 0, win_s = 0, win_nch = 0, win_level = -1;
  bool may_chunk = false;
  bool values_external = false;
  WinPlan plan;
  std::string why;
};

struct PeriodInfo {
  Grid g{};
  int64_t S = 0;      // grid states
  int64_t S_pad = 0;  // padded to a multiple of world_size
  int64_t lo = 0, hi = 0;  // this rank's slab
  int32_t nD = 0;
  size_t pmf_off = 0;   // element offset of this period's demand array inside d_pmf
  // The window kernels index demands by j = (d - d_0) / step.  A support with gaps (DiscreteDistribution-style
  // {2, 5, 9}) is laid out on the unit-stride grid with probability 0 in the gaps: a zero-probability step adds
  // exact zeros to the accumulator, so the sums are unchanged.  nD_win = 0: too sparse, generic kernel instead.
  int32_t nD_win = 0;      // demand steps of the unit-stride layout
  size_t pmf_win_off = 0;  // element offset of its probability array (== pmf_off + nD when there are no gaps)
  size_t v_off = 0;     // element offset of V_t inside the value arena
  size_t pol_off = 0;   // element offset of this rank's policy slab
  double overhead = 0;
  bool overhead_set = false;
  int64_t cells_rank = 0, cells_all = 0;
  bool cells_counted = false;  // count_cells has run for this slab, overhead and action counts (reset by whatever changes them)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  int32_t kernel_used = 0;
  // executed fp64 add/mul operations per cell of the kernel plan that ran this period (identical operations of
  // neighbouring cells are formed once, see sdp_window.hpp / sdp_cash.hpp); 0 = the kernel has no such model
  double ops_cell = 0;
  // F1 window periods: every V_t of the row is >= 0 (a minimum or maximum of sums of non-negative terms, f1_terms_nonneg) --
  // what the period below needs before it may stop level blocks early
  bool v_nonneg = false;
  // window_f1_level_kernel: demand steps of level blocks the launch planned (waves x blocks x d_pad; 0: another kernel), and
  // whether it ran with the cut-off, i.e. counted the steps it ran and its tests on the device (sdpgpu_handle::d_cut_count)
  int64_t lvl_steps_planned = 0;
  bool lvl_cut = false;
  int32_t lvl_screen_start = 0;  // the step screened level blocks started at in the last launch (0: the screen was off)
  int32_t lvl_r = 0, lvl_s = 0;  // the level launch's register block (R action rows x S levels per lane)
  bool lvl_future = false;       // the level launch had a future term
  int32_t lvl_form = -1, lvl_wgs = 0, lvl_threads = 0;  // its launch form, workgroups and threads each (sdpgpu_f1_level_form_get)
  double pre_ops = 0;  // fp64 operations of the cut-off's pre-pass (Q(i, 0) of every state), in total
  // the decided split of the last launch: its boundary (live states [lo, dec_c), decided [dec_c, hi)) and the live launch's
  // chunk rows; -1: the launch did not split (sdpgpu_f1_decided_get; flush_pending makes two finalize jobs of a split period)
  int64_t dec_c = -1;
  int dec_live_chunks = 0;
  double lds_cell = 0, l1_cell = 0;  // bytes per cell through the LDS / the vector L1 of the kernel that ran the period (0: no model)
  mutable WinPlanCache win_plan;     // (a cache: filled through const handles by plan_window)
};

struct sdpgpu_handle {
  sdpgpu_desc d{};
  int32_t T = 0;
  int32_t n_actions_full = 0;
  std::vector<PeriodInfo> per;  // index period-1
  std::vector<std::vector<double>> pmf_d, pmf_p;
  std::vector<char> pmf_set;
  bool laid_out = false;
  bool allocated = false;
  double* d_pmf = nullptr;
  double* d_values = nullptr;
  size_t values_elems = 0;
  bool values_external = false;
  int32_t* d_policy = nullptr;
  size_t policy_elems = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool stream_given = false;  // sdpgpu_set_stream was called (NULL then means the legacy default stream)
  bool profiling = false;
  hipEvent_t ev_solve0 = nullptr, ev_solve1 = nullptr;
  bool solve_timed = false;
  std::vector<char> period_done;  // V_t valid (a ping-pong table may have been overwritten since)
  std::vector<char> policy_done;  // the policy slab of period t has been computed
  double* d_part_val[2] = {nullptr, nullptr};  // window kernels: partial arg-opt rows [chunk][slab], by period parity
  int32_t* d_part_idx[2] = {nullptr, nullptr};
  size_t part_elems[2] = {0, 0};
  // F1 window kernel with several tasks per tile (small grids): V_t is reduced into order-preserving
  // keys by atomics and the (value, action) rows of the chunks are kept until flush_pending() turns
  // them into the final V_t / policy rows in ONE launch (see sdp_window.hpp finalize_kernel).
  unsigned long long* d_keys = nullptr;  // [T][key_stride]
  bool keys_external = false;            // caller memory (sdpgpu_attach_keys), e.g. a tensor RCCL can address
  size_t key_stride = 0;
  std::vector<char> key_row_clean;       // row t holds the reduction identity (+-Double.MAX_VALUE)
  double* d_chunk_val = nullptr;         // arena of chunk rows, period t at chunk_off[t-1]
  int32_t* d_chunk_idx = nullptr;
  std::vector<size_t> chunk_off;
  size_t chunk_arena_elems = 0;          // elements of each of the two arenas (12 bytes per element in all)
  std::vector<int> pending_chunks;       // >0: period's final rows not written yet (value = n_chunks)
  int n_pending = 0;
  sdp::FinalizeJob* d_jobs = nullptr;
  std::vector<unsigned char> jobs_host;  // upload source of d_jobs: 2 T FinalizeJobs at a fixed address (flush_pending)
  int32_t* d_rowperm = nullptr;  // cash row kernel, F5: rows of the launch ordered by level x + preQ (RowTiling::perm)
  std::vector<int32_t> rowperm_host;
  int64_t rowperm_key[4] = {-1, -1, -1, -1};
  int2* d_units = nullptr;       // F5 pair kernel: (row group, tile) units in diagonal order (RowTiling::units)
  int64_t units_key[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  char* d_rowtab = nullptr;  // cash_row_table_kernel's (row, action) blocks of the period being run (cash_row_pair_kernel<TAB>)
  size_t rowtab_bytes = 0;
  void* d_diag = nullptr;  // cash_diag_kernel: the DiagStep table of the period being run, and its padded p * gamma row
  size_t diag_bytes = 0;
  bool fuse_combine = true;
  bool use_cash_shift = true;
  bool use_cash_row = true;   // SDPGPU_CASH_ROW=0 turns the cash row kernel off (generic kernel instead)
  int win_prio_fair = 1;  // window kernel: s_setprio by progress (SDPGPU_WIN_PRIO=0 turns it off)
  int win_r = 0, win_nch = 0, win_s = 0;  // tuning overrides (SDPGPU_WIN_R / SDPGPU_WIN_NCH / SDPGPU_WIN_S), 0 = heuristic
  int f1_cutoff = 1;   // SDPGPU_F1_CUTOFF=0: the level kernel never stops a level block early (A/B runs, tests)
  double* d_f1_u = nullptr;  // the cut-off's row U(i) = Q(i, 0) of the period being run (window_f1_level_kernel)
  size_t f1_u_elems = 0;
  // SDPGPU_F1_SCREEN: -1 = the screen where the planner chose the level kernel by itself (win_level < 0) and not under a
  // forced plan, 1 = wherever the cut-off is on, 0 = never.  It never goes beyond the cut-off's gate (f1_cutoff_on).
  int f1_screen = -1;
  double f1_screen_mass = kF1ScreenMass;
  int f1_screen_rows = kF1ScreenRows;  // SDPGPU_F1_SCREEN_ROWS: action rows of a screened pass (1, 2 or 4 = all)
  int f1_step_group = kF1StepGroup;    // SDPGPU_F1_STEP_GROUP: cells a step of the level kernel takes together (1, 2 or 4)
  int f1_level_form = kF1LevelForm;    // SDPGPU_F1_LEVEL_FORM: the launch form of the level kernel (0, 1 or 2)
  int f1_level_wgs = kLevelResidentWgs;  // SDPGPU_F1_LEVEL_WGS: the most workgroups form 2 launches (diagnostic)
  int f1_level_rounds = 1;             // SDPGPU_F1_LEVEL_ROUNDS: the round count plan_level's band search starts at (diagnostic)
  unsigned* d_level_claim = nullptr;   // [T]: form 2's claim word of each period's level launch, zeroed before it
  // SDPGPU_F1_DECIDED=1: the decided split wherever the level kernel runs with the cut-off; unset or 0: never (opt-in:
  // f1_decided_on, sdpgpu_window.hip)
  int f1_decided = 0;
  // [T][kCutCounters], per period: steps run and tests made by the level kernel's waves, then its level blocks -- screened
  // and stopped, screens that failed, walked exactly (sdpgpu_f1_screen_get) -- and the steps of its screened passes
  // (sdpgpu_f1_screen_rows_get)
  unsigned long long* d_cut_count = nullptr;
  int win_level = -1;  // SDPGPU_WIN_LEVEL: 1 = the action-major level kernel wherever it can run, 0 = never, -1 = where it wins
  uint8_t* d_reach = nullptr;      // reachable masks, period t at reach_off[t-1]
  std::vector<size_t> reach_off;
  bool reach_done = false;
  // user-defined functor (sdpgpu_create_custom): code object compiled by hipRTC at create time, loaded at
  // first use; every period then runs sdp_custom_period instead of a built-in kernel
  bool custom = false;
  std::vector<char> custom_code;
  std::vector<double> custom_params;
  hipModule_t custom_mod = nullptr;
  hipFunction_t custom_period[3] = {nullptr, nullptr, nullptr};  // 64 / 16 / 4 states per workgroup
  hipFunction_t custom_reach = nullptr;
  // user lambdas of the LEVEL SHAPE (SDP_SHAPE_LEVEL in the text): the F1 window kernel runs them from per-period tables
  // M(m), c(a) filled once by the user's own compiled functions (sdp_custom_tabulate)
  bool level_shape = false;
  hipFunction_t custom_tabulate = nullptr;
  double* d_level_tabs = nullptr;             // per period: [m_tab (n_m)] [c_tab (n_a)]
  std::vector<size_t> level_tab_off;          // element offset of period t's m_tab
  std::vector<int32_t> level_m_min, level_m_n;
  // the rollout program of a user functor (sdpgpu_customsim.hip; sdp_custom_src.hpp: kCustomSim): the user's text and the
  // options of the engine compile WITHOUT -fno-honor-nans are kept from create; compiled at the first rollout call, loaded at
  // the first one that reaches the device, released by sdpgpu_destroy
  std::string custom_source;
  std::vector<std::string> custom_sim_opts;
  std::vector<char> custom_sim_code;
  hipModule_t custom_sim_mod = nullptr;
  hipFunction_t custom_sim = nullptr, custom_first = nullptr, custom_rule_sim = nullptr;
  double* d_custom_params = nullptr;
  unsigned long long* d_custom_cells = nullptr;  // [T]
  int* d_custom_err = nullptr;
  // sdpgpu_set_halo: a sharded caller may run a period on its slab widened by up to `halo` states on either side
  // (sdpgpu_run_period_range); the chunk-row arenas are sized for that
  int64_t halo = 0;
  // STAFF family (sdpgpu_set_level_pmf): per period the table transposed, lvl_p[t][j * rows + y], and its row lengths
  std::vector<std::vector<double>> lvl_p;
  std::vector<std::vector<int32_t>> lvl_len;
  std::vector<int32_t> lvl_rows, lvl_maxj;
  std::vector<double*> d_lvl_p;
  std::vector<int32_t*> d_lvl_len;
  std::vector<void*> staff_owned;   // the distinct device tables (periods given the same table share one)
  double* d_staff_val = nullptr;    // partial arg-min rows [group][slab]
  int32_t* d_staff_idx = nullptr;
  size_t staff_part_elems = 0;
  double* d_staff_g = nullptr;      // separable mode: the rows G and P over the levels a slab reaches, [2][levels], grown on demand
  size_t staff_g_elems = 0;
  // kernel-form switches, read at create time (staff_read_switches): SDPGPU_STAFF_R (register block of staff_block_kernel, 4 | 8),
  // _BLOCK=0 (staff_period_kernel, one action at a time), _PAIR (-1 unset: two states per lane where it pays, 0: never, 1: any
  // other value, wherever it can run), _WIN (-1 unset: by the staff range's size, else the value given: 2 | 4 states per lane,
  // anything else turns the window form off), _LANES (-1 unset: periods of at most 16 states, 0: never, 1: always lanes =
  // actions), _UNI=0 (window kernel without the scalar-probability form)
  int staff_r = 4;
  bool staff_plain = false;
  int staff_pair = -1, staff_win = -1, staff_lanes = -1;
  bool staff_uni = true;
  bool staff_tables_nonneg = false;  // sdpgpu_staff_simulate has found no negative entry in the (by then frozen) level pmfs
  // sdpgpu_set_action_counts: per period the caller's action-list lengths of every grid state (empty: family rule)
  std::vector<std::vector<int32_t>> counts;
  std::vector<int32_t*> d_counts;
  double* d_sep_val = nullptr;      // opt-in separable mode, lead-time family: the table G[q2][y] and its arg-min
  int32_t* d_sep_idx = nullptr;
  size_t sep_elems = 0;
  // multi-GPU (sdpgpu_comm.hip): the communicator of this rank, a second stream for the overlapped schedule, and --
  // sdpgpu_solve_multi with several ranks on ONE device -- the sibling handles whose rows are exchanged by copies
  void* comm = nullptr;  // ncclComm_t
  bool comm_prepared = false;  // sdpgpu_comm_prepare has succeeded (tables allocated, device pinned, RCCL loads)
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_comp = nullptr, ev_comm = nullptr;
  std::vector<sdpgpu_handle*> siblings;  // handles[0..n) of the last sdpgpu_solve_multi (set on every member)
  bool multi_copy = false;               // exchange by device-to-device copies (ranks share a device)
  // sdpgpu_solve as ONE HIP graph (small grids: a sweep of configs[1] is 52 launches of 30 us -- replayed from a graph the
  // sweep no longer depends on how promptly the host thread issues them).  0: no eager sweep yet; 1: one eager sweep done
  // (every lazy allocation, attribute and table upload has happened); 2: graph captured and in use; -1: off (capture refused
  // or SDPGPU_GRAPH=0).  Dropped by whatever changes what a sweep launches (graph_drop).
  int graph_state = 0;
  bool in_solve = false;
  hipGraph_t sweep_graph = nullptr;
  hipGraphExec_t sweep_exec = nullptr;
  int64_t graph_replays = 0;
  int flush_uploads = 0;  // job-list uploads of flush_pending since the counter was last reset (sdpgpu_solve's capture)
  // sdpgpu_set_sampler / sdpgpu_simulate_sampled / sdpgpu_sample_demands (sdpgpu_simsample.hip): per period index the spec's
  // threshold table (null until the first sdpgpu_set_sampler: every period draws from its pmf tile; a shared_ptr because it
  // destroys a type that only that unit completes), and ONE device block for the period records, sampler records, threshold /
  // value arenas, sums, flags and partials of a call
  std::shared_ptr<sdpgpu_detail::SamplerSpecs> samp;
  char* d_sim_scratch = nullptr;
  size_t sim_scratch_bytes = 0;
  hipEvent_t sim_ev0 = nullptr, sim_ev1 = nullptr;
  std::string err;
  std::string plan_error;  // set by a launcher that rejects a period's plan (run_period_impl reports it as SDPGPU_ERR_ARG)
  int device = -1;
};

namespace sdpgpu_detail {

extern thread_local std::string g_create_error;
int fail(sdpgpu_handle* h, int code, const char* fmt, ...);

#define HIP_TRY(h, expr)                                                                        \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return fail(h, SDPGPU_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

inline bool has_cash(int f) {
  return f == SDPGPU_FAMILY_CASH || f == SDPGPU_FAMILY_OVERDRAFT || f == SDPGPU_FAMILY_CASH_LEADTIME ||
         f == SDPGPU_FAMILY_SURVIVAL;
}
inline bool has_preq(int f) { return f == SDPGPU_FAMILY_LEADTIME || f == SDPGPU_FAMILY_CASH_LEADTIME; }

// Java semantics needed on the host for the layout only.
inline int64_t java_round(double x) {
  double f = std::floor(x);
  return (int64_t)((x - f >= 0.5) ? f + 1.0 : f);
}
inline int32_t java_d2i(double x) {
  if (x != x) return 0;
  if (x >= 2147483647.0) return INT32_MAX;
  if (x <= -2147483648.0) return INT32_MIN;
  return (int32_t)x;
}

inline int64_t cash_key_of_bound(const sdpgpu_desc& d, double bound) {
  // key of the grid point the reference's rounding maps `bound` to
  int64_t r = java_round(bound * d.cash_round_mult);
  if (d.cash_round_int_div) return r / (int64_t)d.cash_round_div;
  return r;
}

inline bool is_pow2_int(double s) {
  if (!(s >= 1) || s != std::floor(s) || s > 1073741824.0) return false;
  int64_t v = (int64_t)s;
  return (v & (v - 1)) == 0;
}

// A dispatch carries at most 2^32 - 1 work-items (AQL grid_size is 32 bits); beyond that the launch is
// silently truncated.  Every launcher below sends 256-thread workgroups and refuses a grid over the limit.
inline bool grid_ok(int64_t blocks) { return blocks > 0 && blocks * 256 < 4294967296LL; }

// LDS of a gfx950 compute unit: 160 KiB, all of which one workgroup may take.  A launch that asks for more than the
// 64 KiB of earlier parts raises the kernel's dynamic-LDS limit first (lds_allow); planners budget against kLdsPerCU
// divided by the workgroups they want resident together on a CU.
constexpr size_t kLdsPerCU = 160 * 1024;
constexpr size_t kLdsLegacy = 64 * 1024;
inline int lds_workgroups(size_t smem) { return smem == 0 ? 32 : (int)(kLdsPerCU / smem); }

// Allow a kernel more than 64 KiB of dynamic LDS.  The attribute belongs to the function on the current device: it is
// raised ONCE per kernel instantiation and device, straight to the whole 160 KiB of the CU, under a lock -- so the limit never
// decreases and two host threads (SDPGPU_SHARDED_THREADS with ranks sharing a device, slabs planning different sizes) cannot
// lower it under each other's launch.  `mark` is the caller's per-instantiation record.
struct LdsMark {
  std::mutex m;
  bool raised[64] = {};
};
template <class K>
inline hipError_t lds_allow(K kernel, size_t smem, LdsMark* mark) {
  if (smem <= kLdsLegacy) return hipSuccess;
  if (smem > kLdsPerCU) return hipErrorInvalidValue;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mark->m);
  bool* slot = (dev >= 0 && dev < 64) ? &mark->raised[dev] : nullptr;
  if (slot && *slot) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCU);
  if (e == hipSuccess && slot) *slot = true;
  return e;
}

// the handle evaluates the backorder family's loop shape on the F1 window kernel: the built-in family, or user lambdas that
// declared the level shape
inline bool f1_like(const sdpgpu_handle* h) { return !h->custom || h->level_shape; }

// ---- sdpgpu.hip ----------------------------------------------------------------------------------------
int run_period_impl(sdpgpu_handle* h, int period, int part = SDPGPU_PART_ALL, int64_t range_lo = -1, int64_t range_hi = -1);
void graph_drop(sdpgpu_handle* h);  // forget the captured sweep (the next sdpgpu_solve runs eagerly, the one after captures again)
void count_cells(sdpgpu_handle* h, int period);
int flush_api(sdpgpu_handle* h);
int layout(sdpgpu_handle* h);
int ensure_device(sdpgpu_handle* h);
int allocate(sdpgpu_handle* h);
DevParams make_params(const sdpgpu_handle* h, int period);

// ---- sdpgpu_comm.hip -----------------------------------------------------------------------------------
void comm_release(sdpgpu_handle* h);  // sdpgpu_destroy: communicator, second stream, events

// ---- sdpgpu_generic.hip ----------------------------------------------------------------------------------
hipError_t launch_gather_grid(const DevParams& P, const double* v_next, double* v_cur, int32_t* pol, const double* pmf_d,
                              const double* pmf_p, int64_t lo, int64_t hi, hipStream_t st);
hipError_t launch_gather_query(const DevParams& P, const double* v_next, double* out_val, int32_t* out_act,
                               const double* pmf_d, const double* pmf_p, int64_t n, const double* x, const double* cash,
                               const double* preq, const double* preq2, hipStream_t st);
hipError_t launch_custom_period(sdpgpu_handle* h, int period, const double* v_next, double* v_cur, int32_t* pol,
                                int64_t lo, int64_t hi, const double* qx, const double* qcash, const double* qpreq,
                                bool count);
int custom_check(sdpgpu_handle* h);
int fill_level_tables(sdpgpu_handle* h);  // user lambdas of the level shape: M(m), c(a) of every period (sdp_custom_tabulate)
int compute_reachable(sdpgpu_handle* h);
hipError_t launch_simulate(sdpgpu_handle* h, const sdp::SimPeriod* d_per, const double* d_dem, const double* d_disc,
                           int64_t n_paths, int64_t idx0, double ini_x, double ini_cash, double ini_preq,
                           double ini_preq2, int first_k, double* d_sum, uint8_t* d_valid);

// ---- sdpgpu_staff.hip -----------------------------------------------------------------------------------
int staff_upload(sdpgpu_handle* h);
void staff_read_switches(sdpgpu_handle* h);  // the SDPGPU_STAFF_* switches, once per handle (sdpgpu_create)
StaffPlan plan_staff(const sdpgpu_handle* h, int period, int64_t lo, int64_t hi);
StaffSepPlan plan_staff_separable(const sdpgpu_handle* h, int period, int64_t lo, int64_t hi);
hipError_t launch_staff_separable(sdpgpu_handle* h, int period, const double* v_next, double* v_cur, int32_t* pol, int64_t lo,
                                  int64_t hi, hipStream_t st);
hipError_t launch_staff(sdpgpu_handle* h, int period, const double* v_next, double* v_cur, int32_t* pol, int64_t lo,
                        int64_t hi, hipStream_t st);
int64_t staff_cells(const sdpgpu_handle* h, int period, int64_t lo, int64_t hi);
void staff_reach_intervals(const sdpgpu_handle* h, std::vector<int64_t>* lo_out, std::vector<int64_t>* hi_out);

// ---- sdpgpu_cash.hip ---------------------------------------------------------------------------------------
bool cash_shift_eligible(const sdpgpu_handle* h, int period);
hipError_t launch_cash_shift(sdpgpu_handle* h, const DevParams& P, int period, const double* v_next, double* v_cur,
                             int32_t* pol, const double* pmf_d, const double* pmf_p, int64_t lo, int64_t hi, hipStream_t st);
bool cash_row_eligible(const sdpgpu_handle* h, int period);
size_t cash_row_lds(int nD, int tile_pts);
hipError_t launch_cash_row(sdpgpu_handle* h, const DevParams& P, int period, const double* v_next, double* v_cur,
                           int32_t* pol, const double* pmf_d, const double* pmf_p, int64_t lo, int64_t hi, hipStream_t st, bool levels_only = false);
// F5, OPT-IN separable mode: the rows of one level x + preQ hold identical tables; launch_cash_row(levels_only) evaluates one
// representative row per level, this copies it to the level's other rows
hipError_t launch_level_fill(sdpgpu_handle* h, int period, double* v_cur, int32_t* pol, hipStream_t st);

// ---- sdpgpu_pmf.hip ----------------------------------------------------------------------------------------
// threshold table of one distribution for the batch sampler (host arithmetic): demand = k_lo + #{thr <= u}, or #{thr < u} when
// *strict; a failure leaves its reason in *why
int sample_table_build(const sdpgpu_dist_spec& spec, int32_t* k_lo, std::vector<double>* thr, int32_t* strict, std::string* why);

// ---- sdpgpu_window.hip -------------------------------------------------------------------------------------
bool window_eligible(const sdpgpu_handle* h, int period);
// (why: receives the reason when no plan exists -- a forced plan that is infeasible, or a period too big for the LDS)
WinPlan plan_window(const sdpgpu_handle* h, int period, int64_t lo, int64_t hi, std::string* why = nullptr);
RowPlan plan_row_window(const sdpgpu_handle* h, int period, int64_t lo, int64_t hi, std::string* why = nullptr);
// the step screened level blocks start at under the mass bound `mass` (S: the level kernel's levels per block; 0: none)
int f1_screen_start(const sdpgpu_handle* h, int period, int S, double mass);
int64_t f1_decided_start(const sdpgpu_handle* h, int period);
hipError_t flush_pending(sdpgpu_handle* h);
// the two kernels of chunked periods, defined in this unit only (the batched solve launches them too): key rows to the
// reduction identity of the direction; V_t and policy rows from keys + chunk rows (`total` states over `n_jobs` jobs)
hipError_t launch_key_fill(unsigned long long* keys, int64_t n, int maxdir, hipStream_t st);
hipError_t launch_finalize(const sdp::FinalizeJob* d_jobs, int n_jobs, int64_t total, hipStream_t st);
bool window_interior_tiles(const sdpgpu_handle* h, int period, int64_t lo, int64_t hi, int* first, int* count);
hipError_t launch_separable_f2(sdpgpu_handle* h, const DevParams& P, int period, const double* v_next, double* v_cur,
                               int32_t* pol, const double* pd, const double* pp);
hipError_t launch_separable(sdpgpu_handle* h, const DevParams& P, int period, const double* v_next, double* v_cur,
                            int32_t* pol, const double* pd, const double* pp, bool* too_big);
// geometry of a period's chunk rows: element stride between chunks and the state index of element 0
inline int64_t chunk_row_cap(const sdpgpu_handle* h, const PeriodInfo& p) { return (p.hi - p.lo) + 2 * h->halo; }
inline int64_t chunk_row_lo(const sdpgpu_handle* h, const PeriodInfo& p) { return p.lo - h->halo; }
hipError_t launch_window(sdpgpu_handle* h, const DevParams& P, int period, const double* v_next, double* v_cur,
                         int32_t* pol, const double* pmf_d, const double* pmf_p, int64_t lo, int64_t hi, hipStream_t st,
                         int part);

}  // namespace sdpgpu_detail
