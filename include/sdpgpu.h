/*
 * sdpgpu.h -- C ABI of the MI355X-native finite-horizon SDP engine.
 *
 * This is the drop-in boundary for ONE path of RobinChen121/Stochastic-Inventory:
 * the backward Bellman recursion of src/sdp (the `getExpectedValue` bodies).  A
 * host in any language (the reference's Java over JNI, C++, Python ctypes) binds
 * exactly these entry points.  Plain pointers and sizes only: no JNI, torch or
 * C++ types cross this line, no exception crosses it, every call returns an int
 * status (0 = ok) and the text of the last failure is read with
 * sdpgpu_last_error().
 *
 * Reference interface each entry point replaces (paths relative to the reference
 * checkout):
 *
 *   sdpgpu_create            constructors  src/sdp/inventory/Recursion.java:49-63,
 *                            src/sdp/inventory/LeadtimeRecursion.java:28-45,
 *                            src/sdp/cash/CashRecursion.java:39-56,
 *                            src/sdp/cash/CashLeadtimeRecursion.java:28-46,
 *                            src/capacitated/CLSP.java:22-24.  The three Java lambdas
 *                            (feasible actions / StateTransitionFunction /
 *                            ImmediateValueFunction; StateTransition.java:20-22,
 *                            ImmediateValue.java:23-25) cannot be called from a GPU;
 *                            they are named by `family` + the scalar parameters the
 *                            in-scope drivers close over (see sdpgpu_desc).
 *   sdpgpu_set_pmf           the `double[][][] pmf` constructor argument
 *                            (Recursion.java:38,54): pmf[t][j] = {demand, prob}.
 *                            Also RiskRecursion.java:31-46 (family SURVIVAL).
 *   sdpgpu_solve             the first `getExpectedValue(initialState)` / `getSurvProb(initialState)` call
 *                            (Recursion.java:89-163, CLSP.java:88-138,
 *                            LeadtimeRecursion.java:47-75, CashRecursion.java:79-140,
 *                            CashLeadtimeRecursion.java:48-79): fills the value and
 *                            action maps.  Here: dense backward sweep t = T..1.
 *   sdpgpu_run_period        one level of that recursion (all states of period t).
 *   sdpgpu_solve_sharded /   the same first call with the state axis cut over the GPUs of a node (one rank per
 *   sdpgpu_solve_multi       process, or all devices from one process): still ONE call per rank / per JVM.
 *   sdpgpu_values            `cacheValues` lookups (Recursion.java:36,90).
 *   sdpgpu_policy            `cacheActions` lookups / getAction / getCacheActions
 *                            (Recursion.java:35,160,165-171).
 *   sdpgpu_eval_states       `getExpectedValue(state)` for a state that is not a
 *                            grid point (e.g. an off-grid period-1 initial cash,
 *                            CashConstraint.java:141) and the lazy re-entry of the
 *                            simulators (Simulation.java:62-63).
 *   sdpgpu_simulate          the rollout loops of the simulators (Simulation.java:59-69,
 *                            CashSimulation.java:101-112): policy look-up + imm + transition.
 *   sdpgpu_custom_simulate / the same loops, and the overdraft drivers' rule rollouts (CashSimulation.java:1142-1250:
 *   _simulate_sampled /      simulatesCSDraft, simulatesSOD, simulatesSOD2), for a handle of USER lambdas
 *   sdpgpu_custom_rule_simulate  (sdpgpu_create_custom), through the lambdas' own compiled text.
 *   sdpgpu_reachable        the key set of `cacheActions`, i.e. the states the
 *                            memoised recursion would have visited; getOptTable
 *                            (Recursion.java:177-186) lists exactly those.
 *
 * Numerics contract: all arithmetic fp64, no FMA contraction, demand index
 * ascending, `acc += p*imm; acc += p*[gamma*]V(next)` in that order, strict </>
 * arg-opt in ascending action order (lowest action index wins ties), so values
 * are bit-identical to a literal CPU restatement of the Java loops and the policy
 * indices are bit-exact.
 *
 * Threading: a handle is NOT thread-safe; distinct handles are independent.
 * Ownership: the caller owns every host buffer; the library copies what it needs
 * at the call and owns its device tables unless sdpgpu_attach_values is used.
 */
#ifndef SDPGPU_H
#define SDPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: only this header is exported */
#endif

#define SDPGPU_ABI_VERSION 6

/* status codes */
#define SDPGPU_OK 0
#define SDPGPU_ERR_ARG 1      /* bad descriptor / argument */
#define SDPGPU_ERR_STATE 2    /* call out of order (e.g. values before solve) */
#define SDPGPU_ERR_DEVICE 3   /* HIP runtime error (message carries hipGetErrorString) */
#define SDPGPU_ERR_UNSUPPORTED 4
#define SDPGPU_ERR_ALLOC 5    /* ABI 6: a host allocation failed (std::bad_alloc caught at the boundary) */
#define SDPGPU_ERR_INTERNAL 6 /* ABI 6: any other C++ exception caught at the boundary -- none crosses it */

/* Functor families = the closed-form lambda families of the in-scope drivers. */
typedef enum sdpgpu_family {
  /* state (x). CLSP.java:251-272, CLSPTesting.java:78-106, CLSPforDraw.java:86-103,
   * LevelFitsS.java:85-102.  Backorder, two-ternary clamp, imm on unclamped level. */
  SDPGPU_FAMILY_BACKORDER = 1,
  /* state (x, preQ). Leadtime.java:50-81.  Lead time 1, order arrives next period.  With
   * desc.lead_time = 2 (a generalisation the reference does not have; BASELINE configs[3]) the state is
   * (x, q1, q2): q1 arrives this period, q2 the next; x' = x + q1 - d, q1' = q2, q2' = action. */
  SDPGPU_FAMILY_LEADTIME = 2,
  /* state (x, cash). CashConstraint.java:95-133 (cash_formula 0) and
   * CashConstraintTesting.java:110-148 (cash_formula 1).  Lost sales, cash-limited orders.
   * cash_formula 2: sdp.cash.CashRecursionXR.getExpectedValue (CashRecursionXR.java:79-126) over the lambdas of
   * cash.singleItem.CashConstraintXR (CashConstraintXR.java:84-125; Chao 2008): state (x, R) with working capital
   * R = cash + variCost * x, actions = order-up-to levels y = x, x + 1, ... up to max(x, R / variCost).  The grid is
   * (inventory, cash) as for formula 0 -- the transition rounds the cash balance (:120) before it forms R (:121) --
   * and wherever this header says `cash` for a state of this family (ini_cash, sdpgpu_state_index,
   * sdpgpu_eval_states) the value is R.  Policy indices k stand for y = x + k (getAction = x + k * step).
   * max_order_quantity is not read (the reference's list is bounded by R / variCost only). */
  SDPGPU_FAMILY_CASH = 3,
  /* state (x, cash). CashOverdraft.java:72-118.  Piecewise overdraft interest. */
  SDPGPU_FAMILY_OVERDRAFT = 4,
  /* state (x, cash, preQ). SingleProductLeadtime.java:72-119. */
  SDPGPU_FAMILY_CASH_LEADTIME = 5,
  /* state (x, cash). The survival-probability recursion: RiskRecursion.getSurvProb (RiskRecursion.java:65-108)
   * == CashRecursion.getSurvProb (CashRecursion.java:143-194, which also multiplies by discount_factor) with the
   * lambdas of cashSurvival.java:98-143: orders limited by cash / variCost, no penalty term.  The value is
   * P(final cash >= 0 and no negative cash on the way) under the best policy, MAX only; a successor with
   * negative cash contributes 0 and is not visited. */
  SDPGPU_FAMILY_SURVIVAL = 6,
  /* state (staff number). workforce.StaffRecursion.getExpectedValue (StaffRecursion.java:81-118) with the lambdas of
   * WorkforcePlanning.java:72-101 (clamp_inventory 1) / WorkforceTesting.java:80-107 (clamp_inventory 0): the pmf of
   * a period depends on the hire-up-to level y = staff + hires (sdpgpu_set_level_pmf, not sdpgpu_set_pmf).  MIN only.
   * Descriptor fields: min/max_inventory = minX/maxX (>= 0), ini_inventory = iniStaffNum, max_order_quantity =
   * maxHireNum, step 1, fixed_order_cost = fixCost, unit_order_cost = unitVariCost, holding_cost = salary,
   * penalty_cost = unitPenalty; minStaffNum[t] goes through sdpgpu_set_overhead (an integer). */
  SDPGPU_FAMILY_STAFF = 7
} sdpgpu_family;

/* OptDirection, Recursion.java:44-47 / CashRecursion.java:34-37. */
typedef enum sdpgpu_direction { SDPGPU_MIN = 0, SDPGPU_MAX = 1 } sdpgpu_direction;

/* kernel selection (0 = let the library choose) */
#define SDPGPU_KERNEL_AUTO 0
#define SDPGPU_KERNEL_GATHER 1 /* generic per-cell functor + gather from V_{t+1} in HBM/L2 */
#define SDPGPU_KERNEL_WINDOW 2 /* F1/F2: LDS-staged {L(l), V(clamp l)} window, register sliding */
#define SDPGPU_KERNEL_SEPARABLE 3 /* OPT-IN, never chosen automatically.
                                     F1: Q(x,a) = c(a) + G(x+a), O((S+A)D + SA) per period.  REASSOCIATES the reference's
                                     sum: values agree to rounding (1e-9 relative), the arg-opt may differ on near-ties.
                                     Weights that do not sum to 1 are honoured: the mode forms c(a) * P_t + G(x+a), P_t the
                                     period's weights added in ascending order (the reference's sum carries c(a) * P_t);
                                     P_t == 1.0 leaves c(a) + G(x+a) bit for bit (tests/separable_twin.py is its twin).
                                     F2 (lead time 1 or 2): V_t and the arg-min depend on (x + preQ[, q2]) only: one
                                     evaluation per level in the reference's operation order, O(A (nx+nq) D [nq]) for
                                     that table + one write per state.  EXACT: values and policy bit-identical to the
                                     cell-by-cell kernels (tests/test_gpu_separable.py).
                                     F5 (cash + lead time, ABI 6): SingleProductLeadtime's lambdas read x and preQ through
                                     x + preQ only (SingleProductLeadtime.java:82-119), so every row of a level holds the same
                                     tables: one representative row per level through the cash row kernel, cell by cell in the
                                     reference's order, then one copy per state -- (nx + nq - 1) rows evaluated instead of
                                     nx nq.  EXACT; one rank only.
                                     STAFF (workforce): the lambdas read x and a through the hire-up-to level y = x + a only, so
                                     Q_t(x, a) = c(a) P_t(y) + G_t(y), c(a) = (a > 0 ? fixCost : 0) + unitVariCost a,
                                     G_t(y) = sum_{j < len(row)} p_row(j) w_t(y - j) + p_row(j) V_{t+1}(clamp(y - j)),
                                     row = min(y, rows - 1), w_t(n) = salary n + (n > minStaff_t ? 0 : unitPenalty (minStaff_t - n)),
                                     P_t(y) = the row's weights added in ascending j from 0.0: one serial sum per level and a
                                     scan, sum_levels len + S A steps a period instead of S A D.  REASSOCIATES the reference's
                                     sum: values within 1e-9 relative of the oracle's, the hire count may differ only where two
                                     actions tie to that rounding; tables bit-identical to tests/staff_separable_twin.py; an
                                     instance with fixCost = unitVariCost = salary = 0 is bit-identical to the oracle.  Rank
                                     slabs: each rank builds the levels its slab reaches.  Every other `kernel` value on a
                                     STAFF handle keeps the cell-by-cell kernels (reported as SDPGPU_KERNEL_GATHER). */

/*
 * Problem descriptor: everything the reference's lambdas close over.  Field names
 * follow the reference's variable names.  Inventory, action and demand values must
 * be integer multiples of `step` and `step` itself integer-valued (every in-scope
 * driver uses stepSize = 1), so that x + a - d is exact in fp64 as it is in Java.
 */
typedef struct sdpgpu_desc {
  int32_t abi_version; /* SDPGPU_ABI_VERSION */
  int32_t family;      /* sdpgpu_family */
  int32_t direction;   /* sdpgpu_direction */
  int32_t periods;     /* T = pmf.length */

  /* inventory axis */
  double step;               /* stepSize */
  double min_inventory;      /* minState / minInventory / minInventoryState */
  double max_inventory;      /* maxState / maxInventory / maxInventoryState */
  double max_order_quantity; /* maxOrderQuantity: actions 0, step, ...; count (int)(Q/step)+1 for BACKORDER / LEADTIME
                                (`new double[(int)(maxOrderQuantity/stepSize)+1]`, CLSPTesting.java:79), (int)Q+1 WHATEVER the
                                step for the cash families (`iterate(0, i -> i + stepSize).limit((int) maxQ + 1)`,
                                CashConstraint.java:99).  CASH_LEADTIME, whose order becomes the next state's preQ, therefore
                                needs step = 1 (SDPGPU_ERR_UNSUPPORTED otherwise), like cash_formula 2 and STAFF. */
  int32_t clamp_inventory;   /* 1: clamp as CLSP.java:257-258; 0: no clamp (Leadtime.java:65-66
                                has the clamp commented out) -> per-period boxes grown from ini_* */
  int32_t zero_order_last_period; /* SingleProductLeadtime.java:74-75: maxQ = 0 when period == T */

  /* period-1 initial state: bounding boxes of unclamped families, reachable-set filter */
  double ini_inventory;
  double ini_cash;
  double ini_preq;

  /* cost parameters (F1/F2) */
  double fixed_order_cost; /* fixedOrderingCost / fixOrderCost (K) */
  double unit_order_cost;  /* proportionalOrderingCost / variOrderingCost / variCost (v) */
  double holding_cost;     /* holdingCost (h) */
  double penalty_cost;     /* penaltyCost: backorder pi (F1/F2); endCash<0 multiplier (F3) */

  /* cash families (F3/F4/F5) */
  double price;
  double salvage_value;   /* applied only when period == T */
  double deposit_rate;    /* depositeRate (F3 formula 0) */
  double overhead_cost;   /* overheadCost, same every period unless sdpgpu_set_overhead */
  double overhead_rate;   /* overheadRate (F3 formula 0) */
  double discount_factor; /* CashRecursion.java:120: p * gamma * V, evaluated (p*gamma)*V */
  double min_cash;
  double max_cash;
  double cash_round_mult; /* Math.round(nextCash * mult) ... */
  double cash_round_div;  /* ... / div */
  int32_t cash_round_int_div; /* 1: `/ 10` long division (CashOverdraft.java:116); 0: `/ 10.0` */
  int32_t cash_formula;       /* F3: 0 CashConstraint.java:103-119, 1 CashConstraintTesting.java:117-132,
                                 2 CashConstraintXR.java:91-105 (state (x, R), order-up-to actions) */

  /* overdraft interest schedule (F4/F5): CashOverdraft.java:86-95 */
  double r0;
  double r2;
  double r3;
  double overdraft_limit;
  double interest_free_amount;

  /* execution */
  int32_t kernel;      /* SDPGPU_KERNEL_* */
  int32_t device;      /* HIP device ordinal, -1 = current device */
  int32_t rank;        /* state-axis slab owned by this handle: rank of world_size */
  int32_t world_size;  /* 1 = whole grid */
  int32_t store_all_values; /* 1: keep V_t for every t (values query); 0: two ping-pong tables */
  int32_t lead_time;   /* LEADTIME family only: 0 or 1 = the reference's lead time 1 (Leadtime.java); 2 = two-stage
                          pipeline, state (x, q1, q2), needs clamp_inventory = 1 */
  double ini_preq2;    /* lead_time 2: q2 of the period-1 state (ini_preq is q1) */
  double reserved1;
} sdpgpu_desc;

typedef struct sdpgpu_stats {
  int64_t states_total;     /* sum over periods of grid states (whole grid, all ranks) */
  int64_t cells_evaluated;  /* sum over periods and THIS rank's states of nA(s) * D_t: the cells of the grid DECIDED.  Where the
                               F1 level kernel stops level blocks early (f1_level_steps_run below) not all of them are
                               walked to their last demand step; fp64_ops_executed counts what ran. */
  int64_t cells_all_ranks;  /* the same over the whole grid */
  double  solve_ms;         /* HIP-event time of the last sdpgpu_solve on its stream */
  double  kernel_ms_sum;    /* sum of per-period kernel times when profiling is on, else 0 */
  int32_t periods_run;
  int32_t kernel_used;      /* SDPGPU_KERNEL_* actually launched for the last period run */
  int32_t window_r;         /* F1 window kernel: actions per register block ... */
  int32_t window_s;         /* ... and adjacent states per lane of the plan used for period 1 (0: other kernel) */
  double  fp64_ops_executed; /* sum over periods of THIS rank's cells x the fp64 add/mul operations the kernel that ran
                                the period executes per cell (the reference's five per cell minus the ones that are the
                                same operation on the same operands in neighbouring cells and are formed once; window
                                and uniform-shift kernels).  0 when a period ran a kernel without such a model. */
  double  lds_bytes;        /* ABI 4: bytes THIS rank's cells moved through the LDS (reads and staging writes) and through the */
  double  l1_bytes;         /* vector L1 (per-cell gathers, staging loads), by the same per-kernel models; 0 where a kernel has
                               none.  bench.py prices the kernels these units bind (cash_diag_kernel: LDS; cash_shift_kernel: L1)
                               against 128 and 64 B/clk/CU. */
  int64_t graph_replays;    /* ABI 5: sdpgpu_solve calls served by ONE hipGraphLaunch of the captured sweep.  Opt-in, environment
                               SDPGPU_GRAPH=1 (the first call runs eagerly, the second is captured while it is enqueued, later
                               calls replay; per-period profiling, user functors and the legacy NULL stream run eagerly).  Off
                               by default: replay measured 0.6-1.6 % SLOWER than the eager sweep on ROCm 7.2. */
  int64_t f1_level_steps_planned; /* Additive to ABI 6.  Periods run by the F1 level kernel (window_f1_level_kernel): demand steps */
  int64_t f1_level_steps_run;     /* of level blocks, summed over waves -- what the launches planned, and what their waves walked.
                               run < planned where the cut-off stopped blocks no action of which could still win (MIN, built-in
                               costs, K, v, h, pi >= 0, probabilities >= 0: every running sum is a lower bound of its cell;
                               DESIGN.md).  run == planned with SDPGPU_F1_CUTOFF=0 or an instance the cut-off does not cover;
                               both 0 when no period ran that kernel.  Values and policy are the same bits either way.
                               NOTE: these two fields grew sizeof(sdpgpu_stats) by 16 bytes WITHIN ABI 6 (the version number is
                               unchanged): sdpgpu_stats_get clears and writes the whole struct through the caller's pointer, so
                               every caller compiled against an earlier ABI 6 header must be rebuilt against this one. */
} sdpgpu_stats;

typedef struct sdpgpu_handle sdpgpu_handle;

/* Library identity: returns SDPGPU_ABI_VERSION. */
int sdpgpu_abi_version(void);

/* ABI 6.  Identity of the BINARY: the 16-hex-digit digest of the sources it was built from (every file of csrc/, this
 * header and build.py with its flags -- tools/kernel_sha.py: build_source_sha), baked in at build time by build.py.  The
 * shipped libsdpgpu.so is a prebuilt artefact (git-ignored, carried to the GPU box with the tree): __graft_entry__.smoke()
 * and every bench line compare this string with the digest of the tree they run from, and a mismatch fails smoke.
 * "unknown" when the library was compiled by hand without -DSDPGPU_BUILD_ID.  The reference has no counterpart (a JVM
 * runs the classes it was given: Recursion.java has no native half). */
const char* sdpgpu_build_id(void);

/* Fill a descriptor with the defaults the reference drivers use (discount 1,
 * rounding 10/10.0, clamp on, world 1, store all values, kernel auto). */
void sdpgpu_desc_init(sdpgpu_desc* d);

/* Validate the descriptor, lay out the per-period grids, allocate device tables. */
int sdpgpu_create(const sdpgpu_desc* desc, sdpgpu_handle** out);
void sdpgpu_destroy(sdpgpu_handle* h);

/*
 * User-defined lambdas.  The reference injects a problem as three Java lambdas (Recursion.java:49-52):
 * `Function<State, double[]>` feasible actions, StateTransitionFunction (StateTransition.java:20-22) and
 * ImmediateValueFunction (ImmediateValue.java:23-25).  The built-in families cover the in-scope drivers; any
 * other driver's lambdas are handed over here as HIP device source, compiled at this call with hipRTC for gfx950
 * under the library's numerics contract (-ffp-contract=off) around the same loop (accumulation order,
 * strict-compare arg-opt, discount, survival objective) as the built-in kernels.
 *
 * `functor_source` defines exactly these three device functions (the text may define helpers and constants too):
 *
 *   __device__ int    sdp_feasible_count(const sdp_ctx& c, double x, double cash, double preq);
 *       getFeasibleActions.apply(state).length; action k is k * c.step (DoubleStream.iterate(0, i -> i + stepSize))
 *   __device__ double sdp_immediate(const sdp_ctx& c, double x, double cash, double preq, double action, double demand);
 *       immediateValue.apply(state, action, randomDemand)
 *   __device__ void   sdp_transition(const sdp_ctx& c, double x, double cash, double preq, double action, double demand,
 *                                    double& next_x, double& next_cash, double& next_preq);
 *       stateTransition.apply(state, action, randomDemand), clamped and rounded as the Java lambda does it: the
 *       result must be a grid point of the next period, otherwise the next read of results fails with
 *       SDPGPU_ERR_ARG.
 *
 * ABI 5, optional: a text that also says `#define SDP_USER_CELL 1` and defines
 *   __device__ void   sdp_cell(const sdp_ctx& c, double x, double cash, double preq, double action, double demand,
 *                              double& imm, double& next_x, double& next_cash, double& next_preq);
 * gives the period kernel ONE callback per cell: imm = immediateValue.apply(...) and the successor of the same cell.  The
 * reference's cash-type transitions call immediateValue again (CashConstraint.java:125 `nextCash = cash +
 * immediateValue.apply(...)`); as two functions the increment is spelled out twice per cell.  sdp_immediate and
 * sdp_transition are still required (the reachable-set pass and sdpgpu_eval_states' host twins use them); the
 * natural way to write them is as calls of sdp_cell.
 *
 * ABI 6, optional -- the LEVEL SHAPE: a text that says `#define SDP_SHAPE_LEVEL 1` and defines, INSTEAD of the three lambdas,
 *   __device__ double sdp_action_cost(const sdp_ctx& c, double action);
 *   __device__ double sdp_level_cost(const sdp_ctx& c, double level);
 * declares its lambdas to be
 *   immediateValue  = sdp_action_cost(action) + sdp_level_cost(x + action - demand)      (one addition of the two terms),
 *   stateTransition = x + action - demand, clamped to [min_inventory, max_inventory] as the descriptor says (upper, then lower),
 *   feasible actions = every order 0, step, ... max_order_quantity in every state
 * -- the shape of capacitated.CLSP's lambdas (CLSP.java:251-272) and of the period-1-special second Recursion of CLSPforDraw
 * (CLSPforDraw.java:146-169), with any piecewise, period-dependent costs inside the two functions.  desc->family must be
 * BACKORDER.  The library compiles the two functions with hipRTC, lets them tabulate M(level) and c(action) for every period
 * once (kernel sdp_custom_tabulate), and runs its F1 window kernel from the tables: arbitrary cost closures at the built-in
 * family's speed, and -- each table entry being the user's function of the very level / action the reference would hand it,
 * joined by the one declared addition -- the tables' values are the reference's doubles.  kernel = SDPGPU_KERNEL_GATHER (and
 * sdpgpu_eval_states, sdpgpu_reachable) run the same text through the generic loop; the library forms the three lambdas from
 * the two functions as stated above.
 *
 * with `struct sdp_ctx { int period; int T; double step; const double* params; }` (period = state.getPeriod(),
 * params = the n_params doubles given here: the constants the Java lambdas close over) and the helpers
 * sdp_max / sdp_min / sdp_round / sdp_trunc (java.lang.Math.max / min / round and the (int) cast) and, ABI 6, sdp_ldiv(a, b)
 * (Java's `long / int` on an integer-valued double below 2^31, e.g. `Math.round(cash * 10) / 10`, CashOverdraft.java:116: truncating
 * integer division -- a few integer instructions with a literal divisor, where sdp_trunc(a / b) is an fp64 division per cell).
 *
 * `desc->family` selects the STATE SHAPE and the loop, not the formulas: BACKORDER = (x) under Recursion,
 * LEADTIME = (x, preQ) under LeadtimeRecursion, CASH / OVERDRAFT = (x, cash) under CashRecursion (discounted),
 * CASH_LEADTIME = (x, cash, preQ), SURVIVAL = (x, cash) under getSurvProb.  The grid fields of the descriptor
 * (step, inventory bounds and clamp flag, cash bounds and rounding, max_order_quantity = longest pipeline
 * quantity, ini_*) keep their meaning; the cost fields are ignored.  sdpgpu_simulate is not available (the
 * lambdas also exist on the host, where the reference's simulators call them); the device rollouts of such a handle are
 * entry points of their own: sdpgpu_custom_simulate, sdpgpu_custom_simulate_sampled, sdpgpu_custom_rule_simulate (below).
 *
 * How the text is compiled: -O3, no contraction, no fast-math.  On a CLAMPED grid with finite constants the grid, the step and
 * params[] are baked into the generated source as exact literals (SDPGPU_CUSTOM_BAKE=0: read at run time, as before ABI 6), and
 * that compile additionally assumes the lambdas' arithmetic produces no NaN (-fno-honor-nans; SDPGPU_CUSTOM_NNAN=0 turns it
 * off): a clamp the Java source spells `x > c ? c : x` against a non-zero constant then costs one v_min_f64 instead of a compare
 * and two selects.  For lambdas whose values are numbers the results are the same doubles either way
 * (tests/test_gpu_custom_functor.py runs the three modes against each other); what a lambda that does produce a NaN returns is
 * unspecified in the default mode.  With NaNs honoured, and on every grid that is not baked, it is Java's: the action is skipped
 * (tests/test_gpu_custom_functor.py, test_nan_lambda_*).
 */
int sdpgpu_create_custom(const sdpgpu_desc* desc, const char* functor_source, const double* params, int32_t n_params,
                         sdpgpu_handle** out);

/* Never NULL; empty string when the last call on h succeeded.  h may be NULL to
 * read the message of a failed sdpgpu_create. */
const char* sdpgpu_last_error(const sdpgpu_handle* h);

/* pmf[t] for t = 0..T-1 (period t+1): n pairs, demand[j] ascending as in GetPmf.java:119. */
int sdpgpu_set_pmf(sdpgpu_handle* h, int32_t t, const double* demand, const double* prob, int32_t n);

/* STAFF family: the turnover pmf of period t+1 per hire-up-to level, pmfs[t] of StaffRecursion.java:23,92-95.
 * prob[y * row_stride + j] = pmfs[t][y][j][1] for j < row_len[y] (the realisation pmfs[t][y][j][0] is j itself,
 * WorkforcePlanning.java:57-68); row_len NULL means y + 1 entries per row; a level beyond the table uses its last
 * row.  1 <= row_len[y] <= min(y + 1, row_stride): a realisation never exceeds the staff it applies to. */
int sdpgpu_set_level_pmf(sdpgpu_handle* h, int32_t t, const double* prob, const int32_t* row_len, int32_t n_rows,
                         int32_t row_stride);

/* ---- PMF construction: what a driver runs immediately before the recursion ---------------------
 * `new GetPmf(distributions, truncationQuantile, stepSize).getpmf()[t]` (sdp/inventory/GetPmf.java:82-134; variant
 * SDPGPU_PMF_GETPMF) and capacitated.CLSP.main's inline variant (CLSP.java:219-247; SDPGPU_PMF_CLSP), for the
 * distributions the in-scope drivers use.  GetPmf's structure and quirks are reproduced exactly ((int) truncation of the
 * quantiles, lower bound 0 for integer distributions, prob(j) indexed by position, covered mass as normaliser); the
 * cdf / quantile functions are this library's own double-precision implementations, not SSJ's (parity unpinned at this
 * boundary: the reference records no PMF).  Host arithmetic, no GPU needed.
 * Call with capacity = 0 to learn the number of points of period t (n_out), then with arrays of that size; feed the
 * result to sdpgpu_set_pmf.  Errors through sdpgpu_last_error(NULL). */
#define SDPGPU_DIST_POISSON 1      /* PoissonDist(lambda = a) */
#define SDPGPU_DIST_NORMAL 2       /* NormalDist(mu = a, sigma = b) */
#define SDPGPU_DIST_UNIFORM_INT 3  /* UniformIntDist(i = a, j = b) */
#define SDPGPU_DIST_GAMMA 4        /* GammaDist(alpha = a, lambda = b): shape, RATE (CashConstraintXR.java:67) */
#define SDPGPU_PMF_GETPMF 0
#define SDPGPU_PMF_CLSP 1
typedef struct sdpgpu_dist_spec {
  int32_t kind;
  int32_t reserved;
  double a, b;
} sdpgpu_dist_spec;
int sdpgpu_getpmf(const sdpgpu_dist_spec* distributions, int32_t T, double truncation_quantile, double step,
                  int32_t variant, int32_t t, double* demand, double* prob, int32_t capacity, int32_t* n_out);

/* Optional per-period overhead cost (CashOverdraft.java:38-39 keeps an array).  STAFF family: minStaffNum[t]. */
int sdpgpu_set_overhead(sdpgpu_handle* h, int32_t t, double overhead_cost);

/* Optional: the caller's own action-list LENGTHS.  The reference's `Function<State, double[]> getFeasibleAction`
 * (Recursion.java:49,129) may return any array; every in-scope driver returns a prefix 0, step, 2 step, ... of the
 * action grid whose length follows one of the families' closed forms.  A driver whose list is still such a prefix but
 * with a length of its own (a storage capacity Q <= cap - x, a budget table, ...) hands the lengths over here:
 * counts[i] = getFeasibleAction.apply(state i of period t+1).length for every grid state i (flat index order,
 * n = sdpgpu_num_states), 0 <= counts[i] <= the family's longest list (see max_order_quantity); 0 = no feasible action (the value is
 * then +-Double.MAX_VALUE and the action 0, Recursion.java:132-134).  Such a period runs on the generic kernel (the
 * specialised kernels build on the family's rule).  sdpgpu_eval_states ALWAYS applies the family's rule -- to off-grid
 * states (the caller's list is defined on grid states only) and to on-grid states alike, so for a grid state whose count was
 * overridden here its answer may differ from sdpgpu_values / sdpgpu_policy of the same state: read those for grid states.
 * Before the first run.  Lists that are not prefixes of the action grid need sdpgpu_create_custom. */
int sdpgpu_set_action_counts(sdpgpu_handle* h, int32_t t, const int32_t* counts, int64_t n);

/* Launch kernels on a caller-owned hipStream_t (NULL = the legacy default stream).  Without this
 * call the library creates a non-blocking stream of its own. */
int sdpgpu_set_stream(sdpgpu_handle* h, void* hip_stream);

/* Record a HIP event pair around every period kernel (read back through sdpgpu_period_ms). */
int sdpgpu_set_profiling(sdpgpu_handle* h, int32_t on);

/* ---- geometry ---------------------------------------------------------------------------- */
/* Number of grid states of period t (1-based period, 1..T). */
int64_t sdpgpu_num_states(const sdpgpu_handle* h, int32_t period);
/* Padded row length of the V_t table (multiple of world_size) and this rank's slab [lo, hi). */
int sdpgpu_slab(const sdpgpu_handle* h, int32_t period, int64_t* padded, int64_t* lo, int64_t* hi);
/* Grid of period t: x = x_lo + i*step (i < nx); cash index ic < nc; preQ index iq < nq.
 * Flat index = (iq * nx + ix) * nc + ic.  With lead_time 2 the pipeline axis is the pair
 * iq = iq2 * nq1 + iq1 and sdpgpu_grid reports nq = nq1 * nq2; sdpgpu_grid2 reports both. */
int sdpgpu_grid(const sdpgpu_handle* h, int32_t period, double* x_lo, int64_t* nx, int64_t* nc, int64_t* nq);
int sdpgpu_grid2(const sdpgpu_handle* h, int32_t period, double* x_lo, int64_t* nx, int64_t* nc, int64_t* nq1,
                 int64_t* nq2);
/* Cash value of cash index ic (k / div, exactly the double the reference's rounding yields). */
double sdpgpu_cash_value(const sdpgpu_handle* h, int64_t ic);
/* Dense index of a state tuple in period t, or -1 if it is not a grid point. */
int64_t sdpgpu_state_index(const sdpgpu_handle* h, int32_t period, double x, double cash, double preq);
/* The same with the second pipeline quantity (lead_time 2; preq2 must be 0 otherwise). */
int64_t sdpgpu_state_index2(const sdpgpu_handle* h, int32_t period, double x, double cash, double preq, double preq2);

/* ---- solving ----------------------------------------------------------------------------- */
/* Whole backward sweep t = T..1 on this handle (world_size must be 1).  Asynchronous on the
 * handle's stream unless `sync` != 0. */
int sdpgpu_solve(sdpgpu_handle* h, int32_t sync);
/* One period for this rank's slab, reading the FULL V_{period+1} table.  With world_size > 1
 * the caller all-gathers V_period (device pointer below) across ranks before the next call.
 * With store_all_values = 0, V_period is written into table (period & 1): every other period of that parity stops existing
 * (V_{period+2} inside a sweep; V_{period-2} of an earlier sweep when a period is run again), and whatever reads one of them
 * -- sdpgpu_values, sdpgpu_eval_states, a rollout from a start off the grid, sdpgpu_run_period of the period below -- answers
 * SDPGPU_ERR_STATE until it has been run again. */
int sdpgpu_run_period(sdpgpu_handle* h, int32_t period);
/* The same in two halves, so that a sharded caller can overlap the all-gather of V_{period+1} with
 * compute: INTERIOR = the states all of whose cells read only THIS rank's slab of V_{period+1} (it may
 * run while the exchange is in flight; empty for families without a bounded footprint), BOUNDARY = the
 * rest (after the exchange).  INTERIOR followed by BOUNDARY equals sdpgpu_run_period. */
#define SDPGPU_PART_ALL 0
#define SDPGPU_PART_INTERIOR 1
#define SDPGPU_PART_BOUNDARY 2
int sdpgpu_run_period_part(sdpgpu_handle* h, int32_t period, int32_t part);
/* Fewer exchanges on small slabs: the backorder family on the window kernel reads a BOUNDED neighbourhood of
 * V_{period+1} -- state i needs [i - left, i + right] (sdpgpu_footprint; SDPGPU_ERR_UNSUPPORTED when the family has
 * no such bound).  A sharded caller can therefore run K periods between two exchanges by computing period t on its
 * slab widened by the footprints of the periods still to come in the block (sdpgpu_run_period_range; the widening is
 * redundant work that reproduces the neighbours' values bit for bit), and all-gather only to publish the rows.
 * sdpgpu_set_halo (before the first run) announces the largest widening so that the scratch rows are sized for
 * it.  Values are written for the whole range, policy indices only for this rank's own slab. */
int sdpgpu_footprint(const sdpgpu_handle* h, int32_t period, int64_t* left, int64_t* right);
int sdpgpu_set_halo(sdpgpu_handle* h, int64_t halo);
int sdpgpu_run_period_range(sdpgpu_handle* h, int32_t period, int64_t lo, int64_t hi);
/* Device address of the V_period table (padded row, fp64) -- for the in-place all-gather. */
void* sdpgpu_values_device_ptr(sdpgpu_handle* h, int32_t period);
/* Use caller-owned device memory for the value tables: `bytes` >= sdpgpu_values_bytes(h). */
size_t sdpgpu_values_bytes(const sdpgpu_handle* h);
int sdpgpu_attach_values(sdpgpu_handle* h, void* device_ptr, size_t bytes);
/* The row a sharded caller all-gathers after sdpgpu_run_period(period) and before the next period:
 * padded_row 8-byte elements (sdpgpu_slab).  Usually the fp64 V_period row; on small grids, where a
 * tile is shared by several tasks, the row of order-preserving uint64 keys the kernels reduce into and
 * the next period reads directly (the fp64 row is then written by sdpgpu_finalize).  The key arena can be
 * caller memory, like the value arena: sdpgpu_keys_bytes() is 0 when the handle never uses keys. */
void* sdpgpu_exchange_ptr(sdpgpu_handle* h, int32_t period);
size_t sdpgpu_keys_bytes(const sdpgpu_handle* h);
int sdpgpu_attach_keys(sdpgpu_handle* h, void* device_ptr, size_t bytes);

/* Enqueue (do not wait for) whatever deferred read-out work is outstanding, so that in stream order every
 * V_t and policy row of the periods run so far is complete.  On small grids the window kernel leaves
 * the arg-opt of a period as per-chunk rows and resolves all periods in one launch; every reader
 * below does this implicitly, a caller that reads the device tables itself calls it explicitly. */
int sdpgpu_finalize(sdpgpu_handle* h);
/* sdpgpu_finalize, then block until everything queued on the handle's stream has finished. */
int sdpgpu_synchronize(sdpgpu_handle* h);

/* ---- multi-GPU: the state axis sharded over the GPUs of one node ------------------------------------------
 * The reference's contract is "one call solves everything" (`getExpectedValue(initialState)`,
 * Recursion.java:89); with the state axis cut into world_size slabs that call becomes a sweep of per-slab period
 * kernels with ONE all-gather of V_t between periods (RCCL over xGMI, in place in the row the next period reads,
 * issued by this library -- no Python or torch in the data path).  Two ways to drive it:
 *
 *  (1) one process (or thread) per GPU:  every rank creates its handle with desc.rank / desc.world_size /
 *      desc.device, ONE rank calls sdpgpu_comm_unique_id and hands the 128 bytes to the others by whatever channel
 *      the host has (a file, a socket, MPI, torch.distributed's store), every rank calls sdpgpu_comm_prepare (local:
 *      device tables, RCCL load) and the ranks agree that all succeeded, every rank calls sdpgpu_comm_init (collective:
 *      ncclCommInitRank), then sdpgpu_solve_sharded.
 *  (2) one process that owns all the GPUs (a JVM calling through JNI): one handle per device, all in this process,
 *      and ONE call sdpgpu_solve_multi(handles, n, ...) -- the library builds the communicators itself
 *      (ncclCommInitAll), drives every device from the calling thread and groups the per-period all-gathers
 *      (default), or starts one host thread per rank (SDPGPU_SHARDED_THREADS: for slabs whose periods take tens of
 *      microseconds, where the launches of eight devices issued from one thread would queue up on the host).
 *      Handles that SHARE a device (a rehearsal of N ranks on one GPU) exchange their slabs by device-to-device
 *      copies instead, since RCCL refuses two ranks on one device; the slab arithmetic and results are the same.
 *
 * RCCL is loaded on first use (dlopen of librccl.so.1): a single-GPU caller never pays for it.  RCCL failures come
 * back as SDPGPU_ERR_DEVICE with ncclGetErrorString's text.  Policy tables stay sharded (sdpgpu_policy reads this
 * rank's slab); after the sweep every rank holds every full V_t with t >= 2, and V_1 complete only on its own slab
 * unless `gather_first` is set. */
#define SDPGPU_UNIQUE_ID_BYTES 128
int sdpgpu_comm_unique_id(void* out_id /* SDPGPU_UNIQUE_ID_BYTES */);
/* ABI 5.  The part of sdpgpu_comm_init that can fail on one rank ALONE (device tables do not fit, no device, RCCL does
 * not load), without entering a collective.  Call it on every rank, let the ranks agree over the host's channel that
 * all returned SDPGPU_OK, and only then call sdpgpu_comm_init: a rank that fails here has not left its peers blocked
 * inside ncclCommInitRank.  (sdpgpu_comm_init does the same work itself when this call was skipped.) */
int sdpgpu_comm_prepare(sdpgpu_handle* h);
/* Collective over the `world` ranks; rank / world must equal the handle's desc.rank / desc.world_size.  world = 1 is
 * allowed (a one-rank communicator: the collective path with nobody to talk to -- used by the tests). */
int sdpgpu_comm_init(sdpgpu_handle* h, const void* unique_id, int32_t rank, int32_t world);
int sdpgpu_comm_destroy(sdpgpu_handle* h);
/* The all-gather of the row of `period` alone (sdpgpu_exchange_ptr), enqueued on the handle's stream behind the
 * period's kernel -- for a caller that steps the periods itself with sdpgpu_run_period. */
int sdpgpu_exchange(sdpgpu_handle* h, int32_t period);
/* Whole backward sweep t = T..1 of this rank's slab with the exchanges in between; every rank calls it.
 * flags: SDPGPU_SHARDED_SYNC        wait for the stream before returning (else asynchronous, like sdpgpu_solve)
 *        SDPGPU_SHARDED_OVERLAP     run the all-gather of V_{t+1} on a second stream beside the INTERIOR part of
 *                                   period t (families with a bounded footprint; otherwise same as blocking)
 *        SDPGPU_SHARDED_GATHER_FIRST  also all-gather V_1 (needed only if every rank wants the whole V_1) */
#define SDPGPU_SHARDED_SYNC 1
#define SDPGPU_SHARDED_OVERLAP 2
#define SDPGPU_SHARDED_GATHER_FIRST 4
#define SDPGPU_SHARDED_THREADS 8 /* ABI 5, sdpgpu_solve_multi only: one host thread per rank (see there) */
int sdpgpu_solve_sharded(sdpgpu_handle* h, int32_t flags);
/* Way (2): handles[r] is the handle of rank r (desc.rank = r, desc.world_size = n, any devices; all n describing the
 * same problem -- family, grids, pmf sizes -- else SDPGPU_ERR_ARG).  The communicators are created at the first call
 * and kept in the handles.  Errors are reported on handles[0].  The calling thread's current device is restored. */
int sdpgpu_solve_multi(sdpgpu_handle** handles, int32_t n, int32_t flags);

/* ---- results ----------------------------------------------------------------------------- */
/* Copy V_period[0..n) to host (n <= num_states). */
int sdpgpu_values(sdpgpu_handle* h, int32_t period, double* out, int64_t n);
/* Copy this rank's slab of the arg-opt action INDEX table (action = index * step). */
int sdpgpu_policy(sdpgpu_handle* h, int32_t period, int32_t* out, int64_t lo, int64_t n);
/* Evaluate arbitrary states of period t against V_{t+1}: out_value/out_action_index get n entries. */
int sdpgpu_eval_states(sdpgpu_handle* h, int32_t period, int64_t n, const double* x, const double* cash,
                       const double* preq, double* out_value, int32_t* out_action_index);
/* The same with the second pipeline quantity per state (lead_time 2; preq2 may be NULL = zeros). */
int sdpgpu_eval_states2(sdpgpu_handle* h, int32_t period, int64_t n, const double* x, const double* cash,
                        const double* preq, const double* preq2, double* out_value, int32_t* out_action_index);
/* Reachable-set mask of period t (1 byte per state), forward-propagated from the ini_* state over
 * all feasible actions and all demands -- the key set the memoised recursion would build. */
int sdpgpu_reachable(sdpgpu_handle* h, int32_t period, uint8_t* out, int64_t n);

/* Roll the computed policy forward along n demand paths: the inner loops of
 * Simulation.simulateSDPGivenSamplNum (Simulation.java:59-69) and CashSimulation (CashSimulation.java:101-112)
 * as a batched table-lookup rollout, one path per lane.  demand[i*T + t] is the realised demand of path i in
 * period t+1, already rounded by the caller as the reference does (Math.round, Simulation.java:64);
 * discount[t] multiplies the immediate value of period t+1 (Math.pow(discountFactor, t) in CashSimulation,
 * all 1.0 for the undiscounted classes).  out_sum[i] = sum_t discount[t] * imm_t; out_valid[i] = 0 when
 * the path left the grid (possible only for unclamped families with demands outside the PMF support).
 * The start state is (1, ini_x, ini_cash, ini_preq[, desc.ini_preq2 with lead_time 2]); world_size must be 1.
 * Family SURVIVAL rolls RiskSimulation.simulateLostSale instead (RiskSimulation.java:213-234): out_sum[i] = 1 when
 * path i held negative cash at some point (else 0), bit 1 of out_valid[i] is set when a demand was lost on it, and
 * the order is forced to 0 in a state with negative cash; `discount` is ignored. */
int sdpgpu_simulate(sdpgpu_handle* h, int64_t n_paths, const double* demand, const double* discount, double ini_x,
                    double ini_cash, double ini_preq, double* out_sum, uint8_t* out_valid);

/* Host arithmetic, except: after a solve in which the F1 level kernel ran with its cut-off, the steps its waves walked are
 * read from the device -- the call then waits for the handle's stream (hipStreamSynchronize) and copies a few bytes back, so
 * a caller that polls the statistics between enqueued solves serialises on the stream.  (It also waits for the stream to read
 * solve_ms and a user functor's cell counts.) */
int sdpgpu_stats_get(sdpgpu_handle* h, sdpgpu_stats* out);

/* ABI 5: the launch plan of one period of THIS rank's slab, as the launcher would choose it now (descriptor, pmfs,
 * world size and the SDPGPU_WIN_* overrides read at create time).  Host arithmetic only: no device is touched, so a
 * caller (or a test without a GPU) can see what a period will cost in LDS before it runs.  Reported for the window
 * kernels of the backorder family (F1) and for the row-window kernel of the lead-time family (F2: a period that would run
 * it -- kernel AUTO or WINDOW, a unit-stride demand layout, no action counts of the caller's; r x s is the instantiation,
 * chunk_blocks the register blocks a chunk's waves walk, tiles the row tiles of 64 s states that cover the slab -- the
 * launcher and this call ask one function); other kernels return kernel = SDPGPU_KERNEL_GATHER and zeros.  A plan that
 * cannot run -- a forced register block that does not exist, a forced chunking that exceeds the 160 KiB of LDS of a
 * compute unit, chunk rows where ping-pong tables forbid them, an F2 period whose row segments exceed that LDS under a
 * forced block or kernel = WINDOW -- returns SDPGPU_ERR_ARG with the reason in sdpgpu_last_error, which is also what
 * sdpgpu_run_period then returns (before anything is launched); under the automatic choice with nothing forced such a
 * period runs on, and is reported as, the generic kernel.
 * A handle of the STAFF family reports the form launch_staff would run (the launcher and this call ask one function; the
 * SDPGPU_STAFF_* switches are read at create time): kernel = SDPGPU_KERNEL_GATHER, as sdpgpu_stats reports it; r = actions per
 * register block (64: the lanes of a wave are 64 actions of one state, 1: the plain one-action-at-a-time kernel, else 4 or 8);
 * s = adjacent states per lane (1, 2 for the pair kernel, 2 or 4 for the window kernel); chunks = action groups per state tile;
 * chunk_blocks = trips of a group's action loop (actions per group / r); tiles = state tiles of this slab (64 s states, one
 * state when r = 64), tasks = tiles x chunks = the launch's workgroups; lds_bytes = the window kernel's static LDS, 0 for every
 * other form (which tells the window kernel from the pair kernel at s = 2); workgroups_per_cu = 0.
 * A STAFF handle with kernel = SDPGPU_KERNEL_SEPARABLE reports that mode's scan launch instead: kernel =
 * SDPGPU_KERNEL_SEPARABLE, r = s = chunks = 1, chunk_blocks = 0, tiles = tasks = the workgroups of 64 states of this slab,
 * lds_bytes = their static LDS (the G(y) launch before it has one lane per level and no LDS). */
typedef struct sdpgpu_plan {
  int32_t kernel;            /* SDPGPU_KERNEL_WINDOW or SDPGPU_KERNEL_GATHER (STAFF in its opt-in mode: SDPGPU_KERNEL_SEPARABLE) */
  int32_t r, s;              /* register block: actions x adjacent states per lane */
  int32_t chunks;            /* tasks per state tile (1: no chunk rows, no key atomics, no finalize pass) */
  int32_t chunk_blocks;      /* register blocks of the action axis per task; 0: the action-major level kernel, whose
                                tasks are level bands x blocks of 64 r actions */
  int32_t tiles, tasks;      /* state tiles of 64 s states of this slab; tiles x chunks (level kernel: bands; tasks) */
  int32_t workgroups_per_cu; /* workgroups (four tasks each) the LDS lets a compute unit hold at once (level kernel: at
                                most the two its registers allow, which its bands are planned against) */
  int64_t lds_bytes;         /* dynamic LDS per workgroup */
} sdpgpu_plan;
int sdpgpu_plan_period(const sdpgpu_handle* h, int32_t period, sdpgpu_plan* out);

/* ---- reachable-set engine for the two-product lead-time family -------------------------------------
 * Replaces `new CashRecursionMultiLead(...).getExpectedValue(iniState)` / getAction
 * (src/sdp/cash/multiItem/CashRecursionMultiLead.java:31-95) for the lambdas of
 * src/cash/overdraft/MultiProductLeadtime.java:150-223 with DiscreteDistribution demands
 * (GetPmfMulti.java:157-172).  The state (I1, I2, preQ1, preQ2, cash) carries an un-rounded cash balance,
 * so there is no grid: the engine enumerates the reachable set level by level on the GPU, as the
 * reference's memoised recursion does on the host.  This is the family whose outputs the reference records
 * (MultiProductLeadtime.java:30-50). */
typedef struct sdpgpu_multilead {
  int32_t T;       /* horizon (TLength) */
  int32_t q_bound; /* actions (i, j), i, j in [0, Qbound) */
  double price[2], vari_cost[2], sal_value[2];
  double ini_cash, ini_i1, ini_i2;
  double r0, r1, r2, limit, interest_free;
  double min_inventory, max_inventory, min_cash, max_cash;
  double discount;
  double overhead[16]; /* overheadCost[t] */
  int32_t n1, n2;      /* demand points per product */
  double v1[16], p1[16], v2[16], p2[16];
  int32_t cash_int_cast; /* 1: `nextCash = (int) nextCash` (MultiProductLeadtime.java:219, commented out in the file as it
                            stands: "rounding states to save computing time") */
  int32_t reserved;
} sdpgpu_multilead;

/* final_value = iniCash + V_1(iniState) (MultiProductLeadtime.java:234), (q1, q2) = getAction(iniState);
 * states_per_period (T entries, may be NULL) = size of the reachable set per period, cells = (state, action,
 * demand) evaluations, gpu_ms = device time of expansion + recursion. */
int sdpgpu_multilead_solve(const sdpgpu_multilead* k, double* final_value, int32_t* q1, int32_t* q2,
                           int64_t* states_per_period, int64_t* cells, double* gpu_ms);
const char* sdpgpu_multilead_last_error(void);

/* Read-out of the whole memo of the two-product solvers -- what getCacheActions() / getOptTable() iterate
 * (CashRecursionMulti.java:140-168, CashRecursionMultiLead.java:92-101): register a table before a solve
 * (sdpgpu_multi_set_table, per thread; NULL clears it) and the next sdpgpu_multi*_solve of that thread fills it with one
 * row per visited state: period, the state tuple (q1 = q2 = 0 outside the lead-time family; `cash` holds R for the XR
 * family), V(state), and the chosen action pair (order-up-to levels for the XR family).  `rows` receives the number of
 * visited states; nothing is written when it exceeds `capacity` (call again with larger arrays).  Rows are grouped by
 * period, in no particular order inside a period. */
typedef struct sdpgpu_multi_table {
  int64_t capacity;
  int64_t rows;
  int32_t* period;
  double* i1;
  double* i2;
  double* q1;
  double* q2;
  double* cash;
  double* value;
  int32_t* a1;
  int32_t* a2;
} sdpgpu_multi_table;
void sdpgpu_multi_set_table(sdpgpu_multi_table* table);

/* Which kernel forms the calling thread's last sdpgpu_multi*_solve launched: one bit per launch site of the reachable-set
 * engine, OR-ed over the periods of that solve (0 after a solve that launched nothing).  The engine picks a form per period
 * from the instance's shape (and the SDPGPU_MULTI_* environment switches); a test that means to exercise one reads here
 * that it ran.  Host bookkeeping only: no kernel reads or writes it. */
#define SDPGPU_MULTI_FORM_SORTED_FORWARD 0x0001u /* forward pass over hash-sorted candidates (expand / sort / scatter) */
#define SDPGPU_MULTI_FORM_LATTICE_MARK 0x0002u   /* lattice_mark_kernel: the transition lambda per (state, action, pair) */
#define SDPGPU_MULTI_FORM_FACT_MARK 0x0004u      /* backward_fact_kernel as the lattice's marking pass (LK = 3) */
#define SDPGPU_MULTI_FORM_TRIPLES_MARK 0x0008u   /* XR family: marking through the distinct post-order triples */
#define SDPGPU_MULTI_FORM_FACT_LAST 0x0010u      /* backward_fact_kernel, period T (no successor) */
#define SDPGPU_MULTI_FORM_FACT_UID 0x0020u       /* backward_fact_kernel, LK = 0: successor ids stored per candidate */
#define SDPGPU_MULTI_FORM_FACT_RANK 0x0040u      /* backward_fact_kernel, LK = 1: the lattice's rank word, then the value */
#define SDPGPU_MULTI_FORM_FACT_DENSE 0x0080u     /* backward_fact_kernel, LK = 2: V_{t+1} laid out on the lattice */
#define SDPGPU_MULTI_FORM_FACT_I32 0x0100u       /* a backward_fact_kernel (LK 1, 2 or 3) formed lattice indices in 32-bit words */
#define SDPGPU_MULTI_FORM_FACT_I64 0x0200u       /* ... in 64-bit words */
#define SDPGPU_MULTI_FORM_LEAD_WAVE 0x0400u      /* backward_lead_wave_kernel: lead-time family, a wave per state */
#define SDPGPU_MULTI_FORM_BACKWARD 0x0800u       /* backward_kernel: a workgroup per state, the lambdas per cell */
#define SDPGPU_MULTI_FORM_DENSE_SCATTER 0x1000u  /* dense_scatter_kernel: V_{t+1} scattered to its lattice points */
uint32_t sdpgpu_multi_forms_used(void);

/* sdp.cash.multiItem.CashRecursionMulti.getExpectedValue (CashRecursionMulti.java:82-116) over the lambdas of
 * cash.multiItem.MultiItemCash (MultiItemCash.java:66-118): two products, cash-limited orders
 * (variCost[0] * i + variCost[1] * j < cash + 0.1), no lead time, state (I1, I2, cash) truncated to ints by the
 * transition, the `> val + 0.1` scan.  Runs on the same reachable-set engine as sdpgpu_multilead_solve.
 * The joint pmf of period t+1 is the list GetPmfMulti.getPmf(t) returns (rows {d1, d2, probability}):
 * entries pmf_off[t] .. pmf_off[t+1]-1 of d1 / d2 / p. */
typedef struct sdpgpu_multicash {
  int32_t T;       /* horizon (TLength) */
  int32_t q_bound; /* actions (i, j), i, j in [0, Qbound) */
  double price[2], vari_cost[2], sal_price[2];
  double ini_cash, ini_i1, ini_i2;
  double min_inventory, max_inventory, min_cash, max_cash; /* min_cash >= 0 */
  double discount;
  const int32_t* pmf_off; /* T + 1 offsets */
  const double* d1;
  const double* d2;
  const double* p;
} sdpgpu_multicash;

/* final_value = iniCash + V_1(iniState) (MultiItemCash.java:132); cells counts the offered actions only (the
 * reference evaluates nothing else); errors through sdpgpu_multilead_last_error(). */
int sdpgpu_multicash_solve(const sdpgpu_multicash* k, double* final_value, int32_t* q1, int32_t* q2,
                           int64_t* states_per_period, int64_t* cells, double* gpu_ms);

/* sdp.cash.multiItem.CashRecursionMultiXR.getExpectedValue (CashRecursionMultiXR.java:60-96) over the lambdas of
 * cash.multiItem.MultiItemCashXR (MultiItemCashXR.java:92-148): state (x1, x2, R) with R = cash + variCost . x, actions
 * = order-up-to levels (y1, y2) in [(int) x, (int) x + Qbound), no cash limit on them, demands kept as doubles.  Same
 * descriptor as sdpgpu_multicash_solve (ini_cash is the R of the period-1 state, MultiItemCashXR.java:158) plus
 * depositeRate; final_value = iniCash + V_1(iniState) (:160), (y1, y2) = getAction(iniState). */
int sdpgpu_multixr_solve(const sdpgpu_multicash* k, double deposit_rate, double* final_value, int32_t* y1, int32_t* y2,
                         int64_t* states_per_period, int64_t* cells, double* gpu_ms);

/* ---- sdp.cash.multiItem.CashRecursionV: the two functional equations V(x1, x2, w) and Pi(y1, y2, R) ---------------------
 * Replaces `new CashRecursionV(...).getExpectedValueV(iniState)` / getAction / getYStar / getAlpha
 * (src/sdp/cash/multiItem/CashRecursionV.java:83-194) for the lambdas of cash.multiItem.MultiItemYR.main
 * (MultiItemYR.java:104-158) and MultiItemYRTesting.main (its two order bounds, MultiItemYRTesting.java:100-101, and its
 * rounding, :163-165):
 *   Pi_t(y1, y2, R) = sum over the pmf list, in list order, of p_j * V_{t+1}(successor_j)           (CashRecursionV.java:83-97)
 *     successor (MultiItemYR.java:138-158): e_i = max(0, y_i - d_i); w' = (p1 min(y1, d1) + p2 min(y2, d2)) +
 *     (1 + depositeRate) * ((R - c1 y1) - c2 y2); e1, e2, w' rounded (below); w' clamped to [min_cash, max_cash], e1 clamped
 *     ABOVE only to max_inventory, e2 clamped BELOW only to min_inventory; (t + 1, e1, e2, w').  discountFactor is never used.
 *   V_t(x1, x2, w), t <= T (:100-131): R = (w + c1 x1) + c2 x2; the levels i in [(int) x1, (int) x1 + Q1), j in [(int) x2,
 *     (int) x2 + Q2) with c1 i + c2 j < R + 0.1, row-major, accepted when Pi > val + 0.01 from val = -Double.MAX_VALUE and
 *     best = (x1, x2); then getYStar(t, R).  V_{T+1} = w + sal1 x1 + sal2 x2 (MultiItemYR.java:132-135).
 *   y*(t, R) (:149-173): the UNSHIFTED box [0, Q1) x [0, Q2), every entry, `> val + 0.1`, default (0, 0); alpha(t, R)
 *     (:176-194) is computed iff c1 y1* + c2 y2* >= R + 0.1: the 100 values of `for (alpha = 0; alpha <= 1; alpha += 0.01)`
 *     (fp64 accumulation: the 101st is 1.0000000000000007), y1 = (alpha R) / c1, y2 = ((1 - alpha) R) / c2, `> best + 0.1`,
 *     default 0.
 * Rounding: SDPGPU_MULTIV_TRUNC10 is `Math.round(v * 10) / 10` (long / int: truncates toward zero, MultiItemYR.java:149-151),
 * SDPGPU_MULTIV_ROUND is `Math.round(v)` (MultiItemYRTesting.java:163-165); both leave integers, so the V states of periods
 * 2 .. T live on an integer lattice.  V is a pure function of the state, and the engine solves a SUPERSET of the reference's
 * memo: it evaluates the alpha line of every (t, R), the reference only where y* is not affordable.  Every state, (t, R) row
 * and value of the reference is in the tables, bit for bit; the counts below are the engine's own. */
#define SDPGPU_MULTIV_TRUNC10 0
#define SDPGPU_MULTIV_ROUND 1
typedef struct sdpgpu_multiv {
  int32_t T;          /* horizon, 1 .. 16 */
  int32_t q_bound[2]; /* Q1, Q2 (MultiItemYR.java:89 has one Qbound for both), 1 .. 1024 each */
  int32_t rounding;   /* SDPGPU_MULTIV_TRUNC10 / _ROUND */
  double price[2], vari_cost[2], sal_price[2];
  double deposit_rate;
  double ini_cash, ini_i1, ini_i2; /* the period-1 state (x1, x2, w); integer inventories */
  double min_inventory, max_inventory, min_cash, max_cash; /* integers; 0 <= min_cash */
  const int32_t* pmf_off; /* T + 1 offsets into d1 / d2 / p, as sdpgpu_multicash */
  const double* d1;
  const double* d2;
  const double* p;
} sdpgpu_multiv;

typedef struct sdpgpu_multiv_result {
  double value;        /* V_1(iniState), MultiItemYR.java:172 */
  double y1, y2;       /* getAction(iniState), :174 */
  double ystar1, ystar2; /* getYStar(1, iniCash), :179-180 */
  int32_t constrained; /* 1: the reference computed alpha(1, iniCash) */
  int32_t forms;       /* SDPGPU_MULTIV_FORM_* bits of the Pi kernel forms that ran */
  double alpha;        /* alpha(1, iniCash); defined only when constrained */
  int64_t cells;       /* (Pi entry, demand pair) evaluations of the backward pass */
  double gpu_ms;       /* device time of the forward and the backward pass */
} sdpgpu_multiv_result;
#define SDPGPU_MULTIV_FORM_SIDE 0x1u    /* integer levels: e_i and revenue_i read from the per-product side tables */
#define SDPGPU_MULTIV_FORM_GENERIC 0x2u /* the alpha line's fractional levels: the transition evaluated per cell */

/* The (t, R) rows of CashRecursionV's cacheYStar / cacheAlpha: register before a solve (per thread; NULL clears), filled by
 * the next sdpgpu_multiv_solve of the thread with one row per distinct R of every period, in (period, R) order.  `alpha` is
 * defined only where `constrained` is 1, which is exactly where the reference computed it.  `rows` receives the number of
 * rows; nothing is written when it exceeds `capacity`. */
typedef struct sdpgpu_multiv_rtable {
  int64_t capacity;
  int64_t rows;
  int32_t* period;
  double* R;
  int32_t* y1;
  int32_t* y2;
  int32_t* constrained;
  double* alpha;
} sdpgpu_multiv_rtable;
void sdpgpu_multiv_set_rtable(sdpgpu_multiv_rtable* table);

/* states / distinct R / Pi entries of periods 1 .. T (T entries each, may be NULL).  The V states come out through
 * sdpgpu_multi_set_table (periods 1 .. T; `cash` = w, q1 = q2 = 0, a1 / a2 = the chosen levels).  V_{t+1} is laid out DENSE on
 * the lattice (x1, x2, w) of the bounds; a lattice of more than 2^27 points is refused (SDPGPU_ERR_UNSUPPORTED, naming the
 * bounds), as are, all before any device call and naming the field (SDPGPU_ERR_ARG): min_cash < 0 or ini_cash < 0 (an empty
 * action list would return -Double.MAX_VALUE), non-integer initial inventories or bounds, vari_cost <= 0, q_bound < 1, T out of
 * range, a negative or non-finite demand.  A period whose Pi table (distinct R x levels) exceeds 2^28 entries ends the solve
 * with SDPGPU_ERR_UNSUPPORTED.  Errors through sdpgpu_multilead_last_error(). */
int sdpgpu_multiv_solve(const sdpgpu_multiv* k, sdpgpu_multiv_result* out, int64_t* states_per_period,
                        int64_t* r_per_period, int64_t* entries_per_period);
/* Kernel time of period t of the last solve (ms), needs sdpgpu_set_profiling(h, 1). */
double sdpgpu_period_ms(sdpgpu_handle* h, int32_t period);
/* ABI 6: (state, action, demand) cells of period t on this rank's slab, as sdpgpu_stats.cells_evaluated sums them over the periods
 * run (bench.py prices a kernel's counters against the cells of ITS launches: period T of a family may offer fewer orders).  -1:
 * not counted yet (the period has not run) or not known per period. */
int64_t sdpgpu_period_cells(sdpgpu_handle* h, int32_t period);

/* Additive to ABI 6: the screen of the F1 level kernel (a level block whose predecessor stopped at the cut-off is first walked
 * without the pmf's leading steps).  For period t of the last solve: out[0] = the step its screened blocks started
 * at (0: the screen was off for the period -- another kernel, the cut-off's gate closed, a leading step that carries more than
 * 2^-16 of the probability, a forced plan without SDPGPU_F1_SCREEN=1, or SDPGPU_F1_SCREEN=0), then its level blocks summed over
 * waves: out[1] screened and stopped, out[2] screens that failed (each walked again from step 0), out[3] walked from step 0
 * (out[1] + out[3] = the blocks of the launch); out[4] the demand steps its waves walked and out[5] those the launch planned
 * (the period's share of sdpgpu_stats.f1_level_steps_run / _planned).  All 0 for a period the level kernel's cut-off did not
 * run.  Waits for the handle's stream and copies a few bytes back, as sdpgpu_stats_get does. */
int sdpgpu_f1_screen_get(sdpgpu_handle* h, int32_t period, int64_t out[6]);
/* Host arithmetic, no device: the step the screen's rule gives for the pmf of period t -- the largest multiple of 8 (the
 * level kernel's levels per block) whose leading steps, on the unit-stride layout of the demands, carry at most 2^-16 of the
 * probability (SDPGPU_F1_SCREEN_LOG2=<e> at create time, a diagnostic: 2^-e); 0 below 8.  Whether a launch uses it is decided at the launch.  -1: bad arguments or no layout. */
int32_t sdpgpu_f1_screen_start(sdpgpu_handle* h, int32_t period);
/* Additive to ABI 6: the screen rows of the F1 level kernel.  A screened pass proves cells beaten, nothing else;
 * under the cut-off's gate the sums of one lane and one level are non-decreasing in the action, so it walks RS of the block's R = 4
 * action rows and holds each row's sum against the thresholds of all the rows it stands for.  SDPGPU_F1_SCREEN_ROWS=<1|2|4> at
 * create time chooses RS (unset: 2; 4: every row, the kernel without the collapse; anything else: SDPGPU_ERR_ARG from
 * sdpgpu_create, with a reason).  No table depends on it.  For period t of the last solve: out[0] = the demand steps its waves
 * walked in screened passes, stopped or failed (part of sdpgpu_f1_screen_get's out[4]; 0 where the screen was off or the level
 * kernel's cut-off did not run), out[1] = RS of the handle.  sdpgpu_stats.fp64_ops_executed prices those steps at the RS rows
 * that ran.  Waits for the handle's stream, as sdpgpu_f1_screen_get does. */
int sdpgpu_f1_screen_rows_get(sdpgpu_handle* h, int32_t period, int64_t out[2]);
/* Additive to ABI 6: the launch forms of the F1 level kernel.  The waves of a level launch are independent tasks;
 * a form decides which wave runs which task, and when, and nothing else -- no table, counter or plan depends on it.
 * SDPGPU_F1_LEVEL_FORM=<0|1|2> at create time: 0 = four tasks per 256-thread workgroup in index order, 1 = one wave per
 * workgroup, 2 = resident waves that claim tasks from a counter; 1 and 2 start band 0 and then the last bands first, the
 * longest tasks (unset: 2; anything else: SDPGPU_ERR_ARG from sdpgpu_create, with a reason; so for the diagnostics
 * SDPGPU_F1_LEVEL_WGS=<n >= 1>, the most workgroups form 2 launches, and SDPGPU_F1_LEVEL_ROUNDS=<q>, the round count the
 * planner's band search starts at).  A period-T launch without the cut-off or with all four rows screened runs as form 1
 * where form 2 is asked for (the claim loop would cost it a wave per SIMD).  For period t of the last solve: out[0] = the form
 * that ran, out[1] = the workgroups of its level launch, out[2] = the threads of each; where the level kernel did not run the
 * period: the handle's form, 0, 0.  Host-side: what the launcher recorded, no device read. */
int sdpgpu_f1_level_form_get(sdpgpu_handle* h, int32_t period, int64_t out[3]);
/* Host arithmetic, no handle: the executed fp64 operations per nominal cell that sdpgpu_stats_get charges a level period which
 * counted its steps -- ops_cell for each of the (steps_run - steps_screened) exact steps; for a screened step the
 * screen_rows * levels * (3 with a future term, 2 without) + screen_rows operations of a lane plus the table's levels / 64
 * products, over its rows * levels nominal cells (screen_rows = rows: ops_cell); one compare per cell and test -- all in units of
 * steps_planned.  -1: bad arguments. */
double sdpgpu_f1_level_ops_model(double ops_cell, int32_t future, int32_t rows, int32_t levels, int32_t screen_rows,
                                 int64_t steps_planned, int64_t steps_run, int64_t steps_screened, int64_t tests);

/* Additive to ABI 6: the decided split of the F1 level kernel.  Under the cut-off's gate -- MIN, the built-in
 * costs, K, v, h, pi >= 0, every probability >= 0, values of the library's own -- holding for period t and every later
 * period, action 0 provably wins in every state from an index c_t on, and V_t is non-decreasing there.
 * sdpgpu_f1_decided_start is host arithmetic, no device: c_t for this rank's slab of period t, from the descriptor, the grids
 * and the demand supports alone (c_t = max(0, m0_t + D_t - 1, c_{t+1} - idx_off_t + D_t - 1): m0_t the first level index that is
 * >= 0, D_t the steps of the period's unit-stride demand layout, idx_off_t the index shift into the next period's grid); the
 * slab's end says "none" (the gate is closed for this or a later period, or no state qualifies); -1: bad arguments or no layout.
 * Where the level kernel runs with the cut-off and lo < c_t < hi, the launcher walks only the live states [lo, c_t) and settles
 * [c_t, hi) with one one-action launch -- only with SDPGPU_F1_DECIDED=1 (opt-in, read at create time: the default sweep stays
 * the whole-slab one).
 * sdpgpu_f1_decided_get, host side as well: out[0] = c_t as above; for period t of the last solve out[1] = the live states its
 * level launch covered, out[2] = the decided states, out[3] = 1 where the split ran (else out[1] is the slab and out[2] is 0);
 * out[4] = bytes of the chunk-row arenas (0 before the first chunked launch). */
int64_t sdpgpu_f1_decided_start(sdpgpu_handle* h, int32_t period);
int sdpgpu_f1_decided_get(sdpgpu_handle* h, int32_t period, int64_t out[5]);

/* ---- batched solve: many backorder-family instances, of ONE grid shape or each with its own ----------------------------
 * The reference's parameter sweeps -- capacitated.CLSPTesting.main (CLSPTesting.java:33-141: 10 demand patterns x 2 v x
 * 3 pi x 3 K x 3 coeVar = 540 instances of the grid x in [-500, 500], Q = 0..500, T = 8), LevelFitsS, CLSPforDraw -- build
 * a new Recursion per parameter set and call getExpectedValue(initialState) / getAction(initialState) on each
 * (CLSPTesting.java:108-118).  A batch holds n such instances and runs period t of ALL of them in ONE kernel launch; every
 * instance's tables are bit for bit those of its own sdpgpu_handle.  Additive to ABI 6; an object of its own, separate from
 * sdpgpu_handle.
 *
 * Must agree between the n descriptors: family (SDPGPU_FAMILY_BACKORDER), direction, periods, step, min_inventory,
 * max_inventory, max_order_quantity, clamp_inventory (1), device, store_all_values, world_size (1).  May differ per instance:
 * fixed_order_cost, unit_order_cost, holding_cost, penalty_cost, ini_inventory (a grid point) -- and every pmf.  kernel:
 * SDPGPU_KERNEL_AUTO or _WINDOW.  A mismatch returns SDPGPU_ERR_ARG and names the instance and the field; what is out of
 * scope (another family, clamp_inventory = 0, world_size > 1, another kernel) returns SDPGPU_ERR_UNSUPPORTED with the reason.
 * n = 1 is legal.  Rules as for a handle: status codes; the text of the last failure through sdpgpu_batch_last_error
 * (NULL = the last failed sdpgpu_batch_create of this thread); validation and host layout first, device tables on first
 * use; pmfs frozen once the device tables exist; no C++ exception crosses the boundary; the caller's current device is
 * restored; one batch is not thread-safe.  store_all_values = 1 keeps n x T value tables, 0 two ping-pong tables per instance
 * (V_1 and V_2 survive); the policy tables of all periods are kept either way.
 *
 * RAGGED batches (sdpgpu_batch_create_ragged): the reference's other F1 sweeps -- capacitated.fitss.OneLevelFitsSTest,
 * TwoLevelFitsSTest, ThreeLevelFitsSTest (810 instances each), SimOpt -- take the order limit from the instance
 * (ThreeLevelFitsSTest.java:76-77: 27 distinct limits in one sweep), so the number of actions differs from row to row.  There
 * min_inventory, max_inventory and max_order_quantity may differ per instance as well, and ini_inventory is a point of the
 * instance's OWN grid; family, direction, periods, step, clamp_inventory (1), device, store_all_values, world_size (1) and
 * the kernel still agree, and a mismatch names the instance and the field in the same way.  The object is the same
 * sdpgpu_batch: every other sdpgpu_batch_* entry point works on it, sizes are per instance (sdpgpu_batch_num_states /
 * _num_actions), and the size refusals count the SUM of the instances' states.  sdpgpu_batch_create itself still refuses
 * differing bounds and order limits. */
typedef struct sdpgpu_batch sdpgpu_batch;
typedef struct sdpgpu_batch_stats {
  int32_t instances;
  int32_t periods_run;       /* period launches since the last sdpgpu_batch_solve began */
  int32_t period_launches;   /* launches of the period kernel by the last solve: T -- one per period for all instances */
  int32_t finalize_launches; /* other launches of the last solve: 0 when no period chunks the action axis (large n), else the
                                reset of the key rows and the one finalize pass */
  int32_t window_r;          /* register block of period 1's plan: actions ... */
  int32_t window_s;          /* ... x adjacent states per lane */
  int32_t window_chunks;     /* largest number of action chunks per state tile of any instance, over the periods (1: no
                                key atomics) */
  int32_t reserved;
  int64_t lds_bytes;         /* largest dynamic LDS per workgroup over the periods */
  int64_t cells_evaluated;   /* sum over instances and periods of states x actions x D: what n handles would report */
  double  solve_ms;          /* HIP-event time of the last sdpgpu_batch_solve on its stream */
} sdpgpu_batch_stats;
int sdpgpu_batch_create(const sdpgpu_desc* descs, int32_t n, sdpgpu_batch** out);
int sdpgpu_batch_create_ragged(const sdpgpu_desc* descs, int32_t n, sdpgpu_batch** out);
/* States / actions (order quantities 0 .. max_order_quantity in steps) of one instance; -1 for a bad argument.  In a batch
 * of one shape every instance answers alike. */
int64_t sdpgpu_batch_num_states(const sdpgpu_batch* b, int32_t instance);
int32_t sdpgpu_batch_num_actions(const sdpgpu_batch* b, int32_t instance);
void sdpgpu_batch_destroy(sdpgpu_batch* b);
const char* sdpgpu_batch_last_error(const sdpgpu_batch* b);
/* pmf of period index t (0-based, as sdpgpu_set_pmf takes it) of one instance.  n (= D) and demand[0] may differ between
 * instances and between periods; demand[0] may be negative (GetPmf truncates a negative lower quantile toward zero,
 * GetPmf.java:87: NormalDist(54, 16.2) has the support -6 .. 114).  Validated as sdpgpu_set_pmf does (multiples of step,
 * strictly ascending); additionally the spacing must be exactly `step`, which the window needs. */
int sdpgpu_batch_set_pmf(sdpgpu_batch* b, int32_t instance, int32_t t, const double* demand, const double* prob, int32_t n);
int sdpgpu_batch_set_stream(sdpgpu_batch* b, void* hip_stream);
/* Record a HIP event between the period launches of the next solves (read back through sdpgpu_batch_period_ms). */
int sdpgpu_batch_set_profiling(sdpgpu_batch* b, int32_t on);
/* Whole backward sweep t = T..1 of all instances: T launches of the period kernel (+ the key reset and one finalize pass
 * when the plan of a small batch chunks the action axis).  Asynchronous on the batch's stream unless `sync` != 0. */
int sdpgpu_batch_solve(sdpgpu_batch* b, int32_t sync);
int sdpgpu_batch_synchronize(sdpgpu_batch* b);
/* V_period[0..n) / the arg-opt action INDEX table (action = index * step) of one instance (1-based period); n is checked
 * against the instance's own number of states. */
int sdpgpu_batch_values(sdpgpu_batch* b, int32_t instance, int32_t period, double* out, int64_t n);
int sdpgpu_batch_policy(sdpgpu_batch* b, int32_t instance, int32_t period, int32_t* out, int64_t n);
/* What the sweep mains record (CLSPTesting.java:115-118): V_1(ini_inventory_i) and its action INDEX for all n instances,
 * gathered on the device and copied once. */
int sdpgpu_batch_initial(sdpgpu_batch* b, double* out_value, int32_t* out_action_index);
int sdpgpu_batch_stats_get(sdpgpu_batch* b, sdpgpu_batch_stats* out);
/* Time of period t's launch in the last solve (ms; needs sdpgpu_batch_set_profiling), -1 when there is none. */
double sdpgpu_batch_period_ms(sdpgpu_batch* b, int32_t period);
/* The launch plan of one period (1-based) of the whole batch, as sdpgpu_plan_period is for a handle: host arithmetic only,
 * available once every pmf is set, before a device is touched (SDPGPU_ERR_STATE names the first pmf that is missing).  One
 * register block and ONE chunk_blocks hold for all instances of the period; instance i has ceil(its r-blocks / chunk_blocks)
 * chunks, and the period is chunked -- key rows, one finalize pass per sweep -- as soon as one instance has two.  A forced
 * block that does not exist (SDPGPU_WIN_R / _S) returns SDPGPU_ERR_ARG, a plan whose window exceeds the LDS of a compute
 * unit SDPGPU_ERR_UNSUPPORTED, with the planner's reason. */
typedef struct sdpgpu_batch_plan {
  int32_t r, s;              /* register block: actions x adjacent states per lane */
  int32_t chunk_blocks;      /* register blocks of the action axis per task (an instance with fewer runs its own count) */
  int32_t chunked;           /* 1: some instance has more than one chunk, all instances go through key rows */
  int32_t max_chunks;        /* largest ... */
  int32_t min_chunks;        /* ... and smallest chunk count of an instance */
  int64_t tasks;             /* waves of the launch: sum over instances of state tiles x chunks */
  int64_t lds_bytes;         /* dynamic LDS per workgroup (four tasks), sized for the widest instance */
} sdpgpu_batch_plan;
int sdpgpu_batch_plan_period(sdpgpu_batch* b, int32_t period, sdpgpu_batch_plan* out);

/* ---- batched workforce solve: many STAFF instances of ONE shape, in the separable mode ------------------------------------
 * workforce.WorkforceTesting.main (WorkforceTesting.java:36-41) solves 2 x 3 x 3 x 3 x 4 = 216 instances of one shape (T = 8,
 * hires 0..1000, no clamp, iniStaffNum 0) over two turnover tables; they differ in fixCost, salary, unitPenalty and
 * minStaffNum[t].  sdpgpu_batch_create accepts SDPGPU_FAMILY_STAFF descriptors: the family of instance 0 selects the kind of
 * batch, and a batch holds one family.  Period t of ALL instances runs in TWO launches -- the rows G_t(y), P_t(y) of every
 * instance, then the scan (the separable mode of a STAFF handle, SDPGPU_KERNEL_SEPARABLE) -- and every instance's tables are
 * bit for bit those of its own separable handle.  Additive to ABI 6.
 *
 * Must agree between the n descriptors: family, periods, step (1), min_inventory, max_inventory, max_order_quantity,
 * clamp_inventory (0 or 1), ini_inventory (the unclamped per-period staff ranges grow from it), device, store_all_values,
 * world_size (1): a mismatch returns SDPGPU_ERR_ARG and names the instance and the field.  kernel must be
 * SDPGPU_KERNEL_SEPARABLE on every instance: the batch runs the separable mode only, which is never chosen automatically --
 * SDPGPU_KERNEL_AUTO or any other value returns SDPGPU_ERR_UNSUPPORTED; the exact cell-by-cell tables come from one handle per
 * instance.  May differ per instance: fixed_order_cost, unit_order_cost, holding_cost (salary), penalty_cost, minStaffNum[t]
 * (sdpgpu_batch_set_overhead; default: the descriptor's overhead_cost) and which level table each period uses.
 * sdpgpu_batch_create_ragged refuses the family.  With clamp_inventory = 0 the staff range of a period depends on the longest
 * rows of the tables before it: instances whose tables would give different ranges are refused at layout
 * (SDPGPU_ERR_UNSUPPORTED).
 *
 * Level tables live in a POOL owned by the batch -- a handle stores pmfs[t] once per period and instance; the sweep's 216 x 8
 * tables of 8 MB are two.  sdpgpu_batch_add_level_pmf takes pmfs[t] of StaffRecursion.java:23,92-95 exactly as
 * sdpgpu_set_level_pmf does (prob[y * row_stride + j], row_len NULL = y + 1 entries in row y; whatever lies behind a row's
 * length is never read) and returns the table's id; a table of 2 GiB or more is SDPGPU_ERR_UNSUPPORTED.
 * sdpgpu_batch_use_level_pmf makes period index t (0-based) of `instance` integrate over table `table`; instance = -1: every
 * instance, t = -1: every period.  sdpgpu_batch_set_overhead sets minStaffNum[t] of one instance (an integer value).  Tables
 * are frozen once the device tables exist (SDPGPU_ERR_STATE); minStaffNum, on which no staff range, plan or arena depends, may
 * still be set then: the batch counts as unsolved until the next sdpgpu_batch_solve, which runs with the new value.
 *
 * On a STAFF batch these entry points keep their meaning: sdpgpu_batch_destroy, _last_error, _num_actions, _num_states (the
 * states of period T: the largest staff range, and every period's when clamped; -1 while an unclamped batch lacks a table it
 * depends on), _set_stream, _set_profiling, _solve (2 T launches; SDPGPU_ERR_STATE names the first (instance, period) without
 * a table, before any device call), _synchronize, _values and _policy (n is checked against the states of THAT period:
 * sdpgpu_batch_grid), _initial (V_1(iniStaffNum) and its hire index), _stats_get (period_launches = 2 T, cells_evaluated = the
 * sum of what the n separable handles report; finalize_launches, window_r, window_s, window_chunks and lds_bytes are 0),
 * _period_ms.  Every other sdpgpu_batch_* call but the three of "batched workforce fit and rollout" below returns
 * SDPGPU_ERR_UNSUPPORTED on a STAFF batch, naming the call and the family, before any device call
 * (sdpgpu_batch_simulate_ms: -1); the three table calls and sdpgpu_batch_staff_plan_period return the same on a batch of the
 * backorder family.
 *
 * sdpgpu_batch_grid: staff number of state index 0 and the number of states of one instance in one period (1-based) -- the
 * unclamped ranges differ by period.  Host arithmetic; on a backorder batch x_lo = min_inventory of the instance.
 *
 * sdpgpu_batch_staff_plan_period: the two launches of one period (1-based), host arithmetic only, available once every
 * (instance, period) has a table.  The instances are grouped per (period, table); a G task is one wave: 64 consecutive levels
 * of a block of r instances of one group, which share the probabilities, the row weights P, the staff left and the addresses
 * of a step, each with its own immediate cost, V_{t+1} and sum.  r comes from the group sizes alone: the instance block where
 * some group of the period holds at least that many instances, else 1; a group's last block may be short. */
typedef struct sdpgpu_batch_staff_plan {
  int32_t tables;            /* distinct tables the period uses ... */
  int32_t groups;            /* ... = groups of instances */
  int32_t r;                 /* instances per G task */
  int32_t u;                 /* steps a lane reads ahead per register set */
  int32_t longest_row;       /* longest row of the period's tables: steps of the longest G task */
  int32_t reserved;
  int64_t blocks;            /* instance blocks: sum over the groups of ceil(size / r) */
  int64_t g_tasks;           /* waves of the G launch: blocks x ceil(levels / 64) */
  int64_t scan_workgroups;   /* workgroups of the scan launch: instances x ceil(states / 64) */
  int64_t levels;            /* hire-up-to levels per instance: states + actions - 1 */
  int64_t states;            /* states per instance */
} sdpgpu_batch_staff_plan;
int sdpgpu_batch_add_level_pmf(sdpgpu_batch* b, const double* prob, const int32_t* row_len, int32_t n_rows, int32_t row_stride,
                               int32_t* out_table);
int sdpgpu_batch_use_level_pmf(sdpgpu_batch* b, int32_t instance, int32_t t, int32_t table);
int sdpgpu_batch_set_overhead(sdpgpu_batch* b, int32_t instance, int32_t t, double min_staff);
int sdpgpu_batch_grid(sdpgpu_batch* b, int32_t instance, int32_t period, double* x_lo, int64_t* nx);
int sdpgpu_batch_staff_plan_period(sdpgpu_batch* b, int32_t period, sdpgpu_batch_staff_plan* out);

/* ---- batched simulation: roll the policies of ALL instances of a solved batch along demand paths, one launch ------------
 * What CLSPTesting.main does after every solve -- `new Simulation(distributions, 10000, recursion)
 * .simulateSDPGivenSamplNum(initialState)` (CLSPTesting.java:120-124; Simulation.java:53-74) -- for the whole batch.  Per path
 * and instance, periods 1..T in order: action index of the current grid state from the instance's policy row,
 * `sum += immediateValue(state, action, demand)`, `state = stateTransition(...)` (Simulation.java:59-69 on the lambdas of
 * CLSPTesting.java:89-106).  A path's sum is bit for bit what sdpgpu_simulate gives on a handle of the instance with
 * discount 1.0.  Demands need not lie in the pmf support and may be negative: the grid is clamped.  Works with
 * store_all_values 0 and 1 (the policy rows of all periods are kept either way).  Additive to ABI 6.
 *
 * n_paths: 1 .. 2^24.  ini_x: NULL = every descriptor's ini_inventory, else n grid points (ini_x[i] on instance i's grid).  out_mean[n]: mean of the
 * instance's path sums, formed on the device in a fixed order (the same bits on every call).  out_sum: NULL, or
 * n x n_paths path sums (instance-major).  Errors as for the rest of the batch: SDPGPU_ERR_ARG names the instance and the
 * field, SDPGPU_ERR_STATE when nothing has been solved; validation comes before any device call. */
/* Explicit demands: demand[i * instance_stride + p * T + t] is the demand of path p of instance i in period t + 1, already
 * rounded by the caller as Simulation.java:64 does; instance_stride = 0 shares ONE set of n_paths x T between all
 * instances, otherwise it is >= n_paths * T. */
int sdpgpu_batch_simulate(sdpgpu_batch* b, int32_t n_paths, const double* demand, int64_t instance_stride, const double* ini_x,
                          double* out_mean, double* out_sum);
/* Sampled demands: the latin hypercube of Sampling.generateLHSamples (Sampling.java:86-103) drawn ON the device, seeded and
 * reproducible (Math.random() makes the reference's unrepeatable): path p of (instance i, period t) takes the stratum
 * j = sigma(p) of [0, n_paths) -- sigma a keyed bijection, the per-column shuffle of Sampling.java:326-335 --, a = 53 bits of
 * Philox4x32-10 at counter (j, t, i, 0) under `seed`, u = j / n + a / n (:94), and the demand Math.round(inverseF(u)) (:95,
 * Simulation.java:64) by ONE binary search in a threshold table the host made.  i is the instance's POSITION in the batch.
 * The exact construction is DESIGN.md 4 ("Batched simulation").  Needs step == 1 (Math.round yields integers), else
 * SDPGPU_ERR_UNSUPPORTED.
 * sdpgpu_batch_set_sampler chooses the distribution of (instance, period index t): a spec (any kind of sdpgpu_dist_spec;
 * thresholds = sdpgpu_sample_table) or NULL = the instance's own pmf tile of that period (thresholds = the running fp64
 * sum of its probabilities, the last one +infinity), which is also the default.  Paths drawn from the tile make the mean
 * an unbiased estimate of V_1(ini); with specs it carries the truncation bias of GetPmf's quantile, as the reference's. */
int sdpgpu_batch_set_sampler(sdpgpu_batch* b, int32_t instance, int32_t t, const sdpgpu_dist_spec* spec);
int sdpgpu_batch_simulate_sampled(sdpgpu_batch* b, int32_t n_paths, uint64_t seed, const double* ini_x, double* out_mean,
                                  double* out_sum);
/* The demands (and, when out_u is not NULL, the uniforms) sdpgpu_batch_simulate_sampled uses for ONE instance, produced by
 * the same device code: out[p * T + t].  Needs the pmfs and a device, not a solve. */
int sdpgpu_batch_sample_demands(sdpgpu_batch* b, int32_t instance, int32_t n_paths, uint64_t seed, double* out_demand,
                                double* out_u);
/* HIP-event time (ms) of the kernels of the last sdpgpu_batch_simulate* call on the batch's stream (rollout + means; the
 * copies are outside), -1 when there is none. */
double sdpgpu_batch_simulate_ms(sdpgpu_batch* b);
/* The threshold table of one distribution, host arithmetic only (no device), like sdpgpu_getpmf: ascending c_0 .. c_{n-1},
 * c_q = F(k_lo + q + 0.5) for a continuous distribution (demand = k_lo + #{c <= u}: Math.round(inverseF(u)) = k exactly when
 * F(k - 0.5) <= u < F(k + 0.5)) and F(k_lo + q) for an integer-valued one (demand = k_lo + #{c < u}: inverseF(u) =
 * min{k : F(k) >= u}), over every k whose threshold lies in (2^-64, 1) in fp64; a u below c_0 takes k_lo.  capacity = 0
 * is a sizing call.  More than SDPGPU_SAMPLE_TABLE_CAP thresholds: SDPGPU_ERR_UNSUPPORTED.  Errors through
 * sdpgpu_last_error(NULL). */
#define SDPGPU_SAMPLE_TABLE_CAP 65536
int sdpgpu_sample_table(const sdpgpu_dist_spec* spec, int32_t* k_lo_out, double* thresholds, int32_t capacity, int32_t* n_out);

/* ---- (s, S) level rules of a batch: fit from the policy tables, roll out -------------------------------------------------
 * What the capacitated.fitss drivers do after every solve (ThreeLevelFitsSTest.java:135-145; One- and TwoLevelFitsSTest
 * alike): `recursion.getOptTable()`, fit a one-, two- or three-level (s, S) rule to it (sdp.inventory.FitsS.getSinglesS /
 * getTwosS / getThreesS, FitsS.java:100-291), simulate the rule (capacitated.fitss.SimulateFitsS.simulateSinglesS / TwosS /
 * ThreesS, SimulateFitsS.java:32-130) and record (simFinalValue - finalValue) / finalValue.  Additive to ABI 6.  The exact
 * definition of the fit is DESIGN.md 4 ("Batched (s, S) level rules").
 *
 * The reference's opt table holds the states its memoised recursion visits.  For a batch instance (clamped grid, demand
 * supports spaced `step`) they are ONE interval of grid indices per period: lo_1 = hi_1 = index(ini_inventory),
 * lo_{t+1} = clamp(lo_t - d_max,t / step), hi_{t+1} = clamp(hi_t + (A - 1) - d_0,t / step), clamped to the instance's grid.
 * sdpgpu_batch_reachable gives it for a 1-based period: host arithmetic, needs the instance's pmfs of the periods before
 * (SDPGPU_ERR_STATE names the first one missing), not a device. */
int sdpgpu_batch_reachable(sdpgpu_batch* b, int32_t instance, int32_t period, int32_t* lo, int32_t* hi);
/* FitsS on rows [period, x, Q] (opt_table: n_rows x 3, the rows of a period ascending in x as Recursion.getOptTable gives
 * them; FitsS(maxOrderQuantity, T)): out[t * 2 * levels ...] = s_1, S_1 (, s_2, S_2 (, s_3, S_3)) of period t + 1 for levels
 * = 1 (getSinglesS), 2 (getTwosS), 3 (getThreesS), branch for branch -- period 1 is s = x_0 + 1, S = x_0 + Q_0 of the first
 * row; levelIndex (FitsS.java:39-59); the "last row still at the limit" corrections; the copies of the upper bands.
 * minSquare (:69-98) is the closed form of the problem the reference gives to CPLEX: the fp64 mean of the terms x_i + Q_i
 * (i = the first row not at the limit, and every later row up to upIndex not at the limit), clamped to [lb, 10000].  Host
 * arithmetic only, no device; a period without rows is SDPGPU_ERR_ARG (the reference indexes an empty array there).
 * sdpgpu_fit_level_index and sdpgpu_fit_min_square are levelIndex and minSquare on the rows of ONE period (columns x, q of
 * n rows; out_index holds up to n entries).  Errors through sdpgpu_last_error(NULL). */
int sdpgpu_fit_ss(int32_t levels, int32_t T, double max_order_quantity, const double* opt_table, int64_t n_rows, double* out);
int sdpgpu_fit_level_index(double max_order_quantity, const double* q, int32_t n, int32_t* out_index, int32_t* n_out);
int sdpgpu_fit_min_square(double max_order_quantity, double lb, int32_t up_index, const double* x, const double* q, int32_t n,
                          double* out);
/* The fit of EVERY instance of a solved batch on the device: one kernel reads each (instance, period)'s reachable slice of
 * the policy arena and writes its level row, one copy brings out[n x T x 2 * levels] back -- no policy table crosses to the
 * host.  Bit for bit sdpgpu_fit_ss on the instance's read-back rows (the same statements compiled for the device; with
 * step 1 every min-square term is an integer and the sum exact).  Needs step == 1 (SDPGPU_ERR_UNSUPPORTED otherwise);
 * SDPGPU_ERR_STATE before a solve, SDPGPU_ERR_ARG for levels outside 1..3. */
int sdpgpu_batch_fit_ss(sdpgpu_batch* b, int32_t levels, double* out);
/* Roll a level rule of every instance along demand paths (SimulateFitsS.java:32-130): per path, x = ini; period index 0
 * orders ss[0][1] - ini, uncapped as the reference has it (:43); every later period tests the bands as written -- one level:
 * x >= s_1 ? 0 : min(maxQ, S_1 - x); two and three levels: x < s_1, s_1 <= x < s_2 (, s_2 <= x < s_3) order
 * min(maxQ, S_k - x), 0.0 outside every band --, then `sum += immediateValue(x, Q, d)`, `x = stateTransition(x, Q, d)` with
 * the statements of sdpgpu_batch_simulate.  The state is a double, not a grid index: a fitted S may be fractional.
 * ss: n x T x 2 * levels (what sdpgpu_batch_fit_ss writes; any rule the caller made) -- then the call needs the pmfs and a
 * device, not a solve -- or NULL = fit first, in the same call, the levels staying on the device (needs a solved batch and
 * step == 1).  n_paths, demand, instance_stride, seed, ini_x, out_mean, out_sum, the samplers and the order of the mean's
 * sum: exactly as sdpgpu_batch_simulate / _sampled.  The same (seed, position in the batch, n_paths) therefore rolls the
 * rule along the SAME demand paths as sdpgpu_batch_simulate_sampled rolls the table policy: common random numbers for the
 * gap between the two, which the reference's unseeded Math.random() cannot offer.  sdpgpu_batch_simulate_ms then covers
 * the fit (when ss is NULL), the rollout and the means. */
int sdpgpu_batch_simulate_ss(sdpgpu_batch* b, int32_t levels, const double* ss, int32_t n_paths, const double* demand,
                             int64_t instance_stride, const double* ini_x, double* out_mean, double* out_sum);
int sdpgpu_batch_simulate_ss_sampled(sdpgpu_batch* b, int32_t levels, const double* ss, int32_t n_paths, uint64_t seed,
                                     const double* ini_x, double* out_mean, double* out_sum);

/* ---- structure checks: G(y) rows, K- and CK-convexity ------------------------------------------------------------------
 * The reference's own validation idiom: after a solve the drivers run sdp.inventory.CheckKConvexity on a row of values --
 * ThreeLevelFitsSTest.main (:146-159) checkCK on V_1(x), x = 0 .. 100, the verdict being the last column of its CSV row;
 * CLSPforDraw.main (:144-182) check on G(y), built by a second Recursion whose period 1 is special; WorkforcePlanning.main
 * (:208-209) likewise.  Additive to ABI 6.
 *
 * A row is g[0 .. n): fp64 values at consecutive grid points (the reference's xLength, taken from the first and last abscissa,
 * is n for the unit-spaced rows every caller builds).  Both checks evaluate, in fp64, left to right, without FMA,
 *     t = g_mid - g_near;  t = (double)mult * t;  t = t / (double)div;  rhs0 = g_mid + t;  lhs = g_far + K
 * and a triple PASSES iff lhs > rhs0 - 0.1; anything else -- equality, a NaN on either side -- is a violation, and the check
 * ends at the FIRST one in loop order.
 *   kind 0, check   (CheckKConvexity.java:39-68): a = 0 .. n-1, b = 0 .. a-1, c = 0 .. b-1; far, mid, near = g[a], g[b], g[c];
 *                   mult = a - b, div = b - c; (i0, i1, i2) = (a, b, c).
 *   kind 1, checkCK (:6-36): y = 0 .. n-1, z = 0 .. capacity-1, b = 1 .. capacity-1, skipping y - b <= 0 and y + z >= n;
 *                   far, mid, near = g[y+z], g[y], g[y-b]; mult = z, div = b; (i0, i1, i2) = (y, z, b).
 * holds = 1: no triple violates (rows without any triple hold), the indices are -1 and both doubles 0.0.  holds = 0:
 * (i0, i1, i2) is the first violating triple, lhs and rhs the two numbers the reference prints there (rhs without the - 0.1). */
typedef struct sdpgpu_convexity {
  int32_t holds;
  int32_t i0, i1, i2;
  double lhs;
  double rhs;
} sdpgpu_convexity;
/* One row on the host (no device; the plain loops): what the device entry point is held to, bit for bit.  kind outside
 * {0, 1}, n < 0, a null pointer: SDPGPU_ERR_ARG through sdpgpu_batch_last_error(NULL). */
int sdpgpu_check_convexity(int32_t kind, const double* g, int64_t n, double K, int32_t capacity, sdpgpu_convexity* out);
/* G_period(y) of one instance of a solved batch, y over the instance's grid (CLSPforDraw.java:147-170, its period 1
 * generalised to any period): the cost of STANDING at level y -- sum over the demand index j, ascending, of
 * p_j * (((0.0 + v*y) + h*max(y - d_j, 0)) + pi*max(d_j - y, 0)), then for period < T  p_j * V_{period+1}(clamp(y - d_j)), the
 * clamp as the family's (upper bound first).  The rows of ALL instances and periods are computed on the device at the first
 * request after a solve and kept there; the call copies n <= num_states values of one row.  SDPGPU_ERR_STATE before a solve,
 * and for a period whose V_{period+1} was overwritten (store_all_values = 0 keeps G_1 and G_T). */
int sdpgpu_batch_gy(sdpgpu_batch* b, int32_t instance, int32_t period, double* out, int64_t n);
/* CheckKConvexity on one row of EVERY instance of a solved batch, in one kernel launch: kind as above; source 0 = the value
 * rows V_period (ThreeLevelFitsSTest.java:146-159), 1 = the rows G_period.  x_lo / x_hi (n each, or both NULL = every
 * instance's whole grid): the window of inventory levels x_lo[i] .. x_hi[i] of instance i, both grid points of ITS grid with
 * x_lo <= x_hi, else SDPGPU_ERR_ARG naming the instance (the driver's call is 0 and 100 for all).  K NULL: each instance's
 * fixed_order_cost.  capacity NULL: (int)max_order_quantity of the instance, which needs step == 1 (for kind 1: SDPGPU_ERR_ARG
 * otherwise, asking for explicit capacities; kind 0 reads no capacity).  A window of more than 8192 points is
 * SDPGPU_ERR_UNSUPPORTED.  out: n structs, written only when the call succeeds.  Bit for bit sdpgpu_check_convexity on the
 * read-back rows (one predicate function for host and device; a violating triple is reduced as a 64-bit integer key that sorts
 * like the loop order, so the first one wins whatever the order of the workgroups).  SDPGPU_ERR_STATE before a solve. */
int sdpgpu_batch_check_convexity(sdpgpu_batch* b, int32_t kind, int32_t source, int32_t period, const double* x_lo,
                                 const double* x_hi, const double* K, const int32_t* capacity, sdpgpu_convexity* out);

/* ---- cash structure tables: G(y, R), H, GB - GA - K, F - G and their checks -----------------------------------------------
 * What the cash drivers do after a solve (CashConstraintDraw.main :187-297, CheckFG.main :100-198, CheckMonotony.main
 * :132-257, SingleCrossTesting.main :85-178): a table over a window of (cash R, level y) start states from a recursion whose
 * drawn period ignores the action, post-processed by CashRecursion.java:227-404.  In the drawn period every action yields the
 * same sum, so an entry is the ACTION-0 sum of the handle's own cell statements against the handle's own V_{period+1}.
 * Additive to ABI 6.  DESIGN 4, "Cash structure tables".
 *
 * Scope of a handle: family CASH with cash_formula 1, step 1, an integer cash grid (cash_round_mult = cash_round_div = 1),
 * world_size 1, no user functor; anything else SDPGPU_ERR_UNSUPPORTED naming the field, before any device call.
 *
 * sdpgpu_cash_g_table: out[i * n_x + j] is the entry of cash R = cash_lo + i and level y = x_lo + j
 * (SingleCrossTesting.java:154-165, resultTable[rowIndex][columnIndex]) of `period` (any of 1 .. T).  The entry sums over
 * the demand index ascending from 0.0 (CashRecursion.java:110-122): acc += p * imm, then for period < T
 * acc += (p * gamma) * V_{period+1}(next), with imm and next the CASH cell statements for base = y, fixed = 0.0, the period's
 * overhead, salvage at period T only, the penalty statement, both clamps and the quantiser unchanged, and
 *   kind SDPGPU_CASH_G  (0; SingleCrossTesting.java:110-131,159; CheckFG.java:139-181): var = 0.0; stored acc - v * y
 *   kind SDPGPU_CASH_GA (1; CashConstraintDraw.java:193-214,264-274): var = v * y; stored acc
 *   kind SDPGPU_CASH_GB (2; :217-229): as GA with ncash = ncash - K between ncash = R + inc and the cash clamps
 * x_lo, cash_lo whole numbers, the window inside [min_inventory, max_inventory] x [min_cash, max_cash], n_x, n_r >= 1, else
 * SDPGPU_ERR_ARG naming the argument; more than SDPGPU_CASH_G_MAX_AXIS points on an axis is SDPGPU_ERR_UNSUPPORTED.
 * SDPGPU_ERR_STATE before a solve and for a period whose V_{period+1} a ping-pong handle (store_all_values = 0) has
 * overwritten. */
#define SDPGPU_CASH_G 0
#define SDPGPU_CASH_GA 1
#define SDPGPU_CASH_GB 2
#define SDPGPU_CASH_G_MAX_AXIS 65536 /* points per axis of a G window (the launch's grid dimensions) */
int sdpgpu_cash_g_table(sdpgpu_handle* h, int32_t kind, int32_t period, double x_lo, int32_t n_x, double cash_lo, int32_t n_r,
                        double* out);

/* The request mask of sdpgpu_cash_structure / _host.  A check bit forms the table it reads; check slot 0 = H,
 * 1 = GB - GA - K, 2 = F - G - v j. */
#define SDPGPU_CSTRUCT_H 0x1            /* getH (CashRecursion.java:270-295), and the optyIndex table the reference drops */
#define SDPGPU_CSTRUCT_GAGB 0x2         /* getMinusGAGB (:227-244) */
#define SDPGPU_CSTRUCT_FG 0x4           /* getMinusFG (:252-262) */
#define SDPGPU_CSTRUCT_SINGLE_CROSS 0x8 /* checkSingleCrossing (:298-318) on H */
#define SDPGPU_CSTRUCT_NONINC(slot) (0x10 << (slot)) /* checkNonIncreasing (:363-379) on table `slot` */
#define SDPGPU_CSTRUCT_NONDEC(slot) (0x80 << (slot)) /* checkNonDecreasing (:386-404) on table `slot` */
#define SDPGPU_CSTRUCT_ALL 0x3ff
/* Derived tables and checks work on windows of at most SDPGPU_CSTRUCT_MAX_AXIS points per axis (three indices of 11 bits in
 * a violation key) and SDPGPU_CSTRUCT_MAX_POINTS points in all (the tables of one call: at most 64 MiB of device memory);
 * beyond them SDPGPU_ERR_UNSUPPORTED. */
#define SDPGPU_CSTRUCT_MAX_AXIS 2048
#define SDPGPU_CSTRUCT_MAX_POINTS (1 << 20)

typedef struct sdpgpu_cash_structure_in {
  int32_t source;   /* 0: the tables of the solved handle, formed on the device (G, GA, GB by sdpgpu_cash_g_table's kernel, F =
                       V_period on the window: CheckFG.java:183-196); 1: the caller's tables g / ga / gb / f */
  int32_t mask;     /* SDPGPU_CSTRUCT_* bits, 1 .. SDPGPU_CSTRUCT_ALL */
  int32_t device;   /* source 1 on the device: where the tables are uploaded when the handle is NULL (-1: the current one) */
  int32_t period;   /* source 0: the drawn period (the drivers' `period = 1`, SingleCrossTesting.java:91) */
  int32_t n_r, n_x; /* RLength, xLength (CashRecursion.java:271-272): rows = cash, columns = levels */
  double x_lo;      /* source 0: minInventorys, the level of column 0 (SingleCrossTesting.java:85) */
  double min_cash;  /* minCash: `cash = minCash + i` (CashRecursion.java:232, :275); source 0: the cash of row 0 */
  double fix_cost;  /* fixCost (CashRecursion.java:227, :252, :270) */
  double vari_cost; /* variCost (the same lines) */
  const double* g;  /* source 1: resultG  (CashRecursion.java:270, :252), n_r * n_x, row-major; read by H and F - G */
  const double* ga; /* source 1: resultGA (:227) */
  const double* gb; /* source 1: resultGB (:227) */
  const double* f;  /* source 1: resultF  (:252) */
  /* source 1: a derived table the caller already holds -- resultH of checkSingleCrossing (:298), arr of checkNonIncreasing /
   * checkNonDecreasing (:363, :386).  A slot given here is not formed (its sources are not read, optyIndex is not written):
   * the checks of that slot read the caller's table as it stands. */
  const double* h;
  const double* gagb;
  const double* fg;
} sdpgpu_cash_structure_in;

/* One check's verdict.  holds = 1: the indices are -1 and value 0.0.  holds = 0: the FIRST violation in the reference's loop
 * order.  checkSingleCrossing (:302-310): row i whose last passing column is j, the failing entry resultH[i1][j1] = value.
 * checkNonIncreasing (:367-370): (i, j), (i1, j1) = (i, j + 1), value = arr[i][j + 1] - arr[i][j].  checkNonDecreasing
 * (:393-395): (i, j), (i1, j1) = (i + 1, j), value = arr[i + 1][j] - arr[i][j]. */
typedef struct sdpgpu_cash_verdict {
  int32_t holds;
  int32_t i, j, i1, j1;
  int32_t reserved;
  double value;
} sdpgpu_cash_verdict;

typedef struct sdpgpu_cash_structure_out {
  double* g;  /* optional host copies, n_r * n_x each, of every table the call formed or read (NULL: not copied) */
  double* ga;
  double* gb;
  double* f;
  double* h;          /* `values` of getH (CashRecursion.java:291) */
  int32_t* opt_y;     /* optyIndex of getH (:279, :287) */
  double* gagb;       /* `values` of getMinusGAGB (:240) */
  double* fg;         /* `values` of getMinusFG (:258) */
  sdpgpu_cash_verdict single_crossing;   /* checkSingleCrossing (:298-318) on H */
  sdpgpu_cash_verdict non_increasing[3]; /* checkNonIncreasing (:363-379) on slot 0 / 1 / 2 */
  sdpgpu_cash_verdict non_decreasing[3]; /* checkNonDecreasing (:386-404) */
  double kernel_ms;   /* device path: HIP-event time of the call's kernels (0.0 from the host entry point) */
} sdpgpu_cash_structure_out;

/* The requests, each the reference's loops as they stand, fp64, left to right, no FMA:
 *   H: row i is cash = min_cash + i; ybound = min(n_x - 1, j + max(0, (int)((cash - K) / v))); candidates k = j + 1 .. ybound
 *      with cashIndex = (int)(cash - K - v * (k - j)) used directly as a ROW index; cashIndex < 0 is skipped; the candidate is
 *      G[cashIndex][k] - G[i][j] - K, strict > from the initial -K, the first candidate wins ties.  cashIndex >= n_r, where
 *      Java would throw, is SDPGPU_ERR_ARG naming (i, j, k), found before any table is written.
 *   GB - GA - K: a running maximum (strict >) of GB[i][k], k in [j, min(j + Qbound + 1, n_x)), Qbound = max(0, (int)((cash -
 *      K) / v)), started at GB[i][j]; then - GA[i][j] - K.
 *   F - G - v j: F[i][j] - G[i][j] - v * j with j the COLUMN INDEX.
 *   checkSingleCrossing: an entry passes iff it is > -0.1 (a NaN fails); lastColumnEnd carries from row to row and a row
 *      without a passing entry leaves it unchanged.
 *   checkNonIncreasing: loops i then j, passes iff arr[i][j + 1] - arr[i][j] < 0.1.
 *   checkNonDecreasing: loops j then i, passes iff arr[i + 1][j] - arr[i][j] > -0.1.
 * (int) is Java's narrowing: NaN gives 0, out-of-range values saturate; int sums wrap.  A NaN that is STORED -- an entry of a
 * table formed here, a verdict's value -- is the one NaN of Double.doubleToLongBits, 0x7ff8000000000000 (which NaN an operation
 * yields differs between processors, and Java defines none); a caller's table is copied as it stands.
 *
 * sdpgpu_cash_structure runs them on the device; h may be NULL for source 1 (errors then through sdpgpu_last_error(NULL)).
 * sdpgpu_cash_structure_host runs them on the caller's tables (source 1 only) with the plain loops and no device: what the
 * device path is held to bit for bit -- the per-element predicates and arithmetic are functions shared by both.  A table the
 * mask needs and the caller left NULL, n_r or n_x < 1, a mask outside 1 .. SDPGPU_CSTRUCT_ALL: SDPGPU_ERR_ARG. */
int sdpgpu_cash_structure(sdpgpu_handle* h, const sdpgpu_cash_structure_in* in, sdpgpu_cash_structure_out* out);
int sdpgpu_cash_structure_host(const sdpgpu_cash_structure_in* in, sdpgpu_cash_structure_out* out);

/* ---- sampled simulation on a handle: demand paths drawn ON the device, rolled and reduced there ------------------------
 * What every driver does after its solve -- `new Simulation(distributions, sampleNum, recursion)
 * .simulateSDPGivenSamplNum(initialState)` (Simulation.java:53-74; CashSimulation.java:85-118 for the cash classes;
 * RiskSimulation.java:206-241 for the survival objective) and simulateSDPwithErrorConfidence (Simulation.java:76-107) -- with
 * the SAMPLING (Sampling.generateLHSamples, Sampling.java:86-103; generateRanSamples, :50-60; Math.round, Simulation.java:64)
 * done by the kernel that rolls the paths, for every family sdpgpu_simulate serves.  A handful of numbers cross to the host
 * instead of n_paths x T doubles.  The exact construction is DESIGN.md 4 ("Sampled simulation on a handle").  Additive to
 * ABI 6.
 *
 * SDPGPU_SAMPLE_LHS: the batch's latin hypercube with the instance position fixed at 0 -- path p of period index t takes the
 * stratum j = sigma(p), a = 53 bits of Philox4x32-10 at counter (j, t, 0, 0) under `seed`, u = j / n + a / n; an F1 handle
 * draws what a batch of ONE built from the same descriptor and pmfs draws.  first_path must be 0.
 * SDPGPU_SAMPLE_RANDOM: path P = first_path + p (64 bits), (w0, w1, ., .) = Philox at counter (P mod 2^32, t, P div 2^32, 2),
 * u = ((w0 * 2^32 + w1) >> 11) * 2^-53: calls with (first_path, n) = (0, a) then (a, b) draw what one call (0, a + b) draws.
 * Demand from u, per period index t: a spec set by sdpgpu_set_sampler (thresholds = sdpgpu_sample_table, demand =
 * k_lo + #{c <= u} resp. #{c < u}) or -- the default -- the handle's own pmf tile of that period: thresholds = the running
 * fp64 sum of its probabilities in ascending order, the last one +infinity, demand = the tile's q-th demand VALUE,
 * q = #{c <= u} (a tile may have gaps and any step).  Tile samplers draw from the very distribution the recursion used: every
 * path stays on the grid and the mean estimates V_1(ini) without bias. */
#define SDPGPU_SAMPLE_LHS 0
#define SDPGPU_SAMPLE_RANDOM 1
/* The distribution of period index t (0-based): a spec, or NULL = back to the pmf tile.  Validated like
 * sdpgpu_batch_set_sampler (period index, kind, parameters, SDPGPU_SAMPLE_TABLE_CAP).  A spec needs step == 1
 * (SDPGPU_ERR_UNSUPPORTED otherwise); a tile works at any step.  Host arithmetic only. */
int sdpgpu_set_sampler(sdpgpu_handle* h, int32_t t, const sdpgpu_dist_spec* spec);
typedef struct sdpgpu_sim_result {
  int32_t n_paths;
  int32_t n_valid;   /* paths with bit 0 of their flags set (they stayed on the grid) */
  int32_t n_lost;    /* family SURVIVAL: paths with bit 1 set (a demand was lost), else 0 */
  int32_t reserved;
  double mean;       /* mean of the path sums; SURVIVAL: the share of paths that held negative cash */
  double m2;         /* sum over paths of (sum_p - mean)^2, a second pass over the device-resident sums */
  double kernel_ms;  /* HIP-event time of the kernels of this call (rollout, both reductions; the copies are outside) */
} sdpgpu_sim_result;
/* Sample n_paths (1 .. 2^24) demand paths, roll the computed policy along them and reduce, all on the device.  discount:
 * NULL = all 1.0 (the bits of an explicit array of ones), else T weights as in sdpgpu_simulate.  Start state, off-grid start
 * and the meaning of a path's sum and flags as in sdpgpu_simulate, whose per-period statements this kernel shares: out_sum
 * (NULL or n_paths) and out_valid (NULL or n_paths) equal sdpgpu_simulate on the demands sdpgpu_sample_demands returns, bit for
 * bit.  mean and m2 are formed in an order fixed by n_paths alone, without floating-point atomics: the same bits on every
 * call with the same arguments.  If any path left the grid (n_valid < n_paths: an unclamped family under a spec whose draws
 * leave the pmf support) mean and m2 are NaN and the status is still SDPGPU_OK.  Refusals as sdpgpu_simulate (STAFF, user
 * functors, cash_formula 2, world_size != 1, nothing solved); argument errors name the argument; all validation comes before
 * the first device call. */
int sdpgpu_simulate_sampled(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path,
                            const double* discount, double ini_x, double ini_cash, double ini_preq, sdpgpu_sim_result* result,
                            double* out_sum, uint8_t* out_valid);
/* The demands (and, when out_u is not NULL, the uniforms) sdpgpu_simulate_sampled uses, from the same device functions:
 * out[p * T + t].  Needs the pmfs (or specs) and a device, not a solve. */
int sdpgpu_sample_demands(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path, double* out_demand,
                          double* out_u);

/* ---- STAFF family: a hiring rule rolled out on a sampled tree --------------------------------------------------------
 * What `new SimulatesS(T, dimissionRate).simulatesS(initialState, sS)` does (SimulatesS.java:33-87, the draws of
 * Sampling.java:110-124 made reproducible), on the device in one call; the two calls per instance of WorkforceTesting.main
 * (WorkforceTesting.java:112-165) are one call with n_rules = 2.  Definition: DESIGN 4, "Workforce rollout on a sampled tree".
 *   tree     sample_nums[t] >= 1 children per node of depth t (t = 0 .. T-1), N = their product leaves, 1 <= N <= 2^24.  Leaf
 *            p passes node n_t = p div stride_t (stride_t = product of sample_nums[s], s > t); child digit j = n_t mod
 *            sample_nums[t], parent i = n_t div sample_nums[t]: the reference's `i * K + j` order (SimulatesS.java:45-50).
 *   uniform  of (t, parent i, child j): the latin hypercube of SDPGPU_SAMPLE_LHS above with n = sample_nums[t], instance
 *            position i, period index t, path j -- every node draws its own hypercube of its children.
 *   rule     ss != NULL: n_rules (1 .. 64) level rules, ss[(r * T + t) * 2 + {0, 1}] = (s, S) of period t + 1, truncated toward
 *            zero like Java's (int); the period hires S - x when x < s, else nobody, in every period (SimulatesS.java:55).  Needs
 *            no solve; the staff number may leave every box of an unclamped handle.  ss == NULL (n_rules = 1): the handle's
 *            computed policy table; a staff number outside the period's box ends the leaf with its valid flag clear.
 *   turnover hireTo = x + hires; hireTo <= 0: 0 (SimulatesS.java:64-67); else from row min(hireTo, n_rows - 1) of the period's
 *            level pmf, the row the recursion integrates over (StaffRecursion.java:92-95): thresholds = the running fp64 sum of
 *            the row, the last one +infinity, turnover = #{thresholds <= u}.
 *   step     the period's cost and the next staff number as the recursion forms them (one fp64 operation per statement, the
 *            two-sided clamp when the handle clamps); a leaf's sum adds the periods' costs in order.
 * results[r] (n_rules of them): n_paths = N, n_valid, n_lost = 0, mean and m2 of the rule's leaf sums in the fixed order of
 * sdpgpu_simulate_sampled (NaN when n_valid < N), kernel_ms of the whole call.  m2 is the SPREAD OF THE LEAF SUMS, not a variance
 * of the mean: leaves share prefixes of their paths, so m2 / (N (N - 1)) is no standard error.  The counters of the uniforms do
 * not carry the rule: every rule sees the same uniforms, and a call with R rules returns what R calls with one rule each
 * return, bit for bit.  Optional outputs: out_sum[r * N + p], out_valid[r * N + p] (1 = valid), out_demand[(r * N + p) * T + t]
 * (the turnover drawn, -1 in the periods an ended leaf did not reach).
 * Refusals, all before the first device call and naming the argument: not a STAFF handle SDPGPU_ERR_UNSUPPORTED; world_size
 * != 1, a level pmf missing, the table rule before a solve SDPGPU_ERR_STATE; sample_nums[t] < 1 or more than 2^24 leaves,
 * n_rules outside 1 .. 64, an ss entry not finite or outside int32, (int) S < (int) s - 1 (a negative hire), ini_x not an
 * integer in 0 .. 1e9, ini_x outside period 1's box under the table rule, a negative probability in a level pmf
 * SDPGPU_ERR_ARG. */
int sdpgpu_staff_simulate(sdpgpu_handle* h, const int32_t* sample_nums, uint64_t seed, double ini_x, const double* ss,
                          int32_t n_rules, sdpgpu_sim_result* results, double* out_sum, uint8_t* out_valid, int32_t* out_demand);

/* ---- batched workforce fit and rollout: the rest of WorkforceTesting.main's loop body for the whole sweep --------------
 * After the solve every instance of the sweep runs `getOptTable()`, `new FitsS(Integer.MAX_VALUE, T).getSinglesS(optTable)`
 * and two `SimulatesS.simulatesS(initialState, sS)` (WorkforceTesting.java:112-165).  The three calls below do that for ALL
 * instances of a STAFF batch (sdpgpu_batch_create above) without a handle per instance and without a policy table on the host.  Definition: DESIGN 4,
 * "Workforce batch: fit and rollout".  Additive to ABI 6; on a batch of the backorder family each returns
 * SDPGPU_ERR_UNSUPPORTED, naming the call and the family.
 *
 * sdpgpu_batch_staff_reachable: the ONE interval [*lo, *hi] of staff numbers StaffRecursion.getExpectedValue visits in `period`
 * (1-based) from (1, iniStaffNum) -- the rows of getOptTable for that period, what sdpgpu_reachable marks on a handle of the
 * instance.  From the levels y in [L, H + maxHire] the successors are the union of [y - len(y) + 1, y]; the clamp maps an
 * interval to an interval.  Host arithmetic only; reads the instance's tables of the periods before `period`:
 * SDPGPU_ERR_STATE names the first (instance, period) without one.
 *
 * sdpgpu_batch_staff_fit_ss: `FitsS(max_order_quantity, T).getSinglesS` on every instance's getOptTable rows, on the device --
 * one launch over the (instance, period) slices of the policy arena the intervals above cut out, one copy back:
 * out[(i * T + t) * 2 + {0, 1}] = (s, S) of period t + 1, bit for bit sdpgpu_fit_ss(1, T, max_order_quantity, rows of instance i).
 * max_order_quantity is the CALLER's value, not the hire limit (the drivers pass Integer.MAX_VALUE).  SDPGPU_ERR_STATE before
 * sdpgpu_batch_solve; SDPGPU_ERR_ARG for a limit that is not finite or is negative.
 *
 * sdpgpu_batch_staff_simulate: sdpgpu_staff_simulate (above) for every instance in ONE rollout launch, then the fixed-order
 * reduction of every (instance, rule).  Tree, uniforms, turnover walk, period step, clamp, valid flag and the order of the
 * mean's sum are those of sdpgpu_staff_simulate word for word -- the kernels share the period step.
 *   rule     ss != NULL: n_rules (1 .. 64) level rules PER INSTANCE, ss[((i * n_rules + r) * T + t) * 2 + {0, 1}], truncated
 *            toward zero; needs no solve.  ss == NULL (n_rules = 1): every instance's own policy table; needs a solved batch.
 *   outputs  results[i * n_rules + r]; optional out_sum[(i * n_rules + r) * N + p], out_valid likewise,
 *            out_demand[((i * n_rules + r) * N + p) * T + t].
 * The uniforms' counters carry neither the rule nor the instance: all instances see common random numbers, and instance i,
 * rule r returns bit for bit -- leaf sums, flags, draws, n_valid, mean, m2 -- what sdpgpu_staff_simulate returns on a handle of
 * instance i with the same seed, sample_nums and ini_x.  Every result carries the kernel_ms of the whole call
 * (sdpgpu_batch_simulate_ms stays -1 on a STAFF batch).
 * Refusals, all before the first device call and naming the argument: a level table missing, the table rule before a solve
 * SDPGPU_ERR_STATE; sample_nums[t] < 1 or more than 2^24 leaves per rule, n x n_rules x N above 2^28 (2 GiB of leaf sums),
 * n_rules outside 1 .. 64, n_rules != 1 with ss == NULL, an ss entry not finite or outside int32, (int) S < (int) s - 1, ini_x
 * not an integer in 0 .. 1e9, ini_x outside period 1's box under the table rule, a negative or NaN probability in a pool table
 * in use (named by its id; every table is looked at once) SDPGPU_ERR_ARG. */
int sdpgpu_batch_staff_reachable(sdpgpu_batch* b, int32_t instance, int32_t period, int64_t* lo, int64_t* hi);
int sdpgpu_batch_staff_fit_ss(sdpgpu_batch* b, double max_order_quantity, double* out);
int sdpgpu_batch_staff_simulate(sdpgpu_batch* b, const int32_t* sample_nums, uint64_t seed, double ini_x, const double* ss,
                                int32_t n_rules, sdpgpu_sim_result* results, double* out_sum, uint8_t* out_valid,
                                int32_t* out_demand);

/* ---- workforce structure rows: G(y) of the STAFF family and CheckKConvexity on them --------------------------------------
 * The last step of WorkforcePlanning.main (WorkforcePlanning.java:165-211): a second StaffRecursion whose lambdas ignore the
 * action in period 1 (:171-195), `getExpectedValue(new StaffState(1, y), y)` for y = minX .. maxX through
 * StaffRecursion.java:127-172 (:200-205), and CheckKConvexity.check(yG, fixCost) (:208-209).  Here no second recursion is
 * built: an entry is one serial sum against the V_{t+1} a solved handle or batch already holds, for ANY period.  Definition and
 * the relation to the reference: DESIGN 4, "Workforce structure rows".  Additive to ABI 6.
 *
 * G_t(y) for period t in 1 .. T and level y in 0 .. n_rows_t - 1, row = pmfs[t - 1][y] with len(y) entries, in fp64 without
 * FMA, j ascending from g = 0.0:
 *     n = y - j;  pen = n > minStaff_t ? 0.0 : unitPenalty * (double)(minStaff_t - n)
 *     g += p_row[j] * (((0.0 + unitVariCost * (double)y) + salary * (double)n) + pen)
 *     if t < T:  g += p_row[j] * V_{t+1}(nn),   nn = n, clamped (upper bound first, then lower) when clamp_inventory = 1
 * hireUpStaffNum is not an argument: the reference never reads it.  G_1(y) equals the loop of StaffRecursion.java:127-172 run at
 * every period over the driver's second lambdas, bit for bit, when no state x of periods 2 .. T that those sums reach has
 * x + policy(x) > n_rows - 1 (that loop skips such actions, :148-149; the solved recursion integrates them over the last row,
 * :93-94).  (In the Java text the inner call at :161 has one argument, i.e. the method of :81-118 with the second lambdas, which
 * differ from the solved ones in periods 2 .. T only by the missing clamp.)
 * A level y >= n_rows_t is SDPGPU_ERR_ARG (the reference `continue`s past every action there).  A level is OFF THE GRID when a
 * successor nn, j < len(y), lies outside the stored grid [x_lo, x_lo + nx) of period t + 1, zero-probability entries included:
 * SDPGPU_ERR_ARG naming the first such level and successor; nothing is written.
 *
 * sdpgpu_staff_gy_host: the sum on the host, no device, the tables from anywhere: prob[y * row_stride + j] with row_len[y]
 * entries in row y (NULL: y + 1), v_next[nn - v_x_lo] for v_nx staff numbers (NULL: period T, no future term), the clamp flag
 * and its bounds; out[k] = G(y_lo + k), k < n.  What the device calls are held to, bit for bit (one function for both sides).
 * Errors through sdpgpu_batch_last_error(NULL).
 * sdpgpu_staff_gy: the same levels of `period` of a solved STAFF handle, AUTO or SEPARABLE alike (it reads V only), in ONE
 * launch (lanes of a wave = 64 consecutive levels, each walking its row serially).  SDPGPU_ERR_STATE before a solve and, on a
 * ping-pong handle (store_all_values = 0), once V_{period+1} has been overwritten; SDPGPU_ERR_UNSUPPORTED for world_size > 1,
 * another family or a user functor.
 * sdpgpu_staff_gy_range: the first maximal run *y_lo .. *y_hi of levels of `period` that are not off the grid (*y_lo > *y_hi:
 * none).  Host arithmetic only.
 * sdpgpu_staff_check_convexity: CheckKConvexity (kind as sdpgpu_check_convexity) on one row of the handle: source 0 = V_period
 * over the staff numbers lo .. hi, source 1 = G_period over the levels lo .. hi, formed and checked on the device; bit for bit
 * sdpgpu_check_convexity on the read-back row.  More than 8192 points: SDPGPU_ERR_UNSUPPORTED.
 * sdpgpu_batch_staff_gy: n levels from y_lo of G_period of one instance of a solved STAFF batch.  The rows of ALL instances and
 * periods -- per row the first run of levels that are not off the grid -- are formed in ONE launch at the first request after
 * a solve and kept on the device; a re-solve drops them (sdpgpu_batch_set_overhead may change minStaffNum between solves).
 * Every row is bit for bit sdpgpu_staff_gy on a separable handle of the instance.  SDPGPU_ERR_STATE before a solve and for a
 * period whose V_{period+1} was overwritten (store_all_values = 0 keeps G_1 and G_T).
 * sdpgpu_batch_staff_check_convexity: the check on one row of EVERY instance in one launch; lo / hi (n each, or both NULL: the
 * period's staff numbers for source 0, the kept levels for source 1), K NULL = each instance's fixed_order_cost, capacity NULL =
 * (int)max_order_quantity; out: n structs, written only on success.
 * sdpgpu_batch_gy and sdpgpu_batch_check_convexity keep refusing a STAFF batch; the two calls here refuse a backorder batch. */
int sdpgpu_staff_gy_host(double unit_vari_cost, double salary, double unit_penalty, int32_t min_staff, const double* prob,
                         const int32_t* row_len, int32_t n_rows, int32_t row_stride, const double* v_next, int32_t v_x_lo,
                         int64_t v_nx, int32_t clamp, int32_t min_x, int32_t max_x, int32_t y_lo, int32_t n, double* out);
int sdpgpu_staff_gy(sdpgpu_handle* h, int32_t period, int32_t y_lo, int32_t n, double* out);
int sdpgpu_staff_gy_range(sdpgpu_handle* h, int32_t period, int32_t* y_lo, int32_t* y_hi);
int sdpgpu_staff_check_convexity(sdpgpu_handle* h, int32_t kind, int32_t source, int32_t period, int32_t lo, int32_t hi, double K,
                                 int32_t capacity, sdpgpu_convexity* out);
int sdpgpu_batch_staff_gy(sdpgpu_batch* b, int32_t instance, int32_t period, int32_t y_lo, int32_t n, double* out);
int sdpgpu_batch_staff_check_convexity(sdpgpu_batch* b, int32_t kind, int32_t source, int32_t period, const int32_t* lo,
                                       const int32_t* hi, const double* K, const int32_t* capacity, sdpgpu_convexity* out);

/* ---- CASH family: (s, C, S) ordering rules rolled out along sampled demand paths -------------------------------------
 * What CashSimulation.simulatesCS with (s, C1(x), C2(x), S) (CashSimulation.java:996-1042), simulatesCS with (s, C1(x), S)
 * (:1050-1093) and simulatesMeanCS (:1101-1134) do after a solve, on the device; the four calls of CashConstraintTesting.main
 * (CashConstraintTesting.java:187, 201, 216, 241) are one call with n_rules = 4.  Definition: DESIGN 4, "Cash rule rollout".
 * Additive to ABI 6.
 *   handle   family CASH with cash_formula 0 or 1.  Needs the pmf tiles (or a spec on every period without one) and a device,
 *            NOT a solve: the rule replaces the policy table.
 *   draws    n_paths, seed, mode, first_path as sdpgpu_simulate_sampled: sdpgpu_sample_demands returns the demands EVERY rule
 *            of the call sees (the counters do not carry the rule).
 *   rule r   form[r] one of the three below; rule[(r * T + t) * 4 + {0, 1, 2, 3}] = (s, c1, c2, S) of period index t; optional
 *            dense threshold tables c1_tab, c2_tab [(r * T + t) * NX + ix], NX = the descriptor's inventory points
 *            ((int)((max_inventory - min_inventory) / step) + 1), entry ix keyed by x = min_inventory + ix * step, NaN = key
 *            absent, a NULL table = every key absent, entries of t = 0 not read.  A lookup at x hits only where x IS that
 *            double (TreeMap.get(new State(period, x))).
 *   period   t >= 1: m = max(0, (cash - min_cash_required - fix_order_cost) / vari_cost); form 0: m = (double)(int)m; m =
 *            min(m, max_q).  Below s (x < s): forms 0, 1 read c1 from the table (absent: 0.0), form 0 reads c2 (absent:
 *            10000.0), form 2 keeps the row's c1.  q = min(m, S - x) when x < s and cash > c1 (form 0: and cash < c2), else 0.
 *            t = 0: q = x < s ? S - x : 0; form 1 then takes min(q, max(0, (cash - min_cash_required - fix_order_cost) /
 *            vari_cost)).  A negative q is not refused.  The four scalars are the reference's ARGUMENTS; the descriptor's own
 *            costs enter through the family's statements below.
 *   step     sum += discount[t] * immediateValue(state, q, d); state = stateTransition(state, q, d): the CASH family's
 *            statements with the order quantity as a double (per-period overhead, salvage in period T, penalty, both clamps,
 *            the cash quantiser; one fp64 operation per statement, no contraction).  The state is the two doubles (x, cash):
 *            the inventory may leave the grid, no path ever becomes invalid.  discount NULL = all 1.0.
 * results[r] (n_rules of them): n_paths, n_valid = n_paths, n_lost = 0, mean and m2 of the rule's path sums in the fixed order
 * of sdpgpu_simulate_sampled, kernel_ms of the whole call.  out_sum: NULL or [r * n_paths + p].  A call with R rules returns
 * what R calls with one rule each return, bit for bit; RANDOM calls (0, a) then (a, b) give the sums of one call (0, a + b).
 * Refusals, all before the first device call and naming the argument: not a CASH handle, cash_formula 2, a user functor,
 * n_paths above 2^24 SDPGPU_ERR_UNSUPPORTED; world_size != 1, a period without tile or spec SDPGPU_ERR_STATE; n_paths < 1, a
 * bad mode, LHS with first_path != 0, n_rules outside 1 .. 16, a form outside 0 .. 2, a rule entry, start value or scalar
 * that is not finite, vari_cost <= 0, max_q < 0, a NULL form, rule or results, an infinite table entry SDPGPU_ERR_ARG. */
#define SDPGPU_RULE_SC12S 0   /* (s, C1(x), C2(x), S) */
#define SDPGPU_RULE_SC1S 1    /* (s, C1(x), S) */
#define SDPGPU_RULE_SMEANCS 2 /* (s, C, S), C the row's own c1 */
int sdpgpu_cash_rule_simulate(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path,
                              const double* discount, double ini_x, double ini_cash, int32_t n_rules, const int32_t* form,
                              const double* rule, const double* c1_tab, const double* c2_tab, double min_cash_required,
                              double max_q, double fix_order_cost, double vari_cost, sdpgpu_sim_result* results, double* out_sum);

/* ---- CASH family, cash_formula 2: the (x, R) state of CashConstraintXR rolled out along demand paths -------------------
 * What CashSimulationXR.simulateSDPGivenSamplNum (CashSimulationXR.java:91-113), the sampling loop of
 * simulateSDPwithErrorConfidence (:115-147) and simulateAStar (:153-173) do after CashConstraintXR.main's solve, on the device.
 * Definition: DESIGN 4, "(x, R) rollout".  Additive to ABI 6.  sdpgpu_simulate, sdpgpu_simulate_sampled, sdpgpu_sample_demands
 * and sdpgpu_cash_rule_simulate keep refusing such a handle: this is the family's entry point of its own.
 *   handle   family CASH with cash_formula 2, world_size 1, no user functor.
 *   demands  demand == NULL: drawn on the device -- n_paths, seed, mode, first_path exactly as sdpgpu_simulate_sampled
 *            (latin hypercube or plain random, instance position 0; RANDOM calls (0, a) then (a, b) continue one stream) from
 *            the pmf tiles or the specs of sdpgpu_set_sampler.  demand != NULL (GIVEN): the caller's demand[p * T + t]; seed,
 *            mode and first_path are not read.  The counters do not carry the rule: every rule of a call sees the same demands.
 *   table    levels == NULL, n_rules 1: the handle's policy table, needs a solve.  Per period the statements of
 *   rule     sdpgpu_simulate (optQ = getAction(state), immediateValue, stateTransition); a period-1 state (ini_x, ini_r) off
 *            the grid takes its action from sdpgpu_eval_states.  Both clamps are in the transition: from a grid state no
 *            path leaves the grid.  From a start whose INVENTORY is off the grid the period-1 successor is a grid state only
 *            where the period sells out or fills the shelf; any other path ends there (the reference would re-enter its
 *            recursion at a state no table holds): out_sum keeps period 1's term, n_valid < n_paths, mean and m2 are NaN, as
 *            with sdpgpu_simulate_sampled; the action of such a start values a successor that is no grid state at 0.
 *   level    levels[r * T + t] = a_t of rule r, n_rules 1 .. 16, needs NO solve and no layout.  The state is the two doubles
 *   rule     (x, R), any finite start.  Period index t: y = R > vari_cost * a_t ? a_t : R / vari_cost (:162; a y below x is not
 *            refused: the reference sells stock back at cost there); sum += discount[t] * immediateValue(state, y, d) -- the
 *            statements of CashConstraintXR.java:78-91 with the level itself (action = y - x, fixed = y > x ? K : 0, initCash =
 *            R - v * x, revenue = price * min(y, d), inventoryLevel = y - d: the level before demand is y, not x + (y - x)) --;
 *            state = stateTransition(state, y, d) (:94-110: nextInv = max(0, y - d), nextCash = initCash + imm, both clamps, the
 *            handle's cash quantiser, R' = nextCash + v * nextInv).  One fp64 operation per statement, no contraction.
 *            vari_cost is the reference's constructor ARGUMENT variOrderCost; v, K and the other costs are the descriptor's.
 *            recursion.getExpectedValue(state) of :161 is a memo side effect whose result is discarded: not mirrored.
 * results[r] (n_rules of them): n_paths, n_valid = n_paths (but for the case above), n_lost = 0, mean and m2 of the rule's path
 * sums in the fixed order of sdpgpu_simulate_sampled (no floating-point atomics), kernel_ms of the whole call.  out_sum: NULL or [r * n_paths + p];
 * out_demand: NULL or [p * T + t], the demands every rule saw.  A call with R rules returns what R calls with one rule each
 * return, bit for bit.  iniState.iniR (:110, :142, :170) is added by the caller.
 * Refusals, all before the first device call and naming the argument: not a CASH handle with cash_formula 2, a user functor,
 * n_paths above 2^24 SDPGPU_ERR_UNSUPPORTED; world_size != 1, a period without tile or spec while demand == NULL, the table rule
 * before a solve SDPGPU_ERR_STATE; n_paths < 1, a bad mode, LHS with first_path != 0, n_rules outside 1 .. 16, n_rules != 1
 * under the table rule, a level, start value, discount or given demand that is not finite, vari_cost <= 0 or not finite, NULL
 * results SDPGPU_ERR_ARG. */
int sdpgpu_xr_simulate(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path, const double* demand,
                       const double* discount, double ini_x, double ini_r, int32_t n_rules, const double* levels,
                       double vari_cost, sdpgpu_sim_result* results, double* out_sum, double* out_demand);
/* Chao's a* of every period: RecursionG.getOptY (RecursionG.java:80-153) over pmf tiles, host only and handle-free (as
 * sdpgpu_fit_ss; errors through sdpgpu_last_error(NULL)).  Period index t's tile is elements tile_off[t] .. tile_off[t + 1] - 1 of
 * tile_demand / tile_prob (tile_off[0] = 0).  The reference's two mutually recursive functions, literally: G (:96-123, the
 * statement order of :105-107 and :116-118) and getAStar (:130-153: the scan y = 0; y < max_y; y += 1 from optYValue = -1000,
 * a level taken only where it improves by MORE THAN 0.01); the memo of G is keyed by (period, y as a double).  The reference
 * hard-codes max_y = 200.  aNStar of the constructor (an SSJ quantile, :66-70) is overwritten by the loop of :83-86 before
 * anything reads it: it is not needed.  Math.pow(1 + depositeRate, T - n) is the host libm's pow: agreement with Java's is
 * claimed only where the result is exact (deposit_rate 0, the driver's case).  T x max_y x |pmf| operations per memo entry's
 * first visit; no device code.  SDPGPU_ERR_ARG: T < 1, max_y < 1, a NULL array, an empty tile, a value that is not finite. */
int sdpgpu_xr_opt_levels(int32_t T, const int64_t* tile_off, const double* tile_demand, const double* tile_prob, double price,
                         double vari_cost, double deposit_rate, double salvage, int32_t max_y, double* out_levels);

/* ---- User-functor handles (sdpgpu_create_custom): rollouts of the policy tables and of the overdraft drivers' rules ------
 * What the validation half of the overdraft drivers does after a solve, on the device: simulateSDPGivenSamplNum and the
 * sampling loop of simulateSDPwithErrorConfidence (CashOverdraftLimit.main:122-125), CashSimulation.simulatesSOD
 * (CashSimulation.java:1180-1211; CashOverdraftTesting.main:142-149, CashOverdraft.main:154-163), simulatesCSDraft (:1142-1173;
 * CashOverdraftLimitTesting.main:158) and simulatesSOD2 (:1218-1250).  Definition: DESIGN 4, "User-functor rollouts".  Additive
 * to ABI 6.  sdpgpu_simulate, sdpgpu_simulate_sampled, sdpgpu_sample_demands, sdpgpu_cash_rule_simulate and sdpgpu_xr_simulate
 * keep refusing a user-functor handle: these are its entry points.
 *
 * The rollout program -- two kernels around the handle's own text, the prelude and the helpers of the solve's program -- is
 * compiled by hipRTC at the handle's FIRST rollout call, kept on the handle and released by sdpgpu_destroy.  Options: those of
 * the solve's compile (shape, SDP_NP, the baked grid and constants) WITHOUT -fno-honor-nans.  The compile follows the argument
 * checks and precedes the solve-state and device checks: a text around which the program does not compile is SDPGPU_ERR_ARG on
 * a box without a GPU too.  SDPGPU_CUSTOM_DUMP=path writes the rollout object to path + ".sim".
 *
 * sdpgpu_custom_simulate / sdpgpu_custom_simulate_sampled: arguments, start state, off-grid start (its action is the
 * one sdpgpu_eval_states gives wherever that call answers; a start with a successor that is no grid point, which sdpgpu_eval_states
 * refuses, values that successor at 0 as the built-in families' rollouts do, and its path ends there), flags (bit 0: the path stayed on the grid), discount == NULL (sampled call only), NaN mean / m2 when
 * n_valid < n_paths and kernel_ms mean what they mean for sdpgpu_simulate / sdpgpu_simulate_sampled.  Per period: state =
 * decode(idx), action = policy[idx] * step, sum += discount[t] * immediate (one sdp_cell call under SDP_USER_CELL, else
 * sdp_immediate and, except in period T, sdp_transition), idx = index of the successor.  A successor that is no grid point of the
 * next period ends the path with its valid bit clear -- not an error.  The draws are exactly sdpgpu_simulate_sampled's (tiles or
 * sdpgpu_set_sampler specs, instance position 0, LHS or RANDOM); out_demand (optional, [p * T + t]) returns them.  n_paths * T
 * above 2^27 is SDPGPU_ERR_UNSUPPORTED (the demand buffer is resident).
 *
 * sdpgpu_custom_rule_simulate: handles of the (x, cash) state shape (descriptor family CASH or OVERDRAFT); needs NO solve.
 *   rule r   rule[(r * T + t) * 4 + {0, 1, 2, 3}] = (s, C, S, S2) of period index t; form[r] one of the three below.
 *            m = min(max(0, (cash - min_cash_required - fix_order_cost) / vari_cost), max_q).
 *            SS      t = 0: q = S (the row's S itself);    t >= 1: q = x < s ? min(m, S - x) : 0
 *            SCS     t = 0: q = S - s;                     t >= 1: q = (x < s && cash > C) ? min(m, S - x) : 0   (strict)
 *            SCS1S2  t = 0: q = S - ini_x;                 t >= 1: q = x < s ? (cash <= C + 0.1 ? S - x : S2 - x) : 0; reads no scalar
 *   step     sum += discount[t] * sdp_immediate(ctx{t + 1}, x, cash, 0, q, d); (x, cash) = sdp_transition(...), not in period T.
 *            The state is the two doubles the user's transition returns: nothing is tested against a grid, n_valid = n_paths, a
 *            negative q is not refused.  One fp64 operation per statement; min / max are the prelude's sdp_min / sdp_max.
 *   draws    as above; up to 16 rules see the same demands (the counters do not carry the rule).  A call with R rules returns
 *            what R one-rule calls return, bit for bit; RANDOM calls (0, a) then (a, b) give the sums of one call (0, a + b).
 * results[r]: n_paths, n_valid, n_lost = 0, mean and m2 in the fixed order of sdpgpu_simulate_sampled, kernel_ms of the whole
 * call; out_sum: NULL or [r * n_paths + p]; out_demand: NULL or [p * T + t].  iniState.iniCash is added by the caller.
 *
 * Refusals, all before the first device call and naming the argument: not a user-functor handle, state shape SURVIVAL, the rule
 * call on a shape without a cash axis or with a pipeline quantity, n_paths above 2^24, n_paths * T above 2^27
 * SDPGPU_ERR_UNSUPPORTED; world_size != 1, a period without tile or spec (drawn demands), the table calls before a solve
 * SDPGPU_ERR_STATE; a NULL array that is required, n_paths < 1 (sdpgpu_custom_simulate: < 0), a bad mode, LHS with first_path != 0,
 * n_rules outside 1 .. 16, a form outside 0 .. 2, a rule entry, start value or discount that is not finite, and -- where a form
 * reads them -- a scalar that is not finite, vari_cost <= 0, max_q < 0 SDPGPU_ERR_ARG. */
#define SDPGPU_ORULE_SS 0     /* simulatesSOD: (s, S) */
#define SDPGPU_ORULE_SCS 1    /* simulatesCSDraft: (s, C, S) */
#define SDPGPU_ORULE_SCS1S2 2 /* simulatesSOD2: (s, C, S1, S2) */
int sdpgpu_custom_simulate(sdpgpu_handle* h, int64_t n_paths, const double* demand, const double* discount, double ini_x,
                           double ini_cash, double ini_preq, double* out_sum, uint8_t* out_valid);
int sdpgpu_custom_simulate_sampled(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path,
                                   const double* discount, double ini_x, double ini_cash, double ini_preq,
                                   sdpgpu_sim_result* result, double* out_sum, uint8_t* out_valid, double* out_demand);
int sdpgpu_custom_rule_simulate(sdpgpu_handle* h, int32_t n_paths, uint64_t seed, int32_t mode, uint64_t first_path,
                                const double* discount, double ini_x, double ini_cash, int32_t n_rules, const int32_t* form,
                                const double* rule, double min_cash_required, double max_q, double fix_order_cost,
                                double vari_cost, sdpgpu_sim_result* results, double* out_sum, double* out_demand);

#if defined(__GNUC__)
/* ---- two-product rollout: the computed policy of the three solves above along demand paths, on the device -----------------
 * What `new CashSimulationMulti(...).simulateSDPGivenSamplNum[Multi](iniState)` (CashSimulationMulti.java:65-118) and
 * `new CashSimulationMultiXR(...).simulateSDPGivenSamplNum(iniState)` (CashSimulationMultiXR.java:61-88) do after the solve:
 * every path starts at the descriptor's period-1 state; for t = 0 .. T-1 the action pair of the current state is looked up
 * (recursion.getAction: order-up-to levels for the XR family), sum += discount[t] * immediateValue(state, action, demand) and
 * state = stateTransition(state, action, demand); after period T nothing is looked up.  The states lie on no grid, so the
 * look-up is a probe of a hash table over the memo's (period, state tuple) keys, built once per policy object.  The lead-time
 * family has no simulator in the reference; it gets the same loop over its own lambdas (MultiProductLeadtime.java:162-223).
 * The exact construction is DESIGN.md 4 ("Two-product rollout").  Additive to ABI 6; errors through
 * sdpgpu_multilead_last_error(); no C++ exception crosses these entry points. */
typedef struct sdpgpu_multi_policy sdpgpu_multi_policy;

/* The memo rows are those sdpgpu_multi_set_table received from a solve of the SAME descriptor
   (the oracle's memo of it serves equally).  capacity_log2: 0 = the smallest power of two
   >= 2 x rows, else any k with 2^k > rows.  Checked on the host before any device call: the descriptor as the solves check it;
   memo non-NULL with 1 <= rows <= capacity and non-NULL columns; 2^capacity_log2 > rows; periods within 1 .. T; tuples finite;
   action pairs inside the descriptor's box; exactly one period-1 row, equal to the descriptor's initial state
   (SDPGPU_ERR_ARG naming the argument).  A state that appears twice with the same action pair is kept once; with different
   pairs SDPGPU_ERR_ARG names the two rows.  xr: 0 = CashRecursionMulti, 1 = CashRecursionMultiXR (deposit_rate is read then). */
int sdpgpu_multilead_policy_create(const sdpgpu_multilead* k, const sdpgpu_multi_table* memo,
                                   int32_t capacity_log2, sdpgpu_multi_policy** out);
int sdpgpu_multicash_policy_create(const sdpgpu_multicash* k, int32_t xr, double deposit_rate,
                                   const sdpgpu_multi_table* memo, int32_t capacity_log2,
                                   sdpgpu_multi_policy** out);
void sdpgpu_multi_policy_destroy(sdpgpu_multi_policy* p);

/* getAction for n states on the device: found[i] = 0 where the memo holds no such state. */
int sdpgpu_multi_policy_lookup(sdpgpu_multi_policy* p, int64_t n, const int32_t* period,
                               const double* i1, const double* i2, const double* q1,
                               const double* q2, const double* cash,
                               int32_t* a1, int32_t* a2, uint8_t* found);

/* d1 / d2[path * T + t]: the demand pair of period t + 1, as the caller rounded it.
   discount: NULL = all 1.0, else T weights (the reference's Math.pow(discountFactor, t)).
   out_sum (NULL or n_paths): the path sums; out_valid (NULL or n_paths): bit 0 set when every look-up of the path hit.  A miss
   (a demand outside the pmf support leads to a state the recursion never visited; the reference re-enters the recursion
   there) ends the path and its sum is NaN.  result as sdpgpu_simulate_sampled fills it: mean and m2 in a fixed order (the same
   bits on every call with the same arguments), both NaN when n_valid < n_paths -- the status is still SDPGPU_OK.  n_paths
   1 .. 2^24 (above: SDPGPU_ERR_UNSUPPORTED). */
int sdpgpu_multi_policy_simulate(sdpgpu_multi_policy* p, int32_t n_paths, const double* d1,
                                 const double* d2, const double* discount,
                                 sdpgpu_sim_result* result, double* out_sum, uint8_t* out_valid);
/* The same with the demand pairs drawn on the device: one uniform per (path, period index t) from the streams of
   sdpgpu_simulate_sampled (SDPGPU_SAMPLE_LHS / _RANDOM with instance position 0; mode and first_path rules as there) picks a
   ROW of that period's joint tile -- thresholds = the running fp64 sum of the tile's probabilities in list order, the last one
   +infinity, row q = #{c <= u}; multilead: the pairs in the engine's order i1 * n2 + i2 with p = p1 * p2.  Paths drawn this
   way never leave the memo and their mean estimates V_1 without bias.  (The reference draws two independent columns per
   period, generateLHSamplesMultiProd) */
int sdpgpu_multi_policy_simulate_sampled(sdpgpu_multi_policy* p, int32_t n_paths, uint64_t seed,
                                         int32_t mode, uint64_t first_path, const double* discount,
                                         sdpgpu_sim_result* result, double* out_sum,
                                         uint8_t* out_valid);
/* Exactly what the sampled rollout draws: out_d1 / out_d2 / out_u [path * T + t]. */
int sdpgpu_multi_policy_sample(sdpgpu_multi_policy* p, int32_t n_paths, uint64_t seed,
                               int32_t mode, uint64_t first_path,
                               double* out_d1, double* out_d2, double* out_u /* may be NULL */);

#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SDPGPU_H */
