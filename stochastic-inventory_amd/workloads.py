"""Synthetic workloads = the BASELINE.json configs, as laid out in SURVEY.md section 8(d).

Deterministic, closed-form inputs (no RNG, no data files): a D-point period has support
d = 0..D-1 with p_d proportional to the Poisson(lambda_t) pmf renormalised over the support
(the shape GetPmf.java:123-124 produces), lambda_t = (D/2)(1 + 0.25 sin(2 pi t / T)), so every
period has a distinct PMF tile.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List

import numpy as np

from .functors import BackorderFunctor, CashFunctor, LeadtimeFunctor
from .states import OptDirection


def truncated_poisson_tile(lam: float, D: int) -> np.ndarray:
    """[[d, p_d]] for d = 0..D-1, p_d = Poisson(lam) pmf / sum over the support."""
    d = np.arange(D, dtype=np.float64)
    logp = -lam + d * math.log(lam) - np.array([math.lgamma(k + 1.0) for k in range(D)])
    p = np.exp(logp - logp.max())
    p = p / p.sum()
    return np.stack([d, p], axis=1)


def seasonal_pmf(T: int, D: int) -> List[np.ndarray]:
    return [truncated_poisson_tile((D / 2.0) * (1.0 + 0.25 * math.sin(2.0 * math.pi * (t + 1) / T)), D)
            for t in range(T)]


@dataclass
class Workload:
    name: str
    functor: object
    direction: OptDirection
    pmf: List[np.ndarray]
    note: str = ""

    @property
    def T(self) -> int:
        return len(self.pmf)

    def desc(self):
        return self.functor.to_desc(self.T, self.direction)

    def overhead(self):
        return self.functor.overheads(self.T) if hasattr(self.functor, "overheads") else None


def cfg1_sS(T: int = 12) -> Workload:
    """configs[0]: single-item (s,S), Poisson(10) truncated at q = 0.9999 (support 0..24), 200 states."""
    f = BackorderFunctor(fixedOrderingCost=500, variOrderingCost=0, holdingCost=2, penaltyCost=10,
                         minInventory=-100, maxInventory=99, maxOrderQuantity=100, iniInventory=0)
    pmf = [truncated_poisson_tile(10.0, 25) for _ in range(T)]
    return Workload("cfg1_sS_200x101x25", f, OptDirection.MIN, pmf, "src/sdp Recursion plumbing case")


def cfg2_clsp(T: int = 52, S: int = 10000, A: int = 200, D: int = 100) -> Workload:
    """configs[1]: capacitated lot sizing, 1e4 states x 200 actions x 100 demands, 52 periods."""
    f = BackorderFunctor(fixedOrderingCost=500, variOrderingCost=1, holdingCost=2, penaltyCost=10,
                         minInventory=-(S // 2), maxInventory=S - S // 2 - 1, maxOrderQuantity=A - 1,
                         iniInventory=0)
    return Workload(f"cfg2_clsp_{S}x{A}x{D}x{T}", f, OptDirection.MIN, seasonal_pmf(T, D),
                    "src/capacitated CLSP.f")


def cfg3_cash(T: int = 6, NX: int = 200, NC: int = 5000, A: int = 300, D: int = 150) -> Workload:
    """configs[2]: cash-constrained 2-D state (inventory x cash), 1e6 states x <=300 actions x 150."""
    f = CashFunctor(price=10, fixOrderCost=0, variCost=1, holdingCost=0, depositeRate=0, overheadCost=0,
                    overheadRate=0, salvageValue=0.5, penaltyCost=0, discountFactor=1.0,
                    maxOrderQuantity=A - 1, minInventoryState=0, maxInventoryState=NX - 1,
                    minCashState=0, maxCashState=NC - 1, cashRoundMult=1.0, cashRoundDiv=1.0,
                    cashRoundIntDiv=True, cashFormula=0, iniInventory=0, iniCash=100)
    return Workload(f"cfg3_cash_{NX}x{NC}x{A}x{D}x{T}", f, OptDirection.MAX, seasonal_pmf(T, D),
                    "src/cash CashConstraint via CashRecursion, cash quantum 1")


def cfg4_leadtime(T: int = 50, NX: int = 1000, A: int = 200, D: int = 100) -> Workload:
    """configs[3]: the lead-time pipeline state of src/leadtime -- (period, inventory, preQ), the three
    fields of the reference's LeadtimeState (LeadtimeState.java:10-20) -- at about 1e7 state cells
    (50 periods x 1000 inventory points x 200 pipeline quantities), 200 actions, 100 demands; lead time 1
    exactly as Leadtime.java, on a clamped synthetic grid."""
    f = LeadtimeFunctor(fixedOrderingCost=0, variOrderingCost=1, holdingCost=2, penaltyCost=10,
                        maxOrderQuantity=A - 1, clampInventory=True, minInventory=-50,
                        maxInventory=NX - 51, iniInventory=0, iniPreQ=0)
    return Workload(f"cfg4_leadtime_{NX}x{A}q_{A}x{D}x{T}", f, OptDirection.MIN, seasonal_pmf(T, D),
                    "src/leadtime via LeadtimeRecursion")


def cfg4_pipeline(T: int = 4, NX: int = 250, A: int = 200, D: int = 100) -> Workload:
    """configs[3] as SURVEY.md section 8(d) lays it out: F2 generalised to lead time 2, 3-D state (x, q1, q2) with
    x in [-50, 199] and q1, q2 in [0, 199] = 1e7 states per period, 200 actions, 100 demands (2e11 cells per
    period), inventory clamped.  The reference has lead time 1 only (LeadtimeState.java:10-20): cfg4_leadtime is
    its exact shape, this one the synthetic generalisation."""
    f = LeadtimeFunctor(fixedOrderingCost=0, variOrderingCost=1, holdingCost=2, penaltyCost=10,
                        maxOrderQuantity=A - 1, clampInventory=True, minInventory=-50,
                        maxInventory=NX - 51, iniInventory=0, iniPreQ=0, leadTime=2, iniPreQ2=0)
    return Workload(f"cfg4_pipeline_{NX}x{A}q1x{A}q2_{A}x{D}x{T}", f, OptDirection.MIN, seasonal_pmf(T, D),
                    "src/leadtime generalised to a two-stage pipeline")


def cfg5_scaled(S: int, T: int = 3, A: int = 500, D: int = 200) -> Workload:
    """configs[4] / the north-star target grid: F1 scaled to S states, 500 actions, 200 demands."""
    f = BackorderFunctor(fixedOrderingCost=500, variOrderingCost=1, holdingCost=2, penaltyCost=10,
                         minInventory=0, maxInventory=S - 1, maxOrderQuantity=A - 1, iniInventory=0)
    return Workload(f"cfg5_f1_{S}x{A}x{D}x{T}", f, OptDirection.MIN, seasonal_pmf(T, D), "synthetic scaled F1")


def target_grid(T: int = 6, S: int = 1000000, A: int = 500, D: int = 200) -> Workload:
    """The grid BASELINE.json's target sentence is quoted on: 1e6 states x 500 actions x 200 demands (F1, the
    lambdas of capacitated.CLSP, CLSP.java:251-272), six periods = 6e11 cells per sweep."""
    w = cfg5_scaled(S=S, T=T, A=A, D=D)
    w.name = f"target_f1_{S}x{A}x{D}x{T}"
    w.note = "north-star target grid"
    return w


def cfg3_tenths(T: int = 6, NX: int = 501, maxCash: float = 2000.0, A: int = 101, D: int = 25) -> Workload:
    """configs[2]'s family at the size and cash quantum of the reference's own driver, cash.singleItem.CashConstraint
    .main (CashConstraint.java:44-68,131): cash in TENTHS (Math.round(cash * 10) / 10.0), inventory 0..500, cash
    0..2000 = 501 x 20001 states, orders 0..100, Poisson(10) demand truncated to 25 points, six periods.  Nothing is
    dyadic here, so the uniform-shift kernel does not apply: this is the cash row kernel's workload."""
    f = CashFunctor(price=10, fixOrderCost=0, variCost=1, holdingCost=0, depositeRate=0, overheadCost=0, overheadRate=0,
                    salvageValue=0.5, penaltyCost=0, discountFactor=1.0, maxOrderQuantity=A - 1, minInventoryState=0,
                    maxInventoryState=NX - 1, minCashState=0, maxCashState=maxCash, iniInventory=0, iniCash=100)
    pmf = [truncated_poisson_tile(10.0, D) for _ in range(T)]
    return Workload(f"cfg3t_cash_tenths_{NX}x{int(maxCash * 10) + 1}x{A}x{D}x{T}", f, OptDirection.MAX, pmf,
                    "CashConstraint.main: cash quantum 0.1")


def f5_single_product_leadtime(T: int = 4, mean: float = 20.0) -> Workload:
    """cash.overdraft.SingleProductLeadtime at the size its header calls the limit of the Java code -- "4 periods, mean
    demand 20 ... 50 s ... maximum computational capacity for java, otherwise memory errors" (SingleProductLeadtime.java:22-24):
    F5 (CashLeadtimeRecursion), state (inventory 0..60, cash -200..300 in HUNDREDTHS, preQ 0..30) = 9.5e7 states per period,
    orders 0..30, Poisson(20) truncated at 0.9999 (GetPmf.java:82-134)."""
    from .functors import CashLeadtimeFunctor
    from .pmf import GetPmf, PoissonDist
    f = CashLeadtimeFunctor(price=5, variCost=1, salvageValue=0.5, maxOrderQuantity=30, minInventoryState=0,
                            maxInventoryState=60, minCashState=-200, maxCashState=300, r0=0, r2=0.1, r3=2, limit=500,
                            interestFreeAmount=0, iniInventory=0, iniCash=0, iniPreQ=0, overheadCosts=[0.0] * T)
    pmf = [np.asarray(t, dtype=np.float64) for t in GetPmf([PoissonDist(mean)] * T, 0.9999, 1).getpmf()]
    return Workload(f"f5_spl_61x50001x31q_31x{len(pmf[0])}x{T}", f, OptDirection.MAX, pmf,
                    "SingleProductLeadtime.main via CashLeadtimeRecursion, cash quantum 0.01")


@dataclass
class StaffWorkload:
    """workforce.StaffRecursion: the pmf depends on the hire-up-to level (StaffRecursion.java:93-95), so the workload carries a
    (T, levels, stride) table instead of per-period tiles; `overhead()` hands the engine minStaffNum[t]."""
    name: str
    functor: object
    level_pmf: np.ndarray
    note: str = ""
    pmf = None
    direction = OptDirection.MIN

    @property
    def T(self) -> int:
        return int(self.level_pmf.shape[0])

    def desc(self):
        return self.functor.to_desc(self.T)

    def overhead(self):
        return [float(m) for m in self.functor.minStaffNum]


def staff_testing(T: int = 8, maxHire: int = 1000, rate: float = 0.1) -> StaffWorkload:
    """The first of WorkforceTesting.main's 216 instances (WorkforceTesting.java:45-107): T = 8, hires 0..1000, no clamp
    (staff 0..7000 by period 8), binomial turnover at rate turnoverRates[0] tabulated for 1001 hire-up-to levels."""
    from .pmf import staff_level_pmf
    from .workforce import StaffFunctor
    f = StaffFunctor(fixCost=50, unitVariCost=20, salary=30, unitPenalty=50, minStaffNum=[40] * T, maxHireNum=maxHire,
                     clampStaff=False, iniStaffNum=0)
    one = staff_level_pmf([rate], maxHire + 1)
    return StaffWorkload(f"staff_testing0_{maxHire + 1}hires_x{T}", f, np.repeat(one, T, axis=0), "WorkforceTesting.main[0] via StaffRecursion")


def workforce_planning(maxHire: int = 500, maxX: int = 600) -> StaffWorkload:
    """WorkforcePlanning.main's own instance (WorkforcePlanning.java:33-69): T = 3, turnover 0.5, staff numbers clamped to
    0 .. 600, hires 0 .. 500, a table of 601 levels -- the instance whose G(y) the driver draws and checks (:165-211)."""
    from .pmf import staff_level_pmf
    from .workforce import StaffFunctor
    T = 3
    f = StaffFunctor(fixCost=100, unitVariCost=10, salary=20, unitPenalty=80, minStaffNum=[40] * T, maxHireNum=maxHire, minX=0,
                     maxX=maxX, clampStaff=True, iniStaffNum=0)
    return StaffWorkload(f"staff_planning_{maxX + 1}levels_{maxHire + 1}hires_x{T}", f, staff_level_pmf([0.5] * T, maxX + 1),
                         "WorkforcePlanning.main via StaffRecursion")


def workforce_testing_sweep(T: int = 8, maxHire: int = 1000) -> List[StaffWorkload]:
    """WorkforceTesting.main's 216 instances in its loop order (WorkforceTesting.java:17-51): 2 turnover rates (the loop stops
    at iRate < 2) x 3 fixCost x 3 salary x 3 unitPenalty x 4 minStaffNum rows; one shape (T = 8, hires 0..1000, no clamp,
    iniStaffNum 0).  Each rate's table is built ONCE and every instance holds a zero-stride view of it over the periods:
    copies would take 216 x 64 MB."""
    from .pmf import staff_level_pmf
    from .workforce import StaffFunctor
    turnoverRates = [0.1, 0.5, 0.9]
    fixCosts = [50, 1000, 2000]
    salarys = [30, 100, 200]
    unitPenaltys = [50, 250, 2200]
    minStaffs = [[40, 40, 40, 40, 40, 40, 40, 40], [10, 20, 30, 40, 50, 60, 70, 80], [80, 70, 60, 50, 40, 30, 20, 10],
                 [40, 50, 80, 60, 40, 50, 80, 60]]
    m = len(turnoverRates)
    out = []
    for iRate in range(2):
        one = staff_level_pmf([turnoverRates[iRate]], maxHire + 1)[0]
        table = np.broadcast_to(one, (T,) + one.shape)
        for iFix in range(m):
            for iSalary in range(m):
                for iPenalty in range(3):
                    for iMinStaff in range(m + 1):
                        f = StaffFunctor(fixCost=fixCosts[iFix], unitVariCost=20, salary=salarys[iSalary],
                                         unitPenalty=unitPenaltys[iPenalty], minStaffNum=[minStaffs[iMinStaff][t % 8] for t in range(T)],
                                         maxHireNum=maxHire, clampStaff=False, iniStaffNum=0)
                        out.append(StaffWorkload(f"staff_testing{len(out)}_{maxHire + 1}hires_x{T}", f, table,
                                                 f"WorkforceTesting.main[{len(out)}] via StaffRecursion"))
    return out


def workforce_testing_loop(sweep=None, mip_levels=None, sampleNums=None, seed: int = 12345, device: int = -1) -> dict:
    """The loop body of WorkforceTesting.main (WorkforceTesting.java:112-165) for a whole sweep (default:
    workforce_testing_sweep()) behind ONE batch: solve, FitsS(Integer.MAX_VALUE, T).getSinglesS, and the rollouts of the
    fitted levels -- and, when `mip_levels` (n, T, 2) is given, of the caller's (MIP) levels in a second rule slot of the same
    launch, on the same uniforms.  No per-instance handle and no policy table on the host.  Returns
        opt[n], hires[n]      V_1(iniStaffNum) and its hire count
        levels[n, T, 2]       the fitted (s, S)
        sim[n, R]             the rollout means, R = 1 or 2 (slot 1: mip_levels)
        gapPercent[n, R]      (sim - opt) * 100 / opt"""
    from .workforce import StaffRecursionBatch
    sweep = workforce_testing_sweep() if sweep is None else list(sweep)
    with StaffRecursionBatch([w.functor for w in sweep], [w.level_pmf for w in sweep], sweep[0].T, device=device) as rec:
        opt, hires = rec.initial()
        levels = rec.fitSinglesS(2 ** 31 - 1)
        rules = levels[:, None]
        if mip_levels is not None:
            mip = np.asarray(mip_levels, dtype=np.float64)
            if mip.shape != levels.shape:
                raise ValueError(f"mip_levels of shape {mip.shape}: expected {levels.shape}")
            rules = np.stack([levels, mip], axis=1)
        sim = rec.simulatesS(rules, sampleNums, seed)
    return {"opt": opt, "hires": hires, "levels": levels, "sim": sim, "gapPercent": (sim - opt[:, None]) * 100 / opt[:, None]}


# capacitated.CLSP's three lambdas (CLSP.java:251-272) as the HIP device text a driver hands to sdpgpu_create_custom when its
# lambdas are its own: params = {K, v, h, pi, minInventory, maxInventory, maxOrderQuantity}.  bench.py's `custom_clsp` entry
# runs configs[1] through this text, i.e. through the reference's actual plugin API (arbitrary closures) instead of the
# built-in family.
CLSP_LAMBDAS_HIP = r"""
__device__ int sdp_feasible_count(const sdp_ctx& c, double x, double cash, double preq) {
  return (int)(c.params[6] / c.step) + 1;
}
__device__ double sdp_immediate(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand) {
  double fixedCost = action > 0 ? c.params[0] : 0;
  double variableCost = c.params[1] * action;
  double inventoryLevel = x + action - randomDemand;
  double holdingCosts = c.params[2] * sdp_max(inventoryLevel, 0);
  double penaltyCosts = c.params[3] * sdp_max(-inventoryLevel, 0);
  double totalCosts = fixedCost + variableCost + holdingCosts + penaltyCosts;
  return totalCosts;
}
__device__ void sdp_transition(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand,
                               double& nx, double& ncash, double& npreq) {
  double nextInventory = x + action - randomDemand;
  nextInventory = nextInventory > c.params[5] ? c.params[5] : nextInventory;
  nextInventory = nextInventory < c.params[4] ? c.params[4] : nextInventory;
  nx = nextInventory;
  ncash = 0;
  npreq = 0;
}
"""


# The same lambdas with the LEVEL SHAPE declared (include/sdpgpu.h, SDP_SHAPE_LEVEL): immediate value = the action's cost + the
# cost of the level the demand leaves, next inventory = that level, clamped.  The engine tabulates the two functions per period
# with the driver's own compiled code and runs the F1 window kernel from the tables.
CLSP_LAMBDAS_LEVEL_HIP = r"""
#define SDP_SHAPE_LEVEL 1
__device__ double sdp_action_cost(const sdp_ctx& c, double action) {
  double fixedCost = action > 0 ? c.params[0] : 0;
  double variableCost = c.params[1] * action;
  return fixedCost + variableCost;
}
__device__ double sdp_level_cost(const sdp_ctx& c, double inventoryLevel) {
  double holdingCosts = c.params[2] * sdp_max(inventoryLevel, 0);
  double penaltyCosts = c.params[3] * sdp_max(-inventoryLevel, 0);
  return holdingCosts + penaltyCosts;
}
"""


def clsp_lambda_params(w: Workload):
    f = w.functor
    return [f.fixedOrderingCost, f.variOrderingCost, f.holdingCost, f.penaltyCost, f.minInventory, f.maxInventory,
            f.maxOrderQuantity]


def custom_clsp(**kw) -> Workload:
    """configs[1] with CLSP's lambdas handed over as user text (hipRTC) instead of the built-in F1 family."""
    w = cfg2_clsp(**kw)
    w.name = "custom_clsp_" + w.name[len("cfg2_clsp_"):]
    w.note = "configs[1] through sdpgpu_create_custom (CLSP's lambdas as HIP text)"
    w.custom_source = CLSP_LAMBDAS_HIP
    w.custom_params = clsp_lambda_params(w)
    return w


def custom_clsp_level(**kw) -> Workload:
    """configs[1] with CLSP's lambdas as user text of the level shape: hipRTC compiles the two cost functions, the F1 window
    kernel runs them from tables."""
    w = cfg2_clsp(**kw)
    w.name = "custom_clsp_level_" + w.name[len("cfg2_clsp_"):]
    w.note = "configs[1] through sdpgpu_create_custom, lambdas of the declared level shape"
    w.custom_source = CLSP_LAMBDAS_LEVEL_HIP
    w.custom_params = clsp_lambda_params(w)
    return w


# capacitated.CLSPTesting.main (CLSPTesting.java:33-56): the mean demands of its ten demand patterns and its cost grid
CLSP_TESTING_DEMANDS = (
    (10, 10, 10, 10, 10, 10, 10, 10),
    (15, 16, 15, 14, 11, 7, 6, 3),
    (3, 6, 7, 11, 14, 15, 16, 15),
    (15, 4, 4, 10, 18, 4, 4, 10),
    (12, 7, 7, 10, 13, 7, 7, 12),
    (2, 4, 7, 3, 10, 10, 3, 3),
    (5, 15, 26, 44, 24, 15, 22, 10),
    (4, 23, 28, 50, 39, 26, 19, 32),
    (11, 14, 7, 11, 16, 31, 11, 48),
    (18, 6, 22, 22, 51, 54, 22, 21),
)
CLSP_TESTING_K = (200.0, 300.0, 400.0)
CLSP_TESTING_V = (0.0, 1.0)
CLSP_TESTING_PAI = (5.0, 10.0, 20.0)
CLSP_TESTING_COEVAR = (0.1, 0.2, 0.3)


def clsp_testing_sweep(patterns=None) -> List[Workload]:
    """The instances of capacitated.CLSPTesting.main in its loop order (demand pattern, v, pai, K, coeVar;
    CLSPTesting.java:58-62): 10 x 2 x 3 x 3 x 3 = 540 F1 problems of ONE grid -- x in [-500, 500], orders 0..500, T = 8,
    h = 1, NormalDist(mean, coeVar * mean) demands through GetPmf at the 0.9999 quantile.  `patterns`: a subset of the
    demand patterns, numbered 1..10 as the reference's result file numbers them (54 instances each).  Every workload
    carries `pattern` and `coeVar`.  With coeVar 0.3 a mean of 9 or more puts the lower quantile below zero and GetPmf's
    (int) cast truncates it toward zero (GetPmf.java:87): those supports start at a negative demand."""
    from .pmf import GetPmf, NormalDist
    out = []
    tiles = {}  # (pattern, coeVar) -> pmf: the 18 cost combinations of a pattern share their demand tiles
    for ip in (range(1, len(CLSP_TESTING_DEMANDS) + 1) if patterns is None else patterns):
        mean = CLSP_TESTING_DEMANDS[ip - 1]
        for v in CLSP_TESTING_V:
            for pai in CLSP_TESTING_PAI:
                for K in CLSP_TESTING_K:
                    for cv in CLSP_TESTING_COEVAR:
                        if (ip, cv) not in tiles:
                            dists = [NormalDist(m, cv * m) for m in mean]
                            tiles[(ip, cv)] = [np.asarray(t, dtype=np.float64) for t in GetPmf(dists, 0.9999, 1).getpmf()]
                        f = BackorderFunctor(fixedOrderingCost=K, variOrderingCost=v, holdingCost=1, penaltyCost=pai,
                                             minInventory=-500, maxInventory=500, maxOrderQuantity=500, iniInventory=0)
                        w = Workload(f"clsp_testing_p{ip}_v{v:g}_pai{pai:g}_K{K:g}_cv{cv:g}", f, OptDirection.MIN,
                                     tiles[(ip, cv)], "CLSPTesting.main instance")
                        w.pattern, w.coeVar = ip, cv
                        out.append(w)
    return out


# capacitated.fitss.ThreeLevelFitsSTest.main (ThreeLevelFitsSTest.java:34-60): the mean demands of its ten demand patterns
# (the first six periods of each, `newLength = 6`) and its cost grid; One- and TwoLevelFitsSTest sweep the same values
FITSS_DEMANDS = (
    (30, 30, 30, 30, 30, 30),
    (6.6, 9.3, 11.1, 12.9, 16.8, 21.6),
    (45.9, 48.6, 49.8, 49.8, 48.6, 45.9),
    (36.3, 30, 23.7, 21, 23.7, 30),
    (47.1, 30, 12.9, 6, 12.9, 30),
    (62.7, 27.3, 9.9, 23.7, 1, 22.8),
    (5, 15.3, 45.6, 140.1, 80.4, 146.7),
    (14.1, 24.3, 70.8, 118.2, 49.2, 86.1),
    (13.2, 34.8, 79.2, 43.2, 43.8, 59.4),
    (14.7, 56.4, 19.2, 83.7, 135.9, 67.2),
)
FITSS_K = (500.0, 800.0, 200.0)
FITSS_V = (0.0, 5.0, 10.0)
FITSS_PAI = (15.0, 10.0, 5.0)
FITSS_CAPACITY = (2.0, 3.0, 4.0)


def fitss_sweep(levels: int = 3, patterns=None) -> List[Workload]:
    """The instances of capacitated.fitss.ThreeLevelFitsSTest.main in its loop order (K, v, pai, demand pattern, capacity;
    ThreeLevelFitsSTest.java:67-71): 3 x 3 x 3 x 10 x 3 = 810 F1 problems -- x in [-300, 800], T = 6, h = 1, Poisson demands
    through GetPmf at the 0.999 quantile -- whose ORDER LIMIT is the instance's own: maxOrderQuantity =
    (int)(Math.round(mean of meanDemand) * capacity) (:76-77), 27 distinct values from 26 to 288.  One grid of states, 27
    numbers of actions: a ragged batch (SdpBatch(..., ragged=True)).  `levels` names the driver (1, 2, 3: One-, Two-,
    ThreeLevelFitsSTest); the instances are the same, the drivers differ in the level rule they fit afterwards
    (SdpBatch.fit_ss / simulate_ss_sampled with that number of levels).  `patterns`: a subset of the demand patterns, numbered 1..10 as the result file numbers them.  Every
    workload carries `pattern` and `capacity`."""
    from .pmf import GetPmf, PoissonDist
    if levels not in (1, 2, 3):
        raise ValueError(f"levels = {levels}: the reference has One-, Two- and ThreeLevelFitsSTest")
    pats = tuple(range(1, len(FITSS_DEMANDS) + 1)) if patterns is None else tuple(patterns)
    tiles = {}
    out = []
    for K in FITSS_K:
        for v in FITSS_V:
            for pai in FITSS_PAI:
                for ip in pats:
                    mean = FITSS_DEMANDS[ip - 1]
                    if ip not in tiles:
                        tiles[ip] = [np.asarray(t, dtype=np.float64)
                                     for t in GetPmf([PoissonDist(m) for m in mean], 0.999, 1).getpmf()]
                    for cap in FITSS_CAPACITY:
                        # Math.round is floor(x + 0.5); the product is exact (an integer times 2, 3 or 4)
                        q = int(math.floor(sum(mean) / len(mean) + 0.5) * cap)
                        f = BackorderFunctor(fixedOrderingCost=K, variOrderingCost=v, holdingCost=1, penaltyCost=pai,
                                             minInventory=-300, maxInventory=800, maxOrderQuantity=q, iniInventory=0)
                        w = Workload(f"fitss{levels}_K{K:g}_v{v:g}_pai{pai:g}_p{ip}_cap{cap:g}", f, OptDirection.MIN, tiles[ip],
                                     "ThreeLevelFitsSTest.main instance")
                        w.pattern, w.capacity = ip, cap
                        out.append(w)
    return out


SINGLE_CROSS_DEMANDS = [  # SingleCrossTesting.java:35-40
    [15, 15, 15, 15, 15, 15, 15, 15, 15, 15],
    [21.15, 18.9, 17.7, 16.5, 15.15, 13.95, 12.75, 11.55, 10.35, 9.15], [6.6, 9.3, 11.1, 12.9, 16.8, 21.6, 24, 26.4, 31.5, 33.9],
    [12.1, 10, 7.9, 7, 7.9, 10, 12.1, 13, 12.1, 10], [15.7, 10, 4.3, 2, 4.3, 10, 15.7, 18, 15.7, 10],
    [41.8, 6.6, 2, 21.8, 44.8, 9.6, 2.6, 17, 30, 35.4], [4.08, 12.16, 37.36, 21.44, 39.12, 35.68, 19.84, 22.48, 29.04, 12.4],
    [4.7, 8.1, 23.6, 39.4, 16.4, 28.7, 50.8, 39.1, 75.4, 69.4], [4.4, 11.6, 26.4, 14.4, 14.6, 19.8, 7.4, 18.3, 20.4, 11.4],
    [4.9, 18.8, 6.4, 27.9, 45.3, 22.4, 22.3, 51.7, 29.1, 54.7]]


def single_cross_testing(patterns=None, prices=(5, 6, 7), T: int = 2, max_inventory: float = 200, min_cash: float = -100,
                         max_cash: float = 1500, max_inventorys: int = 30, window_cash: int = 30) -> List[Workload]:
    """The 30 instances of cash.singleItem.SingleCrossTesting.main (SingleCrossTesting.java:35-91): 10 demand patterns x 3
    prices, T = 2, K = 10, v = 1, h = 0, no salvage, orders up to 150, inventory 0..200 x cash -100..1500, Poisson demand
    through GetPmf at 0.999.  Every workload carries its window -- levels 0 .. 30, cash 0 .. (int) K + 30 -- as
    `window = (minInventorys, maxInventorys, minCash, maxCash)` and the drawn `period` (1).  The keyword arguments shrink the
    grid and the window for tests."""
    from .pmf import GetPmf, PoissonDist
    out = []
    K = 10.0
    for ip in (patterns if patterns is not None else range(1, len(SINGLE_CROSS_DEMANDS) + 1)):
        mean = SINGLE_CROSS_DEMANDS[ip - 1][:T]
        tiles = [np.asarray(t, dtype=np.float64) for t in GetPmf([PoissonDist(m) for m in mean], 0.999, 1).getpmf()]
        for price in prices:
            f = CashFunctor(price=price, fixOrderCost=K, variCost=1, holdingCost=0, overheadCost=0, salvageValue=0, penaltyCost=0,
                            discountFactor=1.0, maxOrderQuantity=150, minInventoryState=0, maxInventoryState=max_inventory,
                            minCashState=min_cash, maxCashState=max_cash, cashRoundMult=1.0, cashRoundDiv=1.0, cashRoundIntDiv=True,
                            cashFormula=1, iniInventory=0, iniCash=0)
            w = Workload(f"single_cross_p{ip}_price{price:g}", f, OptDirection.MAX, tiles, "SingleCrossTesting.main instance")
            w.pattern, w.period = ip, 1
            w.window = (0, max_inventorys, 0, int(K) + window_cash)
            out.append(w)
    return out


def check_fg() -> Workload:
    """cash.singleItem.CheckFG.main's instance and window (CheckFG.java:30-47, :100-106): Poisson(8) x 3 at 0.9999, K = 10,
    v = 1, price 8, salvage 0.5, orders up to 200, inventory 0..500 x cash -100..2000; levels 0 .. 100, cash 0 .. 90."""
    from .pmf import GetPmf, PoissonDist
    tiles = [np.asarray(t, dtype=np.float64) for t in GetPmf([PoissonDist(8)] * 3, 0.9999, 1).getpmf()]
    f = CashFunctor(price=8, fixOrderCost=10, variCost=1, holdingCost=0, overheadCost=0, salvageValue=0.5, penaltyCost=0,
                    discountFactor=1.0, maxOrderQuantity=200, minInventoryState=0, maxInventoryState=500, minCashState=-100,
                    maxCashState=2000, cashRoundMult=1.0, cashRoundDiv=1.0, cashRoundIntDiv=True, cashFormula=1, iniInventory=0,
                    iniCash=13)
    w = Workload("check_fg", f, OptDirection.MAX, tiles, "CheckFG.main instance")
    w.period = 1
    w.window = (0, 100, 0, 10 + 80)
    return w


def by_name(name: str, **kw) -> Workload:
    table = {"cfg1": cfg1_sS, "cfg2": cfg2_clsp, "cfg3": cfg3_cash, "cfg3t": cfg3_tenths, "cfg4": cfg4_leadtime,
             "cfg4p": cfg4_pipeline, "target": target_grid, "f5_spl": f5_single_product_leadtime, "staff": staff_testing,
             "custom_clsp": custom_clsp, "custom_clsp_level": custom_clsp_level}
    if name in table:
        return table[name](**kw)
    if name == "cfg5":
        return cfg5_scaled(**kw)
    raise KeyError(name)
