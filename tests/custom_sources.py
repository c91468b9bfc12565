"""Lambdas of reference drivers written as HIP device text for sdpgpu_create_custom.  The same text is compiled
for the host by the oracle harness (oracle/sdpref.py: custom_functor), so both sides run the same three functions
and the test compares the ENGINES around them (loop, layout, arg-opt, discount)."""

# capacitated.CLSP's lambdas (CLSP.java:251-272); params = {K, v, h, pi, minInventory, maxInventory, maxOrderQuantity}
BACKORDER = r"""
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

# leadtime.Leadtime's lambdas (Leadtime.java:50-81, inventory clamp added); params = {K, v, h, pi, min, max, maxQ}
LEADTIME = r"""
__device__ int sdp_feasible_count(const sdp_ctx& c, double x, double cash, double preq) {
  return (int)(c.params[6] / c.step) + 1;
}
__device__ double sdp_immediate(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand) {
  double fixedCost = action > 0 ? c.params[0] : 0;
  double variableCost = c.params[1] * action;
  double inventoryLevel = x + preq - randomDemand;
  double holdingCosts = c.params[2] * sdp_max(inventoryLevel, 0);
  double penaltyCosts = c.params[3] * sdp_max(-inventoryLevel, 0);
  return fixedCost + variableCost + holdingCosts + penaltyCosts;
}
__device__ void sdp_transition(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand,
                               double& nx, double& ncash, double& npreq) {
  double nextInventory = x + preq - randomDemand;
  nextInventory = nextInventory > c.params[5] ? c.params[5] : nextInventory;
  nextInventory = nextInventory < c.params[4] ? c.params[4] : nextInventory;
  nx = nextInventory;
  ncash = 0;
  npreq = action;
}
"""

# cash.overdraft.CashOverdraftLimit's lambdas (CashOverdraftLimit.java:61-99) -- NOT one of the built-in families:
# simple interest / deposit on the balance before revenue, holding cost inside that balance, per-period overhead,
# `Math.round(nextCash * 10) / 10` (long division).
# params = {price, fixOrderCost, variCost, holdingCost, interestRate, depositeRate, salvageValue, maxOrderQuantity,
#           minInventoryState, maxInventoryState, minCashState, maxCashState, overheadCost[0..T-1]}
OVERDRAFT_LIMIT = r"""
__device__ int sdp_feasible_count(const sdp_ctx& c, double x, double cash, double preq) {
  double maxQ = c.params[7];  // CashOverdraftLimit.java:65: `maxQ = maxOrderQuantity` overrides the cash bound
  return (int)maxQ + 1;
}
__device__ double sdp_immediate(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand) {
  const double price = c.params[0], fixOrderCost = c.params[1], variCost = c.params[2], holdingCost = c.params[3];
  const double interestRate = c.params[4], depositeRate = c.params[5], salvageValue = c.params[6];
  double revenue = price * sdp_min(x + action, randomDemand);
  double fixedCost = action > 0 ? fixOrderCost : 0;
  double variableCost = variCost * action;
  double inventoryLevel = x + action - randomDemand;
  double holdCosts = holdingCost * sdp_max(inventoryLevel, 0);
  double cashBalanceBeforeRevenue = cash - fixedCost - variableCost - holdCosts - c.params[12 + c.period - 1];
  double interest = interestRate * sdp_max(-cashBalanceBeforeRevenue, 0);
  double deposite = depositeRate * sdp_max(cashBalanceBeforeRevenue, 0);
  double cashBalanceAfter = cashBalanceBeforeRevenue - interest + deposite + revenue;
  double cashIncrement = cashBalanceAfter - cash;
  double salValue = c.period == c.T ? salvageValue * sdp_max(inventoryLevel, 0) : 0;
  cashIncrement += salValue;
  return cashIncrement;
}
__device__ void sdp_transition(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand,
                               double& nx, double& ncash, double& npreq) {
  double nextInventory = sdp_max(0, x + action - randomDemand);
  double nextCash = cash + sdp_immediate(c, x, cash, preq, action, randomDemand);
  nextCash = nextCash > c.params[11] ? c.params[11] : nextCash;
  nextCash = nextCash < c.params[10] ? c.params[10] : nextCash;
  nextInventory = nextInventory > c.params[9] ? c.params[9] : nextInventory;
  nextInventory = nextInventory < c.params[8] ? c.params[8] : nextInventory;
  nextCash = sdp_trunc(sdp_round(nextCash * 10) / 10);  // Math.round(nextCash * 10) / 10: long / int
  nx = nextInventory;
  ncash = nextCash;
  npreq = 0;
}
"""

# the same lambdas with the FUSED callback (ABI 5): the increment is formed once per cell and both the immediate value and the
# successor are read off it; sdp_immediate / sdp_transition are calls of sdp_cell
OVERDRAFT_LIMIT_FUSED = r"""
#define SDP_USER_CELL 1
__device__ int sdp_feasible_count(const sdp_ctx& c, double x, double cash, double preq) {
  double maxQ = c.params[7];
  return (int)maxQ + 1;
}
__device__ void sdp_cell(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand,
                         double& imm, double& nx, double& ncash, double& npreq) {
  const double price = c.params[0], fixOrderCost = c.params[1], variCost = c.params[2], holdingCost = c.params[3];
  const double interestRate = c.params[4], depositeRate = c.params[5], salvageValue = c.params[6];
  double revenue = price * sdp_min(x + action, randomDemand);
  double fixedCost = action > 0 ? fixOrderCost : 0;
  double variableCost = variCost * action;
  double inventoryLevel = x + action - randomDemand;
  double holdCosts = holdingCost * sdp_max(inventoryLevel, 0);
  double cashBalanceBeforeRevenue = cash - fixedCost - variableCost - holdCosts - c.params[12 + c.period - 1];
  double interest = interestRate * sdp_max(-cashBalanceBeforeRevenue, 0);
  double deposite = depositeRate * sdp_max(cashBalanceBeforeRevenue, 0);
  double cashBalanceAfter = cashBalanceBeforeRevenue - interest + deposite + revenue;
  double cashIncrement = cashBalanceAfter - cash;
  double salValue = c.period == c.T ? salvageValue * sdp_max(inventoryLevel, 0) : 0;
  cashIncrement += salValue;
  imm = cashIncrement;
  double nextInventory = sdp_max(0, inventoryLevel);
  double nextCash = cash + cashIncrement;
  nextCash = nextCash > c.params[11] ? c.params[11] : nextCash;
  nextCash = nextCash < c.params[10] ? c.params[10] : nextCash;
  nextInventory = nextInventory > c.params[9] ? c.params[9] : nextInventory;
  nextInventory = nextInventory < c.params[8] ? c.params[8] : nextInventory;
  nextCash = sdp_trunc(sdp_round(nextCash * 10) / 10);
  nx = nextInventory;
  ncash = nextCash;
  npreq = 0;
}
__device__ double sdp_immediate(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand) {
  double imm, nx, nc, nq;
  sdp_cell(c, x, cash, preq, action, randomDemand, imm, nx, nc, nq);
  return imm;
}
__device__ void sdp_transition(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand,
                               double& nx, double& ncash, double& npreq) {
  double imm;
  sdp_cell(c, x, cash, preq, action, randomDemand, imm, nx, ncash, npreq);
}
"""

# a transition that forgets to clamp: leaves the grid
BROKEN_TRANSITION = BACKORDER.replace("nextInventory = nextInventory < c.params[4] ? c.params[4] : nextInventory;", "")


# the same two texts with the long division `Math.round(nextCash * 10) / 10` written through the prelude's integer helper
# (sdp_ldiv: truncating integer division, a few integer instructions with a literal divisor) instead of an fp64 division
OVERDRAFT_LIMIT_LDIV = OVERDRAFT_LIMIT.replace("sdp_trunc(sdp_round(nextCash * 10) / 10)", "sdp_ldiv(sdp_round(nextCash * 10), 10)")
OVERDRAFT_LIMIT_FUSED_LDIV = OVERDRAFT_LIMIT_FUSED.replace("sdp_trunc(sdp_round(nextCash * 10) / 10)", "sdp_ldiv(sdp_round(nextCash * 10), 10)")
assert "sdp_ldiv" in OVERDRAFT_LIMIT_LDIV and "sdp_ldiv" in OVERDRAFT_LIMIT_FUSED_LDIV


# ---------------------------------------------------------------------------------------------------------------
# The built-in CASH families restated as user text, statement for statement after oracle/sdpref.c's n_actions / imm_value /
# transition (and the family notes of include/sdpgpu.h).  One parameter layout for the four texts (_params_common below);
# the cash quantiser's form -- `/ div` as long division, or `/ div` in doubles -- is chosen by params[13..15], because the
# host compile of the oracle has no -D of its own.
# ---------------------------------------------------------------------------------------------------------------
P_OVERHEAD = 22  # params[P_OVERHEAD + period - 1]: the period's overhead (as OVERDRAFT_LIMIT's params[12 + ...])

_CASH_HELPERS = r"""
// round_cash (Math.round(nextCash * mult) / div): params[15] != 0 is Java's `long / int`, else `/ (double)`
__device__ inline double sdp_user_round_cash(const sdp_ctx& c, double nextCash) {
  double r = sdp_round(nextCash * c.params[13]);
  if (c.params[15] != 0) return sdp_ldiv(r, (int)c.params[14]);
  return r / c.params[14];
}
// the piecewise interest of CashOverdraft.java:87-95 == SingleProductLeadtime.java:88-96
__device__ inline double sdp_user_interest(const sdp_ctx& c, double cashBalanceBefore) {
  const double r0 = c.params[17], r2 = c.params[18], r3 = c.params[19], interestFree = c.params[20], limit = c.params[21];
  double interest = 0;
  if (cashBalanceBefore >= 0)
    interest = -r0 * cashBalanceBefore;
  else if (cashBalanceBefore >= -interestFree)
    interest = 0;
  else if (cashBalanceBefore >= -limit)
    interest = r2 * (-cashBalanceBefore - interestFree);
  else
    interest = r3 * (-cashBalanceBefore - limit) + r2 * (limit - interestFree);
  return interest;
}
"""

_IMM_CALL = "sdp_immediate(c, x, cash, preq, action, randomDemand)"
_IMM_RETURN = "return cashIncrement;"


def _three(count, imm, trans):
    """The three-function spelling: count / imm / trans are the bodies of the three lambdas."""
    assert imm.rstrip().endswith(_IMM_RETURN) and imm.count("return") == 1 and trans.count(_IMM_CALL) == 1
    return (_CASH_HELPERS
            + "__device__ int sdp_feasible_count(const sdp_ctx& c, double x, double cash, double preq) {" + count + "}\n"
            + "__device__ double sdp_immediate(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand) {"
            + imm + "}\n"
            + "__device__ void sdp_transition(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand,\n"
            + "                               double& nx, double& ncash, double& npreq) {" + trans + "}\n")


def _fused(count, imm, trans):
    """The SDP_USER_CELL spelling derived from the same bodies: sdp_cell runs the immediate value's statements once, the
    transition's statements read the increment off `imm` where the three-function text calls sdp_immediate again; sdp_immediate
    and sdp_transition are calls of sdp_cell (as in OVERDRAFT_LIMIT_FUSED)."""
    assert imm.rstrip().endswith(_IMM_RETURN) and imm.count("return") == 1 and trans.count(_IMM_CALL) == 1
    return ("#define SDP_USER_CELL 1\n" + _CASH_HELPERS
            + "__device__ int sdp_feasible_count(const sdp_ctx& c, double x, double cash, double preq) {" + count + "}\n"
            + "__device__ void sdp_cell(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand,\n"
            + "                         double& imm, double& nx, double& ncash, double& npreq) {"
            + imm.replace(_IMM_RETURN, "imm = cashIncrement;") + trans.replace(_IMM_CALL, "imm") + "}\n"
            + r"""__device__ double sdp_immediate(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand) {
  double imm, nx, nc, nq;
  sdp_cell(c, x, cash, preq, action, randomDemand, imm, nx, nc, nq);
  return imm;
}
__device__ void sdp_transition(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand,
                               double& nx, double& ncash, double& npreq) {
  double imm;
  sdp_cell(c, x, cash, preq, action, randomDemand, imm, nx, ncash, npreq);
}
""")


# the transition CashConstraint.java:122-133, cashSurvival.java:128-143 and CashOverdraft.java:107-118 share
_CASH_TRANS = r"""
  double nextInventory = sdp_max(0, x + action - randomDemand);
  double nextCash = cash + sdp_immediate(c, x, cash, preq, action, randomDemand);
  nextCash = nextCash > c.params[12] ? c.params[12] : nextCash;
  nextCash = nextCash < c.params[11] ? c.params[11] : nextCash;
  nextInventory = nextInventory > c.params[10] ? c.params[10] : nextInventory;
  nextInventory = nextInventory < c.params[9] ? c.params[9] : nextInventory;
  nextCash = sdp_user_round_cash(c, nextCash);
  nx = nextInventory;
  ncash = nextCash;
  npreq = 0;
"""

# F3: CashConstraint.java:95-133 (params[16] == 0) / CashConstraintTesting.java:110-148 (params[16] == 1)
_CASH = (r"""
  double maxQ = (double)(int)sdp_min(c.params[8], sdp_max(0.0, (cash - c.params[22 + c.period - 1] - c.params[1]) / c.params[2]));
  return (int)maxQ + 1;
""", r"""
  double revenue = c.params[0] * sdp_min(x + action, randomDemand);
  double fixedCost = action > 0 ? c.params[1] : 0;
  double variableCost = c.params[2] * action;
  double inventoryLevel = x + action - randomDemand;
  double holdCosts = c.params[3] * sdp_max(inventoryLevel, 0);
  double cashIncrement;
  if (c.params[16] == 0) {
    double deposite = (cash - fixedCost - variableCost) * (1 + c.params[4]);
    cashIncrement = (1 - c.params[5]) * revenue + deposite - holdCosts - c.params[22 + c.period - 1] - cash;
  } else {
    cashIncrement = revenue - fixedCost - variableCost - holdCosts - c.params[22 + c.period - 1];
  }
  double salValue = c.period == c.T ? c.params[6] * sdp_max(inventoryLevel, 0) : 0;
  cashIncrement += salValue;
  double endCash = cash + cashIncrement;
  if (endCash < 0) {
    cashIncrement += c.params[7] * endCash;
  }
  return cashIncrement;
""", _CASH_TRANS)

# F4: CashOverdraft.java:72-118
_OVERDRAFT = (r"""
  return (int)c.params[8] + 1;
""", r"""
  double revenue = c.params[0] * sdp_min(x + action, randomDemand);
  double fixedCost = action > 0 ? c.params[1] : 0;
  double variableCost = c.params[2] * action;
  double inventoryLevel = x + action - randomDemand;
  double cashBalanceBefore = cash - fixedCost - variableCost - c.params[22 + c.period - 1];
  double interest = sdp_user_interest(c, cashBalanceBefore);
  double cashBalanceAfter = cashBalanceBefore - interest + revenue;
  double cashIncrement = cashBalanceAfter - cash;
  double salValue = c.period == c.T ? c.params[6] * sdp_max(inventoryLevel, 0) : 0;
  cashIncrement += salValue;
  return cashIncrement;
""", _CASH_TRANS)

# F5: SingleProductLeadtime.java:72-119; the state is (x, cash, preQ), the order becomes the next preQ
_CASH_LEADTIME = (r"""
  double maxQ = c.params[8];
  if (c.params[16] != 0 && c.period == c.T) maxQ = 0;
  return (int)maxQ + 1;
""", r"""
  double revenue = c.params[0] * sdp_min(x + preq, randomDemand);
  double variableCost = c.params[2] * action;
  double inventoryLevel = x + preq - randomDemand;
  double cashBalanceBefore = cash - variableCost - c.params[22 + c.period - 1];
  double interest = sdp_user_interest(c, cashBalanceBefore);
  double cashBalanceAfter = cashBalanceBefore - interest + revenue;
  double cashIncrement = cashBalanceAfter - cash;
  double salValue = c.period == c.T ? c.params[6] * sdp_max(inventoryLevel, 0) : 0;
  cashIncrement += salValue;
  return cashIncrement;
""", r"""
  double nextInventory = sdp_max(0, x + preq - randomDemand);
  double nextCash = cash + sdp_immediate(c, x, cash, preq, action, randomDemand);
  double nextPreQ = action;
  nextCash = nextCash > c.params[12] ? c.params[12] : nextCash;
  nextCash = nextCash < c.params[11] ? c.params[11] : nextCash;
  nextInventory = nextInventory > c.params[10] ? c.params[10] : nextInventory;
  nextInventory = nextInventory < c.params[9] ? c.params[9] : nextInventory;
  nextCash = sdp_user_round_cash(c, nextCash);
  nx = nextInventory;
  ncash = nextCash;
  npreq = nextPreQ;
""")

# F6: cashSurvival.java:98-143, the lambdas RiskRecursion.getSurvProb runs over
_SURVIVAL = (r"""
  double maxQ = sdp_min(cash / c.params[2], c.params[8]);
  maxQ = sdp_max(maxQ, 0);
  return (int)maxQ + 1;
""", r"""
  double revenue = c.params[0] * sdp_min(x + action, randomDemand);
  double fixedCost = action > 0 ? c.params[1] : 0;
  double variableCost = c.params[2] * action;
  double deposite = (cash - fixedCost - variableCost) * (1 + c.params[4]);
  double inventoryLevel = x + action - randomDemand;
  double holdCosts = c.params[3] * sdp_max(inventoryLevel, 0);
  double cashIncrement = revenue + deposite - holdCosts - c.params[22 + c.period - 1] - cash;
  double salValue = c.period == c.T ? c.params[6] * sdp_max(inventoryLevel, 0) : 0;
  cashIncrement += salValue;
  return cashIncrement;
""", _CASH_TRANS)

assert "params[22 + " in _CASH[1] and P_OVERHEAD == 22
CASH, CASH_FUSED = _three(*_CASH), _fused(*_CASH)
OVERDRAFT, OVERDRAFT_FUSED = _three(*_OVERDRAFT), _fused(*_OVERDRAFT)
CASH_LEADTIME, CASH_LEADTIME_FUSED = _three(*_CASH_LEADTIME), _fused(*_CASH_LEADTIME)
SURVIVAL, SURVIVAL_FUSED = _three(*_SURVIVAL), _fused(*_SURVIVAL)


def _params_common(f, overheads, selector=0.0):
    """{price, fixOrderCost, variCost, holdingCost, depositeRate, overheadRate, salvageValue, penaltyCost, maxOrderQuantity,
    minInventoryState, maxInventoryState, minCashState, maxCashState, cashRoundMult, cashRoundDiv, cashRoundIntDiv, selector,
    r0, r2, r3, interestFreeAmount, limit, overhead[0 .. T-1]}"""
    g = lambda name: float(getattr(f, name, 0.0) or 0.0)  # noqa: E731
    out = [g("price"), g("fixOrderCost"), g("variCost"), g("holdingCost"), g("depositeRate"), g("overheadRate"), g("salvageValue"),
           g("penaltyCost"), g("maxOrderQuantity"), g("minInventoryState"), g("maxInventoryState"), g("minCashState"),
           g("maxCashState"), g("cashRoundMult"), g("cashRoundDiv"), 1.0 if f.cashRoundIntDiv else 0.0, float(selector),
           g("r0"), g("r2"), g("r3"), g("interestFreeAmount"), g("limit")]
    assert len(out) == P_OVERHEAD
    return out + [float(o) for o in overheads]


def _params_cash(functor, overheads):
    return _params_common(functor, overheads, functor.cashFormula)


def _params_overdraft(functor, overheads):
    return _params_common(functor, overheads)


def _params_cash_leadtime(functor, overheads):
    return _params_common(functor, overheads, 1.0 if functor.zeroOrderLastPeriod else 0.0)


def _params_survival(functor, overheads):
    return _params_common(functor, overheads)


def cash_text(w, fused=False):
    """(text, params) that restate the cash-family workload `w` (families 3-6) as user lambdas."""
    family = int(w.desc().family)
    text, fz, prm = {3: (CASH, CASH_FUSED, _params_cash), 4: (OVERDRAFT, OVERDRAFT_FUSED, _params_overdraft),
                     5: (CASH_LEADTIME, CASH_LEADTIME_FUSED, _params_cash_leadtime),
                     6: (SURVIVAL, SURVIVAL_FUSED, _params_survival)}[family]
    oh = w.overhead()
    if oh is None:
        oh = [w.functor.overheadCost] * w.T
    return (fz if fused else text), prm(w.functor, oh)


# the two inventory texts without their clamps: per-period grids grown from the initial state (P.cur != P.next, nothing baked)
def _unclamp(text):
    out = text
    for line in ("  nextInventory = nextInventory > c.params[5] ? c.params[5] : nextInventory;\n",
                 "  nextInventory = nextInventory < c.params[4] ? c.params[4] : nextInventory;\n"):
        assert out.count(line) == 1
        out = out.replace(line, "")
    return out


BACKORDER_UNCLAMPED = _unclamp(BACKORDER)
LEADTIME_UNCLAMPED = _unclamp(LEADTIME)


# BACKORDER with an immediate value that is NaN -- formed at run time from the arguments, 0.0 / 0.0 -- (a) for the order
# params[7] in every state, (b) for every order in the states params[8] <= x <= params[9], (c) in the one cell (state
# params[10], order params[11], demand params[12]); the transition is BACKORDER's, so every successor stays on the grid.
# params = BACKORDER's seven + those six
def _nan_text(text):
    tail = "  return totalCosts;\n"
    assert text.count(tail) == 1
    return text.replace(tail, r"""  double z = (x + action - randomDemand) - (x + action - randomDemand);
  double notANumber = z / z;
  bool a = action == c.params[7];
  bool b = x >= c.params[8] && x <= c.params[9];
  bool cell = x == c.params[10] && action == c.params[11] && randomDemand == c.params[12];
  return (a || b || cell) ? notANumber : totalCosts;
""")


BACKORDER_NAN = _nan_text(BACKORDER)
BACKORDER_NAN_UNCLAMPED = _nan_text(BACKORDER_UNCLAMPED)
