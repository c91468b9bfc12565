"""CashOverdraftTesting's lambdas (CashOverdraftTesting.java:78-120) as user-functor text, in the reference's three-function
form and with the fused per-cell callback, and the small instance the user-functor rollout tests run them on.

params = [price, fixOrderCost, variCost, holdingCost, interestRate, maxOrderQuantity, minCashRequired, minInventoryState,
maxInventoryState, minCashState, maxCashState].  `Math.round(nextCash * 10) / 10.0` (:117) is a DOUBLE division here (the
descriptor's cash quantiser with cashRoundIntDiv False), unlike CashOverdraft.main's `/ 10`."""
import numpy as np

import cases

_COUNT = r"""
__device__ int sdp_feasible_count(const sdp_ctx& c, double x, double cash, double preq) {
  double maxQ = sdp_trunc(sdp_min(c.params[5], sdp_max(0, (cash - c.params[6] - c.params[1]) / c.params[2])));
  return (int)maxQ + 1;
}
"""

OVERDRAFT_TESTING = _COUNT + r"""
__device__ double sdp_immediate(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand) {
  const double price = c.params[0], fixOrderCost = c.params[1], variCost = c.params[2], holdingCost = c.params[3];
  const double interestRate = c.params[4];
  double revenue = price * sdp_min(x + action, randomDemand);
  double fixedCost = action > 0 ? fixOrderCost : 0;
  double variableCost = variCost * action;
  double inventoryLevel = x + action - randomDemand;
  double holdCosts = holdingCost * sdp_max(inventoryLevel, 0);
  double cashBalanceBefore = cash + revenue - fixedCost - variableCost - holdCosts;
  double interest = interestRate * sdp_max(-cashBalanceBefore, 0);
  double cashBalanceAfter = cashBalanceBefore - interest;
  double cashIncrement = cashBalanceAfter - cash;
  return cashIncrement;
}
__device__ void sdp_transition(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand,
                               double& nx, double& ncash, double& npreq) {
  const double price = c.params[0], fixOrderCost = c.params[1], variCost = c.params[2], holdingCost = c.params[3];
  const double interestRate = c.params[4];
  double nextInventory = sdp_max(0, x + action - randomDemand);
  double revenue = price * sdp_min(x + action, randomDemand);
  double fixedCost = action > 0 ? fixOrderCost : 0;
  double variableCost = variCost * action;
  double holdCosts = holdingCost * sdp_max(nextInventory, 0);
  double nextCash = cash + revenue - fixedCost - variableCost - holdCosts;
  nextCash = nextCash - sdp_max(-nextCash, 0) * interestRate;
  nextCash = nextCash > c.params[10] ? c.params[10] : nextCash;
  nextCash = nextCash < c.params[9] ? c.params[9] : nextCash;
  nextInventory = nextInventory > c.params[8] ? c.params[8] : nextInventory;
  nextInventory = nextInventory < c.params[7] ? c.params[7] : nextInventory;
  nextCash = sdp_round(nextCash * 10) / 10.0;
  nx = nextInventory;
  ncash = nextCash;
  npreq = 0;
}
"""

# the same statements once per cell: the balance before interest is what both lambdas form (the holding cost of max(level, 0)
# and of max(max(0, level), 0) is the same double)
OVERDRAFT_TESTING_FUSED = "#define SDP_USER_CELL 1\n" + _COUNT + r"""
__device__ void sdp_cell(const sdp_ctx& c, double x, double cash, double preq, double action, double randomDemand,
                         double& imm, double& nx, double& ncash, double& npreq) {
  const double price = c.params[0], fixOrderCost = c.params[1], variCost = c.params[2], holdingCost = c.params[3];
  const double interestRate = c.params[4];
  double revenue = price * sdp_min(x + action, randomDemand);
  double fixedCost = action > 0 ? fixOrderCost : 0;
  double variableCost = variCost * action;
  double inventoryLevel = x + action - randomDemand;
  double nextInventory = sdp_max(0, inventoryLevel);
  double holdCosts = holdingCost * sdp_max(inventoryLevel, 0);
  double cashBalanceBefore = cash + revenue - fixedCost - variableCost - holdCosts;
  double nextCash = cashBalanceBefore - interestRate * sdp_max(-cashBalanceBefore, 0);
  imm = nextCash - cash;
  nextCash = nextCash > c.params[10] ? c.params[10] : nextCash;
  nextCash = nextCash < c.params[9] ? c.params[9] : nextCash;
  nextInventory = nextInventory > c.params[8] ? c.params[8] : nextInventory;
  nextInventory = nextInventory < c.params[7] ? c.params[7] : nextInventory;
  nx = nextInventory;
  ncash = sdp_round(nextCash * 10) / 10.0;
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

# ---- the instance of the tests: 19 x 1601 states, T = 4 ------------------------------------------------------------------------
PRICE, FIX, VARI, HOLD, RATE, MAXQ = 5.0, 6.0, 2.0, 1.0, 0.1, 14.0
MIN_CASH_REQUIRED = -5.0
PARAMS = [PRICE, FIX, VARI, HOLD, RATE, MAXQ, MIN_CASH_REQUIRED, 0.0, 18.0, -40.0, 120.0]
T = 4
INI = (0.0, 10.0)
SCALARS = dict(min_cash_required=MIN_CASH_REQUIRED, max_q=MAXQ, fix_order_cost=FIX, vari_cost=VARI)


def pmf():
    return cases._pmf([4, 6, 3, 5], 10)


def shape(sia):
    """The state shape and grid of the handle: (x, cash), cash in tenths by a double division."""
    return sia.OverdraftFunctor(price=PRICE, fixOrderCost=FIX, variCost=VARI, maxOrderQuantity=MAXQ, minInventoryState=0,
                                maxInventoryState=18, minCashState=-40, maxCashState=120, cashRoundMult=10.0, cashRoundDiv=10.0,
                                cashRoundIntDiv=False, iniInventory=INI[0], iniCash=INI[1])


def desc(sia, gamma=0.95):
    d = shape(sia).to_desc(T, sia.OptDirection.MAX)
    d.discount_factor = gamma
    return d


# rule rows (s, C, S, S2) of the three forms, the same in every period; rules 3 and 4 of the mixed call shift them
ROWS = ((5.0, 0.0, 12.0, 0.0), (6.0, -10.0, 13.0, 0.0), (5.0, 20.0, 9.0, 14.0))
MIXED_FORMS = (0, 1, 2, 0, 1)


def rules(which=(0, 1, 2)):
    """(forms, rows[R, T, 4]) of the rules with the given indices into MIXED_FORMS."""
    rows = []
    for r in which:
        row = np.array(ROWS[MIXED_FORMS[r]], dtype=np.float64)
        if r >= 3:
            row = row + np.array([1.5, 4.25, 2.75, 0.0])
        rows.append(np.tile(row, (T, 1)))
    return np.array([MIXED_FORMS[r] for r in which], dtype=np.int32), np.stack(rows)
