"""Host twin of the level rule of sdpgpu_xr_simulate and of sdpgpu_xr_opt_levels, written from DESIGN 4 "(x, R) rollout" in plain
Python floats.  The rollout goes through CashXRFunctor.immediateValue / stateTransition -- the mirror of the reference's lambdas
(CashConstraintXR.java:78-110) -- exactly as CashSimulationXR.simulateAStar does (CashSimulationXR.java:158-167); it shares no
code with the kernel or with stochastic_inventory_amd.simulation.  RecursionG is the reference's two mutually recursive
functions over dict memos (RecursionG.java:96-153).

simulate() also returns a TRACE: how often each event of the definition occurred, per rule, over all paths and periods (the
reference's loop takes the transition in every period, the last one included):
    level        R > c a_t: the rule orders up to a_t
    capped       else: y = R / c
    below_stock  y < x (stock is sold back at cost)
    frac_y       y is not an integer
    frac_x       the next inventory is not an integer
    stockout     y < d
    cash_hi      the high cash clamp acts
    inv_hi       the inventory clamp acts
`before_last` holds the same counts over the periods whose transition the device takes (all but the last)."""
import math

import numpy as np

EVENTS = ("level", "capped", "below_stock", "frac_y", "frac_x", "stockout", "cash_hi", "inv_hi")


def simulate(functor, T, demands, disc, ini_x, ini_r, levels, vari_cost):
    """Path sums [R, n] of the rules levels[R, T] along demands[n, T] from (ini_x, ini_r), and the trace."""
    from stochastic_inventory_amd.states import CashStateXR
    f = functor
    levels = np.asarray(levels, dtype=np.float64)
    if levels.ndim == 1:
        levels = levels[None]
    n = len(demands)
    sums = np.empty((len(levels), n))
    events, before_last = [], []
    for r, row in enumerate(levels.tolist()):
        ev = dict.fromkeys(EVENTS, 0)
        ev2 = dict.fromkeys(EVENTS, 0)
        for p in range(n):
            total = 0.0
            state = CashStateXR(1, float(ini_x), float(ini_r), f.variCost)
            for t in range(T):
                d = float(demands[p][t])
                x, R = state.getIniInventory(), state.getIniR()
                seen = []
                if R > vari_cost * row[t]:
                    y = row[t]
                    seen.append("level")
                else:
                    y = R / vari_cost
                    seen.append("capped")
                if y < x:
                    seen.append("below_stock")
                if y != math.floor(y):
                    seen.append("frac_y")
                if y < d:
                    seen.append("stockout")
                imm = f.immediateValue(state, y, d, T)
                total += float(disc[t]) * imm
                if (R - f.variCost * x) + imm > f.maxCashState:
                    seen.append("cash_hi")
                if max(0.0, y - d) > f.maxInventoryState:
                    seen.append("inv_hi")
                state = f.stateTransition(state, y, d, T)
                if state.getIniInventory() != math.floor(state.getIniInventory()):
                    seen.append("frac_x")
                for e in seen:
                    ev[e] += 1
                    if t < T - 1:
                        ev2[e] += 1
            sums[r, p] = total
        events.append(ev)
        before_last.append(ev2)
    return {"sum": sums, "events": events, "before_last": before_last}


class RecursionG:
    """RecursionG.java:28-153 over dict memos: pmf[t] rows of [demand, probability]."""

    def __init__(self, pmf, price, variCost, depositeRate, salvageValue, maxY=200):
        self.pmf = [[(float(d), float(p)) for d, p in tile] for tile in pmf]
        self.T = len(self.pmf)
        self.price, self.variCost, self.depositeRate, self.salvageValue = float(price), float(variCost), float(depositeRate), float(salvageValue)
        self.maxY = maxY
        self.cacheGValues, self.cachePeriodBestY = {}, {}

    def G(self, n, y):
        key = (n, y)
        if key in self.cacheGValues:
            return self.cacheGValues[key]
        price, variCost, depositeRate, salvageValue, T = self.price, self.variCost, self.depositeRate, self.salvageValue, self.T
        dAndP = self.pmf[n - 1]
        expectValue = 0.0
        if n == T:
            for d, p in dAndP:
                thisDValue = (price - variCost) * min(d, y) - depositeRate * variCost * y + (salvageValue - variCost) * max(y - d, 0.0)
                expectValue += p * thisDValue
        else:
            nextAStar = self.getAStar(n + 1)
            for d, p in dAndP:
                newY = max(nextAStar, max(y - d, 0.0))
                thisDValue = math.pow(1 + depositeRate, T - n) * ((price - variCost) * min(d, y) - depositeRate * variCost * y) + self.G(n + 1, newY)
                expectValue += p * thisDValue
        self.cacheGValues[key] = expectValue
        return expectValue

    def getAStar(self, n):
        if n in self.cachePeriodBestY:
            return self.cachePeriodBestY[n]
        optY, optYValue = 0.0, -1000.0
        y = 0.0
        while y < self.maxY:
            thisYValue = self.G(n, y)
            if thisYValue - optYValue > 0.01:
                optYValue, optY = thisYValue, y
            y = y + 1
        self.cachePeriodBestY[n] = optY
        return optY

    def getOptY(self):
        out = [0.0] * self.T
        for t in range(self.T - 1, -1, -1):
            out[t] = self.getAStar(t + 1)
        return out
