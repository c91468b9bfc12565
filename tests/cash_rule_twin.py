"""Host twin of the cash rule rollout (sdpgpu_cash_rule_simulate), written from its DEFINITION in DESIGN.md section 4 ("Cash rule
rollout"): plain Python floats (IEEE fp64, one operation per statement, no FMA), the period's cash increment and the next state
through functors.CashFunctor.immediateValue / stateTransition.  It shares no code with the kernel, nor with the helpers of
stochastic_inventory_amd.simulation.  Besides the path sums it returns a TRACE: how often each branch of the definition was taken,
which the host tests turn into a coverage condition on the rules the GPU test uses."""
import math
from collections import Counter

import numpy as np

from stochastic_inventory_amd.states import CashState

SC12S, SC1S, SMEANCS = 0, 1, 2
EVENTS = ("capped_by_cash", "up_to_S", "x_ge_s", "cash_le_c1", "cash_ge_c2", "table_hit", "table_miss", "fractional_inventory")
# the events a form can show: only form 0 has a C2, form 2 reads no table
EVENTS_OF_FORM = {
    SC12S: EVENTS,
    SC1S: tuple(e for e in EVENTS if e != "cash_ge_c2"),
    SMEANCS: tuple(e for e in EVENTS if e not in ("cash_ge_c2", "table_hit", "table_miss")),
}


def java_int(v):
    """(int) of a double: toward zero, saturating, NaN -> 0."""
    if v != v:
        return 0
    if v >= 2147483647.0:
        return 2147483647
    if v <= -2147483648.0:
        return -2147483648
    return int(v)


class Problem:
    """What the definition reads of a case: the functor's lambdas, the horizon, the descriptor's inventory grid."""

    def __init__(self, functor, T):
        self.f, self.T = functor, T
        self.x_lo, self.step = float(functor.minInventoryState), float(functor.stepSize)
        self.nx = int((functor.maxInventoryState - functor.minInventoryState) / functor.stepSize) + 1

    def key(self, ix):
        return self.x_lo + ix * self.step

    def index_of(self, x):
        """ix with key(ix) == x as doubles, or None."""
        i = float(np.rint((x - self.x_lo) * (1.0 / self.step)))
        if not (0.0 <= i < self.nx):
            return None
        i = int(i)
        return i if self.key(i) == x else None


def lookup(P, tab, r, t, x, events):
    """The entry of tab[r, t] at x, or None: a NULL table, x off the grid, or a NaN entry."""
    ix = None if tab is None else P.index_of(x)
    if ix is None or math.isnan(tab[r, t, ix]):
        events["table_miss"] += 1
        return None
    events["table_hit"] += 1
    return float(tab[r, t, ix])


def order(P, form, t, row, c1_tab, c2_tab, r, x, cash, mcr, max_q, K, v, events):
    s, c1, c2, S = (float(e) for e in row)
    if t == 0:
        q = S - x if x < s else 0.0
        if not x < s:
            events["x_ge_s"] += 1
        if form == SC1S:
            m0 = max(0.0, (cash - mcr - K) / v)
            if x < s:
                events["capped_by_cash" if m0 < q else "up_to_S"] += 1
            q = min(q, m0)
        elif x < s:
            events["up_to_S"] += 1
        return q
    m = max(0.0, (cash - mcr - K) / v)
    if form == SC12S:
        m = float(java_int(m))
    m = min(m, max_q)
    if not x < s:
        events["x_ge_s"] += 1
        return 0.0
    if form in (SC12S, SC1S):
        hit = lookup(P, c1_tab, r, t, x, events)
        c1 = 0.0 if hit is None else hit
    if form == SC12S:
        hit = lookup(P, c2_tab, r, t, x, events)
        c2 = 10000.0 if hit is None else hit
    if not cash > c1:
        events["cash_le_c1"] += 1
        return 0.0
    if form == SC12S and not cash < c2:
        events["cash_ge_c2"] += 1
        return 0.0
    events["capped_by_cash" if m < S - x else "up_to_S"] += 1
    return min(m, S - x)


def simulate(P, demands, disc, ini_x, ini_cash, forms, rules, c1_tab, c2_tab, mcr, max_q, K, v):
    """demands[n, T], disc[T]; forms[R]; rules[R, T, 4]; c1_tab / c2_tab None or [R, T, NX].  Returns {"sum": [R, n], "events":
    [Counter per rule]}."""
    f, T = P.f, P.T
    rules = np.asarray(rules, dtype=np.float64)
    R, n = len(forms), len(demands)
    assert rules.shape == (R, T, 4) and np.asarray(demands).shape == (n, T)
    for tab in (c1_tab, c2_tab):
        assert tab is None or np.asarray(tab).shape == (R, T, P.nx)
    sums = np.empty((R, n))
    traces = []
    for r, form in enumerate(int(e) for e in forms):
        ev = Counter()
        for p in range(n):
            state, total = CashState(1, float(ini_x), float(ini_cash)), 0.0
            for t in range(T):
                d = float(demands[p][t])
                q = order(P, form, t, rules[r, t], c1_tab, c2_tab, r, state.getIniInventory(), state.getIniCash(), mcr, max_q, K, v, ev)
                total += float(disc[t]) * f.immediateValue(state, q, d, T)
                state = f.stateTransition(state, q, d, T)
                if t + 1 < T and P.index_of(state.getIniInventory()) is None:
                    ev["fractional_inventory"] += 1
            sums[r, p] = total
        traces.append(ev)
    return {"sum": sums, "events": traces}


def pack(P, cache):
    """{(period, x): value}, period 1-based -> dense [T, NX], NaN where absent; a key off the grid is dropped."""
    tab = np.full((P.T, P.nx), np.nan)
    for (period, x), val in cache.items():
        ix = P.index_of(float(x))
        if ix is not None and 1 <= period <= P.T:
            tab[period - 1, ix] = val
    return tab
