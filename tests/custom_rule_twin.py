"""The rule rollout of a user-functor handle (sdpgpu_custom_rule_simulate) in Python, written from DESIGN 4, "User-functor
rollouts".  The user's lambdas are the SAME text compiled for the host (oracle.sdpref.custom_functor: sdpref_user_imm /
sdpref_user_trans through ctypes); demands come from tests/sampler_twin.py.  Every decision is counted, so that a test can assert
that parity was reached on branches that were taken."""
import ctypes as C
from collections import Counter

import numpy as np

SS, SCS, SCS1S2 = 0, 1, 2


class _Ctx(C.Structure):
    _fields_ = [("period", C.c_int), ("T", C.c_int), ("step", C.c_double), ("params", C.POINTER(C.c_double))]


class Lambdas:
    """sdp_immediate / sdp_transition of a text, compiled for the host."""

    def __init__(self, text, params, T, step=1.0):
        from oracle import sdpref
        self.cf = sdpref.custom_functor(text, params)
        self.T, self.step = int(T), float(step)
        self.params = np.ascontiguousarray(params, dtype=np.float64)
        u = self.cf.user
        u.sdpref_user_imm.restype = C.c_double
        u.sdpref_user_imm.argtypes = [C.POINTER(_Ctx)] + [C.c_double] * 5
        u.sdpref_user_trans.restype = None
        u.sdpref_user_trans.argtypes = [C.POINTER(_Ctx)] + [C.c_double] * 5 + [C.POINTER(C.c_double)] * 3

    def _ctx(self, period):
        return _Ctx(period, self.T, self.step, self.params.ctypes.data_as(C.POINTER(C.c_double)))

    def imm(self, period, x, cash, q, d):
        return float(self.cf.user.sdpref_user_imm(C.byref(self._ctx(period)), x, cash, 0.0, q, d))

    def trans(self, period, x, cash, q, d):
        nx, nc, nq = C.c_double(), C.c_double(), C.c_double()
        self.cf.user.sdpref_user_trans(C.byref(self._ctx(period)), x, cash, 0.0, q, d, C.byref(nx), C.byref(nc), C.byref(nq))
        return nx.value, nc.value


def order(form, t, row, x, cash, ini_x, mcr, max_q, K, v, ev):
    """q of period index t under rule row (s, C, S, S2); one fp64 operation per statement."""
    s, Cc, S, S2 = (float(e) for e in row)
    if form == SCS1S2:
        if t == 0:
            return S - ini_x
        if not x < s:
            ev["no_order"] += 1
            return 0.0
        ev["S1" if cash <= Cc + 0.1 else "S2"] += 1
        return S - x if cash <= Cc + 0.1 else S2 - x
    if t == 0:
        return S if form == SS else S - s
    m = cash - mcr
    m = m - K
    m = m / v
    m = max(0.0, m)
    m = min(m, max_q)
    if not x < s:
        ev["no_order" if form == SS else "x_ge_s"] += 1
        return 0.0
    if form == SCS and not cash > Cc:
        ev["cash_le_C"] += 1
        return 0.0
    up = S - x
    ev["m_binds" if m < up else "up_to_S"] += 1
    return min(m, up)


def simulate(lam, demands, disc, ini_x, ini_cash, forms, rules, mcr=0.0, max_q=0.0, K=0.0, v=1.0, imm=None, trans=None, cash_box=None):
    """demands[n, T], disc[T], forms[R], rules[R, T, 4] -> {"sum": [R, n], "events": [Counter per rule]}.  imm / trans: other
    lambdas than the host compile's (the mirror's Python callables), (period, x, cash, q, d) -> float / (x, cash).  cash_box =
    (minCash, maxCash) counts the transitions whose balance the user's clamp moved."""
    imm = lam.imm if imm is None else imm
    trans = lam.trans if trans is None else trans
    rules = np.asarray(rules, dtype=np.float64)
    demands = np.asarray(demands, dtype=np.float64)
    R, (n, T) = len(forms), demands.shape
    assert rules.shape == (R, T, 4)
    sums = np.empty((R, n))
    traces = []
    for r, form in enumerate(int(e) for e in forms):
        ev = Counter()
        for p in range(n):
            x, cash, total = float(ini_x), float(ini_cash), 0.0
            for t in range(T):
                d = float(demands[p, t])
                q = order(form, t, rules[r, t], x, cash, float(ini_x), mcr, max_q, K, v, ev)
                inc = imm(t + 1, x, cash, q, d)
                total += float(disc[t]) * inc
                if t + 1 < T:
                    if cash_box is not None and not cash_box[0] <= cash + inc <= cash_box[1]:
                        ev["cash_clamp"] += 1
                    x, cash = trans(t + 1, x, cash, q, d)
                    if x != float(int(x)):
                        ev["fractional_inventory"] += 1
            sums[r, p] = total
        traces.append(ev)
    return {"sum": sums, "events": traces}


# what every form must have taken at least once for parity to mean something (tests/test_custom_sim_host.py)
BRANCHES = {SS: ("no_order", "m_binds", "up_to_S"), SCS: ("x_ge_s", "cash_le_C", "m_binds", "up_to_S"), SCS1S2: ("no_order", "S1", "S2")}


def coverage_gaps(forms, traces):
    """[(rule, branch)] never taken, plus the two global conditions."""
    gaps = [(r, b) for r, f in enumerate(int(e) for e in forms) for b in BRANCHES[f] if traces[r][b] == 0]
    total = Counter()
    for ev in traces:
        total.update(ev)
    return gaps + [(-1, b) for b in ("cash_clamp", "fractional_inventory") if total[b] == 0]
