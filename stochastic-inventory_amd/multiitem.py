"""Two-product lead-time family on the reachable-set engine (sdpgpu_multilead_solve).

Host mirror of `sdp.cash.multiItem.CashRecursionMultiLead` as `cash.overdraft.MultiProductLeadtime.main`
uses it (src/cash/overdraft/MultiProductLeadtime.java:87-239): the lambdas there are fixed in form, so the
mirror takes their parameters, not closures.  This is the only family the reference records outputs
for (the comment block at MultiProductLeadtime.java:30-50).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List

from . import _abi
import numpy as np

from ._abi import SdpgpuError, SdpgpuMulticash, SdpgpuMultilead


@dataclass
class MultiLeadResult:
    finalValue: float          # iniCash + getExpectedValue(iniState)
    firstAction: int           # getAction(iniState).getFirstAction()
    secondAction: int
    statesPerPeriod: List[int]
    cells: int
    gpu_ms: float
    # rows {period, i1, i2, q1, q2, cash (R for the XR family), value, action 1, action 2} of every visited state in the
    # order of the reference's TreeMap keys -- what getCacheActions() / getOptTable() iterate; None unless asked for
    table: object = None
    # SDPGPU_MULTI_FORM_* bits (_abi.MULTI_FORMS) of the kernel forms the solve launched (sdpgpu_multi_forms_used)
    forms: int = 0


def fill_multilead(k, *, T, q_bound, price, vari_cost, sal_value, ini_cash, ini_i1, ini_i2, r0, r1, r2, limit,
                   interest_free, min_inventory, max_inventory, min_cash, max_cash, discount, overhead, values, probs,
                   cash_int_cast=False):
    k.T, k.q_bound = T, q_bound
    k.cash_int_cast = 1 if cash_int_cast else 0
    for name, val in (("price", price), ("vari_cost", vari_cost), ("sal_value", sal_value)):
        getattr(k, name)[0], getattr(k, name)[1] = val
    for name, val in (("ini_cash", ini_cash), ("ini_i1", ini_i1), ("ini_i2", ini_i2), ("r0", r0), ("r1", r1), ("r2", r2),
                      ("limit", limit), ("interest_free", interest_free), ("min_inventory", min_inventory),
                      ("max_inventory", max_inventory), ("min_cash", min_cash), ("max_cash", max_cash),
                      ("discount", discount)):
        setattr(k, name, float(val))
    for t, v in enumerate(overhead):
        k.overhead[t] = float(v)
    k.n1, k.n2 = len(values[0]), len(values[1])
    for i, (v, p) in enumerate(zip(values[0], probs[0])):
        k.v1[i], k.p1[i] = float(v), float(p)
    for i, (v, p) in enumerate(zip(values[1], probs[1])):
        k.v2[i], k.p2[i] = float(v), float(p)
    return k


def _run(call, T: int, want_table: bool) -> MultiLeadResult:
    """call(fv, q1, q2, states, cells, ms) -> rc.  With want_table the solve is run a second time with a table large
    enough for every visited state (the first run says how many there are)."""
    lib = _abi.load()

    def once():
        fv, q1, q2 = C.c_double(), C.c_int32(), C.c_int32()
        states = (C.c_int64 * T)()
        cells, ms = C.c_int64(), C.c_double()
        rc = call(C.byref(fv), C.byref(q1), C.byref(q2), states, C.byref(cells), C.byref(ms))
        if rc:
            raise SdpgpuError(rc, lib.sdpgpu_multilead_last_error().decode())
        return MultiLeadResult(fv.value, q1.value, q2.value, list(states), cells.value, ms.value,
                               forms=int(lib.sdpgpu_multi_forms_used()))

    res = once()
    if want_table:
        t, arrs = _abi.make_multi_table(sum(res.statesPerPeriod))
        lib.sdpgpu_multi_set_table(C.byref(t))
        try:
            res = once()
        finally:
            lib.sdpgpu_multi_set_table(None)
        res.table = _abi.multi_table_rows(t, arrs)
    return res


def multilead_solve(table: bool = False, **kw) -> MultiLeadResult:
    """One call = `recursion.getExpectedValue(iniState)` + `getAction(iniState)` of MultiProductLeadtime.main;
    table=True also returns the whole memo (see MultiLeadResult.table)."""
    lib = _abi.load()
    k = fill_multilead(SdpgpuMultilead(), **kw)
    return _run(lambda *out: lib.sdpgpu_multilead_solve(C.byref(k), *out), k.T, table)


def fill_multicash(k, *, T, q_bound, price, vari_cost, sal_price, ini_cash, ini_i1, ini_i2, min_inventory, max_inventory,
                   min_cash, max_cash, discount, pmf):
    """pmf[t] = rows {d1, d2, probability}: what GetPmfMulti.getPmf(t) returns (GetPmfMulti.java:41-69).  The
    arrays the struct points to are kept alive on `k._keep`."""
    k.T, k.q_bound = T, q_bound
    for name, val in (("price", price), ("vari_cost", vari_cost), ("sal_price", sal_price)):
        getattr(k, name)[0], getattr(k, name)[1] = val
    for name, val in (("ini_cash", ini_cash), ("ini_i1", ini_i1), ("ini_i2", ini_i2), ("min_inventory", min_inventory),
                      ("max_inventory", max_inventory), ("min_cash", min_cash), ("max_cash", max_cash),
                      ("discount", discount)):
        setattr(k, name, float(val))
    if len(pmf) != T:
        raise ValueError(f"pmf has {len(pmf)} periods, T = {T}")
    tiles = [np.asarray(t, dtype=np.float64).reshape(-1, 3) for t in pmf]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tiles])]).astype(np.int32)
    allp = np.concatenate(tiles, axis=0)
    d1, d2, p = (np.ascontiguousarray(allp[:, c]) for c in range(3))
    k._keep = (off, d1, d2, p)
    k.pmf_off = off.ctypes.data_as(C.POINTER(C.c_int32))
    k.d1, k.d2, k.p = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in (d1, d2, p))
    return k


def multicash_solve(table: bool = False, **kw) -> MultiLeadResult:
    """`sdp.cash.multiItem.CashRecursionMulti` as `cash.multiItem.MultiItemCash.main` sets it up
    (MultiItemCash.java:66-132; the lambdas are fixed in form, so the mirror takes their parameters):
    one call = `iniCash + recursion.getExpectedValue(iniState)` + `getAction(iniState)`; table=True also returns the
    rows `getOptTable` is built from."""
    lib = _abi.load()
    k = fill_multicash(SdpgpuMulticash(), **kw)
    return _run(lambda *out: lib.sdpgpu_multicash_solve(C.byref(k), *out), k.T, table)


def multixr_solve(depositeRate: float = 0.0, table: bool = False, **kw) -> MultiLeadResult:
    """`sdp.cash.multiItem.CashRecursionMultiXR` as `cash.multiItem.MultiItemCashXR.main` sets it up
    (MultiItemCashXR.java:92-164): state (x1, x2, R), actions = order-up-to levels; `ini_cash` is the R of the period-1
    state.  firstAction / secondAction of the result are y1 / y2 (`recursion.getAction(iniState)[0]`, `[1]`)."""
    lib = _abi.load()
    k = fill_multicash(SdpgpuMulticash(), **kw)
    return _run(lambda *out: lib.sdpgpu_multixr_solve(C.byref(k), C.c_double(depositeRate), *out), k.T, table)


# ---------------------------------------------------------------------------------------------------------------
# The computed policy on the device: a hash table over the memo's states and its rollouts (sdpgpu_multi_policy_*;
# DESIGN 4, "Two-product rollout").
# ---------------------------------------------------------------------------------------------------------------
def _sample_mode(mode):
    if mode in ("lhs", _abi.SAMPLE_LHS):
        return _abi.SAMPLE_LHS
    if mode in ("random", _abi.SAMPLE_RANDOM):
        return _abi.SAMPLE_RANDOM
    raise ValueError(f"mode {mode!r}: 'lhs' or 'random'")


def _u64(v):
    return C.c_uint64(int(v) & (2**64 - 1))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def table_from_rows(rows):
    """A sdpgpu_multi_table over memo rows {period, i1, i2, q1, q2, cash or R, value, a1, a2} (MultiLeadResult.table, or the
    oracle's memo): -> (struct, the arrays it points to)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    t, arrs = _abi.make_multi_table(len(rows))
    for c, name in enumerate(("period", "i1", "i2", "q1", "q2", "cash", "value", "a1", "a2")):
        arrs[name][:] = rows[:, c]
    t.rows = len(rows)
    return t, arrs


class MultiPolicy:
    """The policy a two-product solve computed, on the device: `kind` is "multilead", "multicash" or "multixr", `rows` the
    memo of a solve of the SAME keyword arguments (MultiLeadResult.table), `kw` those arguments.  lookup = getAction for many
    states; simulate / simulate_sampled roll the policy along demand pairs from the period-1 state as CashSimulationMulti /
    CashSimulationMultiXR do; sample returns what simulate_sampled draws.  close() releases the device memory."""

    def __init__(self, kind: str, rows, capacity_log2: int = 0, depositeRate: float = 0.0, **kw):
        self._lib = _abi.load()
        self._h = C.c_void_p()
        self.kind = kind
        t, arrs = table_from_rows(rows)
        if kind == "multilead":
            k = fill_multilead(SdpgpuMultilead(), **kw)
            rc = self._lib.sdpgpu_multilead_policy_create(C.byref(k), C.byref(t), int(capacity_log2), C.byref(self._h))
        elif kind in ("multicash", "multixr"):
            k = fill_multicash(SdpgpuMulticash(), **kw)
            rc = self._lib.sdpgpu_multicash_policy_create(C.byref(k), 1 if kind == "multixr" else 0, float(depositeRate), C.byref(t),
                                                          int(capacity_log2), C.byref(self._h))
        else:
            raise ValueError(f"kind {kind!r}: 'multilead', 'multicash' or 'multixr'")
        self._check(rc)
        self.T = int(k.T)
        self.rows = int(t.rows)

    def _check(self, rc):
        if rc:
            raise SdpgpuError(rc, self._lib.sdpgpu_multilead_last_error().decode())

    def close(self):
        if self._h:
            self._lib.sdpgpu_multi_policy_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lookup(self, period, i1, i2, q1, q2, cash):
        """getAction of n states: (a1[n], a2[n], found[n]); found is False where the memo holds no such state."""
        per = np.ascontiguousarray(period, dtype=np.int32)
        cols = [np.ascontiguousarray(c, dtype=np.float64) for c in (i1, i2, q1, q2, cash)]
        n = len(per)
        if any(c.shape != (n,) for c in cols):
            raise ValueError("period, i1, i2, q1, q2 and cash must have one entry per state")
        a1, a2 = np.zeros(n, np.int32), np.zeros(n, np.int32)
        found = np.zeros(n, np.uint8)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.sdpgpu_multi_policy_lookup(self._h, n, ip(per), *(_dp(c) for c in cols), ip(a1), ip(a2),
                                                         found.ctypes.data_as(C.POINTER(C.c_uint8))))
        return a1, a2, found.astype(bool)

    def _disc(self, discount):
        if discount is None:
            return None
        disc = np.ascontiguousarray(discount, dtype=np.float64)
        if disc.shape != (self.T,):
            raise ValueError("discount must have one entry per period")
        return disc

    def simulate(self, d1, d2, discount=None):
        """Roll the policy along the demand pairs d1 / d2 [n, T] (as the caller rounded them): -> (SdpgpuSimResult, sums[n],
        valid[n]).  A path whose look-up misses ends there: its sum is NaN, and mean and m2 of the result are NaN then."""
        d1 = np.ascontiguousarray(d1, dtype=np.float64)
        d2 = np.ascontiguousarray(d2, dtype=np.float64)
        if d1.ndim != 2 or d1.shape[1] != self.T or d2.shape != d1.shape:
            raise ValueError(f"d1 and d2 must both have shape (n_paths, {self.T})")
        disc = self._disc(discount)
        n = len(d1)
        res = _abi.SdpgpuSimResult()
        sums, valid = np.empty(n), np.zeros(n, np.uint8)
        self._check(self._lib.sdpgpu_multi_policy_simulate(self._h, n, _dp(d1), _dp(d2), None if disc is None else _dp(disc), C.byref(res),
                                                           _dp(sums), valid.ctypes.data_as(C.POINTER(C.c_uint8))))
        return res, sums, valid

    def simulate_sampled(self, n_paths: int, seed: int, *, mode="lhs", first_path: int = 0, discount=None, want_sums: bool = False):
        """Draw n_paths paths of demand pairs on the device (a row of each period's joint tile per uniform), roll and reduce
        there: -> SdpgpuSimResult; with want_sums also (sums[n], valid[n])."""
        disc = self._disc(discount)
        n = int(n_paths)
        res = _abi.SdpgpuSimResult()
        sums = np.empty(max(n, 0)) if want_sums else None
        valid = np.zeros(max(n, 0), np.uint8) if want_sums else None
        self._check(self._lib.sdpgpu_multi_policy_simulate_sampled(
            self._h, n, _u64(seed), _sample_mode(mode), _u64(first_path), None if disc is None else _dp(disc), C.byref(res),
            None if sums is None else _dp(sums), None if valid is None else valid.ctypes.data_as(C.POINTER(C.c_uint8))))
        return (res, sums, valid) if want_sums else res

    def sample(self, n_paths: int, seed: int, *, mode="lhs", first_path: int = 0):
        """(d1[n, T], d2[n, T], u[n, T]): exactly what simulate_sampled draws."""
        n = max(int(n_paths), 0)
        d1, d2, u = (np.empty((n, self.T)) for _ in range(3))
        self._check(self._lib.sdpgpu_multi_policy_sample(self._h, int(n_paths), _u64(seed), _sample_mode(mode), _u64(first_path), _dp(d1),
                                                         _dp(d2), _dp(u)))
        return d1, d2, u


# ---------------------------------------------------------------------------------------------------------------
# Mirror classes: the reference's names and methods over the solvers above.  As elsewhere the lambdas are accepted
# and kept for the caller's own use (simulators), and a functor -- here simply the keyword arguments of the solver --
# names the closed-form family the device evaluates.  The first getExpectedValue runs the solve and reads the whole
# memo back, so every state the reference's recursion would have visited can be asked for afterwards.
# ---------------------------------------------------------------------------------------------------------------
class Actions:
    """sdp.cash.multiItem.Actions (Actions.java:17-33)."""

    def __init__(self, action1: int, action2: int):
        self.action1, self.action2 = int(action1), int(action2)

    def getFirstAction(self) -> int:
        return self.action1

    def getSecondAction(self) -> int:
        return self.action2

    def __eq__(self, o):
        return isinstance(o, Actions) and (o.action1, o.action2) == (self.action1, self.action2)

    def __repr__(self):
        return f"Actions({self.action1}, {self.action2})"


class CashStateMulti:
    """sdp.cash.multiItem.CashStateMulti (CashStateMulti.java:14-70)."""

    def __init__(self, period: int, iniInventory1: float, iniInventory2: float, iniCash: float):
        self.period, self.iniInventory1, self.iniInventory2, self.iniCash = int(period), float(iniInventory1), float(iniInventory2), float(iniCash)

    def getPeriod(self): return self.period
    def getIniInventory1(self): return self.iniInventory1
    def getIniInventory2(self): return self.iniInventory2
    def getIniCash(self): return self.iniCash

    def getIniR(self, variCosts):
        return self.iniCash + variCosts[0] * self.iniInventory1 + variCosts[1] * self.iniInventory2

    def _key(self): return (self.period, self.iniInventory1, self.iniInventory2, 0.0, 0.0, self.iniCash)


class CashStateMultiXR:
    """sdp.cash.multiItem.CashStateMultiXR (CashStateMultiXR.java:21-73): (period, x1, x2, R)."""

    def __init__(self, period: int, iniInventory1: float, iniInventory2: float, R: float):
        self.period, self.iniInventory1, self.iniInventory2, self.iniR = int(period), float(iniInventory1), float(iniInventory2), float(R)

    def getPeriod(self): return self.period
    def getIniInventory1(self): return self.iniInventory1
    def getIniInventory2(self): return self.iniInventory2
    def getIniR(self): return self.iniR
    def _key(self): return (self.period, self.iniInventory1, self.iniInventory2, 0.0, 0.0, self.iniR)


class CashStateMultiLead:
    """sdp.cash.multiItem.CashStateMultiLead (CashStateMultiLead.java:10-80)."""

    def __init__(self, period: int, iniInventory1: float, iniInventory2: float, preQ1: float, preQ2: float, iniCash: float):
        self.period = int(period)
        self.iniInventory1, self.iniInventory2 = float(iniInventory1), float(iniInventory2)
        self.preQ1, self.preQ2, self.iniCash = float(preQ1), float(preQ2), float(iniCash)

    def getPeriod(self): return self.period
    def getIniInventory1(self): return self.iniInventory1
    def getIniInventory2(self): return self.iniInventory2
    def getPreQ1(self): return self.preQ1
    def getPreQ2(self): return self.preQ2
    def getIniCash(self): return self.iniCash

    def getIniR(self, variCosts):
        return self.iniCash + variCosts[0] * self.iniInventory1 + variCosts[1] * self.iniInventory2

    def _key(self): return (self.period, self.iniInventory1, self.iniInventory2, self.preQ1, self.preQ2, self.iniCash)


class _MultiRecursionBase:
    _solver = None       # multilead_solve / multicash_solve / multixr_solve
    _state_type = None

    def __init__(self, discountFactor, Pmf, buildActionList=None, stateTransition=None, immediateValue=None,
                 TLength=None, *, functor=None):
        if functor is None:
            raise TypeError("functor: the parameters of the driver's lambdas (the keyword arguments of the solver)")
        self.discountFactor, self.Pmf, self.TLength = discountFactor, Pmf, TLength
        self.buildActionList, self.stateTransition, self.immediateValue = buildActionList, stateTransition, immediateValue
        self.functor = dict(functor)
        self.functor["discount"] = discountFactor
        if TLength is not None:
            self.functor["T"] = int(TLength)
        self._result = None
        self._memo = None

    def _solve(self, state):
        if self._result is None:
            f = self.functor
            ini = state._key()
            if ini[0] != 1:
                raise ValueError("the first getExpectedValue must be asked for a period-1 state (it fixes the reachable set)")
            self._result = self._run(f, ini)
            self._ini = ini
            t = self._result.table
            self._memo = {tuple(r[:6]): (float(r[6]), int(r[7]), int(r[8])) for r in t}
        return self._result

    def _lookup(self, state):
        self._solve(state)
        k = state._key()
        k = (float(k[0]),) + k[1:]
        if k not in self._memo:
            raise KeyError(f"state {k} was not visited from the initial state (the reference's getAction would return null)")
        return self._memo[k]

    def getExpectedValue(self, state) -> float:
        return self._lookup(state)[0]

    def getCacheActions(self):
        """{state key (period, i1, i2, preQ1, preQ2, cash or R): action pair} in the reference's key order."""
        return {k: v[1:] for k, v in sorted(self._memo.items())} if self._memo else {}

    @property
    def result(self) -> MultiLeadResult:
        return self._result

    _kind = None  # "multilead" / "multicash" / "multixr"

    def policy(self, capacity_log2: int = 0) -> MultiPolicy:
        """The computed policy on the device, from the memo the first getExpectedValue read back."""
        if self._result is None:
            raise RuntimeError("policy(): ask getExpectedValue for the period-1 state first (it runs the solve)")
        return MultiPolicy(self._kind, self._result.table, capacity_log2, **self._solve_kw)


class CashRecursionMultiLead(_MultiRecursionBase):
    """sdp.cash.multiItem.CashRecursionMultiLead (CashRecursionMultiLead.java:31-101) for the lambdas of
    MultiProductLeadtime.main; functor = the keyword arguments of multilead_solve (initial state and T come from the call)."""

    _kind = "multilead"

    def _run(self, f, ini):
        kw = dict(f, ini_i1=ini[1], ini_i2=ini[2], ini_cash=ini[5])
        self._solve_kw = dict(kw)
        return multilead_solve(table=True, **kw)

    def getAction(self, state: CashStateMultiLead) -> Actions:
        _, a1, a2 = self._lookup(state)
        return Actions(a1, a2)


class CashRecursionMulti(_MultiRecursionBase):
    """sdp.cash.multiItem.CashRecursionMulti (CashRecursionMulti.java:39-211) for the lambdas of MultiItemCash.main;
    functor = the keyword arguments of multicash_solve; `Pmf` = the per-period lists GetPmfMulti.getPmf(t) returns."""

    _kind = "multicash"

    def _run(self, f, ini):
        kw = dict(f, ini_i1=ini[1], ini_i2=ini[2], ini_cash=ini[5], pmf=self.Pmf)
        self._solve_kw = dict(kw)
        return multicash_solve(table=True, **kw)

    def getAction(self, state: CashStateMulti) -> Actions:
        _, a1, a2 = self._lookup(state)
        return Actions(a1, a2)

    def getOptTable(self, variCost):
        """CashRecursionMulti.java:171-199: rows {period, x1, x2, w, R, boolAlpha, alpha, Q1, Q2, c1, c2}."""
        rows = []
        for (period, x1, x2, _, _, w), (_, Q1, Q2) in sorted(self._memo.items()):
            alpha, boolAlpha = 10000.0, 0.0
            R = w + x1 * variCost[0] + x2 * variCost[1]
            if w <= variCost[0] * Q1 + variCost[1] * Q2 and Q1 > 0 and Q2 > 0:
                boolAlpha = 1.0
                alpha = variCost[0] * Q1 / w
            rows.append([period, x1, x2, w, R, boolAlpha, alpha, float(Q1), float(Q2), variCost[0], variCost[1]])
        return np.array(rows)


class CashRecursionMultiXR(_MultiRecursionBase):
    """sdp.cash.multiItem.CashRecursionMultiXR (CashRecursionMultiXR.java:39-148) for the lambdas of
    MultiItemCashXR.main; functor = the keyword arguments of multixr_solve (+ "depositeRate")."""

    _kind = "multixr"

    def _run(self, f, ini):
        kw = dict(f, ini_i1=ini[1], ini_i2=ini[2], ini_cash=ini[5], pmf=self.Pmf)
        self._solve_kw = dict(kw)  # (MultiPolicy takes depositeRate by that name)
        dep = kw.pop("depositeRate", 0.0)
        return multixr_solve(dep, table=True, **kw)

    def getAction(self, state: CashStateMultiXR):
        """the optimal order-up-to levels {y1, y2} (CashRecursionMultiXR.java:103-105)."""
        _, y1, y2 = self._lookup(state)
        return [float(y1), float(y2)]

    def getOptTable(self, variCost):
        """CashRecursionMultiXR.java:122-148: rows {period, x1, x2, w, R, boolAlpha, alpha, y1, y2, c1, c2}."""
        rows = []
        for (period, x1, x2, _, _, R), (_, y1, y2) in sorted(self._memo.items()):
            Q1, Q2 = y1 - x1, y2 - x2
            alpha, boolAlpha = 10000.0, 0.0
            w = R - x1 * variCost[0] - x2 * variCost[1]
            if R <= variCost[0] * y1 + variCost[1] * y2 + 0.1 and Q1 > 0.1 and Q2 > 0.1:
                boolAlpha = 1.0
                alpha = variCost[0] * y1 / R
            rows.append([period, x1, x2, w, R, boolAlpha, alpha, float(y1), float(y2), variCost[0], variCost[1]])
        return np.array(rows)


class _MultiSimulationBase:
    """What the two simulators share: the sampled rollout of the recursion's policy on the device.  The reference draws two
    independent latin-hypercube columns per period (Sampling.generateLHSamplesMultiProd); here ONE uniform per (path, period)
    picks a row of the period's joint tile, so that every path stays inside the memo ("Two-product rollout").
    `distributions`, stateTransition and immediateValue are kept for the caller; the device evaluates the closed forms the
    recursion's functor names."""

    def __init__(self, sampleNum, distributions, discountFactor, recursion, stateTransition=None, immediateValue=None, *, seed: int = 0):
        self.sampleNum, self.distributions, self.discountFactor, self.recursion = int(sampleNum), distributions, discountFactor, recursion
        self.stateTransition, self.immediateValue = stateTransition, immediateValue
        self.seed = seed
        self.last_result = None

    def setSampleNum(self, n):
        self.sampleNum = int(n)

    def _simulate(self, iniState) -> float:
        self.recursion.getExpectedValue(iniState)  # (the first call runs the solve)
        if iniState._key() != self.recursion._ini:
            raise ValueError("the policy's paths start at the period-1 state the recursion was solved from; simulate from that state")
        T = len(self.recursion.result.statesPerPeriod)
        with self.recursion.policy() as pol:
            # Math.pow(discountFactor, t)
            self.last_result = pol.simulate_sampled(self.sampleNum, self.seed, discount=[self.discountFactor ** t for t in range(T)])
        return self.last_result.mean


class CashSimulationMulti(_MultiSimulationBase):
    """sdp.cash.multiItem.CashSimulationMulti (CashSimulationMulti.java:23-118) over a CashRecursionMulti."""

    def simulateSDPGivenSamplNum(self, iniState: CashStateMulti) -> float:
        """CashSimulationMulti.java:65-91: the mean of the path sums + iniState.iniCash."""
        return self._simulate(iniState) + iniState.iniCash

    def simulateSDPGivenSamplNumMulti(self, iniState: CashStateMulti) -> float:
        """CashSimulationMulti.java:98-118 (the two-product Poisson driver's call): the same rollout."""
        return self._simulate(iniState) + iniState.iniCash


class CashSimulationMultiXR(_MultiSimulationBase):
    """sdp.cash.multiItem.CashSimulationMultiXR (CashSimulationMultiXR.java:23-88) over a CashRecursionMultiXR."""

    def simulateSDPGivenSamplNum(self, iniState: CashStateMultiXR) -> float:
        """CashSimulationMultiXR.java:61-88: the mean of the path sums + iniState.iniR."""
        return self._simulate(iniState) + iniState.iniR


# ---------------------------------------------------------------------------------------------------------------
# sdp.cash.multiItem.CashRecursionV: the two functional equations V(x1, x2, w) and Pi(y1, y2, R) (sdpgpu_multiv_solve;
# DESIGN 4, "V / Pi recursion").
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class MultiVResult:
    value: float               # getExpectedValueV(iniState), MultiItemYR.java:172
    action: List[float]        # getAction(iniState), :174
    yStar: List[float]         # getYStar(1, iniCash), :179-180
    constrained: bool          # the reference computed alpha(1, iniCash)
    alpha: float               # ... and this is it (defined only then)
    statesPerPeriod: List[int]
    rPerPeriod: List[int]      # distinct R
    entriesPerPeriod: List[int]  # Pi entries: flagged cells of the (R, y1, y2) table + the alpha line of every R
    cells: int
    gpu_ms: float
    forms: int = 0             # SDPGPU_MULTIV_FORM_* bits (_abi.MULTIV_FORMS)
    # rows {period, x1, x2, 0, 0, w, V, y1, y2} in the key order of cacheActions; None unless asked for
    table: object = None
    # rows {period, R, y1*, y2*, constrained, alpha} in the key order of cacheYStar; alpha is defined where constrained is 1
    rtable: object = None


def multiv_alpha_list() -> List[float]:
    """The values `for (alpha = 0; alpha <= 1; alpha = alpha + 0.01)` visits (CashRecursionV.java:180): 100 of them, the
    last 0.9900000000000007 (the 101st would be 1.0000000000000007)."""
    out, alpha = [], 0.0
    while alpha <= 1:
        out.append(alpha)
        alpha = alpha + 0.01
    return out


def _rounding_mode(rounding):
    if rounding in ("trunc10", _abi.MULTIV_TRUNC10):
        return _abi.MULTIV_TRUNC10
    if rounding in ("round", _abi.MULTIV_ROUND):
        return _abi.MULTIV_ROUND
    raise ValueError(f"rounding {rounding!r}: 'trunc10' (MultiItemYR) or 'round' (MultiItemYRTesting)")


def fill_multiv(k, *, T, q_bound, rounding, price, vari_cost, sal_price, ini_cash, ini_i1, ini_i2, min_inventory, max_inventory,
                min_cash, max_cash, pmf, deposit_rate=0.0):
    """pmf[t] = rows {d1, d2, probability} as for fill_multicash; q_bound = Qbound or (Qbound1, Qbound2)."""
    qb = (q_bound, q_bound) if np.isscalar(q_bound) else tuple(q_bound)
    k.T, k.rounding = T, _rounding_mode(rounding)
    k.q_bound[0], k.q_bound[1] = int(qb[0]), int(qb[1])
    for name, val in (("price", price), ("vari_cost", vari_cost), ("sal_price", sal_price)):
        getattr(k, name)[0], getattr(k, name)[1] = val
    for name, val in (("deposit_rate", deposit_rate), ("ini_cash", ini_cash), ("ini_i1", ini_i1), ("ini_i2", ini_i2),
                      ("min_inventory", min_inventory), ("max_inventory", max_inventory), ("min_cash", min_cash),
                      ("max_cash", max_cash)):
        setattr(k, name, float(val))
    if len(pmf) != T:
        raise ValueError(f"pmf has {len(pmf)} periods, T = {T}")
    tiles = [np.asarray(t, dtype=np.float64).reshape(-1, 3) for t in pmf]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tiles])]).astype(np.int32)
    allp = np.concatenate(tiles, axis=0)
    d1, d2, p = (np.ascontiguousarray(allp[:, c]) for c in range(3))
    k._keep = (off, d1, d2, p)
    k.pmf_off = off.ctypes.data_as(C.POINTER(C.c_int32))
    k.d1, k.d2, k.p = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in (d1, d2, p))
    return k


def multiv_solve(table: bool = False, **kw) -> MultiVResult:
    """`sdp.cash.multiItem.CashRecursionV` as `cash.multiItem.MultiItemYR.main` sets it up (MultiItemYR.java:104-181;
    rounding='round' and a pair of bounds: MultiItemYRTesting.main): one call = getExpectedValueV(iniState) +
    getAction(iniState) + getYStar(1, iniCash).  table=True also returns the V states and the (t, R) rows (a second run
    with tables large enough for them)."""
    lib = _abi.load()
    k = fill_multiv(_abi.SdpgpuMultiv(), **kw)
    T = int(k.T)

    def once():
        out = _abi.SdpgpuMultivResult()
        states, rs, entries = ((C.c_int64 * max(T, 1))() for _ in range(3))
        rc = lib.sdpgpu_multiv_solve(C.byref(k), C.byref(out), states, rs, entries)
        if rc:
            raise SdpgpuError(rc, lib.sdpgpu_multilead_last_error().decode())
        return MultiVResult(out.value, [out.y1, out.y2], [out.ystar1, out.ystar2], bool(out.constrained), out.alpha,
                            list(states)[:T], list(rs)[:T], list(entries)[:T], out.cells, out.gpu_ms, forms=int(out.forms))

    res = once()
    if table:
        vt, varrs = _abi.make_multi_table(sum(res.statesPerPeriod))
        rt, rarrs = _abi.make_multiv_rtable(sum(res.rPerPeriod))
        lib.sdpgpu_multi_set_table(C.byref(vt))
        lib.sdpgpu_multiv_set_rtable(C.byref(rt))
        try:
            res = once()
        finally:
            lib.sdpgpu_multi_set_table(None)
            lib.sdpgpu_multiv_set_rtable(None)
        res.table = _abi.multi_table_rows(vt, varrs)
        n = int(rt.rows)
        res.rtable = np.stack([rarrs[c][:n].astype(np.float64) for c in ("period", "R", "y1", "y2", "constrained", "alpha")], axis=1)
    return res


class CashStateMultiYR:
    """sdp.cash.multiItem.CashStateMultiYR (CashStateMultiYR.java:14-40): (period, y1, y2, R)."""

    def __init__(self, period: int, iniInventory1: float, iniInventory2: float, R: float):
        self.period, self.iniInventory1, self.iniInventory2, self.iniR = int(period), float(iniInventory1), float(iniInventory2), float(R)

    def getPeriod(self): return self.period
    def getIniInventory1(self): return self.iniInventory1
    def getIniInventory2(self): return self.iniInventory2
    def getIniR(self): return self.iniR


class CashStateR:
    """sdp.cash.multiItem.CashStateR (CashStateR.java:13-30): (period, R)."""

    def __init__(self, period: int, R: float):
        self.period, self.iniR = int(period), float(R)

    def getPeriod(self): return self.period
    def getIniR(self): return self.iniR


def opt_table(rrows, variCost):
    """CashRecursionV.getOptTable (CashRecursionV.java:251-272) from the (t, R) rows {period, R, y1*, y2*, constrained, alpha}:
    rows {period, R, c1, c2, y1*, y2*, cashConstrained, alpha}, alpha = 10000 where y* is affordable."""
    c1, c2 = variCost
    out = []
    for period, R, y1, y2, cons, a in np.asarray(rrows, dtype=np.float64).reshape(-1, 6):
        cashConstrained, alpha = 0.0, 10000.0
        if c1 * y1 + c2 * y2 >= R + 0.1:
            cashConstrained = 1.0
            alpha = a if cons else float("nan")  # (cacheAlpha.get; the two conditions are the same statement)
        out.append([period, R, c1, c2, y1, y2, cashConstrained, alpha])
    return np.array(out).reshape(-1, 8)


def opt_table_detail(vrows, rrows, variCost):
    """CashRecursionV.getOptTableDetail (CashRecursionV.java:279-325) from the V-state rows {period, x1, x2, ., ., w, V, y1, y2}
    and the (t, R) rows: rows {period, x1, x2, w, c1, c2, R, y1*, y2*, cashConstrained, alpha, yHead1, yHead2} with the
    reference's five cases and tolerances as written.  Case 2 reads cacheAlpha; where the reference never computed it (y* costs
    within 0.1 of R: its `cacheAlpha.get` would throw a NullPointerException) alpha and the yHeads are NaN."""
    c1, c2 = variCost
    rr = np.asarray(rrows, dtype=np.float64).reshape(-1, 6)
    ystar = {(int(r[0]), float(r[1]) + 0.0): r for r in rr}
    out = []
    for row in sorted(np.asarray(vrows, dtype=np.float64).reshape(-1, 9).tolist(), key=lambda r: (r[0], r[1], r[2], r[5])):
        period, x1, x2, w = int(row[0]), row[1], row[2], row[5]
        R = w + c1 * x1 + c2 * x2  # CashStateMulti.getIniR
        rrow = ystar[(period, R + 0.0)]
        ys = (rrow[2], rrow[3])
        cashConstrained, alpha = 0.0, 10000.0
        yHeads = [0.0, 0.0]
        if x1 < ys[0] + 0.1 and x2 < ys[1] and c1 * ys[0] + c2 * ys[1] < R + 0.1:
            yHeads = [ys[0], ys[1]]
            cashConstrained = 1.0
        elif x1 > ys[0] - 0.1 and x2 > ys[1] - 0.1:
            yHeads = [x1, x2]
            cashConstrained = 5.0
        elif x1 > ys[0] - 0.1 and x2 < ys[1] + 0.1:
            yHeads = [x1, min(ys[1], (R - x1 * c1) / c2)]
            cashConstrained = 4.0
        elif x1 < ys[0] + 0.1 and x2 > ys[1] - 0.1:
            yHeads = [min(ys[0], (R - x2 * c2) / c1), x2]
            cashConstrained = 3.0
        elif x1 < ys[0] + 0.1 and x2 < ys[1] + 0.1 and c1 * ys[0] + c2 * ys[1] > R - 0.1:
            alpha = rrow[5] if rrow[4] else float("nan")
            yHeads = [alpha * R / c1, (1 - alpha) * R / c2]
            cashConstrained = 2.0
        out.append([period, x1, x2, w, c1, c2, R, ys[0], ys[1], cashConstrained, alpha, yHeads[0], yHeads[1]])
    return np.array(out).reshape(-1, 13)


class CashRecursionV:
    """sdp.cash.multiItem.CashRecursionV (CashRecursionV.java:28-325) for the lambdas of MultiItemYR.main / MultiItemYRTesting.main;
    functor = the keyword arguments of multiv_solve (initial state, T and pmf come from the calls).  The lambdas are accepted
    and kept for the caller.  discountFactor is kept too and, as in the reference, never used.  The first getExpectedValueV
    runs the solve and reads both tables back; they hold a superset of the reference's memo (the engine evaluates the alpha line
    of every (t, R)), so getOptTable / getOptTableDetail may show rows the reference's run would not have visited."""

    def __init__(self, discountFactor, Pmf, buildActionListV=None, buildActionListPai=None, stateTransition=None,
                 boundFinalCash=None, T=None, variCost=None, *, functor=None):
        if functor is None:
            raise TypeError("functor: the parameters of the driver's lambdas (the keyword arguments of multiv_solve)")
        self.discountFactor, self.Pmf, self.T = discountFactor, Pmf, T
        self.buildActionListV, self.buildActionListPai = buildActionListV, buildActionListPai
        self.stateTransition, self.boundFinalCash = stateTransition, boundFinalCash
        self.functor = dict(functor)
        if T is not None:
            self.functor["T"] = int(T)
        self.variCost = list(variCost) if variCost is not None else list(self.functor["vari_cost"])
        self._result = None

    def _solve(self, state):
        if self._result is None:
            if state.getPeriod() != 1:
                raise ValueError("the first getExpectedValueV must be asked for a period-1 state (it fixes the reachable set)")
            kw = dict(self.functor, ini_i1=state.iniInventory1, ini_i2=state.iniInventory2, ini_cash=state.iniCash, pmf=self.Pmf)
            self._result = multiv_solve(table=True, **kw)
            self._memo = {(int(r[0]), r[1], r[2], r[5] + 0.0): (float(r[6]), [float(r[7]), float(r[8])]) for r in self._result.table.tolist()}
            self._rows = {(int(r[0]), r[1] + 0.0): r for r in self._result.rtable.tolist()}
        return self._result

    @property
    def result(self) -> MultiVResult:
        return self._result

    def _lookup(self, state):
        self._solve(state)
        k = (state.getPeriod(), state.iniInventory1, state.iniInventory2, state.iniCash + 0.0)
        if k not in self._memo:
            raise KeyError(f"state {k} was not visited from the initial state")
        return self._memo[k]

    def getExpectedValueV(self, state: CashStateMulti) -> float:
        return self._lookup(state)[0]

    def getAction(self, state: CashStateMulti):
        """the optimal levels {y1, y2} of (x1, x2, w) (CashRecursionV.java:139-141)."""
        return list(self._lookup(state)[1])

    def _row(self, stateR: CashStateR):
        if self._result is None:
            raise RuntimeError("ask getExpectedValueV for the period-1 state first (it runs the solve)")
        k = (stateR.getPeriod(), stateR.getIniR() + 0.0)
        if k not in self._rows:
            raise KeyError(f"(period, R) = {k} is not an R of a visited state (a new solve would be needed)")
        return self._rows[k]

    def getYStar(self, stateR: CashStateR):
        """y1*, y2* of (t, R) (CashRecursionV.java:149-173)."""
        r = self._row(stateR)
        return [r[2], r[3]]

    def getAlpha(self, stateR: CashStateR) -> float:
        """alpha(t, R) (CashRecursionV.java:176-194), where the reference's solve computed it (y* not affordable)."""
        r = self._row(stateR)
        if not r[4]:
            raise KeyError(f"alpha{(stateR.getPeriod(), stateR.getIniR())}: y* is affordable there, the reference's memo holds no alpha")
        return r[5]

    def getOptTable(self):
        return opt_table(self._result.rtable, self.variCost)

    def getOptTableDetail(self):
        return opt_table_detail(self._result.table, self._result.rtable, self.variCost)
