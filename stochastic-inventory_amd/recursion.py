"""Host-side mirror of the reference's recursion classes, backed by the HIP engine.

Same public names, argument meaning and behaviour as

    sdp.inventory.Recursion              src/sdp/inventory/Recursion.java:33-188
    sdp.inventory.LeadtimeRecursion      src/sdp/inventory/LeadtimeRecursion.java:19-104
    sdp.cash.CashRecursion               src/sdp/cash/CashRecursion.java:23-218
    sdp.cash.CashLeadtimeRecursion       src/sdp/cash/CashLeadtimeRecursion.java:19-107
    capacitated.CLSP (f / cacheActions)  src/capacitated/CLSP.java:61-138

with ONE addition: a `functor` descriptor (functors.py) naming the closed-form family the three
lambdas belong to -- a GPU cannot call host closures per cell.  The lambdas are still accepted
and kept (getStateTransitionFunction / getImmediateValueFunction serve the simulators exactly
as in Simulation.java:39-40); `validateFunctor` checks on sampled cells that they compute what
the functor computes, and runs by itself before the first solve whenever a lambda was supplied
(`recursion.strict = False` turns that off).

`getExpectedValue(state)` runs the full backward sweep on the GPU on its first call (the
reference fills its memo maps on the first call too, Recursion.java:89-163) and answers from
the device tables afterwards.  There is no CPU fallback.
"""
from __future__ import annotations

import random
from typing import Callable, Dict, Optional

import numpy as np

from .cash_structure import CashStructureMethods
from .engine import SdpEngine
from .states import OptDirection


class _GpuRecursionBase:
    _direction_fixed: Optional[OptDirection] = None

    def __init__(self, optDirection, pmf, getFeasibleAction=None, stateTransition=None, immediateValue=None,
                 functor=None, discountFactor: float = 1.0, device: int = -1, kernel: int = 0):
        if functor is None:
            raise TypeError(
                "a functor descriptor is required: the GPU engine evaluates closed-form lambda families, "
                "see stochastic-inventory_amd/functors.py")
        self.optDirection = optDirection
        self.pmf = pmf  # shared by reference, never copied (Recursion.java:54)
        self.functor = functor
        self.T = len(pmf)
        T = self.T
        # lambdas the caller supplied are checked against the functor before the first solve (`strict`, on by
        # default): a driver whose lambdas are NOT the closed-form family would otherwise get tables for a
        # different model without a word, and the simulators would then roll the host lambdas against that policy
        self._user_lambdas = any(f is not None for f in (getFeasibleAction, stateTransition, immediateValue))
        self.strict = True
        self.getFeasibleActions = getFeasibleAction or (lambda s: functor.feasibleActions(s, T))
        self.stateTransition = stateTransition or (lambda s, a, r: functor.stateTransition(s, a, r, T))
        self.immediateValue = immediateValue or (lambda s, a, r: functor.immediateValue(s, a, r, T))
        self.discountFactor = discountFactor
        holder = getattr(functor, "shape", None) or functor  # a CustomFunctor borrows its grid from `shape`
        if hasattr(holder, "discountFactor"):
            holder.discountFactor = discountFactor
        desc = functor.to_desc(T, optDirection)
        desc.device = device
        desc.kernel = kernel
        overhead = functor.overheads(T) if hasattr(functor, "overheads") else None
        source = getattr(functor, "source", None) or None  # CustomFunctor: the lambdas as HIP device text
        self._engine = SdpEngine(desc, pmf, overhead, custom_source=source,
                                 custom_params=getattr(functor, "params", None) if source else None)
        self._solved = False
        self._values: Dict[int, np.ndarray] = {}
        self._policy: Dict[int, np.ndarray] = {}
        self._extra: Dict[object, tuple] = {}  # off-grid states answered by eval_states

    # -- reference API ----------------------------------------------------------------------
    def getStateTransitionFunction(self) -> Callable:
        return self.stateTransition

    def getImmediateValueFunction(self) -> Callable:
        return self.immediateValue

    def setTreeMapCacheAction(self):
        """Recursion.java:80-86 swaps the action map for a TreeMap; the dense tables are already
        in comparator order, so there is nothing to do."""

    def _solve(self):
        if not self._solved:
            if self._user_lambdas and self.strict and all(hasattr(self.functor, m) for m in
                                                          ("feasibleActions", "immediateValue", "stateTransition")):
                self.validateFunctor(nSamples=96)  # raises ValueError on the first cell that differs
            self._engine.solve(sync=True)
            self._solved = True

    def _table(self, period: int):
        if period not in self._values:
            self._values[period] = self._engine.values(period)
            self._policy[period] = self._engine.policy(period)
        return self._values[period], self._policy[period]

    def _lookup(self, state):
        self._solve()
        period = state.getPeriod()
        if period < 1 or period > self.T:
            raise IndexError(f"period {period} outside 1..{self.T}")
        x, cash, preq = self.functor.tuple_of(state)
        idx = self._engine.state_index(period, x, cash, preq)
        if idx >= 0:
            v, p = self._table(period)
            return float(v[idx]), int(p[idx])
        if state not in self._extra:
            val, act = self._engine.eval_states(period, [x], [cash], [preq])
            self._extra[state] = (float(val[0]), int(act[0]))
        return self._extra[state]

    def getExpectedValue(self, state) -> float:
        return self._lookup(state)[0]

    def getAction(self, state) -> float:
        return self._lookup(state)[1] * self.functor.stepSize

    def getCacheActions(self) -> Dict[object, float]:
        """The reference returns its (state -> action) map of VISITED states; here: the reachable set."""
        return {self.functor.make_state(int(r[0]), *self._row_tuple(r)): float(r[-1]) for r in self.getOptTable()}

    def _row_tuple(self, row):
        raise NotImplementedError

    def _opt_columns(self, period, idx, pol):
        raise NotImplementedError

    def getOptTable(self) -> np.ndarray:
        """Rows in the comparator order of the reference's sorted map, reachable states only
        (Recursion.java:177-186 iterates cacheActions, which holds exactly the visited states)."""
        self._solve()
        rows = []
        for period in range(1, self.T + 1):
            mask = self._engine.reachable(period)
            idx = np.nonzero(mask)[0]
            if len(idx) == 0:
                continue
            _, pol = self._table(period)
            rows.append(self._opt_columns(period, idx, pol[idx].astype(np.float64) * self.functor.stepSize))
        ini = self._initial_state()
        if self._engine.state_index(1, *self.functor.tuple_of(ini)) < 0:  # off-grid period-1 state
            rows.insert(0, self._row_of_state(ini, self.getAction(ini)))
        out = np.concatenate(rows, axis=0) if rows else np.zeros((0, self._ncols()))
        return out

    def _initial_state(self):
        f = self.functor
        return f.make_state(1, getattr(f, "iniInventory", 0.0), getattr(f, "iniCash", 0.0), getattr(f, "iniPreQ", 0.0))

    def _row_of_state(self, s, action):
        raise NotImplementedError

    def _ncols(self):
        raise NotImplementedError

    # -- additions --------------------------------------------------------------------------
    @property
    def engine(self) -> SdpEngine:
        return self._engine

    def validateFunctor(self, nSamples: int = 256, seed: int = 1) -> int:
        """Check on sampled (state, action, demand) cells that the lambdas passed to the constructor
        compute exactly what the functor family computes.  Returns the number of cells checked;
        raises ValueError on the first mismatch."""
        rng = random.Random(seed)
        f, T = self.functor, self.T
        checked = 0
        for _ in range(nSamples):
            period = rng.randint(1, T)
            x_lo, nx, nc, nq = self._engine.grid(period)
            ix, ic, iq = rng.randrange(nx), rng.randrange(nc), rng.randrange(nq)
            cash = self._engine.cash_value(ic) if nc > 1 or hasattr(f, "minCashState") else 0.0
            s = f.make_state(period, x_lo + ix * f.stepSize, cash, iq * f.stepSize)
            acts_ref = list(self.getFeasibleActions(s))
            acts = f.feasibleActions(s, T)
            if [float(a) for a in acts_ref] != [float(a) for a in acts]:
                raise ValueError(f"feasible actions differ at {s}: lambda {acts_ref[:5]}.. vs functor {acts[:5]}..")
            a = rng.choice(acts)
            d = rng.choice(self.pmf[period - 1])[0]
            i1, i2 = self.immediateValue(s, a, d), f.immediateValue(s, a, d, T)
            if i1 != i2:
                raise ValueError(f"immediateValue differs at {s}, a={a}, d={d}: lambda {i1!r} vs functor {i2!r}")
            if period < T:
                n1, n2 = self.stateTransition(s, a, d), f.stateTransition(s, a, d, T)
                if f.tuple_of(n1) != f.tuple_of(n2) or n1.getPeriod() != n2.getPeriod():
                    raise ValueError(f"stateTransition differs at {s}, a={a}, d={d}: {n1} vs {n2}")
            checked += 1
        return checked


class Recursion(_GpuRecursionBase):
    """sdp.inventory.Recursion (Recursion.java:49-63): rows of getOptTable are {period, x, Q}."""

    def __init__(self, optDirection, pmf, getFeasibleAction=None, stateTransition=None, immediateValue=None, *,
                 functor=None, device: int = -1, kernel: int = 0):
        super().__init__(optDirection, pmf, getFeasibleAction, stateTransition, immediateValue, functor=functor,
                         device=device, kernel=kernel)

    def _opt_columns(self, period, idx, q):
        x_lo, nx, nc, nq = self._engine.grid(period)
        x = x_lo + idx.astype(np.float64) * self.functor.stepSize
        return np.stack([np.full(len(idx), float(period)), x, q], axis=1)

    def _row_tuple(self, r):
        return (r[1],)

    def _row_of_state(self, s, action):
        return np.array([[float(s.getPeriod()), s.getIniInventory(), action]])

    def _ncols(self):
        return 3


class CLSP(Recursion):
    """capacitated.CLSP: the self-contained copy of the same loop (CLSP.java:88-138), MIN only.
    `f(state)` is its name for getExpectedValue; `cacheActions` its public action map."""

    def __init__(self, pmf, *, functor=None, device: int = -1, kernel: int = 0):
        super().__init__(OptDirection.MIN, pmf, functor=functor, device=device, kernel=kernel)

    def f(self, state) -> float:
        return self.getExpectedValue(state)

    @property
    def cacheActions(self):
        return self.getCacheActions()


class LeadtimeRecursion(_GpuRecursionBase):
    """sdp.inventory.LeadtimeRecursion (LeadtimeRecursion.java:28-45): MIN only; rows
    {period, x, preQ, Q} ordered by (period, x, preQ) (LeadtimeRecursion.java:37-40,93-102)."""

    def __init__(self, pmf, getFeasibleAction=None, stateTransition=None, immediateValue=None, *, functor=None,
                 device: int = -1, kernel: int = 0):
        super().__init__(OptDirection.MIN, pmf, getFeasibleAction, stateTransition, immediateValue, functor=functor,
                         device=device, kernel=kernel)

    def getCacheValues(self):
        self._solve()
        out = {}
        for r in self.getOptTable():
            s = self.functor.make_state(int(r[0]), r[1], 0.0, r[2])
            out[s] = self.getExpectedValue(s)
        return out

    def _opt_columns(self, period, idx, q):
        x_lo, nx, nc, nq = self._engine.grid(period)
        iq, ix = idx // nx, idx % nx
        step = self.functor.stepSize
        rows = np.stack([np.full(len(idx), float(period)), x_lo + ix * step, iq * step, q], axis=1)
        order = np.lexsort((rows[:, 2], rows[:, 1]))  # by x, then preQ
        return rows[order]

    def _row_tuple(self, r):
        return (r[1], 0.0, r[2])

    def _row_of_state(self, s, action):
        return np.array([[float(s.getPeriod()), s.getIniInventory(), s.getPreQ(), action]])

    def _ncols(self):
        return 4


class CashRecursion(_GpuRecursionBase, CashStructureMethods):
    """sdp.cash.CashRecursion (CashRecursion.java:39-56): discounted future term
    `p * discountFactor * V` (CashRecursion.java:120); rows {period, x, cash, Q} (:209-218).  The table methods of
    CashRecursion.java:227-404 (getH, getMinusGAGB, getMinusFG, getH3Column, checkSingleCrossing, checkNonIncreasing,
    checkNonDecreasing) come from cash_structure.CashStructureMethods and run on the host entry point."""

    def __init__(self, optDirection, pmf, getFeasibleAction=None, stateTransition=None, immediateValue=None,
                 discountFactor: float = 1.0, *, functor=None, device: int = -1, kernel: int = 0):
        super().__init__(optDirection, pmf, getFeasibleAction, stateTransition, immediateValue, functor=functor,
                         discountFactor=discountFactor, device=device, kernel=kernel)

    _G_KINDS = {"G": 0, "GA": 1, "GB": 2}

    def drawG(self, kind, minInventorys, maxInventorys, minCash, maxCash, period: int = 1):
        """The sweep of the drivers' second recursion (isForDrawGy; SingleCrossTesting.java:149-165, CashConstraintDraw.java
        :255-283) from THIS handle: kind "G", "GA" or "GB" (or 0, 1, 2).  Returns (resultTable[R - minCash][y - minInventorys],
        yG), yG being the drivers' rows [cash, inventory, value], cash outer."""
        self._solve()
        k = self._G_KINDS[kind] if isinstance(kind, str) else int(kind)
        table = self._engine.cash_g_table(k, period, minInventorys, maxInventorys, minCash, maxCash)
        n_r, n_x = table.shape
        yG = np.empty((n_r * n_x, 3), dtype=np.float64)
        yG[:, 0] = np.repeat(float(minCash) + np.arange(n_r, dtype=np.float64), n_x)
        yG[:, 1] = np.tile(float(minInventorys) + np.arange(n_x, dtype=np.float64), n_r)
        yG[:, 2] = table.reshape(-1)
        return table, yG

    def structure(self, mask, minInventorys, maxInventorys, minCash, maxCash, period: int = 1, *, fixCost=None, variCost=None,
                  want_tables: bool = True):
        """The device path from the solved handle: the derived tables and checks `mask` names (cash_structure.mask_of) on the
        window, G / GA / GB / F never leaving the device unless want_tables.  -> cash_structure.CashStructure."""
        self._solve()
        return self._engine.cash_structure(mask, period, minInventorys, maxInventorys, minCash, maxCash, fix_cost=fixCost, vari_cost=variCost,
                                           want_tables=want_tables)

    def _opt_columns(self, period, idx, q):
        x_lo, nx, nc, nq = self._engine.grid(period)
        ix, ic = idx // nc, idx % nc
        cash = np.array([self._engine.cash_value(int(c)) for c in np.unique(ic)])
        cash_of = dict(zip(np.unique(ic).tolist(), cash.tolist()))
        return np.stack([np.full(len(idx), float(period)), x_lo + ix * self.functor.stepSize,
                         np.array([cash_of[int(c)] for c in ic]), q], axis=1)

    def _row_tuple(self, r):
        return (r[1], r[2])

    def _row_of_state(self, s, action):
        return np.array([[float(s.getPeriod()), s.getIniInventory(), s.getIniCash(), action]])

    def _ncols(self):
        return 4


class CashRecursionXR(CashRecursion):
    """sdp.cash.CashRecursionXR (CashRecursionXR.java:39-56,79-126): the discounted loop of CashRecursion on
    CashStateXR keys (period, x, R), R = cash + variCost * x; the actions ARE order-up-to levels, so getAction
    returns y (`bestY`, :96,:103-113).  Rows of getOptTable are {period, x, S, R, y} with S = R - unitVariCost * x
    (:185-200).  Functor: CashXRFunctor (the lambdas of cash.singleItem.CashConstraintXR)."""

    def getAction(self, state) -> float:
        return state.getIniInventory() + self._lookup(state)[1] * self.functor.stepSize

    def _opt_columns(self, period, idx, q):
        x_lo, nx, nc, nq = self._engine.grid(period)
        ix, ic = idx // nc, idx % nc
        x = x_lo + ix * self.functor.stepSize
        cash_of = {int(c): self._engine.cash_value(int(c)) for c in np.unique(ic)}
        cash = np.array([cash_of[int(c)] for c in ic])
        R = cash + self.functor.variCost * x  # what the transition stores (CashConstraintXR.java:121)
        return np.stack([np.full(len(idx), float(period)), x, R - self.functor.variCost * x, R, x + q], axis=1)

    def _row_tuple(self, r):
        return (r[1], r[3])

    def _row_of_state(self, s, action):
        return np.array([[float(s.getPeriod()), s.getIniInventory(), s.getIniR() - self.functor.variCost * s.getIniInventory(),
                          s.getIniR(), action]])

    def _ncols(self):
        return 5

    def getCacheActions(self):
        return {self.functor.make_state(int(r[0]), r[1], r[3]): float(r[4]) for r in self.getOptTable()}


class RecursionG:
    """sdp.cash.RecursionG(pmf, distributions, price, variCost, depositeRate, salvageValue) (RecursionG.java:47-72): Chao's
    a* of every period by the two mutually recursive functions G and getAStar (:96-153), on the host (sdpgpu_xr_opt_levels;
    no device and no engine).  `distributions` is kept for the signature only: the constructor's aNStar, an SSJ quantile of
    the last one, is overwritten by getOptY's loop (:83-86) before anything reads it.  maxY is the reference's hard-coded 200
    (:136)."""

    def __init__(self, pmf, distributions, price: float, variCost: float, depositeRate: float, salvageValue: float):
        self.pmf = [np.asarray(t, dtype=np.float64) for t in pmf]
        self.distributions = distributions
        self.price, self.variCost = float(price), float(variCost)
        self.depositeRate, self.salvageValue = float(depositeRate), float(salvageValue)

    def getOptY(self, maxY: int = 200) -> np.ndarray:
        import ctypes as C

        from . import _abi
        lib = _abi.load()
        T = len(self.pmf)
        off = np.zeros(T + 1, dtype=np.int64)
        for t, tile in enumerate(self.pmf):
            if tile.ndim != 2 or tile.shape[1] != 2:
                raise ValueError(f"pmf[{t}] of shape {tile.shape}: rows of [demand, probability]")
            off[t + 1] = off[t] + len(tile)
        dem = np.ascontiguousarray(np.concatenate([t[:, 0] for t in self.pmf])) if T else np.zeros(0)
        prob = np.ascontiguousarray(np.concatenate([t[:, 1] for t in self.pmf])) if T else np.zeros(0)
        out = np.zeros(max(T, 1), dtype=np.float64)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        rc = lib.sdpgpu_xr_opt_levels(T, off.ctypes.data_as(C.POINTER(C.c_int64)), dp(dem), dp(prob), self.price, self.variCost,
                                      self.depositeRate, self.salvageValue, int(maxY), dp(out))
        if rc:
            raise _abi.SdpgpuError(rc, lib.sdpgpu_last_error(None).decode())
        return out[:T]


class RiskRecursion(CashRecursion):
    """sdp.cash.RiskRecursion (RiskRecursion.java:31-46): the survival-probability recursion, MAX only, no
    discount; `getSurvProb` (:65-108) takes the place of getExpectedValue.  Rows of getOptTable are
    {period, x, cash, bankruptBefore, Q} (:123-132; the flag is always 0, RiskState.java:17)."""

    def __init__(self, pmf, getFeasibleAction=None, stateTransition=None, immediateValue=None, *, functor=None,
                 device: int = -1, kernel: int = 0):
        super().__init__(OptDirection.MAX, pmf, getFeasibleAction, stateTransition, immediateValue, 1.0,
                         functor=functor, device=device, kernel=kernel)

    def getSurvProb(self, state) -> float:
        return self._lookup(state)[0]

    def getExpectedValue(self, state):
        raise AttributeError("RiskRecursion has getSurvProb, not getExpectedValue (RiskRecursion.java:65)")

    def _opt_columns(self, period, idx, q):
        c = super()._opt_columns(period, idx, q)
        return np.concatenate([c[:, :3], np.zeros((len(idx), 1)), c[:, 3:]], axis=1)

    def _row_tuple(self, r):
        return (r[1], r[2])

    def _row_of_state(self, s, action):
        return np.array([[float(s.getPeriod()), s.getIniInventory(), s.getIniCash(), 0.0, action]])

    def _ncols(self):
        return 5


class CashLeadtimeRecursion(_GpuRecursionBase):
    """sdp.cash.CashLeadtimeRecursion (CashLeadtimeRecursion.java:28-46): MAX only, no discount;
    rows {period, x, cash, preQ, Q} (:97-106).  The reference's comparator (:37-41) is malformed
    (its cash test compares a value with itself); this mirror keys on the full tuple."""

    def __init__(self, pmf, getFeasibleAction=None, stateTransition=None, immediateValue=None, *, functor=None,
                 device: int = -1, kernel: int = 0):
        super().__init__(OptDirection.MAX, pmf, getFeasibleAction, stateTransition, immediateValue, functor=functor,
                         device=device, kernel=kernel)

    def getCacheValues(self):
        self._solve()
        out = {}
        for r in self.getOptTable():
            s = self.functor.make_state(int(r[0]), r[1], r[2], r[3])
            out[s] = self.getExpectedValue(s)
        return out

    def _opt_columns(self, period, idx, q):
        x_lo, nx, nc, nq = self._engine.grid(period)
        ic = idx % nc
        r = idx // nc
        ix, iq = r % nx, r // nx
        step = self.functor.stepSize
        ucs = np.unique(ic)
        cash_of = {int(c): self._engine.cash_value(int(c)) for c in ucs}
        rows = np.stack([np.full(len(idx), float(period)), x_lo + ix * step,
                         np.array([cash_of[int(c)] for c in ic]), iq * step, q], axis=1)
        order = np.lexsort((rows[:, 2], rows[:, 3], rows[:, 1]))  # by x, preQ, cash
        return rows[order]

    def _row_tuple(self, r):
        return (r[1], r[2], r[3])

    def _row_of_state(self, s, action):
        return np.array([[float(s.getPeriod()), s.getIniInventory(), s.getIniCash(), s.getPreQ(), action]])

    def _ncols(self):
        return 5


class RecursionBatch:
    """Many sdp.inventory.Recursion objects behind one solve: the body of a parameter sweep such as
    capacitated.CLSPTesting.main (CLSPTesting.java:58-118), which builds a Recursion per parameter set and asks each for
    getExpectedValue(initialState) and getAction(initialState).  `functors[i]` / `pmfs[i]` describe instance i (backorder
    family, same inventory bounds, order limit, step and horizon; costs, initial inventory and demand tiles are the
    instance's own).  With `ragged=True` the inventory bounds and the order limit are the instance's own as well, as in
    capacitated.fitss.ThreeLevelFitsSTest.main (ThreeLevelFitsSTest.java:67-77), and states are looked up on its own grid.  The first query runs period t of ALL instances in one kernel launch per period (SdpBatch); every
    instance's answers are those of its own Recursion, bit for bit.  There is no CPU fallback."""

    def __init__(self, functors, pmfs, optDirection: OptDirection = OptDirection.MIN, device: int = -1, ragged: bool = False):
        from .batch import SdpBatch
        self.functors = list(functors)
        self.pmfs = pmfs  # shared by reference, never copied (Recursion.java:54)
        if not self.functors:
            raise ValueError("a batch needs at least one instance")
        if len(self.functors) != len(pmfs):
            raise ValueError(f"{len(self.functors)} functors but {len(pmfs)} pmfs")
        self.optDirection = optDirection
        self.T = len(pmfs[0])
        descs = [f.to_desc(self.T, optDirection) for f in self.functors]
        self._batch = SdpBatch(descs, pmfs, ragged=ragged, device=device)
        self._solved = False
        self._values: Dict[tuple, np.ndarray] = {}
        self._policy: Dict[tuple, np.ndarray] = {}
        self._initial = None

    def __len__(self):
        return len(self.functors)

    @property
    def batch(self):
        return self._batch

    def close(self):
        self._batch.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _solve(self):
        if not self._solved:
            self._batch.solve(sync=True)
            self._solved = True

    def _lookup(self, i: int, state):
        self._solve()
        f = self.functors[i]
        period = state.getPeriod()
        if period < 1 or period > self.T:
            raise IndexError(f"period {period} outside 1..{self.T}")
        x = state.getIniInventory()
        pos = (x - f.minInventory) / f.stepSize
        if pos != int(pos) or not 0 <= pos < self._batch.num_states_of(i):
            raise ValueError(f"state {x} is not a point of the batch's grid [{f.minInventory}, {f.maxInventory}]")
        if period == 1 and x == f.iniInventory:  # what a sweep asks of every instance: one gathered copy for all of them
            if self._initial is None:
                self._initial = self._batch.initial()
            return float(self._initial[0][i]), int(self._initial[1][i])
        if (i, period) not in self._values:
            self._values[(i, period)] = self._batch.values(i, period)
            self._policy[(i, period)] = self._batch.policy(i, period)
        return float(self._values[(i, period)][int(pos)]), int(self._policy[(i, period)][int(pos)])

    def getExpectedValue(self, i: int, state) -> float:
        return self._lookup(i, state)[0]

    def getAction(self, i: int, state) -> float:
        return self._lookup(i, state)[1] * self.functors[i].stepSize

    def getOptTable(self, i: int) -> np.ndarray:
        """Instance i's rows [period, inventory, quantity] in the comparator's order, reachable states only -- what
        Recursion.getOptTable gives for a handle of the instance (Recursion.java:177-186).  The reachable states of a batch
        instance are one interval of grid indices per period (SdpBatch.reachable)."""
        self._solve()
        f = self.functors[i]
        rows = []
        for period in range(1, self.T + 1):
            lo, hi = self._batch.reachable(i, period)
            if (i, period) not in self._policy:
                self._values[(i, period)] = self._batch.values(i, period)
                self._policy[(i, period)] = self._batch.policy(i, period)
            idx = np.arange(lo, hi + 1)
            x = f.minInventory + idx.astype(np.float64) * f.stepSize
            q = self._policy[(i, period)][idx].astype(np.float64) * f.stepSize
            rows.append(np.stack([np.full(len(idx), float(period)), x, q], axis=1))
        return np.concatenate(rows, axis=0)

    def _check_convexity(self, kind, source, period, x_lo, x_hi, fixOrderCost, capacity):
        self._solve()
        return self._batch.check_convexity(kind, source=source, period=period, x_lo=x_lo, x_hi=x_hi, K=fixOrderCost, capacity=capacity)

    def checkKConvexity(self, source="values", period: int = 1, x_lo=None, x_hi=None, fixOrderCost=None):
        """CheckKConvexity.check (CheckKConvexity.java:39-68) on V_period ("values") or G_period ("gy") of every instance
        over the window x_lo .. x_hi, on the device in one launch: the reference's return value per instance."""
        return [bool(h) for h in self._check_convexity(0, source, period, x_lo, x_hi, fixOrderCost, None)["holds"]]

    def checkCK(self, source="values", period: int = 1, x_lo=None, x_hi=None, fixOrderCost=None, capacity=None):
        """CheckKConvexity.checkCK (:6-36; ThreeLevelFitsSTest.java:146-159 is source "values", period 1, window 0 .. 100,
        the instance's own fixedOrderingCost and maxOrderQuantity): "CK convexity holds" or "not CK convex" per instance."""
        from .structure import CK_FAILS, CK_HOLDS
        return [CK_HOLDS if h else CK_FAILS for h in self._check_convexity(1, source, period, x_lo, x_hi, fixOrderCost, capacity)["holds"]]
