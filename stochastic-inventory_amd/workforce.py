"""Host-side mirror of the reference's workforce recursion, backed by the HIP engine (STAFF family).

    workforce.StaffState        src/workforce/StaffState.java:4-35
    workforce.StaffRecursion    src/workforce/StaffRecursion.java:16-118, 262-279
    workforce.SimulatesS        src/workforce/SimulatesS.java:14-94

Same names, argument meaning and behaviour for the path the drivers solve -- `getExpectedValue(StaffState)`
(WorkforcePlanning.java:104-112, WorkforceTesting.java:116-124): the turnover pmf of a period is picked by the
hire-up-to level, `pmfs[t][min(iniStaffNum + orderQty, pmfs[t].length - 1)]` (StaffRecursion.java:92-95).  As with the
other mirrors the three lambdas are kept for the caller's own use and a `functor` descriptor names the closed-form
family the device evaluates.  The G(y)-drawing variant the driver uses (`getExpectedValue(state, hireUpStaffNum)` on a
second recursion with special period-1 lambdas, WorkforcePlanning.java:165-211) lives in `StaffRecursion.drawGy` and
`.checkK`: a G entry is one sum against this recursion's own V_{t+1}, formed on the device for any period (DESIGN 4,
"Workforce structure rows"); the method itself keeps raising NotImplementedError.  `getExpectedValue2` and
`getExpectedValueNoHireFirst` (StaffRecursion.java:175-330), which no driver calls, are not built.  There is no CPU
fallback.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import _abi
from .engine import SdpEngine


class StaffState:
    """workforce.StaffState: (period, iniStaffNum), both ints."""

    __slots__ = ("period", "iniStaffNum")

    def __init__(self, period: int, iniStaffNum: int):
        object.__setattr__(self, "period", int(period))
        object.__setattr__(self, "iniStaffNum", int(iniStaffNum))

    def __setattr__(self, *a):
        raise AttributeError("StaffState is immutable")

    def __eq__(self, o):
        return isinstance(o, StaffState) and o.period == self.period and o.iniStaffNum == self.iniStaffNum

    def __hash__(self):
        return hash((self.period, self.iniStaffNum))

    def __repr__(self):
        return f"period = {self.period}, initial staff number = {self.iniStaffNum}"


@dataclass
class StaffFunctor:
    """F7: the lambdas of WorkforcePlanning.java:72-101 (clampStaff True) / WorkforceTesting.java:80-107 (False)."""

    fixCost: float = 0.0
    unitVariCost: float = 0.0
    salary: float = 0.0
    unitPenalty: float = 0.0
    minStaffNum: Sequence[int] = field(default_factory=list)  # per period
    maxHireNum: int = 0
    minX: int = 0
    maxX: int = 0
    clampStaff: bool = True
    iniStaffNum: int = 0

    stepSize = 1

    def to_desc(self, T: int):
        if len(self.minStaffNum) != T:
            raise ValueError("minStaffNum needs one entry per period")
        d = _abi.desc_defaults()
        d.family = _abi.FAMILY_STAFF
        d.direction = _abi.MIN
        d.periods = T
        d.step = 1.0
        d.min_inventory, d.max_inventory = float(self.minX), float(self.maxX)
        d.clamp_inventory = 1 if self.clampStaff else 0
        d.ini_inventory = float(self.iniStaffNum)
        d.max_order_quantity = float(self.maxHireNum)
        d.fixed_order_cost, d.unit_order_cost = self.fixCost, self.unitVariCost
        d.holding_cost, d.penalty_cost = self.salary, self.unitPenalty
        return d

    # host restatement (default lambdas; never used to compute tables)
    def feasibleActions(self, s) -> List[int]:
        return list(range(0, self.maxHireNum + 1))

    def immediateValue(self, s, action: int, randomDemand: int) -> float:
        fixHireCost = self.fixCost if action > 0 else 0.0
        variHireCost = self.unitVariCost * action
        nextStaffNum = s.iniStaffNum + action - randomDemand
        salaryCost = self.salary * nextStaffNum
        t = s.period - 1
        penaltyCost = 0.0 if nextStaffNum > self.minStaffNum[t] else self.unitPenalty * (self.minStaffNum[t] - nextStaffNum)
        return fixHireCost + variHireCost + salaryCost + penaltyCost

    def stateTransition(self, s, action: int, randomDemand: int) -> StaffState:
        nextStaffNum = s.iniStaffNum + action - randomDemand
        if self.clampStaff:
            nextStaffNum = self.maxX if nextStaffNum > self.maxX else nextStaffNum
            nextStaffNum = self.minX if nextStaffNum < self.minX else nextStaffNum
        return StaffState(s.period + 1, nextStaffNum)


def pack_level_pmf(pmf) -> tuple:
    """The reference's `double[T][rows][len][2]` (pmfs[t][y][j] = {j, prob}) -> (table (T, rows, stride), row_len or
    None).  An ndarray (T, rows, stride) is passed through (row y then has y + 1 entries)."""
    if isinstance(pmf, np.ndarray) and pmf.ndim == 3:
        return np.ascontiguousarray(pmf, dtype=np.float64), None
    T, rows = len(pmf), len(pmf[0])
    lens = [len(r) for r in pmf[0]]
    stride = max(max(len(r) for r in per) for per in pmf)
    table = np.zeros((T, rows, stride))
    for t, per in enumerate(pmf):
        if len(per) != rows or [len(r) for r in per] != lens:
            raise ValueError("every period must have the same table shape")
        for y, row in enumerate(per):
            arr = np.asarray(row, dtype=np.float64).reshape(-1, 2)
            if not np.array_equal(arr[:, 0], np.arange(len(arr))):
                raise ValueError(f"pmfs[{t}][{y}][j][0] must be j (WorkforcePlanning.java:64)")
            table[t, y, :len(arr)] = arr[:, 1]
    default = lens == [y + 1 for y in range(rows)]
    return table, (None if default else np.asarray(lens, dtype=np.int32))


class StaffRecursion:
    """workforce.StaffRecursion(getFeasibleAction, stateTransition, immediateValue, pmf, T) -- StaffRecursion.java:42-56."""

    def __init__(self, getFeasibleAction: Optional[Callable] = None, stateTransition: Optional[Callable] = None,
                 immediateValue: Optional[Callable] = None, pmf=None, T: Optional[int] = None, *,
                 functor: Optional[StaffFunctor] = None, device: int = -1, separable: bool = False):
        """separable: opt into SDPGPU_KERNEL_SEPARABLE (one G(y) row per period instead of every (state, hire, turnover)
        cell): values within 1e-9 relative of the cell-by-cell tables, the hire count may differ where two actions tie to
        that rounding (include/sdpgpu.h)."""
        if functor is None:
            raise TypeError("a StaffFunctor descriptor is required: the GPU engine evaluates closed-form lambda families")
        if pmf is None:
            raise TypeError("pmf: the level-dependent table pmfs[t][y][j]")
        table, row_len = pack_level_pmf(pmf)
        self.T = int(T) if T is not None else table.shape[0]
        if table.shape[0] != self.T:
            raise ValueError(f"pmf has {table.shape[0]} periods, T = {self.T}")
        self.pmfs = pmf
        self.functor = functor
        self.getFeasibleAction = getFeasibleAction or functor.feasibleActions
        self.stateTransition = stateTransition or functor.stateTransition
        self.immediateValue = immediateValue or functor.immediateValue
        desc = functor.to_desc(self.T)
        desc.device = device
        if separable:
            desc.kernel = _abi.KERNEL_SEPARABLE
        self._engine = SdpEngine(desc, None, [float(m) for m in functor.minStaffNum], level_pmf=table,
                                 level_row_len=row_len)
        self._solved = False
        self._tables = {}

    def getStateTransitionFunction(self):
        return self.stateTransition

    def getImmediateValueFunction(self):
        return self.immediateValue

    @property
    def engine(self) -> SdpEngine:
        return self._engine

    def _lookup(self, state: StaffState):
        if not self._solved:
            self._engine.solve(sync=True)
            self._solved = True
        period = state.period
        if period < 1 or period > self.T:
            raise IndexError(f"period {period} outside 1..{self.T}")
        if period not in self._tables:
            self._tables[period] = (self._engine.values(period), self._engine.policy(period))
        idx = self._engine.state_index(period, float(state.iniStaffNum), 0.0, 0.0)
        if idx < 0:
            raise KeyError(f"{state!r} lies outside the staff numbers the recursion can reach")
        v, p = self._tables[period]
        return float(v[idx]), int(p[idx])

    def getExpectedValue(self, state: StaffState, hireUpStaffNum: Optional[int] = None) -> float:
        if hireUpStaffNum is not None:
            raise NotImplementedError("the G(y)-drawing variant (StaffRecursion.java:127-172) is not built")
        return self._lookup(state)[0]

    def getAction(self, state: StaffState) -> int:
        return self._lookup(state)[1]

    def drawGy(self, minX: int, maxX: int, period: int = 1) -> np.ndarray:
        """The driver's `yG` (WorkforcePlanning.java:199-206) as an (n, 2) array: rows {y, G_period(y)} for y = minX .. maxX,
        formed on the device against this recursion's own V_{period+1} (SdpEngine.staff_gy)."""
        self._lookup(StaffState(1, self.functor.iniStaffNum))
        g = self._engine.staff_gy(period, int(minX), int(maxX))
        return np.stack([np.arange(int(minX), int(maxX) + 1, dtype=np.float64), g], axis=1)

    def checkK(self, period: int = 1, source: str = "gy", kind: int = 0, fixCost: Optional[float] = None, capacity: Optional[int] = None,
               minX: Optional[int] = None, maxX: Optional[int] = None):
        """`CheckKConvexity.check(yG, fixCost)` (WorkforcePlanning.java:208-209; kind 1: checkCK) on G_period ("gy") or V_period
        ("values"), formed and checked on the device (SdpEngine.staff_check_convexity).  fixCost defaults to the functor's,
        capacity to the hire limit, the window to the whole row.  Returns the sdpgpu_convexity record."""
        self._lookup(StaffState(1, self.functor.iniStaffNum))
        return self._engine.staff_check_convexity(kind, source, period, minX, maxX, fixCost, capacity)

    def getOptTable(self) -> np.ndarray:
        """Rows {period, iniStaffNum, action} of the visited states in comparator order (StaffRecursion.java:245-254)."""
        self._lookup(StaffState(1, self.functor.iniStaffNum))
        rows = []
        for period in range(1, self.T + 1):
            idx = np.nonzero(self._engine.reachable(period))[0]
            if len(idx) == 0:
                continue
            x_lo = self._engine.grid(period)[0]
            if period not in self._tables:
                self._tables[period] = (self._engine.values(period), self._engine.policy(period))
            pol = self._tables[period][1]
            rows.append(np.stack([np.full(len(idx), float(period)), x_lo + idx.astype(np.float64),
                                  pol[idx].astype(np.float64)], axis=1))
        return np.concatenate(rows, axis=0) if rows else np.zeros((0, 3))

    def close(self):
        self._engine.close()


class SimulatesS:
    """workforce.SimulatesS(recursion, T, dimissionRate) -- SimulatesS.java:21-27: the rollout of an (s, S) hiring rule on a
    sampled tree, on the device (SdpEngine.staff_simulate; DESIGN 4, "Workforce rollout on a sampled tree").

    `dimissionRate` is kept for the signature and NOT used: the turnover of a period is drawn from the row of the recursion's own
    table, pmfs[t][min(hireTo, rows - 1)] -- for the drivers' tables that row IS BinomialDist(hireTo, dimissionRate[t]).  The
    reference resets its random stream per call (Sampling.resetStartStream); here the draws are a function of `seed`."""

    def __init__(self, recursion: StaffRecursion, T: int, dimissionRate=None, seed: int = 12345):
        if int(T) != recursion.T:
            raise ValueError(f"T = {T}, the recursion has {recursion.T} periods")
        self.recursion = recursion
        self.T = int(T)
        self.dimissionRate = dimissionRate
        self.seed = int(seed)
        self.stateTransition = recursion.getStateTransitionFunction()
        self.immediateValue = recursion.getImmediateValueFunction()
        self.last_results = None

    def defaultSampleNums(self) -> List[int]:
        """10 children in the first four periods, one from the fifth on (SimulatesS.java:33-41)."""
        return [10 if t <= 3 else 1 for t in range(self.T)]

    @staticmethod
    def _ini(iniState) -> int:
        return int(iniState.iniStaffNum) if isinstance(iniState, StaffState) else int(iniState)

    def simulatesS(self, iniState, optimalsS, sampleNums=None):
        """Mean of the leaf sums under the level rule optimalsS[t] = (s, S): a float for shape (T, 2), an array for (R, T, 2)
        (R rules in one launch, on the same uniforms).  The SdpgpuSimResults stay in `last_results`."""
        ss = np.asarray(optimalsS, dtype=np.float64)
        k = self.defaultSampleNums() if sampleNums is None else sampleNums
        res = self.recursion.engine.staff_simulate(k, self.seed, self._ini(iniState), ss)
        self.last_results = res
        means = np.array([r.mean for r in res])
        return float(means[0]) if ss.ndim == 2 else means

    def simulateTable(self, iniState, sampleNums=None) -> float:
        """The same rollout under the recursion's own policy table (solved first if it has not been)."""
        self.recursion._lookup(StaffState(1, self.recursion.functor.iniStaffNum))
        k = self.defaultSampleNums() if sampleNums is None else sampleNums
        res = self.recursion.engine.staff_simulate(k, self.seed, self._ini(iniState), None)
        self.last_results = res
        return float(res[0].mean)


def staff_reach_intervals(functor: StaffFunctor, lens_by_period) -> list:
    """[(L, H)] per period: the staff numbers StaffRecursion.getExpectedValue visits from (1, iniStaffNum) -- one interval a
    period, as the library computes it for a handle: from the levels y in [L, H + maxHire] the successors are the union of
    [y - len(y) + 1, y].  lens_by_period[t] = the row lengths of period t's table."""
    L = H = int(functor.iniStaffNum)
    out = []
    for lens in lens_by_period:
        out.append((L, H))
        rows = len(lens)
        top = H + int(functor.maxHireNum)
        y = np.arange(L, min(top, rows - 1) + 1, dtype=np.int64)
        low = int((y - lens[y] + 1).min()) if len(y) else None
        if top > rows - 1:
            beyond = max(L, rows) - int(lens[rows - 1]) + 1
            low = beyond if low is None else min(low, beyond)
        L, H = low, top
        if functor.clampStaff:
            L, H = (min(max(v, functor.minX), functor.maxX) for v in (L, H))
    return out


class StaffRecursionBatch:
    """Many workforce.StaffRecursion objects behind one solve: the body of WorkforceTesting.main's sweep
    (WorkforceTesting.java:36-124), which builds a StaffRecursion per parameter set and asks each for
    getExpectedValue(initialState).  `functors[i]` is instance i's StaffFunctor -- one shape for all: hire limit, bounds, clamp
    and iniStaffNum; the costs and minStaffNum are the instance's own -- and `pmfs[i]` its table (T, rows, stride), or the
    reference's nested list.  Per-period slices that ARE the same memory (same data pointer, shape and strides: a
    zero-stride np.broadcast_to view over T, one array handed to many instances) become ONE table of the batch's pool.  The
    first query runs period t of ALL instances in two kernel launches (StaffBatch, the separable mode); every instance's
    answers are those of its own StaffRecursion(separable=True), bit for bit.  There is no CPU fallback."""

    def __init__(self, functors, pmfs, T: Optional[int] = None, device: int = -1):
        from .batch import StaffBatch
        self.functors = list(functors)
        if not self.functors:
            raise ValueError("a batch needs at least one instance")
        if len(self.functors) != len(pmfs):
            raise ValueError(f"{len(self.functors)} functors but {len(pmfs)} pmfs")
        self.pmfs = pmfs
        tables, use, keys, self._keep = [], [], {}, []
        self._lens = []  # [pool id]: row lengths
        for i, pmf in enumerate(pmfs):
            if isinstance(pmf, np.ndarray) and pmf.ndim == 3 and pmf.dtype == np.float64:
                table, row_len = pmf, None  # (never copied: the sweep's views share two buffers)
            else:
                table, row_len = pack_level_pmf(pmf)
            if T is None:
                T = table.shape[0]
            if table.shape[0] != int(T):
                raise ValueError(f"pmf of instance {i} has {table.shape[0]} periods, T = {T}")
            self._keep.append(table)
            row = []
            for t in range(int(T)):
                sl = table[t]
                key = (sl.__array_interface__["data"][0], sl.shape, sl.strides, None if row_len is None else row_len.tobytes())
                if key not in keys:
                    keys[key] = len(tables)
                    tables.append((sl, row_len))
                    self._lens.append(np.arange(sl.shape[0], dtype=np.int64) + 1 if row_len is None else np.asarray(row_len, dtype=np.int64))
                row.append(keys[key])
            use.append(row)
        self.T = int(T)
        self.use = use
        descs = []
        for f in self.functors:
            d = f.to_desc(self.T)
            d.kernel = _abi.KERNEL_SEPARABLE
            descs.append(d)
        self._batch = StaffBatch(descs, tables, use, [list(f.minStaffNum) for f in self.functors], device=device)
        self._solved = False
        self._tables = {}
        self._initial = None
        self._grid = {}
        self.last_results = None

    def __len__(self):
        return len(self.functors)

    @property
    def batch(self):
        return self._batch

    @property
    def num_tables(self) -> int:
        """Tables of the batch's pool."""
        return len(self._lens)

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

    def _table(self, i: int, period: int):
        if (i, period) not in self._tables:
            self._tables[(i, period)] = (self._batch.values(i, period), self._batch.policy(i, period))
        return self._tables[(i, period)]

    def initial(self):
        """(values[n], hires[n]) of (1, iniStaffNum) for all instances: what the sweep records, one gathered copy."""
        self._solve()
        if self._initial is None:
            self._initial = self._batch.initial()
        return self._initial

    def _lookup(self, i: int, state: StaffState):
        self._solve()
        period = state.period
        if period < 1 or period > self.T:
            raise IndexError(f"period {period} outside 1..{self.T}")
        if period == 1 and state.iniStaffNum == self.functors[i].iniStaffNum:
            val, act = self.initial()
            return float(val[i]), int(act[i])
        if period not in self._grid:
            self._grid[period] = self._batch.grid(i, period)
        x_lo, nx = self._grid[period]
        idx = state.iniStaffNum - int(x_lo)
        if not 0 <= idx < nx:
            raise KeyError(f"{state!r} lies outside the staff numbers the recursion can reach")
        v, p = self._table(i, period)
        return float(v[idx]), int(p[idx])

    def getExpectedValue(self, i: int, state: StaffState) -> float:
        return self._lookup(i, state)[0]

    def getAction(self, i: int, state: StaffState) -> int:
        return self._lookup(i, state)[1]

    def getOptTable(self, i: int) -> np.ndarray:
        """Instance i's rows {period, iniStaffNum, action} of the visited states in comparator order -- what
        StaffRecursion.getOptTable gives for a handle of the instance."""
        self._solve()
        rows = []
        for period in range(1, self.T + 1):
            L, H = self._batch.reachable(i, period)  # (staff_reach_intervals above states the same intervals in numpy)
            x_lo = int(self._batch.grid(i, period)[0])
            pol = self._table(i, period)[1]
            x = np.arange(L, H + 1, dtype=np.int64)
            rows.append(np.stack([np.full(len(x), float(period)), x.astype(np.float64), pol[x - x_lo].astype(np.float64)], axis=1))
        return np.concatenate(rows, axis=0) if rows else np.zeros((0, 3))

    # ---- the structure step of WorkforcePlanning.main (WorkforcePlanning.java:165-211), per instance ----
    def drawGy(self, i: int, minX: int, maxX: int, period: int = 1) -> np.ndarray:
        """StaffRecursion.drawGy of instance i: rows {y, G_period(y)}, y = minX .. maxX.  The rows of all instances and periods
        are formed in one launch at the first request after the solve."""
        self._solve()
        g = self._batch.staff_gy(i, period, int(minX), int(maxX))
        return np.stack([np.arange(int(minX), int(maxX) + 1, dtype=np.float64), g], axis=1)

    def checkK(self, i: Optional[int] = None, period: int = 1, source: str = "gy", kind: int = 0, fixCost=None, capacity=None, minX=None,
               maxX=None):
        """StaffRecursion.checkK for every instance in one launch: the records [n], or instance i's alone."""
        self._solve()
        out = self._batch.staff_check_convexity(kind, source, period, minX, maxX, fixCost, capacity)
        return out if i is None else out[i]

    # ---- the rest of WorkforceTesting.main's loop body (WorkforceTesting.java:112-165), for all instances at once ----
    def defaultSampleNums(self) -> List[int]:
        """SimulatesS.defaultSampleNums: 10 children in the first four periods, one from the fifth on."""
        return [10 if t <= 3 else 1 for t in range(self.T)]

    def fitSinglesS(self, maxOrderQuantity: float = 2 ** 31 - 1) -> np.ndarray:
        """`new FitsS(maxOrderQuantity, T).getSinglesS(getOptTable())` of every instance, on the device: (n, T, 2).  No policy
        table comes to the host."""
        self._solve()
        return self._batch.fit_ss(maxOrderQuantity)

    def _rollout(self, ss, sampleNums, seed):
        k = self.defaultSampleNums() if sampleNums is None else sampleNums
        res = self._batch.staff_simulate(k, seed, int(self.functors[0].iniStaffNum), ss)
        self.last_results = res
        return np.array([[r.mean for r in row] for row in res])

    def simulatesS(self, optimalsS, sampleNums=None, seed: int = 12345):
        """`SimulatesS.simulatesS(initialState, optimalsS[i])` of every instance in one rollout launch, from (1, iniStaffNum):
        optimalsS of shape (n, T, 2) gives means (n,), (n, R, T, 2) gives (n, R) -- R rules per instance on the same uniforms
        (the fitted levels and the MIP's, say).  All instances see common random numbers.  The SdpgpuSimResults stay in
        `last_results` [n][R]."""
        ss = np.asarray(optimalsS, dtype=np.float64)
        means = self._rollout(ss, sampleNums, seed)
        return means[:, 0] if ss.ndim == 3 else means

    def simulateTable(self, sampleNums=None, seed: int = 12345) -> np.ndarray:
        """The same rollout under every instance's own policy table (solved first if it has not been): means (n,)."""
        self._solve()
        return self._rollout(None, sampleNums, seed)[:, 0]
