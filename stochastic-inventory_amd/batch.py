"""Thin object wrapper over one sdpgpu_batch (include/sdpgpu.h): N backorder-family instances, period t of all of them in
one kernel launch -- the parameter sweeps of the reference's *Testing mains.  The instances share ONE grid shape
(CLSPTesting.java:33-141) or, with `ragged=True`, each has its own inventory bounds and order limit
(ThreeLevelFitsSTest.java:67-77).

`pmfs[i]` is instance i's `double[][][] pmf` (Recursion.java:38): pmfs[i][t][j] = [demand, prob].

`StaffBatch` is the same object for N workforce (STAFF family) instances of one shape in the separable mode
(WorkforceTesting.java:36-41): a pool of level tables, two launches per period for all instances.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _abi
from ._abi import SdpgpuBatchPlan, SdpgpuBatchStaffPlan, SdpgpuBatchStats, SdpgpuConvexity, SdpgpuDesc, SdpgpuError
from .engine import _dp, _ip, split_pmf


class _Batch:
    """What the two kinds of batch share: one sdpgpu_batch (self._b) of self.n instances, its life time, its stream and timing,
    the solve and the calls that read no table shape."""

    def _check(self, rc: int):
        if rc:
            raise SdpgpuError(rc, self._lib.sdpgpu_batch_last_error(self._b).decode())

    def close(self):
        if getattr(self, "_b", None) is not None and self._b:
            self._lib.sdpgpu_batch_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return self.n

    def set_stream(self, hip_stream: int):
        self._check(self._lib.sdpgpu_batch_set_stream(self._b, C.c_void_p(hip_stream)))

    def set_profiling(self, on: bool):
        self._check(self._lib.sdpgpu_batch_set_profiling(self._b, 1 if on else 0))

    def solve(self, sync: bool = True):
        self._check(self._lib.sdpgpu_batch_solve(self._b, 1 if sync else 0))

    def synchronize(self):
        self._check(self._lib.sdpgpu_batch_synchronize(self._b))

    def num_actions_of(self, i: int) -> int:
        """Actions of instance i (order quantities 0 .. maxOrderQuantity in steps; hires 0 .. maxHireNum)."""
        n = int(self._lib.sdpgpu_batch_num_actions(self._b, i))
        if n < 0:
            raise IndexError(f"instance {i} outside 0 .. {self.n - 1}")
        return n

    def initial(self):
        """(values[n], action_index[n]): V_1 at every instance's initial state (ini_inventory_i; iniStaffNum) and its action
        index (of a workforce batch: the hire count), all instances, one copy."""
        val = np.empty(self.n, dtype=np.float64)
        act = np.empty(self.n, dtype=np.int32)
        self._check(self._lib.sdpgpu_batch_initial(self._b, _dp(val), _ip(act)))
        return val, act

    def stats(self) -> SdpgpuBatchStats:
        st = SdpgpuBatchStats()
        self._check(self._lib.sdpgpu_batch_stats_get(self._b, C.byref(st)))
        return st

    def period_ms(self, period: int) -> float:
        return float(self._lib.sdpgpu_batch_period_ms(self._b, period))


class SdpBatch(_Batch):
    """N independent problems on one GPU -- of one shape, or (ragged=True) each with its own bounds and order limit;
    results per instance are those of N SdpEngines, bit for bit."""

    def __init__(self, descs: Sequence[SdpgpuDesc], pmfs, ragged: bool = False, *, device: int = -1):
        self._lib = _abi.load()
        self._b = C.c_void_p()
        descs = list(descs)
        if len(descs) != len(pmfs):
            raise ValueError(f"{len(descs)} descriptors but {len(pmfs)} pmfs")
        arr = (SdpgpuDesc * max(len(descs), 1))()
        for i, d in enumerate(descs):
            C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(SdpgpuDesc))
            if device >= 0:
                arr[i].device = device
        self.n = len(descs)
        self.ragged = bool(ragged)
        create = self._lib.sdpgpu_batch_create_ragged if self.ragged else self._lib.sdpgpu_batch_create
        rc = create(arr, self.n, C.byref(self._b))
        if rc:
            raise SdpgpuError(rc, self._lib.sdpgpu_batch_last_error(None).decode())
        self.T = int(arr[0].periods)
        self.step = float(arr[0].step)
        self.num_states = int((arr[0].max_inventory - arr[0].min_inventory) / arr[0].step) + 1  # (of instance 0)
        try:
            for i, pmf in enumerate(pmfs):
                tiles = split_pmf(pmf)
                if len(tiles) != self.T:
                    raise ValueError(f"pmf of instance {i} has {len(tiles)} periods, the descriptors say {self.T}")
                for t, (d, p) in enumerate(tiles):
                    self._check(self._lib.sdpgpu_batch_set_pmf(self._b, i, t, _dp(d), _dp(p), len(d)))
        except Exception:
            self.close()
            raise

    def num_states_of(self, i: int) -> int:
        """States of instance i's own grid."""
        n = int(self._lib.sdpgpu_batch_num_states(self._b, i))
        if n < 0:
            raise IndexError(f"instance {i} outside 0 .. {self.n - 1}")
        return n

    def plan(self, period: int) -> SdpgpuBatchPlan:
        """The launch plan of one period (1-based) for the whole batch: host arithmetic, no device needed."""
        pl = SdpgpuBatchPlan()
        self._check(self._lib.sdpgpu_batch_plan_period(self._b, period, C.byref(pl)))
        return pl

    def values(self, i: int, period: int) -> np.ndarray:
        out = np.empty(self.num_states_of(i), dtype=np.float64)
        self._check(self._lib.sdpgpu_batch_values(self._b, i, period, _dp(out), len(out)))
        return out

    def policy(self, i: int, period: int) -> np.ndarray:
        """Arg-opt action INDEX of every state (action = index * step)."""
        out = np.empty(self.num_states_of(i), dtype=np.int32)
        self._check(self._lib.sdpgpu_batch_policy(self._b, i, period, _ip(out), len(out)))
        return out

    # ---- simulation of all instances (sdpgpu_batch_simulate*; Simulation.java:53-74 for the whole sweep) ----
    def _ini(self, ini_x):
        if ini_x is None:
            return None, None
        arr = np.ascontiguousarray(ini_x, dtype=np.float64)
        if arr.shape != (self.n,):
            raise ValueError(f"ini_x has shape {arr.shape}, the batch holds {self.n} instances")
        return arr, _dp(arr)

    def _sim_result(self, mean, sums, want_sums):
        return (mean, sums) if want_sums else mean

    def simulate(self, demands, ini_x=None, want_sums: bool = False):
        """Roll every instance's policy along given demand paths: `demands` is [n_paths, T] (one set shared by all
        instances) or [n, n_paths, T] (a set per instance), already rounded as Simulation.java:64 does.  Returns the n
        means, or (means, sums[n, n_paths]) with want_sums."""
        dem = np.ascontiguousarray(demands, dtype=np.float64)
        if dem.ndim == 2 and dem.shape[1] == self.T:
            n_paths, stride = dem.shape[0], 0
        elif dem.ndim == 3 and dem.shape[0] == self.n and dem.shape[2] == self.T:
            n_paths, stride = dem.shape[1], dem.shape[1] * self.T
        else:
            raise ValueError(f"demands of shape {dem.shape}: expected [n_paths, {self.T}] or [{self.n}, n_paths, {self.T}]")
        ini, ini_p = self._ini(ini_x)
        mean = np.empty(self.n, dtype=np.float64)
        sums = np.empty((self.n, n_paths), dtype=np.float64) if want_sums else None
        self._check(self._lib.sdpgpu_batch_simulate(self._b, n_paths, _dp(dem), stride, ini_p, _dp(mean),
                                                    _dp(sums) if want_sums else None))
        return self._sim_result(mean, sums, want_sums)

    def set_sampler(self, i: int, t: int, dist=None):
        """Distribution the device sampler draws period index `t` of instance `i` from: None = the instance's own pmf tile
        (the default), a pmf.py distribution (PoissonDist / NormalDist / GammaDist / UniformIntDist), an SdpgpuDistSpec, or
        a (kind, a, b) tuple."""
        if dist is None:
            self._check(self._lib.sdpgpu_batch_set_sampler(self._b, i, t, None))
            return
        from .pmf import dist_spec
        spec = dist_spec(dist)
        self._check(self._lib.sdpgpu_batch_set_sampler(self._b, i, t, C.byref(spec)))

    def simulate_sampled(self, n_paths: int, seed: int, ini_x=None, want_sums: bool = False):
        """Draw n_paths latin-hypercube demand paths per instance ON the device (seeded, reproducible) and roll
        the policies along them in the same launch."""
        ini, ini_p = self._ini(ini_x)
        mean = np.empty(self.n, dtype=np.float64)
        sums = np.empty((self.n, int(n_paths)), dtype=np.float64) if want_sums and n_paths > 0 else None
        self._check(self._lib.sdpgpu_batch_simulate_sampled(self._b, int(n_paths), C.c_uint64(seed & (2**64 - 1)), ini_p, _dp(mean),
                                                            _dp(sums) if sums is not None else None))
        return self._sim_result(mean, sums, want_sums)

    def sample_demands(self, i: int, n_paths: int, seed: int):
        """(demands[n_paths, T], uniforms[n_paths, T]) simulate_sampled uses for instance i, from the same device code."""
        dem = np.empty((max(int(n_paths), 0), self.T), dtype=np.float64)
        u = np.empty_like(dem)
        self._check(self._lib.sdpgpu_batch_sample_demands(self._b, i, int(n_paths), C.c_uint64(seed & (2**64 - 1)), _dp(dem), _dp(u)))
        return dem, u

    def simulate_ms(self) -> float:
        return float(self._lib.sdpgpu_batch_simulate_ms(self._b))

    # ---- (s, S) level rules (sdpgpu_batch_reachable / _fit_ss / _simulate_ss*; FitsS.java, SimulateFitsS.java) ----
    def reachable(self, i: int, period: int):
        """(lo, hi): the grid indices of the states of `period` (1-based) the reference's memoised recursion visits from
        instance i's initial state -- one interval.  Host arithmetic, no device."""
        lo, hi = C.c_int32(), C.c_int32()
        self._check(self._lib.sdpgpu_batch_reachable(self._b, i, period, C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def fit_ss(self, levels: int) -> np.ndarray:
        """The one-, two- or three-level (s, S) rule of every instance, fitted ON the device from the solved policy tables
        (FitsS.getSinglesS / getTwosS / getThreesS): [n, T, 2 * levels]."""
        out = np.empty((self.n, self.T, 2 * max(int(levels), 0)), dtype=np.float64)
        self._check(self._lib.sdpgpu_batch_fit_ss(self._b, int(levels), _dp(out) if out.size else None))
        return out

    def _rule(self, levels, ss):
        if ss is None:
            return None, None
        arr = np.ascontiguousarray(ss, dtype=np.float64)
        if arr.shape != (self.n, self.T, 2 * int(levels)):
            raise ValueError(f"ss of shape {arr.shape}: expected [{self.n}, {self.T}, {2 * int(levels)}] for {levels} level(s)")
        return arr, _dp(arr)

    def simulate_ss(self, levels: int, demands, ss=None, ini_x=None, want_sums: bool = False):
        """Roll a level rule of every instance along given demand paths (SimulateFitsS.simulateSinglesS / TwosS / ThreesS);
        `demands` as for simulate(); ss: [n, T, 2 * levels], or None = fit on the device first (needs a solve)."""
        dem = np.ascontiguousarray(demands, dtype=np.float64)
        if dem.ndim == 2 and dem.shape[1] == self.T:
            n_paths, stride = dem.shape[0], 0
        elif dem.ndim == 3 and dem.shape[0] == self.n and dem.shape[2] == self.T:
            n_paths, stride = dem.shape[1], dem.shape[1] * self.T
        else:
            raise ValueError(f"demands of shape {dem.shape}: expected [n_paths, {self.T}] or [{self.n}, n_paths, {self.T}]")
        rule, rule_p = self._rule(levels, ss)
        ini, ini_p = self._ini(ini_x)
        mean = np.empty(self.n, dtype=np.float64)
        sums = np.empty((self.n, n_paths), dtype=np.float64) if want_sums else None
        self._check(self._lib.sdpgpu_batch_simulate_ss(self._b, int(levels), rule_p, n_paths, _dp(dem), stride, ini_p, _dp(mean),
                                                       _dp(sums) if want_sums else None))
        return self._sim_result(mean, sums, want_sums)

    def simulate_ss_sampled(self, levels: int, n_paths: int, seed: int, ss=None, ini_x=None, want_sums: bool = False):
        """Draw the demand paths of simulate_sampled(n_paths, seed) -- the same ones -- and roll a level rule along them."""
        rule, rule_p = self._rule(levels, ss)
        ini, ini_p = self._ini(ini_x)
        mean = np.empty(self.n, dtype=np.float64)
        sums = np.empty((self.n, int(n_paths)), dtype=np.float64) if want_sums and n_paths > 0 else None
        self._check(self._lib.sdpgpu_batch_simulate_ss_sampled(self._b, int(levels), rule_p, int(n_paths), C.c_uint64(seed & (2**64 - 1)),
                                                               ini_p, _dp(mean), _dp(sums) if sums is not None else None))
        return self._sim_result(mean, sums, want_sums)

    # ---- structure checks (sdpgpu_batch_gy / _check_convexity; CheckKConvexity.java, CLSPforDraw.java:147-170) ----
    def gy(self, i: int, period: int) -> np.ndarray:
        """G_period(y) of instance i over its grid: the cost of standing at level y (CLSPforDraw's second Recursion for any
        period), computed for all instances on the device at the first request after a solve."""
        out = np.empty(self.num_states_of(i), dtype=np.float64)
        self._check(self._lib.sdpgpu_batch_gy(self._b, i, period, _dp(out), len(out)))
        return out

    def _per_instance(self, v, dtype):
        """A scalar for all instances or one value each -> a contiguous [n] array (None stays None: the library's default)."""
        return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (self.n,)))

    def check_convexity(self, kind: int, source="values", period: int = 1, x_lo=None, x_hi=None, K=None, capacity=None) -> np.ndarray:
        """CheckKConvexity.check (kind 0) or checkCK (kind 1) on one row of EVERY instance, in one kernel launch: the rows
        V_period (source "values") or G_period ("gy"), over the inventory window x_lo .. x_hi (scalars or one per instance;
        None = the whole grid), with K (None = each instance's fixed ordering cost) and capacity (None = its order limit).
        Returns a structured array [n] with the fields holds, i0, i1, i2, lhs, rhs of sdpgpu_convexity."""
        from .structure import CONVEXITY_DTYPE
        src = {"values": 0, "gy": 1}.get(source, source)
        if not isinstance(src, (int, np.integer)):
            raise ValueError(f"source {source!r}: 'values' or 'gy'")
        if (x_lo is None) != (x_hi is None):
            raise ValueError("x_lo and x_hi are given together, or neither")
        lo, hi = self._per_instance(x_lo, np.float64), self._per_instance(x_hi, np.float64)
        k, cap = self._per_instance(K, np.float64), self._per_instance(capacity, np.int32)
        out = np.zeros(self.n, dtype=CONVEXITY_DTYPE)
        assert out.itemsize == C.sizeof(SdpgpuConvexity)
        self._check(self._lib.sdpgpu_batch_check_convexity(
            self._b, int(kind), int(src), int(period), _dp(lo) if lo is not None else None, _dp(hi) if hi is not None else None,
            _dp(k) if k is not None else None, _ip(cap) if cap is not None else None, out.ctypes.data_as(C.POINTER(SdpgpuConvexity))))
        return out


class StaffBatch(_Batch):
    """N workforce (STAFF family) instances of ONE shape in the separable mode -- the sweep of WorkforceTesting.main
    (WorkforceTesting.java:36-41): period t of all instances in two kernel launches, every instance's tables bit for bit
    those of its own separable handle (SdpEngine with kernel = KERNEL_SEPARABLE).

    descs      one STAFF descriptor per instance, kernel = KERNEL_SEPARABLE (StaffFunctor.to_desc)
    tables     the pool of level tables: a list of (prob[rows, stride], row_len | None)
    use        use[i][t] = id of the pool table period index t of instance i integrates over
    min_staff  min_staff[i][t] = minStaffNum[t] of instance i"""

    def __init__(self, descs: Sequence[SdpgpuDesc], tables, use, min_staff, device: int = -1):
        self._lib = _abi.load()
        self._b = C.c_void_p()
        descs = list(descs)
        if len(use) != len(descs) or len(min_staff) != len(descs):
            raise ValueError(f"{len(descs)} descriptors but {len(use)} rows of table ids and {len(min_staff)} of minStaffNum")
        arr = (SdpgpuDesc * max(len(descs), 1))()
        for i, d in enumerate(descs):
            C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(SdpgpuDesc))
            if device >= 0:
                arr[i].device = device
        self.n = len(descs)
        rc = self._lib.sdpgpu_batch_create(arr, self.n, C.byref(self._b))
        if rc:
            raise SdpgpuError(rc, self._lib.sdpgpu_batch_last_error(None).decode())
        self.T = int(arr[0].periods)
        try:
            self.table_ids = []
            for prob, row_len in tables:
                prob = np.ascontiguousarray(prob, dtype=np.float64)
                if prob.ndim != 2:
                    raise ValueError(f"a level table is [rows, stride], got shape {prob.shape}")
                lens = None if row_len is None else np.ascontiguousarray(row_len, dtype=np.int32)
                if lens is not None and lens.shape != (prob.shape[0],):
                    raise ValueError(f"row_len of shape {lens.shape} for a table of {prob.shape[0]} rows")
                tid = C.c_int32(-1)
                self._check(self._lib.sdpgpu_batch_add_level_pmf(self._b, _dp(prob), _ip(lens) if lens is not None else None,
                                                                 prob.shape[0], prob.shape[1], C.byref(tid)))
                self.table_ids.append(int(tid.value))
            for i in range(self.n):
                if len(use[i]) != self.T or len(min_staff[i]) != self.T:
                    raise ValueError(f"instance {i}: {len(use[i])} table ids and {len(min_staff[i])} minStaffNum for {self.T} periods")
                row = [int(k) for k in use[i]]
                if len(set(row)) == 1:
                    self._check(self._lib.sdpgpu_batch_use_level_pmf(self._b, i, -1, self.table_ids[row[0]]))
                else:
                    for t, k in enumerate(row):
                        self._check(self._lib.sdpgpu_batch_use_level_pmf(self._b, i, t, self.table_ids[k]))
                for t, m in enumerate(min_staff[i]):
                    self._check(self._lib.sdpgpu_batch_set_overhead(self._b, i, t, float(m)))
        except Exception:
            self.close()
            raise

    def grid(self, i: int, period: int):
        """(x_lo, nx): staff number of state index 0 and the number of states of instance i in `period` (1-based)."""
        x_lo, nx = C.c_double(), C.c_int64()
        self._check(self._lib.sdpgpu_batch_grid(self._b, i, period, C.byref(x_lo), C.byref(nx)))
        return float(x_lo.value), int(nx.value)

    def plan(self, period: int) -> SdpgpuBatchStaffPlan:
        """The two launches of one period (1-based) for the whole batch: host arithmetic, no device needed."""
        pl = SdpgpuBatchStaffPlan()
        self._check(self._lib.sdpgpu_batch_staff_plan_period(self._b, period, C.byref(pl)))
        return pl

    def values(self, i: int, period: int) -> np.ndarray:
        out = np.empty(self.grid(i, period)[1], dtype=np.float64)
        self._check(self._lib.sdpgpu_batch_values(self._b, i, period, _dp(out), len(out)))
        return out

    def policy(self, i: int, period: int) -> np.ndarray:
        """Arg-min hire count of every state of the period."""
        out = np.empty(self.grid(i, period)[1], dtype=np.int32)
        self._check(self._lib.sdpgpu_batch_policy(self._b, i, period, _ip(out), len(out)))
        return out

    # ---- fit and rollout of every instance (sdpgpu_batch_staff_reachable / _fit_ss / _simulate; WorkforceTesting.java:112-165) ----
    def reachable(self, i: int, period: int):
        """(L, H): the staff numbers of `period` (1-based) StaffRecursion.getExpectedValue visits from (1, iniStaffNum) of
        instance i -- one interval, the rows of getOptTable.  Host arithmetic, no device."""
        lo, hi = C.c_int64(), C.c_int64()
        self._check(self._lib.sdpgpu_batch_staff_reachable(self._b, i, period, C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def fit_ss(self, max_order_quantity: float) -> np.ndarray:
        """FitsS(max_order_quantity, T).getSinglesS of every instance, fitted ON the device from the solved policy tables:
        [n, T, 2] = (s, S) per period.  The limit is the caller's (the drivers pass Integer.MAX_VALUE), not the hire limit."""
        out = np.empty((self.n, self.T, 2), dtype=np.float64)
        self._check(self._lib.sdpgpu_batch_staff_fit_ss(self._b, float(max_order_quantity), _dp(out)))
        return out

    # ---- structure rows (sdpgpu_batch_staff_gy / _check_convexity; WorkforcePlanning.java:165-211) ----
    def staff_gy(self, i: int, period: int, y_lo: int, y_hi: int) -> np.ndarray:
        """G_period(y) of instance i for the levels y_lo .. y_hi, both ends included: SdpEngine.staff_gy of a separable handle
        of the instance, bit for bit.  The rows of ALL instances and periods are formed in one launch at the first request
        after a solve and kept on the device until the next solve."""
        n = int(y_hi) - int(y_lo) + 1
        out = np.empty(max(n, 0), dtype=np.float64)
        self._check(self._lib.sdpgpu_batch_staff_gy(self._b, int(i), int(period), int(y_lo), n, _dp(out)))
        return out

    def staff_check_convexity(self, kind: int, source="gy", period: int = 1, lo=None, hi=None, K=None, capacity=None) -> np.ndarray:
        """CheckKConvexity.check (kind 0) or checkCK (kind 1) on one row of EVERY instance in one launch: the rows V_period
        (source "values", over the staff numbers lo .. hi) or G_period ("gy", over the levels lo .. hi); lo / hi scalars or one
        per instance, None = the whole row; K None = each instance's fixed hiring cost, capacity None = its hire limit.
        Returns a structured array [n] with the fields of sdpgpu_convexity."""
        from .structure import CONVEXITY_DTYPE
        src = {"values": 0, "gy": 1}.get(source, source)
        if not isinstance(src, (int, np.integer)):
            raise ValueError(f"source {source!r}: 'values' or 'gy'")
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi are given together, or neither")

        def per_instance(v, dtype):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (self.n,)))

        a, c = per_instance(lo, np.int32), per_instance(hi, np.int32)
        k, cap = per_instance(K, np.float64), per_instance(capacity, np.int32)
        out = np.zeros(self.n, dtype=CONVEXITY_DTYPE)
        self._check(self._lib.sdpgpu_batch_staff_check_convexity(
            self._b, int(kind), int(src), int(period), None if a is None else _ip(a), None if c is None else _ip(c),
            None if k is None else _dp(k), None if cap is None else _ip(cap), out.ctypes.data_as(C.POINTER(SdpgpuConvexity))))
        return out

    def staff_simulate(self, sample_nums, seed: int, ini_x: int, ss=None, want_sums: bool = False, want_demands: bool = False):
        """SdpEngine.staff_simulate for every instance in one rollout launch (sdpgpu_batch_staff_simulate; DESIGN 4, "Workforce
        batch: fit and rollout").  ss = None: every instance's own policy table (one rule), else (s, S) levels of shape
        (n, T, 2) or (n, R, T, 2).  Returns the SdpgpuSimResults as a nested list [n][R]; with want_sums also
        (sums[n, R, N], valid[n, R, N]); with want_demands also the turnovers drawn, demands[n, R, N, T] (int32)."""
        k = np.ascontiguousarray(sample_nums, dtype=np.int32)
        if k.shape != (self.T,):
            raise ValueError("sample_nums must have one entry per period")
        levels, n_rules = None, 1
        if ss is not None:
            levels = np.asarray(ss, dtype=np.float64)
            if levels.ndim == 3:
                levels = levels[:, None]
            if levels.ndim != 4 or levels.shape[0] != self.n or levels.shape[2:] != (self.T, 2):
                raise ValueError(f"ss must have shape ({self.n}, {self.T}, 2) or ({self.n}, rules, {self.T}, 2)")
            levels = np.ascontiguousarray(levels)
            n_rules = levels.shape[1]
        n = 1
        for v in k.tolist():  # (the library refuses a bad tree; the buffers below only need a size)
            n *= max(int(v), 1)
        n = min(n, 1 << 24)
        rows = min(max(n_rules, 1), 64)
        if self.n * rows * n > 1 << 28:  # (refused by the library: no buffers for it)
            n = 1
        res = (_abi.SdpgpuSimResult * (self.n * max(n_rules, 1)))()
        sums = np.empty((self.n, rows, n), dtype=np.float64) if want_sums else None
        valid = np.empty((self.n, rows, n), dtype=np.uint8) if want_sums else None
        dem = np.empty((self.n, rows, n, self.T), dtype=np.int32) if want_demands else None
        self._check(self._lib.sdpgpu_batch_staff_simulate(
            self._b, _ip(k), C.c_uint64(int(seed) & (2**64 - 1)), float(ini_x), None if levels is None else _dp(levels), n_rules, res,
            None if sums is None else _dp(sums), None if valid is None else valid.ctypes.data_as(C.POINTER(C.c_uint8)),
            None if dem is None else _ip(dem)))
        flat = list(res)
        out = [[flat[i * n_rules:(i + 1) * n_rules] for i in range(self.n)]]
        if want_sums:
            out += [sums, valid.astype(bool)]
        if want_demands:
            out.append(dem)
        return out[0] if len(out) == 1 else tuple(out)
