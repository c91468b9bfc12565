"""Thin object wrapper over one sdpgpu_handle (include/sdpgpu.h).

`pmf` follows the reference's `double[][][] pmf` (Recursion.java:38): pmf[t][j] = [demand, prob].
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._abi import SdpgpuDesc, SdpgpuError, SdpgpuStats


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def split_pmf(pmf):
    """pmf[t][j] = (demand, prob) -> list of (demand array, prob array) per period."""
    out = []
    for tile in pmf:
        arr = np.asarray(tile, dtype=np.float64)
        if arr.ndim != 2 or arr.shape[1] != 2 or arr.shape[0] < 1:
            raise ValueError("pmf[t] must be an array of [demand, prob] pairs")
        out.append((np.ascontiguousarray(arr[:, 0]), np.ascontiguousarray(arr[:, 1])))
    return out


class SdpEngine:
    """One backward-recursion problem on one GPU (or one rank's state slab of it)."""

    def __init__(self, desc: SdpgpuDesc, pmf, overhead: Optional[Sequence[float]] = None,
                 custom_source: Optional[str] = None, custom_params: Optional[Sequence[float]] = None,
                 level_pmf=None, level_row_len=None):
        """custom_source: HIP device text of the three lambdas (see sdpgpu_create_custom in include/sdpgpu.h),
        custom_params: the doubles they read through `c.params`.
        level_pmf (STAFF family, instead of pmf): array (T, rows, stride), level_pmf[t, y, j] = P(turnover j | level y);
        level_row_len: entries per row (default y + 1).  `overhead` then carries minStaffNum[t]."""
        self._lib = _abi.load()
        self._h = C.c_void_p()
        self.desc = desc
        staff = desc.family == _abi.FAMILY_STAFF
        if staff:
            if level_pmf is None:
                raise ValueError("the STAFF family needs level_pmf")
            level_pmf = np.ascontiguousarray(level_pmf, dtype=np.float64)
            if level_pmf.ndim != 3 or level_pmf.shape[0] != desc.periods:
                raise ValueError("level_pmf must have shape (periods, rows, stride)")
            if level_row_len is not None:
                level_row_len = np.ascontiguousarray(level_row_len, dtype=np.int32)
                if level_row_len.shape != (level_pmf.shape[1],):
                    raise ValueError("level_row_len must have one entry per row")
        tiles = [] if staff else split_pmf(pmf)
        if not staff and len(tiles) != desc.periods:
            raise ValueError(f"pmf has {len(tiles)} periods, descriptor says {desc.periods}")
        if custom_source is None:
            rc = self._lib.sdpgpu_create(C.byref(desc), C.byref(self._h))
        else:
            prm = np.ascontiguousarray(custom_params if custom_params is not None else [], dtype=np.float64)
            rc = self._lib.sdpgpu_create_custom(C.byref(desc), custom_source.encode(), _dp(prm) if len(prm) else None,
                                                len(prm), C.byref(self._h))
        if rc:
            raise SdpgpuError(rc, self._lib.sdpgpu_last_error(None).decode())
        try:
            for t, (d, p) in enumerate(tiles):
                self._check(self._lib.sdpgpu_set_pmf(self._h, t, _dp(d), _dp(p), len(d)))
            if staff:
                for t in range(desc.periods):
                    self._check(self._lib.sdpgpu_set_level_pmf(
                        self._h, t, _dp(level_pmf[t]), None if level_row_len is None else _ip(level_row_len),
                        level_pmf.shape[1], level_pmf.shape[2]))
            if overhead is not None:
                for t, oh in enumerate(overhead):
                    self._check(self._lib.sdpgpu_set_overhead(self._h, t, float(oh)))
        except Exception:
            self.close()
            raise
        self.T = desc.periods

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc:
            raise SdpgpuError(rc, self._lib.sdpgpu_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.sdpgpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- geometry ---------------------------------------------------------------------------
    def num_states(self, period: int) -> int:
        n = self._lib.sdpgpu_num_states(self._h, period)
        if n < 0:
            raise SdpgpuError(2, self._lib.sdpgpu_last_error(self._h).decode() or "layout not available")
        return int(n)

    def slab(self, period: int):
        pad, lo, hi = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.sdpgpu_slab(self._h, period, C.byref(pad), C.byref(lo), C.byref(hi)))
        return pad.value, lo.value, hi.value

    def grid(self, period: int):
        x_lo = C.c_double()
        nx, nc, nq = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.sdpgpu_grid(self._h, period, C.byref(x_lo), C.byref(nx), C.byref(nc), C.byref(nq)))
        return x_lo.value, nx.value, nc.value, nq.value

    def grid2(self, period: int):
        """(x_lo, nx, nc, nq1, nq2): the pipeline axis split in two (lead_time 2), nq2 = 1 otherwise."""
        x_lo = C.c_double()
        nx, nc, q1, q2 = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.sdpgpu_grid2(self._h, period, C.byref(x_lo), C.byref(nx), C.byref(nc), C.byref(q1),
                                           C.byref(q2)))
        return x_lo.value, nx.value, nc.value, q1.value, q2.value

    def cash_value(self, ic: int) -> float:
        return float(self._lib.sdpgpu_cash_value(self._h, ic))

    def state_index(self, period: int, x: float, cash: float = 0.0, preq: float = 0.0, preq2: float = 0.0) -> int:
        return int(self._lib.sdpgpu_state_index2(self._h, period, float(x), float(cash), float(preq), float(preq2)))

    # -- execution --------------------------------------------------------------------------
    def set_action_counts(self, t: int, counts):
        """The caller's own action-list lengths of every grid state of period t+1 (sdpgpu_set_action_counts)."""
        c = np.ascontiguousarray(counts, dtype=np.int32)
        self._check(self._lib.sdpgpu_set_action_counts(self._h, t, _ip(c), len(c)))

    def set_stream(self, hip_stream: int):
        self._check(self._lib.sdpgpu_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_profiling(self, on: bool):
        self._check(self._lib.sdpgpu_set_profiling(self._h, 1 if on else 0))

    def solve(self, sync: bool = True):
        self._check(self._lib.sdpgpu_solve(self._h, 1 if sync else 0))

    def run_period(self, period: int):
        self._check(self._lib.sdpgpu_run_period(self._h, period))

    def keys_bytes(self) -> int:
        return int(self._lib.sdpgpu_keys_bytes(self._h))

    def attach_keys(self, device_ptr: int, nbytes: int):
        self._check(self._lib.sdpgpu_attach_keys(self._h, C.c_void_p(device_ptr), nbytes))

    def exchange_ptr(self, period: int) -> int:
        p = self._lib.sdpgpu_exchange_ptr(self._h, period)
        if not p:
            raise SdpgpuError(3, self._lib.sdpgpu_last_error(self._h).decode() or "no exchange table")
        return int(p)

    def finalize(self):
        """Enqueue the deferred read-out of every period run so far (no host wait)."""
        self._check(self._lib.sdpgpu_finalize(self._h))

    def footprint(self, period: int):
        """(left, right): state i of `period` reads V_{period+1}[i - left .. i + right]; None if unbounded."""
        l, r = C.c_int64(), C.c_int64()
        rc = self._lib.sdpgpu_footprint(self._h, period, C.byref(l), C.byref(r))
        if rc == 4:
            return None
        self._check(rc)
        return l.value, r.value

    def plan(self, period: int):
        """sdpgpu_plan_period: the launch plan of `period` (host arithmetic only; raises SdpgpuError when the plan -- e.g.
        one forced through SDPGPU_WIN_R / _S / _NCH -- cannot run)."""
        from ._abi import SdpgpuPlan
        out = SdpgpuPlan()
        self._check(self._lib.sdpgpu_plan_period(self._h, period, C.byref(out)))
        return out

    def set_halo(self, halo: int):
        self._check(self._lib.sdpgpu_set_halo(self._h, int(halo)))

    def run_period_range(self, period: int, lo: int, hi: int):
        self._check(self._lib.sdpgpu_run_period_range(self._h, period, int(lo), int(hi)))

    def run_period_part(self, period: int, part: int):
        self._check(self._lib.sdpgpu_run_period_part(self._h, period, part))

    # -- multi-GPU through the C ABI (csrc/sdpgpu_comm.hip) -------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId: ONE rank calls this and hands the 128 bytes to the others."""
        lib = _abi.load()
        _abi.share_rccl_with_torch()
        buf = C.create_string_buffer(_abi.UNIQUE_ID_BYTES)
        rc = lib.sdpgpu_comm_unique_id(buf)
        if rc:
            raise SdpgpuError(rc, lib.sdpgpu_last_error(None).decode())
        return buf.raw

    def comm_prepare(self):
        """sdpgpu_comm_prepare: what can fail on this rank ALONE (device tables, RCCL load) -- before the ranks agree to
        enter the collective comm_init."""
        _abi.share_rccl_with_torch()
        self._check(self._lib.sdpgpu_comm_prepare(self._h))

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        """Collective over the world's ranks (ncclCommInitRank on this handle's device)."""
        if len(unique_id) != _abi.UNIQUE_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        _abi.share_rccl_with_torch()
        self._check(self._lib.sdpgpu_comm_init(self._h, C.c_char_p(unique_id), rank, world))

    def comm_destroy(self):
        self._check(self._lib.sdpgpu_comm_destroy(self._h))

    def exchange(self, period: int):
        """All-gather of the row of `period` on the handle's stream (needs comm_init)."""
        self._check(self._lib.sdpgpu_exchange(self._h, period))

    def solve_sharded(self, overlap: bool = False, sync: bool = True, gather_first: bool = False):
        """This rank's whole sweep with the per-period all-gathers in between; every rank calls it."""
        flags = (_abi.SHARDED_SYNC if sync else 0) | (_abi.SHARDED_OVERLAP if overlap else 0) | \
                (_abi.SHARDED_GATHER_FIRST if gather_first else 0)
        self._check(self._lib.sdpgpu_solve_sharded(self._h, flags))

    @staticmethod
    def solve_multi(engines, sync: bool = True, gather_first: bool = False, threads: bool = False):
        """One process driving every rank: engines[r] is rank r of len(engines) (sdpgpu_solve_multi).  threads: one host
        thread per rank inside the library (SDPGPU_SHARDED_THREADS) instead of one thread issuing for all."""
        lib = _abi.load()
        _abi.share_rccl_with_torch()
        arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
        flags = (_abi.SHARDED_SYNC if sync else 0) | (_abi.SHARDED_GATHER_FIRST if gather_first else 0) | \
                (_abi.SHARDED_THREADS if threads else 0)
        rc = lib.sdpgpu_solve_multi(arr, len(engines), flags)
        if rc:
            raise SdpgpuError(rc, lib.sdpgpu_last_error(engines[0]._h).decode())

    def synchronize(self):
        self._check(self._lib.sdpgpu_synchronize(self._h))

    def values_bytes(self) -> int:
        return int(self._lib.sdpgpu_values_bytes(self._h))

    def attach_values(self, device_ptr: int, nbytes: int):
        self._check(self._lib.sdpgpu_attach_values(self._h, C.c_void_p(device_ptr), nbytes))

    def values_device_ptr(self, period: int) -> int:
        p = self._lib.sdpgpu_values_device_ptr(self._h, period)
        if not p:
            raise SdpgpuError(3, self._lib.sdpgpu_last_error(self._h).decode() or "no device table")
        return int(p)

    # -- results ----------------------------------------------------------------------------
    def values(self, period: int) -> np.ndarray:
        n = self.num_states(period)
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.sdpgpu_values(self._h, period, _dp(out), n))
        return out

    def policy(self, period: int) -> np.ndarray:
        """Arg-opt action INDEX of this rank's slab (action = index * step)."""
        _, lo, hi = self.slab(period)
        out = np.empty(hi - lo, dtype=np.int32)
        self._check(self._lib.sdpgpu_policy(self._h, period, _ip(out), lo, hi - lo))
        return out

    def eval_states(self, period: int, x, cash=None, preq=None, preq2=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = len(x)
        cash_a = None if cash is None else np.ascontiguousarray(cash, dtype=np.float64)
        preq_a = None if preq is None else np.ascontiguousarray(preq, dtype=np.float64)
        preq2_a = None if preq2 is None else np.ascontiguousarray(preq2, dtype=np.float64)
        val = np.empty(n, dtype=np.float64)
        act = np.empty(n, dtype=np.int32)
        self._check(
            self._lib.sdpgpu_eval_states2(
                self._h, period, n, _dp(x), None if cash_a is None else _dp(cash_a),
                None if preq_a is None else _dp(preq_a), None if preq2_a is None else _dp(preq2_a), _dp(val),
                _ip(act)))
        return val, act

    def reachable(self, period: int) -> np.ndarray:
        n = self.num_states(period)
        out = np.empty(n, dtype=np.uint8)
        self._check(self._lib.sdpgpu_reachable(self._h, period, out.ctypes.data_as(C.POINTER(C.c_uint8)), n))
        return out.astype(bool)

    def simulate(self, demand, discount, ini_x: float, ini_cash: float = 0.0, ini_preq: float = 0.0):
        """Roll the policy along demand paths: demand[n][T] (rounded), discount[T] -> (sums[n], valid[n])."""
        dem = np.ascontiguousarray(demand, dtype=np.float64)
        if dem.ndim != 2 or dem.shape[1] != self.T:
            raise ValueError(f"demand must be [n_paths][{self.T}]")
        disc = np.ascontiguousarray(discount, dtype=np.float64)
        if disc.shape != (self.T,):
            raise ValueError("discount must have one entry per period")
        n = dem.shape[0]
        out = np.empty(n, dtype=np.float64)
        valid = np.empty(n, dtype=np.uint8)
        self._check(self._lib.sdpgpu_simulate(self._h, n, _dp(dem), _dp(disc), float(ini_x), float(ini_cash),
                                              float(ini_preq), _dp(out), valid.ctypes.data_as(C.POINTER(C.c_uint8))))
        self.last_sim_flags = valid  # bit 0: path stayed on the grid; bit 1 (family SURVIVAL): a demand was lost
        return out, (valid & 1).astype(bool)

    def set_sampler(self, t: int, dist=None):
        """Distribution the device sampler draws period index `t` from: None = the handle's own pmf tile of that period (the
        default; any step, gaps allowed), a pmf.py distribution, an SdpgpuDistSpec, or a (kind, a, b) tuple (step 1 only)."""
        if dist is None:
            self._check(self._lib.sdpgpu_set_sampler(self._h, int(t), None))
            return
        from .pmf import dist_spec
        spec = dist_spec(dist)
        self._check(self._lib.sdpgpu_set_sampler(self._h, int(t), C.byref(spec)))

    @staticmethod
    def _sample_mode(mode) -> int:
        if mode in ("lhs", _abi.SAMPLE_LHS):
            return _abi.SAMPLE_LHS
        if mode in ("random", _abi.SAMPLE_RANDOM):
            return _abi.SAMPLE_RANDOM
        raise ValueError(f"mode {mode!r}: 'lhs' or 'random'")

    def simulate_sampled(self, n_paths: int, seed: int, ini_x: float, ini_cash: float = 0.0, ini_preq: float = 0.0, *,
                         mode="lhs", first_path: int = 0, discount=None, want_sums: bool = False):
        """Draw n_paths demand paths ON the device (latin hypercube or plain random, seeded), roll the policy along
        them and reduce there, in one call.  Returns the SdpgpuSimResult (n_paths, n_valid, n_lost, mean, m2, kernel_ms);
        with want_sums also (sums[n], flags[n]) -- bit 0 of a flag: the path stayed on the grid, bit 1 (SURVIVAL): a demand
        was lost."""
        disc = None
        if discount is not None:
            disc = np.ascontiguousarray(discount, dtype=np.float64)
            if disc.shape != (self.T,):
                raise ValueError("discount must have one entry per period")
        n = int(n_paths)
        res = _abi.SdpgpuSimResult()
        sums = np.empty(max(n, 0), dtype=np.float64) if want_sums else None
        flags = np.empty(max(n, 0), dtype=np.uint8) if want_sums else None
        self._check(self._lib.sdpgpu_simulate_sampled(
            self._h, n, C.c_uint64(int(seed) & (2**64 - 1)), self._sample_mode(mode), C.c_uint64(int(first_path) & (2**64 - 1)),
            None if disc is None else _dp(disc), float(ini_x), float(ini_cash), float(ini_preq), C.byref(res),
            None if sums is None else _dp(sums), None if flags is None else flags.ctypes.data_as(C.POINTER(C.c_uint8))))
        if want_sums:
            self.last_sim_flags = flags
            return res, sums, flags
        return res

    def sample_demands(self, n_paths: int, seed: int, *, mode="lhs", first_path: int = 0):
        """(demands[n_paths, T], uniforms[n_paths, T]) simulate_sampled uses, from the same device code.  Needs no solve."""
        n = max(int(n_paths), 0)
        dem = np.empty((n, self.T), dtype=np.float64)
        u = np.empty_like(dem)
        self._check(self._lib.sdpgpu_sample_demands(self._h, int(n_paths), C.c_uint64(int(seed) & (2**64 - 1)), self._sample_mode(mode),
                                                    C.c_uint64(int(first_path) & (2**64 - 1)), _dp(dem), _dp(u)))
        return dem, u

    def staff_simulate(self, sample_nums, seed: int, ini_x: int, ss=None, *, want_sums: bool = False, want_demands: bool = False):
        """STAFF family: roll hiring rules out on a sampled tree (sdpgpu_staff_simulate; DESIGN 4, "Workforce rollout on a
        sampled tree").  sample_nums[t] children per node of depth t; ss = None: the computed policy table (one rule), else
        (s, S) levels of shape (T, 2) or (R, T, 2).  Returns the list of SdpgpuSimResult, one per rule; with want_sums also
        (sums[R, N], valid[R, N]); with want_demands also the turnovers drawn, demands[R, N, T] (int32)."""
        k = np.ascontiguousarray(sample_nums, dtype=np.int32)
        if k.shape != (self.T,):
            raise ValueError("sample_nums must have one entry per period")
        levels, n_rules = None, 1
        if ss is not None:
            levels = np.ascontiguousarray(ss, dtype=np.float64)
            if levels.ndim == 2:
                levels = levels[None]
            if levels.ndim != 3 or levels.shape[1:] != (self.T, 2):
                raise ValueError(f"ss must have shape ({self.T}, 2) or (rules, {self.T}, 2)")
            n_rules = levels.shape[0]
        n = 1
        for v in k.tolist():  # (the library refuses a bad tree; the buffers below only need a size)
            n *= max(int(v), 1)
        n = min(n, 1 << 24)
        rows = min(max(n_rules, 1), 64)
        res = (_abi.SdpgpuSimResult * max(n_rules, 1))()
        sums = np.empty((rows, n), dtype=np.float64) if want_sums else None
        valid = np.empty((rows, n), dtype=np.uint8) if want_sums else None
        dem = np.empty((rows, n, self.T), dtype=np.int32) if want_demands else None
        self._check(self._lib.sdpgpu_staff_simulate(
            self._h, _ip(k), C.c_uint64(int(seed) & (2**64 - 1)), float(ini_x), None if levels is None else _dp(levels), n_rules, res,
            None if sums is None else _dp(sums), None if valid is None else valid.ctypes.data_as(C.POINTER(C.c_uint8)),
            None if dem is None else _ip(dem)))
        out = [list(res)]
        if want_sums:
            out += [sums, valid.astype(bool)]
        if want_demands:
            out.append(dem)
        return out[0] if len(out) == 1 else tuple(out)

    def rule_table_points(self) -> int:
        """NX of the threshold tables of cash_rule_simulate: the descriptor's inventory points, entry ix keyed by
        min_inventory + ix * step."""
        d = self.desc
        return int((d.max_inventory - d.min_inventory) / d.step) + 1

    def cash_rule_simulate(self, n_paths: int, seed: int, ini_x: float, ini_cash: float, forms, rules, *, min_cash_required: float,
                           max_q: float, fix_order_cost: float, vari_cost: float, c1_tab=None, c2_tab=None, mode="lhs",
                           first_path: int = 0, discount=None, want_sums: bool = False):
        """CASH family: roll (s, C, S) ordering rules out along demand paths drawn on the device (sdpgpu_cash_rule_simulate;
        DESIGN 4, "Cash rule rollout").  forms: one of _abi.RULE_SC12S / RULE_SC1S / RULE_SMEANCS per rule; rules: (s, c1, c2, S)
        rows of shape (T, 4) or (R, T, 4); c1_tab / c2_tab: None or dense threshold tables (R, T, NX), NX = rule_table_points(),
        NaN = key absent.  Needs no solve.  Returns the list of SdpgpuSimResult, one per rule; with want_sums also sums[R, n]."""
        rows = np.ascontiguousarray(rules, dtype=np.float64)
        if rows.ndim == 2:
            rows = rows[None]
        if rows.ndim != 3 or rows.shape[1:] != (self.T, 4):
            raise ValueError(f"rules must have shape ({self.T}, 4) or (rules, {self.T}, 4)")
        n_rules = rows.shape[0]
        fm = np.ascontiguousarray(np.atleast_1d(forms), dtype=np.int32)
        if fm.shape != (n_rules,):
            raise ValueError(f"forms must have one entry per rule ({n_rules})")
        nx = self.rule_table_points()
        tabs = []
        for name, tab in (("c1_tab", c1_tab), ("c2_tab", c2_tab)):
            if tab is not None:
                tab = np.ascontiguousarray(tab, dtype=np.float64)
                if tab.ndim == 2:
                    tab = tab[None]
                if tab.shape != (n_rules, self.T, nx):
                    raise ValueError(f"{name} must have shape ({n_rules}, {self.T}, {nx})")
            tabs.append(tab)
        disc = None
        if discount is not None:
            disc = np.ascontiguousarray(discount, dtype=np.float64)
            if disc.shape != (self.T,):
                raise ValueError("discount must have one entry per period")
        n = min(max(int(n_paths), 0), 1 << 24)  # (the library refuses a bad count; the buffer below only needs a size)
        res = (_abi.SdpgpuSimResult * max(n_rules, 1))()
        sums = np.empty((min(max(n_rules, 1), 16), n), dtype=np.float64) if want_sums else None
        self._check(self._lib.sdpgpu_cash_rule_simulate(
            self._h, int(n_paths), C.c_uint64(int(seed) & (2**64 - 1)), self._sample_mode(mode), C.c_uint64(int(first_path) & (2**64 - 1)),
            None if disc is None else _dp(disc), float(ini_x), float(ini_cash), n_rules, _ip(fm), _dp(rows),
            None if tabs[0] is None else _dp(tabs[0]), None if tabs[1] is None else _dp(tabs[1]), float(min_cash_required), float(max_q),
            float(fix_order_cost), float(vari_cost), res, None if sums is None else _dp(sums)))
        return (list(res), sums) if want_sums else list(res)

    # -- STAFF family: the G(y) rows and CheckKConvexity on them ("Workforce structure rows") -----------------------
    def staff_gy_range(self, period: int):
        """(y_lo, y_hi): the first run of levels of `period` none of whose successors leaves period + 1's stored staff numbers
        (sdpgpu_staff_gy_range; y_lo > y_hi: none).  Host arithmetic, no device."""
        lo, hi = C.c_int32(), C.c_int32()
        self._check(self._lib.sdpgpu_staff_gy_range(self._h, int(period), C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def staff_gy(self, period: int, y_lo: int = None, y_hi: int = None) -> np.ndarray:
        """G_period(y) for the levels y_lo .. y_hi, both ends included (default: staff_gy_range(period)), of a solved STAFF
        handle in one kernel launch (sdpgpu_staff_gy): the cost of standing at hire-up-to level y, the sum
        WorkforcePlanning.main draws, against the handle's own V_{period+1}."""
        if y_lo is None or y_hi is None:
            r_lo, r_hi = self.staff_gy_range(period)
            y_lo, y_hi = (r_lo if y_lo is None else y_lo), (r_hi if y_hi is None else y_hi)
        n = int(y_hi) - int(y_lo) + 1
        out = np.empty(max(n, 0), dtype=np.float64)
        self._check(self._lib.sdpgpu_staff_gy(self._h, int(period), int(y_lo), n, _dp(out)))
        return out

    def staff_check_convexity(self, kind: int, source="gy", period: int = 1, lo: int = None, hi: int = None, K: float = None,
                              capacity: int = None) -> np.ndarray:
        """CheckKConvexity.check (kind 0) or checkCK (kind 1) on one row of a solved STAFF handle, formed and checked on the
        device (sdpgpu_staff_check_convexity): source "values" = V_period over the staff numbers lo .. hi (default: the
        period's grid), "gy" = G_period over the levels lo .. hi (default: staff_gy_range).  K defaults to the fixed hiring
        cost, capacity to the hire limit.  Returns a structured scalar with the fields of sdpgpu_convexity."""
        from .structure import CONVEXITY_DTYPE
        src = {"values": 0, "gy": 1}.get(source, source)
        if not isinstance(src, (int, np.integer)):
            raise ValueError(f"source {source!r}: 'values' or 'gy'")
        if lo is None or hi is None:
            if src == 0:
                x_lo, nx = self.grid(period)[:2]
                d_lo, d_hi = int(x_lo), int(x_lo) + int(nx) - 1
            else:
                d_lo, d_hi = self.staff_gy_range(period)
            lo, hi = (d_lo if lo is None else lo), (d_hi if hi is None else hi)
        out = np.zeros(1, dtype=CONVEXITY_DTYPE)
        self._check(self._lib.sdpgpu_staff_check_convexity(
            self._h, int(kind), int(src), int(period), int(lo), int(hi), float(self.desc.fixed_order_cost if K is None else K),
            int(self.desc.max_order_quantity if capacity is None else capacity), out.ctypes.data_as(C.POINTER(_abi.SdpgpuConvexity))))
        return out[0]

    def cash_g_table(self, kind: int, period: int, x_lo: float, x_hi: float, cash_lo: float, cash_hi: float) -> np.ndarray:
        """CASH family, formula 1: the table G (kind _abi.CASH_G), GA (CASH_GA) or GB (CASH_GB) of `period` over the window of
        levels x_lo .. x_hi and cash cash_lo .. cash_hi, both ends included (sdpgpu_cash_g_table; DESIGN 4, "Cash structure
        tables").  Returns out[R - cash_lo, y - x_lo], the drivers' resultTable[rowIndex][columnIndex].  Needs a solve."""
        n_x, n_r = int(x_hi - x_lo) + 1, int(cash_hi - cash_lo) + 1
        out = np.empty((max(n_r, 1), max(n_x, 1)), dtype=np.float64)
        self._check(self._lib.sdpgpu_cash_g_table(self._h, int(kind), int(period), float(x_lo), n_x, float(cash_lo), n_r, _dp(out)))
        return out

    def cash_structure(self, mask: int, period: int, x_lo: float, x_hi: float, cash_lo: float, cash_hi: float, *, fix_cost: float = None,
                       vari_cost: float = None, want_tables: bool = True):
        """The derived tables and checks `mask` names (_abi.CSTRUCT_*; cash_structure.mask_of) of the solved handle's G, GA, GB
        and F = V_period over the window, all formed on the device (sdpgpu_cash_structure, source 0).  fix_cost / vari_cost
        default to the descriptor's.  Returns a cash_structure.CashStructure; want_tables=False copies no table back."""
        from . import cash_structure as cs
        return cs.run(mask, source=0, handle=self._h, period=period, x_lo=x_lo, n_x=int(x_hi - x_lo) + 1, n_r=int(cash_hi - cash_lo) + 1,
                      min_cash=cash_lo, fix_cost=self.desc.fixed_order_cost if fix_cost is None else fix_cost,
                      vari_cost=self.desc.unit_order_cost if vari_cost is None else vari_cost, want_tables=want_tables)

    def xr_simulate(self, n_paths: int = None, seed: int = 0, ini_x: float = 0.0, ini_r: float = 0.0, levels=None, *, vari_cost: float = None,
                    demand=None, mode="lhs", first_path: int = 0, discount=None, want_sums: bool = False, want_demands: bool = False):
        """CASH family with cash_formula 2: roll the policy table (levels=None; needs a solve) or Chao's a* levels -- shape
        (T,) or (R, T), no solve needed -- out on the (x, R) state along demand paths (sdpgpu_xr_simulate; DESIGN 4, "(x, R)
        rollout").  The demands are drawn on the device (mode "lhs" / "random", seed, first_path as simulate_sampled) or GIVEN
        as demand[n, T].  vari_cost: the reference's variOrderCost (default: the descriptor's unit cost).  Returns the list of
        SdpgpuSimResult, one per rule; with want_sums also sums[R, n]; with want_demands also the demands[n, T] every rule saw."""
        lv, n_rules = None, 1
        if levels is not None:
            lv = np.ascontiguousarray(levels, dtype=np.float64)
            if lv.ndim == 1:
                lv = lv[None]
            if lv.ndim != 2 or lv.shape[1] != self.T:
                raise ValueError(f"levels must have shape ({self.T},) or (rules, {self.T})")
            n_rules = lv.shape[0]
        given = None
        if demand is not None:
            given = np.ascontiguousarray(demand, dtype=np.float64)
            if given.ndim != 2 or given.shape[1] != self.T:
                raise ValueError(f"demand must have shape (paths, {self.T})")
            if n_paths is not None and int(n_paths) != given.shape[0]:
                raise ValueError(f"n_paths = {n_paths}, demand has {given.shape[0]} paths")
            n_paths = given.shape[0]
        elif n_paths is None:
            raise ValueError("n_paths is needed where no demand is given")
        disc = None
        if discount is not None:
            disc = np.ascontiguousarray(discount, dtype=np.float64)
            if disc.shape != (self.T,):
                raise ValueError("discount must have one entry per period")
        n = min(max(int(n_paths), 0), 1 << 24)  # (the library refuses a bad count; the buffers below only need a size)
        res = (_abi.SdpgpuSimResult * max(n_rules, 1))()
        sums = np.empty((min(max(n_rules, 1), 16), n), dtype=np.float64) if want_sums else None
        dem = np.empty((n, self.T), dtype=np.float64) if want_demands else None
        self._check(self._lib.sdpgpu_xr_simulate(
            self._h, int(n_paths), C.c_uint64(int(seed) & (2**64 - 1)), self._sample_mode(mode), C.c_uint64(int(first_path) & (2**64 - 1)),
            None if given is None else _dp(given), None if disc is None else _dp(disc), float(ini_x), float(ini_r), n_rules,
            None if lv is None else _dp(lv), float(self.desc.unit_order_cost if vari_cost is None else vari_cost), res,
            None if sums is None else _dp(sums), None if dem is None else _dp(dem)))
        out = [list(res)]
        if want_sums:
            out.append(sums)
        if want_demands:
            out.append(dem)
        return out[0] if len(out) == 1 else tuple(out)

    # -- user-functor handles: rollouts of their own ("User-functor rollouts") --------------------------------------
    def _disc_or_none(self, discount):
        if discount is None:
            return None
        disc = np.ascontiguousarray(discount, dtype=np.float64)
        if disc.shape != (self.T,):
            raise ValueError("discount must have one entry per period")
        return disc

    def custom_simulate(self, demand, discount, ini_x: float, ini_cash: float = 0.0, ini_preq: float = 0.0):
        """simulate() for a handle made with custom_source: roll the policy tables through the user's compiled lambdas along
        demand[n][T] with weights discount[T] -> (sums[n], valid[n]) (sdpgpu_custom_simulate)."""
        dem = np.ascontiguousarray(demand, dtype=np.float64)
        if dem.ndim != 2 or dem.shape[1] != self.T:
            raise ValueError(f"demand must be [n_paths][{self.T}]")
        disc = self._disc_or_none(discount)
        n = dem.shape[0]
        out = np.empty(n, dtype=np.float64)
        valid = np.empty(n, dtype=np.uint8)
        self._check(self._lib.sdpgpu_custom_simulate(self._h, n, _dp(dem), None if disc is None else _dp(disc), float(ini_x), float(ini_cash),
                                                     float(ini_preq), _dp(out), valid.ctypes.data_as(C.POINTER(C.c_uint8))))
        self.last_sim_flags = valid
        return out, (valid & 1).astype(bool)

    def custom_simulate_sampled(self, n_paths: int, seed: int, ini_x: float, ini_cash: float = 0.0, ini_preq: float = 0.0, *, mode="lhs",
                                first_path: int = 0, discount=None, want_sums: bool = False, want_demands: bool = False):
        """simulate_sampled() for a handle made with custom_source (sdpgpu_custom_simulate_sampled): the draws of simulate_sampled,
        the rollout through the user's compiled lambdas, the reduction on the device.  Returns the SdpgpuSimResult; with want_sums
        also (sums[n], flags[n]); with want_demands also the demands[n, T] drawn (sample_demands refuses these handles)."""
        disc = self._disc_or_none(discount)
        n = min(max(int(n_paths), 0), 1 << 24)  # (the library refuses a bad count; the buffers below only need a size)
        res = _abi.SdpgpuSimResult()
        sums = np.empty(n, dtype=np.float64) if want_sums else None
        flags = np.empty(n, dtype=np.uint8) if want_sums else None
        dem = np.empty((n, self.T), dtype=np.float64) if want_demands else None
        self._check(self._lib.sdpgpu_custom_simulate_sampled(
            self._h, int(n_paths), C.c_uint64(int(seed) & (2**64 - 1)), self._sample_mode(mode), C.c_uint64(int(first_path) & (2**64 - 1)),
            None if disc is None else _dp(disc), float(ini_x), float(ini_cash), float(ini_preq), C.byref(res),
            None if sums is None else _dp(sums), None if flags is None else flags.ctypes.data_as(C.POINTER(C.c_uint8)),
            None if dem is None else _dp(dem)))
        out = [res]
        if want_sums:
            self.last_sim_flags = flags
            out += [sums, flags]
        if want_demands:
            out.append(dem)
        return out[0] if len(out) == 1 else tuple(out)

    def custom_rule_simulate(self, n_paths: int, seed: int, ini_x: float, ini_cash: float, forms, rules, *, min_cash_required: float = 0.0,
                             max_q: float = 0.0, fix_order_cost: float = 0.0, vari_cost: float = 1.0, mode="lhs", first_path: int = 0,
                             discount=None, want_sums: bool = False, want_demands: bool = False):
        """A handle made with custom_source on the (x, cash) state shape: roll the overdraft drivers' ordering rules out through
        the user's compiled lambdas along demand paths drawn on the device (sdpgpu_custom_rule_simulate).  forms: one of
        _abi.ORULE_SS / ORULE_SCS / ORULE_SCS1S2 per rule; rules: (s, C, S, S2) rows of shape (T, 4) or (R, T, 4).  Needs no solve.
        Returns the list of SdpgpuSimResult, one per rule; with want_sums also sums[R, n]; with want_demands the demands[n, T]."""
        rows = np.ascontiguousarray(rules, dtype=np.float64)
        if rows.ndim == 2:
            rows = rows[None]
        if rows.ndim != 3 or rows.shape[1:] != (self.T, 4):
            raise ValueError(f"rules must have shape ({self.T}, 4) or (rules, {self.T}, 4)")
        n_rules = rows.shape[0]
        fm = np.ascontiguousarray(np.atleast_1d(forms), dtype=np.int32)
        if fm.shape != (n_rules,):
            raise ValueError(f"forms must have one entry per rule ({n_rules})")
        disc = self._disc_or_none(discount)
        n = min(max(int(n_paths), 0), 1 << 24)  # (the library refuses a bad count; the buffers below only need a size)
        res = (_abi.SdpgpuSimResult * max(n_rules, 1))()
        sums = np.empty((min(max(n_rules, 1), 16), n), dtype=np.float64) if want_sums else None
        dem = np.empty((n, self.T), dtype=np.float64) if want_demands else None
        self._check(self._lib.sdpgpu_custom_rule_simulate(
            self._h, int(n_paths), C.c_uint64(int(seed) & (2**64 - 1)), self._sample_mode(mode), C.c_uint64(int(first_path) & (2**64 - 1)),
            None if disc is None else _dp(disc), float(ini_x), float(ini_cash), n_rules, _ip(fm), _dp(rows), float(min_cash_required),
            float(max_q), float(fix_order_cost), float(vari_cost), res, None if sums is None else _dp(sums),
            None if dem is None else _dp(dem)))
        out = [list(res)]
        if want_sums:
            out.append(sums)
        if want_demands:
            out.append(dem)
        return out[0] if len(out) == 1 else tuple(out)

    def stats(self) -> SdpgpuStats:
        st = SdpgpuStats()
        self._check(self._lib.sdpgpu_stats_get(self._h, C.byref(st)))
        return st

    def period_ms(self, period: int) -> float:
        return float(self._lib.sdpgpu_period_ms(self._h, period))

    def f1_screen(self, period: int):
        """The screen of the F1 level kernel in `period` of the last solve: (screen_start, level blocks screened and stopped,
        screens failed, blocks walked from step 0, demand steps walked, demand steps planned); all 0 where the level kernel's
        cut-off did not run."""
        out = (C.c_int64 * 6)()
        self._check(self._lib.sdpgpu_f1_screen_get(self._h, period, out))
        return tuple(int(v) for v in out)

    def f1_screen_rows(self, period: int):
        """The screen rows of the F1 level kernel in `period` of the last solve: (demand steps walked in screened passes, the
        action rows RS such a pass walks -- SDPGPU_F1_SCREEN_ROWS, of the block's 4)."""
        out = (C.c_int64 * 2)()
        self._check(self._lib.sdpgpu_f1_screen_rows_get(self._h, period, out))
        return tuple(int(v) for v in out)

    def f1_level_form(self, period: int):
        """The launch form of the F1 level kernel in `period` of the last solve: (form -- SDPGPU_F1_LEVEL_FORM: 0 four tasks per
        workgroup, 1 one wave per workgroup, 2 waves that claim tasks --, workgroups launched, threads per workgroup); (the
        handle's form, 0, 0) where the level kernel did not run the period."""
        out = (C.c_int64 * 3)()
        self._check(self._lib.sdpgpu_f1_level_form_get(self._h, period, out))
        return tuple(int(v) for v in out)

    def f1_screen_start(self, period: int) -> int:
        """Host arithmetic: the step the screen's rule gives for the pmf of `period` (0: no screen)."""
        return int(self._lib.sdpgpu_f1_screen_start(self._h, period))

    def f1_decided_start(self, period: int) -> int:
        """Host arithmetic: the first state index of `period`'s slab from which action 0 provably wins (the slab's end: none)."""
        return int(self._lib.sdpgpu_f1_decided_start(self._h, period))

    def f1_decided(self, period: int):
        """The decided split of `period`: (boundary by the host rule, live states and decided states of the last solve's launch,
        1 where the split ran, bytes of the chunk-row arenas)."""
        out = (C.c_int64 * 5)()
        self._check(self._lib.sdpgpu_f1_decided_get(self._h, period, out))
        return tuple(int(v) for v in out)

    def period_cells(self, period: int) -> int:
        """Cells of `period` on this rank's slab (-1: not counted)."""
        return int(self._lib.sdpgpu_period_cells(self._h, period))
