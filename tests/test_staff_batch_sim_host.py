"""The fit and rollout of a STAFF batch (sdpgpu_batch_staff_reachable / _fit_ss / _simulate; DESIGN 4 "Workforce batch: fit and
rollout") as far as it goes without a GPU: every refusal with its status and a text that names the call and the argument --
with device = -1 and BEFORE any device call, so a machine without a GPU sees the refusal and not a device error --, the
refusals between the two kinds of batch, and the reachable intervals against workforce.staff_reach_intervals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import staff_block_cases as sb  # noqa: E402
import staff_cases  # noqa: E402
from test_staff_batch_host import _add, _create, _dp, _err, _f1_descs, _ip, _staff_descs  # noqa: E402

OK, ERR_ARG, ERR_STATE, ERR_DEVICE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4
SIM, FIT, REACH = "sdpgpu_batch_staff_simulate", "sdpgpu_batch_staff_fit_ss", "sdpgpu_batch_staff_reachable"
T, N = 3, 3


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


@pytest.fixture
def batch(sia, lib):
    """Three unclamped instances (hires 0..12 from 0, device -1) over one 13-row table in every period."""
    rc, b, err = _create(lib, _staff_descs(sia, N, T), N)
    assert rc == 0 and b.value, err
    assert _add(lib, b, sia.staff_level_pmf([0.3], 13)[0]) == (0, 0)
    assert lib.sdpgpu_batch_use_level_pmf(b, -1, -1, 0) == 0
    yield b
    lib.sdpgpu_batch_destroy(b)


def _sim(sia, lib, b, K=(2, 2, 2), ini=0.0, ss="default", n_rules=None, results=True, k_null=False, n=N):
    k = np.asarray(K, dtype=np.int32)
    if isinstance(ss, str):
        ss = np.tile(np.array([3.0, 9.0]), (n, 1, T, 1))
    lev = None if ss is None else np.ascontiguousarray(ss, dtype=np.float64)
    nr = n_rules if n_rules is not None else (1 if lev is None else lev.shape[1])
    res = (sia._abi.SdpgpuSimResult * (n * 64))()
    rc = lib.sdpgpu_batch_staff_simulate(b, None if k_null else _ip(k), 1, float(ini), None if lev is None else _dp(lev), nr,
                                         res if results else None, None, None, None)
    return rc, _err(lib, b)


def test_the_symbols_and_methods_exist(sia, lib):
    header = open(os.path.join(ROOT, "include", "sdpgpu.h")).read()
    for name in (SIM, FIT, REACH):
        assert name in sia._abi.EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.sdpgpu_abi_version() == 6  # additive
    for m in ("reachable", "fit_ss", "staff_simulate"):
        assert callable(getattr(sia.StaffBatch, m))
    for m in ("fitSinglesS", "simulatesS", "simulateTable", "defaultSampleNums"):
        assert callable(getattr(sia.StaffRecursionBatch, m))
    from stochastic_inventory_amd import workloads
    assert callable(workloads.workforce_testing_loop)


def test_rollout_refusals_name_the_call_and_the_argument(sia, lib, batch):
    b = batch

    def refused(code, *words, **kw):
        rc, err = _sim(sia, lib, b, **kw)
        assert rc == code, (kw, rc, err)
        assert SIM in err and all(w in err for w in words), (kw, err)

    refused(ERR_ARG, "sample_nums", k_null=True)
    refused(ERR_ARG, "results", results=False)
    refused(ERR_ARG, "sample_nums[1]", K=(2, 0, 2))
    refused(ERR_ARG, "sample_nums[2]", K=(2, 2, -1))
    refused(ERR_ARG, "sample_nums", "leaves", K=(4096, 4096, 2))            # 2^25 leaves per rule
    refused(ERR_ARG, "leaf sums", "n_rules", K=(4096, 4096, 1), n_rules=64, ss=np.tile(np.array([3.0, 9.0]), (N, 64, T, 1)))  # 3 x 64 x 2^24
    refused(ERR_ARG, "n_rules = 0", n_rules=0)
    refused(ERR_ARG, "n_rules = 65", n_rules=65)
    refused(ERR_ARG, "n_rules = 2", "ss == NULL", ss=None, n_rules=2)
    for bad in (float("nan"), float("inf"), 2.0 ** 31, -2.0 ** 31 - 1.0):
        ss = np.tile(np.array([3.0, 9.0]), (N, 2, T, 1))
        ss[2, 1, 1, 1] = bad
        refused(ERR_ARG, "ss[2][1][1]", ss=ss)
    ss = np.tile(np.array([3.0, 9.0]), (N, 1, T, 1))
    ss[1, 0, 2] = (7.0, 5.0)
    refused(ERR_ARG, "ss[1][0][2]", "S < s - 1", ss=ss)
    ss[1, 0, 2] = (7.9, 6.0)  # (int) S = (int) s - 1 is legal: hires 0 at x = s - 1; without a device the call then ends there
    rc, err = _sim(sia, lib, b, ss=ss)
    assert rc in (OK, ERR_DEVICE), err
    for bad in (-1.0, 0.5, 1e9 + 1, float("nan")):
        refused(ERR_ARG, "ini_x", ini=bad)
    # the table rule: period 1's box is [0, 0]; inside it, the missing solve
    refused(ERR_ARG, "ini_x", "period 1", ss=None, ini=1.0)
    refused(ERR_STATE, "solved", ss=None, ini=0.0)


def test_a_missing_or_bad_table_is_refused(sia, lib):
    rc, b, err = _create(lib, _staff_descs(sia, N, T), N)
    assert rc == 0, err
    try:
        good = sia.staff_level_pmf([0.3], 13)[0]
        neg = good.copy()
        neg[5, 2] = -1e-9
        nan = good.copy()
        nan[7, 0] = float("nan")
        assert _add(lib, b, good) == (0, 0) and _add(lib, b, neg) == (0, 1) and _add(lib, b, nan) == (0, 2)
        assert lib.sdpgpu_batch_use_level_pmf(b, 0, -1, 0) == 0 and lib.sdpgpu_batch_use_level_pmf(b, 1, 0, 0) == 0
        rc, err = _sim(sia, lib, b)
        assert rc == ERR_STATE and SIM in err and "instance 1" in err and "period 2" in err, err
        lo, hi = C.c_int64(), C.c_int64()
        assert lib.sdpgpu_batch_staff_reachable(b, 1, 2, C.byref(lo), C.byref(hi)) == OK  # (period 2 needs period 1's table only)
        assert lib.sdpgpu_batch_staff_reachable(b, 1, 3, C.byref(lo), C.byref(hi)) == ERR_STATE
        err = _err(lib, b)
        assert REACH in err and "instance 1" in err and "period 2" in err, err
        assert lib.sdpgpu_batch_use_level_pmf(b, -1, -1, 0) == 0 and lib.sdpgpu_batch_use_level_pmf(b, 2, 1, 1) == 0
        rc, err = _sim(sia, lib, b)
        assert rc == ERR_ARG and SIM in err and "table 1" in err and "negative or NaN" in err and "level 5" in err, err
        assert lib.sdpgpu_batch_use_level_pmf(b, 2, 1, 2) == 0
        rc, err = _sim(sia, lib, b)
        assert rc == ERR_ARG and "table 2" in err and "level 7" in err, err
        assert lib.sdpgpu_batch_use_level_pmf(b, 2, 1, 0) == 0  # (tables 1 and 2 stay in the pool, unused: not looked at)
        rc, err = _sim(sia, lib, b)
        assert rc in (OK, ERR_DEVICE), err
    finally:
        lib.sdpgpu_batch_destroy(b)


def test_fit_and_reachable_refusals(sia, lib, batch):
    b = batch
    out = np.zeros(N * T * 2)
    for bad in (float("nan"), float("inf"), -1.0):
        assert lib.sdpgpu_batch_staff_fit_ss(b, bad, _dp(out)) == ERR_ARG
        assert FIT in _err(lib, b) and "max_order_quantity" in _err(lib, b)
    assert lib.sdpgpu_batch_staff_fit_ss(b, 12.0, None) == ERR_ARG and "out" in _err(lib, b)
    assert lib.sdpgpu_batch_staff_fit_ss(b, float(2 ** 31 - 1), _dp(out)) == ERR_STATE
    assert FIT in _err(lib, b) and "sdpgpu_batch_solve" in _err(lib, b)
    lo, hi = C.c_int64(), C.c_int64()
    assert lib.sdpgpu_batch_staff_reachable(b, N, 1, C.byref(lo), C.byref(hi)) == ERR_ARG and f"instance {N}" in _err(lib, b)
    assert lib.sdpgpu_batch_staff_reachable(b, 0, 0, C.byref(lo), C.byref(hi)) == ERR_ARG and "period 0" in _err(lib, b)
    assert lib.sdpgpu_batch_staff_reachable(b, 0, T + 1, C.byref(lo), C.byref(hi)) == ERR_ARG and REACH in _err(lib, b)
    assert lib.sdpgpu_batch_staff_reachable(b, 0, 1, None, C.byref(hi)) == ERR_ARG and "null" in _err(lib, b)
    assert lib.sdpgpu_batch_staff_reachable(None, 0, 1, C.byref(lo), C.byref(hi)) == ERR_ARG


def test_the_two_kinds_of_batch_refuse_each_others_calls(sia, lib, batch):
    rc, f1, err = _create(lib, _f1_descs(sia, 2), 2)
    assert rc == 0, err
    try:
        lo, hi = C.c_int64(), C.c_int64()
        out = np.zeros(64)
        k = np.array([2, 2, 2], dtype=np.int32)
        res = (sia._abi.SdpgpuSimResult * 4)()
        calls = {
            REACH: lambda: lib.sdpgpu_batch_staff_reachable(f1, 0, 1, C.byref(lo), C.byref(hi)),
            FIT: lambda: lib.sdpgpu_batch_staff_fit_ss(f1, 12.0, _dp(out)),
            SIM: lambda: lib.sdpgpu_batch_staff_simulate(f1, _ip(k), 1, 0.0, _dp(out), 1, res, None, None, None),
        }
        for name, call in calls.items():
            assert call() == ERR_UNSUPPORTED, name
            assert name in _err(lib, f1) and "backorder family" in _err(lib, f1), (name, _err(lib, f1))
    finally:
        lib.sdpgpu_batch_destroy(f1)
    # and the backorder batch's fit, reachable and rollouts stay refused on a staff batch, sdpgpu_batch_simulate_ms included
    b = batch
    lo32, hi32 = C.c_int32(), C.c_int32()
    out = np.zeros(64)
    assert lib.sdpgpu_batch_reachable(b, 0, 1, C.byref(lo32), C.byref(hi32)) == ERR_UNSUPPORTED and "staff family" in _err(lib, b)
    assert lib.sdpgpu_batch_fit_ss(b, 1, _dp(out)) == ERR_UNSUPPORTED and "sdpgpu_batch_fit_ss" in _err(lib, b)
    assert lib.sdpgpu_batch_simulate_ss_sampled(b, 1, _dp(out), 1, C.c_uint64(1), None, _dp(out), None) == ERR_UNSUPPORTED
    assert lib.sdpgpu_batch_simulate_ms(b) == -1.0 and "staff family" in _err(lib, b)


def _lens(c):
    rows = c.table.shape[1]
    return np.arange(rows, dtype=np.int64) + 1 if c.row_len is None else np.asarray(c.row_len, dtype=np.int64)


def _one_table_per_period(sia, cases):
    descs, tables, use, mins = [], [], [], []
    for c in cases:
        d = c.functor.to_desc(c.T)
        d.kernel = sia._abi.KERNEL_SEPARABLE
        descs.append(d)
        use.append(list(range(len(tables), len(tables) + c.T)))
        tables += [(c.table[t], c.row_len) for t in range(c.T)]
        mins.append(list(c.functor.minStaffNum))
    return sia.StaffBatch(descs, tables, use, mins)


@pytest.mark.parametrize("make", [staff_cases.staff_testing_small, sb.growing, staff_cases.staff_rates, staff_cases.staff_planning_small,
                                  staff_cases.staff_short_rows, staff_cases.staff_single], ids=lambda f: f.__name__)
def test_reachable_is_staff_reach_intervals(sia, make):
    """Unclamped growing boxes (from 0 and from a start above it), clamped cases, rows shorter than y + 1 (row_len)."""
    from stochastic_inventory_amd.workforce import staff_reach_intervals
    c = make()
    want = staff_reach_intervals(c.functor, [_lens(c)] * c.T)
    with _one_table_per_period(sia, [c, c]) as b:
        for i in (0, 1):
            assert [b.reachable(i, t) for t in range(1, c.T + 1)] == want, (c.name, i)


def test_reachable_with_tables_that_differ_by_period(sia):
    """Two instances of one shape and one staff range whose rows end differently by period: full rows in one period, rows of at
    most 6 entries in the other -- instance 0 walks (short, full, full), instance 1 (full, short, full).  Unclamped boxes need
    ONE staff range per period, so the two orders share a clamped shape."""
    from stochastic_inventory_amd.workforce import StaffFunctor, staff_reach_intervals
    rows = 25
    full = sia.staff_level_pmf([0.4], rows)[0]
    short_len = np.minimum(np.arange(rows) + 1, 6).astype(np.int32)
    f = StaffFunctor(fixCost=30, unitVariCost=3, salary=4, unitPenalty=40, minStaffNum=[6, 6, 6], maxHireNum=3, minX=0, maxX=24,
                     clampStaff=True, iniStaffNum=20)
    descs = []
    for _ in range(2):
        d = f.to_desc(3)
        d.kernel = sia._abi.KERNEL_SEPARABLE
        descs.append(d)
    full_len = np.arange(rows, dtype=np.int64) + 1
    use = [[1, 0, 0], [0, 1, 0]]
    lens = [full_len, short_len.astype(np.int64)]
    with sia.StaffBatch(descs, [(full, None), (full[:, :6].copy(), short_len)], use, [[6, 6, 6]] * 2) as b:
        got = [[b.reachable(i, t) for t in (1, 2, 3)] for i in (0, 1)]
    want = [staff_reach_intervals(f, [lens[k] for k in use[i]]) for i in (0, 1)]
    assert got == want
    assert got[0] != got[1]  # (the case tells the two walks apart)


def test_get_opt_table_takes_its_intervals_from_the_library(sia):
    """StaffRecursionBatch.getOptTable no longer recomputes the intervals in numpy."""
    from stochastic_inventory_amd import workforce
    import inspect
    src = inspect.getsource(workforce.StaffRecursionBatch.getOptTable)
    assert "reachable(" in src and "staff_reach_intervals(f" not in src
