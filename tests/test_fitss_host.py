"""The (s, S) level rules (sdpgpu_batch_reachable, sdpgpu_fit_ss, sdpgpu_batch_fit_ss, sdpgpu_batch_simulate_ss*; DESIGN 4
"Batched (s, S) level rules") as far as they go without a GPU: the reachable interval of a batch instance against the
oracle's mask, the host fit and the Python FitsS against the independent twin (tests/fitss_twin.py) bit for bit -- on the
oracle's tables of fitss_sweep(patterns=(2, 7)) and on synthetic rows that reach every live branch of the three methods --
and every refusal, before any device call."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fitss_twin as tw  # noqa: E402
from test_gpu_batch_ragged import _ragged_instances  # noqa: E402  (the seeded ragged mix)

NEW_SYMBOLS = ("sdpgpu_batch_reachable", "sdpgpu_fit_ss", "sdpgpu_fit_level_index", "sdpgpu_fit_min_square", "sdpgpu_batch_fit_ss",
               "sdpgpu_batch_simulate_ss", "sdpgpu_batch_simulate_ss_sampled")


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def opt_table(desc, pol, masks):
    """Rows [period, x, Q] of the oracle's policy on the oracle's reachable mask, as Recursion.getOptTable orders them."""
    rows = []
    for t, (p, m) in enumerate(zip(pol, masks)):
        idx = np.nonzero(m)[0]
        x = desc.min_inventory + idx.astype(np.float64) * desc.step
        rows.append(np.stack([np.full(len(idx), float(t + 1)), x, p[idx].astype(np.float64) * desc.step], axis=1))
    return np.concatenate(rows, axis=0)


def oracle_tables(oracle, descs, pmfs, workers=8):
    def one(k):
        P = oracle.Problem(descs[k], pmfs[k])
        _, pol, _ = P.solve()
        return opt_table(descs[k], pol, P.reachable())
    with ThreadPoolExecutor(max_workers=workers) as ex:  # (the C solver releases the GIL)
        return list(ex.map(one, range(len(descs))))


@pytest.fixture(scope="module")
def fitss_tables(oracle):
    from stochastic_inventory_amd import workloads
    ws = workloads.fitss_sweep(patterns=(2, 7))
    return ws, oracle_tables(oracle, [w.desc() for w in ws], [w.pmf for w in ws])


def lib_fit(lib, levels, T, max_q, table):
    table = np.ascontiguousarray(table, dtype=np.float64)
    out = np.full((T, 2 * levels), np.nan)
    rc = lib.sdpgpu_fit_ss(levels, T, float(max_q), _dp(table), len(table), _dp(out))
    assert rc == 0, lib.sdpgpu_last_error(None)
    return out


def test_the_new_symbols_are_declared_and_exported(sia, lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdpgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in sia._abi.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert lib.sdpgpu_abi_version() == 6  # additive
    assert {"FitsS", "SimulateFitsS"} <= set(sia.__all__)
    for name in ("reachable", "fit_ss", "simulate_ss", "simulate_ss_sampled"):
        assert hasattr(sia.SdpBatch, name)
    for name in ("simulateSinglesS", "simulateTwosS", "simulateThreesS"):
        assert hasattr(sia.SimulationBatch, name) and hasattr(sia.SimulateFitsS, name)
    assert hasattr(sia.RecursionBatch, "getOptTable")


# ---- the reachable interval --------------------------------------------------------------------------------------------------

def _assert_interval_is_the_mask(b, i, masks, what):
    for period, m in enumerate(masks, start=1):
        lo, hi = b.reachable(i, period)
        want = np.zeros(len(m), dtype=bool)
        want[lo:hi + 1] = True
        assert np.array_equal(want, m), (what, i, period, lo, hi, np.nonzero(m)[0][[0, -1]])


def test_reachable_equals_the_oracles_mask_on_the_ragged_mix(sia, oracle):
    T = 4
    functors, pmfs = _ragged_instances(sia, T=T)
    descs = [f.to_desc(T) for f in functors]
    with sia.SdpBatch(descs, pmfs, ragged=True) as b:
        for i in range(len(descs)):
            _assert_interval_is_the_mask(b, i, oracle.Problem(descs[i], pmfs[i]).reachable(), "ragged mix")


def test_reachable_equals_the_oracles_mask_on_fitss_instances(sia, oracle):
    """The mask depends on the pmfs, the order limit and the initial state, not on the costs: the oracle walks one instance
    per (pattern, capacity); every instance's interval is then checked against its representative's mask."""
    from stochastic_inventory_amd import workloads
    ws = workloads.fitss_sweep(patterns=(2, 7))
    descs, pmfs = [w.desc() for w in ws], [w.pmf for w in ws]
    masks = {}
    for i, w in enumerate(ws):
        if (w.pattern, w.capacity) not in masks:
            masks[(w.pattern, w.capacity)] = oracle.Problem(descs[i], pmfs[i]).reachable()
    assert len(masks) == 6
    with sia.SdpBatch(descs, pmfs, ragged=True) as b:
        for i, w in enumerate(ws):
            _assert_interval_is_the_mask(b, i, masks[(w.pattern, w.capacity)], w.name)
        assert b.reachable(0, 1) == (300, 300)


def test_reachable_refusals(sia, lib):
    T = 3
    functors, pmfs = _ragged_instances(sia, n=2, T=T)
    arr = (sia.SdpgpuDesc * 2)()
    for i, f in enumerate(functors):
        d = f.to_desc(T)
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(sia.SdpgpuDesc))
    b = C.c_void_p()
    assert lib.sdpgpu_batch_create_ragged(arr, 2, C.byref(b)) == 0
    err = lambda: lib.sdpgpu_batch_last_error(b).decode()
    lo, hi = C.c_int32(-7), C.c_int32(-7)
    try:
        assert lib.sdpgpu_batch_reachable(None, 0, 1, C.byref(lo), C.byref(hi)) == 1
        assert lib.sdpgpu_batch_reachable(b, 2, 1, C.byref(lo), C.byref(hi)) == 1 and "instance 2" in err()
        assert lib.sdpgpu_batch_reachable(b, 0, 0, C.byref(lo), C.byref(hi)) == 1 and "period 0" in err()
        assert lib.sdpgpu_batch_reachable(b, 0, T + 1, C.byref(lo), C.byref(hi)) == 1
        assert lib.sdpgpu_batch_reachable(b, 0, 1, None, C.byref(hi)) == 1 and "null" in err()
        # period 1 needs no pmf, period 2 the pmf of period 1
        assert lib.sdpgpu_batch_reachable(b, 0, 1, C.byref(lo), C.byref(hi)) == 0 and lo.value == hi.value
        assert lo.value == int(functors[0].iniInventory - functors[0].minInventory)
        assert lib.sdpgpu_batch_reachable(b, 0, 2, C.byref(lo), C.byref(hi)) == 2 and "instance 0, period 1" in err()
    finally:
        lib.sdpgpu_batch_destroy(b)


# ---- the fit: the oracle's tables ----------------------------------------------------------------------------------------------

def test_fit_on_the_fitss_tables_equals_the_twin(sia, lib, fitss_tables):
    ws, tables = fitss_tables
    T = 6
    lengths = {}
    trace = set()
    for w, table in zip(ws, tables):
        max_q = int(w.functor.maxOrderQuantity)
        fit = sia.FitsS(max_q, T)
        for levels, method in ((1, fit.getSinglesS), (2, fit.getTwosS), (3, fit.getThreesS)):
            want = tw.fit(levels, T, max_q, table, trace)
            assert np.array_equal(lib_fit(lib, levels, T, max_q, table), want), (w.name, levels)
            assert np.array_equal(method(table), want), (w.name, levels)
        for t in range(1, T):
            rows = table[table[:, 0] == t + 1]
            idx = tw.level_index(rows, max_q)
            assert fit.levelIndex(rows).tolist() == idx, (w.name, t + 1)
            lengths[len(idx)] = lengths.get(len(idx), 0) + 1
    # what real tables supply: lists of one, two and three entries, never longer
    assert lengths == {1: 679, 2: 116, 3: 15}, lengths
    assert {"L1:one", "L2:two", "L3:three", "L1:minsq", "L2:minsq"} <= trace and "L3:minsq" not in trace


def test_fitted_levels_of_the_fitss_tables_are_ordered_rules(fitss_tables):
    """Sanity of the definition on real tables, independent of any implementation detail: period 1 is (ini + 1, ini + Q),
    the bands ascend, and an order-up-to level is never below its band's threshold."""
    ws, tables = fitss_tables
    for w, table in list(zip(ws, tables))[::9]:
        o = tw.fit(3, 6, int(w.functor.maxOrderQuantity), table)
        assert o[0, 0] == 1.0 and o[0, 1] == table[0, 2]
        assert np.all(o[1:, 0] <= o[1:, 2]) and np.all(o[1:, 2] <= o[1:, 4]), w.name
        assert np.all(o[1:, 1::2] >= o[1:, 0::2]), w.name


# ---- the fit: synthetic rows ---------------------------------------------------------------------------------------------------

def _table(periods, first=(0.0, 3.0)):
    """[period, x, Q] rows: period 1 = `first`, then one list of (x, Q) per later period."""
    rows = [[1.0, first[0], first[1]]]
    for t, pr in enumerate(periods, start=2):
        rows += [[float(t), float(x), float(q)] for x, q in pr]
    return np.array(rows)


def _hand_made():
    """(name, maxQ, rows of ONE later period)."""
    M = 5
    asc = lambda qs, x0=0: [(x0 + j, q) for j, q in enumerate(qs)]
    return [
        ("plain (s, S)", M, asc([M, M, 4, 3, 2, 1, 0, 0, 0], -4)),
        ("zero in row 0", M, asc([0, 0, 0])),
        ("single row at the limit", M, asc([M], 7)),
        ("single row below the limit", M, asc([2], 7)),
        ("single zero row", M, asc([0], -3)),
        ("every row at the limit: one-level correction", M, asc([M, M, M])),
        ("below the limit, then the last row at it", M, asc([3, M])),
        ("two entries, the last row still at the limit", M, asc([M, 3, M, M])),
        ("two entries ending in a zero", M, asc([M, 3, M, 2, 0, 0])),
        ("three entries, the last row still at the limit", M, asc([M, 3, M, 3, M, M])),
        ("three entries ending in a zero", M, asc([4, M, 4, M, 1, 0])),
        ("four entries", M, asc([4, M, 4, M, 2, M, 1, 0], -10)),
        ("five entries, the last row at the limit", M, asc([1, M, 1, M, 1, M, 1, M, M])),
        ("min-square mean below lb", M, asc([1, M, 1, M, 1, 1, 1, 1, 1, 0])),
        ("min-square with no row below the limit before upIndex", M, asc([M, M, 2, M, M, 3, M, 0])),
        ("maxQ = 0", 0, asc([0, 0, 0, 0], -2)),
        ("maxQ = 0, one row", 0, asc([0])),
        ("quantities above the limit", M, asc([7, M, 6, 3, M, 0])),
        ("fractional levels", M, [(0.25, 4.5), (1.25, M), (2.25, 2.125), (3.25, M), (4.25, 0.7), (5.25, 0.0)]),
        ("no zero at all", M, asc([4, M, 3, M, 2])),
    ]


def _seeded(n_cases=400, seed=20240617):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n_cases):
        M = int(rng.choice([1, 2, 5, 40]))
        n = int(rng.integers(1, 14))
        x0 = int(rng.integers(-50, 50))
        p_zero = float(rng.choice([0.0, 0.1, 0.3]))
        qs = []
        for _ in range(n):
            u = rng.random()
            qs.append(0 if u < p_zero else (M if u < p_zero + 0.4 else int(rng.integers(0, M + 1))))
        out.append((f"seeded {c}", M, [(x0 + j, q) for j, q in enumerate(qs)]))
    return out


def test_fit_on_synthetic_rows_equals_the_twin_and_reaches_every_live_branch(sia, lib):
    trace = set()
    longest = 0
    cases = _hand_made() + _seeded()
    for name, M, rows in cases:
        table = _table([rows, [(0, M), (1, 0)] if M else [(0, 0)]])  # the period under test, then a plain one: T = 3
        fit = sia.FitsS(M, 3)
        for levels, method in ((1, fit.getSinglesS), (2, fit.getTwosS), (3, fit.getThreesS)):
            want = tw.fit(levels, 3, M, table, trace)
            assert np.array_equal(lib_fit(lib, levels, 3, M, table), want), (name, levels)
            assert np.array_equal(method(table), want), (name, levels)
        arr = np.array([[2.0, x, q] for x, q in rows])
        idx = tw.level_index(arr.tolist(), M)
        longest = max(longest, len(idx))
        assert len(idx) >= 1, name  # the list is never empty: the `length == 0` branch is dead code
        assert fit.levelIndex(arr).tolist() == idx, name
        for up in sorted({idx[0], idx[-1], len(rows) - 1}):
            for lb in (arr[up, 1], -1e9, 20000.0):
                assert fit.minSquare(lb, up, arr) == tw.min_square(lb, up, arr.tolist(), M), (name, up, lb)
    assert longest >= 5
    assert trace >= tw.LIVE_BRANCHES, sorted(tw.LIVE_BRANCHES - trace)


def test_named_cases_give_the_levels_the_definition_says(sia):
    M = 5
    by_name = {name: rows for name, _, rows in _hand_made()}
    fit = sia.FitsS(M, 2)
    one = lambda name, method: method(_table([by_name[name]]))[1].tolist()
    # x = -4 .. 4, Q = 5 5 4 3 2 1 0 0 0: the first zero is row 6 (x = 2), the row below it stands at 1 + 1
    assert one("plain (s, S)", fit.getSinglesS) == [2.0, 2.0]
    assert one("plain (s, S)", fit.getThreesS) == [2.0, 2.0] * 3
    assert one("zero in row 0", fit.getTwosS) == [0.0] * 4
    assert one("single row at the limit", fit.getSinglesS) == [7.0, 7.0]  # index 0: "s, S are both" the row's inventory
    # "last row still at the limit": s = x + 1 (the literal 1), S = x + Q
    assert one("every row at the limit: one-level correction", fit.getSinglesS) == [3.0, 7.0]
    assert one("two entries, the last row still at the limit", fit.getTwosS) == [2.0, 4.0, 4.0, 8.0]
    assert one("three entries, the last row still at the limit", fit.getThreesS) == [2.0, 4.0, 4.0, 6.0, 6.0, 10.0]
    # four entries [1, 3, 5, 7] at x = -10 ..: s3 = x_7, S3 = x_6 + 1, s2 = x_5, S2 = x_4 + 2, s1 = x_3, S1 = min-square over rows
    # 0 (4 - 10) and 2 (4 - 8): mean -5, above lb = x_3 = -7
    assert one("four entries", fit.getThreesS) == [-7.0, -5.0, -5.0, -4.0, -3.0, -3.0]
    # terms 1, 3, 5, 6, 7, 8, 9, 9: mean 6 below lb = x_9 = 9
    assert one("min-square mean below lb", fit.getSinglesS) == [9.0, 9.0]
    assert fit.minSquare(-100.0, 9, np.array([[2.0, x, q] for x, q in by_name["min-square mean below lb"]])) == 6.0
    assert sia.FitsS(0, 2).getThreesS(_table([by_name["maxQ = 0"]]))[1].tolist() == [-2.0] * 6
    # period 1: s = x_0 + 1, S = x_0 + Q_0, repeated per level
    assert fit.getThreesS(_table([by_name["plain (s, S)"]], first=(10.0, 4.0)))[0].tolist() == [11.0, 14.0] * 3


def test_get_only_single_s_keeps_the_periods_with_one_level(sia, capsys):
    M = 5
    by_name = {name: rows for name, _, rows in _hand_made()}
    table = _table([by_name["plain (s, S)"], by_name["four entries"], by_name["zero in row 0"]])
    fit = sia.FitsS(M, 4)
    got = fit.getOnlySinglesS(table)
    assert got[0].tolist() == [1.0, 3.0] and got[1].tolist() == [2.0, 2.0]
    assert got[2].tolist() == [0.0, 0.0] and got[3].tolist() == [0.0, 0.0]
    assert capsys.readouterr().out.count("may be wrong!") == 2


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_fit_ss_refusals(sia, lib):
    table = _table([[(0, 5), (1, 0)]])
    out = np.zeros((2, 6))
    err = lambda: lib.sdpgpu_last_error(None).decode()
    for levels in (0, 4, -1):
        assert lib.sdpgpu_fit_ss(levels, 2, 5.0, _dp(table), len(table), _dp(out)) == 1 and "levels" in err()
    assert lib.sdpgpu_fit_ss(1, 2, 5.0, None, len(table), _dp(out)) == 1 and "null" in err()
    assert lib.sdpgpu_fit_ss(1, 2, 5.0, _dp(table), len(table), None) == 1 and "null" in err()
    assert lib.sdpgpu_fit_ss(1, 2, 5.0, _dp(table), 0, _dp(out)) == 1 and "n_rows" in err()
    assert lib.sdpgpu_fit_ss(1, 0, 5.0, _dp(table), len(table), _dp(out)) == 1 and "T = 0" in err()
    assert lib.sdpgpu_fit_ss(1, 3, 5.0, _dp(table), len(table), _dp(out)) == 1 and "period 3" in err()  # no rows of period 3
    assert lib.sdpgpu_fit_ss(1, 2, 5.0, _dp(table), len(table), _dp(out)) == 0 and err() == ""
    n = C.c_int32()
    idx = np.zeros(4, dtype=np.int32)
    q = np.array([5.0, 0.0])
    assert lib.sdpgpu_fit_level_index(5.0, None, 2, idx.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)) == 1
    assert lib.sdpgpu_fit_level_index(5.0, _dp(q), 0, idx.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)) == 0 and n.value == 0
    val = C.c_double()
    assert lib.sdpgpu_fit_min_square(5.0, 0.0, 2, _dp(q), _dp(q), 2, C.byref(val)) == 1 and "up_index" in err()
    assert lib.sdpgpu_fit_min_square(5.0, 0.0, -1, _dp(q), _dp(q), 2, C.byref(val)) == 1
    assert lib.sdpgpu_fit_min_square(5.0, 0.0, 0, _dp(q), _dp(q), 0, C.byref(val)) == 1
    with pytest.raises(ValueError):
        sia.FitsS(5, 2).getSinglesS(np.zeros((3, 4)))
    with pytest.raises(sia.SdpgpuError) as e:
        sia.FitsS(5, 3).getSinglesS(table)
    assert e.value.code == 1 and "period 3" in e.value.message


def _batch(sia, lib, n=3, T=3, step=1.0, with_pmf=True):
    arr = (sia.SdpgpuDesc * n)()
    for i in range(n):
        d = sia.desc_defaults()
        d.periods, d.step = T, step
        d.min_inventory, d.max_inventory, d.max_order_quantity = -20.0, 30.0, 12.0
        d.fixed_order_cost, d.unit_order_cost, d.holding_cost, d.penalty_cost = 10.0 + i, float(i % 2), 1.0, 5.0 + i
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(sia.SdpgpuDesc))
    b = C.c_void_p()
    assert lib.sdpgpu_batch_create(arr, n, C.byref(b)) == 0, lib.sdpgpu_batch_last_error(None)
    if with_pmf:
        dem = np.arange(4, dtype=np.float64) * step
        p = np.full(4, 0.25)
        for i in range(n):
            for t in range(T):
                assert lib.sdpgpu_batch_set_pmf(b, i, t, _dp(dem), _dp(p), 4) == 0
    return b


def test_batch_fit_refusals(sia, lib):
    b = _batch(sia, lib)
    err = lambda: lib.sdpgpu_batch_last_error(b).decode()
    out = np.zeros((3, 3, 6))
    try:
        assert lib.sdpgpu_batch_fit_ss(None, 1, _dp(out)) == 1
        for levels in (0, 4, -2):
            assert lib.sdpgpu_batch_fit_ss(b, levels, _dp(out)) == 1 and "levels" in err()
        assert lib.sdpgpu_batch_fit_ss(b, 2, None) == 1 and "out is null" in err()
        assert lib.sdpgpu_batch_fit_ss(b, 2, _dp(out)) == 2 and "before sdpgpu_batch_solve" in err()
    finally:
        lib.sdpgpu_batch_destroy(b)
    b = _batch(sia, lib, step=2.0)
    try:
        assert lib.sdpgpu_batch_fit_ss(b, 2, _dp(out)) == 4 and b"step == 1" in lib.sdpgpu_batch_last_error(b)
    finally:
        lib.sdpgpu_batch_destroy(b)


def test_simulate_ss_validates_before_any_device_call(sia, lib):
    b = _batch(sia, lib)
    err = lambda: lib.sdpgpu_batch_last_error(b).decode()
    try:
        dem = np.zeros((5, 3))
        mean = np.zeros(3)
        sums = np.zeros((3, 5))
        ss = np.zeros((3, 3, 6))
        sim, sam = lib.sdpgpu_batch_simulate_ss, lib.sdpgpu_batch_simulate_ss_sampled
        assert sim(None, 1, _dp(ss), 5, _dp(dem), 0, None, _dp(mean), None) == 1
        assert sam(None, 1, _dp(ss), 5, 1, None, _dp(mean), None) == 1
        for levels in (0, 4, -1):
            assert sim(b, levels, _dp(ss), 5, _dp(dem), 0, None, _dp(mean), None) == 1 and "levels" in err()
            assert sam(b, levels, _dp(ss), 5, 1, None, _dp(mean), None) == 1 and "levels" in err()
        assert sim(b, 2, _dp(ss), 5, _dp(dem), 0, None, None, None) == 1 and "out_mean" in err()
        assert sam(b, 2, _dp(ss), 5, 1, None, None, None) == 1 and "out_mean" in err()
        assert sim(b, 2, _dp(ss), 5, None, 0, None, _dp(mean), None) == 1 and "demand" in err()
        assert sim(b, 2, _dp(ss), 0, _dp(dem), 0, None, _dp(mean), None) == 1 and "n_paths = 0" in err()
        assert sim(b, 2, _dp(ss), -3, _dp(dem), 0, None, _dp(mean), None) == 1 and "n_paths" in err()
        assert sam(b, 2, _dp(ss), 0, 1, None, _dp(mean), None) == 1 and "n_paths = 0" in err()
        assert sam(b, 2, _dp(ss), (1 << 24) + 1, 1, None, _dp(mean), None) == 4 and "exceeds" in err()
        assert sim(b, 2, _dp(ss), 5, _dp(dem), 7, None, _dp(mean), None) == 1 and "instance_stride" in err()
        for bad in (31.0, -21.0, 0.5, float("nan")):
            ini = np.array([0.0, 3.0, bad])
            assert sim(b, 2, _dp(ss), 5, _dp(dem), 0, _dp(ini), _dp(mean), None) == 1
            assert "instance 2" in err() and "ini_x" in err(), err()
            assert sam(b, 2, _dp(ss), 5, 1, _dp(ini), _dp(mean), None) == 1 and "instance 2" in err()
        # ss = NULL fits first: nothing is solved
        assert sim(b, 2, None, 5, _dp(dem), 0, None, _dp(mean), _dp(sums)) == 2 and "before sdpgpu_batch_solve" in err()
        assert sam(b, 3, None, 5, 1, None, _dp(mean), _dp(sums)) == 2 and "before sdpgpu_batch_solve" in err()
    finally:
        lib.sdpgpu_batch_destroy(b)
    b = _batch(sia, lib, step=2.0)
    try:
        mean, ss = np.zeros(3), np.zeros((3, 3, 2))
        assert lib.sdpgpu_batch_simulate_ss_sampled(b, 1, _dp(ss), 5, 1, None, _dp(mean), None) == 4
        assert b"step == 1" in lib.sdpgpu_batch_last_error(b)
        assert lib.sdpgpu_batch_simulate_ss(b, 1, None, 5, _dp(np.zeros((5, 3))), 0, None, _dp(mean), None) == 4
        assert b"step == 1" in lib.sdpgpu_batch_last_error(b)
    finally:
        lib.sdpgpu_batch_destroy(b)
    b = _batch(sia, lib, with_pmf=False)
    try:  # an explicit rule needs the pmfs (and a device), not a solve
        mean, ss = np.zeros(3), np.zeros((3, 3, 2))
        assert lib.sdpgpu_batch_simulate_ss(b, 1, _dp(ss), 5, _dp(np.zeros((5, 3))), 0, None, _dp(mean), None) == 2
        assert b"instance 0, period 1" in lib.sdpgpu_batch_last_error(b)
    finally:
        lib.sdpgpu_batch_destroy(b)


def test_python_wrappers_check_the_rule_shape(sia):
    functors, pmfs = _ragged_instances(sia, n=3, T=3)
    with sia.SdpBatch([f.to_desc(3) for f in functors], pmfs, ragged=True) as b:
        with pytest.raises(ValueError):
            b.simulate_ss_sampled(2, 10, 1, ss=np.zeros((3, 3, 2)))  # a one-level rule for two levels
        with pytest.raises(ValueError):
            b.simulate_ss(1, np.zeros((10, 3)), ss=np.zeros((2, 3, 2)))
        with pytest.raises(ValueError):
            b.simulate_ss(1, np.zeros((10, 4)), ss=np.zeros((3, 3, 2)))
        with pytest.raises(sia.SdpgpuError) as e:
            b.fit_ss(4)
        assert e.value.code == 1
        with pytest.raises(sia.SdpgpuError) as e:
            b.fit_ss(1)
        assert e.value.code == 2


def test_an_explicit_rule_without_a_device_is_a_device_error(sia, lib):
    """An explicit rule needs the pmfs and a device, not a solve: with valid arguments the only thing that can be missing here
    is the device (SDPGPU_ERR_DEVICE with the runtime's text); where there is one, the call succeeds."""
    has_gpu = False
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        pass
    b = _batch(sia, lib)
    try:
        mean, ss = np.zeros(3), np.zeros((3, 3, 2))
        rc = lib.sdpgpu_batch_simulate_ss_sampled(b, 1, _dp(ss), 5, 1, None, _dp(mean), None)
        if has_gpu:
            assert rc == 0 and np.all(mean > 0)
        else:
            assert rc == 3 and lib.sdpgpu_batch_last_error(b) != b""
    finally:
        lib.sdpgpu_batch_destroy(b)


def test_an_unsolved_batch_rolls_an_explicit_rule_but_not_its_tables(sia, lib):
    """The two rollouts share one instance record and one host path, not their refusals: on a batch with every pmf set and
    nothing solved an explicit rule goes on to the device (here: the error that there is none), the table rollout stops at
    the state error -- before and after the other call."""
    has_gpu = False
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        pass
    b = _batch(sia, lib)
    err = lambda: lib.sdpgpu_batch_last_error(b).decode()
    try:
        dem, mean, ss = np.zeros((5, 3)), np.zeros(3), np.zeros((3, 3, 2))
        for _ in range(2):
            assert lib.sdpgpu_batch_simulate(b, 5, _dp(dem), 0, None, _dp(mean), None) == 2 and "before sdpgpu_batch_solve" in err()
            rc = lib.sdpgpu_batch_simulate_ss(b, 1, _dp(ss), 5, _dp(dem), 0, None, _dp(mean), None)
            if has_gpu:
                assert rc == 0, err()
            else:
                assert rc == 3 and "no HIP device available" in err(), err()
    finally:
        lib.sdpgpu_batch_destroy(b)
