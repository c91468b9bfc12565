"""A batch of STAFF-family instances on the device (csrc/sdp_staff_batch.hpp: two launches per period for all instances).

Parity statement (include/sdpgpu.h): every instance's value and policy tables are BIT-IDENTICAL to those of its own separable
handle (SdpEngine with kernel = KERNEL_SEPARABLE), hence to tests/staff_separable_twin.py; every comparison below is
np.array_equal.  The shapes are the smallest at which each thing can break: one instance, a group that fills instance blocks
and leaves a short one, a lone instance next to it, tables that differ by period, many waves with a part-filled last one,
lanes of unequal row length, two ping-pong tables, exact ties."""
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import staff_block_cases as sb  # noqa: E402
import staff_cases  # noqa: E402
import staff_separable_twin as twin  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def staffref():
    from oracle import staffref as m
    m.build()
    return m


def ragged_small():
    """The construction of tests/test_gpu_staff_separable.py: 70 staff numbers x 41 hires over rows of lengths drawn from
    1 .. min(y + 1, 9), NaN behind every row's length."""
    table, row_len = sb.ragged_table(0.01, 60, 9, 2, seed=22)
    assert np.isnan(table).any()
    return staff_cases.StaffCase("ragged_small", sb._functor([20, 31], 40, 69), table, row_len)


SINGLES = {
    "staff_single": staff_cases.staff_single,                # 1 state, 1 action, 1 period
    "staff_testing_small": staff_cases.staff_testing_small,  # unclamped growing boxes, the last-row clamp, one state in period 1
    "staff_short_rows": staff_cases.staff_short_rows,        # row_len
    "staff_wide_actions": staff_cases.staff_wide_actions,    # 301 actions: further trips of the 4-stride scan; a part-filled second tile
    "ragged_small": ragged_small,                            # NaN behind row ends must reach nothing
}


def variant(c, name, **changes):
    """The instance `c` with other costs / minStaffNum, over the SAME table memory."""
    return staff_cases.StaffCase(name, dataclasses.replace(c.functor, **changes), c.table, c.row_len)


def make_batch(sia, cases, store_all=1):
    """One StaffBatch of staff_cases.StaffCase objects; per-period slices that are the same memory share a pool table."""
    descs, tables, use, mins, keys = [], [], [], [], {}
    for c in cases:
        d = c.functor.to_desc(c.T)
        d.kernel, d.device, d.store_all_values = sia._abi.KERNEL_SEPARABLE, 0, store_all
        descs.append(d)
        row = []
        for t in range(c.T):
            sl = c.table[t]
            key = (sl.__array_interface__["data"][0], sl.shape, sl.strides, id(c.row_len))
            if key not in keys:
                keys[key] = len(tables)
                tables.append((sl, c.row_len))
            row.append(keys[key])
        use.append(row)
        mins.append(list(c.functor.minStaffNum))
    return sia.StaffBatch(descs, tables, use, mins)


def handle_tables(sia, c, store_all=1):
    d = c.functor.to_desc(c.T)
    d.kernel, d.device, d.store_all_values = sia._abi.KERNEL_SEPARABLE, 0, store_all
    with sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len) as eng:
        eng.solve(sync=True)
        st = eng.stats()
        assert st.kernel_used == 3
        periods = range(1, c.T + 1) if store_all else (1, 2)
        return {t: eng.values(t) for t in periods}, [eng.policy(t) for t in range(1, c.T + 1)], int(st.cells_evaluated)


def batch_tables(b, i, T):
    return [b.values(i, t) for t in range(1, T + 1)], [b.policy(i, t) for t in range(1, T + 1)]


def assert_instance(b, i, c, V, pol):
    """Instance i of the batch against its handle's tables (V: {period: values})."""
    for t in range(1, c.T + 1):
        got_v, got_p = b.values(i, t), b.policy(i, t)
        assert got_v.shape == V[t].shape, (c.name, i, t)
        assert np.array_equal(got_v, V[t]), (c.name, i, t, int(np.count_nonzero(got_v != V[t])))
        assert np.array_equal(got_p, pol[t - 1]), (c.name, i, t, int(np.count_nonzero(got_p != pol[t - 1])))


@functools.lru_cache(maxsize=None)
def _mid():
    return sb.clamped_mid()


@pytest.mark.parametrize("name", list(SINGLES))
def test_a_batch_of_one(sia, staffref, name):
    """Every period equals the twin fed the device's own V_{t+1} (a failure names its period), and the separable handle."""
    c = SINGLES[name]()
    P = c.oracle_problem(staffref)
    with make_batch(sia, [c]) as b:
        b.solve()
        assert b.plan(1).r == 1
        V, pol = batch_tables(b, 0, c.T)
        st = b.stats()
    for t in range(c.T, 0, -1):
        assert len(V[t - 1]) == int(P.nx[t - 1]), (name, t)
        tv, tp, _, _ = twin.period(c, P, t, V[t] if t < c.T else None)
        assert np.isfinite(V[t - 1]).all(), (name, t)
        assert np.array_equal(V[t - 1], tv), (name, t, int(np.count_nonzero(V[t - 1] != tv)))
        assert np.array_equal(pol[t - 1], tp), (name, t, int(np.count_nonzero(pol[t - 1] != tp)))
    hV, hpol, cells = handle_tables(sia, c)
    for t in range(1, c.T + 1):
        assert np.array_equal(V[t - 1], hV[t]) and np.array_equal(pol[t - 1], hpol[t - 1]), (name, t)
    assert (st.instances, st.periods_run, st.period_launches, st.cells_evaluated) == (1, c.T, 2 * c.T, cells)
    assert (st.finalize_launches, st.window_r, st.window_s, st.window_chunks, st.lds_bytes) == (0, 0, 0, 0, 0)


def test_scaled_sweep(sia):
    """WorkforceTesting's lambdas at maxHire 12, T = 4, no clamp, ini 0: 2 rates (two pool tables) x 2 x 2 x 2 x 4 = 64 instances
    in the reference's loop order; two groups of 32 per period."""
    T = 4
    tabs = [sia.staff_level_pmf([r] * T, 13) for r in (0.1, 0.5)]
    cases, descs, use = [], [], []
    for g, table in enumerate(tabs):
        for fix in (50, 1000):
            for salary in (30, 200):
                for pen in (50, 2200):
                    for ms in ([4, 4, 4, 4], [1, 2, 3, 4], [8, 6, 4, 2], [4, 5, 8, 6]):
                        f = sia.StaffFunctor(fixCost=fix, unitVariCost=20, salary=salary, unitPenalty=pen, minStaffNum=ms,
                                             maxHireNum=12, clampStaff=False, iniStaffNum=0)
                        cases.append(staff_cases.StaffCase(f"sweep{len(cases)}", f, table))
                        d = f.to_desc(T)
                        d.kernel, d.device = sia._abi.KERNEL_SEPARABLE, 0
                        descs.append(d)
                        use.append([g] * T)
    assert len(cases) == 64
    pool = [(table[0], None) for table in tabs]  # one table per rate for the four periods, as the sweep's views
    with sia.StaffBatch(descs, pool, use, [list(c.functor.minStaffNum) for c in cases]) as b:
        assert len(b.table_ids) == 2
        pl = b.plan(T)
        assert (pl.tables, pl.states, pl.levels) == (2, 37, 49) and pl.blocks == 2 * -(-32 // pl.r)
        b.set_profiling(True)
        b.solve()
        ini_v, ini_a = b.initial()
        cells = 0
        for i, c in enumerate(cases):
            V, pol, n = handle_tables(sia, c)
            cells += n
            assert_instance(b, i, c, V, pol)
            assert ini_v[i] == V[1][0] and ini_a[i] == pol[0][0], i  # (period 1 holds the one state iniStaffNum)
        st = b.stats()
        assert (st.instances, st.period_launches, st.cells_evaluated) == (64, 2 * T, cells)
        assert st.solve_ms > 0 and all(b.period_ms(t) > 0 for t in range(1, T + 1))


def _six(sia):
    """Five instances on table A and one on table B: with an instance block of 4 a full block, a part-filled one and a lone
    instance; with single instances still the cross-group indexing case."""
    a = staff_cases.staff_testing_small()
    tb = sia.staff_level_pmf([0.55] * a.T, 13)
    costs = [(50, 5, 250, [4, 9, 6, 3]), (10, 7.5, 40, [2, 2, 2, 2]), (0, 5, 250, [9, 1, 9, 1]), (300, 1, 90, [4, 9, 6, 3]),
             (50, 5, 2200, [0, 3, 6, 12])]
    cases = [variant(a, f"a{i}", fixCost=k, salary=s, unitPenalty=p, minStaffNum=ms) for i, (k, s, p, ms) in enumerate(costs)]
    lone = staff_cases.StaffCase("b0", dataclasses.replace(a.functor, fixCost=75, minStaffNum=[5, 5, 7, 7]), tb)
    return cases[:3] + [lone] + cases[3:]  # (the lone instance sits in the middle of the caller's order)


def test_short_blocks_and_instance_order(sia):
    cases = _six(sia)
    ref = [handle_tables(sia, c) for c in cases]
    for order in (list(range(6)), list(range(5, -1, -1))):
        with make_batch(sia, [cases[k] for k in order]) as b:
            pl = b.plan(2)
            assert pl.tables == 2 and pl.blocks == -(-5 // pl.r) + 1
            b.solve()
            for i, k in enumerate(order):
                assert_instance(b, i, cases[k], ref[k][0], ref[k][1])


def test_a_table_per_period(sia):
    """staff_rates' three rates as three pool tables; one instance walks them (0, 1, 2), the other (2, 1, 0): every period has
    two groups of one, and a table serves different periods of different instances."""
    c = staff_cases.staff_rates()
    rates = [0.1, 0.6, 0.35]
    pool = [(sia.staff_level_pmf([r], 41)[0], None) for r in rates]
    f0 = c.functor
    f1 = dataclasses.replace(c.functor, fixCost=3.0, unitVariCost=0.5, salary=1.0, unitPenalty=20.0, minStaffNum=[7, 7, 1])
    descs = []
    for f in (f0, f1):
        d = f.to_desc(3)
        d.kernel, d.device = sia._abi.KERNEL_SEPARABLE, 0
        descs.append(d)
    use = [[0, 1, 2], [2, 1, 0]]
    with sia.StaffBatch(descs, pool, use, [list(f0.minStaffNum), list(f1.minStaffNum)]) as b:
        assert [b.plan(t).tables for t in (1, 2, 3)] == [2, 1, 2]
        b.solve()
        for i, f in enumerate((f0, f1)):
            hc = staff_cases.StaffCase(f"rates{i}", f, sia.staff_level_pmf([rates[k] for k in use[i]], 41))
            V, pol, _ = handle_tables(sia, hc)
            assert_instance(b, i, hc, V, pol)


def test_many_waves_and_a_part_filled_last_one(sia):
    """clamped_mid: 5260 levels = 82 waves and 12 lanes; three instances of different costs and minStaffNum in one group."""
    c = _mid()
    cases = [c, variant(c, "mid1", fixCost=500.0, salary=1.0, minStaffNum=[400, 1200, 958]),
             variant(c, "mid2", unitVariCost=0.0, unitPenalty=3.5, minStaffNum=[873, 0, 4000])]
    with make_batch(sia, cases) as b:
        pl = b.plan(1)
        assert (pl.tables, pl.levels, pl.states) == (1, 5260, 4160) and pl.g_tasks == pl.blocks * 83
        b.solve()
        for i, k in enumerate(cases):
            V, pol, _ = handle_tables(sia, k)
            assert_instance(b, i, k, V, pol)


def test_lanes_of_unequal_row_length(sia):
    """long_rows: full binomial rows -- the lanes of the first waves walk rows of 1 .. 396 steps (the guarded trips), the rest
    the unguarded ones."""
    c = sb.long_rows()
    cases = [c, variant(c, "long1", fixCost=5.0, salary=12.0, unitPenalty=90.0, minStaffNum=[300, 2000])]
    with make_batch(sia, cases) as b:
        assert b.plan(1).longest_row == 396
        b.solve()
        for i, k in enumerate(cases):
            V, pol, _ = handle_tables(sia, k)
            assert_instance(b, i, k, V, pol)


@pytest.mark.parametrize("make", [_mid, sb.long_rows], ids=["clamped_mid", "long_rows"])
def test_a_full_and_a_short_instance_block_at_many_waves(sia, make):
    """Five instances of one group: with an instance block of four, a full block and a short one whose spare slots store
    nothing, over many waves and over lanes of unequal row length."""
    c = make()
    T = c.T
    cases = [c] + [variant(c, f"v{k}", fixCost=10.0 * k, salary=1.5 * k, unitPenalty=30.0 + 7 * k,
                           minStaffNum=[(300 * k + 450 * t) % 1900 for t in range(T)]) for k in range(1, 5)]
    with make_batch(sia, cases) as b:
        pl = b.plan(1)
        assert pl.tables == 1 and pl.blocks == -(-5 // pl.r)
        b.solve()
        for i, k in enumerate(cases):
            V, pol, _ = handle_tables(sia, k)
            assert_instance(b, i, k, V, pol)


def test_two_ping_pong_tables(sia):
    """store_all_values = 0: V_1 and V_2 survive and equal the handle's, later periods are refused as the F1 batch refuses
    them; the policies of all periods are kept."""
    a = staff_cases.staff_testing_small()
    cases = [a, variant(a, "pp1", fixCost=0.0, salary=9.0, minStaffNum=[1, 1, 12, 3])]
    with make_batch(sia, cases, store_all=0) as b:
        b.solve()
        for i, c in enumerate(cases):
            V, pol, _ = handle_tables(sia, c, store_all=0)
            for t in (1, 2):
                assert np.array_equal(b.values(i, t), V[t]), (i, t)
            for t in range(1, c.T + 1):
                assert np.array_equal(b.policy(i, t), pol[t - 1]), (i, t)
            for t in (3, 4):
                with pytest.raises(sia.SdpgpuError) as e:
                    b.values(i, t)
                assert e.value.code == 2 and f"V_{t}" in e.value.message and "overwritten" in e.value.message


def test_ties_inside_a_batch_are_the_oracles_bits(sia, staffref):
    """fixCost = unitVariCost = salary = 0: nothing is reassociated, and the strict compare keeps the first of the equal actions
    -- with neighbours of other costs in the same instance block."""
    c = _mid()
    t = sb.ties()
    cases = [c, staff_cases.StaffCase("ties", t.functor, c.table, c.row_len), variant(c, "mid1", fixCost=500.0, minStaffNum=[400, 1200, 958])]
    assert np.array_equal(t.table, c.table) and np.array_equal(t.row_len, c.row_len)  # (the same construction: one group)
    V, pol, _ = t.oracle_problem(staffref).solve(nthreads=8)
    with make_batch(sia, cases) as b:
        assert b.plan(1).tables == 1
        b.solve()
        for p in range(1, t.T + 1):
            assert np.array_equal(b.values(1, p), V[p - 1]) and np.array_equal(b.policy(1, p), pol[p - 1]), p


def test_staff_recursion_batch(sia):
    a = staff_cases.staff_testing_small()
    cases = [a, variant(a, "rb1", fixCost=400.0, salary=2.0, unitPenalty=80.0, minStaffNum=[6, 2, 9, 4])]
    want = []
    for c in cases:
        rec = sia.StaffRecursion(pmf=c.table, T=c.T, functor=c.functor, device=0, separable=True)
        try:
            states = [sia.StaffState(1, 0), sia.StaffState(2, 7), sia.StaffState(4, 30)]
            want.append(([rec.getExpectedValue(s) for s in states], [rec.getAction(s) for s in states], rec.getOptTable()))
        finally:
            rec.close()
    with sia.StaffRecursionBatch([c.functor for c in cases], [c.table for c in cases], a.T, device=0) as rb:
        assert rb.num_tables == a.T  # (one array handed to both instances: its four period slices)
        for i, (vals, acts, table) in enumerate(want):
            assert [rb.getExpectedValue(i, s) for s in states] == vals, i
            assert [rb.getAction(i, s) for s in states] == acts, i
            assert np.array_equal(rb.getOptTable(i), table), i
        v, h = rb.initial()
        assert [float(x) for x in v] == [w[0][0] for w in want] and [int(x) for x in h] == [w[1][0] for w in want]
