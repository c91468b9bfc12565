"""The STAFF family's opt-in separable mode on the device (csrc/sdp_staff_sep.hpp: one G(y) row per period, then a scan).

Its parity statement (include/sdpgpu.h): tables BIT-IDENTICAL to tests/staff_separable_twin.py -- checked period by period,
the twin fed the device's own V_{t+1}, so a failure names its period; an instance with fixCost = unitVariCost = salary = 0 is
bit-identical to the ORACLE.  (That the twin is within 1e-9 of the oracle, differing in the hire count only on ties to that
rounding, is tests/test_staff_separable_twin.py, on the CPU.)  Every other `kernel` value keeps the cell-by-cell kernels."""
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
    """70 staff numbers x 41 hires over rows of lengths drawn from 1 .. min(y + 1, 9), NaN behind every row's length."""
    table, row_len = sb.ragged_table(0.01, 60, 9, 2, seed=22)
    assert np.isnan(table).any()
    return staff_cases.StaffCase("ragged_small", sb._functor([20, 31], 40, 69), table, row_len)


# the smallest sizes at which each thing can break
CASES = {
    "staff_single": staff_cases.staff_single,                # 1 state, 1 action, 1 period
    "staff_testing_small": staff_cases.staff_testing_small,  # unclamped growing boxes, the last-row clamp, one state in period 1
    "staff_short_rows": staff_cases.staff_short_rows,        # row_len
    "staff_wide_actions": staff_cases.staff_wide_actions,    # 301 actions: further trips of the 4-stride loop; 91 states: a part-filled second tile
    "ragged_small": ragged_small,                            # NaN behind row ends must not reach G or P
    "clamped_mid": sb.clamped_mid,                           # 5260 levels: many G workgroups
    "long_rows": sb.long_rows,                               # step loops of hundreds of steps, lanes of unequal length in one wave
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


def _engine(sia, c, kernel, rank=0, world=1):
    d = c.functor.to_desc(c.T)
    d.kernel, d.rank, d.world_size, d.device = kernel, rank, world, 0
    return sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len)


def _assert_twin_bits(sia, staffref, c):
    P = c.oracle_problem(staffref)
    with _engine(sia, c, sia._abi.KERNEL_SEPARABLE) as eng:
        eng.solve(sync=True)
        assert eng.stats().kernel_used == 3
        V = [eng.values(t) for t in range(1, c.T + 1)]
        pol = [eng.policy(t) for t in range(1, c.T + 1)]
    for t in range(c.T, 0, -1):
        assert len(V[t - 1]) == int(P.nx[t - 1]), (c.name, t)
        tv, tp, _, _ = twin.period(c, P, t, V[t] if t < c.T else None)
        assert np.isfinite(V[t - 1]).all(), (c.name, t)
        assert np.array_equal(V[t - 1], tv), (c.name, t, int(np.count_nonzero(V[t - 1] != tv)))
        assert np.array_equal(pol[t - 1], tp), (c.name, t, int(np.count_nonzero(pol[t - 1] != tp)))
    return V, pol


@pytest.mark.parametrize("name", list(CASES))
def test_tables_are_the_twins_bits(sia, staffref, name):
    _assert_twin_bits(sia, staffref, _case(name))


def test_ties_are_the_oracles_bits(sia, staffref):
    """fixCost = unitVariCost = salary = 0: nothing is reassociated, the strict compare keeps the first of the equal actions."""
    c = sb.ties()
    V, pol, _ = c.oracle_problem(staffref).solve(nthreads=8)
    with _engine(sia, c, sia._abi.KERNEL_SEPARABLE) as eng:
        eng.solve(sync=True)
        assert eng.stats().kernel_used == 3
        for t in range(1, c.T + 1):
            assert np.array_equal(eng.values(t), V[t - 1]) and np.array_equal(eng.policy(t), pol[t - 1]), t


def test_rank_slabs(sia):
    """Three ranks of one device through sdpgpu_solve_multi: each builds the levels its slab reaches and scans its slab; every
    rank's whole value tables and its piece of the policy equal the single-rank separable tables."""
    c = _case("staff_wide_actions")
    with _engine(sia, c, sia._abi.KERNEL_SEPARABLE) as one:
        one.solve(sync=True)
        V = [one.values(t) for t in range(1, c.T + 1)]
        pol = [one.policy(t) for t in range(1, c.T + 1)]
    engs = []
    try:
        for r in range(3):
            engs.append(_engine(sia, c, sia._abi.KERNEL_SEPARABLE, r, 3))
        sia.SdpEngine.solve_multi(engs, gather_first=True)  # (V_1 travels too: every rank's whole tables are compared)
        for e in engs:
            assert e.stats().kernel_used == 3
            for t in range(1, c.T + 1):
                _, lo, hi = e.slab(t)
                assert np.array_equal(e.values(t), V[t - 1]), t
                assert np.array_equal(e.policy(t), pol[t - 1][lo:hi]), t
    finally:
        for e in engs:
            e.close()


def test_fuzz_is_the_twins_bits(sia, staffref):
    for c in twin.fuzz_cases()[:20]:
        _assert_twin_bits(sia, staffref, c)


def test_mirror_class_separable(sia):
    """StaffRecursion(separable=True) on an instance without a policy mismatch: getAction, getOptTable and the rollouts of the
    table and of a level rule equal the AUTO handle's exactly; getExpectedValue under the mode's own parity statement, 1e-9
    relative -- the reassociated sum of the initial state is 1255.576333806713 against the oracle's 1255.5763338067127, one
    unit in the last place (tests/staff_separable_twin.py gives the same bits on the CPU)."""
    c = staff_cases.staff_planning_small()
    f = c.functor
    initial = sia.StaffState(1, f.iniStaffNum)
    ss = np.array([[m + 2.0, m + 7.0] for m in f.minStaffNum])
    got = {}
    for separable in (False, True):
        rec = sia.StaffRecursion(pmf=c.table, T=c.T, functor=f, device=0, separable=separable)
        try:
            value, action, table = rec.getExpectedValue(initial), rec.getAction(initial), rec.getOptTable()
            assert rec.engine.stats().kernel_used == (3 if separable else 1)
            sim = sia.SimulatesS(rec, c.T, [0.5] * c.T)
            got[separable] = (value, action, table, sim.simulateTable(initial), sim.simulatesS(initial, ss))
        finally:
            rec.close()
    (v0, a0, t0, st0, sr0), (v1, a1, t1, st1, sr1) = got[False], got[True]
    assert abs(v1 - v0) <= 1e-9 * abs(v0)
    assert a1 == a0 and np.array_equal(t1, t0)
    assert st1 == st0 and sr1 == sr0  # (the rollouts read the policy table and the lambdas, not the value tables)


@pytest.mark.parametrize("kernel", [0, 1], ids=["auto", "gather"])
def test_other_kernel_values_stay_cell_by_cell(sia, staffref, kernel):
    c = staff_cases.staff_rates()
    V, pol, _ = c.oracle_problem(staffref).solve()
    with _engine(sia, c, kernel) as eng:
        eng.solve(sync=True)
        assert eng.stats().kernel_used == 1
        for t in range(1, c.T + 1):
            assert np.array_equal(eng.values(t), V[t - 1]) and np.array_equal(eng.policy(t), pol[t - 1]), t
