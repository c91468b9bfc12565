"""GPU parity of the STAFF family's kernel forms where a group's action loop has a second trip (tests/staff_block_cases.py):
every period's value table and policy bit for bit against oracle/staffref.c, and the cell count, under every switch set --
the launcher's own choice, the window with four and two states per lane (with and without its scalar-probability path), the
pair kernel, the block kernel with 4 and 8 actions per register block, the plain kernel.  What a second trip depends on --
best / bestk carried across blocks under the strict first-best compare, the re-armed rings, the window's barrier before the
next block restages, a wave that changes from the staged to the scalar path, a ragged last block in a ragged last group --
is reached by no shape of tests/test_gpu_staff.py; tests/test_staff_plan.py shows both from the library's plan report.  Each
engine's plan is asserted before its tables are compared: a forced form that did not run cannot pass for free."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import staff_block_cases as sb  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _solved(name):
    """The instance and the oracle's tables, once."""
    from oracle import staffref
    staffref.build()
    c = getattr(sb, name)()
    V, pol, cells = c.oracle_problem(staffref).solve(nthreads=16)
    assert all(np.isfinite(v).all() for v in V)
    return c, V, pol, cells


def _check_all_switch_sets(sia, monkeypatch, name):
    c, V, pol, cells = _solved(name)
    for label, env in sb.switch_sets(c).items():
        sb.set_switches(monkeypatch, env)
        with sb.engine(sia, c) as eng:
            for period in range(1, c.T + 1):
                g = sb.Geometry(eng, c, period)
                assert (g.form, g.chunk_blocks) == sb.expected(c, label, period), (name, label, period)
            eng.solve(sync=True)
            assert eng.stats().cells_evaluated == cells, (name, label)
            for period in range(1, c.T + 1):
                assert np.array_equal(eng.values(period), V[period - 1]), (name, label, period)
                assert np.array_equal(eng.policy(period), pol[period - 1]), (name, label, period)


@pytest.mark.parametrize("name", [m.__name__ for m in sb.MAIN])
def test_two_trips_match_oracle(sia, monkeypatch, name):
    _check_all_switch_sets(sia, monkeypatch, name)


@pytest.mark.parametrize("name", ["ties", "ties_wide"])
def test_ties_keep_the_first_best_action(sia, monkeypatch, name):
    """All actions from the first that clears minStaff + cap - 1 cost exactly +0.0: a `<=` in a kernel's block scan, in a
    group's partial row or in combine_staff_kernel moves the policy.  (ties: 4160 x 1101, two trips under the block
    kernel only; ties_wide: two and more under every form.)"""
    c, V, pol, _ = _solved(name)
    want, ok = sb.ties_closed_form(c)
    assert ok.sum() > 2500 and np.array_equal(pol[-1][ok], want[ok]) and len(np.unique(want[ok])) == c.functor.maxHireNum + 1
    _check_all_switch_sets(sia, monkeypatch, name)


@pytest.mark.parametrize("name", ["ragged_rows", "ragged_wide"])
def test_ragged_rows_with_nan_behind_them(sia, monkeypatch, name):
    """Neighbouring levels of unequal, non-monotone lengths: per-lane step counts and the exec-mask drop-out of the block
    kernel, the longer of a pair's two rows, the window's wave-wide step count.  Behind a row's length the caller's array holds
    NaN; the oracle's tables are finite, so a NaN in the engine's is a read of something the reference does not have."""
    c = _solved(name)[0]
    assert np.isnan(c.table).any() and (np.diff(c.row_len) < 0).sum() >= 1000
    _check_all_switch_sets(sia, monkeypatch, name)


@pytest.mark.parametrize("label,world", sb.SLABS, ids=[f"{a}x{w}" for a, w in sb.SLABS])
def test_slabs_of_the_last_period(sia, monkeypatch, label, world):
    """Slabs with two trips on every rank (no exchange is needed in the last period): tiles that start inside the staff range, a
    lane's second state on the next rank."""
    c, V, pol, _ = _solved("clamped_wide")
    sb.set_switches(monkeypatch, sb.SWITCH_SETS[label])
    got = 0
    for rank in range(world):
        with sb.engine(sia, c, rank, world) as eng:
            g = sb.Geometry(eng, c, c.T)
            assert g.form == label and g.chunk_blocks >= 2, (label, world, rank)
            eng.run_period(c.T)
            _, lo, hi = eng.slab(c.T)
            assert np.array_equal(eng.values(c.T)[lo:hi], V[c.T - 1][lo:hi]), (label, rank)
            assert np.array_equal(eng.policy(c.T), pol[c.T - 1][lo:hi]), (label, rank)
            got += hi - lo
    assert got == len(V[c.T - 1])
