"""The staff family's launch plan (plan_staff in csrc/sdpgpu_staff.hip, reported through sdpgpu_plan_period): which kernel
form serves a period, its state tiles, action groups and the trips of the action loop per group.  Host arithmetic only, no
GPU.  This file states what tests/test_gpu_staff_blocks.py reaches that tests/test_gpu_staff.py does not: every
register-blocked form with a second trip of its `a0` loop, ragged ends together, window waves that run the staged and the
scalar path in one loop -- read from the library's own plan, never from a restatement of its group arithmetic."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import staff_block_cases as sb  # noqa: E402
import staff_cases  # noqa: E402
import test_gpu_staff as tgs  # noqa: E402

# two buffers x S residue classes x ceil((64 S + 4 + S - 2) / S) + 7 = 73 slots of doubles
WINDOW_LDS = {"win2": 2 * 2 * 73 * 8, "win4": 2 * 4 * 73 * 8}


@functools.lru_cache(maxsize=None)
def _case(name):
    return getattr(sb, name)()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import staffref
    staffref.build()
    return _case(name).oracle_problem(staffref).solve(nthreads=8)


def _geometries(sia, monkeypatch, c, env, world=1, rank=0, periods=None):
    sb.set_switches(monkeypatch, env)
    with sb.engine(sia, c, rank, world) as eng:
        return [sb.Geometry(eng, c, t) for t in (periods or range(1, c.T + 1))]


@functools.lru_cache(maxsize=None)
def _all_plans():
    """{(instance, switch set): [Geometry per period]} of the instances and switch sets of tests/test_gpu_staff_blocks.py."""
    import stochastic_inventory_amd as sia
    mp = pytest.MonkeyPatch()
    try:
        return {(make.__name__, label): _geometries(sia, mp, _case(make.__name__), env)
                for make in sb.ALL for label, env in sb.switch_sets(_case(make.__name__)).items()}
    finally:
        mp.undo()


def _todays_shapes():
    """(case, environment) of every launch shape of tests/test_gpu_staff.py, as that file sets the switches."""
    from stochastic_inventory_amd.pmf import staff_level_pmf
    pair, win4, win2 = {"SDPGPU_STAFF_PAIR": "1"}, {"SDPGPU_STAFF_PAIR": "1", "SDPGPU_STAFF_WIN": "4"}, {"SDPGPU_STAFF_PAIR": "1", "SDPGPU_STAFF_WIN": "2"}
    lanes = {"SDPGPU_STAFF_LANES": "1"}
    named = [m() for m in staff_cases.ALL]
    f = staff_cases.StaffFunctor(fixCost=100, unitVariCost=10, salary=20, unitPenalty=80, minStaffNum=[40, 40, 40], maxHireNum=500,
                                 minX=0, maxX=600, clampStaff=True, iniStaffNum=0)
    named.append(staff_cases.StaffCase("workforce_planning_main", f, staff_level_pmf([0.5, 0.5, 0.5], 601)))
    out = [(c, {}) for c in named] + [(_staff_forms(), env) for env in ({}, {"SDPGPU_STAFF_UNI": "0"}, {"SDPGPU_STAFF_UNI": "0", "SDPGPU_STAFF_WIN": "0", "SDPGPU_STAFF_LANES": "0"})]
    out += [(tgs._random_case(s), {}) for s in range(60)]
    out += [(c, env) for env in (pair, win4, win2, lanes) for c in named[:-1]]
    out += [(tgs._random_case(s), pair) for s in range(100, 140)]
    out += [(tgs._random_case(s), env) for env in (win4, win2) for s in range(200, 260)]
    out += [(tgs._random_case(s), lanes) for s in range(300, 340)]
    out += [(tgs._random_case(s, ragged=True), env) for env in tgs.RAGGED_FORMS for s in range(400, 424)]
    return out


def _staff_forms():
    """The instance of test_kernel_forms_chosen_by_range_size: staff ranges of 1, 601, 1201 and 1801 numbers."""
    f = staff_cases.StaffFunctor(fixCost=50, unitVariCost=20, salary=5, unitPenalty=250, minStaffNum=[40, 90, 60, 30], maxHireNum=600,
                                 clampStaff=False, iniStaffNum=0)
    return staff_cases.StaffCase("staff_forms", f, staff_cases.staff_level_pmf([0.3] * 4, 601))


def test_every_switch_set_reports_the_form_it_is_meant_to_reach():
    for (name, label), geos in _all_plans().items():
        c = _case(name)
        for period, g in enumerate(geos, start=1):
            assert (g.form, g.chunk_blocks) == sb.expected(c, label, period), (name, label, period)
            assert g.plan.lds_bytes == WINDOW_LDS.get(g.form, 0), (name, label, period)
            if label not in ("auto", "win4_staged") and g.states > 16:  # (at most 16 states: lanes are actions unless plain is forced)
                assert g.form == label, (name, label, period)


def test_left_alone_the_form_follows_the_staff_range(sia, monkeypatch):
    """One state: lanes are actions; 256 numbers and more: two states per lane from the window; 1536 and more: four.  The
    growing instance (1, 2101, ... 8401 numbers) crosses the first and the last; the 1500 numbers of few_states and the
    601 / 1201 of test_kernel_forms_chosen_by_range_size's instance run two per lane."""
    assert [g.form for g in _all_plans()[("growing", "auto")]] == ["lanes", "win4", "win4", "win4", "win4"]
    assert [g.states for g in _all_plans()[("growing", "auto")]] == [1, 2101, 4201, 6301, 8401]
    assert [g.form for g in _all_plans()[("few_states", "auto")]] == ["win2", "win2"]
    assert [g.form for g in _geometries(sia, monkeypatch, _staff_forms(), {})] == ["lanes", "win2", "win2", "win4"]


def test_every_register_blocked_form_has_a_second_trip():
    reached = {}
    for (name, label), geos in _all_plans().items():
        for g in geos:
            if g.chunk_blocks >= 2:
                reached.setdefault(g.form, set()).add((name, label))
    for form in sb.REGISTER_BLOCKED:
        assert reached.get(form), form
    # the window forms also by the launcher's own choice
    assert any(label == "auto" for _, label in reached["win4"]) and any(label == "auto" for _, label in reached["win2"])
    # and the plain kernel walks a group's actions one by one
    assert reached.get("plain")


def test_ragged_group_block_and_tile_together():
    """A ragged last group whose last block is partial, on a ragged last tile, in a plan with two trips and more."""
    for form in sb.REGISTER_BLOCKED:
        assert any(g.form == form and g.chunk_blocks >= 2 and g.ragged_ends() for geos in _all_plans().values() for g in geos), form


def test_window_waves_that_run_the_staged_and_the_scalar_path():
    """(tile, group) pairs whose first block lies below the table's last row and a later one on or beyond it."""
    count = {"win2": 0, "win4": 0}
    for geos in _all_plans().values():
        for g in geos:
            if g.form in count:
                count[g.form] += g.mixed_waves()
    assert count["win2"] >= 1 and count["win4"] >= 1, count
    auto = _all_plans()[("clamped_wide", "auto")][-1], _all_plans()[("few_states", "auto")][-1]
    assert auto[0].form == "win4" and auto[0].mixed_waves() >= 1 and auto[1].form == "win2" and auto[1].mixed_waves() >= 1


def test_the_shapes_of_test_gpu_staff_have_one_trip_and_no_mixed_wave(sia, monkeypatch):
    """The statement of the gap: every launch of tests/test_gpu_staff.py -- named cases, WorkforcePlanning.main's size, the
    run across the forms, every fuzz seed under its switches -- walks ONE register block per group, so no window wave there
    changes path inside its loop."""
    n = 0
    for c, env in _todays_shapes():
        for g in _geometries(sia, monkeypatch, c, env):
            if g.form != "plain":  # (one action a trip: its groups of 4 are four trips of a loop with nothing to carry but best)
                assert g.chunk_blocks == 1, (c.name, env, g.form)
            assert g.mixed_waves() == 0, (c.name, env)
            n += 1
    assert n > 1000


def test_slabs_keep_two_trips(sia, monkeypatch):
    """Slabs are shorter, so a tile gets more groups: world = 3 slabs of clamped_wide keep two trips under the block kernel;
    under the pair kernel and the window with two states per lane (128-state tiles) world = 3 falls to one trip on every rank
    and world = 2 keeps two; with four states per lane no slab does."""
    c = _case("clamped_wide")
    for label, world in sb.SLABS:
        for rank in range(world):
            g, = _geometries(sia, monkeypatch, c, sb.SWITCH_SETS[label], world, rank, periods=[c.T])
            assert g.form == label and g.chunk_blocks >= 2, (label, world, rank)
    for label in ("win2", "pair"):
        g, = _geometries(sia, monkeypatch, c, sb.SWITCH_SETS[label], 3, 1, periods=[c.T])
        assert g.chunk_blocks == 1
    g, = _geometries(sia, monkeypatch, c, sb.SWITCH_SETS["win4"], 2, 1, periods=[c.T])
    assert g.chunk_blocks == 1


def test_switches_are_read_per_engine(sia, monkeypatch):
    """Every SDPGPU_STAFF_* value set between two engines of one process takes effect on the second and leaves the first alone."""
    c = _case("few_states")
    sb.set_switches(monkeypatch, {})
    first = sb.engine(sia, c)
    try:
        assert sb.form_of(first.plan(c.T)) == "win2"
        for env, form in (({"SDPGPU_STAFF_WIN": "4"}, "win4"), ({"SDPGPU_STAFF_WIN": "0"}, "pair"), ({"SDPGPU_STAFF_PAIR": "0"}, "block4"),
                          ({"SDPGPU_STAFF_PAIR": "0", "SDPGPU_STAFF_R": "8"}, "block8"), ({"SDPGPU_STAFF_BLOCK": "0"}, "plain"),
                          ({"SDPGPU_STAFF_LANES": "1"}, "lanes"), ({"SDPGPU_STAFF_BLOCK": "1", "SDPGPU_STAFF_R": "4"}, "win2")):
            sb.set_switches(monkeypatch, env)
            with sb.engine(sia, c) as eng:
                assert sb.form_of(eng.plan(c.T)) == form, env
            assert sb.form_of(first.plan(c.T)) == "win2", env
    finally:
        first.close()


@pytest.mark.parametrize("name", [m.__name__ for m in sb.MAIN])
def test_best_actions_fall_in_first_and_in_later_blocks(name):
    """What a second trip has to carry is `best`: the instances are only worth their time if the oracle's best action lies in
    a later block of its group for many states and in the first for many.  A state at or below minStaffNum hires up to a fixed
    level, so the hires of a period take some 900 distinct values, spread evenly over the positions in a group; the others
    hire nobody (action 0, first block of the first group).  Asserted for every plan with two trips and more: of the states
    that hire, at least a quarter have their best action in a later block (pol % group_actions >= r), and at least 40 of them
    in the first (evenly spread that is one in chunk_blocks, 45 of 900 at the plain kernel's 20); of all states, at least a
    quarter have it in the first block."""
    c = _case(name)
    _, pol, _ = _oracle(name)
    for period in range(1, c.T + 1):
        if len(pol[period - 1]) > 1:
            assert len(np.unique(pol[period - 1])) >= 800, (name, period)
    checked = 0
    for (n, label), geos in _all_plans().items():
        if n != name:
            continue
        for period, g in enumerate(geos, start=1):
            p = pol[period - 1]
            if g.chunk_blocks < 2 or len(p) == 1:  # (the one state of a run's first period)
                continue
            first, later, hiring = g.block_shares(p)
            assert later >= 0.25 and first * hiring >= 40, (name, label, period, first, later, hiring)
            assert np.count_nonzero(p % g.group_actions < g.r) >= len(p) / 4, (name, label, period)
            checked += 1
    assert checked >= 2


@pytest.mark.parametrize("name,states,distinct,form", [("ties", 2752, 1101, "block4"), ("ties_wide", 5289, 2101, "win4")])
def test_ties_closed_form_on_the_oracle(name, states, distinct, form):
    """K = v = salary = 0: all actions from the first whose level clears minStaff + cap - 1 cost exactly +0.0, and the strict
    compare keeps that first one wherever the hire limit allows it -- at every position of a group's blocks, evenly."""
    c = _case(name)
    V, pol, _ = _oracle(name)
    want, ok = sb.ties_closed_form(c)
    assert ok.sum() == states and np.array_equal(pol[-1][ok], want[ok]) and not V[-1][ok].any()
    assert len(np.unique(pol[-1][ok])) == distinct
    g = _all_plans()[(name, form)][-1]
    pos = np.bincount(pol[-1][ok][want[ok] > 0] % g.group_actions, minlength=g.group_actions)
    assert g.form == form and g.chunk_blocks == 2 and pos.min() >= 130


@pytest.mark.parametrize("name", ["ragged_rows", "ragged_wide"])
def test_ragged_rows_are_ragged_and_the_oracle_never_reads_behind_them(name):
    c = _case(name)
    steps = np.diff(c.row_len)
    assert (steps < 0).sum() >= 1000 and (steps > 0).sum() >= 1000
    j = np.arange(c.table.shape[2])[None, :]
    assert np.isnan(c.table[0][j >= c.row_len[:, None]]).all() and np.isfinite(c.table[0][j < c.row_len[:, None]]).all()
    V, _, _ = _oracle(name)
    assert all(np.isfinite(v).all() for v in V)
