"""The CPU twin of the level kernel's cut-off (tests/level_cut_twin.py) against the oracle, and the conditions the grids of
the GPU tests have to meet -- all of it host arithmetic, no GPU.

The twin really skips the steps of a stopped block, so its tables being the oracle's, bit for bit, is the soundness argument
of sdp_window.hpp ("THE CUT-OFF") checked in fp64 on the CPU.  Its step counts are recorded in level_cut_twin.py; the GPU
tests hold the device counters against the same figures, so a kernel that stops a block later than it could (or earlier,
without changing a table of these grids) does not pass them."""
import numpy as np
import pytest

import level_cut_twin as twin
import test_level_cutoff as tc
from stochastic_inventory_amd import workloads
from stochastic_inventory_amd.functors import BackorderFunctor
from stochastic_inventory_amd.states import OptDirection

_CACHE = {}


def _workload(c):
    return tc._grid(c["S"], c["A"], c["D"], T=c["T"], lo=c["lo"], K=c["K"], v=c["v"], h=c["h"], pi=c["pi"])


def _plan(sia, w, monkeypatch):
    for k in tc._SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDPGPU_WIN_LEVEL", "1")
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        return eng.plan(1)


def _solved(sia, oracle, monkeypatch, key, w):
    """(twin of every period, the oracle's values and policies) of a workload, computed once per session."""
    if key not in _CACHE:
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
        _CACHE[key] = (twin.twin_solve(w, _plan(sia, w, monkeypatch), V), V, pol)
    return _CACHE[key]


def _assert_oracle_tables(t, V, pol, name):
    for period, p in enumerate(t.periods, start=1):
        assert np.array_equal(p.values, V[period - 1]), f"{name}: values of period {period}"
        assert np.array_equal(p.policy, pol[period - 1]), f"{name}: policy of period {period}"


def _tie_workloads():
    """The two tie instances of test_level_cutoff.py (no ordering cost, h = pi = 1, flat pmf stretches)."""
    f = BackorderFunctor(fixedOrderingCost=0, variOrderingCost=0, holdingCost=1, penaltyCost=1, minInventory=0,
                         maxInventory=1199, maxOrderQuantity=399, iniInventory=0)
    flat = [np.column_stack([np.arange(8.0), np.full(8, 0.125)]) for _ in range(3)]
    stop = [np.column_stack([np.arange(24.0), np.full(24, 1.0 / 32)]) for _ in range(3)]
    for t in stop:
        t[:8, 1] = 2.0 / 32
    return [workloads.Workload("cut_ties_1200x400x8x3", f, OptDirection.MIN, flat, "ties"),
            workloads.Workload("cut_ties_1200x400x24x3", f, OptDirection.MIN, stop, "ties, blocks stop")]


@pytest.mark.parametrize("c", twin.ONE_BLOCK_GRIDS + twin.MULTI_BLOCK_GRIDS, ids=lambda c: c["id"])
def test_twin_tables_are_the_oracles_and_its_counts_the_recorded_ones(sia, oracle, monkeypatch, c):
    """Every grid of the GPU cut-off tests: the twin, which skips what the kernel skips, leaves the oracle's tables; its
    steps run per period are the figures recorded next to the grid, and its planned steps the host's formula."""
    w = _workload(c)
    t, V, pol = _solved(sia, oracle, monkeypatch, c["id"], w)
    print(f"{w.name}: band {t.band}, {t.blocks_per_task} blocks per task, steps run {[p.run for p in t.periods]} of "
          f"{[p.planned for p in t.periods]}: walked {t.walked:.4f}, carried-over share {t.carried_share:.3f}")
    _assert_oracle_tables(t, V, pol, w.name)
    assert t.blocks_per_task == c["blocks"]
    assert [p.run for p in t.periods] == c["run"]
    assert all(p.planned == twin.planned_steps(c["S"], c["A"], t.band, t.n_ablocks, t.d_pad) for p in t.periods)


def test_twin_on_the_tie_instances(sia, oracle, monkeypatch):
    """Exact ties between actions of one state, where nothing stops and where blocks do stop: the lowest action everywhere."""
    flat, stop = _tie_workloads()
    for w in (flat, stop):
        t, V, pol = _solved(sia, oracle, monkeypatch, w.name, w)
        _assert_oracle_tables(t, V, pol, w.name)
    assert _CACHE[flat.name][0].run == _CACHE[flat.name][0].planned
    assert _CACHE[stop.name][0].run < _CACHE[stop.name][0].planned


def test_walked_fractions_of_the_one_block_grids(sia, oracle, monkeypatch):
    """The share of the steps walked on the four grids of test_cutoff_fires_and_changes_nothing.  That test's docstring quotes
    0.51 / 0.58 / 0.89 / 0.82 from an emulation of an earlier, similar schedule; the kernel's own schedule gives 0.5842 /
    0.6049 / 0.8942 / 0.7778 -- the twin here, and the device counters (profiles/f1_cutoff_ab.txt, section B, and
    test_cutoff_steps_are_the_twins_on_one_block_grids).  The first stays under that test's cap of 0.75."""
    got = []
    for c in twin.ONE_BLOCK_GRIDS:
        t, _, _ = _solved(sia, oracle, monkeypatch, c["id"], _workload(c))
        print(f"{c['id']}: walked {t.run} of {t.planned} = {t.walked:.4f}")
        got.append((t.run, t.planned))
    assert got == [(184368, 315600), (21776, 36000), (4464, 4992), (32256, 41472)]
    assert [round(r / p, 4) for r, p in got] == [0.5842, 0.6049, 0.8942, 0.7778]


@pytest.mark.parametrize("c", twin.MULTI_BLOCK_GRIDS, ids=lambda c: c["id"])
def test_multi_block_grids_carry_the_schedule_over(sia, oracle, monkeypatch, c):
    """What a grid must show on the CPU before a GPU test may rest on it: at least four level blocks per task, at most 0.9 of
    the steps walked, at least a tenth of the stopped blocks second-or-later blocks of their task, and a task in which a
    block runs to the end after an earlier one stopped (the path that re-arms cut_once)."""
    t, _, _ = _solved(sia, oracle, monkeypatch, c["id"], _workload(c))
    assert t.band >= 32 and t.blocks_per_task >= 4
    assert t.walked <= 0.9
    assert t.carried_share >= 0.1
    assert t.rearmed_tasks >= 1
    assert all((p.tests > 0).all() for p in t.periods)


def test_multi_block_grids_cover_the_paths_asked_for(sia, oracle, monkeypatch):
    """Among the grids: a ragged last band whose level blocks address slots past its states, stops in the second product
    table of a band of several blocks, a third action block with one real lane, a slab a third of which lies below zero."""
    by_id = {c["id"]: c for c in twin.MULTI_BLOCK_GRIDS}
    c = by_id["40000x300x24"]
    t, _, _ = _solved(sia, oracle, monkeypatch, c["id"], _workload(c))
    last = (c["S"] + c["A"] - 1) % t.band
    assert last % twin.LV != 0 and -(-last // twin.LV) > 1     # ragged, and more than one block in the ragged band
    c = by_id["25000x300x100"]
    t, _, _ = _solved(sia, oracle, monkeypatch, c["id"], _workload(c))
    assert t.d_pad > 64 and all(p.stopped_second_table >= 100 for p in t.periods)
    assert all(sum(n for s, n in p.stop_hist.items() if s < 64) >= 100 for p in t.periods)
    c = by_id["30000x513x24"]
    assert c["A"] - 2 * twin.NA == 1
    c = by_id["36000x300x32-deep"]
    t, _, _ = _solved(sia, oracle, monkeypatch, c["id"], _workload(c))
    tasks = t.periods[0].steps.size
    assert c["lo"] <= -c["S"] // 3
    assert all(p.never_stopped_tasks >= tasks // 4 and p.always_stopped_tasks >= tasks // 4 for p in t.periods)


@pytest.mark.parametrize("switch,case_id", [("slot_shift", "50000x64x17"), ("keep_once", "50000x64x17"), ("edge_fill", "26000x257x9")])
def test_step_count_tells_a_wrong_schedule_apart(sia, oracle, monkeypatch, switch, case_id):
    """The twin with one of the kernel's three details wrong -- the test reads the neighbouring slot, cut_once is not cleared
    after a stopped block, slots outside the slab start at a neighbouring state's U instead of -inf -- walks another number
    of steps on these grids (and may well leave the same tables): what the exact count of the GPU tests is for."""
    c = {c["id"]: c for c in twin.MULTI_BLOCK_GRIDS}[case_id]
    w = _workload(c)
    _, V, _ = _solved(sia, oracle, monkeypatch, c["id"], w)
    wrong = twin.twin_solve(w, _plan(sia, w, monkeypatch), V, **{switch: {"slot_shift": 1, "keep_once": True, "edge_fill": "U"}[switch]})
    print(f"{case_id} with {switch}: {wrong.run} steps against {sum(c['run'])}")
    if switch == "slot_shift":
        assert wrong.run != sum(c["run"])
    else:
        assert wrong.run > sum(c["run"])   # (either can only hold a block back)
