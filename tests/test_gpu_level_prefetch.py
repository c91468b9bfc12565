"""The prefetch slot of the F1 level kernel (window_f1_level_kernel, csrc/sdp_window.hpp, "THE PREFETCH SLOT"): the inputs of
a product table are loaded while the table before it is walked, and a table whose inputs were not the ones fetched is built
from direct loads as before.  Nothing a solve returns may depend on which of the two happened: every table with the cut-off
on, with it off, from the state-major kernel and from the oracle is the same bits, and the steps run are EXACTLY those of the
CPU twin (tests/level_cut_twin.py) -- a guess that moved a test step or a stop step would change that count.

The grids (K = 500, v = 1, pi = 10, T = 2, inventory from -300 up; band 32, four level blocks per task) differ in the tables a
block has and in where blocks stop, so that a table is met both with its inputs fetched and without:
  26000x300x200  four tables (64, 64, 64, 8 steps), stops in every one: both outcomes of the guess
  26000x300x130  three tables, stops on a table boundary (a multiple of 64)
  26000x300x128  two full tables and no partial one: the table fetched turns out not to be needed
  26000x300x66   a second table of 8 rows (nj < DB: the min(lane, nj - 1) clamp), nearly every stop in table 0: the
                 next block's first table is almost always the one to fetch
The conditions on the twin's output below keep a grid from passing without meeting these cases."""
import numpy as np
import pytest

import level_cut_twin
import test_level_cutoff as tc
from stochastic_inventory_amd.states import OptDirection

GRIDS = [
    dict(id="D200", S=26000, A=300, D=200, h=0.2, tables=3, boundary=False),
    dict(id="D130", S=26000, A=300, D=130, h=0.2, tables=2, boundary=True),
    dict(id="D128", S=26000, A=300, D=128, h=0.05, tables=2, boundary=True),
    dict(id="D66", S=26000, A=300, D=66, h=0.2, tables=2, boundary=False),
]
_BY_ID = {c["id"]: c for c in GRIDS}
_CACHE = {}


def _workload(c, direction=OptDirection.MIN):
    return tc._grid(c["S"], c["A"], c["D"], T=2, direction=direction, lo=-300, K=500.0, v=1.0, h=c["h"], pi=10.0)


def _level_plan(sia, w, monkeypatch):
    for k in tc._SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDPGPU_WIN_LEVEL", "1")
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        return eng.plan(1)


def _reference(sia, oracle, monkeypatch, c):
    """(workload, the oracle's tables, the twin) of a grid, computed once per session and not changed afterwards."""
    if c["id"] not in _CACHE:
        w = _workload(c)
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
        t = level_cut_twin.twin_solve(w, _level_plan(sia, w, monkeypatch), V)
        _CACHE[c["id"]] = (w, list(zip(V, pol)), t)
    return _CACHE[c["id"]]


def _check_twin_conditions(c, t):
    """What the grid has to show before a count on it means anything (conditions, not measurements)."""
    assert t.band == 32 and t.blocks_per_task == 4
    tables = sorted({step // 64 for p in t.periods for step in p.stop_hist})
    assert len(tables) >= c["tables"], f"{c['id']}: stops in tables {tables}"
    for period, p in enumerate(t.periods, start=1):
        assert p.rearmed_tasks >= 1 and p.never_stopped_tasks >= 1 and p.always_stopped_tasks >= 1, f"{c['id']}: period {period}"
    if c["boundary"]:
        assert any(step % 64 == 0 for p in t.periods for step in p.stop_hist), f"{c['id']}: no stop on a table boundary"
    assert t.run < t.planned


@pytest.mark.gpu
@pytest.mark.parametrize("c", GRIDS, ids=lambda c: c["id"])
def test_prefetch_changes_no_table_and_no_step(sia, oracle, monkeypatch, c):
    """Cut-off on, off, the state-major kernel, the oracle: one set of bits; the steps run are the twin's.  The solve reads
    V_2 from its key row (KEYED_IN: period 2 is still pending when period 1 starts); period 1 run again by hand after the
    tables were read out reads the final fp64 row (the other instantiation): the same tables and the same counters."""
    w, ref, t = _reference(sia, oracle, monkeypatch, c)
    _check_twin_conditions(c, t)
    on, planned, run = tc._solve(sia, w, monkeypatch, 1, None)
    off, planned_off, run_off = tc._solve(sia, w, monkeypatch, 1, 0)
    state, planned_sm, run_sm = tc._solve(sia, w, monkeypatch, 0, None)
    print(f"{w.name}: steps planned {planned}, run {run} ({run / planned:.4f}); the twin: {t.run}")
    tc._same(on, ref, f"{w.name}: cut-off on != oracle")
    tc._same(off, ref, f"{w.name}: cut-off off != oracle")
    tc._same(state, ref, f"{w.name}: window_f1_kernel != oracle")
    assert planned == planned_off == run_off == t.planned and planned_sm == 0 and run_sm == 0
    assert run == t.run, f"{w.name}: the device ran {run} steps, the twin {t.run}"
    for cutoff in (None, 0):
        for k in tc._SWITCHES:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("SDPGPU_WIN_LEVEL", "1")
        if cutoff is not None:
            monkeypatch.setenv("SDPGPU_F1_CUTOFF", str(cutoff))
        with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
            eng.solve(sync=True)
            first = [(eng.values(p), eng.policy(p)) for p in (1, 2)]  # (reading a table resolves what is pending)
            st = eng.stats()
            counters = (int(st.f1_level_steps_planned), int(st.f1_level_steps_run))
            eng.run_period(1)
            eng.synchronize()
            again = [(eng.values(p), eng.policy(p)) for p in (1, 2)]
            st = eng.stats()
            tc._same(first, ref, f"{w.name}: solve, cut-off {cutoff}")
            tc._same(again, ref, f"{w.name}: period 1 from the final row, cut-off {cutoff}")
            assert (int(st.f1_level_steps_planned), int(st.f1_level_steps_run)) == counters
            assert counters == (t.planned, t.run if cutoff is None else t.planned)


@pytest.mark.gpu
def test_prefetch_captured_sweep(sia, oracle, monkeypatch):
    """SDPGPU_GRAPH=1 on the 130-demand grid: eager, captured, replayed -- the oracle's tables and the twin's steps each time."""
    c = _BY_ID["D130"]
    w, ref, t = _reference(sia, oracle, monkeypatch, c)
    for k in tc._SWITCHES + ("SDPGPU_GRAPH",):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDPGPU_WIN_LEVEL", "1")
    monkeypatch.setenv("SDPGPU_GRAPH", "1")
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        for call, replays in ((1, 0), (2, 1), (3, 2)):
            eng.solve(sync=True)
            assert eng.stats().graph_replays == replays, f"call {call}"
            tc._same([(eng.values(p), eng.policy(p)) for p in (1, 2)], ref, f"{w.name}: call {call}")
            st = eng.stats()
            assert (int(st.f1_level_steps_planned), int(st.f1_level_steps_run)) == (t.planned, t.run), f"call {call}"


@pytest.mark.gpu
def test_prefetch_with_values_in_caller_memory(sia, oracle, monkeypatch):
    """sdpgpu_attach_values on the 200-demand grid: the gate is off below period T, so period 1 runs the instantiation
    without the cut-off (every table of a block is the one fetched) from a key row; period T still cuts."""
    import torch
    c = _BY_ID["D200"]
    w, ref, t = _reference(sia, oracle, monkeypatch, c)
    for k in tc._SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDPGPU_WIN_LEVEL", "1")
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        buf = torch.zeros(eng.values_bytes() // 8, dtype=torch.float64, device="cuda")
        eng.attach_values(buf.data_ptr(), buf.numel() * 8)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.solve(sync=True)
        tc._same([(eng.values(p), eng.policy(p)) for p in (1, 2)], ref, f"{w.name}: values in caller memory")
        st = eng.stats()
        assert int(st.f1_level_steps_planned) == t.planned
        assert int(st.f1_level_steps_run) == t.periods[0].planned + t.periods[1].run


@pytest.mark.gpu
def test_prefetch_max_direction_gate_off(sia, oracle, monkeypatch):
    """MAX on the 130-demand grid: the host keeps the cut-off off, every block walks its three tables, each of them fetched
    (and the first table of every later block): the level kernel, the state-major kernel and the oracle agree bit for bit."""
    w = _workload(_BY_ID["D130"], direction=OptDirection.MAX)
    V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
    ref = list(zip(V, pol))
    level, planned, run = tc._solve(sia, w, monkeypatch, 1, None)
    state, planned_sm, run_sm = tc._solve(sia, w, monkeypatch, 0, None)
    assert planned > 0 and run == planned and planned_sm == 0 and run_sm == 0
    tc._same(level, ref, f"{w.name}: level kernel != oracle")
    tc._same(state, ref, f"{w.name}: window_f1_kernel != oracle")
