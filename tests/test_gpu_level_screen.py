"""The screen of the F1 level kernel on the device (window_f1_level_kernel<..., CUT>, csrc/sdp_window.hpp "THE SCREEN"): a
level block whose predecessor stopped is first walked from step screen_start with its sums started at +0.0, and again from
step 0 when that does not prove it beaten.  No table may depend on it: screen on, screen off, the state-major kernel and the
oracle are the same bits where screens succeed, where they fail, where nothing ever stops, where screen_start is 0 and where
the cut-off's gate is closed; sdpgpu_f1_screen_get says which of these happened.  Unless said otherwise the plans are forced
with SDPGPU_WIN_LEVEL=1 and the screen asked for with SDPGPU_F1_SCREEN=1 (a forced plan alone keeps the pure cut-off schedule
that tests/test_level_cutoff.py and its neighbours count step by step).  The lemma and the rule for screen_start are checked
without a GPU in tests/test_level_screen.py."""
import collections

import numpy as np
import pytest

import level_cut_twin
import test_gpu_level_prefetch as tp
import test_level_cutoff as tc
from stochastic_inventory_amd import workloads
from stochastic_inventory_amd.functors import BackorderFunctor
from stochastic_inventory_amd.states import OptDirection

_ENV = tc._SWITCHES + ("SDPGPU_F1_SCREEN", "SDPGPU_F1_SCREEN_LOG2", "SDPGPU_GRAPH")
Run = collections.namedtuple("Run", "tabs planned run screen")  # screen: per period (start, stopped, failed, exact, steps run, steps planned)
_ORACLE = {}


def _env(monkeypatch, level, screen, cutoff=None, graph=None):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (("SDPGPU_WIN_LEVEL", level), ("SDPGPU_F1_SCREEN", screen), ("SDPGPU_F1_CUTOFF", cutoff), ("SDPGPU_GRAPH", graph)):
        if v is not None:
            monkeypatch.setenv(k, str(v))


def _read(eng, w):
    tabs = [(eng.values(t), eng.policy(t)) for t in range(1, w.T + 1)]
    st = eng.stats()
    return Run(tabs, int(st.f1_level_steps_planned), int(st.f1_level_steps_run), [eng.f1_screen(t) for t in range(1, w.T + 1)])


def _run(sia, w, monkeypatch, level=1, screen=1, cutoff=None):
    _env(monkeypatch, level, screen, cutoff)
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        if level is not None:
            assert (eng.plan(1).chunk_blocks == 0) == (level == 1)
        eng.solve(sync=True)
        return _read(eng, w)


def _oracle_tables(sia, oracle, monkeypatch, key):
    """The oracle's tables of the grids of item 2, computed once per session (the 26000-state one is the reference that
    tests/test_gpu_level_prefetch.py keeps) and not changed afterwards."""
    if key == "D200":
        w, ref, _ = tp._reference(sia, oracle, monkeypatch, tp._BY_ID["D200"])
        return w, ref
    if key not in _ORACLE:
        w = tc._grid(1601, 500, 200, T=3) if key == "A500" else tc._grid(20000, 300, 200, T=3, lo=-300, h=0.2)
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
        _ORACLE[key] = (w, list(zip(V, pol)))
    return _ORACLE[key]


def _no_screen(run):
    return all(s[:3] == (0, 0, 0) for s in run.screen)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["A500", "D200", "T3"])
def test_screen_both_paths_and_nothing_changes(sia, oracle, monkeypatch, key):
    """1601x500x200x3, 26000x300x200x2 and 20000x300x200x3 (the last two: lo = -300, h = 0.2): screen on, screen off, the
    state-major kernel and the oracle give the same bits in every table.  Conditions (not measurements) that keep a grid from
    passing without meeting both paths: some period has screen_start >= 56 (a screened block's tables are tagged
    screen_start + n DB, here with starts that are and are not multiples of DB = 64), blocks were screened and stopped, at
    least one screen failed (the ordering region near level 0), fewer steps ran than with the screen off, and every block
    ended either screened and stopped or walked exactly.
      The first grid cannot meet the last three, for a reason that is the planner's and not the kernel's: the plan of
    1601x500x200 has band = S, ONE level block per task, and a task's first block is exact -- so nothing is screened there
    (asserted: the counters and steps of a run without the screen, although screen_start is 72).  The third grid has the same
    three-period tiles on bands of three level blocks and, like the second, must meet every condition."""
    w, ref = _oracle_tables(sia, oracle, monkeypatch, key)
    on = _run(sia, w, monkeypatch, 1, 1)
    off = _run(sia, w, monkeypatch, 1, 0)
    state = _run(sia, w, monkeypatch, 0, None)
    print(f"{w.name}: steps planned {on.planned}, run {on.run} with the screen, {off.run} without; per period "
          f"(start, stopped, failed, exact): {on.screen}; without: {off.screen}")
    tc._same(on.tabs, ref, f"{w.name}: screen on != oracle")
    tc._same(off.tabs, ref, f"{w.name}: screen off != oracle")
    tc._same(state.tabs, ref, f"{w.name}: window_f1_kernel != oracle")
    assert on.planned == off.planned > 0 and state.planned == 0
    assert _no_screen(off) and _no_screen(state)
    starts = [s[0] for s in on.screen]
    assert starts == {"A500": [72, 40, 56], "D200": [56, 56], "T3": [72, 40, 56]}[key] and max(starts) >= 56
    for a, b in zip(on.screen, off.screen):
        assert a[1] + a[3] == b[3] and a[2] <= a[3]  # a failed screen is walked exactly afterwards
        assert a[4] <= b[4] < b[5] == a[5]
    assert sum(s[4] for s in on.screen) == on.run and sum(s[5] for s in on.screen) == on.planned
    if key == "A500":
        _env(monkeypatch, 1, 1)
        with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
            band, _, _ = level_cut_twin.plan_geometry(eng.plan(1), 1601, 500, 200)
        assert band == 8  # one level block per task: every block is a task's first
        assert [s[1:] for s in on.screen] == [s[1:] for s in off.screen] and on.run == off.run < on.planned
        return
    assert sum(s[1] for s in on.screen) > 0, "no block was screened and stopped"
    assert sum(s[2] for s in on.screen) >= 1, "no screen failed"
    assert on.run < off.run < on.planned


@pytest.mark.gpu
def test_screen_where_nothing_ever_stops(sia, oracle, monkeypatch):
    """The flat-cost grid (every sum +0.0, nothing strictly beaten) and the grid lying below zero (the highest action wins):
    the oracle's tables; on the flat grid every planned step ran and no block was screened, as without the screen."""
    for w, flat in ((tc._grid(900, 130, 16, K=0.0, v=0.0, h=0.0, pi=0.0), True), (tc._grid(900, 300, 40, lo=-1600), False)):
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
        on = _run(sia, w, monkeypatch, 1, 1)
        off = _run(sia, w, monkeypatch, 1, 0)
        print(f"{w.name}: planned {on.planned}, run {on.run} / {off.run}; {on.screen}")
        tc._same(on.tabs, list(zip(V, pol)), f"{w.name}: screen on != oracle")
        tc._same(off.tabs, list(zip(V, pol)), f"{w.name}: screen off != oracle")
        if flat:
            assert on.run == on.planned == off.run
            assert all(s[1] == 0 and s[2] == 0 for s in on.screen)
            assert [s[3] for s in on.screen] == [s[3] for s in off.screen]


@pytest.mark.gpu
def test_screen_start_zero_is_the_pure_cutoff(sia, oracle, monkeypatch):
    """The dyadic uniform pmf of test_cutoff_ties_where_blocks_stop: its first step carries 1/16 of the mass, so screen_start
    is 0 and the kernel walks what SDPGPU_F1_SCREEN=0 walks -- the same counters -- and the policy keeps the lowest tied
    action (the oracle's)."""
    f = BackorderFunctor(fixedOrderingCost=0, variOrderingCost=0, holdingCost=1, penaltyCost=1, minInventory=0,
                         maxInventory=1199, maxOrderQuantity=399, iniInventory=0)
    pmf = [np.column_stack([np.arange(24.0), np.full(24, 1.0 / 32)]) for _ in range(3)]
    for t in pmf:
        t[:8, 1] = 2.0 / 32
    w = workloads.Workload("screen_ties_1200x400x24x3", f, OptDirection.MIN, pmf, "ties, blocks stop")
    V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
    on = _run(sia, w, monkeypatch, 1, 1)
    off = _run(sia, w, monkeypatch, 1, 0)
    assert (on.planned, on.run, on.screen) == (off.planned, off.run, off.screen)
    assert _no_screen(on) and on.run < on.planned
    tc._same(on.tabs, list(zip(V, pol)), f"{w.name}: screen on != oracle")
    tc._same(off.tabs, list(zip(V, pol)), f"{w.name}: screen off != oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["max", "negative-cost", "negative-weight", "caller-memory"])
def test_screen_gate(sia, monkeypatch, case):
    """Where the cut-off's gate is closed -- MAX, a negative cost parameter, one negative pmf weight, V_{t+1} in caller memory
    -- no block is screened, whatever SDPGPU_F1_SCREEN says, and the tables are the state-major kernel's.  With the values in
    caller memory the gate is closed below period T only: period T may screen, the periods below walk every step."""
    w = tc._grid(2000, 300, 128, direction=OptDirection.MAX if case == "max" else OptDirection.MIN,
                 v=-1.0 if case == "negative-cost" else 1.0)
    if case == "negative-weight":
        w.pmf[w.T - 1][0, 1] = -w.pmf[w.T - 1][0, 1]  # (about -1e-14: every period above loses V >= 0 with it)

    def solve(level, screen):
        _env(monkeypatch, level, screen)
        with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
            if case == "caller-memory":
                import torch
                buf = torch.zeros(eng.values_bytes() // 8, dtype=torch.float64, device="cuda")
                eng.attach_values(buf.data_ptr(), buf.numel() * 8)
                eng.set_stream(torch.cuda.current_stream().cuda_stream)
            assert all(eng.f1_screen_start(t) >= 8 for t in range(1, w.T + 1))  # a screen the gate has to refuse
            eng.solve(sync=True)
            return _read(eng, w)

    on, state = solve(1, 1), solve(0, None)
    print(f"{case}: planned {on.planned}, run {on.run}, {on.screen}")
    tc._same(on.tabs, state.tabs, f"{w.name} ({case}): level kernel != window_f1_kernel")
    assert on.planned > 0 and state.planned == 0
    closed = range(w.T - 1) if case == "caller-memory" else range(w.T)
    for t in closed:
        assert on.screen[t] == (0,) * 6, f"period {t + 1}"
    if case != "caller-memory":
        assert on.run == on.planned


@pytest.mark.gpu
def test_forced_plan_without_the_switch_keeps_the_cutoff_schedule(sia, oracle, monkeypatch):
    """SDPGPU_WIN_LEVEL=1 and SDPGPU_F1_SCREEN unset on the 26000-state grid (where the switch screens three blocks of four):
    the steps of a SDPGPU_F1_SCREEN=0 run, and no block screened."""
    w, ref = _oracle_tables(sia, oracle, monkeypatch, "D200")
    unset = _run(sia, w, monkeypatch, 1, None)
    off = _run(sia, w, monkeypatch, 1, 0)
    assert (unset.planned, unset.run, unset.screen) == (off.planned, off.run, off.screen)
    assert _no_screen(unset) and unset.run < unset.planned
    tc._same(unset.tabs, ref, f"{w.name}: forced plan != oracle")


@pytest.mark.gpu
def test_automatic_plan_screens(sia, oracle, monkeypatch):
    """262144x250x128x2 with no switch set: the planner takes the level kernel by itself and the screen is on with it
    (screen_start >= 8 in some period; asserted).  Tables bit for bit those of a SDPGPU_F1_SCREEN=0 run, and about 2000
    sampled states per period equal the oracle's eval_states fed the GPU's own V_{t+1}, as bench.py's gate does (a full
    oracle solve of this grid would take too long here)."""
    w = tc._grid(262144, 250, 128, T=2)
    auto = _run(sia, w, monkeypatch, None, None)
    _env(monkeypatch, None, None)
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        assert all(eng.plan(t).chunk_blocks == 0 for t in (1, 2)), "the planner did not take the level kernel"
    off = _run(sia, w, monkeypatch, None, 0)
    print(f"{w.name}: planned {auto.planned}, run {auto.run} with the screen, {off.run} without; {auto.screen}")
    assert auto.planned == off.planned > 0
    assert max(s[0] for s in auto.screen) >= 8 and sum(s[1] for s in auto.screen) > 0
    assert _no_screen(off) and auto.run < off.run
    tc._same(auto.tabs, off.tabs, f"{w.name}: screen on != off")
    P = oracle.Problem(w.desc(), w.pmf, w.overhead())
    rng = np.random.default_rng(7)
    n = 262144
    for period in (2, 1):
        pick = np.unique(np.concatenate([rng.integers(0, n, size=2000), np.arange(0, 160), [n - 2, n - 1, 255, 256, 511, 512]]))
        v_next = auto.tabs[period][0] if period < w.T else None
        ov, oa = P.eval_states(period, v_next, pick.astype(np.float64), nthreads=8)
        assert np.array_equal(auto.tabs[period - 1][0][pick], ov), f"values of period {period}"
        assert np.array_equal(auto.tabs[period - 1][1][pick], oa), f"policy of period {period}"


@pytest.mark.gpu
def test_screen_captured_sweep(sia, oracle, monkeypatch):
    """SDPGPU_GRAPH=1 on the 26000-state grid: eager, captured, replayed -- the oracle's tables, the same step counters and
    the same screen counters each time (the captured sweep resets and carries them with the cut-off's)."""
    w, ref = _oracle_tables(sia, oracle, monkeypatch, "D200")
    _env(monkeypatch, 1, 1, graph=1)
    seen = []
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        for call, replays in ((1, 0), (2, 1), (3, 2)):
            eng.solve(sync=True)
            assert eng.stats().graph_replays == replays, f"call {call}"
            r = _read(eng, w)
            tc._same(r.tabs, ref, f"{w.name}: call {call}")
            seen.append((r.planned, r.run, r.screen))
    assert seen[0] == seen[1] == seen[2]
    assert sum(s[1] for s in seen[0][2]) > 0 and sum(s[2] for s in seen[0][2]) >= 1 and seen[0][1] < seen[0][0]
