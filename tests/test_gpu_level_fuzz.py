"""Randomised parity of the F1 level kernel (window_f1_level_kernel, SDPGPU_WIN_LEVEL=1) and its cut-off: the seeded random,
coarser-grid and degenerate family-1 instances of test_gpu_fuzz.py and a generator of this file's own -- action counts around
the 64-lane and 256-action blocks, pmf widths around the 8-step rotation and the 64-step product table, supports that start
above zero, have gaps and zero weights, K = 0, decimal costs, MIN and MAX -- each solved with the cut-off on, with it off and
by the state-major kernel, every period against the CPU oracle bit for bit.  The step counters say whether the level kernel
ran and whether it skipped anything.  Then one handle through many sweeps (eager again, stepped by hand, captured and
replayed, values in caller memory) and a horizon inside which the host's gate switches off.  Sizes are small: seconds."""
import numpy as np
import pytest

import level_cut_twin
import test_gpu_fuzz as tf
from stochastic_inventory_amd import workloads
from stochastic_inventory_amd.functors import BackorderFunctor
from stochastic_inventory_amd.states import OptDirection

_SWITCHES = ("SDPGPU_WIN_R", "SDPGPU_WIN_S", "SDPGPU_WIN_NCH", "SDPGPU_WIN_LEVEL", "SDPGPU_F1_CUTOFF", "SDPGPU_GRAPH")
ACTION_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 300)
PMF_WIDTHS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129)


def make_level_instance(seed):
    """Family 1 at the sizes where the level kernel's lane masks and tables change shape: A - 1 orders with A from
    ACTION_COUNTS (no order at all, one, a wave of lanes give or take one, an action block give or take one, a second block),
    pmf tiles of PMF_WIDTHS points whose support starts at 0 .. 3, is unit-stride or has gaps (laid out with zero padding by the
    library) and carries zero weights at its ends and inside; K = 0 once in four with v > 0; integer, dyadic or decimal costs;
    clamped or not; MIN three times in four."""
    rng = np.random.default_rng(88000 + seed)
    T = int(rng.integers(1, 4))
    kind = ["int", "dyadic", "decimal"][int(rng.integers(0, 3))]
    A = int(ACTION_COUNTS[seed % len(ACTION_COUNTS)])
    K = 0.0 if rng.integers(0, 4) == 0 else tf._money(rng, 1, 60, kind)
    f = BackorderFunctor(fixedOrderingCost=K, variOrderingCost=max(0.25, tf._money(rng, 0, 3, kind)),
                         holdingCost=tf._money(rng, 0, 3, kind), penaltyCost=tf._money(rng, 0, 12, kind),
                         minInventory=-float(rng.integers(0, 120)), maxInventory=float(rng.integers(40, 500)),
                         maxOrderQuantity=float(A - 1), iniInventory=float(rng.integers(-3, 4)),
                         clampInventory=bool(rng.integers(0, 4)))
    direction = OptDirection.MIN if rng.integers(0, 4) else OptDirection.MAX
    tiles = []
    for t in range(T):
        n = int(PMF_WIDTHS[(seed // 2 + 3 * t) % len(PMF_WIDTHS)])
        d0 = float(rng.integers(0, 4))
        if n > 1 and rng.integers(0, 3) == 0:
            d = d0 + np.sort(rng.choice(np.arange(0, 2 * n), size=n, replace=False)).astype(np.float64)
        else:
            d = d0 + np.arange(n, dtype=np.float64)
        p = rng.random(n) + 0.05
        zeros = int(rng.integers(0, 3))
        if zeros and n >= 3:
            p[0] = p[-1] = 0.0
            if zeros == 2:
                inside = rng.random(n) < 0.3
                inside[n // 2] = False
                p[inside] = 0.0
        p /= p.sum()
        tiles.append(np.stack([d, p], axis=1))
    return workloads.Workload(f"fuzz_level_{seed}_A{A}", f, direction, tiles)


def _groups():
    return {
        "random": [tf.make_instance(1, seed) for seed in range(40)],
        "step2": [tf.make_stepped_instance(1, 300 + seed, 2) for seed in range(12)],
        "step4": [tf.make_stepped_instance(1, 300 + seed, 4) for seed in range(12)],
        "shapes": [tf.make_shaped_instance(1, 40 + seed, shape) for shape in tf.SHAPES for seed in range(2)],
        "level": [make_level_instance(seed) for seed in range(36)],
    }


def _engine(sia, w, monkeypatch, level, cutoff=None, graph=False):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDPGPU_WIN_LEVEL", str(level))
    if cutoff is not None:
        monkeypatch.setenv("SDPGPU_F1_CUTOFF", str(cutoff))
    if graph:
        monkeypatch.setenv("SDPGPU_GRAPH", "1")
    return sia.SdpEngine(w.desc(), w.pmf, w.overhead())


def _level_periods(eng, T):
    """How many periods of the handle plan the level kernel (a period whose support is too sparse for a window, or for which the
    planner finds no window plan, runs elsewhere: the level kernel is then not reached, whatever the switch says)."""
    n = 0
    for t in range(1, T + 1):
        pl = eng.plan(t)
        n += pl.kernel == 2 and pl.chunk_blocks == 0 and (pl.r, pl.s) == (4, 8)
    return n


def _tables(eng, T):
    return [(eng.values(t), eng.policy(t)) for t in range(1, T + 1)]


def _counters(eng):
    st = eng.stats()
    return int(st.f1_level_steps_planned), int(st.f1_level_steps_run)


def _assert_tables(got, V, pol, what):
    for t, (v, p) in enumerate(got, start=1):
        assert np.array_equal(p, pol[t - 1]), f"{what}: policy of period {t}"
        assert np.array_equal(v, V[t - 1]), f"{what}: values of period {t}"


def test_level_switch_reaches_the_level_kernel_on_most_instances(sia, monkeypatch):
    """Host arithmetic only (sdpgpu_plan_period): under SDPGPU_WIN_LEVEL=1 at most one instance in five of every group has no
    period on the level kernel, and the new generator's instances cover every action count and pmf width asked for."""
    for name, ws in _groups().items():
        missed = []
        for w in ws:
            with _engine(sia, w, monkeypatch, 1) as eng:
                if _level_periods(eng, w.T) == 0:
                    missed.append(w.name)
        print(f"{name}: {len(missed)} of {len(ws)} instances without a level period: {missed}")
        assert 5 * len(missed) <= len(ws), name
    ws = _groups()["level"]
    assert {int(w.functor.maxOrderQuantity) + 1 for w in ws} == set(ACTION_COUNTS)
    assert {len(t) for w in ws for t in w.pmf} == set(PMF_WIDTHS)
    assert any(w.functor.fixedOrderingCost == 0 and w.functor.variOrderingCost > 0 for w in ws)
    assert any(t[0, 0] > 0 for w in ws for t in w.pmf) and any(np.any(np.diff(t[:, 0]) > 1) for w in ws for t in w.pmf)
    assert any(np.any(t[1:-1, 1] == 0) for w in ws for t in w.pmf)
    assert {w.direction for w in ws} == {OptDirection.MIN, OptDirection.MAX}
    assert {bool(w.functor.clampInventory) for w in ws} == {True, False}


_SEEN = {}  # group -> [(name, direction, level periods, planned, run with the cut-off on)]


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["random", "step2", "step4", "shapes", "level"])
def test_level_kernel_random_instances_bit_exact(sia, oracle, monkeypatch, group):
    seen = _SEEN.setdefault(group, [])
    del seen[:]
    for w in _groups()[group]:
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=4)
        for what, level, cutoff in (("cut-off on", 1, None), ("cut-off off", 1, 0), ("state-major", 0, None)):
            with _engine(sia, w, monkeypatch, level, cutoff) as eng:
                n_level = _level_periods(eng, w.T)
                eng.solve(sync=True)
                _assert_tables(_tables(eng, w.T), V, pol, f"{w.name} {what}")
                planned, run = _counters(eng)
            assert run <= planned, f"{w.name} {what}"
            assert (planned > 0) == (n_level > 0), f"{w.name} {what}"  # the counters say the level kernel ran
            if level == 0:
                assert n_level == 0 and planned == 0
            elif cutoff == 0 or w.direction == OptDirection.MAX:
                assert run == planned, f"{w.name} {what}"                # the gate is off: every step walked
            if level == 1 and cutoff is None:
                seen.append((w.name, w.direction, n_level, planned, run))
    assert 5 * sum(1 for s in seen if s[2] == 0) <= len(seen)


@pytest.mark.gpu
def test_level_fuzz_cutoff_fired_and_stayed_silent(sia):
    """Over the instances of the test above (the whole file has to run): the cut-off skipped steps on some, and on some MIN
    instance that ran the level kernel it skipped none."""
    assert set(_SEEN) == {"random", "step2", "step4", "shapes", "level"}, "run the whole file"
    every = [s for group in _SEEN.values() for s in group]
    fired = [s[0] for s in every if s[4] < s[3]]
    silent = [s[0] for s in every if s[1] == OptDirection.MIN and s[3] > 0 and s[4] == s[3]]
    print(f"cut-off fired on {len(fired)} of {len(every)} instances, silent on {len(silent)} MIN instances")
    assert fired and silent


# ---------------------------------------------------------------------------------------------------------------
# The host's gate inside one horizon
# ---------------------------------------------------------------------------------------------------------------
_HANDLE_CASE = {c["id"]: c for c in level_cut_twin.MULTI_BLOCK_GRIDS}["50000x64x17"]


def _case_workload(c, pmf=None, name=None):
    f = BackorderFunctor(fixedOrderingCost=c["K"], variOrderingCost=c["v"], holdingCost=c["h"], penaltyCost=c["pi"],
                         minInventory=c["lo"], maxInventory=c["lo"] + c["S"] - 1, maxOrderQuantity=c["A"] - 1, iniInventory=c["lo"])
    pmf = workloads.seasonal_pmf(c["T"], c["D"]) if pmf is None else pmf
    return workloads.Workload(name or f"cut_{c['S']}x{c['A']}x{c['D']}x{len(pmf)}", f, OptDirection.MIN, pmf, "level handle test")


_GATE_TAIL_RUN = [96480, 98072]   # the twin's steps run on periods 3 .. 4 of the instance below (checked on the CPU here)


def _gate_instance():
    c = _HANDLE_CASE
    pmf = workloads.seasonal_pmf(4, c["D"])
    pmf[1] = pmf[1].copy()
    pmf[1][3, 1] = -1.0 / 1024
    return _case_workload(c, pmf, "cut_gate_inside"), _case_workload(c, pmf[2:], "cut_gate_inside_tail")


def test_gate_instance_tail_counts_are_the_twins(sia, oracle, monkeypatch):
    """Periods 3 .. 4 of the gate instance as a horizon of their own: the oracle's tables of the long horizon, and the twin's
    count of the steps the cut-off leaves (CPU only)."""
    w, tail = _gate_instance()
    V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
    Vt, polt, _ = oracle.Problem(tail.desc(), tail.pmf, tail.overhead()).solve(nthreads=8)
    assert all(np.array_equal(Vt[t], V[2 + t]) and np.array_equal(polt[t], pol[2 + t]) for t in range(2))
    with _engine(sia, tail, monkeypatch, 1) as eng:
        t = level_cut_twin.twin_solve(tail, eng.plan(1), Vt)
    assert [p.run for p in t.periods] == _GATE_TAIL_RUN and t.run < t.planned


@pytest.mark.gpu
def test_cutoff_gate_switches_off_inside_the_horizon(sia, oracle, monkeypatch):
    """Four periods, one small negative weight in the tile of period 2: a running sum of period 2 is no lower bound, and V_2 need
    not be >= 0 for period 1 -- the gate is on for periods 4 and 3, off for 2 and 1 (v_nonneg is an induction from period T).
    Tables are the oracle's; the steps run are those of periods 3 .. 4 with the cut-off (the same two tiles as a horizon of
    their own) plus the full walk of two periods."""
    w, tail = _gate_instance()
    V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
    with _engine(sia, w, monkeypatch, 1) as eng:
        assert _level_periods(eng, 4) == 4
        eng.solve(sync=True)
        _assert_tables(_tables(eng, 4), V, pol, "gate inside the horizon")
        planned, run = _counters(eng)
    with _engine(sia, w, monkeypatch, 1, 0) as eng:
        eng.solve(sync=True)
        _assert_tables(_tables(eng, 4), V, pol, "gate inside the horizon, cut-off off")
        planned_off, run_off = _counters(eng)
    with _engine(sia, tail, monkeypatch, 1) as eng:
        eng.solve(sync=True)
        _assert_tables(_tables(eng, 2), V[2:], pol[2:], "periods 3 .. 4 alone")
        planned_tail, run_tail = _counters(eng)
    print(f"gate inside: planned {planned}, run {run}; periods 3..4 alone: planned {planned_tail}, run {run_tail}")
    assert planned == planned_off == run_off and planned % 4 == 0 and planned_tail == planned // 2
    assert run_tail == sum(_GATE_TAIL_RUN) < planned_tail   # the cut-off does fire above the negative weight: the twin's count
    assert run == run_tail + 2 * (planned // 4)          # ... and not at all from it down


# ---------------------------------------------------------------------------------------------------------------
# One handle, many sweeps (a multi-block grid of test_level_cutoff.py; the twin's counts: level_cut_twin.MULTI_BLOCK_GRIDS)
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle_case(oracle):
    w = _case_workload(_HANDLE_CASE)
    V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
    return w, V, pol


@pytest.mark.gpu
def test_cutoff_handle_solved_again_and_stepped_by_hand(sia, monkeypatch, handle_case):
    """Three eager solves of one handle (the U row is reused, the device counters are zeroed again per period), then period T by
    hand and a fourth solve: the same tables and the same two counters after every call -- the twin's."""
    w, V, pol = handle_case
    c = _HANDLE_CASE
    with _engine(sia, w, monkeypatch, 1) as eng:
        first = None
        for call in ("solve 1", "solve 2", "solve 3", "run_period(T)", "solve 4"):
            if call.startswith("solve"):
                eng.solve(sync=True)
            else:
                eng.run_period(w.T)
                eng.synchronize()
            _assert_tables(_tables(eng, w.T), V, pol, call)
            first = first or _counters(eng)
            assert _counters(eng) == first, call
        assert first[1] == sum(c["run"]) and first[1] < first[0]


@pytest.mark.gpu
def test_cutoff_handle_captured_sweep(sia, monkeypatch, handle_case):
    """SDPGPU_GRAPH=1, the calls of test_solve_replays_its_sweep_as_one_hip_graph: eager, captured (pre-pass, counter memset
    and CUT kernel inside the capture), replayed twice.  After every call the oracle's tables and the same steps run."""
    w, V, pol = handle_case
    with _engine(sia, w, monkeypatch, 1, graph=True) as eng:
        for call, replays in ((1, 0), (2, 1), (3, 2), (4, 3)):
            eng.solve(sync=True)
            assert eng.stats().graph_replays == replays, f"call {call}"
            _assert_tables(_tables(eng, w.T), V, pol, f"call {call}")
            planned, run = _counters(eng)
            assert run == sum(_HANDLE_CASE["run"]) and run < planned, f"call {call}"


@pytest.mark.gpu
def test_cutoff_gate_with_values_in_caller_memory(sia, monkeypatch, handle_case):
    """sdpgpu_attach_values: the library does not write the value arena alone, so V_{t+1} >= 0 is not trusted -- every period
    below T walks all its steps; period T, which reads no values, still cuts (the twin's count of period T)."""
    import torch
    w, V, pol = handle_case
    c = _HANDLE_CASE
    with _engine(sia, w, monkeypatch, 1) as eng:
        buf = torch.zeros(eng.values_bytes() // 8, dtype=torch.float64, device="cuda")
        eng.attach_values(buf.data_ptr(), buf.numel() * 8)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.solve(sync=True)
        _assert_tables(_tables(eng, w.T), V, pol, "values in caller memory")
        planned, run = _counters(eng)
        assert planned % w.T == 0
        assert run == (w.T - 1) * (planned // w.T) + c["run"][-1] and c["run"][-1] < planned // w.T
