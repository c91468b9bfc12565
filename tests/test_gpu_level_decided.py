"""The decided split of the F1 level kernel on the device (csrc/sdpgpu_window.hip launch_window): where the cut-off
is on and the decided boundary c_t falls inside the slab, the level launch walks the live states [lo, c_t) alone and the states
[c_t, hi) take value Q(i, 0) and action 0 from one one-action launch of window_f1_kernel<1, 8>.  No table may depend on it:
every table here is the oracle's full solve and the table of a SDPGPU_F1_DECIDED=0 run, bit for bit; sdpgpu_f1_decided_get
says where the split ran.  Unless said otherwise the plans are forced with SDPGPU_WIN_LEVEL=1 and the split asked for with
SDPGPU_F1_DECIDED=1.  The claim itself and the host rule are checked without a GPU in tests/test_level_decided.py."""
import collections

import numpy as np
import pytest

import test_gpu_level_screen as ts
import test_level_cutoff as tc
import test_level_decided as td

Run = collections.namedtuple("Run", "tabs planned run decided")  # decided: per period (c_t, live, decided, ran, arena bytes)


def _read(eng, w):
    tabs = [(eng.values(t), eng.policy(t)) for t in range(1, w.T + 1)]
    st = eng.stats()
    return Run(tabs, int(st.f1_level_steps_planned), int(st.f1_level_steps_run), [eng.f1_decided(t) for t in range(1, w.T + 1)])


def _run(sia, w, monkeypatch, decided, level=1):
    td._env(monkeypatch, WIN_LEVEL=level, F1_DECIDED=decided)
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        assert all(eng.plan(t).chunk_blocks == 0 for t in range(1, w.T + 1)), "not the level kernel"
        eng.solve(sync=True)
        return _read(eng, w)


def _both(sia, oracle, monkeypatch, w, want_c, ref=None):
    """Split on and off against the oracle's full solve; returns (on, off).  want_c: the boundaries expected, by period."""
    if ref is None:
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
        ref = list(zip(V, pol))
    on = _run(sia, w, monkeypatch, 1)
    off = _run(sia, w, monkeypatch, 0)
    print(f"{w.name}: decided {on.decided}; steps planned {on.planned} run {on.run}, unsplit {off.planned} / {off.run}")
    tc._same(on.tabs, ref, f"{w.name}: split != oracle")
    tc._same(off.tabs, ref, f"{w.name}: unsplit != oracle")
    n = len(ref[0][0])
    assert [d[0] for d in on.decided] == want_c == [d[0] for d in off.decided]
    assert all(d[1:4] == (n, 0, 0) for d in off.decided)
    for c, d, (v, pol) in zip(want_c, on.decided, ref):
        assert d[1:4] == ((c, n - c, 1) if 0 < c < n else (n, 0, 0))
        assert not pol[c:].any()
    return on, off


@pytest.mark.gpu
def test_split_both_parts(sia, oracle, monkeypatch):
    """1601x500x200x3 from 0: boundaries 597 / 398 / 199, both parts non-empty in every period, far fewer steps planned."""
    w, ref = ts._oracle_tables(sia, oracle, monkeypatch, "A500")
    on, off = _both(sia, oracle, monkeypatch, w, [597, 398, 199], ref)
    assert 0 < on.run <= on.planned < off.planned


@pytest.mark.gpu
def test_split_zero_level_inside_the_slab(sia, oracle, monkeypatch):
    """2000x300x21x3 from -700: level 0 is state 700, boundaries 760 / 740 / 720."""
    _both(sia, oracle, monkeypatch, tc._grid(2000, 300, 21, lo=-700), [760, 740, 720])


@pytest.mark.gpu
def test_no_decided_part_below_zero(sia, oracle, monkeypatch):
    """900x300x40x3 wholly below zero: no decided part, and the steps are the plain run's."""
    on, off = _both(sia, oracle, monkeypatch, tc._grid(900, 300, 40, lo=-1600), [900, 900, 900])
    assert (on.planned, on.run) == (off.planned, off.run)


@pytest.mark.gpu
def test_boundary_leaves_the_slab_in_period_one(sia, oracle, monkeypatch):
    """300x64x128x3 from 0: periods 3 and 2 split at 127 and 254, period 1 has its boundary (381) past the slab: none."""
    _both(sia, oracle, monkeypatch, tc._grid(300, 64, 128), [300, 254, 127])


@pytest.mark.gpu
@pytest.mark.parametrize("lo,c", [(-479, 511), (-480, 512), (-481, 513)])
def test_boundary_at_the_tile_seam(sia, oracle, monkeypatch, lo, c):
    """1200x40x33x1: boundaries 511, 512, 513 -- around the 512-state tile of the one-action kernel."""
    _both(sia, oracle, monkeypatch, tc._grid(1200, 40, 33, T=1, lo=lo), [c])


@pytest.mark.gpu
def test_ragged_top_and_tiny_live_part(sia, oracle, monkeypatch):
    """700x300x21x2 from -450: hi - c_t = 210 and 230 < A; 600x100x45x1 from 40 (level 0 lies 40 steps below the grid): a
    live part of 4 states, less than one level block."""
    _both(sia, oracle, monkeypatch, tc._grid(700, 300, 21, T=2, lo=-450), [490, 470])
    _both(sia, oracle, monkeypatch, tc._grid(600, 100, 45, T=1, lo=40), [4])


@pytest.mark.gpu
def test_one_action(sia, oracle, monkeypatch):
    """A = 1: the live launch has nothing to decide either."""
    _both(sia, oracle, monkeypatch, tc._grid(500, 1, 20, T=2), [38, 19])


@pytest.mark.gpu
def test_ties_everywhere(sia, oracle, monkeypatch):
    """K = 0 and h = 0: above level 0 every action that stays below the clamp ties with action 0 in period T; the policy
    stays 0 above the boundary (asserted for every grid in _both)."""
    _both(sia, oracle, monkeypatch, tc._grid(1000, 100, 30, K=0.0, h=0.0), [87, 58, 29])
    _both(sia, oracle, monkeypatch, tc._grid(1000, 100, 30, K=0.0, h=0.0, v=0.0), [87, 58, 29])


@pytest.mark.gpu
def test_captured_sweep(sia, oracle, monkeypatch):
    """SDPGPU_GRAPH=1 on the first grid: the eager, the capturing and the replayed sweep give the oracle's tables and the same
    getter and step counters."""
    w, ref = ts._oracle_tables(sia, oracle, monkeypatch, "A500")
    td._env(monkeypatch, WIN_LEVEL=1, F1_DECIDED=1, GRAPH=1)
    seen = []
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        for call, replays in ((1, 0), (2, 1), (3, 2)):
            eng.solve(sync=True)
            assert eng.stats().graph_replays == replays, f"call {call}"
            r = _read(eng, w)
            tc._same(r.tabs, ref, f"{w.name}: call {call}")
            seen.append((r.planned, r.run, r.decided))
    assert seen[0] == seen[1] == seen[2]
    assert [d[1:4] for d in seen[0][2]] == [(597, 1004, 1), (398, 1203, 1), (199, 1402, 1)]


@pytest.mark.gpu
def test_reused_handle_and_period_out_of_order(sia, oracle, monkeypatch):
    """One handle solved twice, then period 2 run again on its own (its rows are finalized by a flush of one period): the
    oracle's tables and the same counters each time."""
    w = tc._grid(2000, 300, 21, lo=-700)
    V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
    ref = list(zip(V, pol))
    td._env(monkeypatch, WIN_LEVEL=1, F1_DECIDED=1)
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        eng.solve(sync=True)
        first = _read(eng, w)
        eng.solve(sync=True)
        second = _read(eng, w)
        eng.run_period(2)
        third = _read(eng, w)
    for r in (first, second, third):
        tc._same(r.tabs, ref, f"{w.name}")
        assert r.decided == first.decided and (r.planned, r.run) == (first.planned, first.run)
    assert [d[3] for d in first.decided] == [1, 1, 1]


@pytest.mark.gpu
def test_planner_chosen_level_plan_splits(sia, oracle, monkeypatch):
    """524288x250x32x2 from 0 with no plan forced: the planner takes the level kernel by itself.  With SDPGPU_F1_DECIDED=1 the
    split runs on that plan (the getter); with no switch set it does not (the split is opt-in: the benchmark's contract test
    pins the default headline as a throughput-bound sweep) and the launch is the SDPGPU_F1_DECIDED=0 one.  Tables bit for bit
    those of the unsplit runs; about 2000 sampled states per period and the states around both boundaries equal the oracle's
    eval_states fed the GPU's own V_{t+1} (a full oracle solve would take too long here)."""
    n = 524288
    w = tc._grid(n, 250, 32, T=2)
    auto = _run(sia, w, monkeypatch, 1, level=None)
    off = _run(sia, w, monkeypatch, 0, level=None)
    unset = _run(sia, w, monkeypatch, None, level=None)
    print(f"{w.name}: {auto.decided}; steps planned {auto.planned} run {auto.run}, unsplit {off.planned} / {off.run}")
    assert [d[:4] for d in auto.decided] == [(62, 62, n - 62, 1), (31, 31, n - 31, 1)]
    assert [d[:4] for d in off.decided] == [(62, n, 0, 0), (31, n, 0, 0)]
    assert (unset.planned, unset.run, unset.decided) == (off.planned, off.run, off.decided)
    assert 0 < auto.planned < off.planned
    tc._same(auto.tabs, off.tabs, f"{w.name}: split != unsplit")
    tc._same(unset.tabs, off.tabs, f"{w.name}: no switch != SDPGPU_F1_DECIDED=0")
    P = oracle.Problem(w.desc(), w.pmf, w.overhead())
    rng = np.random.default_rng(11)
    for period in (2, 1):
        pick = np.unique(np.concatenate([rng.integers(0, n, size=2000), np.arange(0, 130), [n - 2, n - 1, 511, 512, 513]]))
        v_next = auto.tabs[period][0] if period < w.T else None
        ov, oa = P.eval_states(period, v_next, pick.astype(np.float64), nthreads=8)
        assert np.array_equal(auto.tabs[period - 1][0][pick], ov), f"values of period {period}"
        assert np.array_equal(auto.tabs[period - 1][1][pick], oa), f"policy of period {period}"
