"""The step groups of the F1 level kernel on the device (window_f1_level_kernel<..., RS, SG>, csrc/sdp_window.hpp "THE STEP
GROUPS"): a step takes its cells SG at a time -- the group's products, then its sums, then its future terms
(SDPGPU_F1_STEP_GROUP = 1, 2 or 4 at create time).  Per cell the operations, operands and order are those of SG = 1, so no
table and no counter may depend on SG, under any screen rows RS.  The plans are forced with SDPGPU_WIN_LEVEL=1 and the screen
asked for with SDPGPU_F1_SCREEN=1, as in tests/test_gpu_level_screen_rows.py.

The grids are the smallest that reach every edge of a pass: 20000 states x 300 actions give bands of three level blocks (the
last band ragged) and two action blocks, the second with 44 real lanes in its first row and three whole padded rows; D = 70
pads to 72 steps, so a second product table runs with nj = 8 < DB and the padded step's row is read; D = 37 is a single short
table; the inventory starts at -300, the ordering region, where screens fail and blocks are walked again exactly; T = 3 runs
period T (no future term) and the keyed future form.  At these short pmfs the default screen mass (2^-16) would skip no step:
SDPGPU_F1_SCREEN_LOG2=4 (any mass is exact) lets the screen start at step 8 or later in every period."""
import collections

import pytest

import level_cut_twin
import test_gpu_level_screen as tg
import test_level_cutoff as tc

_ENV = tg._ENV + ("SDPGPU_F1_SCREEN_ROWS", "SDPGPU_F1_STEP_GROUP")
# screen / rows: per period (start, stopped, failed, exact, steps run, steps planned) and (screened steps, RS); ops prices the
# steps, the screened steps and the tests (sdpgpu_stats): together all six device counters of a period
Run = collections.namedtuple("Run", "tabs planned run ops screen rows")
_GRIDS = {"D70": (20000, 300, 70), "D37": (20000, 300, 37)}
_ORACLE = {}


def _oracle_tables(oracle, key):
    """Computed once per session and not changed afterwards."""
    if key not in _ORACLE:
        S, A, D = _GRIDS[key]
        w = tc._grid(S, A, D, T=3, lo=-300, h=0.2)
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
        _ORACLE[key] = (w, list(zip(V, pol)))
    return _ORACLE[key]


def _run(sia, key, w, monkeypatch, group=None, rows=None, graph=None, calls=1):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (("SDPGPU_WIN_LEVEL", 1), ("SDPGPU_F1_SCREEN", 1), ("SDPGPU_F1_SCREEN_LOG2", 4), ("SDPGPU_GRAPH", graph),
                 ("SDPGPU_F1_SCREEN_ROWS", rows), ("SDPGPU_F1_STEP_GROUP", group)):
        if v is not None:
            monkeypatch.setenv(k, str(v))
    out = []
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        S, A, D = _GRIDS[key]
        # a level plan: bands of three level blocks, two action blocks, the steps padded to a multiple of 8
        assert level_cut_twin.plan_geometry(eng.plan(1), S, A, D) == (24, 2, -(-D // 8) * 8)
        for _ in range(calls):
            eng.solve(sync=True)
            tabs = [(eng.values(t), eng.policy(t)) for t in range(1, w.T + 1)]
            st = eng.stats()
            out.append(Run(tabs, int(st.f1_level_steps_planned), int(st.f1_level_steps_run), float(st.fp64_ops_executed),
                           [eng.f1_screen(t) for t in range(1, w.T + 1)], [eng.f1_screen_rows(t) for t in range(1, w.T + 1)]))
    return out[0] if calls == 1 else out


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(_GRIDS))
def test_step_groups_parity_and_counters(sia, oracle, monkeypatch, key):
    """SG in {1, 2, 4} x RS in {1, 2, 4}: every table is the oracle's, bit for bit, and for each RS the counters of every period
    -- steps run, tests (through the priced operations), blocks screened and stopped, screens failed, exact walks, screened
    steps -- are the same under every SG.  Both outcomes of a screen were met in every run."""
    w, ref = _oracle_tables(oracle, key)
    for rs in (4, 2, 1):
        runs = {}
        for sg in (1, 2, 4):
            r = runs[sg] = _run(sia, key, w, monkeypatch, group=sg, rows=rs)
            print(f"{w.name} RS={rs} SG={sg}: steps planned {r.planned}, run {r.run}, fp64 ops {r.ops:.9g}; per period "
                  f"(start, stopped, failed, exact, run, planned) {r.screen}; (screened steps, RS) {r.rows}")
            tc._same(r.tabs, ref, f"{w.name}: RS = {rs}, SG = {sg} != oracle")
            assert [x[1] for x in r.rows] == [rs] * w.T
            assert all(s[0] >= 8 for s in r.screen), "a period was not screened"
            assert sum(s[1] for s in r.screen) > 0, "no block was screened and stopped"
            assert sum(s[2] for s in r.screen) >= 1, "no screen failed"
            assert all(0 < screened <= s[4] for s, (screened, _) in zip(r.screen, r.rows))
            assert 0 < r.run < r.planned
        for sg in (2, 4):
            assert runs[sg][1:] == runs[1][1:], f"{w.name}: RS = {rs}: the counters of SG = {sg} are not those of SG = 1"


@pytest.mark.gpu
@pytest.mark.parametrize("group", [None, 1, 2, 4])
def test_step_groups_captured_sweep(sia, oracle, monkeypatch, group):
    """SDPGPU_GRAPH=1, the default SG and each value: eager, captured, replayed -- the oracle's tables and the eager sweep's
    counters each time."""
    w, ref = _oracle_tables(oracle, "D70")
    eager = _run(sia, "D70", w, monkeypatch, group=group)
    seen = _run(sia, "D70", w, monkeypatch, group=group, graph=1, calls=3)
    for call, r in enumerate(seen, start=1):
        tc._same(r.tabs, ref, f"{w.name}: SG = {group}, call {call}")
        assert r[1:] == eager[1:], f"{w.name}: SG = {group}, call {call}: counters differ from the eager sweep's"


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["3", "0", "8", "2x", ""])
def test_bad_step_group_is_refused_at_create_time(sia, monkeypatch, bad):
    w = tc._grid(2000, 300, 37)
    monkeypatch.setenv("SDPGPU_F1_STEP_GROUP", bad)
    with pytest.raises(sia._abi.SdpgpuError, match="SDPGPU_F1_STEP_GROUP=" + bad):
        sia.SdpEngine(w.desc(), w.pmf, w.overhead())
