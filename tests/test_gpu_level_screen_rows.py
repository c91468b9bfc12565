"""The screen rows of the F1 level kernel on the device (window_f1_level_kernel<..., CUT, RS>, csrc/sdp_window.hpp "THE SCREEN
ROWS"): a screened pass walks RS of the block's four action rows (SDPGPU_F1_SCREEN_ROWS = 1, 2 or 4 at create time) and holds
each row's sum against the thresholds of all the rows it stands for.  No table may depend on RS; the counters say what ran.
The plans are forced with SDPGPU_WIN_LEVEL=1 and the screen asked for with SDPGPU_F1_SCREEN=1, as in
tests/test_gpu_level_screen.py.  The lemma, a twin of the collapsed test and a wrong variant that the grids below would catch
(levels below 0: the ordering region, where a higher row's threshold is far above its base row's) are checked without a GPU in
tests/test_level_screen_rows.py."""
import collections

import pytest

import test_gpu_level_screen as tg
import test_level_cutoff as tc
from stochastic_inventory_amd.states import OptDirection

_ENV = tg._ENV + ("SDPGPU_F1_SCREEN_ROWS",)
Run = collections.namedtuple("Run", "tabs planned run ops screen rows")  # rows: per period (screened steps, RS)
_ORACLE = {}

# sdpgpu_f1_screen_get of every period -- (start, stopped, failed, exact, steps run, steps planned) -- as the kernel from
# before the screen rows gives them on these grids (forced plan, SDPGPU_F1_SCREEN=1): RS = 4 is that kernel.
PARENT = {
    "D200": [(56, 4847, 1, 1729, 495344, 1315200), (56, 4861, 1, 1715, 466064, 1315200)],
    "T3": [(72, 3298, 2, 1778, 472288, 1015200), (40, 3308, 2, 1768, 351560, 1015200), (56, 3318, 2, 1758, 378808, 1015200)],
    "A500": [(56, 3329, 2, 1797, 407984, 1025200), (56, 3343, 2, 1783, 384376, 1025200)],
}


def _run(sia, w, monkeypatch, rows=None, screen=1, cutoff=None, graph=None, calls=1):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (("SDPGPU_WIN_LEVEL", 1), ("SDPGPU_F1_SCREEN", screen), ("SDPGPU_F1_CUTOFF", cutoff), ("SDPGPU_GRAPH", graph),
                 ("SDPGPU_F1_SCREEN_ROWS", rows)):
        if v is not None:
            monkeypatch.setenv(k, str(v))
    out = []
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        assert eng.plan(1).chunk_blocks == 0
        for _ in range(calls):
            eng.solve(sync=True)
            tabs = [(eng.values(t), eng.policy(t)) for t in range(1, w.T + 1)]
            st = eng.stats()
            out.append(Run(tabs, int(st.f1_level_steps_planned), int(st.f1_level_steps_run), float(st.fp64_ops_executed),
                           [eng.f1_screen(t) for t in range(1, w.T + 1)], [eng.f1_screen_rows(t) for t in range(1, w.T + 1)]))
    return out[0] if calls == 1 else out


def _grid_and_oracle(sia, oracle, monkeypatch, key):
    """26000x300x200x2 and 20000x300x200x3 (lo = -300, h = 0.2: the references tests/test_gpu_level_screen.py keeps) and
    20000x500x200x2 on the same costs, whose plan has bands of three level blocks and a second action block of 244 real
    actions.  Computed once per session and not changed afterwards."""
    if key != "A500":
        return tg._oracle_tables(sia, oracle, monkeypatch, key)
    if key not in _ORACLE:
        w = tc._grid(20000, 500, 200, T=2, lo=-300, h=0.2)
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
        _ORACLE[key] = (w, list(zip(V, pol)))
    return _ORACLE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["D200", "T3", "A500"])
def test_screen_rows_parity_and_counters(sia, oracle, monkeypatch, key):
    """RS = 1, 2 and 4: every table is the oracle's, bit for bit (so the three agree).  A = 300 leaves the upper rows of the
    second action block padded, and the ordering region near level 0 fails screens: blocks were screened and stopped and at
    least one screen failed for every RS, so both outcomes of the collapsed test were met.  Counters: every block ended
    stopped by a screen or walked exactly; the screened steps are some but not all of the steps run; RS = 4 gives the six
    fields of the kernel before the collapse (constants); from RS = 4 to 2 to 1 the executed operations fall while the steps
    walked move by a few per cent at most (the collapsed test stops where the hardest cell of a row group does: the CPU twin's
    1.5 %, here with the mode rule's extra exact walks on top -- 5 % is the bound)."""
    w, ref = _grid_and_oracle(sia, oracle, monkeypatch, key)
    off = _run(sia, w, monkeypatch, screen=0)
    assert all(r == (0, 2) for r in off.rows)  # no screen: no screened step (and the default RS)
    runs = {}
    for rs in (4, 2, 1):
        r = runs[rs] = _run(sia, w, monkeypatch, rows=rs)
        print(f"{w.name} RS={rs}: steps planned {r.planned}, run {r.run} ({off.run} without the screen), fp64 ops {r.ops:.6g}; "
              f"per period (start, stopped, failed, exact, run, planned) {r.screen}; (screened steps, RS) {r.rows}")
        tc._same(r.tabs, ref, f"{w.name}: RS = {rs} != oracle")
        assert [x[1] for x in r.rows] == [rs] * w.T
        assert sum(s[1] for s in r.screen) > 0, "no block was screened and stopped"
        assert sum(s[2] for s in r.screen) >= 1, "no screen failed"
        for s, o, (screened, _) in zip(r.screen, off.screen, r.rows):
            assert s[1] + s[3] == o[3] and s[5] == o[5]
            assert 0 < screened <= s[4]
        assert sum(s[4] for s in r.screen) == r.run < off.run
    tc._same(off.tabs, ref, f"{w.name}: screen off != oracle")
    assert runs[4].screen == PARENT[key]
    assert runs[4].ops > runs[2].ops > runs[1].ops
    for rs in (2, 1):
        assert abs(runs[rs].run - runs[4].run) <= 0.05 * runs[4].run


@pytest.mark.gpu
def test_screen_rows_where_nothing_ever_stops(sia, oracle, monkeypatch):
    """The flat-cost grid (every sum +0.0, nothing strictly beaten): for every RS all planned steps ran, none of them in a
    screened pass, and the tables are the oracle's."""
    w = tc._grid(900, 130, 16, K=0.0, v=0.0, h=0.0, pi=0.0)
    V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
    for rs in (4, 2, 1):
        r = _run(sia, w, monkeypatch, rows=rs)
        tc._same(r.tabs, list(zip(V, pol)), f"{w.name}: RS = {rs} != oracle")
        assert r.run == r.planned > 0
        assert [x[0] for x in r.rows] == [0] * w.T and all(s[1] == 0 and s[2] == 0 for s in r.screen)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [None, 1])
def test_screen_rows_captured_sweep(sia, oracle, monkeypatch, rows):
    """SDPGPU_GRAPH=1 on the 26000-state grid, default RS and RS = 1: eager, captured, replayed -- the oracle's tables and the
    same counters each time, the screened steps among them (the captured sweep resets all six per period)."""
    w, ref = _grid_and_oracle(sia, oracle, monkeypatch, "D200")
    seen = _run(sia, w, monkeypatch, rows=rows, graph=1, calls=3)
    for call, r in enumerate(seen, start=1):
        tc._same(r.tabs, ref, f"{w.name}: call {call}")
    assert all(r[1:] == seen[0][1:] for r in seen[1:])
    assert all(screened > 0 and rs == (rows or 2) for screened, rs in seen[0].rows)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["max", "negative-cost", "cutoff-off"])
def test_screen_rows_gate(sia, oracle, monkeypatch, case):
    """Behind the cut-off's gate and nothing weaker: MAX, a negative cost parameter or SDPGPU_F1_CUTOFF=0 -- no step is
    walked in a screened pass whatever RS says, and the tables are the oracle's."""
    w = tc._grid(2000, 300, 128, direction=OptDirection.MAX if case == "max" else OptDirection.MIN,
                 v=-1.0 if case == "negative-cost" else 1.0)
    V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
    for rs in (1, 2):
        r = _run(sia, w, monkeypatch, rows=rs, cutoff=0 if case == "cutoff-off" else None)
        tc._same(r.tabs, list(zip(V, pol)), f"{w.name} ({case}): RS = {rs} != oracle")
        assert r.rows == [(0, rs)] * w.T and r.screen == [(0,) * 6] * w.T
        assert r.run == r.planned > 0


@pytest.mark.gpu
def test_bad_screen_rows_are_refused_at_create_time(sia, monkeypatch):
    w = tc._grid(2000, 300, 128)
    monkeypatch.setenv("SDPGPU_F1_SCREEN_ROWS", "3")
    with pytest.raises(sia._abi.SdpgpuError, match="SDPGPU_F1_SCREEN_ROWS=3"):
        sia.SdpEngine(w.desc(), w.pmf, w.overhead())
