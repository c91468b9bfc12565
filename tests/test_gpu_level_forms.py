"""The launch forms of the F1 level kernel on the device (window_f1_level_kernel<..., CLAIM>, csrc/sdp_window.hpp "THE LAUNCH
FORMS"; SDPGPU_F1_LEVEL_FORM = 0, 1 or 2 at create time): four tasks per 256-thread workgroup in index order, one wave per
workgroup, or resident waves that claim tasks from a counter -- the last two band 0 first, then from the last band down.  A form decides which
wave runs which task, and when, and nothing else: no table and no counter may depend on it, under any screen rows, with or
without the cut-off, eager or captured.

The grids, the forced plan and the helpers are those of tests/test_gpu_level_step_groups.py: 20000 states x 300 actions, D = 70
and D = 37, T = 3, bands of three level blocks (the last band ragged -- in that order a wave takes it early and then whole
bands in the same LDS region), two action blocks, failed screens, period T and the keyed future form.

Where form 2 is asked for, the period-T instantiations that have three waves per SIMD -- no cut-off, or the cut-off with all
four rows screened -- run as form 1 (the claim loop would cost them the third wave: profiles/f1_level_forms_resources.txt);
sdpgpu_f1_level_form_get reports the form that ran, and `_expect` below is that rule."""
import pytest

import level_cut_twin
import test_gpu_level_step_groups as sg
import test_level_cutoff as tc

_FORM_ENV = ("SDPGPU_F1_LEVEL_FORM", "SDPGPU_F1_LEVEL_WGS", "SDPGPU_F1_LEVEL_ROUNDS")
_ENV = sg._ENV + _FORM_ENV
_RESIDENT_WGS = 512  # kLevelResidentWgs: 2048 wave slots / 4
_BASE = {}   # form 0 per (grid, RS, cut-off): computed once, not changed afterwards
_SMALL = {}


def _expect(form, t, T, tasks, cut=True, rows=2, wgs=None):
    """(form, workgroups, threads per workgroup) that period t's level launch must report."""
    if form == 2 and t == T and (not cut or rows == 4):
        form = 1
    if form == 1:
        return (1, tasks, 64)
    if form == 2:
        return (2, min(-(-tasks // 4), wgs or _RESIDENT_WGS), 256)
    return (0, -(-tasks // 4), 256)


def _run(sia, w, monkeypatch, geometry, form=None, rows=None, wgs=None, cutoff=None, graph=None, calls=1):
    """sg._run with the switches of the forms: a Run per call, and per call what every period's launch reported."""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (("SDPGPU_WIN_LEVEL", 1), ("SDPGPU_F1_SCREEN", 1), ("SDPGPU_F1_SCREEN_LOG2", 4), ("SDPGPU_GRAPH", graph),
                 ("SDPGPU_F1_SCREEN_ROWS", rows), ("SDPGPU_F1_CUTOFF", cutoff), ("SDPGPU_F1_LEVEL_FORM", form),
                 ("SDPGPU_F1_LEVEL_WGS", wgs)):
        if v is not None:
            monkeypatch.setenv(k, str(v))
    out = []
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        S, A, D = geometry
        # a level plan: bands of three level blocks (2000 states: of one), two action blocks, the steps padded to a multiple of 8
        assert level_cut_twin.plan_geometry(eng.plan(1), S, A, D) == (24 if S == 20000 else 8, 2, -(-D // 8) * 8)
        tasks = [int(eng.plan(t).tasks) for t in range(1, w.T + 1)]
        for _ in range(calls):
            eng.solve(sync=True)
            tabs = [(eng.values(t), eng.policy(t)) for t in range(1, w.T + 1)]
            st = eng.stats()
            r = sg.Run(tabs, int(st.f1_level_steps_planned), int(st.f1_level_steps_run), float(st.fp64_ops_executed),
                       [eng.f1_screen(t) for t in range(1, w.T + 1)], [eng.f1_screen_rows(t) for t in range(1, w.T + 1)])
            forms = [eng.f1_level_form(t) for t in range(1, w.T + 1)]
            want = [_expect(form or 0, t, w.T, tasks[t - 1], cut=cutoff != 0, rows=rows or 2, wgs=wgs) for t in range(1, w.T + 1)]
            if form is not None:
                assert forms == want, f"{w.name}: form {form}: the launches report {forms}, not {want}"
            out.append(r)
    return out[0] if calls == 1 else out


def _base(sia, key, w, monkeypatch, rows=None, cutoff=None):
    """Form 0 -- the launch before there were forms -- on grid `key`: what every other form must reproduce."""
    k = (key, rows, cutoff)
    if k not in _BASE:
        _BASE[k] = _run(sia, w, monkeypatch, sg._GRIDS[key], form=0, rows=rows, cutoff=cutoff)
    return _BASE[k]


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(sg._GRIDS))
def test_forms_parity_and_counters(sia, oracle, monkeypatch, key):
    """Forms 0, 1, 2 at the default RS and SG, and form 2 at RS = 1 and 4: every table is the oracle's, bit for bit, every
    counter -- steps planned and run, the priced operations (tests), blocks screened and stopped, screens failed, exact walks,
    screened steps -- is form 0's at the same RS, and every launch reports the form, grid and workgroup size of `_expect`.
    At these grids a plan has 1692 tasks: 423 workgroups in forms 0 and 2, 1692 in form 1."""
    w, ref = sg._oracle_tables(oracle, key)
    S, A, D = sg._GRIDS[key]
    for rs, forms in ((None, (0, 1, 2)), (1, (2,)), (4, (2,))):
        base = _base(sia, key, w, monkeypatch, rows=rs)
        tc._same(base.tabs, ref, f"{w.name}: form 0, RS = {rs} != oracle")
        assert sum(s[1] for s in base.screen) > 0 and sum(s[2] for s in base.screen) >= 1 and 0 < base.run < base.planned
        for form in forms:
            r = base if form == 0 else _run(sia, w, monkeypatch, (S, A, D), form=form, rows=rs)
            print(f"{w.name} RS={rs} form={form}: steps planned {r.planned}, run {r.run}, fp64 ops {r.ops:.9g}; per period "
                  f"(start, stopped, failed, exact, run, planned) {r.screen}; (screened steps, RS) {r.rows}")
            tc._same(r.tabs, ref, f"{w.name}: form {form}, RS = {rs} != oracle")
            assert r[1:] == base[1:], f"{w.name}: RS = {rs}: the counters of form {form} are not those of form 0"
    unset = _run(sia, w, monkeypatch, (S, A, D))  # the default form, whichever it is
    tc._same(unset.tabs, ref, f"{w.name}: default form != oracle")
    assert unset[1:] == _base(sia, key, w, monkeypatch)[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("wgs", [1, 3, 5])
def test_form2_few_workgroups(sia, oracle, monkeypatch, wgs):
    """SDPGPU_F1_LEVEL_WGS = 1, 3, 5: 4, 12 and 20 waves for 1692 tasks.  Every wave runs hundreds of tasks one after the
    other in one LDS region, the task count is not a multiple of the wave count (1692 = 12 x 141, but not of 4 x 5 = 20, and the
    waves do not take equal shares anyway), and the queue runs dry while other waves are still at work."""
    w, ref = sg._oracle_tables(oracle, "D70")
    base = _base(sia, "D70", w, monkeypatch)
    r = _run(sia, w, monkeypatch, sg._GRIDS["D70"], form=2, wgs=wgs)
    tc._same(r.tabs, ref, f"{w.name}: form 2 on {wgs} workgroups != oracle")
    assert r[1:] == base[1:], f"{w.name}: form 2 on {wgs} workgroups: the counters are not those of form 0"


@pytest.mark.gpu
def test_form2_grid_larger_than_the_queue_needs(sia, oracle, monkeypatch):
    """2000 states, the cap at 512: 576 one-block tasks on 144 workgroups.  A task is so short that the waves dispatched first
    empty the queue; the ones that start later claim nothing and must leave cleanly, and nothing may depend on how many did."""
    geometry = (2000, 300, 70)
    if "w" not in _SMALL:
        w = tc._grid(*geometry, T=3, lo=-300, h=0.2)
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
        _SMALL["w"], _SMALL["ref"] = w, list(zip(V, pol))
    w, ref = _SMALL["w"], _SMALL["ref"]
    base = _run(sia, w, monkeypatch, geometry, form=0)
    r = _run(sia, w, monkeypatch, geometry, form=2, wgs=512)
    tc._same(base.tabs, ref, f"{w.name}: form 0 != oracle")
    tc._same(r.tabs, ref, f"{w.name}: form 2 != oracle")
    assert r[1:] == base[1:], f"{w.name}: the counters of form 2 are not those of form 0"


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_forms_without_the_cutoff(sia, oracle, monkeypatch, form):
    """SDPGPU_F1_CUTOFF=0: the CUT = false instantiations fill only the slots of their own states, there is no counter row,
    and the claim word is the only thing zeroed before the launch.  Every planned step runs, in every form."""
    w, ref = sg._oracle_tables(oracle, "D70")
    base = _base(sia, "D70", w, monkeypatch, cutoff=0)
    r = _run(sia, w, monkeypatch, sg._GRIDS["D70"], form=form, cutoff=0)
    tc._same(base.tabs, ref, f"{w.name}: form 0 without the cut-off != oracle")
    tc._same(r.tabs, ref, f"{w.name}: form {form} without the cut-off != oracle")
    assert r[1:] == base[1:] and r.run == r.planned > 0
    assert all(s == (0, 0, 0, 0, 0, 0) for s in r.screen)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_forms_captured_sweep(sia, oracle, monkeypatch, form):
    """SDPGPU_GRAPH=1 on one handle: eager, captured, replayed -- the oracle's tables and the eager sweep's counters each time
    (the captured sweep records the zeroing of the claim word with the launch)."""
    w, ref = sg._oracle_tables(oracle, "D70")
    base = _base(sia, "D70", w, monkeypatch)
    seen = _run(sia, w, monkeypatch, sg._GRIDS["D70"], form=form, graph=1, calls=3)
    for call, r in enumerate(seen, start=1):
        tc._same(r.tabs, ref, f"{w.name}: form {form}, call {call}")
        assert r[1:] == base[1:], f"{w.name}: form {form}, call {call}: counters differ from the eager form 0's"


@pytest.mark.gpu
@pytest.mark.parametrize("var,bad", [("SDPGPU_F1_LEVEL_FORM", b) for b in ("3", "-1", "2x", "", "01")] +
                         [("SDPGPU_F1_LEVEL_WGS", b) for b in ("0", "-4", "8k", "", "99999999999")] +
                         [("SDPGPU_F1_LEVEL_ROUNDS", b) for b in ("0", "65", "x", "", "2.5")])
def test_bad_form_switches_are_refused_at_create_time(sia, monkeypatch, var, bad):
    w = tc._grid(2000, 300, 37)
    for k in _FORM_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(var, bad)
    with pytest.raises(sia._abi.SdpgpuError, match=var + "=" + bad):
        sia.SdpEngine(w.desc(), w.pmf, w.overhead())
