"""The cut-off of the F1 level kernel (window_f1_level_kernel<..., CUT>, SDPGPU_F1_CUTOFF): a level block stops once no
action of it can still win.  Tables with the cut-off on against the same kernel with it off, the state-major
window_f1_kernel and the oracle, bit for bit, where it fires, where it must not fire and where the host's gate keeps it
off; the step counters of sdpgpu_stats say which of the three happened."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import level_cut_twin
from stochastic_inventory_amd import workloads
from stochastic_inventory_amd.functors import BackorderFunctor
from stochastic_inventory_amd.states import OptDirection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SWITCHES = ("SDPGPU_WIN_R", "SDPGPU_WIN_S", "SDPGPU_WIN_NCH", "SDPGPU_WIN_LEVEL", "SDPGPU_F1_CUTOFF")


def _grid(S, A, D, T=3, direction=OptDirection.MIN, lo=0, K=500.0, v=1.0, h=2.0, pi=10.0):
    f = BackorderFunctor(fixedOrderingCost=K, variOrderingCost=v, holdingCost=h, penaltyCost=pi, minInventory=lo,
                         maxInventory=lo + S - 1, maxOrderQuantity=A - 1, iniInventory=lo)
    return workloads.Workload(f"cut_{S}x{A}x{D}x{T}", f, direction, workloads.seasonal_pmf(T, D), "cut-off test")


def _solve(sia, w, monkeypatch, level, cutoff, **kw):
    """(tables of every period, steps planned, steps run) of one solve under the two switches."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDPGPU_WIN_LEVEL", str(level))
    if cutoff is not None:
        monkeypatch.setenv("SDPGPU_F1_CUTOFF", str(cutoff))
    if "custom_source" in kw:
        eng = sia.SdpEngine(w.desc(), w.pmf, **kw)
    else:
        eng = sia.SdpEngine(w.desc(), w.pmf, w.overhead(), **kw)
    with eng:
        assert (eng.plan(1).chunk_blocks == 0) == (level == 1)
        eng.solve(sync=True)
        tabs = [(eng.values(t), eng.policy(t)) for t in range(1, w.T + 1)]
        st = eng.stats()
        return tabs, int(st.f1_level_steps_planned), int(st.f1_level_steps_run)


def _same(a, b, what):
    for t, ((v1, p1), (v0, p0)) in enumerate(zip(a, b), start=1):
        assert np.array_equal(v1, v0) and np.array_equal(p1, p0), f"{what}: period {t}"


def _all_ways(sia, oracle, monkeypatch, w, with_oracle=True, **kw):
    """Cut-off on, off, the state-major kernel, the oracle: all the same bits.  Returns (planned, run) with the cut-off on."""
    on, planned, run = _solve(sia, w, monkeypatch, 1, None, **kw)
    off, planned_off, run_off = _solve(sia, w, monkeypatch, 1, 0, **kw)
    state, planned_sm, run_sm = _solve(sia, w, monkeypatch, 0, None, **kw)
    print(f"{w.name}: steps planned {planned}, run {run} ({run / max(planned, 1):.4f})")
    assert planned > 0 and planned_off == planned and run_off == planned  # SDPGPU_F1_CUTOFF=0: every step walked
    assert planned_sm == 0 and run_sm == 0                                # the level kernel did not run
    _same(on, off, f"{w.name}: cut-off on != off")
    _same(on, state, f"{w.name}: cut-off on != window_f1_kernel")
    if with_oracle:
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
        _same(on, list(zip(V, pol)), f"{w.name}: cut-off on != oracle")
    return planned, run


@pytest.mark.gpu
@pytest.mark.parametrize("S,A,D,lo", [(1601, 500, 200, 0), (900, 300, 40, 0), (700, 130, 16, 0), (2000, 300, 21, -700)],
                         ids=["A500-D200", "A300-D40", "A130-D16", "A300-D21-neg"])
def test_cutoff_fires_and_changes_nothing(sia, oracle, monkeypatch, S, A, D, lo):
    """Grids on which blocks do stop (a CPU emulation of the kernel's schedule walks 0.51 / 0.58 / 0.89 / 0.82 of the steps):
    every table of every period, period T included, is what the full walk gives, and steps were skipped.  The cap on the
    first grid is a condition that a cut-off which never fires cannot meet, not a performance figure."""
    planned, run = _all_ways(sia, oracle, monkeypatch, _grid(S, A, D, lo=lo))
    assert run < planned
    if (S, A, D) == (1601, 500, 200):
        assert run <= 0.75 * planned


@pytest.mark.gpu
def test_cutoff_flat_costs_never_stop(sia, oracle, monkeypatch):
    """K = v = h = pi = 0: every sum is +0.0, every action ties, nothing is ever strictly beaten -- every step is walked."""
    planned, run = _all_ways(sia, oracle, monkeypatch, _grid(900, 130, 16, K=0.0, v=0.0, h=0.0, pi=0.0))
    assert run == planned


@pytest.mark.gpu
def test_cutoff_low_fixed_cost_ties(sia, oracle, monkeypatch):
    """The tie instance of test_level_kernel_low_fixed_cost_ties: exact ties between actions of one state must keep the
    lowest action whether blocks stop or not."""
    f = BackorderFunctor(fixedOrderingCost=0, variOrderingCost=0, holdingCost=1, penaltyCost=1, minInventory=0,
                         maxInventory=1199, maxOrderQuantity=399, iniInventory=0)
    pmf = [np.column_stack([np.arange(8.0), np.full(8, 0.125)]) for _ in range(3)]
    _all_ways(sia, oracle, monkeypatch, workloads.Workload("cut_ties_1200x400x8x3", f, OptDirection.MIN, pmf, "ties"))


@pytest.mark.gpu
def test_cutoff_ties_where_blocks_stop(sia, oracle, monkeypatch):
    """Exact ties between actions of one state on a grid where blocks DO stop: no ordering cost at all and a uniform pmf of
    24 points, h = pi = 1 (all arithmetic exact in fp64, so equal costs are equal bits).  Orders that land on the same flat
    stretch of the cost tie, far too large orders are strictly beaten by action 0 and their blocks stop; the policy must
    still be the lowest optimal action everywhere."""
    f = BackorderFunctor(fixedOrderingCost=0, variOrderingCost=0, holdingCost=1, penaltyCost=1, minInventory=0,
                         maxInventory=1199, maxOrderQuantity=399, iniInventory=0)
    pmf = [np.column_stack([np.arange(24.0), np.full(24, 1.0 / 32)]) for _ in range(3)]
    for t in pmf:
        t[:8, 1] = 2.0 / 32  # dyadic probabilities summing to 1: every product and sum below is exact
    w = workloads.Workload("cut_ties_1200x400x24x3", f, OptDirection.MIN, pmf, "ties, blocks stop")
    planned, run = _all_ways(sia, oracle, monkeypatch, w)
    assert run < planned


@pytest.mark.gpu
def test_cutoff_grid_below_zero(sia, oracle, monkeypatch):
    """A grid lying wholly below zero (levels <= -402 even after the largest order): the highest action always wins, so the
    block that holds it is never beaten by action 0."""
    _all_ways(sia, oracle, monkeypatch, _grid(900, 300, 40, lo=-1600))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["max", "negative-cost", "level-shape"])
def test_cutoff_gate(sia, monkeypatch, case):
    """Where a running sum is no lower bound -- MAX, a negative cost parameter, user tables of the level shape -- the host
    keeps the cut-off off: the counters say every planned step ran, and the tables are the state-major kernel's."""
    kw = {}
    if case == "max":
        w = _grid(2000, 300, 21, direction=OptDirection.MAX)
    elif case == "negative-cost":
        w = _grid(2000, 300, 21, v=-1.0)
    else:
        w = workloads.custom_clsp_level(T=3, S=3000, A=300, D=40)
        kw = dict(custom_source=w.custom_source, custom_params=w.custom_params)
    on, planned, run = _solve(sia, w, monkeypatch, 1, None, **kw)
    state, planned_sm, run_sm = _solve(sia, w, monkeypatch, 0, None, **kw)
    assert planned > 0 and run == planned
    assert planned_sm == 0 and run_sm == 0
    _same(on, state, f"{w.name}: level kernel != window_f1_kernel")


def test_cutoff_stats_fields_match_the_header(sia):
    """The two counters are the last fields of sdpgpu_stats, at the offsets gcc gives them, and read 0 before a solve."""
    names = [f[0] for f in sia.SdpgpuStats._fields_]
    assert names[-2:] == ["f1_level_steps_planned", "f1_level_steps_run"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sdpgpu.h"\nint main(void){printf("%zu %zu %zu", '
           'offsetof(sdpgpu_stats, f1_level_steps_planned), offsetof(sdpgpu_stats, f1_level_steps_run), sizeof(sdpgpu_stats));'
           'return 0;}')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "a.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(td, "a"), os.path.join(td, "a.c")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(td, "a")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [sia.SdpgpuStats.f1_level_steps_planned.offset, sia.SdpgpuStats.f1_level_steps_run.offset,
                   C.sizeof(sia.SdpgpuStats)]
    w = _grid(700, 130, 16)
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        st = eng.stats()
        assert st.f1_level_steps_planned == 0 and st.f1_level_steps_run == 0


# ---------------------------------------------------------------------------------------------------------------
# Bands of several level blocks: what a task carries from one level block to the next (cut_first / cut_dec / cut_once, slots
# that earlier blocks have lowered, the epilogue skipped for some blocks of a task and written for others, the -inf slots of a
# ragged last band).  The device's step counter against the CPU twin's count (tests/level_cut_twin.py; its figures and the
# conditions these grids meet are checked on the CPU by tests/test_level_cut_twin.py).
# ---------------------------------------------------------------------------------------------------------------
def _case_grid(c):
    return _grid(c["S"], c["A"], c["D"], T=c["T"], lo=c["lo"], K=c["K"], v=c["v"], h=c["h"], pi=c["pi"])


def _level_geometry(sia, w, monkeypatch, c):
    """(band, action blocks, padded steps) of the level plan of `w`, from sdpgpu_plan_period."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDPGPU_WIN_LEVEL", "1")
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        return level_cut_twin.plan_geometry(eng.plan(1), c["S"], c["A"], c["D"])


@pytest.mark.gpu
@pytest.mark.parametrize("c", level_cut_twin.MULTI_BLOCK_GRIDS, ids=lambda c: c["id"])
def test_cutoff_bands_of_several_level_blocks(sia, oracle, monkeypatch, c):
    """Grids whose plan gives every task four to six level blocks (asserted from the plan, so that a planner change cannot
    return them to one): tables as in every test above, the planned steps are the host formula's -- level blocks of every
    band x action blocks x padded steps -- and the steps run are EXACTLY the twin's.  A test that reads another slot, a
    schedule that is not carried over as written or a slot outside the slab that holds a block back changes that count, mostly
    without changing a table."""
    w = _case_grid(c)
    planned, run = _all_ways(sia, oracle, monkeypatch, w)
    band, nb, d_pad = _level_geometry(sia, w, monkeypatch, c)
    assert band // 8 == c["blocks"] and band >= 32
    assert planned == c["T"] * level_cut_twin.planned_steps(c["S"], c["A"], band, nb, d_pad)
    assert run == sum(c["run"]), f"{w.name}: the device ran {run} steps, the twin {sum(c['run'])}"
    assert run <= 0.9 * planned


@pytest.mark.gpu
def test_cutoff_steps_are_the_twins_on_one_block_grids(sia, monkeypatch):
    """The four grids of test_cutoff_fires_and_changes_nothing (tables: there): the device counts the twin's steps, 0.5842 /
    0.6049 / 0.8942 / 0.7778 of the planned ones."""
    for c in level_cut_twin.ONE_BLOCK_GRIDS:
        _, planned, run = _solve(sia, _case_grid(c), monkeypatch, 1, None)
        print(f"{c['id']}: steps planned {planned}, run {run} ({run / planned:.4f})")
        assert run == sum(c["run"]), c["id"]
