"""The decided split of the F1 level kernel (csrc/sdpgpu_window.hip f1_decided_start), without a GPU: under the
cut-off's gate, holding for a period and every later one, action 0 wins in every state from an index c_t on and V_t is
non-decreasing there.  c_t is host arithmetic on the descriptor, the grids and the demand supports:
    c_t = max(0, m0_t + D_t - 1, c_{t+1} - idx_off_t + D_t - 1)
(m0_t the first level index that is >= 0, D_t the steps of the unit-stride demand layout, idx_off_t the index shift into the
next period's grid; the slab's end says "none").  Here: the claim against the oracle's full solve on a seeded fuzz, the gate,
and the plan / getter bookkeeping.  The device tests are in tests/test_gpu_level_decided.py."""
import ctypes as C

import numpy as np
import pytest

import test_level_cutoff as tc
from stochastic_inventory_amd import workloads
from stochastic_inventory_amd.functors import BackorderFunctor
from stochastic_inventory_amd.states import OptDirection

_ENV = tc._SWITCHES + ("SDPGPU_F1_SCREEN", "SDPGPU_F1_DECIDED", "SDPGPU_GRAPH")


def _env(monkeypatch, **kw):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        if v is not None:
            monkeypatch.setenv("SDPGPU_" + k, str(v))


def _tile(rng, D, d0, step):
    """[[d, p_d]] on D unit-stride steps from d0: a random pmf, some entries exactly 0 (never the two ends)."""
    p = rng.random(D) + 0.01
    if D > 3:
        p[1:-1][rng.random(D - 2) < 0.25] = 0.0
    p = p / p.sum()
    return np.column_stack([(d0 + np.arange(D)) * step, p])


def _instance(rng):
    S, A, T = int(rng.integers(40, 901)), int(rng.integers(1, 141)), int(rng.integers(1, 6))
    step = float(rng.choice([1.0, 1.0, 1.0, 2.0, 4.0]))
    lo = int(rng.choice([-600, -250, -70, -3, 0, 0, 5, 40]))
    K, v, h, pi = (float(rng.choice(c)) for c in ([0.0, 5.0, 500.0], [0.0, 1.0, 2.5], [0.0, 2.0, 0.3], [0.0, 10.0, 1.7]))
    d0 = int(rng.choice([0, 0, 3]))
    pmf = [_tile(rng, int(rng.integers(1, 71)), d0, step) for _ in range(T)]
    f = BackorderFunctor(fixedOrderingCost=K, variOrderingCost=v, holdingCost=h, penaltyCost=pi, minInventory=lo * step,
                         maxInventory=(lo + S - 1) * step, maxOrderQuantity=(A - 1) * step, stepSize=step,
                         iniInventory=lo * step)
    return workloads.Workload(f"dec_{S}x{A}x{T}_lo{lo}_step{step}", f, OptDirection.MIN, pmf, "decided-split fuzz"), S, lo, d0


def _expected(S, lo, d0, Ds):
    """The rule written again for one grid shared by all periods and integer levels: index of level 0 is d0 - lo."""
    out = []
    for t in range(len(Ds), 0, -1):
        D = Ds[t - 1]
        c = max(0, (d0 - lo) + D - 1)
        if out:  # (idx_off = -d0: the periods share the grid and the lowest demand)
            c = S if out[-1] >= S else max(c, out[-1] + d0 + D - 1)
        out.append(min(c, S))
    return out[::-1]


def test_the_claim_against_the_oracle(sia, oracle, monkeypatch):
    """Seeded fuzz (<= 900 states, <= 140 actions, <= 70 demands, T <= 5; costs of 0, grids from far below zero to above it,
    pmfs with zero entries, lowest demand 0 or 3, a D per period, steps 1, 2 and 4 -- the library takes power-of-two integer
    steps only): in every period the boundary is at most the slab's end, and from it on the oracle's policy is 0 and its
    values are non-decreasing.  The boundary is the rule written again above, exactly."""
    _env(monkeypatch)
    rng = np.random.default_rng(20241019)
    periods_with_states = 0
    for _ in range(60):
        w, S, lo, d0 = _instance(rng)
        with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
            if eng.plan(1).kernel != sia.KERNEL_WINDOW:
                continue
            c = [eng.f1_decided_start(t) for t in range(1, w.T + 1)]
            got = [eng.f1_decided(t) for t in range(1, w.T + 1)]
        want = _expected(S, lo, d0, [len(t) for t in w.pmf])
        assert c == want, w.name
        assert [g[0] for g in got] == c and all(g[1:4] == (S, 0, 0) for g in got)  # nothing has run
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=4)
        for t in range(w.T):
            assert 0 <= c[t] <= S, f"{w.name}: period {t + 1}"
            if c[t] < S:
                periods_with_states += 1
                assert not pol[t][c[t]:].any(), f"{w.name}: period {t + 1} orders above the boundary {c[t]}"
                assert np.all(np.diff(V[t][c[t]:]) >= 0), f"{w.name}: period {t + 1} decreases above the boundary {c[t]}"
    assert periods_with_states >= 40


def test_target_grid_boundaries(sia, monkeypatch):
    """The target grid (1e6 states from 0, 200 demands, six periods): c_t = 199 (7 - t)."""
    _env(monkeypatch)
    w = workloads.target_grid()
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        assert [eng.f1_decided_start(t) for t in range(1, 7)] == [199 * (7 - t) for t in range(1, 7)]


@pytest.mark.parametrize("case", ["max", "negative-cost", "negative-weight-later", "negative-weight-own", "caller-memory",
                                  "cutoff-off"])
def test_the_gate(sia, monkeypatch, case):
    """Where the cut-off's gate is closed the entry point says none (the slab's end): MAX, a negative cost, a negative
    probability in this or a later period (the periods above it keep their boundary), V_{t+1} in caller memory (period T keeps
    its boundary: it reads no values), SDPGPU_F1_CUTOFF=0."""
    _env(monkeypatch, F1_CUTOFF=0 if case == "cutoff-off" else None)
    w = tc._grid(2000, 300, 21, direction=OptDirection.MAX if case == "max" else OptDirection.MIN,
                 v=-1.0 if case == "negative-cost" else 1.0)
    if case == "negative-weight-later":
        w.pmf[1][0, 1] = -w.pmf[1][0, 1]
    if case == "negative-weight-own":
        w.pmf[0][0, 1] = -w.pmf[0][0, 1]
    keep = None
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        if case == "caller-memory":
            keep = (C.c_double * (eng.values_bytes() // 8))()  # (host arithmetic only: nothing is launched on it)
            eng.attach_values(C.addressof(keep), eng.values_bytes())
        got = [eng.f1_decided_start(t) for t in (1, 2, 3)]
    want = {"negative-weight-later": [2000, 2000, 20], "negative-weight-own": [2000, 40, 20],
            "caller-memory": [2000, 2000, 20]}.get(case, [2000, 2000, 2000])
    assert got == want
    del keep


def test_the_gate_user_cost_text(sia, monkeypatch):
    """User lambdas of the level shape (tables of any sign): none in every period."""
    _env(monkeypatch)
    w = workloads.custom_clsp_level(T=3, S=3000, A=300, D=40)
    with sia.SdpEngine(w.desc(), w.pmf, custom_source=w.custom_source, custom_params=w.custom_params) as eng:
        assert [eng.f1_decided_start(t) for t in (1, 2, 3)] == [3000] * 3


def _plan_tuple(p):
    return (p.kernel, p.r, p.s, p.chunks, p.chunk_blocks, p.tiles, p.tasks, p.workgroups_per_cu, p.lds_bytes)


def test_plan_and_getter_agree_with_the_boundary(sia, monkeypatch):
    """The plan reported is the plan launched: with the split, the level launch covers the live states alone -- bands of 16
    levels (two level blocks) over c_t + A - 1 levels, ceil((A - 1) / 16) + action blocks chunk rows -- the same twice in a row;
    under SDPGPU_F1_DECIDED=0, and under a forced plan without the switch, it is today's whole-slab plan.  The split is opt-in
    on the planner's own level plan as well: the target grid with no switch set keeps today's plan (the benchmark's contract
    test pins the default headline as a throughput-bound sweep), and splits with SDPGPU_F1_DECIDED=1."""
    w = tc._grid(1601, 500, 200, T=3)

    def plans(**kw):
        _env(monkeypatch, **kw)
        with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
            a = [_plan_tuple(eng.plan(t)) for t in (1, 2, 3)]
            b = [_plan_tuple(eng.plan(t)) for t in (1, 2, 3)]
            assert a == b
            return a, [eng.f1_decided(t) for t in (1, 2, 3)]

    forced, g0 = plans(WIN_LEVEL=1)
    off, g1 = plans(WIN_LEVEL=1, F1_DECIDED=0)
    on, g2 = plans(WIN_LEVEL=1, F1_DECIDED=1)
    assert forced == off and g0 == g1 == g2
    assert [g[0] for g in g2] == [597, 398, 199] and all(g[1:4] == (1601, 0, 0) for g in g2)
    for t, c in enumerate((597, 398, 199)):
        kernel, r, s, chunks, chunk_blocks, tiles, tasks = on[t][:7]
        assert (kernel, r, s, chunk_blocks) == (sia.KERNEL_WINDOW, 4, 8, 0)
        assert tiles == -(-(c + 499) // 16) and tasks == 2 * tiles and chunks == -(-499 // 16) + 2
        assert on[t] != off[t] and off[t][4] == 0
    # the planner's own level plan: the target grid splits with the switch, and neither without it nor with it at 0
    wt = workloads.target_grid()
    for kw, split in (({"F1_DECIDED": 1}, True), ({}, False), ({"F1_DECIDED": 0}, False)):
        _env(monkeypatch, **kw)
        with sia.SdpEngine(wt.desc(), wt.pmf, wt.overhead()) as eng:
            for t in range(1, 7):
                p = eng.plan(t)
                assert p.chunk_blocks == 0
                c = 199 * (7 - t)
                assert (p.tiles == -(-(c + 499) // 16)) == split, f"period {t}"
