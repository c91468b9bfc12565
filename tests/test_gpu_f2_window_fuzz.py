"""Randomised parity of the F2 row-window kernel (window_f2_kernel / window_combine_kernel, launched by launch_row_window) at the
sizes where it changes shape: action counts around the register blocks of 4 / 5 / 8 actions and around four waves of them,
inventory rows around tiles of 64, 128 and 256 states, pmf widths around the multiples of 4 the demand loop pads to and around
the 192 and 384 slots one and two staging passes cover, supports that start above zero, have gaps and zero weights, K > 0, K = 0
and K = v = 0 (every action of period T ties exactly), clamped rows anywhere below zero, growing unclamped grids, lead times 1 and 2.
Every instance is solved under the automatic plan and under forced S, R and chunk counts, on the generic kernel and in the exact
level mode, every period against the CPU oracle bit for bit; every fourth one also as 2 .. 5 rank slabs.  sdpgpu_plan_period says
which instantiation, how many chunks and how many blocks per wave each launch takes; a CPU test asserts that the generator with
these switch sets reaches every one of them.  Sizes are small: seconds."""
import numpy as np
import pytest

import test_gpu_fuzz as tf
import test_gpu_parity as tp
from stochastic_inventory_amd import workloads
from stochastic_inventory_amd.functors import LeadtimeFunctor
from stochastic_inventory_amd.states import OptDirection

_SWITCHES = ("SDPGPU_WIN_R", "SDPGPU_WIN_S", "SDPGPU_WIN_NCH")
ACTIONS_LEAD1 = (1, 2, 4, 5, 8, 9, 16, 17, 20, 21, 32, 33, 41)
ACTIONS_LEAD2 = (1, 2, 5, 9, 17)
RANGE_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
RANGE_LENGTHS_LEAD2 = RANGE_LENGTHS[:8]
PMF_WIDTHS = (1, 3, 4, 5, 60, 61, 64, 65, 124, 125, 128, 129)
N_INSTANCES = 48
SWITCH_SETS = [{}, {"SDPGPU_WIN_S": "1"}, {"SDPGPU_WIN_S": "2"}, {"SDPGPU_WIN_S": "4"}, {"SDPGPU_WIN_R": "4"}, {"SDPGPU_WIN_R": "5"},
               {"SDPGPU_WIN_R": "8"}, {"SDPGPU_WIN_NCH": "1"}, {"SDPGPU_WIN_NCH": "2"}, {"SDPGPU_WIN_R": "8", "SDPGPU_WIN_S": "2"},
               {"SDPGPU_WIN_R": "5", "SDPGPU_WIN_S": "4"}]
LAUNCHABLE = {(4, 1), (5, 1), (8, 1), (4, 2), (5, 2), (8, 2), (4, 4), (5, 4)}   # the instantiations of launch_row_window


def _ids(env):
    return ",".join(f"{k[11:]}={v}" for k, v in env.items()) or "planned"


def make_row_window_instance(seed):
    """Family 2, MIN (the ABI refuses MAX).  Two seeds in three have lead time 1 with A from ACTIONS_LEAD1, one in three lead time 2
    with A from ACTIONS_LEAD2 (a period has nx A^2 states there).  Clamped rows of RANGE_LENGTHS points (lead time 2: up to 129)
    whose lower bound lies anywhere in -(nx - 1) .. 0; one lead-time-1 instance in three is unclamped (the grid grows per period).
    Pmf tiles of PMF_WIDTHS points, mixed within an instance, whose support starts at 0 .. 3, has gaps once in four (laid out with
    zero padding by the library) and carries zero weights at its ends and inside.  T = 1 .. 3.  Integer, dyadic or decimal costs;
    K = 0 in one instance of three, K = v = 0 in one of six."""
    rng = np.random.default_rng(52000 + seed)
    lead2 = seed % 3 == 2
    kind = ["int", "dyadic", "decimal"][int(rng.integers(0, 3))]
    T = int(rng.integers(1, 4))
    if lead2:
        n2 = seed // 3
        A = ACTIONS_LEAD2[n2 % len(ACTIONS_LEAD2)]
        clamp, nx = True, RANGE_LENGTHS_LEAD2[(3 * n2) % len(RANGE_LENGTHS_LEAD2)]
    else:
        n1 = seed // 3 * 2 + seed % 3
        A = ACTIONS_LEAD1[n1 % len(ACTIONS_LEAD1)]
        clamp = n1 % 3 != 2
        nx = RANGE_LENGTHS[(5 * (n1 - (n1 + 1) // 3)) % len(RANGE_LENGTHS)]
    ties = (seed + seed // 6) % 6
    K = 0.0 if ties in (0, 3) else max(0.5, tf._money(rng, 1, 40, kind))
    v = 0.0 if ties == 0 else max(0.25, tf._money(rng, 0, 3, kind))
    lo = -float(rng.integers(0, nx))
    f = LeadtimeFunctor(fixedOrderingCost=K, variOrderingCost=v, holdingCost=tf._money(rng, 0, 3, kind),
                        penaltyCost=tf._money(rng, 0, 12, kind), maxOrderQuantity=float(A - 1), clampInventory=clamp,
                        minInventory=lo if clamp else 0.0, maxInventory=lo + nx - 1 if clamp else 0.0,
                        iniInventory=lo + float(rng.integers(0, nx)) if clamp else float(rng.integers(-3, 4)), iniPreQ=0.0,
                        leadTime=2 if lead2 else 1)
    tiles = []
    for t in range(T):
        n = int(PMF_WIDTHS[(seed + 5 * t + seed // 12) % len(PMF_WIDTHS)])
        d0 = float(rng.integers(0, 4))
        if n > 1 and rng.integers(0, 4) == 0:
            d = d0 + np.append(0, np.sort(rng.choice(np.arange(1, 2 * n), size=n - 1, replace=False))).astype(np.float64)
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
    return workloads.Workload(f"fuzz_f2_window_{seed}_L{2 if lead2 else 1}_A{A}", f, OptDirection.MIN, tiles)


def instances():
    return [make_row_window_instance(seed) for seed in range(N_INSTANCES)]


def _engine(sia, w, monkeypatch, env, kernel=0, **kw):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = w.desc()
    d.kernel = kernel
    for k, v in kw.items():
        setattr(d, k, v)
    return sia.SdpEngine(d, w.pmf, w.overhead())


def _demand_steps(tile):
    """Demand steps of the unit-stride layout of a pmf tile (step 1): its support, gaps included."""
    return int(tile[-1, 0] - tile[0, 0]) + 1


def test_switch_sets_reach_every_row_window_plan(sia, monkeypatch):
    """Host arithmetic only (sdpgpu_plan_period, which asks the function launch_row_window asks).  Over the generator's periods,
    under the automatic plan and each forced switch set of the GPU tests: every launchable (r, s) occurs; several chunks per tile
    occur (window_combine_kernel runs); one chunk whose waves walk several blocks, re-staging their rows, occurs; rows of several
    tiles with a ragged last one occur; one, two and three staging passes over a row segment occur; at most one instance in five
    has no period on the row-window kernel.  And the generator covers every action count, range length and pmf width asked for,
    both lead times, clamped and unclamped grids, supports with offsets, gaps and zero weights, K > 0, K = 0 and K = v = 0."""
    ws = instances()
    seen = {}
    for env in SWITCH_SETS:
        here = seen.setdefault(_ids(env), {"rs": set(), "passes": set(), "chunked": 0, "long_chunk": 0, "ragged": 0, "missed": []})
        for w in ws:
            with _engine(sia, w, monkeypatch, env) as eng:
                on_window = 0
                for t in range(1, w.T + 1):
                    pl = eng.plan(t)
                    if pl.kernel != 2:
                        continue
                    on_window += 1
                    _, nx, _, nq = eng.grid(t)
                    assert (pl.r, pl.s) in LAUNCHABLE and pl.chunks >= 1 and pl.chunk_blocks >= 1, (w.name, t)
                    per_row = -(-nx // (64 * pl.s))
                    assert pl.tiles == per_row * nq and pl.tasks == pl.tiles * pl.chunks, (w.name, t)
                    assert 0 < pl.lds_bytes <= 160 * 1024 and pl.workgroups_per_cu == 160 * 1024 // pl.lds_bytes, (w.name, t)
                    assert (pl.chunks - 1) * pl.chunk_blocks * pl.r < int(w.functor.maxOrderQuantity) + 1 <= pl.chunks * pl.chunk_blocks * pl.r
                    here["rs"].add((pl.r, pl.s))
                    here["chunked"] += pl.chunks > 1
                    here["long_chunk"] += pl.chunks == 1 and pl.chunk_blocks > 4
                    here["ragged"] += per_row > 1 and nx % (64 * pl.s) != 0
                    if t < w.T:   # (period T stages no rows)
                        d_pad = -(-_demand_steps(w.pmf[t - 1]) // 4) * 4
                        here["passes"].add(-(-(64 * pl.s + d_pad + 2) // 192))
                if not on_window:
                    here["missed"].append(w.name)
        print(f"{_ids(env)}: (r, s) {sorted(here['rs'])}, passes {sorted(here['passes'])}, chunked {here['chunked']}, one long chunk "
              f"{here['long_chunk']}, ragged rows {here['ragged']}, without a window period {here['missed']}")
        assert 5 * len(here["missed"]) <= len(ws), _ids(env)
    every = list(seen.values())
    assert set().union(*(s["rs"] for s in every)) == LAUNCHABLE
    assert set().union(*(s["passes"] for s in every)) == {1, 2, 3}
    assert any(s["chunked"] for s in every) and any(s["long_chunk"] for s in every) and any(s["ragged"] for s in every)
    assert seen["planned"]["chunked"] and seen["planned"]["ragged"]    # the default path itself combines chunks
    lead1 = [w for w in ws if w.functor.leadTime == 1]
    lead2 = [w for w in ws if w.functor.leadTime == 2]
    assert 3 * len(lead2) == len(ws) and all(w.direction == OptDirection.MIN for w in ws)
    assert {int(w.functor.maxOrderQuantity) + 1 for w in lead1} == set(ACTIONS_LEAD1)
    assert {int(w.functor.maxOrderQuantity) + 1 for w in lead2} == set(ACTIONS_LEAD2)
    length = lambda w: int(w.functor.maxInventory - w.functor.minInventory) + 1  # noqa: E731
    clamped = [w for w in lead1 if w.functor.clampInventory]
    assert 3 * (len(lead1) - len(clamped)) in range(len(lead1) - 2, len(lead1) + 3) and all(w.functor.clampInventory for w in lead2)
    assert {length(w) for w in clamped} == set(RANGE_LENGTHS) and {length(w) for w in lead2} == set(RANGE_LENGTHS_LEAD2)
    assert all(-(length(w) - 1) <= w.functor.minInventory <= 0 for w in clamped + lead2)
    assert any(w.functor.minInventory == 0 for w in clamped + lead2) and any(w.functor.minInventory < -100 for w in clamped)
    assert {len(t) for w in ws for t in w.pmf} == set(PMF_WIDTHS) and any(len({len(t) for t in w.pmf}) > 1 for w in ws)
    assert {w.T for w in ws} == {1, 2, 3} and any(w.T == 3 and not w.functor.clampInventory for w in ws)
    assert {int(t[0, 0]) for w in ws for t in w.pmf} == {0, 1, 2, 3}
    gapped = sum(1 for w in ws for t in w.pmf if np.any(np.diff(t[:, 0]) > 1))
    assert 0 < gapped < sum(w.T for w in ws) / 2
    assert any(t[0, 1] == 0 and t[-1, 1] == 0 for w in ws for t in w.pmf) and any(np.any(t[1:-1, 1] == 0) for w in ws for t in w.pmf)
    for group in (lead1, lead2):
        assert any(w.functor.fixedOrderingCost > 0 for w in group)
        assert any(w.functor.fixedOrderingCost == 0 and w.functor.variOrderingCost > 0 for w in group)
        assert any(w.functor.fixedOrderingCost == 0 and w.functor.variOrderingCost == 0 for w in group)
    zero_K = sum(1 for w in ws if w.functor.fixedOrderingCost == 0)
    ties = sum(1 for w in ws if w.functor.fixedOrderingCost == 0 and w.functor.variOrderingCost == 0)
    assert 3 * zero_K == len(ws) and 6 * ties == len(ws)


def _wide_pmf_instance():
    """5 actions x 3495 demand steps: the planner's block of 5 actions stages five row segments of 3626 slots per wave, 174 KiB
    with the level row -- over a compute unit's 160 -- for every period with a future; period T stages none."""
    return workloads.cfg4_leadtime(T=2, NX=80, A=5, D=3495)


def test_row_window_plan_over_the_lds(sia, monkeypatch):
    """Host arithmetic only.  Under the automatic choice with nothing forced such a period runs on the generic kernel, and the
    plan says so; asked for (kernel = WINDOW, or a forced block) the plan is SDPGPU_ERR_ARG with the launcher's reason."""
    w = _wide_pmf_instance()
    with _engine(sia, w, monkeypatch, {}) as eng:
        pl = eng.plan(1)
        assert (pl.kernel, pl.r, pl.s, pl.chunks, pl.tiles, pl.lds_bytes) == (1, 0, 0, 0, 0, 0)
        pl = eng.plan(2)
        assert (pl.kernel, pl.r, pl.s, pl.chunks, pl.chunk_blocks, pl.tiles) == (2, 5, 2, 1, 1, 5)
    for env, kernel in (({}, 2), ({"SDPGPU_WIN_R": "5"}, 0), ({"SDPGPU_WIN_R": "8"}, 0)):
        with _engine(sia, w, monkeypatch, env, kernel=kernel) as eng:
            with pytest.raises(sia.SdpgpuError) as e:
                eng.plan(1)
            assert e.value.code == 1 and "row-window kernel: 3495 demand steps need" in e.value.message, (env, kernel)
            assert "of LDS per workgroup" in e.value.message
            assert eng.plan(2).kernel == 2
    with _engine(sia, w, monkeypatch, {"SDPGPU_WIN_R": "4"}) as eng:   # four segments per wave fit: 146 KiB
        pl = eng.plan(1)
        assert (pl.kernel, pl.r, pl.s, pl.workgroups_per_cu) == (2, 4, 2, 1) and 140000 < pl.lds_bytes <= 160 * 1024


# ---------------------------------------------------------------------------------------------------------------
# GPU: every plan against the oracle
# ---------------------------------------------------------------------------------------------------------------
_SOLVED = {}


def solved(oracle, w):
    """(values, policy, cells) of the oracle, once per instance for every variant (and every file) that needs them."""
    got = _SOLVED.get(w.name)
    if got is None:
        V, pol, cells = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=4)
        for a in list(V) + list(pol):
            a.setflags(write=False)
        got = _SOLVED[w.name] = (V, pol, cells)
    return got


def _assert_solution(eng, w, oracle, what):
    V, pol, cells = solved(oracle, w)
    assert eng.stats().cells_evaluated == cells, f"{w.name} {what}"
    for t in range(1, w.T + 1):
        assert np.array_equal(eng.policy(t), pol[t - 1]), f"{w.name} {what}: policy of period {t}"
        assert np.array_equal(eng.values(t), V[t - 1]), f"{w.name} {what}: values of period {t}"
    if w.functor.fixedOrderingCost == 0 and w.functor.variOrderingCost == 0:
        # every action of period T costs the same, bit for bit: the first one wins, across blocks, waves and chunks
        assert not np.any(pol[w.T - 1]) and not np.any(eng.policy(w.T)), f"{w.name} {what}: ties of period {w.T}"


@pytest.mark.gpu
@pytest.mark.parametrize("env", SWITCH_SETS, ids=_ids)
def test_row_window_plans_bit_exact(sia, oracle, monkeypatch, env):
    on_window = 0
    for w in instances():
        with _engine(sia, w, monkeypatch, env) as eng:
            planned = eng.plan(1).kernel
            eng.solve(sync=True)
            _assert_solution(eng, w, oracle, _ids(env))
            assert eng.stats().kernel_used == planned, f"{w.name} {_ids(env)}"   # what the plan said is what ran
            on_window += planned == 2
    assert 5 * on_window >= 4 * N_INSTANCES


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [1, 3], ids=["generic", "exact-level-mode"])
def test_other_kernels_bit_exact(sia, oracle, monkeypatch, kernel):
    for w in instances():
        with _engine(sia, w, monkeypatch, {}, kernel=kernel) as eng:
            assert eng.plan(1).kernel == 1    # (no window plan is reported for a handle that does not take that kernel)
            eng.solve(sync=True)
            _assert_solution(eng, w, oracle, f"kernel {kernel}")
            assert eng.stats().kernel_used == kernel, w.name


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"SDPGPU_WIN_S": "4"}], ids=_ids)
def test_row_window_slabs_bit_exact(sia, oracle, monkeypatch, env):
    """Every fourth instance as 2 .. 5 rank slabs (test_gpu_parity._run_sharded: every rank ends with the oracle's whole value
    tables, the policy slabs concatenate to the oracle's): slab ends inside 256-state tiles and inside preQ rows."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for n, w in enumerate(instances()[::4]):
        tp._run_sharded(sia, oracle, w, 2 + n % 4)


@pytest.mark.gpu
def test_row_window_plan_over_the_lds_runs_as_planned(sia, oracle, monkeypatch):
    """The instance of test_row_window_plan_over_the_lds: the automatic choice runs period 1 on the generic kernel as the plan
    says, the forced block of 4 actions runs it on the row-window kernel in 146 KiB of LDS, and kernel = WINDOW is refused with
    the plan's reason before anything is launched for period 1."""
    w = _wide_pmf_instance()
    for env, planned in (({}, 1), ({"SDPGPU_WIN_R": "4"}, 2)):
        with _engine(sia, w, monkeypatch, env) as eng:
            assert eng.plan(1).kernel == planned
            eng.solve(sync=True)
            _assert_solution(eng, w, oracle, _ids(env))
            assert eng.stats().kernel_used == planned
    with _engine(sia, w, monkeypatch, {}, kernel=2) as eng:
        with pytest.raises(sia.SdpgpuError) as e:
            eng.solve(sync=True)
        assert e.value.code == 1 and "of LDS per workgroup" in e.value.message
