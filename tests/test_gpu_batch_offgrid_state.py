"""How the two batch rollouts carry the state when a demand is NOT a multiple of the step ("Batched simulation" and
"Batched (s, S) level rules").  The table rollout snaps to the grid every period -- the index of the clamped level is truncated
toward zero, clamped into the row, and the next period starts from min + idx * step, as the handle's rollout does --; the rule
rollout carries the clamped level as the double it is.  Both are this engine's own defined behaviour (the oracle calls an
off-grid state invalid), so the references are a handle of each instance, a restatement in numpy below, and the independent
twin of the rule rollout (tests/fitss_twin.py), each bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fitss_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu

T = 4
GRIDS = ((-6, 9, 5), (-3, 12, 4), (-10, 5, 7))  # lowest state, highest state, order limit: in steps (16 states each)
COSTS = ((40.0, 1.0, 1.0, 5.0), (0.0, 0.0, 2.0, 10.0), (5.0, 2.5, 3.0, 3.0))  # K, v, h, pi
N_PATHS = (1, 64, 65)
# One batch with the unit step and one with another: 2, the smallest other step the library takes (a descriptor's step must be
# a power-of-two INTEGER; sdpgpu_batch_create refuses 0.5 with SDPGPU_ERR_UNSUPPORTED, before and after this test was written).
STEPS = [1.0, 2.0]


def _instances(sia, step):
    rng = np.random.default_rng(20240711)
    functors, pmfs = [], []
    for i, ((lo, hi, limit), (K, v, h, pi)) in enumerate(zip(GRIDS, COSTS)):
        functors.append(sia.BackorderFunctor(fixedOrderingCost=K, variOrderingCost=v, holdingCost=h, penaltyCost=pi, minInventory=lo * step,
                                             maxInventory=hi * step, maxOrderQuantity=limit * step, stepSize=step, iniInventory=0.0))
        tiles = []
        for t in range(T):
            D = 3 + (i + t) % 3
            p = rng.random(D) + 0.05
            tiles.append(np.stack([((i + t) % 3 - 1 + np.arange(D)) * step, p / p.sum()], axis=1))
        pmfs.append(tiles)
    return functors, pmfs


def _cases(functors, step):
    """Per n_paths: demands [N, n_paths, T] from the multiples of 0.25 in [-3, 9] (about half of them off either grid), a few
    far beyond every grid on either side, and a start state on the grid for every instance."""
    rng = np.random.default_rng(97)
    out = []
    for n_paths in N_PATHS:
        dem = rng.integers(-12, 37, size=(len(functors), n_paths, T)).astype(np.float64) / 4
        if n_paths > 1:
            dem[0, 3, 1], dem[1, 7, 0], dem[2, n_paths - 1, 2], dem[2, 5, 3] = 1000.0, -1000.0, 1000.0, -1000.0
        ini = np.array([f.minInventory + step * float(rng.integers(0, 16)) for f in functors])
        out.append((n_paths, dem, ini))
    assert all(np.mean(dem % step != 0) > 0.3 for _, dem, _ in out)
    return out


def _table_rollout(f, pol, dem, x0):
    """The snap restated: truncate toward zero, clamp the index, restart from min + idx * step."""
    step, lo, hi, n = f.stepSize, f.minInventory, f.maxInventory, len(pol[0])
    out = np.empty(len(dem))
    for p, row in enumerate(dem):
        idx, total = int((x0 - lo) / step), 0.0
        for t in range(T):
            x, a = lo + idx * step, float(pol[t][idx]) * step
            level = (x + a) - float(row[t])
            total += (((f.fixedOrderingCost if a > 0 else 0.0) + f.variOrderingCost * a) + f.holdingCost * max(level, 0.0)) + f.penaltyCost * max(-level, 0.0)
            nx = max(min(level, hi), lo)
            idx = min(max(int((nx - lo) * (1.0 / step)), 0), n - 1)
        out[p] = total
    return out


@pytest.mark.parametrize("step", STEPS)
def test_table_rollout_snaps_to_the_grid_as_a_handle_does(sia, step):
    functors, pmfs = _instances(sia, step)
    descs = [f.to_desc(T) for f in functors]
    cases = _cases(functors, step)
    with sia.SdpBatch(descs, pmfs, ragged=True, device=0) as b:
        b.solve()
        got = [b.simulate(dem, ini_x=ini, want_sums=True)[1] for _, dem, ini in cases]
        pols = [[b.policy(i, t + 1) for t in range(T)] for i in range(len(functors))]
    snapped = 0
    for i, f in enumerate(functors):
        d = f.to_desc(T)
        d.device = 0
        with sia.SdpEngine(d, pmfs[i]) as eng:
            eng.solve()
            for c, (n_paths, dem, ini) in enumerate(cases):
                want, ok = eng.simulate(dem[i], np.ones(T), float(ini[i]))
                assert ok.all()
                assert np.array_equal(got[c][i], want), (step, i, n_paths, "handle")
                assert np.array_equal(got[c][i], _table_rollout(f, pols[i], dem[i], float(ini[i]))), (step, i, n_paths, "restatement")
                snapped += int(np.sum(dem[i] % step != 0))
    assert snapped > 0


def _rules(functors, step, levels):
    """Thresholds strictly between grid points, spread over the grid so that the middle bands are met; fractional S."""
    rng = np.random.default_rng(1234 + levels)
    out = np.empty((len(functors), T, 2 * levels))
    for i, f in enumerate(functors):
        for t in range(T):
            at = np.sort(rng.choice(np.arange(3, 14), size=levels, replace=False))
            out[i, t, 0::2] = f.minInventory + (at + rng.choice([0.25, 0.5, 0.75], size=levels)) * step
            out[i, t, 1::2] = out[i, t, 0::2] + rng.integers(1, 24, size=levels) * 0.25 * step
    return out


def _states(levels, rule, dem, ini, f):
    """The states the twin's rollout visits: x[p][t] at the start of period index t."""
    xs = np.empty(dem.shape)
    for p, row in enumerate(dem):
        x = float(ini)
        for t in range(T):
            xs[p, t] = x
            a = tw.order_quantity(levels, t, x, float(ini), [float(z) for z in rule[t]], float(f.maxOrderQuantity))
            x = min(max((x + a) - float(row[t]), f.minInventory), f.maxInventory)
    return xs


@pytest.mark.parametrize("step", STEPS)
def test_rule_rollout_carries_the_state_unsnapped_as_the_twin_does(sia, step):
    functors, pmfs = _instances(sia, step)
    descs = [f.to_desc(T) for f in functors]
    cases = _cases(functors, step)
    with sia.SdpBatch(descs, pmfs, ragged=True, device=0) as b:  # NOT solved: the rules are explicit
        for levels in (1, 2, 3):
            rules = _rules(functors, step, levels)
            assert np.all(((rules[:, :, 0::2] - np.array([f.minInventory for f in functors])[:, None, None]) / step) % 1 != 0)
            middle = off_grid = 0
            for n_paths, dem, ini in cases:
                _, sums = b.simulate_ss(levels, dem, ss=rules, ini_x=ini, want_sums=True)
                for i, f in enumerate(functors):
                    want = tw.rollout(levels, rules[i], dem[i], ini[i], f.maxOrderQuantity, f.fixedOrderingCost, f.variOrderingCost,
                                      f.holdingCost, f.penaltyCost, f.minInventory, f.maxInventory)
                    assert np.array_equal(sums[i], want), (step, levels, n_paths, i)
                    xs = _states(levels, rules[i], dem[i], ini[i], f)
                    off_grid += int(np.sum(((xs - f.minInventory) / step) % 1 != 0))
                    if levels > 1:
                        middle += int(np.sum((rules[i][None, 1:, 0] <= xs[:, 1:]) & (xs[:, 1:] < rules[i][None, 1:, 2])))
            assert off_grid > 0, "some state between grid points"
            assert levels == 1 or middle > 0, "o[0] <= x < o[2] for some (instance, period, path)"
