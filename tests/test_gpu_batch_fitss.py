"""The (s, S) level rules of a batch on the GPU (sdpgpu_batch_fit_ss: batch_fit_ss_kernel; sdpgpu_batch_simulate_ss*:
batch_sim_kernel under LevelRule; DESIGN 4 "Batched (s, S) level rules").  The bar is bit equality throughout: the device fit against
sdpgpu_fit_ss on the batch's own read-back rows and against the independent twin (tests/fitss_twin.py) on the oracle's
tables; the rule rollout against the twin path for path; and, where the optimal policy IS one (s, S) rule, the rule rollout
against the table rollout of the same seed.  Means are held to math.fsum of the path sums at the batched simulation's 1e-13."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fitss_twin as tw  # noqa: E402
from test_fitss_host import lib_fit, opt_table, oracle_tables  # noqa: E402
from test_gpu_batch_ragged import _ragged_instances  # noqa: E402

pytestmark = pytest.mark.gpu


def _check_means(means, sums, what):
    """out_mean against math.fsum(sums) / n_paths within the 1e-13 relative of tests/test_gpu_batch_simulate.py (the same
    reduction: six tree levels in a wave plus the wave partials in order, at most 163 x 2^-53 for 10000 paths)."""
    for i in range(len(means)):
        want = math.fsum(sums[i].tolist()) / sums.shape[1]
        print(f"{what}: instance {i}: mean {means[i]!r} fsum {want!r}") if i < 2 else None
        assert abs(means[i] - want) <= 1e-13 * abs(want), (what, i, means[i], want)


def _assert_fit(sia, lib, functors, pmfs, T, tables, what):
    """fit_ss(levels) of the solved batch == sdpgpu_fit_ss on its own read-back rows == the twin on the oracle's tables."""
    with sia.RecursionBatch(functors, pmfs, device=0, ragged=True) as rb:
        rb._solve()
        own = [rb.getOptTable(i) for i in range(len(functors))]
        for i in range(len(functors)):
            assert np.array_equal(own[i], tables[i]), f"{what}: opt table of instance {i}"
        lengths = set()
        for levels in (1, 2, 3):
            got = rb.batch.fit_ss(levels)
            assert got.shape == (len(functors), T, 2 * levels)
            for i, f in enumerate(functors):
                max_q = int(f.maxOrderQuantity)
                assert np.array_equal(got[i], lib_fit(lib, levels, T, max_q, own[i])), f"{what}: host fit, instance {i}, {levels} level(s)"
                assert np.array_equal(got[i], tw.fit(levels, T, max_q, tables[i])), f"{what}: twin, instance {i}, {levels} level(s)"
            assert np.array_equal(got, rb.batch.fit_ss(levels)), "a second call gives the same bits"
        for i, f in enumerate(functors):
            for t in range(1, T):
                lengths.add(len(tw.level_index(tables[i][tables[i][:, 0] == t + 1], int(f.maxOrderQuantity))))
        return lengths


def test_fit_of_the_fitss_instances_equals_the_host_fit_and_the_twin(sia, oracle):
    from stochastic_inventory_amd import workloads
    lib = sia._abi.load()
    ws = workloads.fitss_sweep(patterns=(2, 7))
    assert len(ws) == 162
    functors, pmfs = [w.functor for w in ws], [w.pmf for w in ws]
    tables = oracle_tables(oracle, [w.desc() for w in ws], pmfs, workers=16)
    assert _assert_fit(sia, lib, functors, pmfs, 6, tables, "fitss") == {1, 2, 3}


def test_fit_of_the_ragged_mix_equals_the_host_fit_and_the_twin(sia, oracle):
    lib = sia._abi.load()
    T = 4
    functors, pmfs = _ragged_instances(sia, T=T)
    tables = oracle_tables(oracle, [f.to_desc(T) for f in functors], pmfs, workers=16)
    lengths = _assert_fit(sia, lib, functors, pmfs, T, tables, "ragged mix")
    print(f"\nragged mix: levelIndex list lengths {sorted(lengths)}")
    assert 1 in lengths


def _random_rules(rng, functors, T, levels):
    """Ascending thresholds inside the grid, order-up-to levels above them, most of them FRACTIONAL."""
    out = np.empty((len(functors), T, 2 * levels))
    for i, f in enumerate(functors):
        for t in range(T):
            s = np.sort(rng.uniform(f.minInventory - 2, f.maxInventory + 2, size=levels))
            if rng.random() < 0.5:
                s = np.round(s)
            S = s + rng.uniform(0.0, 40.0, size=levels)
            if rng.random() < 0.3:
                S = np.round(S * 4) / 4
            out[i, t, 0::2], out[i, t, 1::2] = s, S
    return out


def _twin_sums(levels, rules, demands, functors, ini=None):
    out = []
    for i, f in enumerate(functors):
        dem = demands if demands.ndim == 2 else demands[i]
        out.append(tw.rollout(levels, rules[i], dem, f.iniInventory if ini is None else ini[i], float(int(f.maxOrderQuantity)),
                              f.fixedOrderingCost, f.variOrderingCost, f.holdingCost, f.penaltyCost, f.minInventory, f.maxInventory))
    return np.stack(out)


def test_rule_rollout_with_explicit_demands_equals_the_twin_path_for_path(sia):
    T = 4
    functors, pmfs = _ragged_instances(sia, n=14, T=T, seed=31)
    N = len(functors)
    rng = np.random.default_rng(2718)
    descs = [f.to_desc(T) for f in functors]
    cases = []
    for n_paths in (1, 65, 200):
        shared = rng.integers(-15, 150, size=(n_paths, T)).astype(np.float64)
        per = rng.integers(-15, 150, size=(N, n_paths, T)).astype(np.float64)
        far = rng.random(per.shape)
        per[far < 0.03] = 1000.0   # far beyond every support and every grid
        per[far > 0.97] = -1000.0  # a negative demand larger than every grid
        ini = np.array([f.minInventory + float(rng.integers(0, int(f.maxInventory - f.minInventory) + 1)) for f in functors])
        cases.append((n_paths, shared, per, ini))
    with sia.SdpBatch(descs, pmfs, ragged=True, device=0) as b:  # NOT solved: the rules are explicit
        for levels in (1, 2, 3):
            rules = _random_rules(rng, functors, T, levels)
            assert np.any(rules[:, :, 1::2] != np.round(rules[:, :, 1::2])), "fractional S"
            for n_paths, shared, per, ini in cases:
                m1, s1 = b.simulate_ss(levels, shared, ss=rules, want_sums=True)
                m2, s2 = b.simulate_ss(levels, per, ss=rules, ini_x=ini, want_sums=True)
                assert np.array_equal(s1, _twin_sums(levels, rules, shared, functors)), (levels, n_paths, "shared")
                assert np.array_equal(s2, _twin_sums(levels, rules, per, functors, ini)), (levels, n_paths, "per instance")
                _check_means(m1, s1, f"{levels} level(s), shared n={n_paths}")
                _check_means(m2, s2, f"{levels} level(s), per-instance n={n_paths}")
                assert np.array_equal(m2, b.simulate_ss(levels, per, ss=rules, ini_x=ini)), "two calls, the same bits"
        with pytest.raises(sia.SdpgpuError) as e:  # no rule given: the fit needs the tables
            b.simulate_ss(1, cases[0][1])
        assert e.value.code == 2
        # the sampled demands are the table rollout's: the fused launch equals the explicit one fed sample_demands' paths
        rules = _random_rules(rng, functors, T, 3)
        ms, ss = b.simulate_ss_sampled(3, 1000, 4242, ss=rules, want_sums=True)
        dem = np.stack([b.sample_demands(i, 1000, 4242)[0] for i in range(N)])
        me, se = b.simulate_ss(3, dem, ss=rules, want_sums=True)
        assert np.array_equal(ss, se) and np.array_equal(ms, me)
        assert np.array_equal(se, _twin_sums(3, rules, dem, functors))
        # then solved: ss = None is the device fit, kept on the device
        b.solve()
        for levels in (1, 2, 3):
            fitted = b.fit_ss(levels)
            ma, sa = b.simulate_ss_sampled(levels, 1000, 7, want_sums=True)
            mb, sb = b.simulate_ss_sampled(levels, 1000, 7, ss=fitted, want_sums=True)
            assert np.array_equal(sa, sb) and np.array_equal(ma, mb), levels
            assert np.array_equal(sa, _twin_sums(levels, fitted, np.stack([b.sample_demands(i, 1000, 7)[0] for i in range(N)]), functors))
            assert b.simulate_ms() > 0


# ---- the bridge: where the optimal policy is one (s, S) rule, the rule rollout IS the table rollout ------------------------

BRIDGE = ((100.0, 1.0, 10.0, 150), (50.0, 0.0, 5.0, 120), (200.0, 2.0, 20.0, 200))  # K, v, pi, order limit
BRIDGE_MEANS = (8.0, 24.0, 40.0)  # Poisson, one per period


def _bridge_instances(sia):
    from stochastic_inventory_amd.pmf import GetPmf, PoissonDist
    functors, pmfs = [], []
    for K, v, pi, limit in BRIDGE:
        means = BRIDGE_MEANS
        functors.append(sia.BackorderFunctor(fixedOrderingCost=K, variOrderingCost=v, holdingCost=1, penaltyCost=pi, minInventory=-150,
                                             maxInventory=300, maxOrderQuantity=limit, iniInventory=0))
        pmfs.append([np.asarray(t, dtype=np.float64) for t in GetPmf([PoissonDist(m) for m in means], 0.999, 1).getpmf()])
    return functors, pmfs


def test_where_the_policy_is_one_rule_the_rule_rollout_is_the_table_rollout(sia, oracle):
    T = len(BRIDGE_MEANS)
    functors, pmfs = _bridge_instances(sia)
    descs = [f.to_desc(T) for f in functors]
    tables = oracle_tables(oracle, descs, pmfs, workers=3)
    # first, on the oracle's table: in every period the policy on the reachable rows is exactly one (s, S) rule whose order
    # limit never binds -- the twin's one-level fit reproduces every row
    for f, table in zip(functors, tables):
        max_q = int(f.maxOrderQuantity)
        rule = tw.fit(1, T, max_q, table)
        assert np.all(table[:, 2] < max_q)
        for t in range(1, T):
            rows = table[table[:, 0] == t + 1]
            assert len(tw.level_index(rows, max_q)) == 1
            s, S = rule[t]
            assert S == np.round(S) and S - s < max_q
            want = np.where(rows[:, 1] >= s, 0.0, S - rows[:, 1])
            assert np.array_equal(rows[:, 2], want), (f.fixedOrderingCost, t + 1)
            assert [tw.order_quantity(1, t, x, 0.0, rule[t], max_q) for x in rows[:, 1]] == rows[:, 2].tolist()
        assert rule[0, 1] - f.iniInventory == table[0, 2]
    with sia.SdpBatch(descs, pmfs, ragged=True, device=0) as b:
        b.solve()
        for n_paths, seed in ((10000, 20240617), (777, 5)):
            mt, st = b.simulate_sampled(n_paths, seed, want_sums=True)
            m1, s1 = b.simulate_ss_sampled(1, n_paths, seed, want_sums=True)
            m3, s3 = b.simulate_ss_sampled(3, n_paths, seed, want_sums=True)
            assert np.array_equal(s1, st), "the one-level rule along the same paths gives the table policy's path sums"
            assert np.array_equal(m1, mt)
            assert np.array_equal(s3, s1) and np.array_equal(m3, m1), "three repeated bands are the one band"
            _check_means(m1, s1, f"bridge n={n_paths}")
        fit1, fit3 = b.fit_ss(1), b.fit_ss(3)
        assert np.array_equal(fit3, np.tile(fit1, (1, 1, 3)))
        for i in range(len(functors)):
            assert np.array_equal(fit1[i], tw.fit(1, T, int(functors[i].maxOrderQuantity), tables[i]))


def test_means_of_the_fitss_sweep_rules_and_the_gap(sia):
    """10000 paths per instance on the 162 fitss instances: the means against fsum, two calls with identical bits, and the gap
    (simFinalValue - finalValue) / finalValue of ThreeLevelFitsSTest.java:143-145 is small and not negative beyond noise."""
    from stochastic_inventory_amd import workloads
    ws = workloads.fitss_sweep(patterns=(2, 7))
    descs, pmfs = [w.desc() for w in ws], [w.pmf for w in ws]
    with sia.SdpBatch(descs, pmfs, ragged=True, device=0) as b:
        b.solve()
        final, _ = b.initial()
        table_mean = b.simulate_sampled(10000, 99)
        for levels in (1, 2, 3):
            m, s = b.simulate_ss_sampled(levels, 10000, 99, want_sums=True)
            _check_means(m, s, f"fitss {levels} level(s)")
            assert np.array_equal(m, b.simulate_ss_sampled(levels, 10000, 99)), "two calls, the same bits"
            gap = (m - final) / final
            crn = (m - table_mean) / final  # common random numbers: the rule can only cost more than the optimal policy in expectation
            print(f"\nfitss, {levels} level(s): gap median {np.median(gap):.3e} max {gap.max():.3e}; against the table rollout "
                  f"(same paths) median {np.median(crn):.3e} min {crn.min():.3e} max {crn.max():.3e}; kernels {b.simulate_ms():.3f} ms")
            assert np.all(np.isfinite(m)) and np.all(m > 0)


def test_recursion_simulation_batch_and_the_single_recursion_classes(sia):
    T = 4
    functors, pmfs = _ragged_instances(sia, n=6, T=T, seed=5)
    with sia.RecursionBatch(functors, pmfs, device=0, ragged=True) as rb:
        sim = sia.SimulationBatch(None, 1000, rb, seed=7)
        for levels, name in ((1, "simulateSinglesS"), (2, "simulateTwosS"), (3, "simulateThreesS")):
            means = getattr(sim, name)(want_sums=True)
            assert means.shape == (6,) and sim.last_values.shape == (6, 1000)
            want_m, want_s = rb.batch.simulate_ss_sampled(levels, 1000, 7, want_sums=True)
            assert np.array_equal(means, want_m) and np.array_equal(sim.last_values, want_s)
            rule = rb.batch.fit_ss(levels)
            assert np.array_equal(getattr(sim, name)(optsS=rule), want_m)
            ini = [sia.State(1, f.minInventory) for f in functors]
            assert np.array_equal(getattr(sim, name)(iniStates=ini, optsS=rule),
                                  rb.batch.simulate_ss_sampled(levels, 1000, 7, ss=rule, ini_x=[f.minInventory for f in functors]))
        # one Recursion: FitsS on its getOptTable, SimulateFitsS as a batch of one (position 0: instance 0's demand paths)
        f = functors[0]
        rec = sia.Recursion(sia.OptDirection.MIN, pmfs[0], functor=f, device=0)
        table = rec.getOptTable()
        assert np.array_equal(table, rb.getOptTable(0))
        fit = sia.FitsS(int(f.maxOrderQuantity), T)
        one = sia.SimulateFitsS(None, 1000, rec, seed=7)
        for levels, get, name in ((1, fit.getSinglesS, "simulateSinglesS"), (2, fit.getTwosS, "simulateTwosS"), (3, fit.getThreesS, "simulateThreesS")):
            opts = get(table)
            assert np.array_equal(opts, rb.batch.fit_ss(levels)[0])
            got = getattr(one, name)(sia.State(1, f.iniInventory), opts, int(f.maxOrderQuantity))
            want_m, want_s = rb.batch.simulate_ss_sampled(levels, 1000, 7, want_sums=True)
            assert got == want_m[0] and np.array_equal(one.last_values, want_s[0])
        one.close()


def test_refusals_on_the_device(sia):
    T = 4
    functors, pmfs = _ragged_instances(sia, n=3, T=T, seed=5)
    with sia.SdpBatch([f.to_desc(T) for f in functors], pmfs, ragged=True, device=0) as b:
        b.solve()
        for levels in (0, 4):
            with pytest.raises(sia.SdpgpuError) as e:
                b.fit_ss(levels)
            assert e.value.code == 1 and "levels" in e.value.message
            with pytest.raises(sia.SdpgpuError) as e:
                b.simulate_ss_sampled(levels, 100, 1)
            assert e.value.code == 1 and "levels" in e.value.message
        with pytest.raises(ValueError):
            b.simulate_ss_sampled(2, 100, 1, ss=np.zeros((3, T, 2)))  # a one-level rule for two levels
        with pytest.raises(ValueError):
            b.simulate_ss_sampled(1, 100, 1, ss=np.zeros((2, T, 2)))  # a rule for two instances
        with pytest.raises(ValueError):
            b.simulate_ss(3, np.zeros((10, T)), ss=np.zeros((3, T - 1, 6)))
        bad = np.array([f.minInventory for f in functors])
        bad[1] = functors[1].maxInventory + 1
        with pytest.raises(sia.SdpgpuError) as e:
            b.simulate_ss_sampled(1, 100, 1, ini_x=bad)
        assert e.value.code == 1 and "instance 1" in e.value.message
        assert b.simulate_ss_sampled(1, 100, 1).shape == (3,)  # and the batch still works
