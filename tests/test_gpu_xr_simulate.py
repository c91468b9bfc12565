"""(x, R) rollout on the GPU (sdpgpu_xr_simulate, csrc/sdp_xr_sim.hpp; DESIGN 4 "(x, R) rollout").  Table rule: the path sums
equal the oracle's rollout (oracle.Problem.simulate) bit for bit on the call's own demands, which equal the sampler twins; the
same demands GIVEN back reproduce the sums; the start may lie off the grid.  Level rule: the path sums equal the host twin
(tests/xr_sim_twin.py) bit for bit, R rules in one call equal R calls, RANDOM calls continue one stream, nothing needs a solve,
and the Python mirror's host loop is a third route to the same sums.  The reduction stays inside the bound its documented order
gives; the estimates bracket V_1.  Cases, sizes and rules: tests/test_xr_simulate_host.py, whose coverage condition shows that
the rules show every event of the definition."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
import xr_sim_twin as xt  # noqa: E402
from test_simulate_sampled_host import RANDOM, LHS, reduction_chain, tile_demands, twin_sample  # noqa: E402
from test_xr_simulate_host import CASES, NS, RULES, SEED, discount_of, sixteen_rules, start_of  # noqa: E402

pytestmark = pytest.mark.gpu

_ids = lambda f: f.__name__  # noqa: E731
_solved, _fresh, _oracle = {}, {}, {}


@pytest.fixture(autouse=True)
def the_feature(sia):
    """Every test here is about the (x, R) rollout: without its two symbols each fails at once, the twin's own tests included."""
    lib = sia._abi.load()
    for name in ("sdpgpu_xr_simulate", "sdpgpu_xr_opt_levels"):
        assert name in sia._abi.EXPORTS and hasattr(lib, name), f"{name} is missing"


@pytest.fixture
def solved(sia):
    """(workload, engine) of a case, the engine solved once."""
    def get(make):
        if make.__name__ not in _solved:
            w = make()
            d = w.desc()
            d.device = 0
            eng = sia.SdpEngine(d, w.pmf, w.overhead())
            eng.solve()
            _solved[make.__name__] = (w, eng)
        return _solved[make.__name__]
    return get


@pytest.fixture
def fresh(sia):
    """(workload, engine) of a case, the engine NEVER solved."""
    def get(make):
        if make.__name__ not in _fresh:
            w = make()
            d = w.desc()
            d.device = 0
            _fresh[make.__name__] = (w, sia.SdpEngine(d, w.pmf, w.overhead()))
        return _fresh[make.__name__]
    return get


def oracle_tables(oracle, make):
    """The oracle's problem and its own tables of a case: computed once, shared, never changed."""
    if make.__name__ not in _oracle:
        w = make()
        prob = oracle.Problem(w.desc(), w.pmf, w.overhead())
        V, pol, _ = prob.solve()
        _oracle[make.__name__] = (prob, V, pol)
    return _oracle[make.__name__]


def twin_demands(w, n, mode=LHS, first_path=0):
    return twin_sample(n, SEED, mode, first_path, [lambda u, tile=tile: tile_demands(tile, u) for tile in w.pmf])[0]


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def check_reduction(res, sums, what):
    """n_paths, n_valid, n_lost, and mean / m2 inside (L(n) + 1) u fsum|s| / n and (L(n) + 6) u m2."""
    n = len(sums)
    assert res.n_paths == n and res.n_valid == n and res.n_lost == 0 and res.kernel_ms > 0, what
    u, L = 2.0 ** -53, reduction_chain(n)
    ref = math.fsum(sums.tolist()) / n
    X = math.fsum(np.abs(sums).tolist()) / n
    print(f"{what}: mean {res.mean!r} fsum {ref!r} err/X/u {abs(res.mean - ref) / (X * u) if X else 0:.2f} of {L + 1}")
    assert abs(res.mean - ref) <= (L + 1) * u * X, ("mean", what, res.mean, ref)
    ref2 = math.fsum(((sums - res.mean) ** 2).tolist())
    print(f"    m2 {res.m2!r} fsum {ref2!r} err/m2/u {abs(res.m2 - ref2) / (res.m2 * u) if res.m2 else 0:.2f} of {L + 6}")
    assert abs(res.m2 - ref2) <= (L + 6) * u * res.m2, ("m2", what, res.m2, ref2)


# ---- 1. the table rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_table_rule_equals_the_oracle_on_its_own_demands(solved, oracle, make):
    w, eng = solved(make)
    prob, V, pol = oracle_tables(oracle, make)
    disc = discount_of(w)
    x, R = start_of(w)
    for n in NS:
        for mode, name in ((LHS, "lhs"), (RANDOM, "random")):
            res, sums, dem = eng.xr_simulate(n, SEED, x, R, mode=name, discount=disc, want_sums=True, want_demands=True)
            what = f"{w.name} table rule, {name}, n = {n}"
            assert len(res) == 1 and sums.shape == (1, n) and dem.shape == (n, w.T)
            assert np.array_equal(dem, twin_demands(w, n, mode)), "draws: " + what
            want, valid = prob.simulate(V, pol, dem, disc, x, R)
            assert valid.all() and sums[0].tobytes() == want.tobytes(), "path sums: " + what
            check_reduction(res[0], sums[0], what)
            # the same demands GIVEN back: the same sums, mean and m2; a repeated call gives identical bits
            res2, sums2, dem2 = eng.xr_simulate(demand=dem, ini_x=x, ini_r=R, discount=disc, want_sums=True, want_demands=True)
            assert sums2.tobytes() == sums.tobytes() and dem2.tobytes() == dem.tobytes(), "given: " + what
            assert same_bits(res2[0].mean, res[0].mean) and same_bits(res2[0].m2, res[0].m2), "given: " + what
            res3 = eng.xr_simulate(n, SEED, x, R, mode=name, discount=disc)
            assert same_bits(res3[0].mean, res[0].mean) and same_bits(res3[0].m2, res[0].m2), "repeated: " + what


@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_table_rule_from_an_off_grid_start(solved, oracle, make):
    w, eng = solved(make)
    prob, V, pol = oracle_tables(oracle, make)
    disc = discount_of(w)
    # (0.5, 7.25): the inventory is off the grid, and stays off it unless period 1 sells out -- the oracle ends such a path after
    # period 1's term (the reference would re-enter its recursion there), and so does the rollout: the same sums, the same count
    # of valid paths, mean and m2 NaN.  (0, 7.25): only the cash is off the grid; the quantiser brings every path back.
    for (x, R), stays in (((0.5, 7.25), False), ((0.0, 7.25), True)):
        assert eng.state_index(1, x, R) < 0
        for n in (65, 257):
            res, sums, dem = eng.xr_simulate(n, SEED, x, R, discount=disc, want_sums=True, want_demands=True)
            assert np.array_equal(dem, twin_demands(w, n))
            want, valid = prob.simulate(V, pol, dem, disc, x, R)
            what = f"{w.name} table rule, start ({x}, {R}), n = {n}"
            assert sums[0].tobytes() == want.tobytes(), what
            assert res[0].n_paths == n and res[0].n_valid == int(valid.sum()) and res[0].n_lost == 0, what
            assert bool(valid.all()) == stays, what
            if stays:
                check_reduction(res[0], sums[0], what)
            else:
                assert 0 < res[0].n_valid < n and math.isnan(res[0].mean) and math.isnan(res[0].m2), what


def test_table_rule_needs_a_solve_and_is_one_rule(sia, fresh, solved):
    w, eng = fresh(cases.f3_xr)
    with pytest.raises(sia.SdpgpuError) as e:
        eng.xr_simulate(64, SEED, 0.0, 30.0)
    assert e.value.code == 2 and "nothing has been solved" in str(e.value)
    # the four older entry points keep refusing a solved (x, R) handle
    w, eng = solved(cases.f3_xr)
    for call in (lambda: eng.simulate(np.zeros((4, w.T)), np.ones(w.T), 0.0, 30.0), lambda: eng.simulate_sampled(64, SEED, 0.0, 30.0),
                 lambda: eng.sample_demands(64, SEED)):
        with pytest.raises(sia.SdpgpuError) as e:
            call()
        assert e.value.code == 4 and "not built for the (x, R) state" in str(e.value)


# ---- 2. the level rule -----------------------------------------------------------------------------------------------------
def level_call(w, eng, n, levels, ini=None, mode="lhs", first_path=0):
    x, R = start_of(w) if ini is None else ini
    return eng.xr_simulate(n, SEED, x, R, levels, vari_cost=w.functor.variCost, mode=mode, first_path=first_path, discount=discount_of(w),
                           want_sums=True, want_demands=True)


def level_twin(w, dem, levels, ini=None):
    x, R = start_of(w) if ini is None else ini
    return xt.simulate(w.functor, w.T, dem, discount_of(w), x, R, levels, w.functor.variCost)["sum"]


@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_level_rule_equals_the_twin_without_a_solve(fresh, make):
    w, eng = fresh(make)
    levels = RULES[w.name]
    for n in NS:
        res, sums, dem = level_call(w, eng, n, levels)
        assert len(res) == 3 and sums.shape == (3, n)
        assert np.array_equal(dem, twin_demands(w, n)), (w.name, n)
        want = level_twin(w, dem, levels)
        for r in range(3):
            what = f"{w.name} level rule {r} of three, n = {n}"
            assert sums[r].tobytes() == want[r].tobytes(), "path sums: " + what
            check_reduction(res[r], sums[r], what)
            assert res[r].kernel_ms == res[0].kernel_ms  # (of the whole call)
            # the R-rule call equals R one-rule calls: sums, mean, m2 -- on the same demands
            one, s1, d1 = level_call(w, eng, n, levels[r])
            assert s1[0].tobytes() == sums[r].tobytes() and d1.tobytes() == dem.tobytes(), what
            assert same_bits(one[0].mean, res[r].mean) and same_bits(one[0].m2, res[r].m2), what
        # GIVEN the same demands: the same sums; a repeated call gives identical bits
        res2, sums2 = eng.xr_simulate(demand=dem, ini_x=start_of(w)[0], ini_r=start_of(w)[1], levels=levels, vari_cost=w.functor.variCost,
                                      discount=discount_of(w), want_sums=True)
        assert sums2.tobytes() == sums.tobytes() and all(same_bits(a.mean, b.mean) and same_bits(a.m2, b.m2) for a, b in zip(res, res2))
        res3 = eng.xr_simulate(n, SEED, *start_of(w), levels, vari_cost=w.functor.variCost, discount=discount_of(w))
        assert all(same_bits(a.mean, b.mean) and same_bits(a.m2, b.m2) for a, b in zip(res, res3))
    assert sums[0].tobytes() != sums[1].tobytes() and sums[1].tobytes() != sums[2].tobytes()  # (the rules differ)


def test_level_rule_from_another_start_and_sixteen_rules(fresh):
    w, eng = fresh(cases.f3_xr)
    n = 257
    res, sums, dem = level_call(w, eng, n, RULES["f3_xr"], ini=(3.0, 9.0))
    want = level_twin(w, dem, RULES["f3_xr"], ini=(3.0, 9.0))
    assert sums.tobytes() == want.tobytes()
    for make in CASES:
        w, eng = fresh(make)
        rules = sixteen_rules()
        assert rules.shape == (16, 3)
        res, sums, dem = level_call(w, eng, n, rules)
        assert np.array_equal(dem, twin_demands(w, n))
        want = level_twin(w, dem, rules)
        assert sums.shape == (16, n) and sums.tobytes() == want.tobytes(), w.name
        for r in (0, 7, 15):
            check_reduction(res[r], sums[r], f"{w.name} rule {r} of sixteen")
            one, s1, _ = level_call(w, eng, n, rules[r])
            assert s1[0].tobytes() == sums[r].tobytes() and same_bits(one[0].mean, res[r].mean) and same_bits(one[0].m2, res[r].m2)


@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_random_calls_continue_one_stream(fresh, make):
    w, eng = fresh(make)
    levels = RULES[w.name]
    res, whole, dem = level_call(w, eng, 1000, levels, mode="random")
    assert np.array_equal(dem, twin_demands(w, 1000, RANDOM))
    assert whole.tobytes() == level_twin(w, dem, levels).tobytes()
    _, head, d0 = level_call(w, eng, 300, levels, mode="random", first_path=0)
    _, tail, d1 = level_call(w, eng, 700, levels, mode="random", first_path=300)
    assert np.concatenate([head, tail], axis=1).tobytes() == whole.tobytes()
    assert np.concatenate([d0, d1]).tobytes() == dem.tobytes()
    assert whole.tobytes() != level_call(w, eng, 1000, levels)[1].tobytes()  # another stream than the latin hypercube's


@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_the_mirrors_host_loop_is_a_third_route(sia, make):
    w = make()
    f = w.functor
    n = 257
    rec = sia.CashRecursionXR(w.direction, w.pmf, functor=f, discountFactor=f.discountFactor, device=0)
    try:
        args = (f.discountFactor, f.fixOrderCost, f.price, f.variCost, f.holdingCost, f.salvageValue)
        dev = sia.CashSimulationXR(None, n, rec, *args, seed=SEED, sampler="device")  # None: the recursion's own tiles
        host = sia.CashSimulationXR(None, n, rec, *args, seed=SEED, sampler="host")
        x, R = start_of(w)
        ini = sia.CashStateXR(1, x, R, f.variCost)
        levels = RULES[w.name]
        values = dev.simulateAStar(levels, ini)  # (no solve yet: the a* rollout needs none)
        assert values.shape == (3,) and dev.last_values.shape == (3, n)
        dem = dev.last_demands
        assert np.array_equal(dem, twin_demands(w, n))
        assert dev.last_values.tobytes() == host.simulateOnDemands(ini, dem, levels).tobytes(), w.name
        assert dev.last_values.tobytes() == level_twin(w, dem, levels).tobytes()
        assert [v for v in values] == [r.mean + R for r in dev.last_results]
        one = dev.simulateAStar(levels[1], ini)
        assert isinstance(one, float) and one == values[1] and dev.last_values.tobytes() == host.simulateOnDemands(ini, dem, levels[1]).tobytes()
        # the table policy: the device's sums are the host loop's through getAction on a few paths
        v = dev.simulateSDPGivenSamplNum(ini)
        assert v == dev.last_result.mean + R and dev.last_values.shape == (n,)
        assert dev.last_values[:12].tobytes() == host.simulateOnDemands(ini, dev.last_demands[:12]).tobytes()
    finally:
        rec.engine.close()


# ---- 3. the estimates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_table_rule_mean_is_within_four_standard_errors_of_v1(solved, make):
    w, eng = solved(make)
    x, R = start_of(w)
    v1 = float(eng.values(1)[eng.state_index(1, x, R)])
    n = 20000
    for seed in (11, 12, 13):
        res = eng.xr_simulate(n, seed, x, R, mode="random", discount=discount_of(w))[0]
        se = math.sqrt(res.m2 / (n - 1)) / math.sqrt(n)
        print(f"{w.name} seed {seed}: mean {res.mean!r} V1 {v1!r} se {se!r}: {(res.mean - v1) / se:.2f} standard errors")
        assert res.n_valid == n and abs(res.mean - v1) <= 4 * se, (w.name, seed, res.mean, v1, se)


@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_error_confidence_stops_by_its_rule_and_brackets_v1(sia, make):
    w = make()
    f = w.functor
    rec = sia.CashRecursionXR(w.direction, w.pmf, functor=f, discountFactor=f.discountFactor, device=0)
    try:
        sim = sia.CashSimulationXR(None, 1000, rec, f.discountFactor, f.fixOrderCost, f.price, f.variCost, f.holdingCost, f.salvageValue,
                                   seed=SEED, sampler="device")
        x, R = start_of(w)
        ini = sia.CashStateXR(1, x, R, f.variCost)
        error = 0.02
        centre, radius = sim.simulateSDPwithErrorConfidence(ini, error, 0.95)
        n = len(sim.last_values)
        v1 = rec.getExpectedValue(ini)
        print(f"{w.name}: {n} paths, centre {centre!r} radius {radius!r}, V1 + iniR {v1 + R!r}")
        assert n >= 1000 and n % 1000 == 0 and n < 1000000
        assert radius < (centre - R) * error  # the stopping rule tests the tally's centre, before iniR is added (:123, :142)
        if n > 1000:  # ... and did not hold one round earlier
            head = sim.last_values[:n - 1000]
            r0 = 1.959963984540054 * float(head.std(ddof=1)) / math.sqrt(len(head))
            assert r0 >= float(head.mean()) * error * (1 - 1e-12)
        assert abs(centre - (v1 + R)) <= radius, (w.name, centre, radius, v1 + R)
    finally:
        rec.engine.close()


# ---- 4. the driver, small ------------------------------------------------------------------------------------------------------
def test_the_driver_on_a_small_grid(sia):
    """cash.singleItem.CashConstraintXR.main with maxInventoryState 60 and maxCashState 300: solve, a*, both rollouts."""
    from stochastic_inventory_amd.pmf import GammaDist
    w = cases.xr_main_instance()
    f = w.functor
    f.maxInventoryState, f.maxCashState = 60, 300
    rec = sia.CashRecursionXR(w.direction, w.pmf, functor=f, discountFactor=f.discountFactor, device=0)
    try:
        ini = sia.CashStateXR(1, f.iniInventory, f.iniCash, f.variCost)
        final = f.iniCash + rec.getExpectedValue(ini)
        dists = [GammaDist(8, 2) for _ in range(w.T)]
        optY = sia.RecursionG(w.pmf, dists, f.price, f.variCost, f.depositeRate, f.salvageValue).getOptY()
        assert optY.shape == (w.T,) and optY.tolist() == xt.RecursionG(w.pmf, f.price, f.variCost, f.depositeRate, f.salvageValue).getOptY()
        n = 10000
        sim = sia.CashSimulationXR(None, n, rec, f.discountFactor, f.fixOrderCost, f.price, f.variCost, f.holdingCost, f.salvageValue,
                                   seed=SEED)
        table = sim.simulateSDPGivenSamplNum(ini)
        res = sim.last_result
        astar = sim.simulateAStar(optY, ini)
        print(f"final {final!r} simulated {table!r} a* {optY.tolist()} -> {astar!r}")
        assert math.isfinite(final) and math.isfinite(table) and math.isfinite(astar)
        se = math.sqrt(res.m2 / (n - 1)) / math.sqrt(n)
        assert res.n_valid == n and abs(table - final) <= 4 * se, (table, final, se)
    finally:
        rec.engine.close()
