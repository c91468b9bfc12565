"""Sampled simulation on a handle, on the GPU (sdpgpu_simulate_sampled / sdpgpu_sample_demands, csrc/sdp_sim_sampled.hpp):
the SAMPLER equals its host twins bit for bit (tests/sampler_twin.py at inst = 0 for the latin hypercube, the RANDOM twin of
tests/test_simulate_sampled_host.py), the FUSED launch equals sdpgpu_simulate on those demands and the CPU oracle's rollout,
the REDUCTION stays inside the bound its documented order gives, and the estimate is right ("Sampled simulation on
a handle")."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
import sampler_twin as tw  # noqa: E402
from test_simulate_sampled_host import (LHS, RANDOM, reduction_chain, spec_demands, tile_demands,  # noqa: E402
                                        twin_sample)

pytestmark = pytest.mark.gpu

SEEDS = (20240607, 7, 11)
NS = (1, 2, 63, 64, 65, 1537, 10000, 100000)
CASES = [cases.f1_small, cases.f1_gapped, cases.f1_unclamped, cases.f2_unclamped, cases.f2_clamped, cases.f2_pipeline,
         cases.f3_tenths, cases.f3_row, cases.f3_testing, cases.f3_min_gamma, cases.f4_overdraft, cases.f5_cash_leadtime,
         cases.f6_survival]
MODES = (("lhs", LHS, 0), ("random", RANDOM, 0), ("random", RANDOM, (1 << 32) + 12345))
_ids = lambda f: f.__name__  # noqa: E731


class Ctx:
    """One solved case: engine, oracle tables, start state, discount weights, V_1(ini)."""

    def __init__(self, sia, oracle, make):
        self.w = w = make()
        f = w.functor
        d = w.desc()
        d.device = 0
        self.eng = sia.SdpEngine(d, w.pmf, w.overhead())
        self.eng.solve()
        self.P = oracle.Problem(w.desc(), w.pmf, w.overhead())
        self.V, self.pol, _ = self.P.solve()
        self.T = w.T
        self.family = w.desc().family
        gamma = getattr(f, "discountFactor", 1.0) if self.family in (3, 4) else 1.0
        self.disc = np.array([math.pow(gamma, t) for t in range(w.T)])
        self.ini = (getattr(f, "iniInventory", 0.0), getattr(f, "iniCash", 0.0), getattr(f, "iniPreQ", 0.0))
        idx = self.eng.state_index(1, *self.ini, w.desc().ini_preq2)
        assert idx >= 0
        self.v1 = float(self.V[0][idx])
        self.draw = [lambda u, tile=tile: tile_demands(tile, u) for tile in w.pmf]


_ctx = {}


@pytest.fixture
def ctx(sia, oracle):
    def get(make):
        if make.__name__ not in _ctx:
            _ctx[make.__name__] = Ctx(sia, oracle, make)
        return _ctx[make.__name__]
    return get


# ---- 1. sampler = twin, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_sample_demands_equal_the_host_twins(sia, n):
    from stochastic_inventory_amd import pmf
    specs = [pmf.NormalDist(12.0, 3.6), pmf.PoissonDist(20.0), pmf.GammaDist(25.0, 0.5), pmf.UniformIntDist(0, 10)]
    for make in (cases.f1_small, cases.f1_gapped, cases.f3_tenths):
        w = make()
        d = w.desc()
        d.device = 0
        with sia.SdpEngine(d, w.pmf, w.overhead()) as eng:  # (needs no solve)
            draw = [lambda u, tile=tile: tile_demands(tile, u) for tile in w.pmf]
            for name, mode, fp in MODES:
                dem, u = eng.sample_demands(n, SEEDS[0], mode=name, first_path=fp)
                want_d, want_u = twin_sample(n, SEEDS[0], mode, fp, draw)
                assert np.array_equal(u, want_u), f"{w.name}: uniforms, {name} from {fp}, n = {n}"
                assert np.array_equal(dem, want_d), f"{w.name}: demands, {name} from {fp}, n = {n}"
                if make is cases.f1_gapped:  # the tile's VALUES, not k_lo + q
                    assert set(np.unique(dem)) <= {2.0, 5.0, 9.0}
            if make is cases.f1_small:  # one spec of each kind (T = 4), then back to the tile
                for t, dist in enumerate(specs):
                    eng.set_sampler(t, dist)
                sdraw = [lambda u, tab=pmf.sample_table(dist): spec_demands(tab, u) for dist in specs]
                for name, mode, fp in MODES:
                    dem, u = eng.sample_demands(n, SEEDS[1], mode=name, first_path=fp)
                    want_d, want_u = twin_sample(n, SEEDS[1], mode, fp, sdraw)
                    assert np.array_equal(u, want_u) and np.array_equal(dem, want_d), f"specs, {name} from {fp}, n = {n}"
                eng.set_sampler(1, None)
                dem, _ = eng.sample_demands(n, SEEDS[1])
                assert np.array_equal(dem[:, 1], twin_sample(n, SEEDS[1], LHS, 0, draw)[0][:, 1])
    if n >= 1000:  # the LHS twin is sampler_twin as it stands, at inst = 0
        w = cases.f1_small()
        d = w.desc()
        d.device = 0
        with sia.SdpEngine(d, w.pmf) as eng:
            dem, u = eng.sample_demands(n, SEEDS[2])
            want_d, want_u = tw.sample(n, SEEDS[2], 0, [tw.tile_table(t) for t in w.pmf])
            assert np.array_equal(u, want_u) and np.array_equal(dem, want_d)
            # (0, a) then (a, b) = (0, a + b)
            a = n // 3
            whole, _ = eng.sample_demands(n, SEEDS[2], mode="random")
            assert np.array_equal(whole[:a], eng.sample_demands(a, SEEDS[2], mode="random")[0])
            assert np.array_equal(whole[a:], eng.sample_demands(n - a, SEEDS[2], mode="random", first_path=a)[0])


# ---- 2. fused = unfused = oracle, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_fused_equals_unfused_equals_oracle(ctx, make):
    c = ctx(make)
    eng = c.eng
    for n in (65, 1537):
        for name, mode, fp in MODES:
            dem, _ = eng.sample_demands(n, SEEDS[0], mode=name, first_path=fp)
            res, sums, flags = eng.simulate_sampled(n, SEEDS[0], *c.ini, mode=name, first_path=fp, discount=c.disc, want_sums=True)
            us, uv = eng.simulate(dem, c.disc, *c.ini)
            uflags = eng.last_sim_flags.copy()
            os_, ov = c.P.simulate(c.V, c.pol, dem, c.disc, *c.ini)
            what = f"{c.w.name}, {name} from {fp}, n = {n}"
            assert np.array_equal(sums, us) and np.array_equal(flags, uflags), "fused vs unfused: " + what
            assert np.array_equal(sums, os_) and np.array_equal(flags, c.P.last_sim_flags), "fused vs oracle: " + what
            # tile samplers draw from the pmf support: every path is valid by construction
            assert res.n_paths == n and res.n_valid == n and (flags & 1).all(), what
            assert res.n_lost == (int(((flags >> 1) & 1).sum()) if c.family == 6 else 0)
            assert res.kernel_ms > 0
            # two calls: the same bits; without the sums buffers: the same result
            res2 = eng.simulate_sampled(n, SEEDS[0], *c.ini, mode=name, first_path=fp, discount=c.disc)
            assert (res2.mean, res2.m2, res2.n_valid, res2.n_lost) == (res.mean, res.m2, res.n_valid, res.n_lost), what
            assert np.float64(res.mean).tobytes() == np.float64(res2.mean).tobytes()
    # discount = None equals an explicit array of ones
    ones = np.ones(c.T)
    r1, s1, f1 = eng.simulate_sampled(1537, SEEDS[1], *c.ini, discount=None, want_sums=True)
    r2, s2, f2 = eng.simulate_sampled(1537, SEEDS[1], *c.ini, discount=ones, want_sums=True)
    assert np.array_equal(s1, s2) and np.array_equal(f1, f2) and (r1.mean, r1.m2) == (r2.mean, r2.m2)
    if c.family == 6:
        assert 0 < r1.n_lost < 1537 and 0.0 < r1.mean < 1.0 and set(np.unique(s1)) <= {0.0, 1.0}


def test_off_grid_start(ctx):
    c = ctx(cases.f3_tenths)
    ini = (0.0, 4.93, 0.0)  # 4.93 is not a multiple of the 0.1 cash quantum
    assert c.eng.state_index(1, *ini) < 0
    for name, mode, fp in MODES:
        dem, _ = c.eng.sample_demands(1000, SEEDS[0], mode=name, first_path=fp)
        res, sums, flags = c.eng.simulate_sampled(1000, SEEDS[0], *ini, mode=name, first_path=fp, discount=c.disc, want_sums=True)
        os_, ov = c.P.simulate(c.V, c.pol, dem, c.disc, *ini)
        assert ov.all() and np.array_equal(sums, os_) and res.n_valid == 1000
        assert np.array_equal(sums, c.eng.simulate(dem, c.disc, *ini)[0])


def test_unit_stride_f1_handle_equals_a_batch_of_one(sia, ctx):
    c = ctx(cases.f1_small)
    with sia.SdpBatch([c.w.desc()], [c.w.pmf], device=0) as b:
        b.solve()
        for n in (64, 1537, 10000):
            dem_b, u_b = b.sample_demands(0, n, SEEDS[0])
            dem_h, u_h = c.eng.sample_demands(n, SEEDS[0])
            assert np.array_equal(u_b, u_h) and np.array_equal(dem_b, dem_h)
            mean_b, sums_b = b.simulate_sampled(n, SEEDS[0], ini_x=[c.ini[0]], want_sums=True)
            res, sums, _ = c.eng.simulate_sampled(n, SEEDS[0], *c.ini, want_sums=True)
            assert np.array_equal(sums_b[0], sums)
            assert abs(mean_b[0] - res.mean) <= 200 * 2.0 ** -53 * abs(res.mean)  # (two orders of one sum)


# ---- 3. reduction -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [cases.f1_small, cases.f3_tenths, cases.f3_min_gamma, cases.f4_overdraft, cases.f6_survival], ids=_ids)
def test_reduction_stays_inside_the_bound_of_its_order(ctx, make):
    """|mean - fsum(sums) / n| <= (L(n) + 1) 2^-53 X, X = fsum(|sum_p|) / n (the + 1 is the division), and
    |m2 - fsum((sum_p - mean)^2)| <= (L(n) + 6) 2^-53 m2 (three roundings per term on either side): both follow from the order
    of additions, whose longest chain is L(n) = 6 + ceil(ceil(n / 64) / 1024) + 10."""
    c = ctx(make)
    u = 2.0 ** -53
    for n in (1, 2, 63, 65, 1537, 10000, 100000):
        for name in ("lhs", "random"):
            res, sums, _ = c.eng.simulate_sampled(n, SEEDS[2], *c.ini, mode=name, discount=c.disc, want_sums=True)
            L = reduction_chain(n)
            want = math.fsum(sums.tolist()) / n
            X = math.fsum(np.abs(sums).tolist()) / n
            print(f"{c.w.name} {name} n={n}: mean {res.mean!r} fsum {want!r} err/X/u {abs(res.mean - want) / (X * u) if X else 0:.2f} of {L + 1}")
            assert abs(res.mean - want) <= (L + 1) * u * X, (c.w.name, name, n, res.mean, want)
            want2 = math.fsum(((sums - res.mean) ** 2).tolist())
            print(f"    m2 {res.m2!r} fsum {want2!r} err/m2/u {abs(res.m2 - want2) / (res.m2 * u) if res.m2 else 0:.2f} of {L + 6}")
            assert abs(res.m2 - want2) <= (L + 6) * u * res.m2, (c.w.name, name, n, res.m2, want2)


# ---- 4. invalid paths -------------------------------------------------------------------------------------------------------
def test_paths_that_leave_the_grid(sia, ctx):
    from stochastic_inventory_amd import pmf
    from stochastic_inventory_amd.simulation import Simulation
    c = ctx(cases.f2_unclamped)
    wide = pmf.NormalDist(4.0, 12.0)  # far wider than the tiles' 0 .. 9: many draws leave the period boxes
    n = 2000
    try:
        for t in range(c.T):
            c.eng.set_sampler(t, wide)
        dem, _ = c.eng.sample_demands(n, SEEDS[0])
        res, sums, flags = c.eng.simulate_sampled(n, SEEDS[0], *c.ini, discount=c.disc, want_sums=True)
        os_, ov = c.P.simulate(c.V, c.pol, dem, c.disc, *c.ini)
        valid = (flags & 1).astype(bool)
        assert 0 < res.n_valid < n and res.n_valid == int(valid.sum()) and res.n_paths == n
        assert math.isnan(res.mean) and math.isnan(res.m2)
        assert np.array_equal(valid, ov) and np.array_equal(sums[valid], os_[ov])
    finally:
        for t in range(c.T):
            c.eng.set_sampler(t, None)
    res = c.eng.simulate_sampled(n, SEEDS[0], *c.ini, discount=c.disc)
    assert res.n_valid == n and math.isfinite(res.mean)
    w = cases.f2_unclamped()
    rec = sia.LeadtimeRecursion(w.pmf, functor=w.functor, device=0)
    sim = Simulation([wide] * w.T, n, rec, seed=SEEDS[0], sampler="device")
    with pytest.raises(RuntimeError, match="left the state grid"):
        sim.simulateSDPGivenSamplNum(sia.LeadtimeState(1, 0.0, 0.0))
    rec.engine.close()


# ---- 5. the estimate is right -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_tile_samplers_estimate_v1_without_bias(ctx, make):
    """|mean - V_1(ini)| <= 4 sd / sqrt(n), sd the sample standard deviation of the path sums (1 - mean against the survival
    probability for f6_survival; discount gamma^t for the cash families).  On fixed seeds a condition, not a measurement: the
    twin's demands through the oracle's rollout gave at most 0.86 standard errors over these 78 runs, and check 2 makes the GPU
    reproduce those means."""
    c = ctx(make)
    for n in (10000, 100000):
        for seed in SEEDS:
            res = c.eng.simulate_sampled(n, seed, *c.ini, discount=c.disc)
            assert res.n_valid == n
            sd = math.sqrt(res.m2 / (n - 1))
            est = 1.0 - res.mean if c.family == 6 else res.mean
            z = (est - c.v1) / (sd / math.sqrt(n)) if sd > 0 else 0.0
            print(f"{c.w.name} n={n} seed={seed}: estimate {est!r} V_1 {c.v1!r} z {z:+.3f} kernel {res.kernel_ms:.3f} ms")
            assert abs(est - c.v1) <= 4.0 * sd / math.sqrt(n), (c.w.name, n, seed, est, c.v1, z)


# ---- 6. mirror --------------------------------------------------------------------------------------------------------------
def _recursion(sia, w):
    f = w.functor
    fam = w.desc().family
    if fam == 1:
        return sia.Recursion(w.direction, w.pmf, functor=f, device=0), 1.0
    if fam == 2:
        return sia.LeadtimeRecursion(w.pmf, functor=f, device=0), 1.0
    if fam in (3, 4):
        g = getattr(f, "discountFactor", 1.0)
        return sia.CashRecursion(w.direction, w.pmf, functor=f, discountFactor=g, device=0), g
    if fam == 5:
        return sia.CashLeadtimeRecursion(w.pmf, functor=f, device=0), 1.0
    raise AssertionError(fam)


def test_simulation_mirror_validates_the_sdp_value_with_the_device_sampler(sia):
    """The two instances of tests/test_gpu_simulation.py's mirror tests, to the 2 % those ask of the host sampler."""
    from stochastic_inventory_amd import pmf as PM
    from stochastic_inventory_amd.simulation import Simulation
    dists = [PM.PoissonDist(m) for m in (6.0, 9.0, 4.0, 7.0)]
    tiles = PM.GetPmf(dists, 0.9999, 1).getpmf()
    f = sia.BackorderFunctor(fixedOrderingCost=30, variOrderingCost=1, holdingCost=1, penaltyCost=8, minInventory=-60,
                             maxInventory=80, maxOrderQuantity=40, iniInventory=0)
    rec = sia.Recursion(sia.OptDirection.MIN, tiles, functor=f)
    ini = sia.State(1, 0.0)
    v = rec.getExpectedValue(ini)
    sim = Simulation(dists, 20000, rec, seed=7, sampler="device")
    mean = sim.simulateSDPGivenSamplNum(ini)
    assert abs(mean - v) / v < 0.02 and sim.last_values.shape == (20000,) and sim.last_result.n_valid == 20000
    assert mean == sim.simulateSDPGivenSamplNum(ini)  # seeded: the same bits
    tile_sim = Simulation(None, 20000, rec, seed=7, sampler="device")  # distributions=None: the recursion's own tiles
    assert abs(tile_sim.simulateSDPGivenSamplNum(ini) - v) / v < 0.02
    host = Simulation(dists, 2000, rec, seed=7)  # the default is the host sampler, untouched
    assert host.sampler == "host" and abs(host.simulateSDPGivenSamplNum(ini) - v) / v < 0.05

    dists = [PM.PoissonDist(5.0)] * 3
    tiles = PM.GetPmf(dists, 0.999, 1).getpmf()
    f = sia.CashFunctor(price=5, fixOrderCost=4, variCost=1, salvageValue=0.5, maxOrderQuantity=20,
                        minInventoryState=0, maxInventoryState=40, minCashState=-20, maxCashState=200,
                        cashRoundMult=1.0, cashRoundDiv=1.0, cashRoundIntDiv=True, cashFormula=1, iniCash=12)
    rec = sia.CashRecursion(sia.OptDirection.MAX, tiles, functor=f, discountFactor=1.0)
    ini = sia.CashState(1, 0.0, 12.0)
    final_cash = rec.getExpectedValue(ini) + 12.0
    sim = Simulation(dists, 20000, rec, discountFactor=1.0, seed=11, sampler="device")
    assert abs(sim.simulateSDPGivenSamplNum(ini) - final_cash) / final_cash < 0.02


@pytest.mark.parametrize("make", [cases.f1_small, cases.f1_gapped, cases.f2_clamped, cases.f3_testing, cases.f3_tenths,
                                  cases.f4_overdraft, cases.f5_cash_leadtime], ids=_ids)
def test_error_confidence_runs_on_the_random_stream(sia, ctx, make):
    """simulateSDPwithErrorConfidence(ini, 0.01, 0.95, batch=1000) under tile samplers: radius < 0.01 center, and
    |center - V_1(ini)| <= 4 radius / z.  On the CPU (the RANDOM twin through the oracle's rollout) the 21 runs stop after 2000 to
    11000 paths, every path valid, largest deviation 1.99 standard errors."""
    from scipy.stats import norm
    from stochastic_inventory_amd.simulation import Simulation
    c = ctx(make)
    z = float(norm.ppf(0.975))
    rec, gamma = _recursion(sia, c.w)
    try:
        ini = rec._initial_state()
        assert rec.getExpectedValue(ini) == c.v1
        for seed in SEEDS:
            sim = Simulation(None, 1000, rec, discountFactor=gamma, seed=seed, sampler="device")
            center, radius = sim.simulateSDPwithErrorConfidence(ini, 0.01, 0.95, batch=1000)
            n = len(sim.last_values)
            print(f"{c.w.name} seed={seed}: {n} paths, center {center!r} radius {radius!r} V_1 {c.v1!r} "
                  f"deviation {(center - c.v1) / (radius / z):+.3f} standard errors")
            assert n >= 1000 and n % 1000 == 0
            assert radius < 0.01 * center, (c.w.name, seed, center, radius)
            assert abs(center - c.v1) <= 4.0 * radius / z, (c.w.name, seed, center, c.v1, radius)
            # the merged moments are those of all the paths drawn
            assert abs(center - sim.last_values.mean()) <= 1e-12 * abs(center)
            assert abs(radius - z * sim.last_values.std(ddof=1) / math.sqrt(n)) <= 1e-10 * radius
            # rounds continue ONE stream: the first two rounds are one call of 2000 paths
            if n >= 2000:
                _, sums, _ = rec.engine.simulate_sampled(2000, seed, *c.ini, mode="random", discount=c.disc, want_sums=True)
                assert np.array_equal(sums, sim.last_values[:2000])
    finally:
        rec.engine.close()


def test_risk_simulation_with_the_device_sampler(sia):
    w = cases.f6_survival()
    f = w.functor
    rec = sia.RiskRecursion(w.pmf, functor=f, device=0)
    ini = sia.RiskState(1, f.iniInventory, f.iniCash, False)
    n = 5000
    dev = sia.RiskSimulation(None, n, rec, seed=SEEDS[0], sampler="device")
    got = dev.simulateLostSale(ini)
    dem, _ = rec.engine.sample_demands(n, SEEDS[0])
    host = sia.RiskSimulation([sia.PoissonDist(m) for m in (4, 6, 3, 5)], n, rec)
    want = host.simulateLostSaleOnDemands(ini, dem)
    assert got == want and np.array_equal(dev.last_flags, host.last_flags)
    assert abs(got[0] - rec.getSurvProb(ini)) < 0.05 and 0.0 < got[1] < 1.0
    rec.engine.close()
