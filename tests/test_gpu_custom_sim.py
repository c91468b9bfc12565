"""User-functor rollouts on the GPU (sdpgpu_custom_simulate, sdpgpu_custom_simulate_sampled, sdpgpu_custom_rule_simulate;
csrc/sdp_custom_src.hpp: kCustomSim; DESIGN 4 "User-functor rollouts"): the table rollout equals the oracle running the same text
compiled for the host, byte for byte; a built-in family restated as text rolls out with the built-in handle's bits; a path that
leaves the grid ends with its valid bit clear; the overdraft drivers' rules equal the host twin (tests/custom_rule_twin.py); the
mirror's Simulation / CashSimulation take the device route over a CustomFunctor recursion.

Handles are made once per module (each costs two hipRTC compiles); n in {1, 64, 65, 257}: one lane, a full wave, a wave boundary,
a second workgroup."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
import custom_overdraft_sources as co  # noqa: E402
import custom_rule_twin as ct  # noqa: E402
import custom_sources as cs  # noqa: E402
from test_custom_functor import _params_backorder  # noqa: E402
from test_gpu_custom_functor import _overdraft_limit_case  # noqa: E402
from test_gpu_staff_simulate import check_against_twin  # noqa: E402
from test_simulate_sampled_host import LHS, RANDOM, tile_demands, twin_sample  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20240611
NS = (1, 64, 65, 257)
MODES = (("lhs", LHS), ("random", RANDOM))


class Case:
    """One solved user-functor handle with the oracle's tables of the same text compiled for the host."""

    def __init__(self, sia, oracle, desc, pmf, text, params, level=None):
        self.desc, self.pmf, self.text, self.params, self.T = desc, pmf, text, params, len(pmf)
        self.eng = sia.SdpEngine(desc, pmf, custom_source=text, custom_params=params)
        self.eng.solve()
        self.P = oracle.Problem(desc, pmf)
        self.functor = oracle.custom_functor(text, params, level=level)
        with self.functor:
            self.V, self.pol, _ = self.P.solve(nthreads=4)
        self.draw = [lambda u, tile=tile: tile_demands(tile, u) for tile in pmf]
        self.disc = np.array([math.pow(desc.discount_factor, t) for t in range(self.T)])

    def oracle_sim(self, dem, ini):
        with self.functor:
            return self.P.simulate(self.V, self.pol, dem, self.disc, *ini)


_cases = {}


@pytest.fixture(scope="module")
def table_case(sia, oracle):
    def get(name):
        if name not in _cases:
            if name.startswith("limit"):
                shape, params, pmf = _overdraft_limit_case(sia)
                desc = shape.to_desc(len(pmf), sia.OptDirection.MAX)
                desc.discount_factor = 0.98
                text = cs.OVERDRAFT_LIMIT_FUSED if name.endswith("fused") else cs.OVERDRAFT_LIMIT
            else:
                desc, pmf, params = co.desc(sia), co.pmf(), co.PARAMS
                text = co.OVERDRAFT_TESTING_FUSED if name.endswith("fused") else co.OVERDRAFT_TESTING
            _cases[name] = Case(sia, oracle, desc, pmf, text, params)
        return _cases[name]
    yield get
    for c in _cases.values():
        c.eng.close()
    _cases.clear()


TABLE_CASES = ("limit", "limit-fused", "testing", "testing-fused")


# ---- 1. the table rollout against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLE_CASES)
def test_table_rollout_equals_the_oracle(table_case, name):
    c = table_case(name)
    for ini in ((0.0, 10.0, 0.0), (0.5, 10.37, 0.0)):  # the grid start; an off-grid start (x + 0.5, cash + 0.37)
        for n in NS:
            for mode, m in MODES:
                res, sums, flags, dem = c.eng.custom_simulate_sampled(n, SEED, *ini, mode=mode, discount=c.disc, want_sums=True,
                                                                      want_demands=True)
                want_dem, _ = twin_sample(n, SEED, m, 0, c.draw)
                osum, ovalid = c.oracle_sim(dem, ini)
                what = f"{name} n={n} {mode} ini={ini}"
                check_against_twin(c.eng, res, sums, (flags & 1).astype(bool), dem, {"sum": osum, "valid": ovalid, "demand": want_dem}, what)
                # the given-demand call on the demands the sampled call returned: the same bits
                gsum, gvalid = c.eng.custom_simulate(dem, c.disc, *ini)
                assert gsum.tobytes() == sums.tobytes() and np.array_equal(gvalid, ovalid), what
        # given demands of the caller's own: every path a different corner of the support
        lo, hi = c.pmf[0][0][0], c.pmf[0][-1][0]
        given = np.array([[lo, hi, lo, hi], [hi, hi, hi, hi], [lo, lo, lo, lo], [hi, lo, hi, lo], [lo + 1, hi - 1, lo + 2, hi]][:5])[:, :c.T]
        gsum, gvalid = c.eng.custom_simulate(given, c.disc, *ini)
        osum, ovalid = c.oracle_sim(given, ini)
        assert gsum.tobytes() == osum.tobytes() and np.array_equal(gvalid, ovalid), (name, ini)


def test_draws_are_the_built_in_samplers(sia, table_case):
    """out_demand equals the sampler twin under both modes, a RANDOM stream continues across calls, and a built-in handle with
    the same tiles returns the same demands from sample_demands."""
    c = table_case("testing")
    builtin = sia.SdpEngine(co.shape(sia).to_desc(co.T, sia.OptDirection.MAX), co.pmf())
    for n in NS:
        for mode, m in MODES:
            _, dem = c.eng.custom_simulate_sampled(n, SEED, *co.INI, mode=mode, want_demands=True)
            assert np.array_equal(dem, twin_sample(n, SEED, m, 0, c.draw)[0])
            assert np.array_equal(dem, builtin.sample_demands(n, SEED, mode=mode)[0])
    _, tail = c.eng.custom_simulate_sampled(40, SEED, *co.INI, mode="random", first_path=25, want_demands=True)
    _, whole = c.eng.custom_simulate_sampled(65, SEED, *co.INI, mode="random", want_demands=True)
    assert np.array_equal(tail, whole[25:])
    builtin.close()


# ---- 2. the same model as text and as a built-in family: the same bits ------------------------------------------------------
@pytest.mark.parametrize("which", ["backorder-f1_small", "leadtime-f2_clamped", "level-f1_small"])
def test_builtin_family_as_text_rolls_out_with_the_builtin_bits(sia, which):
    from stochastic_inventory_amd import workloads
    make, text = {"backorder-f1_small": (cases.f1_small, cs.BACKORDER), "leadtime-f2_clamped": (cases.f2_clamped, cs.LEADTIME),
                  "level-f1_small": (cases.f1_small, workloads.CLSP_LAMBDAS_LEVEL_HIP)}[which]
    w = make()
    f = w.functor
    ini = (float(f.iniInventory), 0.0, float(getattr(f, "iniPreQ", 0.0)))
    with sia.SdpEngine(w.desc(), w.pmf, custom_source=text, custom_params=_params_backorder(f)) as eng, \
            sia.SdpEngine(w.desc(), w.pmf) as builtin:
        eng.solve()
        builtin.solve()
        for n in NS:
            for mode, _ in MODES:
                res, sums, flags = eng.custom_simulate_sampled(n, SEED, *ini, mode=mode, want_sums=True)
                bres, bsums, bflags = builtin.simulate_sampled(n, SEED, *ini, mode=mode, want_sums=True)
                assert sums.tobytes() == bsums.tobytes() and np.array_equal(flags, bflags), (which, n, mode)
                assert (res.n_paths, res.n_valid, res.n_lost) == (bres.n_paths, bres.n_valid, bres.n_lost)
                assert np.float64(res.mean).tobytes() == np.float64(bres.mean).tobytes(), (which, n, mode)
                assert np.float64(res.m2).tobytes() == np.float64(bres.m2).tobytes(), (which, n, mode)


# ---- 3. leaving the grid -------------------------------------------------------------------------------------------------------
def test_a_path_that_leaves_the_grid_ends_with_its_valid_bit_clear(sia):
    from stochastic_inventory_amd import workloads
    w = cases.f1_unclamped()
    f = w.functor
    with sia.SdpEngine(w.desc(), w.pmf, custom_source=workloads.CLSP_LAMBDAS_LEVEL_HIP, custom_params=_params_backorder(f)) as eng, \
            sia.SdpEngine(w.desc(), w.pmf) as builtin:
        eng.solve()
        builtin.solve()
        T = w.T
        hi = float(w.pmf[0][-1][0])
        # inside the support; beyond it in period 1, 2 and (no successor is tested there) T; far beyond
        dem = np.array([[2.0] * T, [hi + 3] + [2.0] * (T - 1), [2.0, hi + 5] + [2.0] * (T - 2), [2.0] * (T - 1) + [hi + 9], [0.0] * T,
                        [1e6] * T])
        disc = np.ones(T)
        sums, valid = eng.custom_simulate(dem, disc, float(f.iniInventory))
        bsums, bvalid = builtin.simulate(dem, disc, float(f.iniInventory))
        assert np.array_equal(valid, bvalid) and not valid.all() and valid.any()
        assert sums[valid].tobytes() == bsums[valid].tobytes()
        # sampled from a spec whose demands leave the support: invalid paths, NaN moments, status OK
        eng.set_sampler(0, sia.PoissonDist(30.0))
        res, sums, flags = eng.custom_simulate_sampled(257, SEED, float(f.iniInventory), want_sums=True)
        assert res.n_valid < res.n_paths == 257 and res.n_valid == int((flags & 1).sum())
        assert math.isnan(res.mean) and math.isnan(res.m2)


# ---- 4. the overdraft drivers' rules -------------------------------------------------------------------------------------------
class RuleCtx:
    def __init__(self, sia):
        self.eng = sia.SdpEngine(co.desc(sia), co.pmf(), custom_source=co.OVERDRAFT_TESTING, custom_params=co.PARAMS)  # NOT solved
        self.fused = sia.SdpEngine(co.desc(sia), co.pmf(), custom_source=co.OVERDRAFT_TESTING_FUSED, custom_params=co.PARAMS)
        self.lam = ct.Lambdas(co.OVERDRAFT_TESTING, co.PARAMS, co.T)
        self.draw = [lambda u, tile=tile: tile_demands(tile, u) for tile in co.pmf()]
        self.disc = np.array([math.pow(0.95, t) for t in range(co.T)])
        self._twin = {}

    def twin(self, which, n, mode=LHS, first_path=0, ini=co.INI):
        key = (which, n, mode, first_path, ini)
        if key not in self._twin:
            dem, _ = twin_sample(n, SEED, mode, first_path, self.draw)
            fm, rows = co.rules(which)
            s = co.SCALARS
            out = ct.simulate(self.lam, dem, self.disc, ini[0], ini[1], fm, rows, s["min_cash_required"], s["max_q"], s["fix_order_cost"],
                              s["vari_cost"], cash_box=(-40.0, 120.0))
            self._twin[key] = (dem, out)
        return self._twin[key]

    def run(self, which, n, mode="lhs", first_path=0, ini=co.INI, eng=None):
        fm, rows = co.rules(which)
        return (self.eng if eng is None else eng).custom_rule_simulate(n, SEED, ini[0], ini[1], fm, rows, mode=mode, first_path=first_path, discount=self.disc,
                                                      want_sums=True, want_demands=True, **co.SCALARS)


@pytest.fixture(scope="module")
def rule_ctx(sia):
    c = RuleCtx(sia)
    yield c
    c.eng.close()
    c.fused.close()


def _check_rules(c, which, n, mode, m, ini=co.INI, eng=None):
    res, sums, dem = c.run(which, n, mode=mode, ini=ini, eng=eng)
    want_dem, want = c.twin(which, n, m, 0, ini)
    for r in range(len(which)):
        check_against_twin(c.eng, res[r], sums[r], np.ones(n, bool), dem, {"sum": want["sum"][r], "valid": np.ones(n, bool), "demand": want_dem},
                           f"rules {which} r={r} n={n} {mode} ini={ini}")
    return res, sums


@pytest.mark.parametrize("which", [(0,), (1,), (2,), (0, 1, 2, 3, 4)], ids=["SS", "SCS", "SCS1S2", "mixed"])
def test_rules_equal_the_twin(rule_ctx, which):
    for n in NS:
        for mode, m in MODES:
            _check_rules(rule_ctx, which, n, mode, m)
    if len(which) == 5:  # parity was reached on branches that were taken
        assert ct.coverage_gaps(co.rules(which)[0], rule_ctx.twin(which, 257)[1]["events"]) == []


def test_rules_in_one_call_equal_one_call_each(rule_ctx):
    c = rule_ctx
    which = (0, 1, 2, 3, 4)
    for n in (65, 257):
        res, sums, _ = c.run(which, n)
        for r in which:
            one, osums, _ = c.run((r,), n)
            assert osums[0].tobytes() == sums[r].tobytes()
            assert np.float64(one[0].mean).tobytes() == np.float64(res[r].mean).tobytes()
            assert np.float64(one[0].m2).tobytes() == np.float64(res[r].m2).tobytes()


def test_random_head_and_tail_give_the_whole(rule_ctx):
    c = rule_ctx
    which = (0, 1, 2)
    _, whole, wd = c.run(which, 257, mode="random")
    _, head, _ = c.run(which, 100, mode="random")
    _, tail, td = c.run(which, 157, mode="random", first_path=100)
    assert np.array_equal(td, wd[100:])
    assert np.concatenate([head, tail], axis=1).tobytes() == whole.tobytes()


def test_rules_need_no_solve_and_a_solve_changes_nothing(sia, rule_ctx, table_case):
    c = rule_ctx
    which = (0, 1, 2, 3, 4)
    ini = (0.5, 10.37)  # an off-grid start: the state is two doubles
    _, sums = _check_rules(c, which, 65, "lhs", LHS, ini=ini)
    solved = table_case("testing").eng  # the same text, solved
    _, ssums, _ = c.run(which, 65, ini=ini, eng=solved)
    assert ssums.tobytes() == sums.tobytes()
    _, fsums, _ = c.run(which, 65, ini=ini, eng=c.fused)  # the fused text gives the plain text's sums
    assert fsums.tobytes() == sums.tobytes()


def test_table_calls_before_a_solve_are_a_state_error(sia, rule_ctx):
    with pytest.raises(sia.SdpgpuError, match="nothing has been solved") as e:
        rule_ctx.fused.custom_simulate_sampled(5, 1, *co.INI)
    assert e.value.code == 2


# ---- 5. the mirror -------------------------------------------------------------------------------------------------------------
def test_mirror_classes_over_user_lambdas(sia):
    """Simulation over the CustomFunctor recursion of test_mirror_class_over_user_lambdas, both samplers; CashSimulation's
    overdraft rules: device route = host loop through the Python lambdas."""
    shape, params, pmf = _overdraft_limit_case(sia, T=3)
    T = 3
    price, fix, vari, hold, rate, dep, sal, maxQ, minI, maxI, minC, maxC = params[:12]
    overhead = params[12:]

    def feasible(s):
        return [float(k) for k in range(int(maxQ) + 1)]

    def imm(s, action, d):
        revenue = price * min(s.getIniInventory() + action, d)
        fixedCost = fix if action > 0 else 0
        level = s.getIniInventory() + action - d
        before = s.getIniCash() - fixedCost - vari * action - hold * max(level, 0) - overhead[s.getPeriod() - 1]
        after = before - rate * max(-before, 0) + dep * max(before, 0) + revenue
        inc = after - s.getIniCash()
        inc += sal * max(level, 0) if s.getPeriod() == T else 0
        return inc

    def trans(s, action, d):
        nx = max(0, s.getIniInventory() + action - d)
        nc = s.getIniCash() + imm(s, action, d)
        nc = maxC if nc > maxC else nc
        nc = minC if nc < minC else nc
        nx = maxI if nx > maxI else nx
        nx = minI if nx < minI else nx
        r = sia.java_round(nc * 10)
        nc = float(abs(r) // 10 * (1 if r >= 0 else -1))
        return sia.CashState(s.getPeriod() + 1, nx, nc)

    functor = sia.CustomFunctor(shape=shape, source=cs.OVERDRAFT_LIMIT, params=params, getFeasibleAction=feasible,
                                stateTransitionFn=trans, immediateValueFn=imm)
    rec = sia.CashRecursion(sia.OptDirection.MAX, pmf, feasible, trans, imm, 1.0, functor=functor)
    ini = sia.CashState(1, 0.0, 10.0)
    dists = [sia.DiscreteDistribution([float(v) for v, _ in tile], [float(p) for _, p in tile]) for tile in pmf]
    # sampler="device": the mean is the device's reduction of the sums the host loop reproduces on the same demands
    sim = sia.Simulation(None, 65, rec, 1.0, seed=SEED, sampler="device")
    mean = sim.simulateSDPGivenSamplNum(ini)
    draw = [lambda u, tile=tile: tile_demands(tile, u) for tile in pmf]
    dem, _ = twin_sample(65, SEED, LHS, 0, draw)
    host = sim.simulateOnHost(ini, dem)
    assert sim.last_values.tobytes() == host.tobytes()
    assert abs(mean - (math.fsum(host.tolist()) / 65 + 10.0)) <= 1e-12 * abs(mean)
    center, radius = sim.simulateSDPwithErrorConfidence(ini, 0.5, 0.95, batch=500)
    assert len(sim.last_values) >= 1000 and math.isfinite(center) and math.isfinite(radius)
    # sampler="host": Python sampling, uploaded through custom_simulate
    hsim = sia.Simulation(dists, 33, rec, 1.0, seed=7, sampler="host")
    hmean = hsim.simulateSDPGivenSamplNum(ini)
    assert math.isfinite(hmean) and len(hsim.last_values) == 33
    # CashSimulation.simulatesSOD: the device route equals its host loop on the device's demands
    csim = sia.CashSimulation(None, 65, rec, 1.0, seed=SEED, sampler="device")
    optsS = np.array([[0.0, 9.0], [4.5, 9.5], [3.25, 8.0]])
    got = csim.simulatesSOD(ini, optsS, 0.0, maxQ, fix, vari)
    hsums = csim.simulateOverdraftRulesOnDemands(ini, [(0, optsS)], dem, 0.0, maxQ, fix, vari)
    assert csim.last_values[0].tobytes() == hsums[0].tobytes()
    assert abs(got - (math.fsum(hsums[0].tolist()) / 65 + 10.0)) <= 1e-12 * abs(got)
    rec.engine.close()
