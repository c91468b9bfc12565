"""Cash rule rollout on the GPU (sdpgpu_cash_rule_simulate, csrc/sdp_cash_rule_sim.hpp; DESIGN 4 "Cash rule rollout"): the path
sums equal the host twin (tests/cash_rule_twin.py) bit for bit on the demands sdpgpu_sample_demands returns -- each form alone and
five rules in one call --, the R-rule call equals R one-rule calls, the reduction stays inside the bound its documented order
gives, the start may lie off the grid and nothing needs a solve, RANDOM calls continue one stream, and the Python mirror's device
route equals its host loop.  Cases, sizes and rules: tests/test_cash_rule_host.py, whose coverage condition shows that they take
every branch of the definition."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
import cash_rule_twin as ct  # noqa: E402
from test_cash_rule_host import CASES, LHS, MIXED_FORMS, NS, RANDOM, SEED, reference, setup_of  # noqa: E402
from test_gpu_staff_simulate import check_against_twin  # noqa: E402

pytestmark = pytest.mark.gpu

_ids = lambda f: f.__name__  # noqa: E731
_eng = {}


@pytest.fixture
def ctx(sia):
    """(setup, engine) of a case; the engine is created once and NEVER solved here."""
    def get(make):
        s = setup_of(make)
        if make.__name__ not in _eng:
            d = s.w.desc()
            d.device = 0
            _eng[make.__name__] = sia.SdpEngine(d, s.w.pmf, s.w.overhead())
        return s, _eng[make.__name__]
    return get


def call(s, eng, n, which, mode="lhs", first_path=0, ini=None, c1="own", c2="own"):
    """The rules `which` (indices into the setup's five) in one call -> (results, sums[R, n])."""
    which = list(which)
    x, cash = s.ini if ini is None else ini
    return eng.cash_rule_simulate(n, SEED, x, cash, s.forms[which], s.rules[which], c1_tab=s.c1[which] if isinstance(c1, str) else c1,
                                  c2_tab=s.c2[which] if isinstance(c2, str) else c2, mode=mode, first_path=first_path, discount=s.disc,
                                  want_sums=True, **s.scalars)


def check(eng, res, sums, dem, want_sum, what):
    """Sums, counts and the reduction's bound: the check of tests/test_gpu_staff_simulate.py (every path is valid here)."""
    n = len(want_sum)
    valid = np.ones(n, dtype=bool)
    check_against_twin(eng, res, sums, valid, dem, {"sum": want_sum, "valid": valid, "demand": dem}, what)


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


# ---- 1. parity with the twin, many rules versus one, the reduction ----------------------------------------------------------
@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_each_form_and_the_mixed_call_equal_the_twin(ctx, make):
    s, eng = ctx(make)
    for n in NS:
        dem, want = reference(make, n)
        got_dem, _ = eng.sample_demands(n, SEED)
        assert np.array_equal(got_dem, dem), f"{s.w.name}: demands, n = {n}"
        res, sums = call(s, eng, n, range(5))
        assert len(res) == 5 and sums.shape == (5, n)
        for r in range(5):
            check(eng, res[r], sums[r], dem, want["sum"][r], f"{s.w.name} rule {r} (form {MIXED_FORMS[r]}) of five, n = {n}")
            assert res[r].kernel_ms == res[0].kernel_ms  # (of the whole call)
            # the R-rule call equals R one-rule calls: sums, mean and m2
            one, s1 = call(s, eng, n, [r])
            assert s1[0].tobytes() == sums[r].tobytes(), (s.w.name, n, r)
            assert same_bits(one[0].mean, res[r].mean) and same_bits(one[0].m2, res[r].m2), (s.w.name, n, r)
            assert one[0].n_valid == one[0].n_paths == n and one[0].n_lost == 0
        # without the sums buffer: the same results
        again = eng.cash_rule_simulate(n, SEED, *s.ini, s.forms, s.rules, c1_tab=s.c1, c2_tab=s.c2, discount=s.disc, **s.scalars)
        assert all(same_bits(a.mean, b.mean) and same_bits(a.m2, b.m2) for a, b in zip(again, res))
    # the rules differ: the forms did not all order alike
    assert sums[0].tobytes() != sums[1].tobytes() and sums[1].tobytes() != sums[2].tobytes()


def test_null_tables_are_tables_without_keys(ctx):
    """A NULL c1_tab / c2_tab: every key absent -- the twin with no table, and what an all-NaN table gives."""
    s, eng = ctx(cases.f3_tenths)
    n = 257
    dem, _ = reference(cases.f3_tenths, n)
    want = ct.simulate(s.P, dem, s.disc, *s.ini, s.forms[:2], s.rules[:2], None, None, *s.args())
    res, sums = call(s, eng, n, [0, 1], c1=None, c2=None)
    for r in range(2):
        check(eng, res[r], sums[r], dem, want["sum"][r], f"no tables, rule {r}")
    nan = np.full((2, s.T, s.P.nx), np.nan)
    res2, sums2 = call(s, eng, n, [0, 1], c1=nan, c2=nan)
    assert sums2.tobytes() == sums.tobytes() and same_bits(res2[0].mean, res[0].mean)
    # C2 alone: form 0 with its own C2 and no C1
    want = ct.simulate(s.P, dem, s.disc, *s.ini, s.forms[:1], s.rules[:1], None, s.c2[:1], *s.args())
    res, sums = call(s, eng, n, [0], c1=None)
    check(eng, res[0], sums[0], dem, want["sum"][0], "C2 only")


# ---- 2. start state and solve ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", (cases.f3_tenths, cases.f3_testing), ids=_ids)
def test_off_grid_start_and_no_solve(ctx, make):
    s, eng = ctx(make)
    n = 257
    ini = (0.5, s.ini[1] + 0.37)  # neither an inventory grid point nor a cash key
    assert eng.state_index(1, *ini) < 0
    dem, want = reference(make, n, ini=ini)
    res, sums = call(s, eng, n, range(5), ini=ini)
    for r in range(5):
        check(eng, res[r], sums[r], dem, want["sum"][r], f"{s.w.name} off-grid start, rule {r}")
    # a solve changes nothing: the rollout reads no table of the handle
    eng.solve()
    res2, sums2 = call(s, eng, n, range(5), ini=ini)
    assert sums2.tobytes() == sums.tobytes() and all(same_bits(a.mean, b.mean) and same_bits(a.m2, b.m2) for a, b in zip(res, res2))


# ---- 3. RANDOM mode continues one stream ------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", CASES, ids=_ids)
def test_random_calls_continue_one_stream(ctx, make):
    s, eng = ctx(make)
    dem, want = reference(make, 257, RANDOM, 0)
    assert np.array_equal(eng.sample_demands(257, SEED, mode="random")[0], dem)
    res, whole = call(s, eng, 257, range(5), mode="random")
    for r in range(5):
        check(eng, res[r], whole[r], dem, want["sum"][r], f"{s.w.name} random, rule {r}")
    _, head = call(s, eng, 100, range(5), mode="random", first_path=0)
    _, tail = call(s, eng, 157, range(5), mode="random", first_path=100)
    assert np.concatenate([head, tail], axis=1).tobytes() == whole.tobytes()
    # another stream than the latin hypercube's
    assert whole.tobytes() != reference(make, 257)[1]["sum"].tobytes()


# ---- 4. the Python mirror ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", (cases.f3_tenths, cases.f3_testing), ids=_ids)
def test_cash_simulation_device_route_equals_its_host_loop(sia, make):
    s = setup_of(make)
    w, f = s.w, s.f
    n = 257
    rec = sia.CashRecursion(w.direction, w.pmf, functor=f, discountFactor=f.discountFactor, device=0)
    try:
        dev = sia.CashSimulation(None, n, rec, f.discountFactor, seed=SEED, sampler="device")  # None: the recursion's own tiles
        host = sia.CashSimulation(None, n, rec, f.discountFactor, seed=SEED, sampler="host")
        ini = sia.CashState(1, *s.ini)
        dem, _ = rec.engine.sample_demands(n, SEED)
        rules = s.rule_tuples()
        u = 2.0 ** -53

        def agrees(value, r):
            """The device's path sums are the host loop's; its mean is their mean to the reduction's bound; + iniCash."""
            want = host.simulateRulesOnDemands(ini, [rules[r]], dem, *s.args())[0]
            assert dev.last_values[0].tobytes() == want.tobytes(), (w.name, r)
            res = dev.last_results[0]
            assert value == res.mean + s.ini[1] and res.n_valid == n
            X = math.fsum(np.abs(want).tolist()) / n
            assert abs(res.mean - math.fsum(want.tolist()) / n) <= 18 * u * X  # L(257) + 1

        agrees(dev.simulatesCS(ini, rules[0][1], rules[0][2], rules[0][3], *s.args()), 0)
        agrees(dev.simulatesCS(ini, rules[1][1], rules[1][2], *s.args()), 1)
        agrees(dev.simulatesMeanCS(ini, rules[2][1], *s.args()), 2)
        # the four calls of CashConstraintTesting.main as one
        all4 = dev.simulateRules(ini, rules[:4], *s.args())
        assert all4.shape == (4,) and dev.last_values.shape == (4, n)
        assert dev.last_values.tobytes() == host.simulateRulesOnDemands(ini, rules[:4], dem, *s.args()).tobytes()
        assert all4[0] == dev.simulatesCS(ini, rules[0][1], rules[0][2], rules[0][3], *s.args())
    finally:
        rec.engine.close()
