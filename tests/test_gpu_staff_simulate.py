"""Workforce rollout on a sampled tree, on the GPU (sdpgpu_staff_simulate, csrc/sdp_staff_sim.hpp; DESIGN 4 "Workforce rollout
on a sampled tree"): the draws, flags and leaf sums equal the host twin (tests/staff_sim_twin.py) bit for bit under the level
rule and under the policy table, the reduction stays inside the bound its documented order gives, several rules in one call
equal one call each, and the estimate is unbiased."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import staff_cases  # noqa: E402
import staff_sim_twin as st  # noqa: E402
from test_simulate_sampled_host import reduction_chain  # noqa: E402
from test_staff_simulate_host import UNBIASED_CASES, UNBIASED_SEEDS, UNBIASED_TREE, oracle_tables, unbiased  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20240607
# what can break: one leaf; the reference's order; two waves, one partial; a wave boundary, and sigma's half width changes between
# 64 and 65; odd sizes; one child in the middle (T = 4 only)
TREES = ((1, 1, 1), (3, 2, 1), (10, 10, 1), (63, 2, 1), (64, 2, 1), (65, 2, 1), (17, 4, 2))
TREES_T4 = ((2, 3, 1, 7),)
_ids = lambda f: f.__name__  # noqa: E731


def fit_tree(tree, T):
    return tuple(tree[:T]) + (1,) * max(0, T - len(tree))


def trees_of(T):
    out = []
    for tr in TREES + (TREES_T4 if T == 4 else ()):
        tr = fit_tree(tr, T)
        if tr not in out:
            out.append(tr)
    return out


class Ctx:
    """One solved case: engine, the oracle's tables, the twin's problem record."""

    def __init__(self, sia, make):
        self.c, self.V, self.pol, self.x_lo = oracle_tables(make)
        c = self.c
        d = c.functor.to_desc(c.T)
        d.device = 0
        self.eng = sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len)
        self.eng.solve()
        self.P = st.Problem(c.functor, c.table, c.row_len)
        self.T = c.T
        self.ini = c.functor.iniStaffNum
        # a level rule around the minimum staff, fractional so that the truncation shows
        self.ss = np.array([[m + 1.75, m + 4.25] for m in c.functor.minStaffNum])


_ctx = {}


@pytest.fixture
def ctx(sia):
    def get(make):
        if make.__name__ not in _ctx:
            _ctx[make.__name__] = Ctx(sia, make)
        return _ctx[make.__name__]
    return get


def check_against_twin(eng, res, sums, valid, dem, want, what):
    n = len(want["sum"])
    assert np.array_equal(dem, want["demand"]), "draws: " + what
    assert np.array_equal(valid, want["valid"]), "flags: " + what
    assert sums.tobytes() == want["sum"].astype(np.float64).tobytes(), "leaf sums: " + what
    assert res.n_paths == n and res.n_valid == int(want["valid"].sum()) and res.n_lost == 0 and res.kernel_ms > 0, what
    if res.n_valid < n:
        assert math.isnan(res.mean) and math.isnan(res.m2), what
        return
    u, L = 2.0 ** -53, reduction_chain(n)
    ref = math.fsum(sums.tolist()) / n
    X = math.fsum(np.abs(sums).tolist()) / n
    print(f"{what}: mean {res.mean!r} fsum {ref!r} err/X/u {abs(res.mean - ref) / (X * u) if X else 0:.2f} of {L + 1}")
    assert abs(res.mean - ref) <= (L + 1) * u * X, ("mean", what, res.mean, ref)
    ref2 = math.fsum(((sums - res.mean) ** 2).tolist())
    print(f"    m2 {res.m2!r} fsum {ref2!r} err/m2/u {abs(res.m2 - ref2) / (res.m2 * u) if res.m2 else 0:.2f} of {L + 6}")
    assert abs(res.m2 - ref2) <= (L + 6) * u * res.m2, ("m2", what, res.m2, ref2)


def run_level(c, tree, ss, seed=SEED, ini=None):
    ini = c.ini if ini is None else ini
    res, sums, valid, dem = c.eng.staff_simulate(tree, seed, ini, ss, want_sums=True, want_demands=True)
    want = st.simulate(c.P, tree, seed, ini, ss=ss)
    check_against_twin(c.eng, res[0], sums[0], valid[0], dem[0], want, f"{c.c.name} level rule, tree {tree}")
    return res[0], sums[0]


def run_table(c, tree, seed=SEED):
    res, sums, valid, dem = c.eng.staff_simulate(tree, seed, c.ini, None, want_sums=True, want_demands=True)
    want = st.simulate(c.P, tree, seed, c.ini, policy=c.pol, x_lo=c.x_lo)
    check_against_twin(c.eng, res[0], sums[0], valid[0], dem[0], want, f"{c.c.name} table rule, tree {tree}")
    assert res[0].n_valid == res[0].n_paths  # (the rows drawn from are the recursion's: no leaf leaves the boxes)
    return res[0], sums[0]


# ---- 1. parity with the twin, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("make", staff_cases.ALL, ids=_ids)
def test_both_rules_equal_the_twin(ctx, make):
    c = ctx(make)
    for tree in trees_of(c.T):
        run_level(c, tree, c.ss)
        run_table(c, tree)


# ---- 2. the level rule's edges ----------------------------------------------------------------------------------------------
def test_level_rule_edge_cases(ctx):
    c = ctx(staff_cases.staff_testing_small)  # no clamp, 13 rows
    tree = (17, 4, 2, 1)
    # truncation: (5.99, 9.99) is the rule (5, 9)
    _, a = run_level(c, tree, np.array([[5.99, 9.99]] * 4))
    _, b = run_level(c, tree, np.array([[5.0, 9.0]] * 4))
    _, b6 = run_level(c, tree, np.array([[6.0, 10.0]] * 4))
    assert a.tobytes() == b.tobytes() and a.tobytes() != b6.tobytes()
    # S = s - 1: at x = s - 1 the rule hires 0
    run_level(c, tree, np.array([[7.0, 6.0]] * 4), ini=6)
    run_level(c, tree, np.array([[7.0, 6.0]] * 4), ini=0)
    # never hires from 0: nobody to leave, every draw 0
    res, sums, valid, dem = c.eng.staff_simulate(tree, SEED, 0, [[0, 0]] * 4, want_sums=True, want_demands=True)
    assert not dem.any() and valid.all() and set(sums[0].tolist()) == {250.0 * (4 + 9 + 6 + 3)} and res[0].mean == 5500.0 and res[0].m2 == 0.0
    run_level(c, tree, np.array([[0.0, 0.0]] * 4), ini=0)
    # S beyond the table: the draws come from its last row
    res, sums, valid, dem = c.eng.staff_simulate(tree, SEED, 0, [[20, 20], [30, 40], [5, 100], [1, 1]], want_sums=True, want_demands=True)
    assert 0 <= dem.min() and dem.max() <= 12
    run_level(c, tree, np.array([[20, 20], [30, 40], [5, 100], [1, 1]], dtype=np.float64))
    # the same on a clamped handle: the staff number is clamped AFTER the period's cost
    run_level(ctx(staff_cases.staff_rates), (17, 4, 2), np.array([[45.0, 60.0]] * 3))


# ---- 3. several rules in one call -------------------------------------------------------------------------------------------
def test_rules_in_one_call_equal_one_call_each(ctx):
    for make, tree in ((staff_cases.staff_testing_small, (10, 10, 1, 3)), (staff_cases.staff_short_rows, (65, 2, 3))):
        c = ctx(make)
        rules = np.stack([c.ss, c.ss + 2.0, np.array([[0.0, 0.0]] * c.T)])
        res, sums, valid, dem = c.eng.staff_simulate(tree, SEED, c.ini, rules, want_sums=True, want_demands=True)
        assert len(res) == 3 and sums.shape == (3, int(np.prod(tree)))
        for r in range(3):
            one, s1, v1, d1 = c.eng.staff_simulate(tree, SEED, c.ini, rules[r], want_sums=True, want_demands=True)
            assert s1[0].tobytes() == sums[r].tobytes() and np.array_equal(v1[0], valid[r]) and np.array_equal(d1[0], dem[r])
            assert np.float64(one[0].mean).tobytes() == np.float64(res[r].mean).tobytes()
            assert np.float64(one[0].m2).tobytes() == np.float64(res[r].m2).tobytes() and one[0].n_valid == res[r].n_valid
        assert sums[0].tobytes() != sums[1].tobytes()
        # two identical calls: identical bits, with and without the optional outputs
        again = c.eng.staff_simulate(tree, SEED, c.ini, rules)
        for r in range(3):
            assert (np.float64(again[r].mean).tobytes(), np.float64(again[r].m2).tobytes()) == (np.float64(res[r].mean).tobytes(), np.float64(res[r].m2).tobytes())
        # another seed: other draws
        other = c.eng.staff_simulate(tree, SEED + 1, c.ini, rules, want_sums=True)[1]
        assert other[0].tobytes() != sums[0].tobytes()


# ---- 4. the reference's default tree ----------------------------------------------------------------------------------------
def test_the_default_tree_of_ten_thousand_leaves(sia):
    from stochastic_inventory_amd.pmf import staff_level_pmf
    T = 8
    f = sia.StaffFunctor(fixCost=50, unitVariCost=20, salary=30, unitPenalty=50, minStaffNum=[10, 12, 8, 10, 14, 9, 10, 6], maxHireNum=12,
                         clampStaff=False, iniStaffNum=0)
    table = staff_level_pmf([0.2] * T, 31)
    rec = sia.StaffRecursion(pmf=table, T=T, functor=f, device=0)
    sim = sia.SimulatesS(rec, T, [0.2] * T, seed=SEED)
    tree = sim.defaultSampleNums()
    assert tree == [10, 10, 10, 10, 1, 1, 1, 1]
    P = st.Problem(f, table)
    ss = np.array([[m + 2.0, m + 7.0] for m in f.minStaffNum])
    # level rule: needs no solve
    res, sums, valid, dem = rec.engine.staff_simulate(tree, SEED, 0, ss, want_sums=True, want_demands=True)
    want = st.simulate(P, tree, SEED, 0, ss=ss)
    check_against_twin(rec.engine, res[0], sums[0], valid[0], dem[0], want, "default tree, level rule")
    assert sim.simulatesS(sia.StaffState(1, 0), ss) == res[0].mean and sim.last_results[0].n_valid == 10000
    # table rule
    mean = sim.simulateTable(sia.StaffState(1, 0))
    res, sums, valid, dem = rec.engine.staff_simulate(tree, SEED, 0, None, want_sums=True, want_demands=True)
    pol = [rec.engine.policy(t) for t in range(1, T + 1)]
    x_lo = [int(rec.engine.grid(t)[0]) for t in range(1, T + 1)]
    want = st.simulate(P, tree, SEED, 0, policy=pol, x_lo=x_lo)
    check_against_twin(rec.engine, res[0], sums[0], valid[0], dem[0], want, "default tree, table rule")
    assert mean == res[0].mean
    rec.close()


# ---- 5. a policy that IS a level rule ---------------------------------------------------------------------------------------
def test_level_rule_equals_table_rule_where_the_policy_is_one(ctx):
    """staff_planning_small: the oracle's policy of every period is `S_t - x below s_t, else 0` (asserted here on the oracle's
    tables first); rolling that rule and rolling the table give the same leaf sums bit for bit."""
    c = ctx(staff_cases.staff_planning_small)
    ss = []
    for t, p in enumerate(c.pol):
        x = c.x_lo[t] + np.arange(len(p))
        hires = np.nonzero(p > 0)[0]
        assert len(hires) > 0
        s, S = int(x[hires[-1]]) + 1, int(x[hires[0]] + p[hires[0]])
        assert np.array_equal(p, np.where(x < s, S - x, 0)), f"period {t + 1} is not one (s, S) rule"
        ss.append([s, S])
    assert ss == [[10, 17], [11, 19], [8, 16]]
    for tree in ((10, 10, 1), (17, 4, 2)):
        _, a = run_level(c, tree, np.array(ss, dtype=np.float64))
        _, b = run_table(c, tree)
        assert a.tobytes() == b.tobytes()
    rl = c.eng.staff_simulate((17, 4, 2), SEED, c.ini, ss)[0]
    rt = c.eng.staff_simulate((17, 4, 2), SEED, c.ini, None)[0]
    assert (rl.mean, rl.m2, rl.n_valid) == (rt.mean, rt.m2, rt.n_valid)


# ---- 6. the estimate --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", UNBIASED_CASES, ids=_ids)
def test_the_device_means_are_unbiased(ctx, make):
    c = ctx(make)
    idx = c.eng.state_index(1, float(c.ini))
    v1 = float(c.eng.values(1)[idx])
    means = []
    for seed in UNBIASED_SEEDS:
        r = c.eng.staff_simulate(UNBIASED_TREE, seed, c.ini, None)[0]
        assert r.n_valid == r.n_paths == 100
        means.append(r.mean)
    holds, text = unbiased(means, v1)
    print(c.c.name, text)
    assert holds, text


# ---- 7. the loop body of WorkforceTesting.main ------------------------------------------------------------------------------
def test_the_workforce_testing_loop_body(sia):
    from stochastic_inventory_amd.pmf import staff_level_pmf
    T = 4
    f = sia.StaffFunctor(fixCost=50, unitVariCost=20, salary=5, unitPenalty=250, minStaffNum=[4, 9, 6, 3], maxHireNum=12, clampStaff=False,
                         iniStaffNum=0)
    rec = sia.StaffRecursion(pmf=staff_level_pmf([0.3] * T, 13), T=T, functor=f, device=0)
    initial = sia.StaffState(1, 0)
    simulate = sia.SimulatesS(rec, T, [0.3] * T)
    opt = rec.getExpectedValue(initial)
    opt_table = rec.getOptTable()
    opts_s = sia.FitsS(2 ** 31 - 1, T).getSinglesS(opt_table)
    assert np.asarray(opts_s).shape == (T, 2)
    sim = simulate.simulatesS(initial, opts_s)
    r = simulate.last_results[0]
    assert math.isfinite(sim) and r.n_valid == r.n_paths == 10000 and sim == r.mean
    gap = (sim - opt) * 100 / opt
    print(f"opt {opt!r} sim {sim!r} gap {gap:.2f} % levels {np.asarray(opts_s).tolist()}")
    # two rules at once (the fitted one and a second, as the MIP's would arrive): the first equals the single call
    both = simulate.simulatesS(initial, np.stack([opts_s, np.asarray(opts_s) + 1.0]))
    assert both.shape == (2,) and both[0] == sim and math.isfinite(both[1])
    assert math.isfinite(simulate.simulateTable(initial)) and simulate.last_results[0].n_valid == 10000
    rec.close()
