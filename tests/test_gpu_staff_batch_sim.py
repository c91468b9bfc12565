"""The fit and rollout of a STAFF batch on the GPU (sdpgpu_batch_staff_fit_ss / _simulate, csrc/sdp_staff_batch_sim.hpp; DESIGN 4
"Workforce batch: fit and rollout").

Parity statement (include/sdpgpu.h): instance i, rule r of a batch returns BIT FOR BIT -- draws, flags, leaf sums, n_valid, mean,
m2 -- what sdpgpu_staff_simulate returns on a separable handle of instance i, hence what the host twin
(tests/staff_sim_twin.py) computes; the fit equals sdpgpu_fit_ss on the instance's getOptTable rows.  Every comparison below is
by bytes.  Shapes: hire limit 12, 13-row tables, T = 3-4 (and the SINGLES of tests/test_gpu_staff_batch.py); the trees cover one
leaf, a wave boundary, a part-filled last wave and two waves per (instance, rule)."""
import dataclasses
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import staff_cases  # noqa: E402
import staff_sim_twin as st  # noqa: E402
from test_gpu_staff_batch import SINGLES, _six, make_batch, variant  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20240607
TREES = ((1, 1, 1), (3, 2, 1), (63, 2, 1), (64, 2, 1), (65, 2, 1), (17, 4, 2))
MAXQS = (2 ** 31 - 1, 12)


def fit_tree(tree, T):
    return tuple(tree[:T]) + (1,) * max(0, T - len(tree))


def frac_rule(c):
    """A level rule around the instance's minimum staff, fractional so that the truncation shows: (T, 2)."""
    return np.array([[m + 1.75, m + 4.25] for m in c.functor.minStaffNum])


def bits(x):
    return np.float64(x).tobytes()


class Handle:
    """Instance `c` on its own separable handle, solved."""

    def __init__(self, sia, c, store_all=1):
        d = c.functor.to_desc(c.T)
        d.kernel, d.device, d.store_all_values = sia._abi.KERNEL_SEPARABLE, 0, store_all
        self.eng = sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len)
        self.eng.solve(sync=True)

    def roll(self, tree, ini, ss, seed=SEED):
        return self.eng.staff_simulate(tree, seed, ini, ss, want_sums=True, want_demands=True)

    def close(self):
        self.eng.close()


def assert_same_result(got, want, what):
    assert (got.n_paths, got.n_valid, got.n_lost) == (want.n_paths, want.n_valid, want.n_lost), what
    assert bits(got.mean) == bits(want.mean) and bits(got.m2) == bits(want.m2), (what, got.mean, want.mean, got.m2, want.m2)
    assert got.kernel_ms > 0, what


def assert_batch_equals_handles(b, handles, cases, tree, ss, what, seed=SEED):
    """One batch call (ss: (n, R, T, 2) or None) against one handle call per instance."""
    ini = cases[0].functor.iniStaffNum
    res, sums, valid, dem = b.staff_simulate(tree, seed, ini, ss, want_sums=True, want_demands=True)
    n_leaves = int(np.prod(tree))
    rules = 1 if ss is None else ss.shape[1]
    assert sums.shape == (len(cases), rules, n_leaves) and dem.shape == (len(cases), rules, n_leaves, cases[0].T)
    ms = {r.kernel_ms for row in res for r in row}
    assert len(ms) == 1  # (every result carries the kernel_ms of the whole call)
    for i, h in enumerate(handles):
        hres, hsums, hvalid, hdem = h.roll(tree, ini, None if ss is None else ss[i], seed)
        w = (what, tree, "instance", i)
        assert np.array_equal(dem[i], hdem), ("draws",) + w
        assert np.array_equal(valid[i], hvalid), ("flags",) + w
        assert sums[i].tobytes() == hsums.tobytes(), ("leaf sums",) + w
        for r in range(rules):
            assert_same_result(res[i][r], hres[r], w + ("rule", r))
    return res, sums, valid, dem


@pytest.fixture(scope="module")
def six(sia):
    """The batch of 6 of tests/test_gpu_staff_batch.py (5 variants over one table: a full instance block and a short one; a lone
    instance over another table, in the middle of the caller's order), solved, with every instance's own handle."""
    cases = _six(sia)
    b = make_batch(sia, cases)
    b.solve()
    handles = [Handle(sia, c) for c in cases]
    yield cases, b, handles
    b.close()
    for h in handles:
        h.close()


def rates_pair(sia):
    """tests/test_gpu_staff_batch.py::test_a_table_per_period: the clamped staff_rates, three rates as three pool tables; one
    instance walks them (0, 1, 2), the other (2, 1, 0)."""
    c = staff_cases.staff_rates()
    rates = [0.1, 0.6, 0.35]
    pool = [(sia.staff_level_pmf([r], 41)[0], None) for r in rates]
    f0 = c.functor
    f1 = dataclasses.replace(c.functor, fixCost=3.0, unitVariCost=0.5, salary=1.0, unitPenalty=20.0, minStaffNum=[7, 7, 1])
    use = [[0, 1, 2], [2, 1, 0]]
    descs = []
    for f in (f0, f1):
        d = f.to_desc(3)
        d.kernel, d.device = sia._abi.KERNEL_SEPARABLE, 0
        descs.append(d)
    cases = [staff_cases.StaffCase(f"rates{i}", f, sia.staff_level_pmf([rates[k] for k in use[i]], 41)) for i, f in enumerate((f0, f1))]
    return cases, sia.StaffBatch(descs, pool, use, [list(f0.minStaffNum), list(f1.minStaffNum)])


# ---- 1. parity with the handle, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SINGLES))
def test_a_batch_of_one_equals_its_handle(sia, name):
    c = SINGLES[name]()
    h = Handle(sia, c)
    try:
        with make_batch(sia, [c]) as b:
            b.solve()
            for tree in sorted({fit_tree(tr, c.T) for tr in TREES}):
                assert_batch_equals_handles(b, [h], [c], tree, frac_rule(c)[None, None], name + " level rule")
                res, _, valid, _ = assert_batch_equals_handles(b, [h], [c], tree, None, name + " table rule")
                assert valid.all() and res[0][0].n_valid == res[0][0].n_paths  # (the rows drawn from are the recursion's)
    finally:
        h.close()


def test_the_batch_of_six_equals_its_handles(six):
    cases, b, handles = six
    ss = np.stack([frac_rule(c) for c in cases])[:, None]
    for tree in TREES:
        tree = fit_tree(tree, 4)
        assert_batch_equals_handles(b, handles, cases, tree, ss, "six, level rule")
        assert_batch_equals_handles(b, handles, cases, tree, None, "six, table rule")


def test_tables_that_differ_by_period_and_the_clamp(sia):
    cases, b = rates_pair(sia)
    handles = [Handle(sia, c) for c in cases]
    try:
        with b:
            b.solve()
            # levels above maxX = 40 as well: the staff number is clamped AFTER the period's cost
            ss = np.stack([np.stack([frac_rule(c), np.array([[45.0, 60.0]] * 3)]) for c in cases])
            for tree in TREES:
                assert_batch_equals_handles(b, handles, cases, tree, ss, "rates, level rules")
                assert_batch_equals_handles(b, handles, cases, tree, None, "rates, table rule")
    finally:
        for h in handles:
            h.close()


# ---- 2. parity with the host twin: an oracle that does not run the code under test ---------------------------------------------
def test_the_batch_of_six_equals_the_host_twin(six):
    cases, b, _ = six
    ss = np.stack([frac_rule(c) for c in cases])[:, None]
    probs = [st.Problem(c.functor, c.table, c.row_len) for c in cases]
    pols = [[b.policy(i, t) for t in range(1, 5)] for i in range(len(cases))]
    x_lo = [int(b.grid(0, t)[0]) for t in range(1, 5)]
    for tree in TREES:
        tree = fit_tree(tree, 4)
        for rule in ("level", "table"):
            res, sums, valid, dem = b.staff_simulate(tree, SEED, 0, ss if rule == "level" else None, want_sums=True, want_demands=True)
            for i, P in enumerate(probs):
                want = st.simulate(P, tree, SEED, 0, ss=ss[i, 0]) if rule == "level" else st.simulate(P, tree, SEED, 0, policy=pols[i], x_lo=x_lo)
                w = (rule, tree, i)
                assert np.array_equal(dem[i, 0], want["demand"]), ("draws",) + w
                assert np.array_equal(valid[i, 0], want["valid"]), ("flags",) + w
                assert sums[i, 0].tobytes() == want["sum"].astype(np.float64).tobytes(), ("leaf sums",) + w
                assert res[i][0].n_valid == int(want["valid"].sum()) == res[i][0].n_paths, w


# ---- 3. rules and repeatability ----------------------------------------------------------------------------------------------
def test_rules_instances_and_repeats(sia, six):
    cases, b, _ = six
    tree = (17, 4, 2, 1)
    rules = np.stack([np.stack([frac_rule(c), frac_rule(c) + 2.0, np.zeros((4, 2))]) for c in cases])  # (6, 3, 4, 2)
    res, sums, valid, dem = b.staff_simulate(tree, SEED, 0, rules, want_sums=True, want_demands=True)
    assert sums.shape == (6, 3, 136) and len(res) == 6 and all(len(row) == 3 for row in res)
    # the rules of one call equal one call each
    for r in range(3):
        one, s1, v1, d1 = b.staff_simulate(tree, SEED, 0, rules[:, r], want_sums=True, want_demands=True)
        assert s1[:, 0].tobytes() == sums[:, r].tobytes() and np.array_equal(v1[:, 0], valid[:, r]) and np.array_equal(d1[:, 0], dem[:, r]), r
        for i in range(6):
            assert (bits(one[i][0].mean), bits(one[i][0].m2), one[i][0].n_valid) == (bits(res[i][r].mean), bits(res[i][r].m2), res[i][r].n_valid)
    assert sums[:, 0].tobytes() != sums[:, 1].tobytes()
    # the instances of one batch equal batches of one
    for i, c in enumerate(cases):
        with make_batch(sia, [c]) as b1:
            one, s1, v1, d1 = b1.staff_simulate(tree, SEED, 0, rules[i:i + 1], want_sums=True, want_demands=True)  # (level rules: no solve)
        assert s1[0].tobytes() == sums[i].tobytes() and np.array_equal(v1[0], valid[i]) and np.array_equal(d1[0], dem[i]), i
        for r in range(3):
            assert (bits(one[0][r].mean), bits(one[0][r].m2), one[0][r].n_valid) == (bits(res[i][r].mean), bits(res[i][r].m2), res[i][r].n_valid)
    # two identical calls: identical bits, with and without the optional outputs
    again = b.staff_simulate(tree, SEED, 0, rules)
    again_sums = b.staff_simulate(tree, SEED, 0, rules, want_sums=True)[1]
    assert again_sums.tobytes() == sums.tobytes()
    for i in range(6):
        for r in range(3):
            assert (bits(again[i][r].mean), bits(again[i][r].m2), again[i][r].n_valid) == (bits(res[i][r].mean), bits(res[i][r].m2), res[i][r].n_valid)
    # another seed: other draws
    other = b.staff_simulate(tree, SEED + 1, 0, rules, want_sums=True, want_demands=True)
    assert other[3].tobytes() != dem.tobytes() and other[1].tobytes() != sums.tobytes()


# ---- 4. the level rule's edges, a different rule row per instance --------------------------------------------------------------
def test_level_rule_edges_differ_per_instance(six):
    """The edges of tests/test_gpu_staff_simulate.py::test_level_rule_edge_cases, one per instance: a kernel that reads instance
    0's levels or costs for everybody differs from the handles here."""
    cases, b, handles = six
    tree = (17, 4, 2, 1)
    edge = [
        [[5.99, 9.99]] * 4,                            # truncation: the rule (5, 9)
        [[7.0, 6.0]] * 4,                              # S = s - 1: at x = s - 1 the rule hires 0
        [[0.0, 0.0]] * 4,                              # never hires from 0: nobody to leave, every draw 0
        [[20, 20], [30, 40], [5, 100], [1, 1]],        # S beyond the table: the draws come from its last row
        [[5.0, 9.0]] * 4,
        [[6.0, 10.0]] * 4,
    ]
    ss = np.array(edge, dtype=np.float64)[:, None]
    res, sums, valid, dem = assert_batch_equals_handles(b, handles, cases, tree, ss, "edges")
    assert valid.all()
    # truncation: instance 0 under (5.99, 9.99) is instance 0 under (5, 9), and not under (6, 10)
    ss59, ss610 = ss.copy(), ss.copy()
    ss59[0, 0], ss610[0, 0] = [[5.0, 9.0]] * 4, [[6.0, 10.0]] * 4
    s59 = b.staff_simulate(tree, SEED, 0, ss59, want_sums=True)[1]
    s610 = b.staff_simulate(tree, SEED, 0, ss610, want_sums=True)[1]
    assert s59[0].tobytes() == sums[0].tobytes() and s610[0].tobytes() != sums[0].tobytes()
    assert s59[1:].tobytes() == sums[1:].tobytes()  # (the other instances do not read instance 0's levels)
    # never hiring from 0 (instance 2: salary 5, unitPenalty 250, minStaffNum 9, 1, 9, 1): the closed form
    assert not dem[2].any() and set(sums[2, 0].tolist()) == {250.0 * (9 + 1 + 9 + 1)} and res[2][0].mean == 5000.0 and res[2][0].m2 == 0.0
    # S beyond the 13-row table
    assert 0 <= dem[3].min() and dem[3].max() <= 12
    # the twin as well, so that the handles are not the only witness
    for i, c in enumerate(cases):
        want = st.simulate(st.Problem(c.functor, c.table, c.row_len), tree, SEED, 0, ss=ss[i, 0])
        assert np.array_equal(dem[i, 0], want["demand"]) and sums[i, 0].tobytes() == want["sum"].astype(np.float64).tobytes(), i


# ---- 5. the fit --------------------------------------------------------------------------------------------------------------
def sweep64(sia):
    """The 64 instances of tests/test_gpu_staff_batch.py::test_scaled_sweep, in its order: (cases, descs, pool, use)."""
    T = 4
    tabs = [sia.staff_level_pmf([r] * T, 13) for r in (0.1, 0.5)]
    cases, descs, use = [], [], []
    for g, table in enumerate(tabs):
        for fix in (50, 1000):
            for salary in (30, 200):
                for pen in (50, 2200):
                    for ms in ([4, 4, 4, 4], [1, 2, 3, 4], [8, 6, 4, 2], [4, 5, 8, 6]):
                        f = sia.StaffFunctor(fixCost=fix, unitVariCost=20, salary=salary, unitPenalty=pen, minStaffNum=ms,
                                             maxHireNum=12, clampStaff=False, iniStaffNum=0)
                        cases.append(staff_cases.StaffCase(f"sweep{len(cases)}", f, table))
                        d = f.to_desc(T)
                        d.kernel, d.device = sia._abi.KERNEL_SEPARABLE, 0
                        descs.append(d)
                        use.append([g] * T)
    return cases, descs, [(table[0], None) for table in tabs], use


def reach_of(c):
    from stochastic_inventory_amd.workforce import staff_reach_intervals
    rows = c.table.shape[1]
    lens = np.arange(rows, dtype=np.int64) + 1 if c.row_len is None else np.asarray(c.row_len, dtype=np.int64)
    return staff_reach_intervals(c.functor, [lens] * c.T)


_oracle = {}


def oracle_rows(c):
    """[(x, Q)] per period: the oracle's policy on the staff numbers the recursion visits (oracle/staffref, solved once a case)."""
    if c.name not in _oracle:
        from oracle import staffref
        staffref.build()
        P = c.oracle_problem(staffref)
        _, pol, _ = P.solve()
        out = []
        for t, (L, H) in enumerate(reach_of(c)):
            x0 = int(P.x_lo[t])
            out.append((np.arange(L, H + 1), np.asarray(pol[t][L - x0:H - x0 + 1])))
        _oracle[c.name] = out
    return _oracle[c.name]


def oracle_is_one_rule(c):
    """(s, S) per period when the oracle's policy on the visited rows is `S - x below s, else 0` in EVERY period, else None."""
    ss = []
    for x, q in oracle_rows(c):
        hires = np.nonzero(q > 0)[0]
        if len(hires) == 0:
            return None
        s, S = int(x[hires[-1]]) + 1, int(x[hires[0]] + q[hires[0]])
        if not np.array_equal(q, np.where(x < s, S - x, 0)):
            return None
        ss.append([s, S])
    return ss


def assert_fit_covers_the_branches(cases, limit):
    """On the ORACLE's tables: among the periods 2 .. T of these instances there is one with rows at the limit, one whose first
    row hires 0 and one that hires on every visited row -- the branches of FitsS.levelIndex / getSinglesS."""
    seen = set()
    for c in cases:
        for x, q in oracle_rows(c)[1:]:
            seen |= {"limit"} if (q == limit).any() else set()
            seen |= {"first0"} if q[0] == 0 else set()
            seen |= {"all"} if (q > 0).all() else set()
    assert seen == {"limit", "first0", "all"}, seen


def opt_table(b, i, c):
    """getOptTable of instance i from the batch's policy rows, over the numpy statement of the visited intervals."""
    rows = []
    for period, (L, H) in enumerate(reach_of(c), start=1):
        x_lo = int(b.grid(i, period)[0])
        pol = b.policy(i, period)
        x = np.arange(L, H + 1, dtype=np.int64)
        rows.append(np.stack([np.full(len(x), float(period)), x.astype(np.float64), pol[x - x_lo].astype(np.float64)], axis=1))
    return np.concatenate(rows, axis=0)


def assert_fit_is_the_host_fit(sia, b, cases):
    for maxq in MAXQS:
        got = b.fit_ss(maxq)
        assert got.shape == (len(cases), cases[0].T, 2)
        for i, c in enumerate(cases):
            want = sia.FitsS(maxq, c.T).getSinglesS(opt_table(b, i, c))
            assert got[i].tobytes() == np.asarray(want, dtype=np.float64).tobytes(), (maxq, i, got[i].tolist(), np.asarray(want).tolist())


def test_the_fit_of_the_batch_of_six(sia, six):
    cases, b, _ = six
    assert_fit_covers_the_branches(cases, 12)
    assert_fit_is_the_host_fit(sia, b, cases)


def test_the_fit_of_the_scaled_sweep(sia):
    cases, descs, pool, use = sweep64(sia)
    assert_fit_covers_the_branches(cases, 12)
    with sia.StaffBatch(descs, pool, use, [list(c.functor.minStaffNum) for c in cases]) as b:
        b.solve()
        assert_fit_is_the_host_fit(sia, b, cases)


# ---- 6. the loop body of WorkforceTesting.main -------------------------------------------------------------------------------
def test_the_loop_body_on_the_scaled_sweep(sia):
    cases, _, _, _ = sweep64(sia)
    tree = (10, 10, 1, 3)
    one_rule = {i: ss for i, c in enumerate(cases) for ss in [oracle_is_one_rule(c)] if ss is not None}
    assert len(one_rule) >= 8  # (asserted on the oracle's tables: these policies ARE one (s, S) rule per period)
    with sia.StaffRecursionBatch([c.functor for c in cases], [c.table for c in cases], 4, device=0) as rec:
        assert rec.num_tables == 8  # (two arrays, four period slices each)
        opt, _ = rec.initial()
        levels = rec.fitSinglesS()
        assert levels.shape == (64, 4, 2) and np.isfinite(levels).all()
        both = rec.simulatesS(np.stack([levels, levels + 1.0], axis=1), tree, SEED)
        assert both.shape == (64, 2) and np.isfinite(both).all()
        assert all(r.n_valid == r.n_paths == 300 for row in rec.last_results for r in row)
        single = rec.simulatesS(levels, tree, SEED)
        assert single.shape == (64,) and single.tobytes() == both[:, 0].copy().tobytes()  # slot 0 equals the single-rule call
        table = rec.simulateTable(tree, SEED)
        assert table.shape == (64,) and np.isfinite(table).all()
        assert all(r.n_valid == r.n_paths == 300 for row in rec.last_results for r in row)
        t_sums = rec.batch.staff_simulate(tree, SEED, 0, None, want_sums=True)[1]
        l_sums = rec.batch.staff_simulate(tree, SEED, 0, levels, want_sums=True)[1]
        for i in one_rule:
            assert l_sums[i].tobytes() == t_sums[i].tobytes(), i
            assert bits(single[i]) == bits(table[i]), i
        gap = (single - opt) * 100 / opt
        print(f"gapPercent of the fitted rule: min {gap.min():.3f} max {gap.max():.3f}")
    from stochastic_inventory_amd import workloads
    sweep = [workloads.StaffWorkload(c.name, c.functor, c.table) for c in cases]
    out = workloads.workforce_testing_loop(sweep, mip_levels=levels + 1.0, sampleNums=tree, seed=SEED, device=0)
    assert out["sim"].tobytes() == both.tobytes() and out["levels"].tobytes() == levels.tobytes() and out["opt"].tobytes() == opt.tobytes()
    assert out["gapPercent"].shape == (64, 2) and np.isfinite(out["gapPercent"]).all()


# ---- 7. two ping-pong value tables -------------------------------------------------------------------------------------------
def test_ping_pong_tables_fit_and_roll_like_whole_tables(sia):
    """store_all_values = 0 keeps two value tables, and the whole policy arena: the fit and the table rule read that arena only."""
    a = staff_cases.staff_testing_small()
    cases = [a, variant(a, "pp1", fixCost=0.0, salary=9.0, minStaffNum=[1, 1, 12, 3])]
    tree = (65, 2, 1, 1)
    out = []
    for store_all in (1, 0):
        with make_batch(sia, cases, store_all=store_all) as b:
            b.solve()
            res, sums, valid, dem = b.staff_simulate(tree, SEED, 0, None, want_sums=True, want_demands=True)
            out.append(([b.fit_ss(q).tobytes() for q in MAXQS], sums.tobytes(), valid.tobytes(), dem.tobytes(),
                        [(bits(r.mean), bits(r.m2), r.n_valid) for row in res for r in row]))
            assert valid.all()
    assert out[0] == out[1]
