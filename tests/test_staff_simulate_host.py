"""Workforce rollout on a sampled tree (sdpgpu_staff_simulate, SdpEngine.staff_simulate, workforce.SimulatesS; DESIGN 4
"Workforce rollout on a sampled tree") as far as it goes without a GPU: the new symbol and class, every refusal with a text
naming the argument BEFORE any device call, the self-checks of the host twin (tests/staff_sim_twin.py), and the unbiasedness
of the twin under the oracle's policy -- the statistic tests/test_gpu_staff_simulate.py reuses on the device's means."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
import sampler_twin as tw  # noqa: E402
import staff_cases  # noqa: E402
import staff_sim_twin as st  # noqa: E402

OK, ERR_ARG, ERR_STATE, ERR_DEVICE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the unbiasedness statistic: 64 fixed seeds, the tree (10, 10, 1)
UNBIASED_SEEDS = tuple(1000 + 7 * k for k in range(64))
UNBIASED_TREE = (10, 10, 1)
UNBIASED_CASES = (staff_cases.staff_planning_small, staff_cases.staff_rates)


def unbiased(means, v1):
    """|mean of means - V_1(ini)| <= 4 sd(means) / 8 over the 64 seeds (sd with n - 1).  The means of different seeds are
    independent, so sd / sqrt(64) is a valid standard error of their mean; per-leaf standard errors are not (leaves share
    prefixes).  Returns (holds, text)."""
    means = np.asarray(means, dtype=np.float64)
    assert means.shape == (64,)
    gap, bound = abs(float(means.mean()) - v1), 4.0 * float(means.std(ddof=1)) / 8.0
    return gap <= bound, f"mean of means {means.mean()!r}, V_1 {v1!r}: gap {gap:.6g}, bound {bound:.6g}"


_oracle = {}


def oracle_tables(make):
    """(case, V, policy, x_lo) of the CPU oracle (oracle/staffref), solved once per case."""
    if make.__name__ not in _oracle:
        from oracle import staffref
        c = make()
        p = c.oracle_problem(staffref)
        V, pol, _ = p.solve()
        _oracle[make.__name__] = (c, V, pol, [int(x) for x in p.x_lo])
    return _oracle[make.__name__]


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _staff_engine(sia, make=staff_cases.staff_planning_small, **changes):
    c = make()
    d = c.functor.to_desc(c.T)
    for k, v in changes.items():
        setattr(d, k, v)
    return sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len), c


def _call(lib, eng, K=None, seed=1, ini=0.0, ss="default", n_rules=None, results=True, k_null=False):
    from stochastic_inventory_amd._abi import SdpgpuSimResult
    T = eng.T
    k = np.asarray([2] * T if K is None else K, dtype=np.int32)
    if isinstance(ss, str):
        ss = np.tile(np.array([[3.0, 9.0]]), (1, T, 1))
    lev = None if ss is None else np.ascontiguousarray(ss, dtype=np.float64)
    nr = n_rules if n_rules is not None else (1 if lev is None else lev.shape[0])
    res = (SdpgpuSimResult * 64)()
    rc = lib.sdpgpu_staff_simulate(eng._h, None if k_null else _ip(k), seed, float(ini), None if lev is None else _dp(lev), nr,
                                   res if results else None, None, None, None)
    return rc, lib.sdpgpu_last_error(eng._h).decode()


# ---- the boundary ----------------------------------------------------------------------------------------------------------
def test_the_new_symbol_and_class_exist(sia, lib):
    header = open(os.path.join(ROOT, "include", "sdpgpu.h")).read()
    assert "sdpgpu_staff_simulate" in sia._abi.EXPORTS and hasattr(lib, "sdpgpu_staff_simulate") and "sdpgpu_staff_simulate(" in header
    assert "SimulatesS.java" in header and "not a variance" in header.replace("\n * ", " ").replace("  ", " ")
    assert lib.sdpgpu_abi_version() == 6  # additive
    assert hasattr(sia.SdpEngine, "staff_simulate") and sia.SimulatesS is sia.workforce.SimulatesS and "SimulatesS" in sia.__all__
    import inspect
    sig = inspect.signature(sia.SimulatesS.__init__).parameters
    assert list(sig)[1:] == ["recursion", "T", "dimissionRate", "seed"] and sig["seed"].default == 12345
    assert list(inspect.signature(sia.SimulatesS.simulatesS).parameters)[1:] == ["iniState", "optimalsS", "sampleNums"]
    assert list(inspect.signature(sia.SimulatesS.simulateTable).parameters)[1:] == ["iniState", "sampleNums"]


def test_refusals_come_before_any_device_call_and_name_the_argument(sia, lib):
    assert lib.sdpgpu_staff_simulate(None, None, 1, 0.0, None, 1, None, None, None, None) == ERR_ARG
    # not a STAFF handle
    w = cases.f1_small()
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        rc, err = _call(lib, eng)
        assert rc == ERR_UNSUPPORTED and "STAFF" in err
    # a rank of several
    eng, _ = _staff_engine(sia, world_size=2, rank=0)
    with eng:
        rc, err = _call(lib, eng)
        assert rc == ERR_STATE and "world_size 1" in err
    eng, c = _staff_engine(sia)
    with eng:
        T = eng.T
        rc, err = _call(lib, eng, k_null=True)
        assert rc == ERR_ARG and "sample_nums" in err
        rc, err = _call(lib, eng, results=False)
        assert rc == ERR_ARG and "results" in err
        # the tree
        for K, text in (([2, 0, 2], "sample_nums[1] = 0"), ([-3, 1, 1], "sample_nums[0] = -3"), ([4096, 4096, 2], "sample_nums"),
                        ([1 << 24, 2, 1], "sample_nums"), ([2147483647, 2147483647, 2147483647], "sample_nums")):
            rc, err = _call(lib, eng, K=K)
            assert rc == ERR_ARG and text in err, (K, err)
        # the number of rules
        for nr in (0, -1, 65):
            rc, err = _call(lib, eng, n_rules=nr)
            assert rc == ERR_ARG and f"n_rules = {nr}" in err
        rc, err = _call(lib, eng, ss=None, n_rules=2)
        assert rc == ERR_ARG and "n_rules = 2" in err
        # the levels
        good = np.tile(np.array([[3.0, 9.0]]), (2, T, 1))
        for bad, text in ((float("nan"), "not finite"), (float("inf"), "not finite"), (-float("inf"), "not finite"), (2147483648.0, "int32"),
                          (-2147483649.0, "int32"), (1e300, "int32")):
            for col in (0, 1):
                ss = good.copy()
                ss[1, 2, col] = bad
                rc, err = _call(lib, eng, ss=ss)
                assert rc == ERR_ARG and text in err and "ss[1][2]" in err, (bad, col, err)
        ss = good.copy()
        ss[0, 1] = (9.0, 7.0)  # S < s - 1: a negative hire at x = 8
        rc, err = _call(lib, eng, ss=ss)
        assert rc == ERR_ARG and "ss[0][1]" in err and "S < s - 1" in err
        ss[0, 1] = (9.9, 8.0)  # (int) 9.9 = 9: S = s - 1 hires nobody at x = 8 -- accepted, as are the extremes of int32
        ss[1, 0] = (-2147483648.9, 2147483647.9)
        assert _call(lib, eng, ss=ss)[0] in (OK, ERR_DEVICE)
        # the start
        for ini in (-1.0, 0.5, 2e9, float("nan")):
            rc, err = _call(lib, eng, ini=ini)
            assert rc == ERR_ARG and "ini_x" in err
        # the table rule: a start outside period 1's box is an argument error, a missing solve a state error
        rc, err = _call(lib, eng, ss=None, ini=31.0)
        assert rc == ERR_ARG and "ini_x = 31" in err and "period 1" in err
        rc, err = _call(lib, eng, ss=None, ini=30.0)
        assert rc == ERR_STATE and "nothing has been solved" in err
        # valid arguments of a level rule need no solve: only the device can be missing
        assert _call(lib, eng, K=[1 << 12, 1 << 12, 1])[0] in (OK, ERR_DEVICE)
    # an unclamped handle's period-1 box is the initial staff number alone
    eng, _ = _staff_engine(sia, staff_cases.staff_testing_small)
    with eng:
        rc, err = _call(lib, eng, ss=None, ini=1.0)
        assert rc == ERR_ARG and "period 1" in err
        assert _call(lib, eng, ss=None, ini=0.0)[0] == ERR_STATE
        assert _call(lib, eng, ini=7.0)[0] in (OK, ERR_DEVICE)  # (a level rule starts anywhere)


def test_a_missing_or_negative_level_pmf_is_refused(sia, lib):
    c = staff_cases.staff_planning_small()
    d = c.functor.to_desc(c.T)
    h = C.c_void_p()
    assert lib.sdpgpu_create(C.byref(d), C.byref(h)) == OK
    try:
        from stochastic_inventory_amd._abi import SdpgpuSimResult
        res = (SdpgpuSimResult * 1)()
        k = np.array([2, 2, 2], dtype=np.int32)
        ss = np.tile(np.array([[3.0, 9.0]]), (1, 3, 1))
        tab = np.ascontiguousarray(c.table[0])
        for t in (0, 2):
            assert lib.sdpgpu_set_level_pmf(h, t, _dp(tab), None, tab.shape[0], tab.shape[1]) == OK
        assert lib.sdpgpu_staff_simulate(h, _ip(k), 1, 0.0, _dp(ss), 1, res, None, None, None) == ERR_STATE
        assert b"level pmf of period 2" in lib.sdpgpu_last_error(h)
        neg = tab.copy()
        neg[5, 2] = -1e-9
        assert lib.sdpgpu_set_level_pmf(h, 1, _dp(neg), None, tab.shape[0], tab.shape[1]) == OK
        assert lib.sdpgpu_staff_simulate(h, _ip(k), 1, 0.0, _dp(ss), 1, res, None, None, None) == ERR_ARG
        err = lib.sdpgpu_last_error(h).decode()
        assert "period 2" in err and "negative" in err and "level 5" in err and "turnover 2" in err
    finally:
        lib.sdpgpu_destroy(h)


def test_valid_arguments_without_a_device_are_a_device_error(sia, lib):
    has_gpu = False
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        pass
    eng, c = _staff_engine(sia)
    with eng:
        rc, err = _call(lib, eng)
        assert rc == (OK if has_gpu else ERR_DEVICE) and (has_gpu or err != "")
        if not has_gpu:
            with pytest.raises(sia.SdpgpuError) as e:
                eng.staff_simulate([2, 2, 2], 1, 0, [[3, 9]] * 3)
            assert e.value.code == ERR_DEVICE
        with pytest.raises(ValueError):
            eng.staff_simulate([2, 2], 1, 0, [[3, 9]] * 3)
        with pytest.raises(ValueError):
            eng.staff_simulate([2, 2, 2], 1, 0, [[3, 9]] * 2)
    # the refusal text of the path simulations stays as it was: the new entry point is the door
    eng, _ = _staff_engine(sia)
    with eng:
        from stochastic_inventory_amd._abi import SdpgpuSimResult
        res = SdpgpuSimResult()
        assert lib.sdpgpu_simulate_sampled(eng._h, 5, 1, 0, 0, None, 0.0, 0.0, 0.0, C.byref(res), None, None) == ERR_UNSUPPORTED
        assert lib.sdpgpu_last_error(eng._h).decode().endswith(
            "the workforce drivers simulate an (s, S) rule with binomial draws (SimulatesS.java), not the table policy along demand paths")


# ---- the twin's self-checks ------------------------------------------------------------------------------------------------
def test_leaf_and_node_indexing_is_the_references_nested_loops():
    """K = (3, 2, 1): the sums and draws of the vectorised twin, read per leaf through n_t = p div stride_t, equal a literal
    restatement of SimulatesS.simulatesS's loops, whose arrays are indexed [t][i * K + j]."""
    c = staff_cases.staff_planning_small()
    P = st.Problem(c.functor, c.table, c.row_len)
    K, ss = (3, 2, 1), [[6, 14], [9.7, 12.2], [8, 8]]
    assert st.strides(K) == [2, 1, 1]
    node, child, parent = st.leaf_nodes(K)
    assert node.tolist() == [[0, 0, 0], [0, 1, 1], [1, 2, 2], [1, 3, 3], [2, 4, 4], [2, 5, 5]]
    assert child.tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0], [2, 0, 0], [2, 1, 0]]
    assert parent.tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 2], [0, 1, 3], [0, 2, 4], [0, 2, 5]]
    assert np.array_equal(parent[:, 1:], node[:, :-1])  # the parent index IS the node of the depth above
    for seed in (1, 20240607):
        r = st.simulate(P, K, seed, 2, ss=ss)
        end, dem = st.literal(P, K, seed, 2, ss)
        assert np.array_equal(r["sum"], end) and r["valid"].all()
        for t in range(3):
            assert r["demand"][:, t].tolist() == [dem[t][n] for n in node[:, t]]
        # the per-parent uniforms and the all-parents-at-once form are the same numbers
        for t, k in enumerate(K):
            n_par = int(np.prod(K[:t]))
            assert np.array_equal(st.node_uniforms(k, seed, t, n_par), st.node_uniforms_vec(k, seed, t, n_par))
    for k, n_par in ((1, 5), (10, 3), (63, 2), (64, 2), (65, 2), (17, 4)):
        assert np.array_equal(st.node_uniforms(k, 11, 3, n_par), st.node_uniforms_vec(k, 11, 3, n_par)), k


def test_one_child_draws_the_plain_uniform():
    """K = 1: one stratum, sigma is the identity on {0}, u = a -- the 53 bits of Philox at (0, t, i, 0)."""
    seed = 99
    for t, i in ((0, 0), (2, 7), (5, 1234)):
        w = tw.philox4x32_10((0, t, i, 0), tw._key(seed))
        a = float(((w[0] << 32) | w[1]) >> 11) * 2.0 ** -53
        assert st.node_uniforms(1, seed, t, i + 1)[i, 0] == a and st.node_uniforms_vec(1, seed, t, i + 1)[i, 0] == a


def test_nobody_to_leave_draws_zero():
    """hireTo <= 0 (SimulatesS.java:64-67): a rule that never hires from ini = 0 -- every draw is 0 and a leaf's sum is the
    penalties alone."""
    c = staff_cases.staff_testing_small()
    P = st.Problem(c.functor, c.table, c.row_len)
    r = st.simulate(P, (2, 3, 1, 2), 5, 0, ss=[[0, 0]] * 4)
    assert not r["demand"].any() and r["valid"].all()
    assert set(r["sum"].tolist()) == {250.0 * (4 + 9 + 6 + 3)}


def test_levels_beyond_the_table_use_its_last_row():
    """staff_testing_small: 13 rows, no clamp.  S = 20 > 12: the draws come from row 12 (at most 12 leave) although 20 are
    employed, and equal the count over that row's thresholds."""
    c = staff_cases.staff_testing_small()
    P = st.Problem(c.functor, c.table, c.row_len)
    K = (17, 4, 2, 1)
    r = st.simulate(P, K, 3, 0, ss=[[20, 20]] * 4)
    assert r["demand"].max() <= 12 and r["demand"].min() >= 0
    u0 = st.node_uniforms(17, 3, 0, 1)[0]
    thr = np.cumsum(c.table[0][12])
    want = [(thr[:12] <= u).sum() for u in u0]
    assert r["demand"][:: 8, 0].tolist() == want
    assert st.turnover(P, 0, np.array([12, 13, 20, 500]), np.full(4, 0.77)).tolist() == [int((thr[:12] <= 0.77).sum())] * 4
    # u at and next to a threshold: c_q <= u counts the threshold itself
    q = 4
    assert st.turnover(P, 0, np.array([12, 12]), np.array([thr[q], np.nextafter(thr[q], 0.0)])).tolist() == [q + 1, q]


def test_short_rows_end_at_row_len():
    """staff_short_rows: rows of at most 6 entries -- at most 5 leave whatever u is, the last threshold being +infinity."""
    c = staff_cases.staff_short_rows()
    P = st.Problem(c.functor, c.table, c.row_len)
    r = st.simulate(P, (10, 10, 1), 8, 2, ss=[[20, 24]] * 3)
    assert r["demand"].max() == 5
    one = np.nextafter(1.0, 0.0)
    assert st.turnover(P, 0, np.array([24, 3, 1, 0]), np.full(4, one)).tolist() == [5, 3, 1, 0]


def test_levels_truncate_like_java():
    assert st.trunc_levels([[3.9, -3.9], [-0.5, 2147483647.9]]).tolist() == [[3, -3], [0, 2147483647]]


# ---- the estimate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", UNBIASED_CASES, ids=lambda f: f.__name__)
def test_the_twin_is_unbiased_under_the_oracles_policy(make):
    """Table rule with the oracle's policy: the turnover is drawn from the very rows the recursion integrates over, so the mean of
    the leaf sums estimates V_1(ini) without bias."""
    c, V, pol, x_lo = oracle_tables(make)
    P = st.Problem(c.functor, c.table, c.row_len)
    ini = c.functor.iniStaffNum
    v1 = float(V[0][ini - x_lo[0]])
    means = []
    for seed in UNBIASED_SEEDS:
        r = st.simulate(P, UNBIASED_TREE, seed, ini, policy=pol, x_lo=x_lo)
        assert r["valid"].all()
        means.append(math.fsum(r["sum"].tolist()) / len(r["sum"]))
    holds, text = unbiased(means, v1)
    print(c.name, text)
    assert holds, text
