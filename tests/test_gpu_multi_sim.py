"""The two-product rollout on the GPU (sdpgpu_multi_policy_*; DESIGN 4 "Two-product rollout"): the hash table over the memo
(every row found, perturbed states not, at the automatic and at the tightest capacity), the rollout along EVERY support path of
the 50 instances of tests/test_multi_sim_twin.py bit for bit against the host twin over the ORACLE's memo, the reduction's
shapes, the sampled rollout against its own draws, off-support demands, duplicate rows, the driver's own instance, and the
simulator mirror.  The reference sums (tests/multi_sim_cases.reference) are computed once and shared."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_sim_cases as cases  # noqa: E402
import multi_sim_twin as twin  # noqa: E402
import multicash_cases  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 4
FAMILIES = ["mc-13", "xr-7", "kat1"]  # one instance per family (324, 486 and 81 support paths)

_SOLVED = {}


def solved(sia, cid):
    """The GPU solve of a case with its memo, once per session."""
    if cid not in _SOLVED:
        r = cases.solve(sia, cid)
        r.table.setflags(write=False)
        _SOLVED[cid] = r
    return _SOLVED[cid]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return bits(a).shape == bits(b).shape and (bits(a) == bits(b)).all()


def tight_log2(n):
    """The smallest k with 2^k > n: the fullest table create accepts."""
    return max(1, int(n).bit_length())


# ---- lookup ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", ["auto", "tight"])
@pytest.mark.parametrize("cid", ["mc-10", "xr-1", "kat1"])
def test_every_row_is_found_and_perturbed_states_are_not(sia, cid, capacity):
    rows = solved(sia, cid).table
    n, T = len(rows), cases.case(cid)[1]["T"]
    memo = twin.memo_dict(rows)
    k = 0 if capacity == "auto" else tight_log2(n)
    if capacity == "tight":
        assert (1 << k) > n >= (1 << (k - 1))  # more than half full: long chains, and they wrap at the table's end
    with cases.policy(sia, cid, rows, k) as pol:
        per = rows[:, 0].astype(np.int32)
        cols = [rows[:, c] for c in range(1, 6)]
        a1, a2, found = pol.lookup(per, *cols)
        assert found.all()
        assert (a1 == rows[:, 7]).all() and (a2 == rows[:, 8]).all()
        # the cash field moved by a quarter, the period moved by one (T + 1 and 0 included): what the memo itself says
        for what in ("cash", "period+", "period-"):
            p2, c2 = per.copy(), [c.copy() for c in cols]
            if what == "cash":
                c2[4] = c2[4] + 0.25
            else:
                p2 = p2 + (1 if what == "period+" else -1)
            want = np.array([(int(p), float(a), float(b), float(c), float(d), float(e)) in memo for p, a, b, c, d, e in zip(p2, *c2)])
            assert not want.all(), what  # (a state moved past period T or before period 1 is no state of the memo)
            if what == "cash" and cid != "kat1":
                assert not want.any()  # (the lattice families' states are whole numbers)
            b1, b2, f2 = pol.lookup(p2, *c2)
            assert (f2 == want).all(), what
            hit = np.flatnonzero(want)
            for i in hit:
                assert (b1[i], b2[i]) == memo[(int(p2[i]),) + tuple(float(c[i]) for c in c2)]


def test_lookup_of_nothing_and_argument_errors(sia):
    rows = solved(sia, "mc-0").table
    lib = sia._abi.load()
    with cases.policy(sia, "mc-0", rows) as pol:
        a1, a2, found = pol.lookup([], [], [], [], [], [])
        assert len(a1) == len(a2) == len(found) == 0
        assert lib.sdpgpu_multi_policy_lookup(pol._h, -1, None, None, None, None, None, None, None, None, None) == ERR_ARG
        assert "n = -1" in lib.sdpgpu_multilead_last_error().decode()
        assert lib.sdpgpu_multi_policy_lookup(pol._h, 3, None, None, None, None, None, None, None, None, None) == ERR_ARG
        assert "null argument" in lib.sdpgpu_multilead_last_error().decode()


# ---- explicit paths ----------------------------------------------------------------------------------------------------------
def check_support_paths(sia, oracle, cid, rows, final_value):
    ref = cases.reference(oracle, cid)
    with cases.policy(sia, cid, rows) as pol:
        res, sums, valid = pol.simulate(ref["d1"], ref["d2"], discount=cases.discount_weights(ref["kw"]))
    n = len(ref["prob"])
    assert valid.all() and res.n_valid == res.n_paths == n
    assert same_bits(sums, ref["sums"])
    v1 = final_value - float(ref["kw"]["ini_cash"])
    est = math.fsum(float(p) * float(s) for p, s in zip(ref["prob"], sums))
    err = abs(est - v1) / max(1.0, abs(v1))
    print(f"{cid}: {n} paths, identity against the GPU's final value {err:.3g}")
    assert err <= 1e-12
    return res, sums


@pytest.mark.parametrize("cid", cases.ALL)
def test_all_support_paths_equal_the_twin_over_the_oracles_memo(sia, oracle, cid):
    r = solved(sia, cid)
    check_support_paths(sia, oracle, cid, r.table, r.finalValue)


@pytest.mark.parametrize("cid", ["mc-0", "xr-0", "kat1"])
def test_policy_built_from_the_oracles_memo_rows(sia, oracle, cid):
    ref = cases.reference(oracle, cid)
    check_support_paths(sia, oracle, cid, ref["rows"], solved(sia, cid).finalValue)


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", FAMILIES + cases.ONE_PERIOD + ["xr-11", "xr-14", "xr-21", "xr-23"])
def test_path_counts_around_the_wave_and_the_fixed_order_reduction(sia, oracle, cid):
    ref = cases.reference(oracle, cid)
    disc = cases.discount_weights(ref["kw"])
    with cases.policy(sia, cid, solved(sia, cid).table) as pol:
        for n in (1, 63, 64, 65, 257):
            idx = np.resize(np.arange(len(ref["prob"])), n)  # the support paths, repeated
            d1, d2 = ref["d1"][idx], ref["d2"][idx]
            res, sums, valid = pol.simulate(d1, d2, discount=disc)
            assert valid.all() and (res.n_paths, res.n_valid, res.n_lost) == (n, n, 0)
            assert same_bits(sums, ref["sums"][idx])
            res2, sums2, _ = pol.simulate(d1, d2, discount=disc)
            assert same_bits([res.mean, res.m2], [res2.mean, res2.m2]) and same_bits(sums, sums2)
            want = math.fsum(sums.tolist()) / n
            assert abs(res.mean - want) <= 1e-12 * max(1.0, abs(want)), (n, res.mean, want)
            assert res.m2 >= 0.0 and (n > 1 or res.m2 == 0.0)
        # NULL weights are the bits of an explicit array of ones
        res, sums, _ = pol.simulate(ref["d1"], ref["d2"])
        res1, sums1, _ = pol.simulate(ref["d1"], ref["d2"], discount=np.ones(ref["kw"]["T"]))
        assert same_bits(sums, sums1) and same_bits([res.mean, res.m2], [res1.mean, res1.m2])


# ---- sampled -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["lhs", "random"])
@pytest.mark.parametrize("cid", FAMILIES)
def test_sampled_rollout_equals_the_rollout_of_its_own_draws(sia, oracle, cid, mode):
    kind, kw, dep = cases.case(cid)
    T = kw["T"]
    tl = twin.tiles(kind, kw)
    disc = cases.discount_weights(kw)
    with cases.policy(sia, cid, solved(sia, cid).table) as pol:
        for n, seed in ((257, 5), (1000, 20240611)):
            d1, d2, u = pol.sample(n, seed, mode=mode)
            assert ((u >= 0) & (u < 1)).all()
            for t in range(T):
                q = np.searchsorted(np.cumsum(tl[t][:, 2])[:-1], u[:, t], side="right")
                assert (d1[:, t] == tl[t][q, 0]).all() and (d2[:, t] == tl[t][q, 1]).all(), t
                if mode == "lhs":
                    assert sorted(np.floor(u[:, t] * n).astype(np.int64).tolist()) == list(range(n)), t
            res, sums, valid = pol.simulate_sampled(n, seed, mode=mode, discount=disc, want_sums=True)
            res_g, sums_g, valid_g = pol.simulate(d1, d2, discount=disc)
            assert valid.all() and valid_g.all() and res.n_valid == n
            assert same_bits(sums, sums_g) and same_bits([res.mean, res.m2], [res_g.mean, res_g.m2])
            # the draws never leave the memo, and the twin over the read-back memo walks them to the same sums
            tw, tv = twin.rollout(kind, kw, twin.memo_dict(solved(sia, cid).table), d1[:64], d2[:64], disc, dep)
            assert tv.all() and same_bits(sums[:64], tw)
            res2 = pol.simulate_sampled(n, seed, mode=mode, discount=disc)
            assert same_bits([res.mean, res.m2], [res2.mean, res2.m2])
        if mode == "random":
            a, b = 100, 157
            whole = pol.sample(a + b, 9, mode="random")
            first = pol.sample(a, 9, mode="random")
            second = pol.sample(b, 9, mode="random", first_path=a)
            for w, f, s in zip(whole, first, second):
                assert same_bits(w, np.concatenate([f, s]))
            _, s_whole, _ = pol.simulate_sampled(a + b, 9, mode="random", want_sums=True)
            _, s_second, _ = pol.simulate_sampled(b, 9, mode="random", first_path=a, want_sums=True)
            assert same_bits(s_whole[a:], s_second)


def test_simulate_refusals_name_the_argument(sia):
    from stochastic_inventory_amd._abi import SdpgpuSimResult
    lib = sia._abi.load()
    kind, kw, _ = cases.case("mc-0")
    T = kw["T"]
    res = SdpgpuSimResult()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    d = np.ones((4, T))
    bad, nan_disc = d.copy(), np.ones(T)
    bad[2, 1] = np.inf
    nan_disc[T - 1] = np.nan
    with cases.policy(sia, "mc-0", solved(sia, "mc-0").table) as pol:
        def err():
            return lib.sdpgpu_multilead_last_error().decode()
        for n, code in ((0, ERR_ARG), (-3, ERR_ARG), ((1 << 24) + 1, ERR_UNSUPPORTED)):
            assert lib.sdpgpu_multi_policy_simulate_sampled(pol._h, n, 1, 0, 0, None, C.byref(res), None, None) == code and "n_paths" in err()
            assert lib.sdpgpu_multi_policy_sample(pol._h, n, 1, 0, 0, dp(d), dp(d), None) == code and "n_paths" in err()
            assert lib.sdpgpu_multi_policy_simulate(pol._h, n, dp(d), dp(d), None, C.byref(res), None, None) == code and "n_paths" in err()
        assert lib.sdpgpu_multi_policy_simulate_sampled(pol._h, 4, 1, 2, 0, None, C.byref(res), None, None) == ERR_ARG and "mode = 2" in err()
        assert lib.sdpgpu_multi_policy_simulate_sampled(pol._h, 4, 1, 0, 7, None, C.byref(res), None, None) == ERR_ARG and "first_path = 7" in err()
        assert lib.sdpgpu_multi_policy_sample(pol._h, 4, 1, 0, 7, dp(d), dp(d), None) == ERR_ARG and "first_path = 7" in err()
        assert lib.sdpgpu_multi_policy_sample(pol._h, 4, 1, 0, 0, None, dp(d), None) == ERR_ARG and "out_d1" in err()
        assert lib.sdpgpu_multi_policy_simulate_sampled(pol._h, 4, 1, 0, 0, None, None, None, None) == ERR_ARG and "result is null" in err()
        assert lib.sdpgpu_multi_policy_simulate_sampled(pol._h, 4, 1, 0, 0, dp(nan_disc), C.byref(res), None, None) == ERR_ARG
        assert f"discount[{T - 1}]" in err()
        assert lib.sdpgpu_multi_policy_simulate(pol._h, 4, None, dp(d), None, C.byref(res), None, None) == ERR_ARG and "d1" in err()
        assert lib.sdpgpu_multi_policy_simulate(pol._h, 4, dp(d), dp(bad), None, C.byref(res), None, None) == ERR_ARG and "d2[2][1]" in err()
        with pytest.raises(ValueError):
            pol.simulate(np.ones((4, T + 1)), np.ones((4, T + 1)))
        with pytest.raises(ValueError):
            pol.simulate_sampled(4, 1, mode="sobol")
        # the object still works after the refusals
        assert lib.sdpgpu_multi_policy_simulate_sampled(pol._h, 4, 1, 0, 0, None, C.byref(res), None, None) == OK and res.n_valid == 4


# ---- off-support demand --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["mc-0", "xr-0", "kat1-stocked"])
def test_a_demand_outside_the_support_ends_the_path(sia, oracle, cid):
    ref = cases.reference(oracle, cid)
    kind, kw, dep = ref["kind"], ref["kw"], ref["dep"]
    disc = cases.discount_weights(kw)
    tl = twin.tiles(kind, kw)
    n, where = 70, 66  # (the path sits in the second wave)
    idx = np.resize(np.arange(len(ref["prob"])), n)
    d1, d2 = np.array(ref["d1"][idx]), np.array(ref["d2"][idx])
    d1[where], d2[where] = ref["d1"][0], ref["d2"][0]
    d1[where, 0], d2[where, 0] = tl[0][:, 0].max() + 1, tl[0][:, 1].max() + 1
    t_sums, t_valid = twin.rollout(kind, kw, twin.memo_dict(ref["rows"]), d1, d2, disc, dep)
    assert not t_valid[where] and t_valid.sum() == n - 1 and math.isnan(t_sums[where])  # the twin misses on it, and only on it
    with cases.policy(sia, cid, solved(sia, cid).table) as pol:
        res, sums, valid = pol.simulate(d1, d2, discount=disc)
        assert (valid.astype(bool) == t_valid).all()
        assert same_bits(np.delete(sums, where), np.delete(t_sums, where)) and math.isnan(sums[where])
        assert (res.n_paths, res.n_valid) == (n, n - 1)
        assert math.isnan(res.mean) and math.isnan(res.m2)
        # the next call on the same object is whole again
        res, sums, valid = pol.simulate(ref["d1"][idx], ref["d2"][idx], discount=disc)
        assert valid.all() and res.n_valid == n and not math.isnan(res.mean) and not math.isnan(res.m2)


# ---- duplicates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", FAMILIES)
def test_a_repeated_row_is_kept_once_and_a_contradicting_one_is_refused(sia, oracle, cid):
    ref = cases.reference(oracle, cid)
    kind, kw, _ = cases.case(cid)
    rows = solved(sia, cid).table
    disc = cases.discount_weights(kw)
    n = len(rows)
    src = n // 2  # a row of a later period, once more near the front
    assert rows[src, 0] > 1 and src > 5
    twice = np.concatenate([rows[:5], rows[src:src + 1], rows[5:]])  # the two copies: rows 5 and src + 1
    for k in (0, tight_log2(len(twice))):
        with cases.policy(sia, cid, twice, k) as pol:
            res, sums, valid = pol.simulate(ref["d1"], ref["d2"], discount=disc)
            assert valid.all() and same_bits(sums, ref["sums"])
            a1, a2, found = pol.lookup(rows[:, 0].astype(np.int32), *[rows[:, c] for c in range(1, 6)])
            assert found.all() and (a1 == rows[:, 7]).all() and (a2 == rows[:, 8]).all()
    other = twice.copy()
    qb = kw["q_bound"]
    base = int(other[5, 2]) if kind == "multixr" else 0  # (the XR family's second level counts from (int) x2)
    other[5, 8] = other[5, 8] + 1 if other[5, 8] - base + 1 < qb else other[5, 8] - 1
    with pytest.raises(sia.SdpgpuError) as e:
        cases.policy(sia, cid, other)
    assert e.value.code == ERR_ARG
    assert f"memo rows 5 and {src + 1} hold the same state" in str(e.value) and "different actions" in str(e.value)


# ---- the driver's own instance -------------------------------------------------------------------------------------------------
def test_multiitemcashxr_main_rolls_ten_thousand_paths(sia):
    """MultiItemCashXR.main (T = 2, Qbound 50, 352 demand pairs a period): 71 767 period-2 states in the table."""
    from stochastic_inventory_amd.multiitem import MultiPolicy, multixr_solve
    golden = json.load(open(os.path.join(HERE, "golden", "multixr_main.json")))
    kw = multicash_cases.xr_main_instance()
    r = multixr_solve(0.0, table=True, **kw)
    assert r.finalValue == golden["final_value"] and r.statesPerPeriod == [1, 71767] and len(r.table) == 71768
    n = 10000
    with MultiPolicy("multixr", r.table, **kw) as pol:
        res, sums, valid = pol.simulate_sampled(n, 2024, mode="lhs", want_sums=True)
        d1n, d2n, _ = pol.sample(n, 2024, mode="lhs")
    assert valid.all() and (res.n_paths, res.n_valid) == (n, n)
    tw, tv = twin.rollout("multixr", kw, twin.memo_dict(r.table), d1n[:64], d2n[:64], [1.0, 1.0])
    assert tv.all() and same_bits(sums[:64], tw)
    se = math.sqrt(res.m2 / n) / math.sqrt(n)
    # (not asserted: GetPmfMulti's truncated Poisson tile does not sum to 1, so the recursion's value is no expectation under the
    # distribution the tile's running sum draws from -- DESIGN 4, "Two-product rollout")
    print(f"tile sums {[float(np.sum(np.asarray(t)[:, 2])) for t in kw['pmf']]}")
    print(f"MultiItemCashXR.main: mean + iniR = {res.mean + kw['ini_cash']!r}, final value {golden['final_value']!r}, "
          f"{abs(res.mean + kw['ini_cash'] - golden['final_value']) / se:.2f} standard errors ({se:.4g}) apart, kernels {res.kernel_ms:.3f} ms")


# ---- the mirror ----------------------------------------------------------------------------------------------------------------
def test_the_simulator_mirrors_return_the_mean_plus_the_start(sia):
    from stochastic_inventory_amd import multiitem
    dep, kw = multicash_cases.xr_random_instance(1)
    functor = {k: v for k, v in kw.items() if k not in ("pmf", "ini_cash", "ini_i1", "ini_i2", "T", "discount")}
    functor["depositeRate"] = dep
    rec = multiitem.CashRecursionMultiXR(kw["discount"], kw["pmf"], TLength=kw["T"], functor=functor)
    ini = multiitem.CashStateMultiXR(1, kw["ini_i1"], kw["ini_i2"], kw["ini_cash"])
    sim = multiitem.CashSimulationMultiXR(500, None, kw["discount"], rec, seed=3)
    got = sim.simulateSDPGivenSamplNum(ini)
    assert sim.last_result.n_valid == 500 and got == sim.last_result.mean + ini.iniR
    with rec.policy() as pol:
        want = pol.simulate_sampled(500, 3, discount=[kw["discount"] ** t for t in range(kw["T"])])
    assert same_bits([want.mean, want.m2], [sim.last_result.mean, sim.last_result.m2])
    sim.setSampleNum(64)
    sim.simulateSDPGivenSamplNum(ini)
    assert sim.last_result.n_paths == 64
    # CashSimulationMulti over CashRecursionMulti: both of the reference's method names
    kw = multicash_cases.random_instance(0)
    functor = {k: v for k, v in kw.items() if k not in ("pmf", "ini_cash", "ini_i1", "ini_i2", "T", "discount")}
    rec = multiitem.CashRecursionMulti(kw["discount"], kw["pmf"], TLength=kw["T"], functor=functor)
    ini = multiitem.CashStateMulti(1, kw["ini_i1"], kw["ini_i2"], kw["ini_cash"])
    sim = multiitem.CashSimulationMulti(300, None, kw["discount"], rec, seed=11)
    a = sim.simulateSDPGivenSamplNum(ini)
    assert a == sim.last_result.mean + ini.iniCash and sim.last_result.n_valid == 300
    assert sim.simulateSDPGivenSamplNumMulti(ini) == a
    # within a few standard errors of the value the recursion computed (not a bound on the sampler: a sanity print)
    se = math.sqrt(sim.last_result.m2 / 300) / math.sqrt(300)
    print(f"CashSimulationMulti: {a!r} against {rec.getExpectedValue(ini) + ini.iniCash!r}, standard error {se:.4g}")
