"""Cash rule rollout (sdpgpu_cash_rule_simulate, SdpEngine.cash_rule_simulate, simulation.CashSimulation; DESIGN 4 "Cash rule
rollout") as far as it goes without a GPU: the new symbol and class, every refusal with a text naming the argument BEFORE any
device call, the host twin (tests/cash_rule_twin.py) on hand-computed two-period examples of each form, the packing of the
reference's maps into dense tables, and the COVERAGE CONDITION: on the cases, sizes and rules tests/test_gpu_cash_rule.py uses,
the twin's trace shows every branch of the definition at least once per form it applies to."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
import cash_rule_twin as ct  # noqa: E402
from test_simulate_sampled_host import LHS, RANDOM, tile_demands, twin_sample  # noqa: E402

OK, ERR_ARG, ERR_STATE, ERR_DEVICE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

# ---- what the GPU test runs (shared with tests/test_gpu_cash_rule.py) ------------------------------------------------------
SEED = 20240607
CASES = (cases.f3_testing, cases.f3_tenths, cases.f3_min_gamma, cases.f3_dyadic)
# one lane; a wave boundary (63, 64, 65); two waves in one workgroup (65 .. 128 paths); a second workgroup (more than 256)
NS = (1, 63, 64, 65, 257, 1025)
MIXED_FORMS = (ct.SC12S, ct.SC1S, ct.SMEANCS, ct.SC12S, ct.SC1S)


class Setup:
    """One case with its five rules (forms 0, 1, 2, 0, 1), the reference's four scalars and the twin's problem record.

    The rules are fractional, so that the order and the inventory leave the grid; they sit around the mean demand, the
    thresholds around the cash a path typically holds, so that every branch is taken:
      * s_t = mean demand of period t + 1.5, S_t = s_t + 2.75 (rules 3 and 4: s_t + 1, S_t + 1.5);
      * C1(x) = lo + 0.5 ix on every second grid point from ix = 0 (absent: odd ix), C2(x) = hi - 0.25 ix where ix mod 3 != 1;
        lo / hi = the cash the case starts with -/+ the price of its mean first-period demand, so paths fall on either side;
      * rule 3 (form 0) has no entry in either table (all NaN): every lookup misses, the defaults 0 and 10000 rule;
      * form 2's own C = the start cash;
      * the scalars are the case's own costs: minCashRequired = its first overhead, maxQ = half its order limit (so that the cap
        binds in some periods), fixOrderCost and variCost as the functor's."""

    def __init__(self, make):
        self.w = w = make()
        f = self.f = w.functor
        self.T = T = w.T
        self.P = ct.Problem(f, T)
        self.disc = np.array([math.pow(f.discountFactor, t) for t in range(T)])
        self.ini = (float(f.iniInventory), float(f.iniCash))
        means = [float(np.dot(tile[:, 0], tile[:, 1])) for tile in w.pmf]
        oh = f.overheadCosts[0] if f.overheadCosts is not None else f.overheadCost
        self.scalars = dict(min_cash_required=float(oh), max_q=float(f.maxOrderQuantity) / 2.0, fix_order_cost=float(f.fixOrderCost),
                            vari_cost=float(f.variCost))
        nx = self.P.nx
        lo, hi = f.iniCash - f.price * means[0], f.iniCash + f.price * means[0]
        rules = np.zeros((5, T, 4))
        c1 = np.full((5, T, nx), NAN)
        c2 = np.full((5, T, nx), NAN)
        for r in range(5):
            for t in range(T):
                s = means[t] + 1.5 + (1.0 if r >= 3 else 0.0)
                rules[r, t] = (s, f.iniCash, 0.0, s + 2.75 + (1.5 if r >= 3 else 0.0))
            if r != 3:
                for ix in range(nx):
                    if ix % 2 == 0:
                        c1[r, :, ix] = lo + 0.5 * ix
                    if ix % 3 != 1:
                        c2[r, :, ix] = hi - 0.25 * ix
        self.forms = np.array(MIXED_FORMS, dtype=np.int32)
        self.rules, self.c1, self.c2 = rules, c1, c2
        self.draw = [lambda u, tile=tile: tile_demands(tile, u) for tile in w.pmf]

    def cache(self, tab, r):
        """Rule r's rows of a dense table as the reference's map {(period, x): value}."""
        return {(t + 1, self.P.key(ix)): float(tab[r, t, ix]) for t in range(self.T) for ix in range(self.P.nx) if not math.isnan(tab[r, t, ix])}

    def rule_tuples(self):
        """The five rules as CashSimulation.simulateRules takes them: maps for the tables, the reference's three columns [s, C, S]
        for rules 1 and 2 (rule 3 brings no map: every key absent)."""
        return [(0, self.rules[0], self.cache(self.c1, 0), self.cache(self.c2, 0)), (1, self.rules[1][:, [0, 1, 3]], self.cache(self.c1, 1)),
                (2, self.rules[2][:, [0, 1, 3]]), (0, self.rules[3]), (1, self.rules[4], self.cache(self.c1, 4))]

    def args(self):
        s = self.scalars
        return s["min_cash_required"], s["max_q"], s["fix_order_cost"], s["vari_cost"]


_setup, _ref = {}, {}


def setup_of(make):
    if make.__name__ not in _setup:
        _setup[make.__name__] = Setup(make)
    return _setup[make.__name__]


def reference(make, n, mode=LHS, first_path=0, ini=None):
    """(demands, twin result of the five rules) on the twin sampler's demands -- the demands sdpgpu_sample_demands returns
    (tests/test_gpu_simulate_sampled.py; the GPU test asserts it again before it compares).  Computed once, shared."""
    key = (make.__name__, n, mode, first_path, ini)
    if key not in _ref:
        s = setup_of(make)
        dem, _ = twin_sample(n, SEED, mode, first_path, s.draw)
        x, cash = s.ini if ini is None else ini
        _ref[key] = (dem, ct.simulate(s.P, dem, s.disc, x, cash, s.forms, s.rules, s.c1, s.c2, *s.args()))
    return _ref[key]


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _engine(sia, make=cases.f3_testing, **changes):
    w = make()
    d = w.desc()
    for k, v in changes.items():
        setattr(d, k, v)
    return sia.SdpEngine(d, w.pmf, w.overhead()), w


def _call(lib, eng, n=5, seed=1, mode=LHS, first_path=0, ini=(0.0, 10.0), forms=(0,), rules="default", c1=None, c2=None,
          scalars=(1.0, 5.0, 2.0, 1.0), n_rules=None, null=()):
    from stochastic_inventory_amd._abi import SdpgpuSimResult
    T = eng.T
    fm = np.asarray(forms, dtype=np.int32)
    if isinstance(rules, str):
        rules = np.tile(np.array([[4.5, 3.0, 50.0, 8.25]]), (len(fm), T, 1))
    rules = np.ascontiguousarray(rules, dtype=np.float64)
    nr = len(fm) if n_rules is None else n_rules
    res = (SdpgpuSimResult * 32)()
    rc = lib.sdpgpu_cash_rule_simulate(
        eng._h, n, seed, mode, first_path, None, float(ini[0]), float(ini[1]), nr, None if "form" in null else fm.ctypes.data_as(C.POINTER(C.c_int32)),
        None if "rule" in null else _dp(rules), _dp(c1), _dp(c2), *[float(v) for v in scalars], None if "results" in null else res, None)
    return rc, lib.sdpgpu_last_error(eng._h).decode()


# ---- the boundary ----------------------------------------------------------------------------------------------------------
def test_the_new_symbol_and_class_exist(sia, lib):
    header = open(os.path.join(ROOT, "include", "sdpgpu.h")).read()
    name = "sdpgpu_cash_rule_simulate"
    assert name in sia._abi.EXPORTS and hasattr(lib, name) and name + "(" in header
    for macro, v in (("SDPGPU_RULE_SC12S", 0), ("SDPGPU_RULE_SC1S", 1), ("SDPGPU_RULE_SMEANCS", 2)):
        assert f"#define {macro} {v}" in header
    assert (sia._abi.RULE_SC12S, sia._abi.RULE_SC1S, sia._abi.RULE_SMEANCS) == (0, 1, 2)
    assert "CashSimulation.java:996-1042" in header and "Cash rule rollout" in header
    assert lib.sdpgpu_abi_version() == 6  # additive
    assert len(sia._abi.EXPORTS[name][1]) == 19
    assert hasattr(sia.SdpEngine, "cash_rule_simulate")
    from stochastic_inventory_amd import simulation
    assert sia.CashSimulation is simulation.CashSimulation and "CashSimulation" in sia.__all__
    assert issubclass(simulation.CashSimulation, simulation.Simulation)
    import inspect
    sig = inspect.signature(simulation.CashSimulation.__init__).parameters
    assert list(sig)[1:5] == ["distributions", "sampleNum", "recursion", "discountFactor"] and sig["sampler"].default == "device"
    assert list(inspect.signature(simulation.CashSimulation.simulatesMeanCS).parameters)[1:] == [
        "iniState", "optsCS", "minCashRequired", "maxQ", "fixOrderCost", "variCost"]
    assert list(inspect.signature(simulation.CashSimulation.simulatesCS).parameters)[1:4] == ["iniState", "optsCS", "cacheC1Values"]
    assert list(inspect.signature(simulation.CashSimulation.simulateRules).parameters)[1:3] == ["iniState", "rules"]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**Cash rule rollout:" in design


def test_refusals_come_before_any_device_call_and_name_the_argument(sia, lib):
    from stochastic_inventory_amd._abi import SdpgpuSimResult
    assert lib.sdpgpu_cash_rule_simulate(None, 5, 1, 0, 0, None, 0.0, 0.0, 1, None, None, None, None, 0.0, 1.0, 0.0, 1.0, None, None) == ERR_ARG
    # ERR_UNSUPPORTED: not a CASH handle (F1, and the other families with a cash axis); cash_formula 2; a user functor
    for make in (cases.f1_small, cases.f4_overdraft, cases.f6_survival):
        eng, _ = _engine(sia, make)
        with eng:
            rc, err = _call(lib, eng)
            assert rc == ERR_UNSUPPORTED and "CASH handle" in err, (make.__name__, err)
    eng, _ = _engine(sia, cases.f3_xr)
    with eng:
        rc, err = _call(lib, eng)
        assert rc == ERR_UNSUPPORTED and "cash_formula 2" in err
    import custom_sources
    w = cases.f1_small()
    f = w.functor
    prm = [f.fixedOrderingCost, f.variOrderingCost, f.holdingCost, f.penaltyCost, f.minInventory, f.maxInventory, f.maxOrderQuantity]
    with sia.SdpEngine(w.desc(), w.pmf, None, custom_source=custom_sources.BACKORDER, custom_params=prm) as eng:
        rc, err = _call(lib, eng)
        assert rc == ERR_UNSUPPORTED and "user functor" in err
    # ERR_STATE: a rank of several
    eng, _ = _engine(sia, world_size=2, rank=0)
    with eng:
        rc, err = _call(lib, eng)
        assert rc == ERR_STATE and "world_size 1" in err
    eng, _ = _engine(sia)
    with eng:
        T, nx = eng.T, eng.rule_table_points()
        assert nx == 21
        # n_paths above 2^24 is a limit of the build, not a bad argument
        rc, err = _call(lib, eng, n=(1 << 24) + 1)
        assert rc == ERR_UNSUPPORTED and "n_paths" in err and str(1 << 24) in err
        for n in (0, -4):
            rc, err = _call(lib, eng, n=n)
            assert rc == ERR_ARG and f"n_paths = {n}" in err
        rc, err = _call(lib, eng, mode=2)
        assert rc == ERR_ARG and "mode = 2" in err
        rc, err = _call(lib, eng, mode=LHS, first_path=7)
        assert rc == ERR_ARG and "first_path = 7" in err
        assert _call(lib, eng, mode=RANDOM, first_path=(1 << 33) + 7)[0] in (OK, ERR_DEVICE)
        for nr in (0, -1, 17):
            rc, err = _call(lib, eng, forms=[0] * 17, n_rules=nr)
            assert rc == ERR_ARG and f"n_rules = {nr}" in err
        assert _call(lib, eng, forms=[0, 1, 2] * 5 + [0])[0] in (OK, ERR_DEVICE)  # 16 rules
        for bad in (-1, 3, 99):
            rc, err = _call(lib, eng, forms=[0, bad])
            assert rc == ERR_ARG and f"form[1] = {bad}" in err
        for what in ("form", "rule", "results"):
            rc, err = _call(lib, eng, null=(what,))
            assert rc == ERR_ARG and f"{what} is null" in err
        good = np.tile(np.array([[4.5, 3.0, 50.0, 8.25]]), (2, T, 1))
        for bad in (NAN, float("inf"), -float("inf")):
            for col in range(4):
                rules = good.copy()
                rules[1, 2, col] = bad
                rc, err = _call(lib, eng, forms=[0, 2], rules=rules)
                assert rc == ERR_ARG and f"rule[1][2][{col}]" in err and "not finite" in err, (bad, col, err)
            for k, name in enumerate(("ini_x", "ini_cash")):
                ini = [0.0, 10.0]
                ini[k] = bad
                rc, err = _call(lib, eng, ini=ini)
                assert rc == ERR_ARG and name in err, (bad, name, err)
            for k, name in enumerate(("min_cash_required", "max_q", "fix_order_cost", "vari_cost")):
                sc = [1.0, 5.0, 2.0, 1.0]
                sc[k] = bad
                rc, err = _call(lib, eng, scalars=sc)
                assert rc == ERR_ARG and name in err, (bad, name, err)
        for v in (0.0, -1.0):
            rc, err = _call(lib, eng, scalars=(1.0, 5.0, 2.0, v))
            assert rc == ERR_ARG and "vari_cost" in err
        rc, err = _call(lib, eng, scalars=(1.0, -0.5, 2.0, 1.0))
        assert rc == ERR_ARG and "max_q = -0.5" in err
        assert _call(lib, eng, scalars=(-3.0, 0.0, -2.0, 1e-3))[0] in (OK, ERR_DEVICE)  # negative costs and max_q = 0 are arguments like any
        # tables: finite values and NaN pass, an infinite entry is refused with its place
        tab = np.full((2, T, nx), NAN)
        tab[0, 1, 3], tab[1, 0, 0] = 7.5, -2.0
        assert _call(lib, eng, forms=[0, 1], c1=tab, c2=tab)[0] in (OK, ERR_DEVICE)
        for which, name in (("c1", "c1_tab"), ("c2", "c2_tab")):
            for bad in (float("inf"), -float("inf")):
                t2 = tab.copy()
                t2[1, 2, 5] = bad
                rc, err = _call(lib, eng, forms=[0, 1], **{which: t2})
                assert rc == ERR_ARG and f"{name}[1][2][5]" in err and "infinite" in err, err
        # a negative order (S < x < s) and an off-grid start are not refused
        assert _call(lib, eng, ini=(0.5, 10.25), rules=np.tile(np.array([[9.0, 0.0, 0.0, 0.25]]), (1, T, 1)))[0] in (OK, ERR_DEVICE)


def test_a_period_without_tile_or_spec_is_a_state_error(sia, lib):
    d = cases.f3_testing().desc()
    h = C.c_void_p()
    assert lib.sdpgpu_create(C.byref(d), C.byref(h)) == OK
    try:
        from stochastic_inventory_amd._abi import DIST_POISSON, SdpgpuDistSpec, SdpgpuSimResult
        res = (SdpgpuSimResult * 1)()
        fm = np.zeros(1, dtype=np.int32)
        rules = np.tile(np.array([[4.5, 3.0, 50.0, 8.25]]), (1, d.periods, 1))

        def call():
            return lib.sdpgpu_cash_rule_simulate(h, 5, 1, LHS, 0, None, 0.0, 10.0, 1, fm.ctypes.data_as(C.POINTER(C.c_int32)), _dp(rules), None,
                                                 None, 0.0, 5.0, 2.0, 1.0, res, None)
        tile = cases.f3_testing().pmf[0]
        dd, pp = np.ascontiguousarray(tile[:, 0]), np.ascontiguousarray(tile[:, 1])
        for t in (0, 2, 3):
            assert lib.sdpgpu_set_pmf(h, t, _dp(dd), _dp(pp), len(dd)) == OK
        assert call() == ERR_STATE
        assert b"pmf of period 2" in lib.sdpgpu_last_error(h)
        # a spec on the period without a tile: nothing is missing but the device (the rollout reads no table, so it needs no layout)
        spec = SdpgpuDistSpec()
        spec.kind, spec.a, spec.b = DIST_POISSON, 4.0, 0.0
        assert lib.sdpgpu_set_sampler(h, 1, C.byref(spec)) == OK
        assert call() in (OK, ERR_DEVICE)
    finally:
        lib.sdpgpu_destroy(h)


def test_valid_arguments_without_a_device_are_a_device_error(sia, lib):
    has_gpu = False
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        pass
    eng, w = _engine(sia)
    with eng:  # (no solve)
        rc, err = _call(lib, eng, forms=[0, 1, 2])
        assert rc == (OK if has_gpu else ERR_DEVICE) and (has_gpu or "no HIP device" in err)
        rows = np.tile(np.array([[4.5, 3.0, 50.0, 8.25]]), (eng.T, 1))
        kw = dict(min_cash_required=0.0, max_q=5.0, fix_order_cost=2.0, vari_cost=1.0)
        if not has_gpu:
            with pytest.raises(sia.SdpgpuError) as e:
                eng.cash_rule_simulate(5, 1, 0.0, 10.0, [0], rows, **kw)
            assert e.value.code == ERR_DEVICE
        with pytest.raises(ValueError):
            eng.cash_rule_simulate(5, 1, 0.0, 10.0, [0], rows[:-1], **kw)
        with pytest.raises(ValueError):
            eng.cash_rule_simulate(5, 1, 0.0, 10.0, [0, 1], rows, **kw)
        with pytest.raises(ValueError):
            eng.cash_rule_simulate(5, 1, 0.0, 10.0, [0], rows, c1_tab=np.zeros((1, eng.T, 20)), **kw)


# ---- the twin on hand-computed examples ------------------------------------------------------------------------------------
def _hand_functor(sia, **changes):
    """Formula 1 on an integer cash grid, T = 2: imm = price min(x + q, d) - (q > 0 ? 3 : 0) - 2 q - 1 max(x + q - d, 0) - 1, plus
    0.5 max(x + q - d, 0) in period 2; next cash = round(cash + imm), next inventory = max(0, x + q - d)."""
    kw = dict(price=4, fixOrderCost=3, variCost=2, holdingCost=1, overheadCost=1, salvageValue=0.5, penaltyCost=0, maxOrderQuantity=20,
              minInventoryState=0, maxInventoryState=20, minCashState=-50, maxCashState=20000, cashRoundMult=1.0, cashRoundDiv=1.0,
              cashRoundIntDiv=True, cashFormula=1)
    kw.update(changes)
    return sia.CashFunctor(**kw)


HAND_RULE = [[4.0, 0.0, 0.0, 6.0], [5.5, 0.0, 0.0, 9.5]]  # (s, c1, c2, S) of the two periods
HAND_ARGS = (1.0, 20.0, 3.0, 2.0)  # minCashRequired, maxQ, fixOrderCost, variCost


def _hand(sia, form, ini, c1=None, c2=None, disc=(1.0, 1.0), args=HAND_ARGS, rule=HAND_RULE, demands=((3.0, 2.0),)):
    P = ct.Problem(_hand_functor(sia), 2)
    tabs = []
    for cache in (c1, c2):
        tabs.append(None if cache is None else ct.pack(P, cache)[None])
    r = ct.simulate(P, np.array(demands), np.array(disc), ini[0], ini[1], [form], [rule], tabs[0], tabs[1], *args)
    return float(r["sum"][0, 0]), r["events"][0]


def test_twin_form_0_by_hand(sia):
    """(s, C1(x), C2(x), S), CashSimulation.java:996-1042; x = 1, cash = 20, demands (3, 2).
    t = 0 (:1011): 1 < 4, q = 6 - 1 = 5.  imm = 4 min(6, 3) - 3 - 2 * 5 - 1 * 3 - 1 = 12 - 3 - 10 - 3 - 1 = -5; cash 15, x = 3.
    t = 1 (:1013): m = (int) max(0, (15 - 1 - 3) / 2) = (int) 5.5 = 5; min(5, 20) = 5 (:1014).  3 < 5.5; no tables: C1 = 0
    (:1017), C2 = 10000 (:1021); 15 > 0 and 15 < 10000 (:1026): q = min(5, 9.5 - 3) = 5 (:1028).
    imm = 4 min(8, 2) - 3 - 10 - 1 * 6 - 1 = -12, salvage 0.5 * 6 = 3: -9.  sum = -5 - 9 = -14."""
    total, ev = _hand(sia, ct.SC12S, (1.0, 20.0))
    assert total == -14.0 and ev["table_miss"] == 2 and ev["capped_by_cash"] == 1 and ev["up_to_S"] == 1
    # discount weights (1, 0.5): -5 + 0.5 * -9
    assert _hand(sia, ct.SC12S, (1.0, 20.0), disc=(1.0, 0.5))[0] == -9.5
    # the (int): cash 10 -> t = 0 as above, cash 5; t = 1: m = (int) ((5 - 1 - 3) / 2) = (int) 0.5 = 0, q = min(0, 6.5) = 0:
    # imm = 4 min(3, 2) - 0 - 0 - 1 * 1 - 1 + 0.5 * 1 = 6.5; sum = -5 + 6.5 = 1.5
    assert _hand(sia, ct.SC12S, (1.0, 10.0))[0] == 1.5
    # C1(3) = 15 present in period 2: 15 > 15 fails (strict, :1026), q = 0: imm = 4 * 2 - 1 * 1 - 1 + 0.5 = 6.5; sum = 1.5
    total, ev = _hand(sia, ct.SC12S, (1.0, 20.0), c1={(2, 3.0): 15.0})
    assert total == 1.5 and ev["table_hit"] == 1 and ev["table_miss"] == 1 and ev["cash_le_c1"] == 1
    assert _hand(sia, ct.SC12S, (1.0, 20.0), c1={(2, 3.0): 14.5})[0] == -14.0
    # C2(3) = 15: 15 < 15 fails
    total, ev = _hand(sia, ct.SC12S, (1.0, 20.0), c2={(2, 3.0): 15.0})
    assert total == 1.5 and ev["cash_ge_c2"] == 1
    assert _hand(sia, ct.SC12S, (1.0, 20.0), c2={(2, 3.0): 15.5})[0] == -14.0
    # entries of other keys are not this key's: period 1, inventory 4, an off-grid 3.5
    assert _hand(sia, ct.SC12S, (1.0, 20.0), c1={(1, 3.0): 99.0, (2, 4.0): 99.0, (2, 3.5): 99.0})[0] == -14.0
    # the default C2 = 10000: cash 10020 -> 10015; 10015 < 10000 fails, q = 0 (sum 1.5); C2(3) = 20000 lets the rule order:
    # m = (int) 5005.5 = 5005, min(5005, 20) = 20, q = min(20, 6.5) = 6.5: imm = 4 * 2 - 3 - 13 - 7.5 - 1 + 3.75 = -12.75; -17.75
    assert _hand(sia, ct.SC12S, (1.0, 10020.0))[0] == 1.5
    assert _hand(sia, ct.SC12S, (1.0, 10020.0), c2={(2, 3.0): 20000.0})[0] == -17.75
    # the default C1 = 0: cash 3 -> -2 after period 1; minCashRequired = -20 leaves m = (int) ((-2 + 20 - 3) / 2) = 7, but -2 > 0
    # fails: q = 0, imm = 6.5, sum 1.5; C1(3) = -5: q = min(7, 6.5) = 6.5, imm = -12.75, sum -17.75
    args = (-20.0, 20.0, 3.0, 2.0)
    assert _hand(sia, ct.SC12S, (1.0, 3.0), args=args)[0] == 1.5
    assert _hand(sia, ct.SC12S, (1.0, 3.0), args=args, c1={(2, 3.0): -5.0})[0] == -17.75


def test_twin_form_1_by_hand(sia):
    """(s, C1(x), S), CashSimulation.java:1050-1093; x = 1, cash = 10, demands (3, 2).
    t = 0 (:1064-1066): q = 6 - 1 = 5, capped: min(5, max(0, (10 - 1 - 3) / 2)) = min(5, 3) = 3.
    imm = 4 min(4, 3) - 3 - 2 * 3 - 1 * 1 - 1 = 12 - 3 - 6 - 1 - 1 = 1; cash 11, x = 1.
    t = 1 (:1069): m = (11 - 1 - 3) / 2 = 3.5, NO (int); min(3.5, 20).  1 < 5.5, C1 absent = 0 (:1073), 11 > 0 (:1078): q = min(3.5,
    9.5 - 1) = 3.5 (:1079).  imm = 4 min(4.5, 2) - 3 - 7 - 1 * 2.5 - 1 = -5.5, salvage 0.5 * 2.5 = 1.25: -4.25.  sum = -3.25."""
    total, ev = _hand(sia, ct.SC1S, (1.0, 10.0))
    assert total == -3.25 and ev["capped_by_cash"] == 2 and ev["table_miss"] == 1
    # forms 0 and 2 do not cap period 1: q = 5, imm = -5, cash 5; form 2 then orders m = 0.5 where form 0 ordered (int) 0.5 = 0:
    # imm = 4 min(3.5, 2) - 3 - 1 - 1 * 1.5 - 1 + 0.75 = 2.25; sum = -2.75 (form 0: 1.5, above)
    assert _hand(sia, ct.SMEANCS, (1.0, 10.0))[0] == -2.75
    # max_q caps m: maxQ = 2 -> q = min(2, 8.5) = 2: imm = 4 * 2 - 3 - 4 - 1 * 1 - 1 + 0.5 = -0.5; sum = 0.5
    assert _hand(sia, ct.SC1S, (1.0, 10.0), args=(1.0, 2.0, 3.0, 2.0))[0] == 0.5
    # C1(1) = 11 in period 2: 11 > 11 fails, q = 0: imm = 4 min(1, 2) - 0 - 0 - 0 - 1 = 3 (level -1: no holding, no salvage); sum 4
    total, ev = _hand(sia, ct.SC1S, (1.0, 10.0), c1={(2, 1.0): 11.0})
    assert total == 4.0 and ev["table_hit"] == 1 and ev["cash_le_c1"] == 1
    # a fractional inventory never hits: start x = 0.5 -> q = min(5.5, 3) = 3, level 3.5 - 3 = 0.5: imm = 12 - 3 - 6 - 0.5 - 1 = 1.5,
    # cash round(11.5) = 12, x = 0.5; an entry at (2, 0.0) or (2, 1.0) is not x = 0.5's
    total, ev = _hand(sia, ct.SC1S, (0.5, 10.0), c1={(2, 0.0): 99.0, (2, 1.0): 99.0})
    assert ev["table_miss"] == 1 and ev["table_hit"] == 0 and ev["fractional_inventory"] == 1
    # t = 1: m = (12 - 1 - 3) / 2 = 4, q = min(4, 9) = 4: imm = 4 * 2 - 3 - 8 - 2.5 - 1 + 1.25 = -5.25; sum = -3.75
    assert total == -3.75


def test_twin_form_2_by_hand(sia):
    """(s, C, S) with the row's own C, CashSimulation.java:1101-1134; x = 1, cash = 20, demands (3, 2), rule rows (4, -, -, 6) and
    (5.5, C, -, 9.5).  t = 0 (:1113): q = 5, imm = -5 (as form 0), cash 15, x = 3.
    t = 1 (:1115-1116): m = min((15 - 1 - 3) / 2, 20) = 5.5; C = 14: 15 > 14 (:1119), q = min(5.5, 6.5) = 5.5 (:1120).
    imm = 4 min(8.5, 2) - 3 - 11 - 1 * 6.5 - 1 = -13.5, salvage 3.25: -10.25.  sum = -15.25.  C = 15: not above, q = 0, sum 1.5."""
    rule = [[4.0, 0.0, 0.0, 6.0], [5.5, 14.0, 0.0, 9.5]]
    total, ev = _hand(sia, ct.SMEANCS, (1.0, 20.0), rule=rule)
    assert total == -15.25 and ev["table_hit"] == ev["table_miss"] == 0 and ev["capped_by_cash"] == 1
    rule[1][1] = 15.0
    total, ev = _hand(sia, ct.SMEANCS, (1.0, 20.0), rule=rule)
    assert total == 1.5 and ev["cash_le_c1"] == 1
    # form 2 reads no table: an entry that would stop forms 0 and 1 changes nothing
    rule[1][1] = 14.0
    assert _hand(sia, ct.SMEANCS, (1.0, 20.0), rule=rule, c1={(2, 3.0): 99.0})[0] == -15.25
    # x >= s in both periods: nothing ordered.  x = 7: imm = 4 * 3 - 4 - 1 = 7, x = 4... 4 < 5.5 orders; take s = (4, 3.5) instead
    total, ev = _hand(sia, ct.SMEANCS, (7.0, 20.0), rule=[[4.0, 0.0, 0.0, 6.0], [3.5, 0.0, 0.0, 9.5]])
    # t = 0: imm = 12 - 1 * 4 - 1 = 7, cash 27, x = 4; t = 1: 4 >= 3.5: imm = 4 * 2 - 1 * 2 - 1 + 0.5 * 2 = 6; sum 13
    assert total == 13.0 and ev["x_ge_s"] == 2
    # a negative order is not refused: x = 3.75 < s = 4 with S = 3 gives q = -0.75 in period 1: no fixed cost, v q = -1.5:
    # imm = 4 min(3, 3) - 0 + 1.5 - 0 - 1 = 12.5; cash round(32.5) = 33, x = 0; t = 1: x >= s = -1: imm = 4 * 0 - 1 = -1; sum 11.5
    assert _hand(sia, ct.SMEANCS, (3.75, 20.0), rule=[[4.0, 0.0, 0.0, 3.0], [-1.0, 0.0, 0.0, 9.5]])[0] == 11.5


def test_java_int_saturates():
    assert [ct.java_int(v) for v in (5.99, -5.99, 1e300, -1e300, NAN, 2147483646.5)] == [5, -5, 2147483647, -2147483648, 0, 2147483646]


# ---- Python: packing, the mapping of optsCS, the host route ----------------------------------------------------------------
def test_dict_to_table_packing(sia):
    from stochastic_inventory_amd.simulation import cash_rule_rows, cash_rule_table_index, pack_cash_rule_table
    tab = pack_cash_rule_table({(1, 0.0): 1.5, (2, 3.0): -2.0, (2, 3.5): 9.0, (3, 10.0): 4.0, (2, 11.0): 5.0, (4, 1.0): 6.0,
                                sia.CashState(3, 2.0, 77.0): 8.0}, 3, 0.0, 1.0, 11)
    want = np.full((3, 11), NAN)
    want[0, 0], want[1, 3], want[2, 10], want[2, 2] = 1.5, -2.0, 4.0, 8.0  # 3.5 and 11 are off the grid, period 4 past the horizon
    assert np.array_equal(tab, want, equal_nan=True)
    assert np.isnan(pack_cash_rule_table(None, 2, 0.0, 1.0, 4)).all()
    # a half-unit grid from -1: key ix = -1 + 0.5 ix
    assert [cash_rule_table_index(x, -1.0, 0.5, 5) for x in (-1.0, -0.5, 1.0, 1.5, 0.25, -1.5)] == [0, 1, 4, None, None, None]
    # the twin's own packing agrees
    P = ct.Problem(_hand_functor(sia), 2)
    cache = {(1, 0.0): 1.5, (2, 3.0): -2.0, (2, 3.5): 9.0, (2, 21.0): 5.0}
    assert np.array_equal(ct.pack(P, cache), pack_cash_rule_table(cache, 2, 0.0, 1.0, 21), equal_nan=True)
    # optsCS: three columns [s, C, S] of forms 1 and 2 -> (s, C, 0, S); four columns as they are
    assert cash_rule_rows(1, [[4, 7, 9], [5, 8, 10]]).tolist() == [[4, 7, 0, 9], [5, 8, 0, 10]]
    assert cash_rule_rows(0, [[4, 1, 2, 9]]).tolist() == [[4, 1, 2, 9]]
    with pytest.raises(ValueError):
        cash_rule_rows(0, [[4, 7, 9]])


def test_the_host_route_equals_the_twin(sia):
    """CashSimulation(sampler="host") rolls the rules through the recursion's lambdas: on given demands it gives the twin's sums,
    and its reference signatures return mean + iniCash."""
    from stochastic_inventory_amd import pmf as PM
    s = setup_of(cases.f3_tenths)
    w = s.w
    rec = sia.CashRecursion(w.direction, w.pmf, functor=w.functor, discountFactor=w.functor.discountFactor)
    try:
        sim = sia.CashSimulation([PM.PoissonDist(m) for m in (3, 4, 2)], 40, rec, discountFactor=w.functor.discountFactor, seed=5,
                                 sampler="host")
        dem, want = reference(cases.f3_tenths, 65)
        ini = sia.CashState(1, *s.ini)
        rules = s.rule_tuples()
        c1, c2 = rules[0][2], rules[0][3]
        got = sim.simulateRulesOnDemands(ini, rules, dem, *s.args())
        assert got.tobytes() == want["sum"].tobytes()
        # host-sampled: the three reference methods are simulateRules of one rule (the sampler is seeded: the same paths)
        a = sia.CashSimulation(sim.distributions, 40, rec, w.functor.discountFactor, seed=5, sampler="host")
        v0 = a.simulatesCS(ini, s.rules[0], c1, c2, *s.args())
        assert a.last_values.shape == (1, 40) and v0 == math.fsum(a.last_values[0].tolist()) / 40 + s.ini[1]
        b = sia.CashSimulation(sim.distributions, 40, rec, w.functor.discountFactor, seed=5, sampler="host")
        all3 = b.simulateRules(ini, rules[:3], *s.args())
        assert all3[0] == v0
        c = sia.CashSimulation(sim.distributions, 40, rec, w.functor.discountFactor, seed=5, sampler="host")
        assert c.simulatesCS(ini, s.rules[1][:, [0, 1, 3]], c1, *s.args()) != v0
        with pytest.raises(TypeError):
            c.simulatesCS(ini, s.rules[0], c1, 1.0, 2.0)
    finally:
        rec.engine.close()


# ---- the coverage condition ------------------------------------------------------------------------------------------------
def test_the_gpu_tests_rules_take_every_branch():
    """Over the cases and sizes of the GPU test, the twin's trace shows every event at least once per form it applies to; the
    fractional inventory occurs on f3_tenths (under every form: its variCost of 0.7 makes cash / variCost fractional, and the
    levels S are fractional).  The demands are the twin sampler's: no device is needed."""
    seen = {form: {} for form in (ct.SC12S, ct.SC1S, ct.SMEANCS)}
    per_case = {}
    for make in CASES:
        for n in NS:
            _, ref = reference(make, n)
            for r, form in enumerate(MIXED_FORMS):
                for e, k in ref["events"][r].items():
                    seen[form][e] = seen[form].get(e, 0) + k
                    per_case[(make.__name__, form, e)] = per_case.get((make.__name__, form, e), 0) + k
    for form, events in ct.EVENTS_OF_FORM.items():
        print(form, {e: seen[form].get(e, 0) for e in ct.EVENTS})
        for e in events:
            assert seen[form].get(e, 0) > 0, (form, e)
        for e in set(ct.EVENTS) - set(events):
            assert seen[form].get(e, 0) == 0, (form, e)
    for form in seen:
        assert per_case.get(("f3_tenths", form, "fractional_inventory"), 0) > 0, form
    # the all-NaN tables of rule 3 miss every time; the populated ones hit and miss
    for make in CASES:
        ev = reference(make, 1025)[1]["events"]
        assert ev[3]["table_hit"] == 0 and ev[3]["table_miss"] > 0
        print(make.__name__, [dict(e) for e in ev])
