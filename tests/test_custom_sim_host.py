"""User-functor rollouts (sdpgpu_custom_simulate, sdpgpu_custom_simulate_sampled, sdpgpu_custom_rule_simulate; DESIGN 4
"User-functor rollouts") as far as they go without a GPU: the new symbols and mirror methods, every refusal with its status and
a text naming the argument BEFORE any device call, the rollout program compiling for gfx950 around every kind of user text, the
host twin (tests/custom_rule_twin.py) against the mirror's host loop through Python lambdas, the FindsSOverDraft mirror on a
hand-made table, and the COVERAGE CONDITION: on the rules and paths tests/test_gpu_custom_sim.py uses, the twin's trace shows
every branch of the definition at least once."""
import ctypes as C
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
from test_simulate_sampled_host import LHS, RANDOM, tile_demands, twin_sample  # noqa: E402

OK, ERR_ARG, ERR_STATE, ERR_DEVICE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdpgpu_custom_simulate", "sdpgpu_custom_simulate_sampled", "sdpgpu_custom_rule_simulate")
SEED = 20240611  # (tests/test_gpu_custom_sim.py draws with the same seed)


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _overdraft(sia, text=None, **changes):
    d = co.desc(sia)
    for k, v in changes.items():
        setattr(d, k, v)
    return sia.SdpEngine(d, co.pmf(), custom_source=co.OVERDRAFT_TESTING if text is None else text, custom_params=co.PARAMS)


def _rule(lib, eng, n=5, seed=1, mode=LHS, first_path=0, ini=(0.0, 10.0), forms=(0,), rules="default", scalars=(-5.0, 14.0, 6.0, 2.0),
          n_rules=None, null=(), disc=None):
    from stochastic_inventory_amd._abi import SdpgpuSimResult
    T = eng.T
    fm = np.asarray(forms, dtype=np.int32)
    if isinstance(rules, str):
        rules = np.tile(np.array([[5.0, 0.0, 12.0, 14.0]]), (len(fm), T, 1))
    rules = np.ascontiguousarray(rules, dtype=np.float64)
    res = (SdpgpuSimResult * 32)()
    rc = lib.sdpgpu_custom_rule_simulate(
        eng._h, n, seed, mode, first_path, _dp(disc), float(ini[0]), float(ini[1]), len(fm) if n_rules is None else n_rules,
        None if "form" in null else fm.ctypes.data_as(C.POINTER(C.c_int32)), None if "rule" in null else _dp(rules),
        *[float(v) for v in scalars], None if "results" in null else res, None, None)
    return rc, lib.sdpgpu_last_error(eng._h).decode()


def _sampled(lib, eng, n=5, seed=1, mode=LHS, first_path=0, result=True):
    from stochastic_inventory_amd._abi import SdpgpuSimResult
    res = SdpgpuSimResult()
    rc = lib.sdpgpu_custom_simulate_sampled(eng._h, n, seed, mode, first_path, None, 0.0, 10.0, 0.0, C.byref(res) if result else None, None,
                                            None, None)
    return rc, lib.sdpgpu_last_error(eng._h).decode()


def _given(lib, eng, n=5, null=()):
    dem, disc, out = np.zeros((max(n, 1), eng.T)), np.ones(eng.T), np.zeros(max(n, 1))
    valid = np.zeros(max(n, 1), dtype=np.uint8)
    rc = lib.sdpgpu_custom_simulate(eng._h, n, None if "demand" in null else _dp(dem), None if "discount" in null else _dp(disc), 0.0, 10.0, 0.0,
                                    None if "out_sum" in null else _dp(out),
                                    None if "out_valid" in null else valid.ctypes.data_as(C.POINTER(C.c_uint8)))
    return rc, lib.sdpgpu_last_error(eng._h).decode()


# ---- the boundary ----------------------------------------------------------------------------------------------------------
def test_the_new_symbols_and_methods_exist(sia, lib):
    header = open(os.path.join(ROOT, "include", "sdpgpu.h")).read()
    for name in NEW:
        assert name in sia._abi.EXPORTS and hasattr(lib, name) and name + "(" in header
    for macro, v in (("SDPGPU_ORULE_SS", 0), ("SDPGPU_ORULE_SCS", 1), ("SDPGPU_ORULE_SCS1S2", 2)):
        assert f"#define {macro} {v}" in header
    assert (sia._abi.ORULE_SS, sia._abi.ORULE_SCS, sia._abi.ORULE_SCS1S2) == (0, 1, 2)
    assert lib.sdpgpu_abi_version() == 6  # additive
    assert [len(sia._abi.EXPORTS[n][1]) for n in NEW] == [9, 13, 18]
    for m in ("custom_simulate", "custom_simulate_sampled", "custom_rule_simulate"):
        assert hasattr(sia.SdpEngine, m)
    import inspect
    from stochastic_inventory_amd import simulation
    args = ["iniState", "optsS", "minCashRequired", "maxQ", "fixOrderCost", "variCost"]
    assert list(inspect.signature(simulation.CashSimulation.simulatesSOD).parameters)[1:] == args
    assert list(inspect.signature(simulation.CashSimulation.simulatesCSDraft).parameters)[1:] == ["iniState", "optsCS"] + args[2:]
    assert list(inspect.signature(simulation.CashSimulation.simulatesSOD2).parameters)[1:] == ["iniState", "optsCS"]
    assert list(inspect.signature(simulation.CashSimulation.simulateOverdraftRules).parameters)[1:3] == ["iniState", "rules"]
    assert sia.FindsSOverDraft is not None and "FindsSOverDraft" in sia.__all__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**User-functor rollouts:" in design
    assert "sdpgpu_custom_simulate" in header.split("sdpgpu_simulate is not available")[1][:400]  # the pointer to the new calls


def test_refusals_come_before_any_device_call_and_name_the_argument(sia, lib):
    assert lib.sdpgpu_custom_rule_simulate(None, 5, 1, 0, 0, None, 0.0, 0.0, 1, None, None, 0.0, 1.0, 0.0, 1.0, None, None, None) == ERR_ARG
    assert lib.sdpgpu_custom_simulate_sampled(None, 5, 1, 0, 0, None, 0.0, 0.0, 0.0, None, None, None, None) == ERR_ARG
    assert lib.sdpgpu_custom_simulate(None, 5, None, None, 0.0, 0.0, 0.0, None, None) == ERR_ARG
    # ERR_UNSUPPORTED: not a user-functor handle -- the text points at the built-in families' calls
    w = cases.f3_testing()
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        for call in (_rule, _sampled, _given):
            rc, err = call(lib, eng)
            assert rc == ERR_UNSUPPORTED and "not a user-functor handle" in err and "sdpgpu_simulate* / sdpgpu_cash_rule_simulate" in err
    # ... the state shape SURVIVAL
    d = co.desc(sia)
    d.family = 6
    with sia.SdpEngine(d, co.pmf(), custom_source=co.OVERDRAFT_TESTING, custom_params=co.PARAMS) as eng:
        for call in (_rule, _sampled, _given):
            rc, err = call(lib, eng)
            assert rc == ERR_UNSUPPORTED and "SURVIVAL" in err
    # ... the rule call on a shape without a cash axis, or with a pipeline quantity
    for make, text in ((cases.f1_small, cs.BACKORDER), (cases.f2_clamped, cs.LEADTIME)):
        w = make()
        with sia.SdpEngine(w.desc(), w.pmf, custom_source=text, custom_params=_params_backorder(w.functor)) as eng:
            rc, err = _rule(lib, eng)
            assert rc == ERR_UNSUPPORTED and "cash axis" in err and "pipeline quantity" in err
    d = co.desc(sia)
    d.family = 5  # (x, cash, preQ)
    with sia.SdpEngine(d, co.pmf(), custom_source=co.OVERDRAFT_TESTING, custom_params=co.PARAMS) as eng:
        rc, err = _rule(lib, eng)
        assert rc == ERR_UNSUPPORTED and "pipeline quantity" in err
    # ERR_STATE: a rank of several
    with _overdraft(sia, world_size=2, rank=0) as eng:
        for call in (_rule, _sampled, _given):
            rc, err = call(lib, eng)
            assert rc == ERR_STATE and "world_size 1" in err
    with _overdraft(sia) as eng:
        T = eng.T
        # limits of the build, not bad arguments
        for call in (_rule, _sampled, _given):
            rc, err = call(lib, eng, n=(1 << 24) + 1)
            assert rc == ERR_UNSUPPORTED and "n_paths" in err and str(1 << 24) in err
        # ERR_ARG: counts, mode, first_path
        for call in (_rule, _sampled):
            for n in (0, -3):
                rc, err = call(lib, eng, n=n)
                assert rc == ERR_ARG and "n_paths" in err
            rc, err = call(lib, eng, mode=2)
            assert rc == ERR_ARG and "mode" in err
            rc, err = call(lib, eng, mode=LHS, first_path=7)
            assert rc == ERR_ARG and "first_path" in err
        rc, err = _given(lib, eng, n=-1)
        assert rc == ERR_ARG and "n_paths" in err
        # NULL arrays
        for name in ("form", "rule", "results"):
            rc, err = _rule(lib, eng, null=(name,))
            assert rc == ERR_ARG and f"{name} is null" in err
        rc, err = _sampled(lib, eng, result=False)
        assert rc == ERR_ARG and "result is null" in err
        for name in ("demand", "discount", "out_sum", "out_valid"):
            rc, err = _given(lib, eng, null=(name,))
            assert rc == ERR_ARG and f"{name} is null" in err
        # n_rules, form
        for nr in (0, 17, -1):
            rc, err = _rule(lib, eng, n_rules=nr)
            assert rc == ERR_ARG and "n_rules" in err
        for bad in (3, -1):
            rc, err = _rule(lib, eng, forms=(0, bad))
            assert rc == ERR_ARG and "form[1]" in err
        # finiteness: rule entries, start values, discount
        rules = np.tile(np.array([[5.0, 0.0, 12.0, 14.0]]), (1, T, 1))
        for bad in (math.nan, math.inf):
            r = rules.copy()
            r[0, 2, 1] = bad
            rc, err = _rule(lib, eng, rules=r)
            assert rc == ERR_ARG and "rule[0][2][1]" in err
            rc, err = _rule(lib, eng, ini=(bad, 10.0))
            assert rc == ERR_ARG and "ini_x" in err
            rc, err = _rule(lib, eng, ini=(0.0, bad))
            assert rc == ERR_ARG and "ini_cash" in err
            disc = np.ones(T)
            disc[1] = bad
            rc, err = _rule(lib, eng, disc=disc)
            assert rc == ERR_ARG and "discount[1]" in err
        # the scalars, where a form reads them ...
        for k, name in enumerate(("min_cash_required", "max_q", "fix_order_cost", "vari_cost")):
            sc = [-5.0, 14.0, 6.0, 2.0]
            sc[k] = math.nan
            for form in (0, 1):
                rc, err = _rule(lib, eng, forms=(form,), scalars=sc)
                assert rc == ERR_ARG and name in err
        rc, err = _rule(lib, eng, scalars=(-5.0, -1.0, 6.0, 2.0))
        assert rc == ERR_ARG and "max_q" in err
        for v in (0.0, -2.0):
            rc, err = _rule(lib, eng, scalars=(-5.0, 14.0, 6.0, v))
            assert rc == ERR_ARG and "vari_cost" in err
        # ... and not where no form does (simulatesSOD2 takes none): such a call gets as far as the device
        rc, err = _rule(lib, eng, forms=(2,), scalars=(math.nan, -1.0, math.nan, 0.0))
        assert rc in (OK, ERR_DEVICE), err
        # the table calls before a solve
        for call in (_sampled, _given):
            rc, err = call(lib, eng)
            assert rc == ERR_STATE and "nothing has been solved" in err
    # n_paths * T above 2^27: a horizon long enough that 2^24 paths do not fit
    Tl = 9
    f = co.shape(sia)
    d = f.to_desc(Tl, sia.OptDirection.MAX)
    with sia.SdpEngine(d, cases._pmf([4] * Tl, 10), custom_source=co.OVERDRAFT_TESTING, custom_params=co.PARAMS) as eng:
        for call in (_rule, _sampled):
            rc, err = call(lib, eng, n=1 << 24)
            assert rc == ERR_UNSUPPORTED and "n_paths * T" in err and str(1 << 27) in err
    # ERR_STATE: a period without tile or spec
    d = co.desc(sia)
    h = C.c_void_p()
    prm = np.array(co.PARAMS)
    assert lib.sdpgpu_create_custom(C.byref(d), co.OVERDRAFT_TESTING.encode(), _dp(prm), len(prm), C.byref(h)) == OK
    try:
        from stochastic_inventory_amd._abi import SdpgpuSimResult
        res = (SdpgpuSimResult * 1)()
        fm = np.zeros(1, dtype=np.int32)
        rules = np.tile(np.array([[5.0, 0.0, 12.0, 14.0]]), (1, co.T, 1))
        rc = lib.sdpgpu_custom_rule_simulate(h, 5, 1, LHS, 0, None, 0.0, 10.0, 1, fm.ctypes.data_as(C.POINTER(C.c_int32)), _dp(rules), -5.0, 14.0,
                                             6.0, 2.0, res, None, None)
        assert rc == ERR_STATE and b"pmf of period 1" in lib.sdpgpu_last_error(h)
    finally:
        lib.sdpgpu_destroy(h)


def test_the_five_older_entry_points_still_refuse_a_user_functor(sia, lib):
    with _overdraft(sia) as eng:
        with pytest.raises(sia.SdpgpuError, match="user functor"):
            eng.simulate(np.zeros((1, eng.T)), np.ones(eng.T), 0.0, 10.0)
        with pytest.raises(sia.SdpgpuError, match="user functor"):
            eng.simulate_sampled(5, 1, 0.0, 10.0)
        with pytest.raises(sia.SdpgpuError, match="user functor"):
            eng.sample_demands(5, 1)
        with pytest.raises(sia.SdpgpuError, match="user functor"):
            eng.cash_rule_simulate(5, 1, 0.0, 10.0, [2], np.zeros((eng.T, 4)), min_cash_required=0, max_q=1, fix_order_cost=0, vari_cost=1)
        with pytest.raises(sia.SdpgpuError):
            eng.xr_simulate(5, 1, 0.0, 10.0, np.zeros(eng.T))


def test_the_rollout_program_compiles_around_every_kind_of_text(sia, lib, tmp_path, monkeypatch):
    """A valid call goes through the hipRTC compile for gfx950 before it looks for a solve or a device: with SDPGPU_CUSTOM_DUMP set
    the rollout object appears beside the engine's.  A cash-shaped text's rule call then lacks nothing but the device; a table
    call cannot have its solve on a box without one, and says so -- neither reports a compile error."""
    from stochastic_inventory_amd import workloads
    from test_gpu_custom_functor import _overdraft_limit_case
    has_gpu = _has_gpu()
    shape, lparams, lpmf = _overdraft_limit_case(sia)
    ldesc = shape.to_desc(len(lpmf), sia.OptDirection.MAX)
    w1, w2 = cases.f1_small(), cases.f2_clamped()
    texts = [("backorder", w1.desc(), w1.pmf, cs.BACKORDER, _params_backorder(w1.functor), False),
             ("leadtime", w2.desc(), w2.pmf, cs.LEADTIME, _params_backorder(w2.functor), False),
             ("limit", ldesc, lpmf, cs.OVERDRAFT_LIMIT, lparams, True),
             ("limit-fused", ldesc, lpmf, cs.OVERDRAFT_LIMIT_FUSED, lparams, True),
             ("level", w1.desc(), w1.pmf, workloads.CLSP_LAMBDAS_LEVEL_HIP, _params_backorder(w1.functor), False),
             ("testing", co.desc(sia), co.pmf(), co.OVERDRAFT_TESTING, co.PARAMS, True),
             ("testing-fused", co.desc(sia), co.pmf(), co.OVERDRAFT_TESTING_FUSED, co.PARAMS, True)]
    for name, desc, pmf, text, params, cash in texts:
        dump = tmp_path / f"{name}.co"
        monkeypatch.setenv("SDPGPU_CUSTOM_DUMP", str(dump))
        with sia.SdpEngine(desc, pmf, custom_source=text, custom_params=params) as eng:
            assert dump.exists() and not os.path.exists(str(dump) + ".sim")  # lazy: nothing at create
            rc, err = _sampled(lib, eng)
            assert rc == ERR_STATE and "nothing has been solved" in err and "compile" not in err, (name, err)
            sim = str(dump) + ".sim"
            assert os.path.getsize(sim) > 1000 and open(sim, "rb").read(4) == b"\x7fELF", name
            for kernel in (b"sdp_custom_sim", b"sdp_custom_rule_sim", b"sdp_custom_first"):
                assert kernel in open(sim, "rb").read(), (name, kernel)
            stamp = os.path.getmtime(sim)
            if cash:
                rc, err = _rule(lib, eng, forms=(0, 1, 2))
                assert rc == (OK if has_gpu else ERR_DEVICE) and "compile" not in err, (name, err)
                if not has_gpu:
                    assert "no HIP device" in err
            assert os.path.getmtime(sim) == stamp  # compiled once per handle
    # a text that compiles nowhere is reported at create, as before
    w = cases.f1_small()
    with pytest.raises(sia.SdpgpuError, match="does not compile"):
        sia.SdpEngine(w.desc(), w.pmf, custom_source="this is not C++", custom_params=[1.0])


# ---- the twin ----------------------------------------------------------------------------------------------------------------
def _python_lambdas():
    """CashOverdraftTesting's lambdas (CashOverdraftTesting.java:85-120) as the mirror's Python callables on (period, x, cash, q, d)."""
    price, K, v, h, rate, _, _, minI, maxI, minC, maxC = co.PARAMS

    def imm(period, x, cash, q, d):
        revenue = price * min(x + q, d)
        fixedCost = K if q > 0 else 0
        variableCost = v * q
        inventoryLevel = x + q - d
        holdCosts = h * max(inventoryLevel, 0)
        before = cash + revenue - fixedCost - variableCost - holdCosts
        interest = rate * max(-before, 0)
        after = before - interest
        return after - cash

    def trans(period, x, cash, q, d):
        from stochastic_inventory_amd import java_round
        nextInventory = max(0, x + q - d)
        revenue = price * min(x + q, d)
        fixedCost = K if q > 0 else 0
        nextCash = cash + revenue - fixedCost - v * q - h * max(nextInventory, 0)
        nextCash = nextCash - max(-nextCash, 0) * rate
        nextCash = maxC if nextCash > maxC else nextCash
        nextCash = minC if nextCash < minC else nextCash
        nextInventory = maxI if nextInventory > maxI else nextInventory
        nextInventory = minI if nextInventory < minI else nextInventory
        return float(nextInventory), java_round(nextCash * 10) / 10.0

    return imm, trans


_twin = {}


def twin_reference(which=(0, 1, 2, 3, 4), n=257, mode=LHS):
    key = (which, n, mode)
    if key not in _twin:
        draw = [lambda u, tile=tile: tile_demands(tile, u) for tile in co.pmf()]
        dem, _ = twin_sample(n, SEED, mode, 0, draw)
        fm, rows = co.rules(which)
        disc = np.array([math.pow(0.95, t) for t in range(co.T)])
        s = co.SCALARS
        args = (dem, disc, co.INI[0], co.INI[1], fm, rows, s["min_cash_required"], s["max_q"], s["fix_order_cost"], s["vari_cost"])
        _twin[key] = (dem, disc, fm, rows, args)
    return _twin[key]


def test_the_twin_equals_the_mirrors_host_loop(sia, oracle):
    """The twin calls the host compile of the device text; the mirror's host loop calls Python lambdas: the same sums, bit for bit,
    for the plain and the fused text -- and the same from simulation.overdraft_rule_order as from the twin's own order()."""
    from stochastic_inventory_amd import simulation
    dem, disc, fm, rows, args = twin_reference()
    imm, trans = _python_lambdas()
    plain = ct.simulate(ct.Lambdas(co.OVERDRAFT_TESTING, co.PARAMS, co.T), *args, cash_box=(-40.0, 120.0))
    fused = ct.simulate(ct.Lambdas(co.OVERDRAFT_TESTING_FUSED, co.PARAMS, co.T), *args)
    python = ct.simulate(None, *args, imm=imm, trans=trans)
    assert plain["sum"].tobytes() == fused["sum"].tobytes() == python["sum"].tobytes()
    s = co.SCALARS
    for r, form in enumerate(fm.tolist()):  # the mirror's order function, on every decision of 40 paths
        for p in range(40):
            x, cash, total = co.INI[0], co.INI[1], 0.0
            for t in range(co.T):
                q = simulation.overdraft_rule_order(form, t, rows[r, t], x, cash, co.INI[0], s["min_cash_required"], s["max_q"],
                                                    s["fix_order_cost"], s["vari_cost"])
                total += disc[t] * imm(t + 1, x, cash, q, float(dem[p, t]))
                if t + 1 < co.T:
                    x, cash = trans(t + 1, x, cash, q, float(dem[p, t]))
            assert np.float64(total).tobytes() == plain["sum"][r, p].tobytes(), (r, p)
    # the reference's arrays as rows
    assert np.array_equal(simulation.overdraft_rule_rows(0, [[5, 12]] * co.T, co.T), np.tile([5.0, 0.0, 12.0, 0.0], (co.T, 1)))
    assert np.array_equal(simulation.overdraft_rule_rows(1, [[6, -10, 13]] * co.T, co.T), np.tile([6.0, -10.0, 13.0, 0.0], (co.T, 1)))
    assert np.array_equal(simulation.overdraft_rule_rows(2, [[5, 20, 9, 14]] * co.T, co.T), np.tile([5.0, 20.0, 9.0, 14.0], (co.T, 1)))
    with pytest.raises(ValueError):
        simulation.overdraft_rule_rows(2, [[5, 20, 9]] * co.T, co.T)


def test_hand_computed_orders():
    ev = ct.Counter()
    row = (5.0, 20.0, 12.0, 14.0)
    a = (-5.0, 14.0, 6.0, 2.0)
    # t = 0: S itself; S - s; S - ini_x
    assert ct.order(ct.SS, 0, row, 3.0, 10.0, 3.0, *a, ev) == 12.0
    assert ct.order(ct.SCS, 0, row, 3.0, 10.0, 3.0, *a, ev) == 7.0
    assert ct.order(ct.SCS1S2, 0, row, 3.0, 10.0, 3.0, *a, ev) == 9.0
    # t >= 1: m = min(max(0, (cash + 5 - 6) / 2), 14)
    assert ct.order(ct.SS, 1, row, 2.5, 10.0, 0.0, *a, ev) == 4.5       # m = 4.5 binds (S - x = 9.5)
    assert ct.order(ct.SS, 1, row, 2.5, 40.0, 0.0, *a, ev) == 9.5       # S - x binds (m = 14: the cap)
    assert ct.order(ct.SS, 1, row, 5.0, 40.0, 0.0, *a, ev) == 0.0       # x < s is strict
    assert ct.order(ct.SS, 1, row, 2.5, -3.0, 0.0, *a, ev) == 0.0       # m = max(0, -2) = 0
    assert ct.order(ct.SCS, 1, row, 2.5, 20.0, 0.0, *a, ev) == 0.0      # cash > C is strict
    assert ct.order(ct.SCS, 1, row, 2.5, 20.5, 0.0, *a, ev) == 9.5
    assert ct.order(ct.SCS1S2, 1, row, 2.5, 20.1, 0.0, *a, ev) == 9.5   # cash <= C + 0.1: up to S1
    assert ct.order(ct.SCS1S2, 1, row, 2.5, 20.2, 0.0, *a, ev) == 11.5  # above: up to S2
    assert ct.order(ct.SCS1S2, 1, row, 7.0, 0.0, 0.0, *a, ev) == 0.0
    assert ct.order(ct.SCS1S2, 1, (5.0, 20.0, 1.0, 2.0), 2.5, 0.0, 0.0, *a, ev) == -1.5  # a negative q is not refused


def test_coverage_condition_on_the_gpu_tests_rules_and_paths(oracle):
    """Parity on the GPU cannot pass on an untaken branch: over the five mixed rules and the 257 LHS paths of
    tests/test_gpu_custom_sim.py (the device's own draws: the sampler twin) every branch is taken at least once -- form 0: no
    order, m binds, S - x binds; form 1: x >= s, cash <= C, m binds, S - x binds; form 2: no order, S1, S2; at least one cash clamp
    and one fractional inventory."""
    dem, disc, fm, rows, args = twin_reference()
    out = ct.simulate(ct.Lambdas(co.OVERDRAFT_TESTING, co.PARAMS, co.T), *args, cash_box=(-40.0, 120.0))
    for r, ev in enumerate(out["events"]):
        print(r, int(fm[r]), dict(ev))
    assert ct.coverage_gaps(fm, out["events"]) == []
    # the three base rules alone take every branch of their forms as well
    assert [g for g in ct.coverage_gaps(fm[:3], out["events"][:3]) if g[0] >= 0] == []


# ---- FindsSOverDraft ---------------------------------------------------------------------------------------------------------
def test_finds_s_overdraft_on_a_hand_made_table(sia):
    # rows [period, x, cash, Q], sorted by (period, x, cash)
    tab = np.array([
        [1, 0, 10, 7],
        [2, 0, -5, 0], [2, 0, 5, 6], [2, 1, -5, 0], [2, 1, 5, 4], [2, 2, 5, 3], [2, 3, 5, 0], [2, 4, 5, 0],
        [3, 0, 0, 5], [3, 1, -8, 0], [3, 1, 2, 0], [3, 1, 9, 2], [3, 2, 0, 0],
    ], dtype=np.float64)
    f = sia.FindsSOverDraft(3, 10.0)
    assert f.T == 3 and f.iniCash == 10.0
    # getsS: period 1 = (x, x + Q); then from the LAST ordering row j of the period: s = x of row j + 1, S = x + Q of row j
    assert np.array_equal(f.getsS(tab), [[0, 7], [3, 5], [2, 3]])
    # getsCS: S = x + Q of the ordering rows passing `cash + Q > S so far` (scanned from the end); C = the largest cash of a
    # non-ordering row at or below an ordering one, from -500
    #   period 2, from the end: (2, 5, 3): 5 + 3 > 0 -> S = 5; (1, 5, 4): 9 > 5 -> S = 5; (1, -5, 0): C = -5; (0, 5, 6): 11 > 5 ->
    #   S = 6; (0, -5, 0): C stays -5
    #   period 3: (1, 9, 2): 11 > 0 -> S = 3; (1, 2, 0): C = 2; (1, -8, 0): stays; (0, 0, 5): 5 > 3 -> S = 5
    assert np.array_equal(f.getsCS(tab), [[0, 10, 7], [3, -5, 6], [2, 2, 5]])
    # a period that orders nowhere keeps the zeros / the -500
    quiet = np.array([[1, 0, 10, 7], [2, 0, 5, 0], [2, 1, 5, 0]], dtype=np.float64)
    g = sia.FindsSOverDraft(2, 10.0)
    assert np.array_equal(g.getsS(quiet), [[0, 7], [0, 0]]) and np.array_equal(g.getsCS(quiet), [[0, 10, 7], [0, -500, 0]])
    # the read of row j + 1 where the last row of a period orders: the reference's ArrayIndexOutOfBoundsException
    broken = np.array([[1, 0, 10, 7], [2, 0, 5, 0], [2, 1, 5, 3]], dtype=np.float64)
    for fn in (g.getsS, g.getsCS):
        with pytest.raises(IndexError, match="last row of period 2"):
            fn(broken)
    with pytest.raises(ValueError):
        g.getsS(np.zeros((0, 4)))
