"""User-defined lambdas on the GPU (sdpgpu_create_custom): the three Java lambdas of a driver written as HIP
device text, compiled by hipRTC around the engine's loop.  Parity: (i) a built-in family restated as user text
gives the built-in kernels' tables bit for bit; (ii) a driver OUTSIDE the built-in families
(CashOverdraftLimit.java) equals the oracle running the same text compiled for the host."""
import numpy as np
import pytest

import cases
import custom_sources as cs
from test_custom_functor import _params_backorder, fuzz_text_instances

pytestmark = pytest.mark.gpu


def _tables_equal(eng, V, pol, what):
    for period in range(1, len(V) + 1):
        gv, gp = eng.values(period), eng.policy(period)
        assert np.array_equal(gp, pol[period - 1]), f"{what} t={period}: policy indices differ"
        assert np.all(np.abs(gv - V[period - 1]) <= 1e-9 * np.maximum(np.abs(V[period - 1]), 1e-300))
        assert np.array_equal(gv, V[period - 1]), f"{what} t={period}: values not bit-identical"


@pytest.mark.parametrize("make,src", [(cases.f1_small, cs.BACKORDER), (cases.f1_max, cs.BACKORDER),
                                      (cases.f1_clsp_main, cs.BACKORDER), (cases.f2_clamped, cs.LEADTIME)],
                         ids=["f1_small", "f1_max", "f1_clsp_main", "f2_clamped"])
def test_builtin_family_as_user_text(sia, oracle, make, src):
    w = make()
    prm = _params_backorder(w.functor)
    eng = sia.SdpEngine(w.desc(), w.pmf, custom_source=src, custom_params=prm)
    eng.solve()
    builtin = sia.SdpEngine(w.desc(), w.pmf)
    builtin.solve()
    V, pol, cells = oracle.Problem(w.desc(), w.pmf).solve()
    _tables_equal(eng, V, pol, f"{w.name} custom")
    _tables_equal(builtin, V, pol, f"{w.name} builtin")
    assert eng.stats().cells_evaluated == cells == builtin.stats().cells_evaluated
    for period in (1, w.T):
        assert np.array_equal(eng.reachable(period), builtin.reachable(period))
    eng.close()
    builtin.close()


def _overdraft_limit_case(sia, T=4):
    """CashOverdraftLimit.main's shape on a small box: cash in integers (`/ 10` long division), overhead per
    period, interest 10 % on a negative balance before revenue, no deposit interest."""
    shape = sia.OverdraftFunctor(price=6, fixOrderCost=2, variCost=1, salvageValue=0.5, maxOrderQuantity=14,
                                 minInventoryState=0, maxInventoryState=18, minCashState=-40, maxCashState=120,
                                 cashRoundMult=10.0, cashRoundDiv=10.0, cashRoundIntDiv=True, iniInventory=0,
                                 iniCash=10)
    overhead = [9.0, 12.0, 7.0, 10.0][:T]
    params = [6, 2, 1, 0.25, 0.1, 0.0, 0.5, 14, 0, 18, -40, 120] + overhead
    pmf = cases._pmf([4, 6, 3, 5][:T], 10)
    return shape, params, pmf


@pytest.mark.parametrize("source", ["OVERDRAFT_LIMIT", "OVERDRAFT_LIMIT_FUSED", "OVERDRAFT_LIMIT_LDIV", "OVERDRAFT_LIMIT_FUSED_LDIV"],
                         ids=["three-functions", "fused-sdp_cell", "three-functions-sdp_ldiv", "fused-sdp_ldiv"])
def test_driver_outside_the_builtin_families(sia, oracle, source):
    """CashOverdraftLimit's lambdas as user text, written as the reference's three lambdas and with the fused per-cell callback
    (ABI 5: `#define SDP_USER_CELL 1` + sdp_cell, one evaluation of the increment per cell): tables, reachable sets, off-grid
    evaluations and the memoised recursion's root value all match the oracle running the SAME text compiled for the host."""
    shape, params, pmf = _overdraft_limit_case(sia)
    T = len(pmf)
    desc = shape.to_desc(T, sia.OptDirection.MAX)
    desc.discount_factor = 0.98
    text = getattr(cs, source)
    eng = sia.SdpEngine(desc, pmf, custom_source=text, custom_params=params)
    eng.solve()
    P = oracle.Problem(desc, pmf)
    with oracle.custom_functor(text, params):
        V, pol, cells = P.solve(nthreads=4)
        m = P.memo()
        reach = P.reachable()
        xs, cs_, _ = P.state_arrays(2)
        pick = np.arange(0, len(xs), 97)
        ov, oa = P.eval_states(2, V[2], xs[pick], cs_[pick] + 0.37, None)
    _tables_equal(eng, V, pol, "overdraft-limit")
    assert eng.stats().cells_evaluated == cells
    for period in range(1, T + 1):
        assert np.array_equal(eng.reachable(period), reach[period - 1])
    gv, ga = eng.eval_states(2, xs[pick], cs_[pick] + 0.37)
    assert np.array_equal(gv, ov) and np.array_equal(ga, oa)
    i0 = eng.state_index(1, 0.0, 10.0)
    assert eng.values(1)[i0] == m["value"] and eng.policy(1)[i0] == m["action"]
    if source.endswith("FUSED"):  # ... and the fused text gives the three-function text's tables
        with sia.SdpEngine(desc, pmf, custom_source=cs.OVERDRAFT_LIMIT, custom_params=params) as plain:
            plain.solve()
            for period in range(1, T + 1):
                assert np.array_equal(plain.values(period), eng.values(period)) and np.array_equal(plain.policy(period), eng.policy(period))
    # the built-in OVERDRAFT family (CashOverdraft.java's piecewise schedule) is a different model
    other = sia.SdpEngine(desc, pmf, [9.0, 12.0, 7.0, 10.0])
    other.solve()
    assert not np.array_equal(other.values(1), V[0])
    eng.close()
    other.close()


def test_mirror_class_over_user_lambdas(sia, oracle):
    """CashRecursion with the driver's own lambdas on both sides: Python callables for the host mirror, device
    text for the engine; validateFunctor cross-checks the two on sampled cells through the GPU tables."""
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
    P = oracle.Problem(shape.to_desc(T, sia.OptDirection.MAX), pmf)
    with oracle.custom_functor(cs.OVERDRAFT_LIMIT, params):
        m = P.memo()
    assert rec.getExpectedValue(ini) == m["value"] and rec.getAction(ini) == m["action"]
    assert rec.getOptTable().shape == (m["n"], 4)
    # host lambdas == device text, cell by cell, on the successor the GPU tables were built from
    s1 = trans(ini, rec.getAction(ini), float(pmf[0][3][0]))
    order = {(int(p), x, c): v for p, x, c, v in zip(m["period"], m["x"], m["cash"], m["values"])}
    assert rec.getExpectedValue(s1) == order[(2, s1.getIniInventory(), s1.getIniCash())]


@pytest.mark.parametrize("env", [{"SDPGPU_CUSTOM_NNAN": "0"}, {"SDPGPU_CUSTOM_BAKE": "0"}], ids=["honor-nans", "not-baked"])
def test_compile_modes_give_the_same_tables(sia, oracle, env, monkeypatch):
    """The generated source with the grid and the user's constants baked in and NaN-free arithmetic assumed (the default on a
    clamped grid: `x > c ? c : x` against a non-zero constant becomes one v_min_f64), with NaNs honoured, and with everything
    read at run time: the same tables, bit for bit, for a built-in family as text and for CashOverdraftLimit's lambdas -- and for one F5 and
    one F6 instance as text: the folded three-axis index ((iq * NX + ix) * NC + ic) and the survival arm, baked against not baked."""
    w = cases.f1_clsp_main()
    shape, params, pmf = _overdraft_limit_case(sia)
    desc = shape.to_desc(len(pmf), sia.OptDirection.MAX)
    more = [cases.f5_cash_leadtime(), cases.f6_survival_gamma()]
    handles = [(w.desc(), w.pmf, None, cs.BACKORDER, _params_backorder(w.functor)), (desc, pmf, None, cs.OVERDRAFT_LIMIT, params)]
    handles += [(m.desc(), m.pmf, m.overhead(), *cs.cash_text(m)) for m in more]

    def tables():
        out = []
        for d, pm, oh, src, prm in handles:
            e = sia.SdpEngine(d, pm, oh, custom_source=src, custom_params=prm)
            e.solve()
            out.append([(e.values(t).copy(), e.policy(t).copy()) for t in range(1, len(pm) + 1)])
            e.close()
        return out

    default = tables()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    other = tables()
    assert len(default) == len(other) == 4
    for a, b in zip(default, other):
        assert len(a) == len(b) > 0
        for (va, pa), (vb, pb) in zip(a, b):
            assert np.array_equal(va, vb) and np.array_equal(pa, pb)
    for got, m in zip([default[0]] + default[2:], [w] + more):
        V, pol, _ = oracle.Problem(m.desc(), m.pmf, m.overhead()).solve()
        assert len(got) == len(V)
        for t, (va, pa) in enumerate(got):
            assert np.array_equal(va, V[t]) and np.array_equal(pa, pol[t]), m.name


def test_transition_that_leaves_the_grid_is_reported(sia):
    w = cases.f1_small()
    eng = sia.SdpEngine(w.desc(), w.pmf, custom_source=cs.BROKEN_TRANSITION, custom_params=_params_backorder(w.functor))
    with pytest.raises(sia.SdpgpuError, match="not a grid point"):
        eng.solve()
    with pytest.raises(sia.SdpgpuError, match="host"):
        eng.simulate(np.zeros((1, w.T)), np.ones(w.T), 0.0)
    eng.close()


def test_random_instances_as_user_text(sia, oracle):
    """Seeded random backorder / lead-time instances (tests/test_gpu_fuzz.py) restated as user text: the hipRTC path
    must give the oracle's tables whatever the parameters, the direction and the PMF support look like.  Unclamped seeds run the
    unclamped texts: per-period grids grown from the initial state, nothing baked, P.cur != P.next in c_next_index."""
    import test_gpu_fuzz as tf
    done = unclamped = 0
    for family, src, loose in ((1, cs.BACKORDER, cs.BACKORDER_UNCLAMPED), (2, cs.LEADTIME, cs.LEADTIME_UNCLAMPED)):
        for seed in range(24):
            w = tf.make_instance(family, seed)
            f = w.functor
            if getattr(f, "leadTime", 1) != 1:
                continue  # the pipeline shape is built in: sdpgpu_create_custom refuses lead time 2
            if not f.clampInventory:
                src_, unclamped = loose, unclamped + 1
            else:
                src_ = src
            eng = sia.SdpEngine(w.desc(), w.pmf, custom_source=src_, custom_params=_params_backorder(f))
            eng.solve()
            V, pol, cells = oracle.Problem(w.desc(), w.pmf).solve()
            _tables_equal(eng, V, pol, w.name)
            assert eng.stats().cells_evaluated == cells
            eng.close()
            done += 1
    # by the generator: 48 seeds, 11 of them lead time 2, 14 unclamped -- the old bound of 20 clamped instances plus those 14
    assert unclamped == 14 and done == 37 and done >= 20 + 14


# ---------------------------------------------------------------------------------------------------------------
# The LEVEL SHAPE (round 4): a text that declares `#define SDP_SHAPE_LEVEL 1` and defines sdp_action_cost / sdp_level_cost runs on
# the library's F1 window kernel from per-period tables its own compiled functions fill (include/sdpgpu.h)
# ---------------------------------------------------------------------------------------------------------------
# period-dependent piecewise costs in the manner of CLSPforDraw's second Recursion (CLSPforDraw.java:146-169: period-1-special
# lambdas): a fixed cost that period 1 waives, a holding cost with a kink, a penalty that doubles beyond a backlog
LEVEL_PIECEWISE = r"""
#define SDP_SHAPE_LEVEL 1
__device__ double sdp_action_cost(const sdp_ctx& c, double action) {
  double fixedCost = (action > 0 && c.period > 1) ? c.params[0] : 0;
  double variableCost = action > c.params[4] ? c.params[1] * c.params[4] + 0.75 * c.params[1] * (action - c.params[4]) : c.params[1] * action;
  return fixedCost + variableCost;
}
__device__ double sdp_level_cost(const sdp_ctx& c, double level) {
  double hold = level > 10 ? c.params[2] * 10 + 1.5 * c.params[2] * (level - 10) : c.params[2] * sdp_max(level, 0);
  double pen = level < -6 ? c.params[3] * 6 + 2 * c.params[3] * (-level - 6) : c.params[3] * sdp_max(-level, 0);
  return (hold + pen) * (c.period == c.T ? 0.5 : 1.0);
}
"""


def _level_eng(sia, w, text, params, kernel=0):
    d = w.desc()
    d.kernel = kernel
    return sia.SdpEngine(d, w.pmf, custom_source=text, custom_params=params)


@pytest.mark.parametrize("make", [cases.f1_small, cases.f1_max, cases.f1_clsp_main, cases.f1_gapped, cases.f1_unclamped],
                         ids=lambda f: f.__name__)
def test_level_shape_clsp_text_equals_the_builtin_family(sia, oracle, make):
    """CLSP's lambdas as a text of the level shape: the window kernel reads the user's tabulated costs and gives the built-in
    family's tables (and the oracle's) bit for bit; so does the generic loop around the same text (kernel = GATHER)."""
    from stochastic_inventory_amd import workloads
    w = make()
    prm = _params_backorder(w.functor)
    V, pol, cells = oracle.Problem(w.desc(), w.pmf).solve()
    for kernel, used in ((0, 2), (1, 1)):
        eng = _level_eng(sia, w, workloads.CLSP_LAMBDAS_LEVEL_HIP, prm, kernel)
        eng.solve()
        _tables_equal(eng, V, pol, f"{w.name} level shape, kernel {kernel}")
        assert eng.stats().kernel_used == used and eng.stats().cells_evaluated == cells
        eng.close()
    with oracle.custom_functor(workloads.CLSP_LAMBDAS_LEVEL_HIP, prm, level=w.desc()):  # the same text compiled for the host
        V2, pol2, _ = oracle.Problem(w.desc(), w.pmf).solve()
    for a, b in zip(V, V2):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("make", [cases.f1_small, cases.f1_clsp_main, cases.f1_gapped], ids=lambda f: f.__name__)
def test_level_shape_piecewise_costs_match_the_oracles_host_compile(sia, oracle, make):
    """Piecewise, period-dependent costs no built-in family has: window kernel from tables, generic loop, and the oracle running
    the SAME text compiled for the host -- bit-identical tables; off-grid evaluations and the reachable set as well."""
    w = make()
    f = w.functor
    prm = [f.fixedOrderingCost, f.variOrderingCost, f.holdingCost, f.penaltyCost, 3.0]
    with oracle.custom_functor(LEVEL_PIECEWISE, prm, level=w.desc()):
        P = oracle.Problem(w.desc(), w.pmf)
        V, pol, cells = P.solve()
        win = _level_eng(sia, w, LEVEL_PIECEWISE, prm, 0)
        win.solve()
        gen = _level_eng(sia, w, LEVEL_PIECEWISE, prm, 1)
        gen.solve()
        _tables_equal(win, V, pol, f"{w.name} piecewise, window")
        _tables_equal(gen, V, pol, f"{w.name} piecewise, generic")
        assert win.stats().kernel_used == 2 and gen.stats().kernel_used == 1
        assert np.array_equal(win.reachable(1), gen.reachable(1)) and np.array_equal(win.reachable(w.T), gen.reachable(w.T))
        x = np.array([f.minInventory - 7.0, f.maxInventory + 3.0])  # beyond the grid: getExpectedValue on such a state
        for period in (1, w.T):
            v_next = win.values(period + 1) if period < w.T else None
            gv, ga = win.eval_states(period, x)
            ov, oa = P.eval_states(period, v_next, x)
            assert np.array_equal(gv, ov) and np.array_equal(ga, oa)
        win.close()
        gen.close()


def test_level_shape_cfg2_full_width(sia, oracle):
    """configs[1] at full width (1e4 x 200 x 100, six periods) through the level-shape text: every table equals the built-in
    family's, which is bit-identical to the oracle (tests/test_gpu_parity.py)."""
    from stochastic_inventory_amd import workloads
    w = workloads.custom_clsp_level(T=6)
    eng = sia.SdpEngine(w.desc(), w.pmf, custom_source=w.custom_source, custom_params=w.custom_params)
    eng.solve()
    ref = sia.SdpEngine(w.desc(), w.pmf)
    ref.solve()
    assert eng.stats().kernel_used == 2
    for period in range(1, w.T + 1):
        assert np.array_equal(eng.values(period), ref.values(period)) and np.array_equal(eng.policy(period), ref.policy(period))
    eng.close()
    ref.close()


def test_level_shape_needs_the_backorder_family(sia):
    w = cases.f3_grid_prices()
    from stochastic_inventory_amd import workloads
    with pytest.raises(sia.SdpgpuError, match="SDP_SHAPE_LEVEL"):
        sia.SdpEngine(w.desc(), w.pmf, custom_source=workloads.CLSP_LAMBDAS_LEVEL_HIP, custom_params=[1, 1, 1, 1, 0, 0, 0])


# ---------------------------------------------------------------------------------------------------------------
# The built-in CASH families as user text (tests/custom_sources.py: CASH, OVERDRAFT, CASH_LEADTIME, SURVIVAL).  tests/
# test_custom_functor.py proves on the CPU that the texts restate the families; a mismatch here is the engine's
# (csrc/sdp_custom_src.hpp: custom_period_body, c_next_index, c_decode, sdp_custom_reach)
# ---------------------------------------------------------------------------------------------------------------
FUZZ_CHUNK = 5  # instances per test case (one hipRTC compile each)


def _fuzz_chunks():
    return [pytest.param(family, first, id=f"f{family}-seeds-{first}-{min(first + FUZZ_CHUNK, 16 if family == 5 else 40) - 1}")
            for family in (3, 4, 5, 6) for first in range(0, 16 if family == 5 else 40, FUZZ_CHUNK)]


@pytest.mark.parametrize("family,first", _fuzz_chunks())
def test_cash_family_fuzz_instances_as_user_text(sia, oracle, family, first):
    """The seeds of test_gpu_fuzz.test_random_instances_bit_exact, families 3-6: user-text handle == built-in handle (automatic
    kernel) == oracle, per period: values, policy and the reachable set; the cell counts of the three as well.  Among them
    (counted on the CPU: tests/test_custom_functor.py::test_fuzz_seeds_cover_the_loop_variants) are
    the `!SDP_CASH_INT_DIV` branch (tenths and halves in doubles), a cash shape under MIN, both F3 formulas, the three-axis index
    of F5 and both arms of the survival loop with the `nc < 0` skip of sdp_custom_reach."""
    for w, text, prm in fuzz_text_instances(family)[first:first + FUZZ_CHUNK]:
        P = oracle.Problem(w.desc(), w.pmf, w.overhead())
        V, pol, cells = P.solve(nthreads=4)
        reach = P.reachable()
        with sia.SdpEngine(w.desc(), w.pmf, w.overhead(), custom_source=text, custom_params=prm) as eng, \
                sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as builtin:
            eng.solve()
            builtin.solve()
            assert eng.stats().kernel_used == 1, w.name
            assert eng.stats().cells_evaluated == builtin.stats().cells_evaluated == cells, w.name
            for t in range(1, w.T + 1):
                gv, gp, gr = eng.values(t), eng.policy(t), eng.reachable(t)
                assert np.array_equal(gp, builtin.policy(t)) and np.array_equal(gv, builtin.values(t)), f"{w.name} t={t}: built-in handle"
                assert np.array_equal(gp, pol[t - 1]) and np.array_equal(gv, V[t - 1]), f"{w.name} t={t}: oracle"
                assert np.array_equal(gr, builtin.reachable(t)) and np.array_equal(gr, reach[t - 1]), f"{w.name} t={t}: reachable"


@pytest.mark.parametrize("make", [cases.f3_tenths, cases.f4_overdraft, cases.f5_cash_leadtime, cases.f6_survival_gamma],
                         ids=lambda m: m.__name__)
def test_cash_family_texts_off_grid_and_fused(sia, oracle, make):
    """One instance per family: sdpgpu_eval_states on balances between the grid's keys (+0.37) against the built-in oracle's
    eval_states, and the fused SDP_USER_CELL spelling of the text against the three-function spelling."""
    w = make()
    text, prm = cs.cash_text(w)
    fused, _ = cs.cash_text(w, fused=True)
    P = oracle.Problem(w.desc(), w.pmf, w.overhead())
    V, pol, cells = P.solve(nthreads=4)
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead(), custom_source=text, custom_params=prm) as eng, \
            sia.SdpEngine(w.desc(), w.pmf, w.overhead(), custom_source=fused, custom_params=prm) as one:
        eng.solve()
        one.solve()
        _tables_equal(eng, V, pol, f"{w.name} as text")
        for t in range(1, w.T + 1):
            assert np.array_equal(one.values(t), eng.values(t)) and np.array_equal(one.policy(t), eng.policy(t)), f"{w.name} fused t={t}"
        assert eng.stats().cells_evaluated == one.stats().cells_evaluated == cells
        for period in sorted({1, 2, w.T}):
            xs, cash, preq = P.state_arrays(period)
            pick = np.arange(0, len(xs), 53)
            kw = dict(cash=cash[pick] + 0.37)
            if w.desc().family == 5:
                kw["preq"] = preq[pick]
            ov, oa = P.eval_states(period, V[period] if period < w.T else None, xs[pick], **kw)
            for e in (eng, one):
                gv, ga = e.eval_states(period, xs[pick], **kw)
                assert np.array_equal(gv, ov) and np.array_equal(ga, oa), f"{w.name}: off-grid balances, period {period}"


# ---------------------------------------------------------------------------------------------------------------
# A lambda that yields NaN, where include/sdpgpu.h promises Java's answer: with NaNs honoured (SDPGPU_CUSTOM_NNAN=0) and on every
# grid that is not baked.  Java: every comparison with NaN is false, so the action is skipped; +-Double.MAX_VALUE and action 0
# stay if nothing improves (Recursion.java:129-161).  The default baked mode is unspecified: nothing is asserted about it.
# ---------------------------------------------------------------------------------------------------------------
DBL_MAX = 1.7976931348623157e308


def _nan_case(oracle, w):
    """Parameters of cs.BACKORDER_NAN for workload w, from the grid of its LAST period: (a) order 1 * step everywhere, (b) a band
    of four inventory levels a third of the way up, (c) one (state, order, demand) cell near the top."""
    P = oracle.Problem(w.desc(), w.pmf)
    xs = P.state_arrays(w.T)[0]
    band = (float(xs[len(xs) // 3]), float(xs[len(xs) // 3 + 3]))
    cell = (float(xs[-3]), 2.0 * w.functor.stepSize, float(np.asarray(w.pmf[-1])[1, 0]))
    return P, _params_backorder(w.functor) + [1.0 * w.functor.stepSize, band[0], band[1], *cell], band


def _run_nan(sia, oracle, w, text):
    P, prm, band = _nan_case(oracle, w)
    with oracle.custom_functor(text, prm):
        V, pol, cells = P.solve()
    xs = P.state_arrays(w.T)[0]
    inside = (xs >= band[0]) & (xs <= band[1])
    worst = -DBL_MAX if w.direction == sia.OptDirection.MAX else DBL_MAX
    assert inside.sum() == 4 and np.all(V[-1][inside] == worst) and np.all(pol[-1][inside] == 0)  # (the oracle itself)
    assert np.all(np.abs(V[-1][~inside]) < 1e6) and not any(np.isnan(v).any() for v in V)
    with sia.SdpEngine(w.desc(), w.pmf, custom_source=text, custom_params=prm) as eng:
        eng.solve()
        assert eng.stats().kernel_used == 1 and eng.stats().cells_evaluated == cells
        gv, gp = eng.values(w.T), eng.policy(w.T)
        assert np.all(gv[inside] == worst) and np.all(gp[inside] == 0), f"{w.name}: the band of period T"
        for t in range(1, w.T + 1):  # (what +-MAX_VALUE turns into in the earlier periods is whatever the oracle gets)
            assert np.array_equal(eng.policy(t), pol[t - 1]), f"{w.name} t={t}: policy"
            assert np.array_equal(eng.values(t), V[t - 1]), f"{w.name} t={t}: values"


@pytest.mark.parametrize("make", [cases.f1_small, cases.f1_max], ids=["MIN", "MAX"])
def test_nan_lambda_with_nans_honoured(sia, oracle, make, monkeypatch):
    """SDPGPU_CUSTOM_NNAN=0 on a clamped (baked) grid, both directions: every table equals the oracle running the same text."""
    monkeypatch.setenv("SDPGPU_CUSTOM_NNAN", "0")
    _run_nan(sia, oracle, make(), cs.BACKORDER_NAN)


def test_nan_lambda_on_a_grid_that_is_not_baked(sia, oracle):
    """The unclamped text on an unclamped grid (per-period boxes: nothing is baked, NaNs are honoured by default)."""
    _run_nan(sia, oracle, cases.f1_unclamped(), cs.BACKORDER_NAN_UNCLAMPED)
