"""Cash structure tables on the GPU (sdpgpu_cash_g_table, sdpgpu_cash_structure; csrc/sdp_cash_structure.hpp; DESIGN 4 "Cash
structure tables"): a. the G / GA / GB tables of solved handles equal the twin (tests/cash_structure_twin.py) fed the handle's
read-back V_{t+1}, and for period 1 the drivers' own construction (pyref.memo_recursion over the isForDrawGy lambdas); b. the
source-0 structure call equals the host entry point on the read-back tables, and the twin; c. the source-1 call on hand-built
and special-value tables equals the host entry point; d. the refusals; e. one shrunk SingleCrossTesting instance end to end
through the mirror.  Everything by bits (uint64 views), no tolerances."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
import cash_structure_cases as cc  # noqa: E402
import cash_structure_twin as tw  # noqa: E402
import pyref  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = (0, 1, 2)
T = 3


def plain():
    return cases.f3_testing(T)


def holding_penalty():
    w = cases.f3_testing(T)
    w.functor.holdingCost, w.functor.penaltyCost = 1.0, 2.0
    w.name = "f3_testing_h1_pi2"
    return w


def discount_overheads():
    w = cases.f3_testing(T)
    w.functor.discountFactor = 0.9375
    w.functor.overheadCosts = [1.5, 0.5, 2.0]
    w.name = "f3_testing_gamma_overheads"
    return w


MAKERS = (plain, holding_penalty, discount_overheads)
_ids = lambda f: f.__name__  # noqa: E731
_ctx = {}


class Ctx:
    """A solved handle, its read-back value tables, and the twin's whole-grid G tables of every kind and period: computed
    once, shared, never changed."""

    def __init__(self, sia, make):
        self.w = w = make()
        self.f = f = w.functor
        d = w.desc()
        d.device = 0
        self.eng = sia.SdpEngine(d, w.pmf, w.overhead())
        self.eng.solve(sync=True)
        self.V = [self.eng.values(t) for t in range(1, T + 1)]
        x_lo, self.nx, self.nc, _ = self.eng.grid(1)
        assert x_lo == f.minInventoryState == 0 and self.nx == 21 and self.nc == 131
        self.k_lo = int(f.minCashState)
        self.x0, self.c0 = int(f.minInventoryState), int(f.minCashState)
        oh = w.overhead() or [f.overheadCost] * T
        self.G = {}
        for t in range(1, T + 1):
            v_next = self.V[t] if t < T else None
            for kind in KINDS:
                g = tw.g_table(kind, f, T, t, w.pmf[t - 1], float(oh[t - 1]), v_next, self.nc, x_lo, self.k_lo, self.x0, self.nx, self.c0,
                               self.nc)
                g.setflags(write=False)
                self.G[kind, t] = g
        for v in self.V:
            v.setflags(write=False)

    def want(self, kind, t, x_lo, x_hi, c_lo, c_hi):
        return self.G[kind, t][c_lo - self.c0:c_hi - self.c0 + 1, x_lo - self.x0:x_hi - self.x0 + 1]

    def F(self, t, x_lo, x_hi, c_lo, c_hi):
        """V_t on the window, rows = cash."""
        v = self.V[t - 1].reshape(self.nx, self.nc)
        return np.ascontiguousarray(v[x_lo - self.x0:x_hi - self.x0 + 1, c_lo - self.c0:c_hi - self.c0 + 1].T)


@pytest.fixture
def ctx(sia):
    def get(make):
        if make.__name__ not in _ctx:
            _ctx[make.__name__] = Ctx(sia, make)
        return _ctx[make.__name__]
    return get


# windows (x_lo, x_hi, cash_lo, cash_hi) of the 21 x 131 grid (levels 0..20, cash -10..120): the whole grid (three cash blocks of
# 64 lanes, the last ragged; six level blocks of four waves, the last with one); single points inside and at the corners; cash
# lengths 1, 2, 63, 64, 65 and 129; one touching max_cash, min_cash and max_inventory, where clamped successors occur
WHOLE = (0, 20, -10, 120)
WINDOWS = [WHOLE, (7, 7, 13, 13), (0, 0, -10, -10), (20, 20, 120, 120), (3, 9, 5, 5), (3, 9, 5, 6), (0, 4, 0, 62), (0, 4, 0, 63), (2, 6, -3, 61),
           (1, 3, -9, 119), (17, 20, 100, 120), (0, 20, -10, -5), (20, 20, -10, 120)]


# ---- a. the G tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", MAKERS, ids=_ids)
def test_g_tables_equal_the_twin(ctx, make):
    c = ctx(make)
    for t in range(1, T + 1):
        for kind in KINDS:
            for win in WINDOWS:
                got = c.eng.cash_g_table(kind, t, *win)
                want = c.want(kind, t, *win)
                assert cc.same_table(got, want), (c.w.name, t, kind, win, int((cc.bits(got) != cc.bits(want)).sum()))
            # a second read gives the same bits
            assert cc.same_table(c.eng.cash_g_table(kind, t, *WHOLE), c.want(kind, t, *WHOLE))
    # the windows reach clamped successors: some entry of GB at min_cash differs from GA there, and the kinds differ
    assert not cc.same_table(c.G[1, 1], c.G[2, 1]) and not cc.same_table(c.G[0, 1], c.G[1, 1])


@pytest.mark.parametrize("make", MAKERS, ids=_ids)
def test_kind_0_plus_vy_is_the_action_0_sum(ctx, make):
    """The stored G is acc - v*y: one multiply and one subtract after the sum the twin forms with variableCost = 0."""
    c = ctx(make)
    f, oh = c.f, c.w.overhead() or [c.f.overheadCost] * T
    for t in range(1, T + 1):
        got = c.eng.cash_g_table(0, t, *WHOLE)
        for (i, j) in ((0, 0), (23, 7), (130, 20), (64, 3), (65, 20)):
            R, y = float(c.c0 + i), float(c.x0 + j)
            stored = tw.g_entry(0, f, T, t, c.w.pmf[t - 1], float(oh[t - 1]), c.V[t] if t < T else None, c.nc, 0.0, c.k_lo, R, y)
            # the sum itself: the twin's G entry before its last statement, i.e. GA's statements with variableCost = 0
            acc = stored_sum(f, t, c, oh, R, y)
            assert np.float64(acc - f.variCost * y).tobytes() == np.float64(stored).tobytes() == np.float64(got[i, j]).tobytes()


def stored_sum(f, t, c, oh, R, y):
    """The action-0 sum of kind G without the final `- v*y`: a functor with variCost = 0 makes the twin's G return it."""
    g = dataclasses.replace(f, variCost=0.0)
    return tw.g_entry(0, g, T, t, c.w.pmf[t - 1], float(oh[t - 1]), c.V[t] if t < T else None, c.nc, 0.0, c.k_lo, R, y)


def draw_functor(sia, f, kind):
    """The reference's isForDrawGy lambdas, literally (SingleCrossTesting.java:110-144 for G; CashConstraintDraw.java:193-229,
    :264-274 for GB and GA), over the project's CashFunctor for every other period."""

    @dataclasses.dataclass
    class Draw(sia.CashFunctor):
        def immediateValue(self, state, action, randomDemand, T=None):
            if state.getPeriod() != 1:
                return super().immediateValue(state, action, randomDemand, T)
            revenue = self.price * min(state.getIniInventory(), randomDemand)
            fixedCost = 0.0
            variableCost = 0.0 if kind == 0 else self.variCost * state.getIniInventory()
            inventoryLevel = state.getIniInventory() - randomDemand
            holdCosts = self.holdingCost * max(inventoryLevel, 0.0)
            cashIncrement = revenue - fixedCost - variableCost - holdCosts - self._oh(1)
            salValue = self.salvageValue * max(inventoryLevel, 0.0) if state.getPeriod() == T else 0.0
            cashIncrement += salValue
            endCash = state.getIniCash() + cashIncrement
            if endCash < 0:
                cashIncrement += self.penaltyCost * endCash
            return cashIncrement

        def stateTransition(self, state, action, randomDemand, T=None):
            if state.getPeriod() != 1:
                return super().stateTransition(state, action, randomDemand, T)
            nextInventory = max(0.0, state.getIniInventory() - randomDemand)
            nextCash = state.getIniCash() + self.immediateValue(state, action, randomDemand, T)
            if kind == 2:
                nextCash -= self.fixOrderCost
            nextCash = self.maxCashState if nextCash > self.maxCashState else nextCash
            nextCash = self.minCashState if nextCash < self.minCashState else nextCash
            nextInventory = self.maxInventoryState if nextInventory > self.maxInventoryState else nextInventory
            nextInventory = self.minInventoryState if nextInventory < self.minInventoryState else nextInventory
            return sia.CashState(2, nextInventory, self._round_cash(nextCash))

    return Draw(**{fl.name: getattr(f, fl.name) for fl in dataclasses.fields(f)})


@pytest.mark.parametrize("make", MAKERS, ids=_ids)
def test_period_1_equals_the_drivers_second_recursion(sia, ctx, make):
    """A whole second (third) CashRecursion with the special period-1 lambdas, as the drivers build it -- every action of the
    drawn period yields the same sum, so its value is the G entry."""
    c = ctx(make)
    win = (2, 4, 12, 14)
    for kind in KINDS:
        fd = draw_functor(sia, c.f, kind)
        got = c.eng.cash_g_table(kind, 1, *win)
        for i, R in enumerate(range(win[2], win[3] + 1)):
            for j, y in enumerate(range(win[0], win[1] + 1)):
                root, _, _ = pyref.memo_recursion(fd, c.w.pmf, c.w.direction, sia.CashState(1, float(y), float(R)), cash_loop=True,
                                                  gamma=c.f.discountFactor)
                want = root - c.f.variCost * float(y) if kind == 0 else root
                assert np.float64(want).tobytes() == np.float64(got[i, j]).tobytes(), (c.w.name, kind, R, y, want, got[i, j])


# ---- b. source 0 -------------------------------------------------------------------------------------------------------
STRUCT_WINDOWS = [WHOLE, (0, 20, 0, 40), (3, 15, -10, 54), (0, 0, 0, 0), (5, 5, -2, 70), (0, 20, 11, 11)]


@pytest.mark.parametrize("make", MAKERS, ids=_ids)
def test_source_0_equals_the_host_entry_point_and_the_twin(sia, ctx, make):
    cs = sia.cash_structure
    c = ctx(make)
    K, v = c.f.fixOrderCost, c.f.variCost
    for t in (1, 2, 3):
        for win in STRUCT_WINDOWS:
            res = c.eng.cash_structure(cc.ALL, t, *win)
            tables = {"g": c.want(0, t, *win), "ga": c.want(1, t, *win), "gb": c.want(2, t, *win), "f": c.F(t, *win)}
            for name, tab in tables.items():
                assert cc.same_table(res.tables[name], tab), (c.w.name, t, win, name)
            n_r, n_x = tables["g"].shape
            host = cs.run(cc.ALL, n_r=n_r, n_x=n_x, min_cash=win[2], fix_cost=K, vari_cost=v, host=True, **tables)
            cc.compare(res, {k: host.tables[k] for k in ("h", "opt_y", "gagb", "fg")}, host.verdicts, what=(c.w.name, t, win, "host"))
            cc.compare(res, *cc.expected(cc.ALL, tables, float(win[2]), K, v), what=(c.w.name, t, win, "twin"))
            assert res.kernel_ms > 0
    # a single request forms what it needs alone, and copies nothing back when asked not to
    one = c.eng.cash_structure(sia._abi.CSTRUCT_SINGLE_CROSS, 1, *WHOLE, want_tables=False)
    assert one.tables == {} and tw.same_verdict(one.verdicts["single_crossing"], tw.checkSingleCrossing(tw.getH(c.want(0, 1, *WHOLE), -10.0, K, v)))
    # the caller's costs, not the descriptor's
    res = c.eng.cash_structure(cc.ALL, 1, 0, 20, 0, 40, fix_cost=2.5, vari_cost=0.7)
    tables = {"g": c.want(0, 1, 0, 20, 0, 40), "ga": c.want(1, 1, 0, 20, 0, 40), "gb": c.want(2, 1, 0, 20, 0, 40), "f": c.F(1, 0, 20, 0, 40)}
    cc.compare(res, *cc.expected(cc.ALL, tables, 0.0, 2.5, 0.7), what="caller's costs")


# ---- c. source 1 on the device -----------------------------------------------------------------------------------------
SHAPES = (1, 2, 64, 65, 129)


def device(cs, mask, tables, min_cash, K, v, **kw):
    n_r, n_x = next(iter(tables.values())).shape
    return cs.run(mask, n_r=n_r, n_x=n_x, min_cash=min_cash, fix_cost=K, vari_cost=v, device=0, **tables, **kw)


def host(cs, mask, tables, min_cash, K, v, **kw):
    n_r, n_x = next(iter(tables.values())).shape
    return cs.run(mask, n_r=n_r, n_x=n_x, min_cash=min_cash, fix_cost=K, vari_cost=v, host=True, **tables, **kw)


def same_results(a, b, what):
    assert set(a.tables) == set(b.tables), what
    cc.compare(a, b.tables, b.verdicts, what)


@pytest.mark.parametrize("n_r", SHAPES)
def test_source_1_random_and_special_tables_equal_the_host(sia, n_r):
    cs = sia.cash_structure
    for n_x in SHAPES:
        for p, (min_cash, K, v) in enumerate(cc.PARAMS):
            if p % 2 == (n_r + n_x) % 2:  # (half the parameter sets per shape, every set on half the shapes)
                continue
            for tables in (cc.random_tables(31 * n_r + n_x + p, n_r, n_x), cc.special_tables(57 * n_r + n_x + p, n_r, n_x)):
                same_results(device(cs, cc.ALL, tables, min_cash, K, v), host(cs, cc.ALL, tables, min_cash, K, v), (n_r, n_x, min_cash, K, v))


@pytest.mark.parametrize("n_r", SHAPES)
def test_source_1_hand_built_tables_equal_the_host(sia, n_r):
    """The only device coverage of failing single-crossing and passing non-decreasing verdicts: solved handles of this shape
    always cross once and are never non-decreasing."""
    cs = sia.cash_structure
    seen = set()
    for n_x in SHAPES:
        for check, make in cc.HAND_BUILT:
            table, pinned = make()
            big = cc.embed(table, n_r, n_x, check)
            if big is None:
                continue
            got = cs.check_table(check, big, host=False, device=0)
            want = cs.check_table(check, big, host=True)
            assert tw.same_verdict(got, want) and tw.same_verdict(got, cc.TWIN_CHECK[check](big)), (check, make.__name__, n_r, n_x, got, want)
            assert got[:5] == pinned[:5]
            seen.add((check, bool(got[0])))
        # the thresholds, as a caller's table of every slot at once
        t = cc.threshold_table(n_r, n_x)
        tabs = {"h": t, "gagb": t[::-1].copy(), "fg": -t}
        same_results(device(cs, 0x3f8, tabs, 0.0, 1.0, 1.0), host(cs, 0x3f8, tabs, 0.0, 1.0, 1.0), ("thresholds", n_r, n_x))
    if n_r >= 64:
        assert {("single_crossing", False), ("single_crossing", True), ("non_decreasing", True), ("non_decreasing", False),
                ("non_increasing", False)} <= seen


def test_source_1_native_shapes_pin_the_index_on_the_device(sia):
    cs = sia.cash_structure
    for check, make in cc.HAND_BUILT:
        table, pinned = make()
        assert tw.same_verdict(cs.check_table(check, table, host=False, device=0), pinned), (check, make.__name__)


def test_source_1_index_refusal_comes_before_any_table(sia):
    cs = sia.cash_structure
    tables = cc.random_tables(3, 5, 6)
    with pytest.raises(sia.SdpgpuError) as e:
        device(cs, cc.ALL, tables, 12.5, 10.0, 1.0)
    assert e.value.code == 1 and "(i, j, k) = (4, 0, 1)" in e.value.message


# ---- d. refusals -------------------------------------------------------------------------------------------------------
def engine(sia, w):
    d = w.desc()
    d.device = 0
    return sia.SdpEngine(d, w.pmf, w.overhead())


def refused(sia, call, code, text):
    with pytest.raises(sia.SdpgpuError) as e:
        call()
    assert e.value.code == code and text in e.value.message, e.value.message


def test_refused_before_a_solve_and_outside_the_scope(sia):
    ARG, STATE, UNSUP = 1, 2, 4
    with engine(sia, plain()) as eng:
        refused(sia, lambda: eng.cash_g_table(0, 1, 0, 4, 0, 4), STATE, "period 1 has not been solved")
        refused(sia, lambda: eng.cash_structure(cc.ALL, 1, 0, 4, 0, 4), STATE, "period 1 has not been solved")
        # a window outside the grid, fractional origins, bad kind and period: named, before the solve state is looked at
        refused(sia, lambda: eng.cash_g_table(0, 1, 0, 21, 0, 4), ARG, "outside [min_inventory, max_inventory]")
        refused(sia, lambda: eng.cash_g_table(0, 1, -1, 4, 0, 4), ARG, "outside [min_inventory, max_inventory]")
        refused(sia, lambda: eng.cash_g_table(0, 1, 0, 4, -11, 4), ARG, "outside [min_cash, max_cash]")
        refused(sia, lambda: eng.cash_g_table(0, 1, 0, 4, 100, 121), ARG, "outside [min_cash, max_cash]")
        refused(sia, lambda: eng.cash_structure(1, 1, 0, 4, 100, 121), ARG, "outside [min_cash, max_cash]")
        refused(sia, lambda: eng.cash_g_table(0, 1, 0.5, 4.5, 0, 4), ARG, "x_lo = 0.5 is not a whole number")
        refused(sia, lambda: eng.cash_g_table(0, 1, 0, 4, 0.25, 4.25), ARG, "cash_lo = 0.25 is not a whole number")
        refused(sia, lambda: eng.cash_g_table(3, 1, 0, 4, 0, 4), ARG, "kind = 3")
        refused(sia, lambda: eng.cash_g_table(0, 4, 0, 4, 0, 4), ARG, "period = 4")
        refused(sia, lambda: eng.cash_g_table(0, 1, 4, 0, 0, 4), ARG, "n_x = -3")
    for make, text in ((cases.f3_dyadic, "cash_formula = 0"), (cases.f3_xr, "cash_formula = 2"), (cases.f6_survival, "family = 6")):
        with engine(sia, make(3)) as eng:
            refused(sia, lambda: eng.cash_g_table(0, 1, 0, 1, 0, 1), UNSUP, text)
            refused(sia, lambda: eng.cash_structure(1, 1, 0, 1, 0, 1), UNSUP, text)
    w = plain()
    w.functor.stepSize = 2.0
    w.pmf = [np.stack([2.0 * tile[:, 0], tile[:, 1]], axis=1) for tile in w.pmf]  # (demands are multiples of the step)
    with engine(sia, w) as eng:
        refused(sia, lambda: eng.cash_g_table(0, 1, 0, 1, 0, 1), UNSUP, "step = 2")
    w = plain()
    w.functor.cashRoundMult, w.functor.cashRoundDiv, w.functor.cashRoundIntDiv = 10.0, 10.0, False
    with engine(sia, w) as eng:
        refused(sia, lambda: eng.cash_g_table(0, 1, 0, 1, 0, 1), UNSUP, "cash_round_mult = 10")
    # oversize windows, on grids that hold them (nothing is allocated before a solve)
    w = plain()
    w.functor.maxCashState = 70000.0
    with engine(sia, w) as eng:
        refused(sia, lambda: eng.cash_structure(1, 1, 0, 4, 0, 2048), UNSUP, "n_r = 2049 exceeds 2048 points")
        refused(sia, lambda: eng.cash_structure(4, 1, 0, 20, 0, 49999), UNSUP, "exceeds 2048 points")
        refused(sia, lambda: eng.cash_g_table(0, 1, 0, 4, 0, 65536), UNSUP, "n_r = 65537 exceeds 65536 points")
    w = plain()
    w.functor.maxInventoryState, w.functor.maxCashState = 1023.0, 1100.0
    with engine(sia, w) as eng:
        refused(sia, lambda: eng.cash_structure(4, 1, 0, 1023, 0, 1024), UNSUP, "n_r * n_x = 1049600 exceeds 1048576 points")


def test_ping_pong_handle_keeps_two_periods(sia, ctx):
    """store_all_values = 0 with T = 3: V_3 shares its table with V_1 and is gone after the solve -- G_2 is refused, G_1 (from
    V_2) and G_3 (no future term) equal the stored-values handle's."""
    c = ctx(plain)
    w = plain()
    d = w.desc()
    d.device, d.store_all_values = 0, 0
    with sia.SdpEngine(d, w.pmf, w.overhead()) as eng:
        eng.solve(sync=True)
        for kind in KINDS:
            assert cc.same_table(eng.cash_g_table(kind, 1, *WHOLE), c.G[kind, 1])
            assert cc.same_table(eng.cash_g_table(kind, 3, *WHOLE), c.G[kind, 3])
            refused(sia, lambda: eng.cash_g_table(kind, 2, *WHOLE), 2, "needs V_3")
        refused(sia, lambda: eng.cash_structure(1, 2, 0, 20, 0, 40), 2, "needs V_3")
        refused(sia, lambda: eng.cash_structure(4, 3, 0, 20, 0, 40), 2, "F of period 3 is V_3")
        ok = eng.cash_structure(cc.ALL, 1, 0, 20, 0, 40)
        assert cc.same_table(ok.f, c.F(1, 0, 20, 0, 40)) and cc.same_table(ok.gb, c.want(2, 1, 0, 20, 0, 40))
        assert cc.same_table(eng.cash_structure(1, 3, 0, 20, 0, 40).g, c.want(0, 3, 0, 20, 0, 40))


# ---- e. one SingleCrossTesting instance, shrunk, through the mirror -----------------------------------------------------
def test_single_cross_testing_loop_body(sia):
    from stochastic_inventory_amd import workloads
    (w,) = workloads.single_cross_testing(patterns=[1], prices=(5,), max_inventory=40, min_cash=-20, max_cash=200, max_inventorys=12,
                                          window_cash=20)
    minInventorys, maxInventorys, minCash, maxCash = w.window
    assert (minInventorys, maxInventorys, minCash, maxCash) == (0, 12, 0, 30) and w.T == 2
    f = w.functor
    recursion = sia.CashRecursion(sia.OptDirection.MAX, w.pmf, functor=f, discountFactor=1.0, device=0)
    resultTableG, yG = recursion.drawG("G", minInventorys, maxInventorys, minCash, maxCash, period=1)
    assert resultTableG.shape == (31, 13) and yG.shape == (31 * 13, 3)
    assert yG[14].tolist() == [1.0, 1.0, resultTableG[1, 1]] and cc.same_table(yG[:, 2].reshape(31, 13), resultTableG)
    resultH = recursion.getH(resultTableG, minCash, f.fixOrderCost, f.variCost)
    singleCrossing = recursion.checkSingleCrossing(resultH)
    res = recursion.structure(sia.cash_structure.mask_of(["h"], single_crossing=True), minInventorys, maxInventorys, minCash, maxCash)
    assert cc.same_table(res.g, resultTableG) and cc.same_table(res.h, resultH) and res.holds("single_crossing") is singleCrossing
    assert cc.same_table(resultH, tw.getH(resultTableG, float(minCash), f.fixOrderCost, f.variCost))
    assert singleCrossing is bool(tw.checkSingleCrossing(resultH)[0])
    # the table is the twin's, from the handle's V_2
    eng = recursion.engine
    x_lo, nx, nc, _ = eng.grid(2)
    want = tw.g_table(0, f, 2, 1, w.pmf[0], 0.0, eng.values(2), nc, x_lo, int(f.minCashState), 0, 13, 0, 31)
    assert cc.same_table(resultTableG, want)
    assert (resultH > -10.0).any()  # some state prefers ordering: H is not the trivial -K everywhere
