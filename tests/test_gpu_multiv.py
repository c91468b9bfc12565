"""sdpgpu_multiv_solve on the GPU against the memoised twin of CashRecursionV (tests/multiv_twin.py), bit for bit: V_1, the
action, y*(1, iniCash); every V state of the twin's memo with its value and levels; every (t, R) row with its y*; `constrained`
exactly where the twin holds an alpha, and that alpha.  The engine solves a superset (it evaluates the alpha line of every
(t, R)), and that superset is pinned too: the state set, the R set and the Pi entries of every period equal the forward closure
the header's contract describes (multiv_twin.Closure, built from the twin's lambdas alone), and EVERY row of both tables --
the twin's memo or not -- is compared with the twin evaluated at that row.  No tolerance anywhere."""
import ctypes as C
import struct

import numpy as np
import pytest

import multiv_twin as mt

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_D = -77, -777.25


def bits(v):
    return struct.pack("<d", float(v) + 0.0)


def check(sia, kw):
    """-> (the twin, grown to every row of the engine; the result; the closure; the rows beyond the twin's own memo)."""
    tw, value, action, ystar = mt.drive(kw)
    cl = mt.Closure(kw)
    extra = cl.extra(tw)
    res = sia.multiv_solve(table=True, **kw)
    T = kw["T"]
    periods = range(1, T + 1)
    assert bits(res.value) == bits(value), (res.value, value)
    assert [bits(v) for v in res.action] == [bits(v) for v in action]
    assert [bits(v) for v in res.yStar] == [bits(v) for v in ystar]
    key1 = (1, float(kw["ini_cash"]) + 0.0)
    assert res.constrained == (key1 in tw.cacheAlpha)
    if res.constrained:
        assert bits(res.alpha) == bits(tw.cacheAlpha[key1])
    # every V state of the twin: value and levels
    memo = {(int(r[0]), bits(r[1]), bits(r[2]), bits(r[5])): r for r in res.table.tolist()}
    assert len(memo) == len(res.table) == sum(res.statesPerPeriod)
    for (t, x1, x2, w), ys in tw.cacheActions.items():
        r = memo[(t, bits(x1), bits(x2), bits(w))]
        assert bits(r[6]) == bits(tw.cacheValuesV[(t, x1, x2, w)]), (t, x1, x2, w)
        assert (r[7], r[8]) == ys, (t, x1, x2, w)
    # every (t, R) row of the twin: y*, and alpha exactly where the twin computed one
    rows = {(int(r[0]), bits(r[1])): r for r in res.rtable.tolist()}
    assert len(rows) == len(res.rtable) == sum(res.rPerPeriod)
    for (t, R), ys in tw.cacheYStar.items():
        r = rows[(t, bits(R))]
        assert (r[2], r[3]) == ys, (t, R)
        assert bool(r[4]) == ((t, R) in tw.cacheAlpha), (t, R)
        if r[4]:
            assert bits(r[5]) == bits(tw.cacheAlpha[(t, R)]), (t, R)
    # the engine's own rows: at least the twin's, per period (the reference's memo, before the rows below grow it)
    tv, tr, tp = (mt.per_period(c, T) for c in (tw.cacheActions, tw.cacheYStar, tw.cacheValuesPai))
    assert all(a >= b for a, b in zip(res.statesPerPeriod, tv)) and res.statesPerPeriod[0] == 1
    assert all(a >= b for a, b in zip(res.rPerPeriod, tr))
    assert all(a >= b for a, b in zip(res.entriesPerPeriod, tp))
    # (t, R) rows come in the key order of cacheYStar, V rows in that of cacheActions
    assert res.rtable[:, :2].tolist() == sorted(res.rtable[:, :2].tolist())
    assert res.table[:, [0, 1, 2, 5]].tolist() == sorted(res.table[:, [0, 1, 2, 5]].tolist())
    # the state set, the R set and the Pi entries are the closure's, exactly: no spurious mark, none missing
    want_s = {(t, bits(x1), bits(x2), bits(w)) for p in periods for (t, x1, x2, w) in cl.S[p]}
    assert set(memo) == want_s, (sorted(set(memo) - want_s)[:3], sorted(want_s - set(memo))[:3])
    assert res.statesPerPeriod == [len(cl.S[p]) for p in periods]
    want_r = {(p, bits(R)) for p in periods for R in cl.R[p]}
    assert set(rows) == want_r, (sorted(set(rows) - want_r)[:3], sorted(want_r - set(rows))[:3])
    assert res.rPerPeriod == [len(cl.R[p]) for p in periods]
    # entriesPerPeriod counts the flagged cells of the (R, y1, y2) table AND the alpha line of every R (multiitem.MultiVResult)
    assert res.entriesPerPeriod == [len(cl.E[p]) + 100 * len(cl.R[p]) for p in periods]
    assert res.cells == sum((len(cl.E[p]) + 100 * len(cl.R[p])) * len(kw["pmf"][p - 1]) for p in periods) > 0
    # every V row, the twin's or the engine's own: the twin evaluates any state on demand
    for r in res.table.tolist():
        s = (int(r[0]), r[1] + 0.0, r[2] + 0.0, r[5] + 0.0)
        assert bits(r[6]) == bits(tw.getExpectedValueV(s)), s
        assert (r[7], r[8]) == tw.getAction(s), s
    # every (t, R) row: y*; `constrained` exactly where the twin's getYStar went on to getAlpha, and then that alpha
    for r in res.rtable.tolist():
        k = (int(r[0]), r[1] + 0.0)
        assert (r[2], r[3]) == tw.getYStar(k), k
        assert bool(r[4]) == (k in tw.cacheAlpha), k
        if r[4]:
            assert bits(r[5]) == bits(tw.cacheAlpha[k]), k
    assert cl.covers(tw)
    # run bookkeeping; both forms of the Pi kernel ran
    from stochastic_inventory_amd import _abi
    assert res.cells == sum(e * len(p) for e, p in zip(res.entriesPerPeriod, kw["pmf"])) > 0 and res.gpu_ms > 0
    assert res.forms == _abi.MULTIV_FORMS["SIDE"] | _abi.MULTIV_FORMS["GENERIC"]
    return tw, res, cl, extra


@pytest.mark.parametrize("rounding", ["trunc10", "round"])
def test_instance_d(sia, rounding):
    kw = mt.instance_d(rounding)
    tw, res, cl, extra = check(sia, kw)
    memo = mt.per_period(mt.drive(kw)[0].cacheActions, 3)
    print(f"instance D {rounding}: states {res.statesPerPeriod} (+{[a - b for a, b in zip(res.statesPerPeriod, memo)]} beyond the "
          f"twin's memo), R {res.rPerPeriod}, entries {res.entriesPerPeriod}, cells {res.cells}, {res.gpu_ms:.3f} ms")
    assert extra[0] and len(extra[0]) == sum(res.statesPerPeriod) - sum(memo)


@pytest.mark.parametrize("seed", range(24))
def test_random_instances(sia, seed):
    check(sia, mt.random_instance(seed))


@pytest.mark.parametrize("seed", range(mt.HARD_SEEDS))
def test_hard_instances(sia, seed):
    """Off the inputs on which much of the arithmetic is the identity (multiv_twin.hard_instance; what the 24 seeds reach
    between them is asserted without a device in test_multiv_host.py)."""
    check(sia, mt.hard_instance(seed))


@pytest.mark.parametrize("name", ["T1", "Q11", "one_pair", "pairs72", "yr_small"])
def test_named_edges(sia, name):
    kw = mt.edge_instances()[name]
    tw, res, cl, extra = check(sia, kw)
    if name == "T1":
        assert res.statesPerPeriod == [1]
    if name == "pairs72":
        assert all(len(p) == 72 for p in kw["pmf"])
    if name == "yr_small":
        assert res.value == 65.97500000000001 and res.constrained and res.alpha == 0.4000000000000002
        assert res.entriesPerPeriod[1] >= 2220 and res.rPerPeriod[1] >= 37


@pytest.mark.parametrize("name", mt.HARD_EDGES)
def test_hard_edges(sia, name):
    kw = mt.edge_instances()[name]
    tw, res, cl, extra = check(sia, kw)
    t, x1, x2, w = (res.table[:, c] for c in (0, 1, 2, 5))
    later = t >= 2
    if name == "w0_offset":  # the cash lattice starts at min_cash = 3, not at 0
        assert (kw["min_cash"], kw["max_cash"]) == (3, 9)
        assert (w == 3).any() and (w == 9).any() and ((w >= 3) & (w <= 9)).all()
        assert tw.count["w_lo"] > 0 and tw.count["w_hi"] > 0
    if name == "one_cash_plane":  # nw = 1
        assert kw["min_cash"] == kw["max_cash"] and later.any() and (w[later] == kw["min_cash"]).all()
    if name == "no_stock_kept":  # n1 = 1; e2 is clamped from below only
        assert (kw["max_inventory"], kw["min_inventory"]) == (0, 2)
        assert later.any() and (x1[later] == 0).all() and (x2[later] >= 2).all()
        assert all(s[1] == 0 and s[2] >= 2 for s in cl.S[kw["T"] + 1])
    if name == "blocks_257":  # v_scan_kernel, ystar_kernel and state_ridx_kernel span more than one block
        assert res.statesPerPeriod[2] > 256 and res.rPerPeriod[2] > 256
    if name == "T5_tiny":  # four hand-overs of V_{t+1}
        assert kw["T"] == 5 and kw["max_cash"] <= 12 and len(res.statesPerPeriod) == 5 and min(res.statesPerPeriod[1:]) > 1
    if name.startswith("rounding_ties"):  # y - d sits half way between two lattice points, on integer levels
        assert tw.count["tie"] > 0 and tw.count["tie_inv"] > 0 and tw.count["inv_up"] > 0  # and rounding them is not truncating them


def test_the_mirror_classes(sia):
    """CashRecursionV over the solver: the driver's three questions (MultiItemYR.java:170-181) and the two tables."""
    kw = mt.instance_d("trunc10")
    tw, value, action, ystar = mt.drive(kw)
    functor = {k: v for k, v in kw.items() if k not in ("pmf", "ini_cash", "ini_i1", "ini_i2", "T")}
    rec = sia.CashRecursionV(1.0, kw["pmf"], T=kw["T"], variCost=kw["vari_cost"], functor=functor)
    ini = sia.CashStateMulti(1, 0, 0, 3)
    assert rec.getExpectedValueV(ini) == value and tuple(rec.getAction(ini)) == action
    assert tuple(rec.getYStar(sia.CashStateR(1, 3))) == ystar
    assert rec.getAlpha(sia.CashStateR(1, 3)) == tw.cacheAlpha[(1, 3.0)]
    (t, x1, x2, w), ys = sorted(tw.cacheActions.items())[-1]
    assert rec.getExpectedValueV(sia.CashStateMulti(t, x1, x2, w)) == tw.cacheValuesV[(t, x1, x2, w)]
    free = next(k for k in tw.cacheYStar if k not in tw.cacheAlpha)
    with pytest.raises(KeyError):
        rec.getAlpha(sia.CashStateR(*free))
    c1, c2 = kw["vari_cost"]
    opt = {(int(r[0]), r[1]): r for r in rec.getOptTable().tolist()}
    for (t, R), ys in tw.cacheYStar.items():  # CashRecursionV.java:251-272 over the twin's caches
        cons = c1 * ys[0] + c2 * ys[1] >= R + 0.1
        assert opt[(t, R)] == [t, R, c1, c2, ys[0], ys[1], float(cons), tw.cacheAlpha[(t, R)] if cons else 10000.0]
    det = rec.getOptTableDetail()
    assert det.shape == (sum(rec.result.statesPerPeriod), 13) and set(det[:, 9]) <= {1.0, 2.0, 3.0, 4.0, 5.0}
    assert not np.isnan(det).any()


MIRROR_SEED = 53  # a hard instance (beyond the 24 of test_hard_instances) whose extra (t, R) rows are of both kinds: alpha held, and y* affordable


def test_the_mirror_classes_answer_for_the_extra_rows(sia):
    """The rows the reference's run from iniState would not have visited are no dead output: getExpectedValueV / getAction /
    getYStar / getAlpha / getOptTable hand them out, so they answer as the twin does when asked there."""
    kw = mt.hard_instance(MIRROR_SEED)
    tw, value, action, ystar = mt.drive(kw)
    extra_states, extra_rows = mt.Closure(kw).extra(tw)
    assert extra_states and extra_rows
    functor = {k: v for k, v in kw.items() if k not in ("pmf", "ini_cash", "ini_i1", "ini_i2", "T")}
    rec = sia.CashRecursionV(1.0, kw["pmf"], T=kw["T"], variCost=kw["vari_cost"], functor=functor)
    ini = sia.CashStateMulti(1, kw["ini_i1"], kw["ini_i2"], kw["ini_cash"])
    assert bits(rec.getExpectedValueV(ini)) == bits(value) and tuple(rec.getAction(ini)) == action
    c1, c2 = kw["vari_cost"]
    for s in extra_states:
        assert bits(rec.getExpectedValueV(sia.CashStateMulti(*s))) == bits(tw.getExpectedValueV(s)), s
        assert tuple(rec.getAction(sia.CashStateMulti(*s))) == tw.getAction(s), s
    held = 0
    for k in extra_rows:
        assert tuple(rec.getYStar(sia.CashStateR(*k))) == tw.getYStar(k), k
        if k in tw.cacheAlpha:
            assert bits(rec.getAlpha(sia.CashStateR(*k))) == bits(tw.cacheAlpha[k]), k
            held += 1
        else:
            with pytest.raises(KeyError):
                rec.getAlpha(sia.CashStateR(*k))
    assert 0 < held < len(extra_rows)  # both answers of getAlpha were asked of an extra row
    opt = {(int(r[0]), r[1]): r for r in rec.getOptTable().tolist()}
    for k in extra_rows:
        ys = tw.cacheYStar[k]
        assert opt[k] == [k[0], k[1], c1, c2, ys[0], ys[1], float(k in tw.cacheAlpha), tw.cacheAlpha.get(k, 10000.0)]


def test_a_short_table_is_reported_and_left_alone(sia):
    """include/sdpgpu.h on both tables: `rows` receives the number of rows; nothing is written when it exceeds `capacity`."""
    from stochastic_inventory_amd import _abi
    from stochastic_inventory_amd.multiitem import fill_multiv
    lib = _abi.load()
    kw = mt.instance_d("trunc10")
    T = kw["T"]
    k = fill_multiv(_abi.SdpgpuMultiv(), **kw)

    def solve(vcap, rcap):
        vt, varrs = _abi.make_multi_table(vcap)
        rt, rarrs = _abi.make_multiv_rtable(rcap)
        for a in list(varrs.values()) + list(rarrs.values()):
            a[:] = SENTINEL_I if a.dtype == np.int32 else SENTINEL_D
        out = _abi.SdpgpuMultivResult()
        counts = [(C.c_int64 * T)() for _ in range(3)]
        lib.sdpgpu_multi_set_table(C.byref(vt))
        lib.sdpgpu_multiv_set_rtable(C.byref(rt))
        try:
            rc = lib.sdpgpu_multiv_solve(C.byref(k), C.byref(out), *counts)
        finally:
            lib.sdpgpu_multi_set_table(None)
            lib.sdpgpu_multiv_set_rtable(None)
        scalars = (rc, bits(out.value), out.y1, out.y2, out.ystar1, out.ystar2, out.constrained, bits(out.alpha), out.cells, out.forms,
                   [list(c) for c in counts])
        return scalars, (int(vt.rows), varrs), (int(rt.rows), rarrs)

    def untouched(arrs):
        return all((a == (SENTINEL_I if a.dtype == np.int32 else SENTINEL_D)).all() for a in arrs.values())

    def filled(n, arrs):
        return all(len(a) == n and not (a == (SENTINEL_I if a.dtype == np.int32 else SENTINEL_D)).any() for a in arrs.values())

    full = sia.multiv_solve(table=True, **kw)
    nv, nr = sum(full.statesPerPeriod), sum(full.rPerPeriod)
    assert (nv, nr) == (len(full.table), len(full.rtable)) and nv > 1 and nr > 1
    ref, (rows_v, varrs), (rows_r, rarrs) = solve(nv, nr)
    assert ref[0] == 0 and (rows_v, rows_r) == (nv, nr) and filled(nv, varrs) and filled(nr, rarrs)
    assert ref[1:] == (bits(full.value), *full.action, *full.yStar, int(full.constrained), bits(full.alpha), full.cells, full.forms,
                       [full.statesPerPeriod, full.rPerPeriod, full.entriesPerPeriod])
    for vcap, rcap in ((nv - 1, nr), (nv, nr - 1), (nv - 1, nr - 1), (0, 0)):
        got, (rows_v, varrs), (rows_r, rarrs) = solve(vcap, rcap)
        assert got == ref, (vcap, rcap)  # return code OK, every scalar and count as with full tables
        assert (rows_v, rows_r) == (nv, nr), (vcap, rcap)  # the true counts, so that the caller can size the tables
        assert untouched(varrs) if vcap < nv else filled(nv, varrs), (vcap, rcap)
        assert untouched(rarrs) if rcap < nr else filled(nr, rarrs), (vcap, rcap)
    # the rows as the library writes them (multi_table_rows sorts its copy): (period, R) order, as the header says
    ref, (rows_v, varrs), (rows_r, rarrs) = solve(nv, nr)
    raw = list(zip(rarrs["period"].tolist(), rarrs["R"].tolist()))
    assert raw == sorted(raw) and raw == [(int(r[0]), r[1]) for r in full.rtable.tolist()]
    assert np.array_equal(rarrs["alpha"], full.rtable[:, 5]) and np.array_equal(varrs["value"][np.lexsort(
        (varrs["cash"], varrs["i2"], varrs["i1"], varrs["period"]))], full.table[:, 6])
