"""sdpgpu_multiv_solve on the GPU against the memoised twin of CashRecursionV (tests/multiv_twin.py), bit for bit: V_1, the
action, y*(1, iniCash); every V state of the twin's memo with its value and levels; every (t, R) row with its y*; `constrained`
exactly where the twin holds an alpha, and that alpha.  The engine solves a superset (it evaluates the alpha line of every
(t, R)): its extra rows are counted, not compared."""
import struct

import numpy as np
import pytest

import multiv_twin as mt

pytestmark = pytest.mark.gpu


def bits(v):
    return struct.pack("<d", float(v) + 0.0)


def check(sia, kw):
    tw, value, action, ystar = mt.drive(kw)
    res = sia.multiv_solve(table=True, **kw)
    T = kw["T"]
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
    # the engine's own rows: at least the twin's, per period
    tv, tr, tp = (mt.per_period(c, T) for c in (tw.cacheActions, tw.cacheYStar, tw.cacheValuesPai))
    assert all(a >= b for a, b in zip(res.statesPerPeriod, tv)) and res.statesPerPeriod[0] == 1
    assert all(a >= b for a, b in zip(res.rPerPeriod, tr))
    assert all(a >= b for a, b in zip(res.entriesPerPeriod, tp))
    # (t, R) rows come in the key order of cacheYStar, V rows in that of cacheActions
    assert res.rtable[:, :2].tolist() == sorted(res.rtable[:, :2].tolist())
    assert res.table[:, [0, 1, 2, 5]].tolist() == sorted(res.table[:, [0, 1, 2, 5]].tolist())
    # run bookkeeping; both forms of the Pi kernel ran
    from stochastic_inventory_amd import _abi
    assert res.cells == sum(e * len(p) for e, p in zip(res.entriesPerPeriod, kw["pmf"])) > 0 and res.gpu_ms > 0
    assert res.forms == _abi.MULTIV_FORMS["SIDE"] | _abi.MULTIV_FORMS["GENERIC"]
    return tw, res


@pytest.mark.parametrize("rounding", ["trunc10", "round"])
def test_instance_d(sia, rounding):
    tw, res = check(sia, mt.instance_d(rounding))
    extra = [a - b for a, b in zip(res.statesPerPeriod, mt.per_period(tw.cacheActions, 3))]
    print(f"instance D {rounding}: states {res.statesPerPeriod} (+{extra} beyond the twin's memo), R {res.rPerPeriod}, "
          f"entries {res.entriesPerPeriod}, cells {res.cells}, {res.gpu_ms:.3f} ms")


@pytest.mark.parametrize("seed", range(24))
def test_random_instances(sia, seed):
    check(sia, mt.random_instance(seed))


@pytest.mark.parametrize("name", ["T1", "Q11", "one_pair", "pairs72", "yr_small"])
def test_named_edges(sia, name):
    kw = mt.edge_instances()[name]
    tw, res = check(sia, kw)
    if name == "T1":
        assert res.statesPerPeriod == [1]
    if name == "pairs72":
        assert all(len(p) == 72 for p in kw["pmf"])
    if name == "yr_small":
        assert res.value == 65.97500000000001 and res.constrained and res.alpha == 0.4000000000000002
        assert res.entriesPerPeriod[1] >= 2220 and res.rPerPeriod[1] >= 37


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
