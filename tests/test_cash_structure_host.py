"""sdpgpu_cash_structure_host -- getH, getMinusGAGB, getMinusFG, checkSingleCrossing, checkNonIncreasing, checkNonDecreasing of
sdp.cash.CashRecursion (CashRecursion.java:227-404) on caller tables, on the host (include/sdpgpu.h) -- against the plain
Python twin of tests/cash_structure_twin.py.  Everything is compared by bits: the integers, and the doubles through their
uint64 views, so NaN and the sign of zero count.  No tolerances.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cash_structure_cases as cc
import cash_structure_twin as tw

SIZES = (1, 2, 3, 17)


@pytest.fixture(scope="module")
def cs(sia):
    import __graft_entry__ as g
    g.build()
    sia._abi.load()
    return sia.cash_structure


def host(cs, mask, tables, min_cash, K, v, **kw):
    n_r, n_x = next(iter(tables.values())).shape
    return cs.run(mask, n_r=n_r, n_x=n_x, min_cash=min_cash, fix_cost=K, vari_cost=v, host=True, **tables, **kw)


def test_abi_symbols_exist(sia):
    lib = sia._abi.load()
    for name in ("sdpgpu_cash_g_table", "sdpgpu_cash_structure", "sdpgpu_cash_structure_host"):
        assert name in sia._abi.EXPORTS and getattr(lib, name) is not None
    # the structs of include/sdpgpu.h, by size: 6 int32 + 4 doubles + 7 pointers; 6 int32 + a double; 8 pointers + 7 verdicts + a double
    assert C.sizeof(sia._abi.SdpgpuCashStructureIn) == 24 + 32 + 56
    assert C.sizeof(sia._abi.SdpgpuCashVerdict) == 32
    assert C.sizeof(sia._abi.SdpgpuCashStructureOut) == 64 + 7 * 32 + 8


@pytest.mark.parametrize("n_x", SIZES)
@pytest.mark.parametrize("n_r", SIZES)
def test_random_tables_equal_the_twin(cs, n_r, n_x):
    for p, (min_cash, K, v) in enumerate(cc.PARAMS):
        tables = cc.random_tables(1000 * n_r + 10 * n_x + p, n_r, n_x)
        res = host(cs, cc.ALL, tables, min_cash, K, v)
        cc.compare(res, *cc.expected(cc.ALL, tables, min_cash, K, v), what=(n_r, n_x, min_cash, K, v))
        # the sources come back as they went in
        for name in ("g", "ga", "gb", "f"):
            assert cc.same_table(res.tables[name], tables[name])


@pytest.mark.parametrize("n_x", SIZES)
@pytest.mark.parametrize("n_r", SIZES)
def test_special_values_equal_the_twin(cs, n_r, n_x):
    """NaN, +-inf, -0.0 and entries exactly at +-0.1 in every source table."""
    for p, (min_cash, K, v) in enumerate(cc.PARAMS):
        tables = cc.special_tables(7000 + 100 * n_r + 10 * n_x + p, n_r, n_x)
        res = host(cs, cc.ALL, tables, min_cash, K, v)
        cc.compare(res, *cc.expected(cc.ALL, tables, min_cash, K, v), what=(n_r, n_x, min_cash, K, v))


def test_the_int_truncations_matter_with_a_non_integer_vari_cost(cs):
    """With variCost = 0.7 the candidates' rows (int)(cash - K - 0.7 (k - j)) and the bound (int)((cash - K) / 0.7) differ from
    their rounded and floored versions on this table -- and the library follows the truncation."""
    n_r, n_x, min_cash, K, v = 17, 17, 0.0, 2.5, 0.7
    tables = cc.random_tables(5, n_r, n_x)
    want, opt = tw.getH(tables["g"], min_cash, K, v, with_index=True)
    res = host(cs, 1, {"g": tables["g"]}, min_cash, K, v)
    assert cc.same_table(res.h, want) and cc.same_table(res.opt_y, opt)
    rows = {tw.java_int(min_cash + i - K - v * m) for i in range(n_r) for m in range(1, n_x)}
    rounded = {int(np.floor(min_cash + i - K - v * m + 0.5)) for i in range(n_r) for m in range(1, n_x)}
    assert rows != rounded and (opt != np.arange(n_x)[None, :]).any()
    # v * (k - j) is not exact: 0.7 * 3 != 2.1
    assert 0.7 * 3 != 2.1


def test_threshold_entries(cs):
    """Entries exactly at -0.1 fail the single crossing's `> -0.1`; neighbours exactly 0.1 apart fail `< 0.1`, exactly -0.1 apart
    fail `> -0.1` -- handed over as caller tables of each slot."""
    t = cc.threshold_table(5, 6)
    assert (t == -0.1).any() and (np.diff(t, axis=1) == 0.1).any() and (np.diff(t, axis=0) == -0.1).any()
    for slot in cc.SLOTS:
        mask = (0x10 | 0x80) << cc.SLOTS.index(slot) | (0x8 if slot == "h" else 0)
        res = host(cs, mask, {slot: t}, 0.0, 1.0, 1.0)
        _, want = cc.expected(mask, {slot: t}, 0.0, 1.0, 1.0, given=(slot,))
        cc.compare(res, {}, want, what=slot)
        assert not res.holds("non_increasing:" + slot) and not res.holds("non_decreasing:" + slot)
    at = np.full((2, 3), 0.0)
    at[1, 1] = -0.1
    assert cs.check_table("single_crossing", at) == (0, 0, 2, 1, 1, -0.1)
    at[1, 1] = np.nextafter(-0.1, 0.0)
    assert cs.check_table("single_crossing", at) == tw.HOLDS


@pytest.mark.parametrize("check,make", cc.HAND_BUILT, ids=[m.__name__ for _, m in cc.HAND_BUILT])
def test_hand_built_tables_pin_the_failing_index(cs, sia, check, make):
    table, want = make()
    assert tw.same_verdict(cc.TWIN_CHECK[check](table), want)  # the twin agrees with the hand count
    got = cs.check_table(check, table)
    assert tw.same_verdict(got, want), (got, want)
    method = {"single_crossing": sia.CashRecursion.checkSingleCrossing, "non_increasing": sia.CashRecursion.checkNonIncreasing,
              "non_decreasing": sia.CashRecursion.checkNonDecreasing}[check]
    assert method(table) is bool(want[0])
    # embedded in a larger table the verdict stays where it was
    big = cc.embed(table, 17, 17, check)
    assert tw.same_verdict(cs.check_table(check, big), cc.TWIN_CHECK[check](big))
    assert cs.check_table(check, big)[:5] == want[:5]


def test_min_cash_above_K_plus_1_is_refused_where_java_would_throw(cs, sia):
    """minCash > K + 1: row i reaches cashIndex = (int)(minCash + i - K - v) >= n_r for the last rows."""
    n_r, n_x, min_cash, K, v = 5, 6, 12.5, 10.0, 1.0
    tables = cc.random_tables(3, n_r, n_x)
    with pytest.raises(tw.IndexOutOfBounds) as java:
        tw.getH(tables["g"], min_cash, K, v)
    i, j, k = java.value.args[0]
    before = np.full((n_r, n_x), 77.0)
    with pytest.raises(sia.SdpgpuError) as e:
        cs.run(1, n_r=n_r, n_x=n_x, min_cash=min_cash, fix_cost=K, vari_cost=v, host=True, g=tables["g"])
    assert e.value.code == 1 and f"(i, j, k) = ({i}, {j}, {k})" in e.value.message and "cashIndex" in e.value.message
    # the other requests of the same call are not written either: found before any table
    lib = sia._abi.load()
    inp, out = sia._abi.SdpgpuCashStructureIn(), sia._abi.SdpgpuCashStructureOut()
    inp.source, inp.mask, inp.n_r, inp.n_x, inp.min_cash, inp.fix_cost, inp.vari_cost = 1, cc.ALL, n_r, n_x, min_cash, K, v
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    inp.g, inp.ga, inp.gb, inp.f = (ptr(tables[n]) for n in ("g", "ga", "gb", "f"))
    out.fg = ptr(before)
    assert lib.sdpgpu_cash_structure_host(C.byref(inp), C.byref(out)) == 1
    assert (before == 77.0).all()
    # minCash = K + 1 exactly still fits: cashIndex = i - (k - j) + 1 - 1... the last row reaches n_r - 1 at most
    res = cs.run(1, n_r=n_r, n_x=n_x, min_cash=K + 1, fix_cost=K, vari_cost=v, host=True, g=tables["g"])
    assert cc.same_table(res.h, tw.getH(tables["g"], K + 1, K, v))


def test_reference_methods_on_the_mirror(sia):
    """The reference's names, arguments and return shapes on recursion.CashRecursion, without an instance or a device."""
    R = sia.CashRecursion
    t = cc.random_tables(11, 6, 7)
    assert cc.same_table(R.getH(t["g"], 0, 10, 1), tw.getH(t["g"], 0.0, 10.0, 1.0))
    assert cc.same_table(R.getMinusGAGB(t["ga"], t["gb"], 0, 2.5, 0.7), tw.getMinusGAGB(t["ga"], t["gb"], 0.0, 2.5, 0.7))
    assert cc.same_table(R.getMinusFG(t["g"], t["f"], 0, 2.5, 0.7), tw.getMinusFG(t["g"], t["f"], 0.0, 2.5, 0.7))
    h3 = R.getH3Column(t["g"], 0, 10, 1)
    assert h3.shape == (42, 3) and cc.same_table(h3, tw.getH3Column(t["g"], 0.0, 10.0, 1.0))
    assert R.checkNonIncreasing(-np.add.outer(np.zeros(3), np.arange(4.0))) is True
    assert R.checkNonDecreasing(cc.nondec_holds()[0]) is True
    assert R.checkSingleCrossing(cc.crossing_holds()[0]) is True
    # lists of lists, as the drivers hold them
    assert R.checkSingleCrossing(cc.crossing_fails()[0].tolist()) is False


def test_refusals(cs, sia):
    t = cc.random_tables(1, 3, 4)

    def refused(code, text, **kw):
        args = dict(n_r=3, n_x=4, min_cash=0.0, fix_cost=10.0, vari_cost=1.0, host=True)
        args.update(kw)
        mask = args.pop("mask", cc.ALL)
        with pytest.raises(sia.SdpgpuError) as e:
            cs.run(mask, **args)
        assert e.value.code == code and text in e.value.message, e.value.message

    refused(1, "mask = 0x0", mask=0, **t)
    refused(1, "mask = 0x400", mask=0x400, **t)
    refused(1, "mask = 0x", mask=-1, **t)
    refused(1, "reads table g, which is null")
    refused(1, "reads table gb, which is null", mask=2, ga=t["ga"])
    refused(1, "reads table f, which is null", mask=4, g=t["g"])
    refused(1, "source = 0", source=0, **t)
    refused(1, "source = 2", source=2, **t)
    lib = sia._abi.load()
    inp, out = sia._abi.SdpgpuCashStructureIn(), sia._abi.SdpgpuCashStructureOut()
    inp.source, inp.mask, inp.n_r, inp.n_x = 1, 1, 0, 4
    assert lib.sdpgpu_cash_structure_host(C.byref(inp), C.byref(out)) == 1 and b"n_r = 0 (at least 1)" in lib.sdpgpu_last_error(None)
    inp.n_r, inp.n_x = 3, -2
    assert lib.sdpgpu_cash_structure_host(C.byref(inp), C.byref(out)) == 1 and b"n_x = -2 (at least 1)" in lib.sdpgpu_last_error(None)
    assert lib.sdpgpu_cash_structure_host(None, C.byref(out)) == 1 and b"in is null" in lib.sdpgpu_last_error(None)
    assert lib.sdpgpu_cash_structure_host(C.byref(inp), None) == 1 and b"out is null" in lib.sdpgpu_last_error(None)
    # beyond the stated limits: unsupported, before anything is read
    inp.n_r, inp.n_x = sia._abi.CSTRUCT_MAX_AXIS + 1, 1
    assert lib.sdpgpu_cash_structure_host(C.byref(inp), C.byref(out)) == 1  # (g is null: named first)
    one = np.zeros(1)
    inp.g = one.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.sdpgpu_cash_structure_host(C.byref(inp), C.byref(out)) == 4 and b"exceeds 2048 points" in lib.sdpgpu_last_error(None)
    # a request succeeds after refusals, and clears the text
    res = cs.run(4, n_r=3, n_x=4, min_cash=0.0, fix_cost=1.0, vari_cost=1.0, host=True, g=t["g"], f=t["f"])
    assert cc.same_table(res.fg, tw.getMinusFG(t["g"], t["f"], 0.0, 1.0, 1.0)) and lib.sdpgpu_last_error(None) == b""
