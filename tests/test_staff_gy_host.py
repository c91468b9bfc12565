"""The G(y) rows of the STAFF family as far as they go without a GPU (include/sdpgpu.h, "workforce structure rows"):
sdpgpu_staff_gy_host against the plain-float twin on the oracle's tables, the relation to the reference's drawing recursion and
its condition, the V/G identity, and every refusal that comes before a device is touched."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import staff_cases  # noqa: E402
import staff_gy_twin as twin  # noqa: E402

ARG, STATE, UNSUPPORTED = 1, 2, 4
MEETS = ["staff_planning_small", "staff_rates", "staff_short_rows", "staff_wide_actions", "staff_single"]


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


@pytest.fixture(scope="module")
def staffref():
    from oracle import staffref as m
    m.build()
    return m


@functools.lru_cache(maxsize=None)
def _case(name):
    return {f.__name__: f for f in staff_cases.ALL}[name]()


_SOLVED = {}


def _solved(staffref, name):
    """(case, oracle problem, V, policy): computed once, shared, left unchanged."""
    if name not in _SOLVED:
        c = _case(name)
        P = c.oracle_problem(staffref)
        V, pol, _ = P.solve()
        _SOLVED[name] = (c, P, V, pol)
    return _SOLVED[name]


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def host_gy(lib, c, t, v_next, v_x_lo, y_lo, n, out=True):
    """sdpgpu_staff_gy_host for period t (1-based) of case c -> (rc, values, error text)."""
    f = c.functor
    table = np.ascontiguousarray(c.table[t - 1], dtype=np.float64)
    buf = np.full(max(n, 1), np.nan)
    vn = None if v_next is None else np.ascontiguousarray(v_next, dtype=np.float64)
    rc = lib.sdpgpu_staff_gy_host(float(f.unitVariCost), float(f.salary), float(f.unitPenalty), int(f.minStaffNum[t - 1]), _dp(table),
                                  _ip(c.row_len), table.shape[0], table.shape[1], _dp(vn), int(v_x_lo), 0 if vn is None else len(vn),
                                  1 if f.clampStaff else 0, int(f.minX), int(f.maxX), int(y_lo), int(n), _dp(buf) if out else None)
    return rc, buf[:max(n, 0)], lib.sdpgpu_batch_last_error(None).decode()


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", [f.__name__ for f in staff_cases.ALL])
def test_host_entry_is_the_twin_by_bits(lib, staffref, name):
    c, P, V, _ = _solved(staffref, name)
    rows = c.table.shape[1]
    for t in range(1, c.T + 1):
        v_next = V[t] if t < c.T else None
        x_lo = int(P.x_lo[t]) if t < c.T else 0
        rc, got, err = host_gy(lib, c, t, v_next, x_lo, 0, rows)
        assert rc == 0, (name, t, err)
        want = twin.gy_row(c, t, v_next, x_lo)
        assert np.array_equal(_bits(got), _bits(want)), (name, t, int(np.count_nonzero(_bits(got) != _bits(want))))
    # a window with y_lo > 0 is the same entries
    rc, part, _ = host_gy(lib, c, 1, V[1] if c.T > 1 else None, int(P.x_lo[1]) if c.T > 1 else 0, rows // 2, rows - rows // 2)
    assert rc == 0
    assert np.array_equal(_bits(part), _bits(twin.gy_row(c, 1, V[1] if c.T > 1 else None, int(P.x_lo[1]) if c.T > 1 else 0, rows // 2)))


@pytest.mark.parametrize("name", MEETS)
def test_g1_is_the_second_recursion_where_the_condition_holds(lib, staffref, name):
    c, P, V, pol = _solved(staffref, name)
    assert twin.condition(c, pol, P.x_lo), name
    rows = c.table.shape[1]
    rc, got, err = host_gy(lib, c, 1, V[1] if c.T > 1 else None, int(P.x_lo[1]) if c.T > 1 else 0, 0, rows)
    assert rc == 0, err
    want, _ = twin.second_recursion(c)
    assert np.array_equal(_bits(got), _bits(want)), (name, int(np.count_nonzero(_bits(got) != _bits(want))))


def test_the_condition_reports_the_short_table_as_outside(staffref):
    c, P, _, pol = _solved(staffref, "staff_testing_small")
    assert not twin.condition(c, pol, P.x_lo)


@pytest.mark.parametrize("name", ["staff_planning_small", "staff_rates", "staff_short_rows", "staff_wide_actions"])
def test_value_is_the_minimum_over_g(lib, staffref, name):
    """V_t(x) = min_a G_t(x + a) + K [a > 0] - v x over the actions inside the table, to the separable mode's 1e-9 relative."""
    c, P, V, pol = _solved(staffref, name)
    f, rows = c.functor, c.table.shape[1]
    for t in range(1, c.T + 1):
        rc, g, err = host_gy(lib, c, t, V[t] if t < c.T else None, int(P.x_lo[t]) if t < c.T else 0, 0, rows)
        assert rc == 0, err
        checked = 0
        for i, x in enumerate(range(int(P.x_lo[t - 1]), int(P.x_lo[t - 1]) + int(P.nx[t - 1]))):
            a = np.arange(0, min(f.maxHireNum, rows - 1 - x) + 1)
            if len(a) == 0:
                continue
            q = g[x + a] + np.where(a > 0, float(f.fixCost), 0.0) - float(f.unitVariCost) * x
            v = V[t - 1][i]
            assert q.min() >= v - 1e-9 * abs(v), (name, t, x)
            if x + int(pol[t - 1][i]) <= rows - 1:
                assert abs(q.min() - v) <= 1e-9 * abs(v), (name, t, x, q.min(), v)
                checked += 1
        assert checked > 0, (name, t)


def off_grid_case():
    """Unclamped, iniStaffNum 5, rows of at most 3 entries: period 2 stores the staff numbers 3 .. 9, so the levels 0 .. 4 of
    period 1 have a successor below it."""
    rows, T = 13, 2
    full = staff_cases.staff_level_pmf([0.3] * T, rows)
    row_len = np.minimum(np.arange(rows) + 1, 3).astype(np.int32)
    table = np.zeros((T, rows, 3))
    for y in range(rows):
        table[:, y, :row_len[y]] = full[:, y, :row_len[y]]
    f = staff_cases.StaffFunctor(fixCost=50, unitVariCost=20, salary=5, unitPenalty=250, minStaffNum=[4, 6], maxHireNum=4,
                                 clampStaff=False, iniStaffNum=5)
    return staff_cases.StaffCase("off_grid", f, table, row_len)


def test_host_entry_refusals(lib):
    c = _case("staff_planning_small")
    v = np.zeros(31)
    rc, _, err = host_gy(lib, c, 1, v, 0, 30, 2)
    assert rc == ARG and "level 31 is not a row of the table (n_rows = 31" in err
    rc, _, err = host_gy(lib, c, 1, v, 0, 31, 1)
    assert rc == ARG and "level 31" in err
    rc, _, err = host_gy(lib, c, 1, v, 0, 0, -1)
    assert rc == ARG and "n = -1" in err
    rc, _, err = host_gy(lib, c, 1, v, 0, 0, 4, out=False)
    assert rc == ARG and "out is null" in err
    rc, _, err = host_gy(lib, c, 1, v, 0, -1, 2)
    assert rc == ARG and "y_lo = -1" in err
    o = off_grid_case()
    out = np.full(13, 7.0)
    table = np.ascontiguousarray(o.table[0])
    v2 = np.zeros(7)  # the staff numbers 3 .. 9
    rc = lib.sdpgpu_staff_gy_host(20.0, 5.0, 250.0, 4, _dp(table), _ip(o.row_len), 13, 3, _dp(v2), 3, 7, 0, 0, 0, 0, 13, _dp(out))
    err = lib.sdpgpu_batch_last_error(None).decode()
    assert rc == ARG and "level 0 is off the grid: its successor 0 (j = 0)" in err, err
    assert (out == 7.0).all()  # nothing is written
    rc = lib.sdpgpu_staff_gy_host(20.0, 5.0, 250.0, 4, _dp(table), _ip(o.row_len), 13, 3, _dp(v2), 3, 7, 0, 0, 0, 4, 2, _dp(out))
    err = lib.sdpgpu_batch_last_error(None).decode()
    assert rc == ARG and "level 4 is off the grid: its successor 2 (j = 2)" in err, err
    rc = lib.sdpgpu_staff_gy_host(20.0, 5.0, 250.0, 4, _dp(table), _ip(o.row_len), 13, 3, _dp(v2), 3, 7, 0, 0, 0, 9, 2, _dp(out))
    err = lib.sdpgpu_batch_last_error(None).decode()
    assert rc == ARG and "level 10 is off the grid: its successor 10 (j = 0)" in err, err
    rc = lib.sdpgpu_staff_gy_host(20.0, 5.0, 250.0, 4, _dp(table), _ip(o.row_len), 13, 3, _dp(v2), 3, 7, 0, 0, 0, 5, 5, _dp(out))
    assert rc == 0 and np.isfinite(out[:5]).all()


def _engine(sia, c, **kw):
    d = c.functor.to_desc(c.T)
    for k, val in kw.items():
        setattr(d, k, val)
    return sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len)


def _handle_err(lib, eng):
    return lib.sdpgpu_last_error(eng._h).decode()


def test_handle_refusals_come_before_the_device(sia, lib):
    out = np.zeros(64)
    with _engine(sia, off_grid_case()) as eng:
        assert eng.staff_gy_range(1) == (5, 9)
        assert eng.staff_gy_range(2) == (0, 12)  # period T reads no V
        rc = lib.sdpgpu_staff_gy(eng._h, 1, 1, 1, _dp(out))
        assert rc == ARG and "level 1 of period 1 is off the grid: its successor 1 (j = 0) lies outside period 2's staff numbers 3 .. 9" in _handle_err(lib, eng)
        rc = lib.sdpgpu_staff_gy(eng._h, 1, 5, 9, _dp(out))
        assert rc == ARG and "level 13 is not a row of period 1's table" in _handle_err(lib, eng)
        assert lib.sdpgpu_staff_gy(eng._h, 1, 5, -1, _dp(out)) == ARG and "n = -1" in _handle_err(lib, eng)
        assert lib.sdpgpu_staff_gy(eng._h, 1, 5, 2, None) == ARG and "out is null" in _handle_err(lib, eng)
        assert lib.sdpgpu_staff_gy(eng._h, 3, 5, 2, _dp(out)) == ARG and "period = 3" in _handle_err(lib, eng)
        # valid arguments, no solve yet
        assert lib.sdpgpu_staff_gy(eng._h, 1, 5, 5, _dp(out)) == STATE and "has not been solved" in _handle_err(lib, eng)
        conv = sia._abi.SdpgpuConvexity()
        assert lib.sdpgpu_staff_check_convexity(eng._h, 0, 1, 1, 5, 9, 50.0, 4, C.byref(conv)) == STATE
        assert lib.sdpgpu_staff_check_convexity(eng._h, 0, 1, 1, 4, 9, 50.0, 4, C.byref(conv)) == ARG and "off the grid" in _handle_err(lib, eng)
        assert lib.sdpgpu_staff_check_convexity(eng._h, 2, 1, 1, 5, 9, 50.0, 4, C.byref(conv)) == ARG and "kind = 2" in _handle_err(lib, eng)
    with _engine(sia, _case("staff_planning_small")) as eng:
        assert eng.staff_gy_range(1) == (0, 30) and eng.staff_gy_range(3) == (0, 30)  # clamped: no level is off the grid
    with _engine(sia, _case("staff_planning_small"), world_size=2) as eng:
        assert lib.sdpgpu_staff_gy(eng._h, 1, 0, 4, _dp(out)) == UNSUPPORTED and "world_size = 2" in _handle_err(lib, eng)
    d = sia.desc_defaults()
    d.periods = 2
    d.min_inventory, d.max_inventory, d.max_order_quantity = -5.0, 10.0, 4.0
    pmf = [[[0.0, 0.5], [1.0, 0.5]]] * 2
    with sia.SdpEngine(d, pmf) as eng:
        assert lib.sdpgpu_staff_gy(eng._h, 1, 0, 4, _dp(out)) == UNSUPPORTED and "family = " in _handle_err(lib, eng)
        lo, hi = C.c_int32(), C.c_int32()
        assert lib.sdpgpu_staff_gy_range(eng._h, 1, C.byref(lo), C.byref(hi)) == UNSUPPORTED


def test_staff_only_batch_calls_refuse_a_backorder_batch(sia, lib):
    arr = (sia.SdpgpuDesc * 2)()
    for i in range(2):
        d = sia.desc_defaults()
        d.periods = 3
        d.min_inventory, d.max_inventory, d.max_order_quantity = -20.0, 30.0, 12.0
        d.fixed_order_cost = 10.0 + i
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(sia.SdpgpuDesc))
    b = C.c_void_p()
    assert lib.sdpgpu_batch_create(arr, 2, C.byref(b)) == 0
    try:
        out = np.zeros(8)
        conv = (sia._abi.SdpgpuConvexity * 2)()
        assert lib.sdpgpu_batch_staff_gy(b, 0, 1, 0, 4, _dp(out)) == UNSUPPORTED
        assert "sdpgpu_batch_staff_gy: the batch is of the backorder family" in lib.sdpgpu_batch_last_error(b).decode()
        assert lib.sdpgpu_batch_staff_check_convexity(b, 0, 1, 1, None, None, None, None, conv) == UNSUPPORTED
        assert "sdpgpu_batch_staff_check_convexity: the batch is of the backorder family" in lib.sdpgpu_batch_last_error(b).decode()
    finally:
        lib.sdpgpu_batch_destroy(b)


def test_staff_batch_calls_before_a_solve(sia, lib):
    c = _case("staff_planning_small")
    d = c.functor.to_desc(c.T)
    d.kernel = sia._abi.KERNEL_SEPARABLE
    with sia.StaffBatch([d, d], [(c.table[0], None)], [[0] * c.T] * 2, [list(c.functor.minStaffNum)] * 2) as b:
        with pytest.raises(sia.SdpgpuError) as e:
            b.staff_gy(0, 1, 0, 30)
        assert e.value.code == STATE and "before sdpgpu_batch_solve" in e.value.message
        with pytest.raises(sia.SdpgpuError) as e:
            b.staff_check_convexity(0, "gy", 1)
        assert e.value.code == STATE
        with pytest.raises(sia.SdpgpuError) as e:
            b.staff_gy(2, 1, 0, 30)
        assert e.value.code == ARG and "instance 2" in e.value.message
