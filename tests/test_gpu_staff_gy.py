"""The G(y) rows of the STAFF family on the device (csrc/sdp_staff_structure.hpp, sdpgpu_staff_gy and its neighbours).

Parity statement (include/sdpgpu.h): a device row is BIT-IDENTICAL to sdpgpu_staff_gy_host fed that handle's own V_{period+1}
(one function for the sum of a level, compiled for both sides); a device check is byte for byte sdpgpu_check_convexity on the
read-back row; a batch row is bit for bit sdpgpu_staff_gy on a separable handle of the instance.  That the host entry is the
definition, and how it relates to the reference's drawing recursion, is tests/test_staff_gy_host.py, on the CPU."""
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
import test_staff_gy_host as H  # noqa: E402  (host_gy, off_grid_case)

pytestmark = pytest.mark.gpu

STATE = 2


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


@functools.lru_cache(maxsize=None)
def _case(name):
    return {f.__name__: f for f in staff_cases.ALL}[name]()


def rows131():
    """131 levels: two full waves and a part-filled third; hires 0 .. 8, clamped, T = 2."""
    f = staff_cases.StaffFunctor(fixCost=60, unitVariCost=7, salary=11, unitPenalty=90, minStaffNum=[25, 40], maxHireNum=8, minX=0,
                                 maxX=130, clampStaff=True, iniStaffNum=3)
    return staff_cases.StaffCase("rows131", f, staff_cases.staff_level_pmf([0.35, 0.6], 131))


def _engine(sia, c, kernel=0, **kw):
    d = c.functor.to_desc(c.T)
    d.kernel, d.device = kernel, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _host_row(lib, eng, c, t, y_lo, y_hi):
    """sdpgpu_staff_gy_host on the levels y_lo .. y_hi of period t, fed the handle's own V_{t+1}."""
    v_next, x_lo = (eng.values(t + 1), int(eng.grid(t + 1)[0])) if t < c.T else (None, 0)
    rc, g, err = H.host_gy(lib, c, t, v_next, x_lo, y_lo, y_hi - y_lo + 1)
    assert rc == 0, err
    return g


def _assert_rows(sia, lib, c, kernel):
    with _engine(sia, c, kernel) as eng:
        eng.solve(sync=True)
        for t in range(1, c.T + 1):
            lo, hi = eng.staff_gy_range(t)
            assert (lo, hi) == (0, c.table.shape[1] - 1), (c.name, t)  # (every case keeps all its levels on the grid)
            got = eng.staff_gy(t)
            want = _host_row(lib, eng, c, t, lo, hi)
            assert np.isfinite(got).all(), (c.name, t)
            assert np.array_equal(_bits(got), _bits(want)), (c.name, kernel, t, int(np.count_nonzero(_bits(got) != _bits(want))))


@pytest.mark.parametrize("kernel", [0, 3], ids=["auto", "separable"])
@pytest.mark.parametrize("name", [f.__name__ for f in staff_cases.ALL])
def test_device_rows_are_the_host_entrys_bits(sia, lib, name, kernel):
    _assert_rows(sia, lib, _case(name), kernel)


def test_level_windows(sia, lib):
    c = rows131()
    with _engine(sia, c) as eng:
        eng.solve(sync=True)
        for t in (1, 2):
            full = _host_row(lib, eng, c, t, 0, 130)
            assert np.array_equal(_bits(eng.staff_gy(t)), _bits(full)), t
            for y_lo, n in [(0, 1), (130, 1), (0, 63), (0, 64), (0, 65), (0, 129), (2, 129), (1, 64), (67, 64), (100, 31), (64, 65)]:
                got = eng.staff_gy(t, y_lo, y_lo + n - 1)
                assert np.array_equal(_bits(got), _bits(full[y_lo:y_lo + n])), (t, y_lo, n)
        assert len(eng.staff_gy(1, 5, 4)) == 0  # n = 0: nothing to do


def test_off_grid_levels_are_refused_and_the_rest_served(sia, lib):
    c = H.off_grid_case()
    with _engine(sia, c) as eng:
        eng.solve(sync=True)
        assert eng.staff_gy_range(1) == (5, 9)
        got = eng.staff_gy(1)
        assert np.array_equal(_bits(got), _bits(_host_row(lib, eng, c, 1, 5, 9)))
        with pytest.raises(sia.SdpgpuError) as e:
            eng.staff_gy(1, 4, 9)
        assert e.value.code == 1 and "level 4 of period 1 is off the grid" in e.value.message
        assert np.array_equal(_bits(eng.staff_gy(2)), _bits(_host_row(lib, eng, c, 2, 0, 12)))


def test_ping_pong_handle_serves_g_while_v_next_is_held(sia, lib):
    f = staff_cases.StaffFunctor(fixCost=30, unitVariCost=3, salary=4, unitPenalty=40, minStaffNum=[6, 5, 7, 4, 6], maxHireNum=6, minX=0,
                                 maxX=20, clampStaff=True, iniStaffNum=2)
    c = staff_cases.StaffCase("pingpong5", f, staff_cases.staff_level_pmf([0.4] * 5, 21))
    with _engine(sia, c, store_all_values=0) as eng:
        for t in range(5, 0, -1):
            eng.run_period(t)
            eng.synchronize()
            got = eng.staff_gy(t)  # V_{t+1} is the table just read
            assert np.array_equal(_bits(got), _bits(_host_row(lib, eng, c, t, 0, 20))), t
            if t + 2 <= 5:  # V_{t+2} has just been overwritten by V_t: G_{t+1} is gone
                with pytest.raises(sia.SdpgpuError) as e:
                    eng.staff_gy(t + 1)
                assert e.value.code == STATE and f"needs V_{t + 2}" in e.value.message
        assert len(eng.staff_gy(5)) == 21  # period T reads no V


def _check_host(sia, lib, kind, row, K, capacity):
    conv = sia._abi.SdpgpuConvexity()
    row = np.ascontiguousarray(row, dtype=np.float64)
    assert lib.sdpgpu_check_convexity(kind, row.ctypes.data_as(C.POINTER(C.c_double)), len(row), float(K), int(capacity), C.byref(conv)) == 0
    return bytes(conv)


def test_device_checks_are_the_host_checks_bytes(sia, lib):
    c = rows131()
    with _engine(sia, c) as eng:
        eng.solve(sync=True)
        violations = 0  # of the K = 0 calls alone
        for source, row_of in (("gy", lambda t: eng.staff_gy(t)), ("values", lambda t: eng.values(t))):
            for t in (1, 2):
                row = row_of(t)
                for kind in (0, 1):
                    for K in (float(c.functor.fixCost), 0.0):
                        got = eng.staff_check_convexity(kind, source, t, K=K, capacity=8)
                        assert got.tobytes() == _check_host(sia, lib, kind, row, K, 8), (source, t, kind, K)
                        violations += int(K == 0.0 and got["holds"] == 0)
                # a window with lo > 0
                got = eng.staff_check_convexity(0, source, t, lo=7, hi=99, K=0.0)
                assert got.tobytes() == _check_host(sia, lib, 0, row[7:100], 0.0, 8)
        assert violations > 0  # a K = 0 call found a violation: its first one in loop order was compared above


@functools.lru_cache(maxsize=None)
def _batch_instances():
    """Six instances of one shape over two pooled tables (three each), costs and minStaffNum of their own."""
    T, rows = 3, 70
    tabs = [staff_cases.staff_level_pmf([r] * T, rows) for r in (0.2, 0.55)]
    out = []
    for i in range(6):
        f = staff_cases.StaffFunctor(fixCost=40.0 + 15 * i, unitVariCost=6.0 + i, salary=9.0 + 2 * i, unitPenalty=70.0 + 5 * i,
                                     minStaffNum=[20 + i, 30 - i, 25], maxHireNum=12, minX=0, maxX=rows - 1, clampStaff=True, iniStaffNum=4)
        out.append(staff_cases.StaffCase(f"batch{i}", f, tabs[i % 2]))
    return out


def test_batch_rows_and_checks_are_the_handles(sia, lib):
    cases = _batch_instances()
    T, rows = 3, 70
    want, want_chk = {}, {}
    for i, c in enumerate(cases):
        with _engine(sia, c, 3) as eng:
            eng.solve(sync=True)
            for t in range(1, T + 1):
                want[(i, t)] = eng.staff_gy(t)
                for source in ("gy", "values"):
                    want_chk[(i, t, source)] = eng.staff_check_convexity(0, source, t, K=0.0).tobytes()
    # (one table per rate for every period: zero-stride views over the periods pool to two tables)
    views = [np.broadcast_to(c.table[0], c.table.shape) for c in cases[:2]]
    with sia.StaffRecursionBatch([c.functor for c in cases], [views[i % 2] for i in range(6)]) as rb:
        assert rb.num_tables == 2
        for i in range(6):
            for t in range(1, T + 1):
                got = rb.drawGy(i, 0, rows - 1, t)
                assert got.shape == (rows, 2) and np.array_equal(got[:, 0], np.arange(rows))
                assert np.array_equal(_bits(got[:, 1]), _bits(want[(i, t)])), (i, t)
        assert np.array_equal(_bits(rb.batch.staff_gy(3, 2, 10, 41)), _bits(want[(3, 2)][10:42]))
        for t in range(1, T + 1):
            for source in ("gy", "values"):
                got = rb.checkK(period=t, source=source, fixCost=0.0)
                for i in range(6):
                    assert got[i].tobytes() == want_chk[(i, t, source)], (i, t, source)
        # a re-solve with another minStaffNum drops the kept rows
        before = rb.batch.staff_gy(1, 1, 0, rows - 1)
        rb.batch._check(lib.sdpgpu_batch_set_overhead(rb.batch._b, 1, 0, 33.0))
        rb.batch.solve(sync=True)
        after = rb.batch.staff_gy(1, 1, 0, rows - 1)
        assert not np.array_equal(before, after)
        f2 = staff_cases.StaffFunctor(**{**cases[1].functor.__dict__, "minStaffNum": [33, 29, 25]})
        with _engine(sia, staff_cases.StaffCase("batch1b", f2, cases[1].table), 3) as eng:
            eng.solve(sync=True)
            assert np.array_equal(_bits(after), _bits(eng.staff_gy(1)))


def test_set_overhead_reaches_a_level_rule_rollout_without_a_solve(sia, lib):
    """sdpgpu_batch_set_overhead once the device tables exist: a level-rule rollout needs no solve, and must cost its paths with
    the NEW minStaffNum -- the means of a fresh batch that was given it from the start, bit for bit."""
    cases = _batch_instances()
    views = [np.broadcast_to(c.table[0], c.table.shape) for c in cases[:2]]
    pmfs = [views[i % 2] for i in range(6)]
    ss = np.tile(np.array([[15.0, 30.0]] * 3), (6, 1, 1))
    k = [4, 3, 2]
    with sia.StaffRecursionBatch([c.functor for c in cases], pmfs) as rb:
        rb.batch.solve(sync=True)
        base = rb.simulatesS(ss, k)
        rb.batch._check(lib.sdpgpu_batch_set_overhead(rb.batch._b, 1, 0, 33.0))
        got = rb.simulatesS(ss, k)  # no solve in between
        with pytest.raises(sia.SdpgpuError) as e:  # the tables answer the old value: unsolved until the next solve
            rb.batch.staff_simulate(k, 12345, 4, None)
        assert e.value.code == STATE
        with pytest.raises(sia.SdpgpuError) as e:
            rb.batch.staff_gy(1, 1, 0, 69)
        assert e.value.code == STATE
    functors = [c.functor for c in cases]
    functors[1] = staff_cases.StaffFunctor(**{**cases[1].functor.__dict__, "minStaffNum": [33, 29, 25]})
    with sia.StaffRecursionBatch(functors, pmfs) as fresh:
        want = fresh.simulatesS(ss, k)
    assert np.array_equal(_bits(got), _bits(want))
    assert got[1] != base[1] and np.array_equal(_bits(np.delete(got, 1)), _bits(np.delete(base, 1)))


def test_workforce_planning_draws_and_checks(sia, lib):
    from stochastic_inventory_amd import workloads
    w = workloads.workforce_planning()
    c = staff_cases.StaffCase(w.name, w.functor, w.level_pmf)
    rec = sia.StaffRecursion(pmf=w.level_pmf, functor=w.functor, device=0)
    try:
        yG = rec.drawGy(0, 600)
        assert yG.shape == (601, 2) and np.array_equal(yG[:, 0], np.arange(601.0))
        for t in (1, 2, 3):
            got = rec.engine.staff_gy(t, 0, 600)
            assert np.array_equal(_bits(got), _bits(_host_row(lib, rec.engine, c, t, 0, 600))), t
        assert np.array_equal(_bits(yG[:, 1]), _bits(rec.engine.staff_gy(1, 0, 600)))
        verdict = rec.checkK()
        assert verdict.tobytes() == _check_host(sia, lib, 0, yG[:, 1], w.functor.fixCost, w.functor.maxHireNum)
        with pytest.raises(NotImplementedError):
            rec.getExpectedValue(sia.StaffState(1, 0), 0)
    finally:
        rec.close()
