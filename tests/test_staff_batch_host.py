"""A batch of STAFF-family instances (sdpgpu_batch_* on SDPGPU_FAMILY_STAFF descriptors, include/sdpgpu.h) as far as it goes
without a GPU: the library validates and lays out before it touches a device.  Create-time refusals with instance and field,
the pool of level tables, the refusals between the two kinds of batch, the per-period staff ranges against the oracle's, the
call-order error of a solve, the launch plan, and the WorkforceTesting sweep the batch exists for."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import staff_block_cases as sb  # noqa: E402
import staff_cases  # noqa: E402


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


@pytest.fixture(scope="module")
def staffref():
    from oracle import staffref as m
    m.build()
    return m


def _staff_descs(sia, n, T=3, **kw):
    """n unclamped instances of one shape (hires 0..12 from iniStaffNum 0) with costs of their own, kernel SEPARABLE."""
    arr = (sia.SdpgpuDesc * n)()
    for i in range(n):
        f = sia.StaffFunctor(fixCost=50.0 + i, unitVariCost=20.0, salary=5.0 * (i + 1), unitPenalty=250.0, minStaffNum=[4] * T,
                             maxHireNum=12, clampStaff=False, iniStaffNum=0)
        d = f.to_desc(T)
        d.kernel = sia._abi.KERNEL_SEPARABLE
        for k, v in kw.items():
            setattr(d, k, v)
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(sia.SdpgpuDesc))
    return arr


def _f1_descs(sia, n, T=3):
    arr = (sia.SdpgpuDesc * n)()
    for i in range(n):
        d = sia.desc_defaults()
        d.periods = T
        d.min_inventory, d.max_inventory, d.max_order_quantity = -20.0, 30.0, 12.0
        d.fixed_order_cost, d.unit_order_cost, d.holding_cost, d.penalty_cost = 10.0 + i, 1.0, 1.0, 5.0
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(sia.SdpgpuDesc))
    return arr


def _create(lib, arr, n, ragged=False):
    b = C.c_void_p()
    rc = (lib.sdpgpu_batch_create_ragged if ragged else lib.sdpgpu_batch_create)(arr, n, C.byref(b))
    return rc, b, lib.sdpgpu_batch_last_error(None).decode()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _add(lib, b, table, row_len=None):
    table = np.ascontiguousarray(table, dtype=np.float64)
    tid = C.c_int32(-1)
    rc = lib.sdpgpu_batch_add_level_pmf(b, _dp(table), _ip(row_len) if row_len is not None else None, table.shape[0],
                                        table.shape[1], C.byref(tid))
    return rc, int(tid.value)


@pytest.fixture
def batch3(sia, lib):
    rc, b, err = _create(lib, _staff_descs(sia, 3), 3)
    assert rc == 0 and b.value, err
    yield b
    lib.sdpgpu_batch_destroy(b)


def _err(lib, b):
    return lib.sdpgpu_batch_last_error(b).decode()


def test_create_accepts_separable_staff_descriptors(sia, lib):
    rc, b, err = _create(lib, _staff_descs(sia, 3), 3)
    assert rc == 0 and b.value and err == ""
    assert lib.sdpgpu_batch_num_actions(b, 0) == 13 and lib.sdpgpu_batch_num_actions(b, 3) == -1
    lib.sdpgpu_batch_destroy(b)
    rc, b, _ = _create(lib, _staff_descs(sia, 1), 1)  # n = 1 is legal
    assert rc == 0
    lib.sdpgpu_batch_destroy(b)
    # clamp_inventory = 1 is in scope as well
    rc, b, err = _create(lib, _staff_descs(sia, 2, clamp_inventory=1, min_inventory=0.0, max_inventory=30.0), 2)
    assert rc == 0, err
    assert lib.sdpgpu_batch_num_states(b, 1) == 31
    lib.sdpgpu_batch_destroy(b)


@pytest.mark.parametrize("field,value", [
    ("periods", 4), ("min_inventory", 1.0), ("max_inventory", 31.0), ("max_order_quantity", 13.0), ("clamp_inventory", 0),
    ("ini_inventory", 2.0), ("device", 3), ("store_all_values", 0),
])
def test_create_names_the_instance_and_the_field(sia, lib, field, value):
    arr = _staff_descs(sia, 3, clamp_inventory=1, min_inventory=0.0, max_inventory=30.0, ini_inventory=5.0)
    setattr(arr[2], field, value)  # (every changed descriptor is valid by itself: the mismatch is what must be reported)
    rc, b, err = _create(lib, arr, 3)
    assert rc == 1 and not b.value
    assert "instance 2" in err and field in err, err


def test_create_refuses_an_unsupported_step_and_world_size(sia, lib):
    arr = _staff_descs(sia, 3)
    arr[1].step = 2.0  # (the family counts heads: refused by the descriptor's own validation, with its instance)
    rc, b, err = _create(lib, arr, 3)
    assert rc == 4 and not b.value and "instance 1" in err and "step" in err, err
    arr = _staff_descs(sia, 3)
    arr[2].world_size = 2
    rc, b, err = _create(lib, arr, 3)
    assert rc == 4 and not b.value and "instance 2" in err and "world_size" in err, err


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_only_the_separable_mode_runs_in_a_batch(sia, lib, kernel):
    arr = _staff_descs(sia, 3)
    arr[1].kernel = kernel
    rc, b, err = _create(lib, arr, 3)
    assert rc == 4 and not b.value
    assert "instance 1" in err and "kernel" in err and "separable mode only" in err and "one handle per instance" in err, err


def test_families_do_not_mix_and_ragged_refuses_staff(sia, lib):
    arr = _staff_descs(sia, 3)
    C.memmove(C.byref(arr[2]), C.byref(_f1_descs(sia, 1)[0]), C.sizeof(sia.SdpgpuDesc))
    rc, b, err = _create(lib, arr, 3)
    assert rc == 4 and not b.value and "instance 2" in err and "family" in err, err
    arr = _f1_descs(sia, 3)
    C.memmove(C.byref(arr[1]), C.byref(_staff_descs(sia, 1, clamp_inventory=1, min_inventory=0.0, max_inventory=30.0)[0]),
              C.sizeof(sia.SdpgpuDesc))
    rc, b, err = _create(lib, arr, 3)
    assert rc == 4 and not b.value and "instance 1" in err and "family" in err, err
    for fam in (2, 3, 4, 5, 6):  # every other family is refused as before
        arr = _f1_descs(sia, 2)
        arr[0].family = fam
        rc, b, err = _create(lib, arr, 2)
        assert rc != 0 and not b.value and "instance 0" in err, (fam, err)
    rc, b, err = _create(lib, _staff_descs(sia, 2), 2, ragged=True)
    assert rc == 4 and not b.value and "instance 0" in err and "family" in err, err


def test_add_level_pmf_validates_like_set_level_pmf(sia, lib, batch3):
    b = batch3
    table = sia.staff_level_pmf([0.3], 13)[0]
    rc, tid = _add(lib, b, table)
    assert rc == 0 and tid == 0
    rc, tid = _add(lib, b, table)
    assert rc == 0 and tid == 1
    lens = np.minimum(np.arange(13) + 1, 6).astype(np.int32)
    rc, tid = _add(lib, b, table, lens)
    assert rc == 0 and tid == 2
    bad = lens.copy()
    bad[2] = 4  # row 2 has at most 3 entries
    rc, _ = _add(lib, b, table, bad)
    assert rc == 1 and "row 2" in _err(lib, b)
    rc, _ = _add(lib, b, table[:, :5], lens)  # a row_len above the stride
    assert rc == 1 and "row 5" in _err(lib, b)
    bad = lens.copy()
    bad[4] = 0
    rc, _ = _add(lib, b, table, bad)
    assert rc == 1 and "row 4" in _err(lib, b)
    tid = C.c_int32()
    assert lib.sdpgpu_batch_add_level_pmf(b, None, None, 13, 13, C.byref(tid)) == 1 and "null" in _err(lib, b)
    assert lib.sdpgpu_batch_add_level_pmf(b, _dp(table), None, 13, 13, None) == 1
    assert lib.sdpgpu_batch_add_level_pmf(b, _dp(table), None, 0, 13, C.byref(tid)) == 1
    assert lib.sdpgpu_batch_add_level_pmf(None, _dp(table), None, 13, 13, C.byref(tid)) == 1


def test_use_level_pmf_and_missing_tables(sia, lib, batch3):
    b = batch3
    table = sia.staff_level_pmf([0.3], 13)[0]
    assert _add(lib, b, table) == (0, 0) and _add(lib, b, table) == (0, 1)
    assert lib.sdpgpu_batch_use_level_pmf(b, 0, 0, 2) == 1 and "table 2" in _err(lib, b)
    assert lib.sdpgpu_batch_use_level_pmf(b, 0, 0, -1) == 1
    assert lib.sdpgpu_batch_use_level_pmf(b, 3, 0, 0) == 1 and "instance 3" in _err(lib, b)
    assert lib.sdpgpu_batch_use_level_pmf(b, -2, 0, 0) == 1
    assert lib.sdpgpu_batch_use_level_pmf(b, 0, 3, 0) == 1 and "period index 3" in _err(lib, b)
    assert lib.sdpgpu_batch_use_level_pmf(b, 0, -2, 0) == 1
    # a solve and a plan name the first (instance, period) without a table -- before any device call: this machine has none
    assert lib.sdpgpu_batch_solve(b, 1) == 2
    assert "instance 0" in _err(lib, b) and "period 1" in _err(lib, b)
    assert lib.sdpgpu_batch_use_level_pmf(b, 0, -1, 0) == 0  # every period of instance 0
    assert lib.sdpgpu_batch_solve(b, 1) == 2 and "instance 1" in _err(lib, b) and "period 1" in _err(lib, b)
    assert lib.sdpgpu_batch_use_level_pmf(b, -1, 0, 1) == 0  # period index 0 of every instance
    assert lib.sdpgpu_batch_use_level_pmf(b, 1, 1, 1) == 0
    pl = sia.SdpgpuBatchStaffPlan()
    assert lib.sdpgpu_batch_staff_plan_period(b, 1, C.byref(pl)) == 2
    assert "instance 1" in _err(lib, b) and "period 3" in _err(lib, b)
    assert lib.sdpgpu_batch_use_level_pmf(b, -1, -1, 0) == 0  # everything
    assert lib.sdpgpu_batch_staff_plan_period(b, 1, C.byref(pl)) == 0 and pl.tables == 1


def test_a_good_call_after_a_failed_one_leaves_no_error_text(sia, lib, batch3):
    """Every entry point clears the batch's last error on entry, the forwarded ones included."""
    b = batch3
    table = sia.staff_level_pmf([0.3], 13)[0]
    v = np.zeros(13)
    pl = sia.SdpgpuBatchStaffPlan()
    x_lo, nx, lo, hi = C.c_double(), C.c_int64(), C.c_int64(), C.c_int64()
    failing = [lambda: lib.sdpgpu_batch_values(b, 0, 1, _dp(v), 1), lambda: lib.sdpgpu_batch_solve(b, 1),
               lambda: lib.sdpgpu_batch_staff_plan_period(b, 4, C.byref(pl)), lambda: lib.sdpgpu_batch_period_ms(b, 1),
               lambda: lib.sdpgpu_batch_use_level_pmf(b, 0, 0, 7), lambda: lib.sdpgpu_batch_set_overhead(b, 0, 0, 0.5),
               lambda: lib.sdpgpu_batch_staff_fit_ss(b, 10.0, _dp(v)), lambda: lib.sdpgpu_batch_plan_period(b, 1, None)]
    good = [lambda: lib.sdpgpu_batch_synchronize(b), lambda: lib.sdpgpu_batch_set_profiling(b, 1),
            lambda: lib.sdpgpu_batch_grid(b, 1, 1, C.byref(x_lo), C.byref(nx)), lambda: _add(lib, b, table)[0],
            lambda: lib.sdpgpu_batch_set_overhead(b, 0, 0, 5.0),
            lambda: lib.sdpgpu_batch_staff_reachable(b, 0, 1, C.byref(lo), C.byref(hi))]
    for k, bad in enumerate(failing):
        assert bad() != 0 and _err(lib, b) != ""
        assert good[k % len(good)]() == 0 and _err(lib, b) == ""
    assert (x_lo.value, nx.value, lo.value, hi.value) == (0.0, 1, 0, 0)


def test_set_overhead_takes_integers(sia, lib, batch3):
    b = batch3
    assert lib.sdpgpu_batch_set_overhead(b, 1, 2, 7.0) == 0
    assert lib.sdpgpu_batch_set_overhead(b, 1, 2, 7.5) == 1 and "integer" in _err(lib, b)
    assert lib.sdpgpu_batch_set_overhead(b, 1, 2, float("nan")) == 1
    assert lib.sdpgpu_batch_set_overhead(b, 3, 0, 7.0) == 1 and "instance 3" in _err(lib, b)
    assert lib.sdpgpu_batch_set_overhead(b, 0, 3, 7.0) == 1 and "period index 3" in _err(lib, b)


def _f1_only_calls(sia, lib, b):
    d = np.arange(4, dtype=np.float64)
    p = np.full(4, 0.25)
    out = np.zeros(64)
    iout = np.zeros(64, dtype=np.int32)
    lo, hi = C.c_int32(), C.c_int32()
    pl = sia.SdpgpuBatchPlan()
    cv = (sia.SdpgpuConvexity * 4)()
    u64 = C.c_uint64(1)
    return {
        "sdpgpu_batch_set_pmf": lambda: lib.sdpgpu_batch_set_pmf(b, 0, 0, _dp(d), _dp(p), 4),
        "sdpgpu_batch_plan_period": lambda: lib.sdpgpu_batch_plan_period(b, 1, C.byref(pl)),
        "sdpgpu_batch_simulate": lambda: lib.sdpgpu_batch_simulate(b, 1, _dp(out), 0, None, _dp(out), None),
        "sdpgpu_batch_simulate_sampled": lambda: lib.sdpgpu_batch_simulate_sampled(b, 1, u64, None, _dp(out), None),
        "sdpgpu_batch_simulate_ss": lambda: lib.sdpgpu_batch_simulate_ss(b, 1, _dp(out), 1, _dp(out), 0, None, _dp(out), None),
        "sdpgpu_batch_simulate_ss_sampled": lambda: lib.sdpgpu_batch_simulate_ss_sampled(b, 1, _dp(out), 1, u64, None, _dp(out), None),
        "sdpgpu_batch_set_sampler": lambda: lib.sdpgpu_batch_set_sampler(b, 0, 0, None),
        "sdpgpu_batch_sample_demands": lambda: lib.sdpgpu_batch_sample_demands(b, 0, 1, u64, _dp(out), None),
        "sdpgpu_batch_reachable": lambda: lib.sdpgpu_batch_reachable(b, 0, 1, C.byref(lo), C.byref(hi)),
        "sdpgpu_batch_fit_ss": lambda: lib.sdpgpu_batch_fit_ss(b, 1, _dp(out)),
        "sdpgpu_batch_gy": lambda: lib.sdpgpu_batch_gy(b, 0, 1, _dp(out), 1),
        "sdpgpu_batch_check_convexity": lambda: lib.sdpgpu_batch_check_convexity(b, 0, 0, 1, None, None, None, None, cv),
    }


def test_f1_only_calls_are_refused_on_a_staff_batch(sia, lib, batch3):
    for name, call in _f1_only_calls(sia, lib, batch3).items():
        assert call() == 4, name
        err = _err(lib, batch3)
        assert name in err and "staff family" in err, (name, err)
    assert lib.sdpgpu_batch_simulate_ms(batch3) == -1.0 and "staff family" in _err(lib, batch3)


def test_staff_calls_are_refused_on_an_f1_batch_except_grid(sia, lib):
    rc, b, err = _create(lib, _f1_descs(sia, 2), 2)
    assert rc == 0, err
    try:
        table = sia.staff_level_pmf([0.3], 13)[0]
        tid = C.c_int32()
        pl = sia.SdpgpuBatchStaffPlan()
        calls = {
            "sdpgpu_batch_add_level_pmf": lambda: lib.sdpgpu_batch_add_level_pmf(b, _dp(table), None, 13, 13, C.byref(tid)),
            "sdpgpu_batch_use_level_pmf": lambda: lib.sdpgpu_batch_use_level_pmf(b, 0, 0, 0),
            "sdpgpu_batch_set_overhead": lambda: lib.sdpgpu_batch_set_overhead(b, 0, 0, 4.0),
            "sdpgpu_batch_staff_plan_period": lambda: lib.sdpgpu_batch_staff_plan_period(b, 1, C.byref(pl)),
        }
        for name, call in calls.items():
            assert call() == 4, name
            err = _err(lib, b)
            assert name in err and "backorder family" in err, (name, err)
        x_lo, nx = C.c_double(), C.c_int64()
        assert lib.sdpgpu_batch_grid(b, 1, 3, C.byref(x_lo), C.byref(nx)) == 0
        assert (x_lo.value, nx.value) == (-20.0, 51)
        assert lib.sdpgpu_batch_grid(b, 2, 1, C.byref(x_lo), C.byref(nx)) == 1 and "instance 2" in _err(lib, b)
        assert lib.sdpgpu_batch_grid(b, 0, 4, C.byref(x_lo), C.byref(nx)) == 1 and "period 4" in _err(lib, b)
    finally:
        lib.sdpgpu_batch_destroy(b)


def _case_batch(sia, cases):
    """One StaffBatch of instances given as staff_cases.StaffCase objects: one pool table per (case, period)."""
    descs, tables, use, mins = [], [], [], []
    for c in cases:
        d = c.functor.to_desc(c.T)
        d.kernel = sia._abi.KERNEL_SEPARABLE
        descs.append(d)
        use.append(list(range(len(tables), len(tables) + c.T)))
        tables += [(c.table[t], c.row_len) for t in range(c.T)]
        mins.append(list(c.functor.minStaffNum))
    return sia.StaffBatch(descs, tables, use, mins)


@pytest.mark.parametrize("make", [staff_cases.staff_testing_small, staff_cases.staff_rates, staff_cases.staff_short_rows,
                                  staff_cases.staff_single, sb.growing], ids=lambda f: f.__name__)
def test_grid_is_the_oracles(sia, staffref, make):
    """Clamped: one box.  Unclamped: from [ini, ini], down by the period's longest row less one (never below 0), up by the
    hire limit -- including a start above 0 and rows shorter than y + 1."""
    c = make()
    P = c.oracle_problem(staffref)
    with _case_batch(sia, [c, c]) as b:
        for t in range(1, c.T + 1):
            assert b.grid(1, t) == (float(P.x_lo[t - 1]), int(P.nx[t - 1])), t
        assert int(b._lib.sdpgpu_batch_num_states(b._b, 0)) == int(P.nx[c.T - 1])
        st = b.stats()  # (host arithmetic before a solve: nothing has run)
        assert (st.instances, st.period_launches, st.cells_evaluated, st.window_r, st.lds_bytes) == (2, 0, 0, 0, 0)


def test_grid_of_an_unclamped_start_above_zero(sia, staffref):
    f = sia.StaffFunctor(fixCost=50, unitVariCost=20, salary=5, unitPenalty=250, minStaffNum=[4, 9, 6, 3], maxHireNum=12,
                         clampStaff=False, iniStaffNum=30)
    c = staff_cases.StaffCase("ini30", f, sia.staff_level_pmf([0.3] * 4, 13))
    P = c.oracle_problem(staffref)
    assert int(P.x_lo[1]) == 18  # the lower end moves: 30 - (13 - 1)
    with _case_batch(sia, [c]) as b:
        for t in range(1, 5):
            assert b.grid(0, t) == (float(P.x_lo[t - 1]), int(P.nx[t - 1])), t


def test_unclamped_instances_must_share_their_staff_ranges(sia, lib):
    f = sia.StaffFunctor(fixCost=50, unitVariCost=20, salary=5, unitPenalty=250, minStaffNum=[4, 9], maxHireNum=12,
                         clampStaff=False, iniStaffNum=30)
    a = staff_cases.StaffCase("a", f, sia.staff_level_pmf([0.3] * 2, 13))
    lens = np.minimum(np.arange(13) + 1, 6).astype(np.int32)
    c = staff_cases.StaffCase("c", f, a.table, lens)  # rows of at most 6 entries: period 2 starts at 25, not at 18
    with _case_batch(sia, [a, c]) as b:
        with pytest.raises(sia.SdpgpuError) as e:
            b.plan(1)
        assert e.value.code == 4 and "instance 1" in e.value.message and "period 2" in e.value.message


def _plan_batch(sia, group_sizes, T=2):
    """Instances of staff_testing_small's shape; group g (of group_sizes[g] instances) uses pool table g in every period."""
    c = staff_cases.staff_testing_small(T)
    n = sum(group_sizes)
    descs = []
    for i in range(n):
        d = c.functor.to_desc(T)
        d.kernel = sia._abi.KERNEL_SEPARABLE
        d.fixed_order_cost = 50.0 + i
        descs.append(d)
    tables = [(sia.staff_level_pmf([0.1 + 0.2 * g], 13)[0], None) for g in range(len(group_sizes))]
    use = [[g] * T for g, size in enumerate(group_sizes) for _ in range(size)]
    return sia.StaffBatch(descs, tables, use, [list(c.functor.minStaffNum)] * n), c


@pytest.mark.parametrize("group_sizes", [[1], [5, 1], [4], [3, 3], [9, 2, 4]])
def test_plan_groups_blocks_and_tasks(sia, staffref, group_sizes):
    b, c = _plan_batch(sia, group_sizes)
    P = c.oracle_problem(staffref)
    n = sum(group_sizes)
    with b:
        for t in (1, 2):
            pl = b.plan(t)
            states = int(P.nx[t - 1])
            levels = states + c.functor.maxHireNum
            assert (pl.tables, pl.groups, pl.states, pl.levels, pl.longest_row) == (len(group_sizes), len(group_sizes), states, levels, 13)
            # the instance block from the group sizes alone: where some group fills one, else single instances
            assert pl.r in (1, 2, 4) and (pl.r == 1 or max(group_sizes) >= pl.r)
            if max(group_sizes) == 1:
                assert pl.r == 1
            blocks = sum(-(-size // pl.r) for size in group_sizes)
            assert pl.blocks == blocks and pl.g_tasks == blocks * -(-levels // 64)
            assert pl.scan_workgroups == n * -(-states // 64)
            assert pl.u >= 1


def test_the_kept_instance_block_serves_a_group_that_fills_it(sia):
    """What a group of at least r instances reaches, whatever r the library kept: a lone instance runs r = 1, and if a form
    r > 1 was kept, a group of 4 (the largest block built) runs it."""
    b, _ = _plan_batch(sia, [1])
    with b:
        assert b.plan(1).r == 1
    b, _ = _plan_batch(sia, [4, 1])
    with b:
        kept = b.plan(1).r
    b, _ = _plan_batch(sia, [8])
    with b:
        assert b.plan(1).r == kept and b.plan(2).r == kept


def test_reach_intervals_are_the_handles(sia):
    """StaffRecursionBatch.getOptTable walks the intervals of workforce.staff_reach_intervals: the handle's own (host
    arithmetic behind SdpEngine.reachable), clamped or not, with full and truncated rows."""
    import staff_separable_twin as twin
    from stochastic_inventory_amd.workforce import staff_reach_intervals
    cases = [make() for make in staff_cases.ALL] + twin.fuzz_cases()[:25]
    for c in cases:
        rows = c.table.shape[1]
        lens = np.arange(rows, dtype=np.int64) + 1 if c.row_len is None else np.asarray(c.row_len, dtype=np.int64)
        got = staff_reach_intervals(c.functor, [lens] * c.T)
        with sb.engine(sia, c) as eng:
            for t in range(1, c.T + 1):
                x_lo = int(eng.grid(t)[0])
                idx = np.nonzero(eng.reachable(t))[0]
                assert (x_lo + int(idx[0]), x_lo + int(idx[-1])) == got[t - 1] and len(idx) == idx[-1] - idx[0] + 1, (c.name, t)


def test_workforce_testing_sweep(sia):
    from stochastic_inventory_amd import workloads
    sweep = workloads.workforce_testing_sweep()
    assert len(sweep) == 216
    first = workloads.staff_testing()
    f0, g0 = sweep[0].functor, first.functor
    assert f0 == g0 and sweep[0].T == first.T == 8
    assert sweep[0].level_pmf.shape == first.level_pmf.shape and np.array_equal(sweep[0].level_pmf[3], first.level_pmf[3])
    # the reference's loop order: rate, fixCost, salary, unitPenalty, minStaffNum row (innermost)
    key = [(w.functor.fixCost, w.functor.salary, w.functor.unitPenalty, tuple(w.functor.minStaffNum)) for w in sweep]
    assert key[:108] == key[108:] and len(set(key[:108])) == 108
    assert [k[3][0] for k in key[:4]] == [40, 10, 80, 40] and key[3][3] == (40, 50, 80, 60, 40, 50, 80, 60)
    assert [k[2] for k in key[0:12:4]] == [50, 250, 2200] and [k[1] for k in key[0:36:12]] == [30, 100, 200]
    assert [k[0] for k in key[0:108:36]] == [50, 1000, 2000]
    assert all(w.functor.unitVariCost == 20 and w.functor.maxHireNum == 1000 and not w.functor.clampStaff and
               w.functor.iniStaffNum == 0 for w in sweep)
    # two table buffers, shared by zero-stride views over the periods
    ptrs = {w.level_pmf.__array_interface__["data"][0] for w in sweep}
    assert len(ptrs) == 2 and all(w.level_pmf.strides[0] == 0 for w in sweep)
    assert len({w.level_pmf.__array_interface__["data"][0] for w in sweep[:108]}) == 1
    # StaffRecursionBatch maps them to a pool of 2, and the whole sweep plans as 2 groups of 108
    rec = sia.StaffRecursionBatch([w.functor for w in sweep], [w.level_pmf for w in sweep], 8)
    try:
        assert rec.num_tables == 2 and len(rec) == 216
        assert [row for row in rec.use[:2]] == [[0] * 8] * 2 and rec.use[108] == [1] * 8
        pl = rec.batch.plan(8)
        assert (pl.tables, pl.states, pl.levels, pl.longest_row) == (2, 7001, 8001, 1001)
        assert pl.blocks == 2 * -(-108 // pl.r) and pl.g_tasks == pl.blocks * 126 and pl.scan_workgroups == 216 * 110
        assert rec.batch.plan(1).states == 1
    finally:
        rec.close()
