"""The ragged batch (sdpgpu_batch_create_ragged, include/sdpgpu.h) as far as it goes without a GPU: instances with inventory
bounds and an order limit of their own are accepted, every field that must still agree is refused with instance index and
field, sizes are per instance, the per-period plan (sdpgpu_batch_plan_period: host arithmetic) adds up, forced blocks are
honoured or refused with the planner's reason -- and the sweep the entry point exists for, the 810 instances of
capacitated.fitss.ThreeLevelFitsSTest.main (workloads.fitss_sweep), plans as ONE launch per period."""
import ctypes as C

import numpy as np
import pytest

FITSS_ORDER_LIMITS = [26, 39, 46, 50, 52, 54, 60, 69, 75, 81, 90, 92, 96, 100, 108, 120, 126, 138, 144, 180, 184, 189, 192,
                      216, 240, 252, 288]

# (min_inventory, max_inventory, max_order_quantity): 51 / 1 / 64 / 130 / 700 states, 13 / 1 / 2 / 300 / 31 actions
SHAPES = [(-20.0, 30.0, 12.0), (5.0, 5.0, 0.0), (0.0, 63.0, 1.0), (-129.0, 0.0, 299.0), (-300.0, 399.0, 30.0)]


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


def _descs(sia, shapes=SHAPES, T=3, **kw):
    arr = (sia.SdpgpuDesc * len(shapes))()
    for i, (lo, hi, q) in enumerate(shapes):
        d = sia.desc_defaults()
        d.periods = T
        d.min_inventory, d.max_inventory, d.max_order_quantity = lo, hi, q
        d.ini_inventory = lo  # a point of the instance's OWN grid (0 is not one of [5, 5])
        d.fixed_order_cost, d.unit_order_cost, d.holding_cost, d.penalty_cost = 10.0 + i, float(i % 2), 1.0, 5.0 + i
        for k, v in kw.items():
            setattr(d, k, v)
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(sia.SdpgpuDesc))
    return arr


def _create(lib, arr, n, ragged=True):
    b = C.c_void_p()
    fn = lib.sdpgpu_batch_create_ragged if ragged else lib.sdpgpu_batch_create
    rc = fn(arr, n, C.byref(b))
    return rc, b, lib.sdpgpu_batch_last_error(None).decode()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _tile(D, d0=0.0):
    p = np.arange(1, D + 1, dtype=np.float64)
    return np.stack([d0 + np.arange(D, dtype=np.float64), p / p.sum()], axis=1)


def _ceil(a, b):
    return -(-a // b)


def test_differing_bounds_and_order_limits_are_accepted_only_by_the_ragged_entry_point(sia, lib):
    n = len(SHAPES)
    rc, b, err = _create(lib, _descs(sia), n)
    assert rc == 0 and b.value and err == ""
    try:
        assert [lib.sdpgpu_batch_num_states(b, i) for i in range(n)] == [51, 1, 64, 130, 700]
        assert [lib.sdpgpu_batch_num_actions(b, i) for i in range(n)] == [13, 1, 2, 300, 31]
        assert lib.sdpgpu_batch_num_states(b, n) == -1 and lib.sdpgpu_batch_num_actions(b, -1) == -1
        assert lib.sdpgpu_batch_num_states(None, 0) == -1
    finally:
        lib.sdpgpu_batch_destroy(b)
    rc, b, err = _create(lib, _descs(sia), n, ragged=False)  # sdpgpu_batch_create itself does not change
    assert rc == 1 and not b.value and "instance 1" in err and "min_inventory" in err and "one grid shape" in err
    rc, b, err = _create(lib, _descs(sia), 0)
    assert rc == 1 and "n = 0" in err
    rc, b, err = _create(lib, None, 2)
    assert rc == 1 and "null" in err


@pytest.mark.parametrize("field,value,code", [
    ("periods", 4, 1), ("step", 2.0, 1), ("direction", 1, 1), ("store_all_values", 0, 1), ("device", 3, 1),
    ("family", 2, 4), ("clamp_inventory", 0, 4), ("world_size", 2, 4), ("kernel", 3, 4), ("kernel", 1, 4),
])
def test_create_ragged_names_the_instance_and_the_field_that_must_agree(sia, lib, field, value, code):
    arr = _descs(sia)
    if field == "step":  # (keep instance 2's bounds multiples of the new step: the mismatch is what must be reported)
        arr[2].min_inventory, arr[2].max_inventory, arr[2].max_order_quantity, arr[2].ini_inventory = 0.0, 62.0, 2.0, 0.0
    setattr(arr[2], field, value)
    rc, b, err = _create(lib, arr, len(SHAPES))
    assert rc == code and not b.value
    assert "instance 2" in err and field in err, err


def test_ini_inventory_must_lie_on_the_instances_own_grid(sia, lib):
    arr = _descs(sia)
    arr[3].ini_inventory = 10.0  # a point of instance 0's grid [-20, 30], not of instance 3's [-129, 0]
    rc, b, err = _create(lib, arr, len(SHAPES))
    assert rc == 1 and not b.value and "instance 3" in err and "ini_inventory" in err and "[-129, 0]" in err
    arr = _descs(sia)
    arr[0].ini_inventory = 30.0  # the upper end of its own grid, outside instance 3's
    arr[3].ini_inventory = -129.0
    rc, b, err = _create(lib, arr, len(SHAPES))
    assert rc == 0, err
    lib.sdpgpu_batch_destroy(b)


def test_read_out_is_sized_per_instance(sia, lib):
    rc, b, _ = _create(lib, _descs(sia), len(SHAPES))
    assert rc == 0
    try:
        v = np.zeros(700)
        # argument errors come before the state error: instance 1 has ONE state, instance 4 has 700
        assert lib.sdpgpu_batch_values(b, 1, 1, _dp(v), 2) == 1
        assert b"the grid has 1 states" in lib.sdpgpu_batch_last_error(b)
        assert lib.sdpgpu_batch_values(b, 1, 1, _dp(v), 1) == 2
        assert lib.sdpgpu_batch_values(b, 4, 1, _dp(v), 700) == 2
        assert lib.sdpgpu_batch_values(b, 4, 1, _dp(v), 701) == 1
        assert lib.sdpgpu_batch_values(b, 0, 1, _dp(v), 52) == 1
        # the window's limit of 3500 actions + demand points is the instance's own
        d = np.arange(3300, dtype=np.float64)
        p = np.full(3300, 1.0 / 3300)
        assert lib.sdpgpu_batch_set_pmf(b, 3, 0, _dp(d), _dp(p), 3300) == 4
        assert b"300 actions" in lib.sdpgpu_batch_last_error(b)
    finally:
        lib.sdpgpu_batch_destroy(b)


def _ragged(sia, shapes=SHAPES, T=3, Ds=(7, 33, 64, 2, 130), **kw):
    descs = _descs(sia, shapes, T, **kw)
    pmfs = [[_tile(Ds[(i + t) % len(Ds)], float([-3, 0, 2][(i + t) % 3])) for t in range(T)] for i in range(len(shapes))]
    return sia.SdpBatch([descs[i] for i in range(len(shapes))], pmfs, ragged=True), pmfs


def _expected_tasks(shapes, pl):
    """sum of tiles_i x chunks_i from the plan's own (r, s, chunk_blocks)."""
    total, chunks = 0, []
    for lo, hi, q in shapes:
        nx, A = int(hi - lo) + 1, int(q) + 1
        c = _ceil(_ceil(A, pl.r), pl.chunk_blocks)
        chunks.append(c)
        total += _ceil(nx, 64 * pl.s) * c
    return total, chunks


def test_plan_period_without_a_device(sia):
    b, pmfs = _ragged(sia)
    with b:
        assert [b.num_states_of(i) for i in range(5)] == [51, 1, 64, 130, 700]
        assert [b.num_actions_of(i) for i in range(5)] == [13, 1, 2, 300, 31]
        with pytest.raises(IndexError):
            b.num_states_of(5)
        st = b.stats()
        assert st.instances == 5 and st.period_launches == 0 and st.cells_evaluated == 0
        worst = 0
        for period in (1, 2, 3):
            pl = b.plan(period)
            assert pl.r == 4 and pl.s in (1, 2, 4, 8) and pl.chunk_blocks >= 1
            total, chunks = _expected_tasks(SHAPES, pl)
            assert pl.tasks == total
            assert pl.max_chunks == max(chunks) and pl.min_chunks == min(chunks)
            assert pl.chunked == (1 if max(chunks) > 1 else 0)
            assert 0 < pl.lds_bytes <= 160 * 1024
            worst = max(worst, pl.max_chunks)
        # five small instances leave most SIMDs idle: the 300 actions of instance 3 are cut, the 1 action of instance 1 is not
        assert worst > 1 and st.window_chunks == worst and b.plan(1).min_chunks == 1
        with pytest.raises(sia.SdpgpuError) as e:
            b.plan(4)
        assert e.value.code == 1 and "period 4" in e.value.message
    # a pmf is missing: a state error that says which
    descs = _descs(sia)
    lib = sia._abi.load()
    rc, h, _ = _create(lib, descs, len(SHAPES))
    assert rc == 0
    try:
        pl = sia.SdpgpuBatchPlan()
        assert lib.sdpgpu_batch_plan_period(h, 1, C.byref(pl)) == 2
        assert b"instance 0, period 1" in lib.sdpgpu_batch_last_error(h)
        assert lib.sdpgpu_batch_plan_period(h, 1, None) == 1
    finally:
        lib.sdpgpu_batch_destroy(h)


def test_a_uniform_batch_reports_its_plan_too(sia):
    shapes = [(-20.0, 30.0, 12.0)] * 3
    descs = _descs(sia, shapes, ini_inventory=0.0)
    pmfs = [[_tile(9)] * 3] * 3
    for ragged in (False, True):
        with sia.SdpBatch([descs[i] for i in range(3)], pmfs, ragged=ragged) as b:
            pl = b.plan(2)
            total, chunks = _expected_tasks(shapes, pl)
            assert pl.tasks == total and pl.max_chunks == pl.min_chunks == chunks[0] == b.stats().window_chunks
            assert b.stats().lds_bytes == max(b.plan(p).lds_bytes for p in (1, 2, 3))


def test_forced_blocks_are_honoured_or_refused_with_the_planners_reason(sia, monkeypatch):
    monkeypatch.setenv("SDPGPU_WIN_S", "4")
    monkeypatch.setenv("SDPGPU_WIN_NCH", "3")
    b, _ = _ragged(sia)
    with b:
        for period in (1, 2, 3):
            pl = b.plan(period)
            # 300 actions are 75 blocks of 4: three chunks of 25; instances with at most 25 blocks keep ONE chunk
            assert pl.s == 4 and pl.r == 4 and pl.chunk_blocks == 25 and pl.max_chunks == 3 and pl.min_chunks == 1
            assert pl.chunked == 1 and pl.tasks == _expected_tasks(SHAPES, pl)[0] == 1 + 1 + 1 + 3 + 3
            assert pl.lds_bytes <= 160 * 1024
    monkeypatch.setenv("SDPGPU_WIN_S", "3")  # no such register block
    b, _ = _ragged(sia)
    with b:
        with pytest.raises(sia.SdpgpuError) as e:
            b.plan(1)
        assert e.value.code == 1 and "SDPGPU_WIN_S=3" in e.value.message and "no instantiation" in e.value.message
    # one chunk forced on a window that does not fit the LDS of a compute unit: refused, with the size
    monkeypatch.delenv("SDPGPU_WIN_S")
    monkeypatch.setenv("SDPGPU_WIN_NCH", "1")
    shapes = [(-20.0, 30.0, 12.0), (0.0, 99.0, 2200.0)]
    descs = _descs(sia, shapes, T=1)
    wide = sia.SdpBatch([descs[0], descs[1]], [[_tile(900)], [_tile(1100)]], ragged=True)
    with wide:
        with pytest.raises(sia.SdpgpuError) as e:
            wide.plan(1)
        assert e.value.code == 4 and "LDS" in e.value.message and "2201 actions" in e.value.message
    monkeypatch.delenv("SDPGPU_WIN_NCH")
    wide = sia.SdpBatch([descs[0], descs[1]], [[_tile(900)], [_tile(1100)]], ragged=True)
    with wide:  # left to itself the planner cuts the action axis and fits
        pl = wide.plan(1)
        assert pl.chunked == 1 and pl.max_chunks > pl.min_chunks and pl.lds_bytes <= 160 * 1024
        assert pl.tasks == _expected_tasks(shapes, pl)[0]


@pytest.fixture(scope="module")
def sweep():
    from stochastic_inventory_amd import workloads
    return workloads.fitss_sweep()


def test_fitss_sweep_has_the_reference_shape(sia, sweep):
    from collections import Counter
    assert len(sweep) == 810
    limits = Counter(int(w.functor.maxOrderQuantity) for w in sweep)
    assert sorted(limits) == FITSS_ORDER_LIMITS
    assert sorted(limits.values()) == [27] * 24 + [54] * 3
    for w in sweep:
        d = w.desc()
        assert w.T == 6 and d.periods == 6 and d.family == sia.FAMILY_BACKORDER
        assert (d.min_inventory, d.max_inventory, d.step, d.holding_cost, d.ini_inventory) == (-300, 800, 1, 1, 0)
        for tile in w.pmf:
            assert abs(tile[:, 1].sum() - 1.0) <= 1e-12 and np.all(np.diff(tile[:, 0]) == 1.0) and tile[0, 0] >= 0
    # the reference's loop order: K outermost, then v, pai, demand pattern, capacity innermost (ThreeLevelFitsSTest.java:67-71)
    assert [w.capacity for w in sweep[:3]] == [2, 3, 4] and [w.pattern for w in sweep[:31:3]] == list(range(1, 11)) + [1]
    assert [int(w.functor.maxOrderQuantity) for w in sweep[:6]] == [60, 90, 120, 26, 39, 52]
    assert sweep[0].functor.fixedOrderingCost == 500 and sweep[270].functor.fixedOrderingCost == 800
    assert sweep[0].functor.penaltyCost == 15 and sweep[30].functor.penaltyCost == 10 and sweep[90].functor.variOrderingCost == 5
    assert len({(w.pattern, w.capacity, w.functor.fixedOrderingCost, w.functor.variOrderingCost, w.functor.penaltyCost)
                for w in sweep}) == 810
    from stochastic_inventory_amd import workloads
    sub = workloads.fitss_sweep(patterns=(2, 8))
    assert len(sub) == 162 and {w.pattern for w in sub} == {2, 8} and {w.capacity for w in sub} == {2, 3, 4}
    with pytest.raises(ValueError):
        workloads.fitss_sweep(levels=4)


def test_the_fitss_sweep_plans_one_launch_per_period_and_no_chunks(sia, sweep):
    """810 instances x 18 tiles of 64 states are 14,580 tasks, above the planner's threshold of 4096: every period is ONE
    launch of one task per (instance, tile), no key rows, no finalize pass -- where the 27 batches grouped by order limit
    (486 tiles each) are all chunked."""
    descs = [w.desc() for w in sweep]
    pmfs = [w.pmf for w in sweep]
    with pytest.raises(sia.SdpgpuError) as e:
        sia.SdpBatch(descs, pmfs)
    assert "max_order_quantity" in e.value.message and "instance 1" in e.value.message
    with sia.SdpBatch(descs, pmfs, ragged=True) as b:
        for period in range(1, 7):
            pl = b.plan(period)
            assert pl.chunked == 0 and pl.max_chunks == 1 and pl.min_chunks == 1
            assert pl.tasks == 810 * _ceil(1101, 64 * pl.s)
            assert pl.chunk_blocks == _ceil(289, pl.r) and 0 < pl.lds_bytes <= 160 * 1024
        st = b.stats()
        assert st.instances == 810 and st.window_chunks == 1 and st.period_launches == 0
        assert {b.num_actions_of(i) for i in range(810)} == {q + 1 for q in FITSS_ORDER_LIMITS}
        assert all(b.num_states_of(i) == 1101 for i in range(0, 810, 37))
    group = [i for i, w in enumerate(sweep) if w.functor.maxOrderQuantity == 26]
    assert len(group) == 27
    with sia.SdpBatch([descs[i] for i in group], [pmfs[i] for i in group]) as g:  # today's only route: chunked
        assert g.stats().window_chunks > 1


def test_recursion_batch_takes_the_ragged_keyword(sia):
    tile = np.array([[0.0, 0.5], [1.0, 0.5]])
    fs = [sia.BackorderFunctor(minInventory=-5, maxInventory=5 + i, maxOrderQuantity=3 + i) for i in range(2)]
    with pytest.raises(sia.SdpgpuError):
        sia.RecursionBatch(fs, [[tile, tile]] * 2)
    with sia.RecursionBatch(fs, [[tile, tile]] * 2, ragged=True) as rb:
        assert len(rb) == 2 and rb.batch.ragged and rb.batch.num_states_of(1) == 12 and rb.batch.num_actions_of(1) == 5
