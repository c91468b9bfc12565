"""What the two kinds of batch share around a solve (csrc/sdpgpu_batch_frame.hpp): the stream a batch runs on (its own or the
caller's), the timing events of a sweep, the row read-outs with their refusals, initial()'s staging block and the release.  Every
check runs on a backorder batch (3 instances, 3 periods, 40 states, 8 actions, 5 demand points) and on a workforce batch (3
unclamped instances, 3 periods, hires 0 .. 12), the smallest of tests/test_gpu_batch.py and tests/test_staff_batch_host.py;
tables are compared with np.array_equal, refusals by status code and text."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, T = 3, 3
ERR_ARG, ERR_STATE = 1, 2


class F1:
    """3 backorder instances on the grid -10 .. 29 with order quantities 0 .. 7."""
    name = "f1"
    solved_before_output = False  # the order of the two refusals of a read, as each family has always reported them

    @staticmethod
    def make(sia, store_all=1):
        rng = np.random.default_rng(5)
        descs, pmfs = [], []
        for i in range(N):
            f = sia.BackorderFunctor(fixedOrderingCost=5.0 * i, variOrderingCost=1.0, holdingCost=1.0 + i, penaltyCost=9.0, minInventory=-10,
                                     maxInventory=29, maxOrderQuantity=7, iniInventory=float(3 * i - 2))
            d = f.to_desc(T)
            d.store_all_values = store_all
            descs.append(d)
            tiles = []
            for t in range(T):
                p = rng.random(5) + 0.05
                tiles.append(np.stack([float(t) + np.arange(5, dtype=np.float64), p / p.sum()], axis=1))
            pmfs.append(tiles)
        return sia.SdpBatch(descs, pmfs, device=0)

    @staticmethod
    def rows(b, i, period):
        return 40

    @staticmethod
    def ini_index(b, i):
        return 3 * i - 2 + 10

    @staticmethod
    def states_text(period, nx):
        return f"the grid has {nx} states"


class Staff:
    """3 workforce instances from iniStaffNum 0 over two level tables; the staff range grows with the period."""
    name = "staff"
    solved_before_output = True

    @staticmethod
    def make(sia, store_all=1):
        descs = []
        for i in range(N):
            f = sia.StaffFunctor(fixCost=50.0 + i, unitVariCost=20.0, salary=5.0 * (i + 1), unitPenalty=250.0, minStaffNum=[4] * T,
                                 maxHireNum=12, clampStaff=False, iniStaffNum=0)
            d = f.to_desc(T)
            d.kernel, d.store_all_values = sia._abi.KERNEL_SEPARABLE, store_all
            descs.append(d)
        tables = [(sia.staff_level_pmf([rate], 13)[0], None) for rate in (0.3, 0.15)]
        return sia.StaffBatch(descs, tables, [[i % 2] * T for i in range(N)], [[4] * T] * N, device=0)

    @staticmethod
    def rows(b, i, period):
        return b.grid(i, period)[1]

    @staticmethod
    def ini_index(b, i):
        return 0

    @staticmethod
    def states_text(period, nx):
        return f"period {period} has {nx} states"


@pytest.fixture(scope="module", params=[F1, Staff], ids=lambda f: f.name)
def fam(request):
    return request.param


def _tables(b):
    return [(b.values(i, period), b.policy(i, period)) for i in range(N) for period in range(1, T + 1)]


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def reference(sia, fam):
    """Every table of a fresh batch solved on the stream it made itself."""
    with fam.make(sia) as b:
        b.solve()
        ref = _tables(b)
    assert all(v.size == p.size and v.size > 0 and np.isfinite(v).all() for v, p in ref)
    return ref


def _last_error(b):
    return b._lib.sdpgpu_batch_last_error(b._b).decode()


def _streams(torch):
    """The stream torch is on (the null stream) and a stream of the caller's own."""
    return {"current": torch.cuda.current_stream(), "side": torch.cuda.Stream()}


@pytest.mark.parametrize("which", ["current", "side"])
def test_a_batch_on_the_callers_stream_computes_the_same_tables(sia, fam, reference, which):
    import torch
    stream = _streams(torch)[which]
    with fam.make(sia) as b:
        b.set_stream(stream.cuda_stream)
        b.solve(sync=False)
        b.synchronize()
        assert _same(_tables(b), reference)
    stream.synchronize()


@pytest.mark.parametrize("which", ["current", "side"])
def test_set_stream_after_a_solve_replaces_the_owned_stream(sia, fam, reference, which):
    import torch
    stream = _streams(torch)[which]
    with fam.make(sia) as b:
        b.solve()
        assert _same(_tables(b), reference)
        b.set_stream(stream.cuda_stream)
        b.solve(sync=False)
        b.synchronize()
        assert _same(_tables(b), reference)
    stream.synchronize()


def test_profiling_times_the_sweep_and_every_period(sia, fam):
    with fam.make(sia) as b:
        b.set_profiling(True)
        b.solve()
        solve_ms = b.stats().solve_ms
        period_ms = [b.period_ms(period) for period in range(1, T + 1)]
        print(f"{fam.name}: solve_ms {solve_ms}, period_ms {period_ms}")
        assert solve_ms > 0
        assert all(ms > 0 for ms in period_ms)
        assert _last_error(b) == ""
        for period in (0, T + 1):
            assert b.period_ms(period) == -1.0
            assert f"period {period} has no timing" in _last_error(b)
        assert b.period_ms(1) > 0 and _last_error(b) == ""


def test_a_solve_without_profiling_has_no_period_times(sia, fam):
    with fam.make(sia) as b:
        b.solve()
        assert b.stats().solve_ms > 0
        for period in range(0, T + 2):
            assert b.period_ms(period) == -1.0
            assert "has no timing (sdpgpu_batch_set_profiling before the solve)" in _last_error(b)


def test_initial_is_the_initial_states_entry_of_period_one(sia, fam):
    """N doubles, then N int32 in one staging block: a wrong split shows as a value or an action of another instance."""
    with fam.make(sia) as b:
        b.solve()
        val, act = b.initial()
        assert val.shape == (N,) and act.shape == (N,)
        for i in range(N):
            ix = fam.ini_index(b, i)
            assert val[i] == b.values(i, 1)[ix] and act[i] == b.policy(i, 1)[ix]
        assert len(set(val.tolist())) == N  # (the instances differ: a shifted block cannot pass)


def _read(b, what, i, period, n):
    """The raw call with room for n + 1 entries; (status, text)."""
    if what == "values":
        out = np.zeros(n + 1, dtype=np.float64)
        rc = b._lib.sdpgpu_batch_values(b._b, i, period, out.ctypes.data_as(C.POINTER(C.c_double)), n)
    else:
        out = np.zeros(n + 1, dtype=np.int32)
        rc = b._lib.sdpgpu_batch_policy(b._b, i, period, out.ctypes.data_as(C.POINTER(C.c_int32)), n)
    return rc, _last_error(b)


@pytest.mark.parametrize("what", ["values", "policy"])
def test_read_refusals(sia, fam, what):
    who = f"sdpgpu_batch_{what}"
    with fam.make(sia) as b:
        nx = fam.rows(b, 0, 2)
        # before the solve
        assert _read(b, what, 0, 2, nx) == (ERR_STATE, f"{who} before sdpgpu_batch_solve")
        # two bad things at once: the family's own order decides the status
        rc, text = _read(b, what, 0, 2, nx + 1)
        if fam.solved_before_output:
            assert (rc, text) == (ERR_STATE, f"{who} before sdpgpu_batch_solve")
        else:
            assert (rc, text) == (ERR_ARG, f"{who}: bad output (n = {nx + 1}, {fam.states_text(2, nx)})")
        # the index ranges come first in both
        assert _read(b, what, N, 2, nx) == (ERR_ARG, f"{who}: instance {N} outside 0 .. {N - 1}")
        assert _read(b, what, 0, T + 1, nx) == (ERR_ARG, f"{who}: period {T + 1} outside 1 .. {T}")
        b.solve()
        assert _read(b, what, -1, 2, nx) == (ERR_ARG, f"{who}: instance -1 outside 0 .. {N - 1}")
        assert _read(b, what, 0, 0, nx) == (ERR_ARG, f"{who}: period 0 outside 1 .. {T}")
        assert _read(b, what, 0, 2, nx + 1) == (ERR_ARG, f"{who}: bad output (n = {nx + 1}, {fam.states_text(2, nx)})")
        assert _read(b, what, 0, 2, -1) == (ERR_ARG, f"{who}: bad output (n = -1, {fam.states_text(2, nx)})")
        null = b._lib.sdpgpu_batch_values if what == "values" else b._lib.sdpgpu_batch_policy
        assert null(b._b, 0, 2, None, nx) == ERR_ARG and "bad output" in _last_error(b)
        # a good call leaves no text, and a shorter read is allowed
        assert _read(b, what, 0, 2, nx) == (0, "")
        assert _read(b, what, 0, 2, 1) == (0, "")


def test_ping_pong_tables_refuse_the_overwritten_values(sia, fam):
    with fam.make(sia, store_all=0) as b, fam.make(sia) as full:
        b.solve()
        full.solve()
        with pytest.raises(sia.SdpgpuError) as e:
            b.values(0, 3)
        assert e.value.code == ERR_STATE
        assert ("sdpgpu_batch_values: V_3 was overwritten (store_all_values = 0 keeps two ping-pong tables: periods 1 and 2 survive)"
                in str(e.value))
        for i in range(N):
            for period in (1, 2):
                assert np.array_equal(b.values(i, period), full.values(i, period))
            assert np.array_equal(b.policy(i, 3), full.policy(i, 3))  # (the policy of every period is kept)


def test_destroy_returns_and_leaves_a_foreign_stream_usable(sia, fam):
    import torch
    fam.make(sia).close()  # never solved: nothing on the device
    side = torch.cuda.Stream()
    b = fam.make(sia)
    b.set_stream(side.cuda_stream)
    b.close()  # a foreign stream, never used
    b = fam.make(sia)
    b.solve()
    b.set_stream(side.cuda_stream)  # (releases the stream the batch made)
    b.solve(sync=False)
    b.close()  # drains the foreign stream, does not destroy it
    with torch.cuda.stream(side):
        x = torch.arange(8, device="cuda:0", dtype=torch.float64) * 2.0
    side.synchronize()
    assert x.sum().item() == 56.0
