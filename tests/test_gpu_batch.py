"""The batched solve on the GPU (sdpgpu_batch_*, window_f1_batch_kernel): N backorder-family instances of one grid shape,
one kernel launch per period for all of them.  The bar is the project's own: np.array_equal on values AND policy, every
state, every period, every instance -- against the CPU oracle (oracle.sdpref.Problem, per instance) and against the
single-handle path (SdpEngine) on the same instance."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D_CHOICES = (1, 2, 7, 33, 64, 65, 130)


def _mixed_instances(sia, n=48, T=5, seed=20240607):
    """Seeded: costs vary (v = 0, K = 0 and h = pi included: rich in ties), D_t from D_CHOICES mixed within an instance,
    first demands below, at and above zero."""
    rng = np.random.default_rng(seed)
    functors, pmfs = [], []
    for i in range(n):
        K = float(rng.choice([0.0, 5.0, 40.0, 200.0]))
        v = float(rng.choice([0.0, 1.0, 2.5]))
        h = float(rng.choice([1.0, 2.0, 3.0]))
        pi = h if i % 5 == 0 else float(rng.choice([2.0, 5.0, 10.0, 20.0]))
        if i == 1:
            K, v = 0.0, 0.0
        f = sia.BackorderFunctor(fixedOrderingCost=K, variOrderingCost=v, holdingCost=h, penaltyCost=pi, minInventory=-120,
                                 maxInventory=179, maxOrderQuantity=60, iniInventory=float(rng.integers(-120, 180)))
        tiles = []
        for t in range(T):
            D = int(D_CHOICES[(i + 3 * t + int(rng.integers(0, 7))) % len(D_CHOICES)])
            d0 = float([-9, 0, 4][(i + t) % 3])
            p = rng.random(D) + 0.05
            if D > 3 and i % 4 == 0:
                p[1] = 0.0  # a zero-probability step inside the support
            p = p / p.sum()
            tiles.append(np.stack([d0 + np.arange(D, dtype=np.float64), p], axis=1))
        functors.append(f)
        pmfs.append(tiles)
    return functors, pmfs


def _oracle_tables(oracle, descs, pmfs, workers=16):
    def one(k):
        V, pol, _ = oracle.Problem(descs[k], pmfs[k]).solve()
        return V, pol
    with ThreadPoolExecutor(max_workers=workers) as ex:  # (the C solver releases the GIL)
        return list(ex.map(one, range(len(descs))))


def _assert_tables(batch, i, V, pol, T, what):
    for period in range(1, T + 1):
        assert np.array_equal(batch.values(i, period), V[period - 1]), f"{what}: values of instance {i}, period {period}"
        assert np.array_equal(batch.policy(i, period), pol[period - 1]), f"{what}: policy of instance {i}, period {period}"


def test_mixed_batch_equals_the_oracle_and_the_single_handle(sia, oracle):
    T = 5
    functors, pmfs = _mixed_instances(sia, 48, T)
    descs = [f.to_desc(T) for f in functors]
    firsts = {tile[0, 0] for pmf in pmfs for tile in pmf}
    assert min(firsts) < 0 and 0.0 in firsts and max(firsts) > 0
    assert {len(tile) for pmf in pmfs for tile in pmf} == set(D_CHOICES)
    ref = _oracle_tables(oracle, descs, pmfs)
    with sia.SdpBatch(descs, pmfs, device=0) as b:
        b.solve()
        st = b.stats()
        assert st.period_launches == T and st.periods_run == T
        assert st.cells_evaluated == sum(300 * 61 * len(tile) for pmf in pmfs for tile in pmf)
        ini_v, ini_k = b.initial()
        for i in range(48):
            _assert_tables(b, i, ref[i][0], ref[i][1], T, "oracle")
            ix = int(functors[i].iniInventory + 120)
            assert ini_v[i] == ref[i][0][0][ix] and ini_k[i] == ref[i][1][0][ix]
            d = functors[i].to_desc(T)
            d.device = 0
            with sia.SdpEngine(d, pmfs[i]) as eng:
                eng.solve()
                for period in range(1, T + 1):
                    assert np.array_equal(b.values(i, period), eng.values(period))
                    assert np.array_equal(b.policy(i, period), eng.policy(period))


def test_a_batch_of_one_equals_the_single_handle(sia):
    from stochastic_inventory_amd import workloads
    w = workloads.cfg2_clsp(T=4, S=3000, A=120, D=47)
    d = w.desc()
    d.device = 0
    with sia.SdpBatch([d], [w.pmf]) as b, sia.SdpEngine(d, w.pmf) as eng:
        b.solve()
        eng.solve()
        assert b.stats().window_chunks > 1  # one instance: the action axis is cut, keys + finalize
        assert b.stats().finalize_launches == 2
        for period in range(1, 5):
            assert np.array_equal(b.values(0, period), eng.values(period))
            assert np.array_equal(b.policy(0, period), eng.policy(period))


def test_forced_chunking_equals_the_oracle(sia, oracle, monkeypatch):
    """The keys + finalize route must not go untested because a large batch never takes it: the override the window
    planner honours at create time forces it on a batch of two."""
    T = 5
    functors, pmfs = _mixed_instances(sia, 2, T, seed=7)
    descs = [f.to_desc(T) for f in functors]
    ref = _oracle_tables(oracle, descs, pmfs, workers=2)
    for nch, s in ((3, 0), (4, 2), (2, 8)):
        monkeypatch.setenv("SDPGPU_WIN_NCH", str(nch))
        if s:
            monkeypatch.setenv("SDPGPU_WIN_S", str(s))
        b = sia.SdpBatch(descs, pmfs, device=0)
        monkeypatch.delenv("SDPGPU_WIN_NCH")
        monkeypatch.delenv("SDPGPU_WIN_S", raising=False)
        with b:
            b.solve()
            st = b.stats()
            assert st.window_chunks == nch and st.finalize_launches == 2 and st.period_launches == T
            if s:
                assert st.window_s == s
            for i in range(2):
                _assert_tables(b, i, ref[i][0], ref[i][1], T, f"chunks={nch}")


def test_ping_pong_tables_keep_period_one(sia):
    T = 5
    functors, pmfs = _mixed_instances(sia, 12, T, seed=11)
    full = [f.to_desc(T) for f in functors]
    lean = [f.to_desc(T) for f in functors]
    for d in lean:
        d.store_all_values = 0
    with sia.SdpBatch(full, pmfs, device=0) as a, sia.SdpBatch(lean, pmfs, device=0) as b:
        a.solve()
        b.solve()
        va, ka = a.initial()
        vb, kb = b.initial()
        assert np.array_equal(va, vb) and np.array_equal(ka, kb)
        for i in range(12):
            assert np.array_equal(a.values(i, 1), b.values(i, 1)) and np.array_equal(a.policy(i, 1), b.policy(i, 1))
            assert np.array_equal(a.policy(i, T), b.policy(i, T))  # the policy of every period is kept
        with pytest.raises(sia.SdpgpuError) as e:
            b.values(0, 4)
        assert e.value.code == 2


def test_clsp_testing_reduced_against_the_oracle(sia, oracle):
    """Demand patterns 1 and 7 x the 54 cost / coeVar combinations of CLSPTesting.main: 108 instances of 1001 x 501,
    T = 8, full tables."""
    from stochastic_inventory_amd import workloads
    ws = workloads.clsp_testing_sweep(patterns=(1, 7))
    descs = [w.desc() for w in ws]
    pmfs = [w.pmf for w in ws]
    t0 = time.perf_counter()
    ref = _oracle_tables(oracle, descs, pmfs)
    t_oracle = time.perf_counter() - t0
    with sia.SdpBatch(descs, pmfs, device=0) as b:
        b.solve()
        st = b.stats()
        print(f"\noracle {t_oracle:.1f} s on 16 threads; batch of 108: {st.solve_ms:.2f} ms, chunks {st.window_chunks}, "
              f"R x S = {st.window_r} x {st.window_s}")
        assert st.period_launches == 8
        for i in range(len(ws)):
            _assert_tables(b, i, ref[i][0], ref[i][1], 8, ws[i].name)


def test_clsp_testing_all_540_against_the_looped_single_handle(sia):
    """The whole sweep at the size that is timed (tools/batch_sweep_perf.py): ONE period-kernel launch per period for all
    540 instances, no finalize pass, and the bits of 540 separate handles."""
    from stochastic_inventory_amd import workloads
    ws = workloads.clsp_testing_sweep()
    descs = [w.desc() for w in ws]
    with sia.SdpBatch(descs, [w.pmf for w in ws], device=0) as b:
        b.solve()
        st = b.stats()
        assert st.instances == 540 and st.period_launches == 8 and st.finalize_launches == 0 and st.window_chunks == 1
        ini_v, ini_k = b.initial()
        cells = 0
        for i, w in enumerate(ws):
            d = w.desc()
            d.device = 0
            with sia.SdpEngine(d, w.pmf) as eng:
                eng.solve()
                V1, P1 = eng.values(1), eng.policy(1)
                cells += eng.stats().cells_evaluated
            assert np.array_equal(b.values(i, 1), V1) and np.array_equal(b.policy(i, 1), P1), w.name
            assert ini_v[i] == V1[500] and ini_k[i] == P1[500], w.name  # ini_inventory 0 is state 500 of [-500, 500]
        assert st.cells_evaluated == cells


def test_task_order_does_not_leak_into_results(sia):
    T = 5
    functors, pmfs = _mixed_instances(sia, 20, T, seed=3)
    descs = [f.to_desc(T) for f in functors]
    with sia.SdpBatch(descs, pmfs, device=0) as a, sia.SdpBatch(descs[::-1], pmfs[::-1], device=0) as r:
        a.solve()
        first = [[(a.values(i, p), a.policy(i, p)) for p in range(1, T + 1)] for i in range(20)]
        a.solve()  # a second sweep of the same batch
        r.solve()
        for i in range(20):
            for p in range(1, T + 1):
                v, k = first[i][p - 1]
                assert np.array_equal(a.values(i, p), v) and np.array_equal(a.policy(i, p), k)
                assert np.array_equal(r.values(19 - i, p), v) and np.array_equal(r.policy(19 - i, p), k)


def test_recursion_batch_answers_like_recursion(sia):
    T = 5
    functors, pmfs = _mixed_instances(sia, 6, T, seed=5)
    with sia.RecursionBatch(functors, pmfs, device=0) as rb:
        for i, f in enumerate(functors):
            rec = sia.Recursion(sia.OptDirection.MIN, pmfs[i], functor=f, device=0)
            for s in (sia.State(1, f.iniInventory), sia.State(3, -7.0), sia.State(T, 179.0)):
                assert rb.getExpectedValue(i, s) == rec.getExpectedValue(s)
                assert rb.getAction(i, s) == rec.getAction(s)
