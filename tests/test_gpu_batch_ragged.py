"""The ragged batch on the GPU (sdpgpu_batch_create_ragged; window_f1_batch_kernel with per-instance records and the task
table; batch_sim_kernel on every instance's own grid): N backorder-family instances with inventory bounds and an order limit
of their own, one kernel launch per period for all of them.  The bar is the project's own: np.array_equal on values AND
policy, every state, every period, every instance -- against the CPU oracle (oracle.sdpref.Problem, per instance) and against
the single-handle path (SdpEngine) on the same instance; path sums of the batched simulation bit for bit those of
sdpgpu_simulate on the instance's own handle."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D_CHOICES = (1, 2, 7, 33, 64, 65, 130)  # (the demand counts of tests/test_gpu_batch.py)
# states: 1, 63, 64, 65, about 300, more than 512;  actions: 1 (order limit 0), not a multiple of 4, more than 256
NX_CHOICES = (1, 63, 64, 65, 300, 301, 777)
A_CHOICES = (1, 2, 7, 61, 64, 258, 300)


def _ragged_instances(sia, n=56, T=4, seed=20240611):
    """Seeded: every instance its own grid -- nx from NX_CHOICES, A from A_CHOICES, the lower bound below, at or above zero --,
    costs that vary (v = 0, K = 0 and h = pi included: rich in ties), D_t from D_CHOICES mixed within an instance, first
    demands below, at and above zero."""
    rng = np.random.default_rng(seed)
    functors, pmfs = [], []
    for i in range(n):
        nx = NX_CHOICES[i % len(NX_CHOICES)]
        A = A_CHOICES[(i // len(NX_CHOICES) + 3 * i) % len(A_CHOICES)]
        lo = float([-(nx // 2) - 3, 0, 11, -nx - 5][i % 4])  # below zero (straddling), at zero, above zero, wholly negative
        K = float(rng.choice([0.0, 5.0, 40.0, 200.0]))
        v = float(rng.choice([0.0, 1.0, 2.5]))
        h = float(rng.choice([1.0, 2.0, 3.0]))
        pi = h if i % 5 == 0 else float(rng.choice([2.0, 5.0, 10.0, 20.0]))
        if i == 1:
            K, v = 0.0, 0.0
        f = sia.BackorderFunctor(fixedOrderingCost=K, variOrderingCost=v, holdingCost=h, penaltyCost=pi, minInventory=lo,
                                 maxInventory=lo + nx - 1, maxOrderQuantity=A - 1, iniInventory=lo + float(rng.integers(0, nx)))
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


def _nx(f):
    return int(f.maxInventory - f.minInventory) + 1


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


def _tables(batch, n, T):
    return [[(batch.values(i, p), batch.policy(i, p)) for p in range(1, T + 1)] for i in range(n)]


def test_the_mix_covers_what_it_claims(sia):
    functors, pmfs = _ragged_instances(sia)
    assert len(functors) >= 48
    assert {_nx(f) for f in functors} == set(NX_CHOICES)
    assert {int(f.maxOrderQuantity) + 1 for f in functors} == set(A_CHOICES)
    los = {f.minInventory for f in functors}
    assert min(los) < 0 and 0.0 in los and max(los) > 0
    assert {len(tile) for pmf in pmfs for tile in pmf} == set(D_CHOICES)
    firsts = {tile[0, 0] for pmf in pmfs for tile in pmf}
    assert min(firsts) < 0 and 0.0 in firsts and max(firsts) > 0
    # the small and the large ends meet in both orders: one state with many actions, many states with one action
    shapes = {(_nx(f), int(f.maxOrderQuantity) + 1) for f in functors}
    assert (1, 300) in shapes and (777, 1) in shapes and (1, 1) in shapes
    assert any(nx > 512 and A % 4 for nx, A in shapes)


@pytest.mark.parametrize("direction", ["MIN", "MAX"])
def test_mixed_ragged_batch_equals_the_oracle_and_the_single_handle(sia, oracle, direction):
    T = 4
    dirn = getattr(sia.OptDirection, direction)
    functors, pmfs = _ragged_instances(sia, T=T)
    n = len(functors)
    descs = [f.to_desc(T, dirn) for f in functors]
    ref = _oracle_tables(oracle, descs, pmfs)
    with sia.SdpBatch(descs, pmfs, ragged=True, device=0) as b:
        b.solve()
        st = b.stats()
        assert st.instances == n and st.period_launches == T and st.periods_run == T
        assert st.finalize_launches == (2 if st.window_chunks > 1 else 0)
        assert st.cells_evaluated == sum(_nx(f) * (int(f.maxOrderQuantity) + 1) * len(tile)
                                         for f, pmf in zip(functors, pmfs) for tile in pmf)
        ini_v, ini_k = b.initial()
        for i, f in enumerate(functors):
            assert b.num_states_of(i) == _nx(f) and b.num_actions_of(i) == int(f.maxOrderQuantity) + 1
            _assert_tables(b, i, ref[i][0], ref[i][1], T, f"oracle ({direction})")
            ix = int(f.iniInventory - f.minInventory)
            assert ini_v[i] == ref[i][0][0][ix] and ini_k[i] == ref[i][1][0][ix]
            d = f.to_desc(T, dirn)
            d.device = 0
            with sia.SdpEngine(d, pmfs[i]) as eng:
                eng.solve()
                for period in range(1, T + 1):
                    assert np.array_equal(b.values(i, period), eng.values(period)), (i, period)
                    assert np.array_equal(b.policy(i, period), eng.policy(period)), (i, period)
        first = _tables(b, n, T)
        b.solve()  # a second sweep of the same batch
        again = _tables(b, n, T)
    with sia.SdpBatch(descs[::-1], pmfs[::-1], ragged=True, device=0) as r:  # the same list reversed
        r.solve()
        rev = _tables(r, n, T)
    for i in range(n):
        for p in range(T):
            for got in (again[i][p], rev[n - 1 - i][p]):
                assert np.array_equal(got[0], first[i][p][0]) and np.array_equal(got[1], first[i][p][1]), (i, p + 1)


def _unequal(sia, which, T=4):
    """Two or three unequal instances: 300 actions on 301 states, 7 actions on 777 states (ONE chunk where the first has
    several), 61 actions on 63 states."""
    functors, pmfs = _ragged_instances(sia, T=T, seed=77)
    want = [(301, 300), (777, 7), (63, 61)][:which]
    pick = []
    for nx, A in want:
        pick.append(next(i for i, f in enumerate(functors) if (_nx(f), int(f.maxOrderQuantity) + 1) == (nx, A)))
    return [functors[i] for i in pick], [pmfs[i] for i in pick]


@pytest.mark.parametrize("which", [2, 3])
def test_forced_chunking_on_unequal_instances_equals_the_oracle(sia, oracle, monkeypatch, which):
    """The keys + finalize route with chunk counts that differ between the instances of one launch."""
    T = 4
    functors, pmfs = _unequal(sia, which, T)
    descs = [f.to_desc(T) for f in functors]
    ref = _oracle_tables(oracle, descs, pmfs, workers=which)
    for nch, s in ((3, 0), (5, 2), (2, 8), (4, 4)):
        monkeypatch.setenv("SDPGPU_WIN_NCH", str(nch))
        if s:
            monkeypatch.setenv("SDPGPU_WIN_S", str(s))
        b = sia.SdpBatch(descs, pmfs, ragged=True, device=0)
        monkeypatch.delenv("SDPGPU_WIN_NCH")
        monkeypatch.delenv("SDPGPU_WIN_S", raising=False)
        with b:
            pl = b.plan(1)
            assert pl.chunked == 1 and pl.max_chunks == nch and pl.min_chunks == 1  # 7 actions are two blocks: one chunk
            if s:
                assert pl.s == s
            b.solve()
            st = b.stats()
            assert st.window_chunks == nch and st.finalize_launches == 2 and st.period_launches == T
            for i in range(which):
                _assert_tables(b, i, ref[i][0], ref[i][1], T, f"chunks={nch} s={s}")
            ini_v, ini_k = b.initial()
            for i, f in enumerate(functors):
                ix = int(f.iniInventory - f.minInventory)
                assert ini_v[i] == ref[i][0][0][ix] and ini_k[i] == ref[i][1][0][ix]


def test_ping_pong_tables_keep_periods_one_and_two_and_every_policy_row(sia):
    T = 4
    functors, pmfs = _ragged_instances(sia, n=14, T=T, seed=11)
    full = [f.to_desc(T) for f in functors]
    lean = [f.to_desc(T) for f in functors]
    for d in lean:
        d.store_all_values = 0
    with sia.SdpBatch(full, pmfs, ragged=True, device=0) as a, sia.SdpBatch(lean, pmfs, ragged=True, device=0) as b:
        a.solve()
        b.solve()
        va, ka = a.initial()
        vb, kb = b.initial()
        assert np.array_equal(va, vb) and np.array_equal(ka, kb)
        assert b.stats().window_chunks == 1
        for i in range(14):
            for period in (1, 2):
                assert np.array_equal(a.values(i, period), b.values(i, period)), (i, period)
            for period in range(1, T + 1):
                assert np.array_equal(a.policy(i, period), b.policy(i, period)), (i, period)
        with pytest.raises(sia.SdpgpuError) as e:
            b.values(0, 3)
        assert e.value.code == 2


def _uniform_instances(sia, n=12, T=4, seed=5):
    functors, pmfs = _ragged_instances(sia, n=n, T=T, seed=seed)
    same = [sia.BackorderFunctor(fixedOrderingCost=f.fixedOrderingCost, variOrderingCost=f.variOrderingCost,
                                 holdingCost=f.holdingCost, penaltyCost=f.penaltyCost, minInventory=-40, maxInventory=99,
                                 maxOrderQuantity=45, iniInventory=float(-40 + 7 * i)) for i, f in enumerate(functors)]
    return same, pmfs


def test_equal_shapes_through_the_ragged_entry_point_are_the_uniform_batch(sia):
    T = 4
    functors, pmfs = _uniform_instances(sia, T=T)
    descs = [f.to_desc(T) for f in functors]
    n = len(descs)
    with sia.SdpBatch(descs, pmfs, device=0) as u, sia.SdpBatch(descs, pmfs, ragged=True, device=0) as r:
        u.solve()
        r.solve()
        su, sr = u.stats(), r.stats()
        assert (su.window_r, su.window_s, su.window_chunks, su.lds_bytes, su.cells_evaluated, su.finalize_launches) == \
               (sr.window_r, sr.window_s, sr.window_chunks, sr.lds_bytes, sr.cells_evaluated, sr.finalize_launches)
        for i in range(n):
            for period in range(1, T + 1):
                assert np.array_equal(u.values(i, period), r.values(i, period)), (i, period)
                assert np.array_equal(u.policy(i, period), r.policy(i, period)), (i, period)
        (vu, ku), (vr, kr) = u.initial(), r.initial()
        assert np.array_equal(vu, vr) and np.array_equal(ku, kr)
        for i in (0, 5, n - 1):
            du, uu = u.sample_demands(i, 1000, 42)
            dr, ur = r.sample_demands(i, 1000, 42)
            assert np.array_equal(du, dr) and np.array_equal(uu, ur)
        mu, xu = u.simulate_sampled(10000, 42, want_sums=True)
        mr, xr = r.simulate_sampled(10000, 42, want_sums=True)
        assert np.array_equal(mu, mr) and np.array_equal(xu, xr)


def _check_means(means, sums, what):
    """out_mean against math.fsum(sums) / n_paths within the 1e-13 relative of tests/test_gpu_batch_simulate.py (six tree
    levels in a wave plus the wave partials in order: at most 163 x 2^-53 = 1.8e-14 for 10000 paths of non-negative costs)."""
    for i in range(len(means)):
        want = math.fsum(sums[i].tolist()) / sums.shape[1]
        print(f"{what}: instance {i}: mean {means[i]!r} fsum {want!r}") if i < 2 else None
        assert abs(means[i] - want) <= 1e-13 * abs(want), (what, i, means[i], want)


def test_ragged_simulation_equals_the_handle_on_every_instances_own_grid(sia):
    T = 4
    functors, pmfs = _ragged_instances(sia, T=T)
    N = len(functors)
    rng = np.random.default_rng(99)
    cases = []
    for n_paths in (1, 64, 65, 1000):
        shared = rng.integers(-15, 150, size=(n_paths, T)).astype(np.float64)
        per = rng.integers(-15, 150, size=(N, n_paths, T)).astype(np.float64)
        far = rng.random(per.shape)
        per[far < 0.02] = 1000.0   # far beyond every support and every grid
        per[far > 0.98] = -1000.0  # a negative demand larger than every grid
        ini = np.array([f.minInventory + float(rng.integers(0, _nx(f))) for f in functors])
        cases.append((n_paths, shared, per, ini))
    descs = [f.to_desc(T) for f in functors]
    got = []
    with sia.SdpBatch(descs, pmfs, ragged=True, device=0) as b:
        b.solve()
        for n_paths, shared, per, ini in cases:
            m1, s1 = b.simulate(shared, want_sums=True)
            m2, s2 = b.simulate(per, ini_x=ini, want_sums=True)
            assert s1.shape == (N, n_paths) and np.array_equal(m2, b.simulate(per, ini_x=ini))
            _check_means(m1, s1, f"shared n={n_paths}")
            _check_means(m2, s2, f"per-instance n={n_paths}")
            got.append((s1, s2))
        # an initial state is checked against the instance's OWN grid: 11 + 776 lies on instance 2's, not on instance 0's
        bad = np.array([f.minInventory for f in functors])
        bad[0] = functors[0].maxInventory + 1
        with pytest.raises(sia.SdpgpuError) as e:
            b.simulate(cases[0][1], ini_x=bad)
        assert e.value.code == 1 and "instance 0" in e.value.message and "ini_x" in e.value.message
        # the fused sample-and-roll launch equals the rollout fed the demands the sampler reports
        for n_paths in (65, 10000):
            ms, ss = b.simulate_sampled(n_paths, 4242, want_sums=True)
            dem = np.stack([b.sample_demands(i, n_paths, 4242)[0] for i in range(N)])
            me, se = b.simulate(dem, want_sums=True)
            assert np.array_equal(ss, se) and np.array_equal(ms, me)
            _check_means(ms, ss, f"sampled n={n_paths}")
    for i, f in enumerate(functors):
        d = f.to_desc(T)
        d.device = 0
        with sia.SdpEngine(d, pmfs[i]) as eng:
            eng.solve()
            for c, (n_paths, shared, per, ini) in enumerate(cases):
                h1, ok1 = eng.simulate(shared, np.ones(T), f.iniInventory, 0.0, 0.0)
                h2, ok2 = eng.simulate(per[i], np.ones(T), float(ini[i]), 0.0, 0.0)
                assert ok1.all() and ok2.all()
                assert np.array_equal(got[c][0][i], h1) and np.array_equal(got[c][1][i], h2), f"instance {i}, n_paths {n_paths}"


def test_recursion_and_simulation_batch_over_a_ragged_batch(sia):
    T = 4
    functors, pmfs = _ragged_instances(sia, n=8, T=T, seed=5)
    with sia.RecursionBatch(functors, pmfs, device=0, ragged=True) as rb:
        for i, f in enumerate(functors):
            rec = sia.Recursion(sia.OptDirection.MIN, pmfs[i], functor=f, device=0)
            for s in (sia.State(1, f.iniInventory), sia.State(2, f.minInventory), sia.State(T, f.maxInventory)):
                assert rb.getExpectedValue(i, s) == rec.getExpectedValue(s)
                assert rb.getAction(i, s) == rec.getAction(s)
            with pytest.raises(ValueError):
                rb.getExpectedValue(i, sia.State(1, f.maxInventory + 1))
        sim = sia.SimulationBatch(None, 1000, rb, seed=7)
        means = sim.simulateSDPGivenSamplNum(want_sums=True)
        assert means.shape == (8,) and sim.last_values.shape == (8, 1000)
        assert np.array_equal(means, rb.batch.simulate_sampled(1000, 7))


def test_fitss_two_patterns_against_the_oracle(sia, oracle):
    """Demand patterns 2 and 7 of ThreeLevelFitsSTest.main x its 27 cost combinations x all three capacities: 162 instances of
    1101 states with the order limits 26, 39, 52 and 144, 216, 288, T = 6, full tables."""
    from stochastic_inventory_amd import workloads
    ws = workloads.fitss_sweep(patterns=(2, 7))
    assert len(ws) == 162 and {int(w.functor.maxOrderQuantity) for w in ws} == {26, 39, 52, 144, 216, 288}
    descs = [w.desc() for w in ws]
    pmfs = [w.pmf for w in ws]
    ref = _oracle_tables(oracle, descs, pmfs)
    with sia.SdpBatch(descs, pmfs, ragged=True, device=0) as b:
        b.solve()
        st = b.stats()
        print(f"\nragged batch of 162: {st.solve_ms:.2f} ms, chunks {st.window_chunks}, R x S = {st.window_r} x {st.window_s}")
        assert st.period_launches == 6
        for i in range(len(ws)):
            _assert_tables(b, i, ref[i][0], ref[i][1], 6, ws[i].name)


def test_fitss_all_810_against_the_batches_grouped_by_shape(sia):
    """The whole sweep as ONE ragged batch -- six launches, no finalize pass -- against today's route: 27 batches of one
    shape each, grouped by order limit."""
    from stochastic_inventory_amd import workloads
    ws = workloads.fitss_sweep()
    descs = [w.desc() for w in ws]
    pmfs = [w.pmf for w in ws]
    with sia.SdpBatch(descs, pmfs, ragged=True, device=0) as b:
        b.solve()
        st = b.stats()
        assert st.instances == 810 and st.period_launches == 6 and st.finalize_launches == 0 and st.window_chunks == 1
        ini_v, ini_k = b.initial()
        groups = {}
        for i, w in enumerate(ws):
            groups.setdefault(int(w.functor.maxOrderQuantity), []).append(i)
        assert len(groups) == 27
        cells = 0
        for q, idx in sorted(groups.items()):
            with sia.SdpBatch([descs[i] for i in idx], [pmfs[i] for i in idx], device=0) as g:
                g.solve()
                gv, gk = g.initial()
                cells += g.stats().cells_evaluated
                for j, i in enumerate(idx):
                    assert ini_v[i] == gv[j] and ini_k[i] == gk[j], ws[i].name
                j, i = len(idx) - 1, idx[-1]  # one instance per shape: the whole first period
                assert np.array_equal(b.values(i, 1), g.values(j, 1)) and np.array_equal(b.policy(i, 1), g.policy(j, 1)), ws[i].name
        assert st.cells_evaluated == cells
