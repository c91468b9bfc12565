"""Ping-pong value tables (store_all_values = 0) on the GPU: every family, grids that grow with t, horizons of 5 and 6,
ragged slabs, the read-out side and the bookkeeping of which V_t still exists (tests/pingpong.py; the conditions on the
instances: tests/test_pingpong_inputs.py).  Every comparison is np.array_equal against the CPU oracle (or, for the sampled
rollouts, against the same call on a handle that keeps every table): the chain is bit-exact, there is no tolerance anywhere."""
import math

import numpy as np
import pytest

import custom_sources as cs
import pingpong as pp
import test_gpu_fuzz as fz

pytestmark = pytest.mark.gpu

ERR_STATE = 2  # SDPGPU_ERR_STATE (include/sdpgpu.h)


def _refused(sia, call, *args, **kw):
    with pytest.raises(sia.SdpgpuError) as e:
        call(*args, **kw)
    assert e.value.code == ERR_STATE, (e.value.code, e.value.message)


def _check_solved(sia, eng, ref, what, slab=False):
    """What a ping-pong handle holds after a whole sweep: V_1, V_2, every period's policy; V_3 is gone."""
    T = len(ref["V"])
    for t in range(1, min(T, 2) + 1):
        assert np.array_equal(eng.values(t), ref["V"][t - 1]), f"{what}: V_{t}"
    for t in range(1, T + 1):
        lo, hi = eng.slab(t)[1:] if slab else (0, len(ref["pol"][t - 1]))
        assert np.array_equal(eng.policy(t), ref["pol"][t - 1][lo:hi]), f"{what}: policy of period {t}"
    if T >= 3:
        _refused(sia, eng.values, 3)


# ---- 1. whole solves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", pp.FAMILIES)
def test_whole_solves(sia, oracle, family):
    """Every selected instance with the automatic and the generic kernel on the library's own arena."""
    seen = set()
    for w in pp.instances(family):
        ref = pp.reference(oracle, w)
        for kernel in (0, 1):
            with sia.SdpEngine(pp.ping_pong_desc(w, kernel), w.pmf, w.overhead()) as eng:
                eng.solve()
                if kernel == 0:
                    seen.add(eng.stats().kernel_used)
                assert eng.stats().cells_evaluated == ref["cells"], w.name
                _check_solved(sia, eng, ref, f"{w.name} kernel {kernel}")
    assert 2 in seen  # the specialised kernels took part


def test_whole_solves_xr(sia, oracle):
    seen = set()
    for w in pp.instances("xr"):
        ref = pp.reference(oracle, w)
        for kernel in (0, 1):
            with sia.SdpEngine(pp.ping_pong_desc(w, kernel), w.pmf, w.overhead()) as eng:
                eng.solve()
                seen.add(eng.stats().kernel_used)
                assert eng.stats().cells_evaluated == ref["cells"], w.name
                _check_solved(sia, eng, ref, f"{w.name} kernel {kernel}")
    assert seen == {1, 2}


def test_whole_solves_wide_cash_rows(sia, oracle, monkeypatch):
    monkeypatch.setenv("SDPGPU_CASH_DIAG_CHECK", "1")  # (the guard word behind the diagonal kernel's spread bound)
    for w in pp.instances("wide_cash"):
        ref = pp.reference(oracle, w)
        with sia.SdpEngine(pp.ping_pong_desc(w), w.pmf, w.overhead()) as eng:
            eng.solve()
            assert eng.stats().cells_evaluated == ref["cells"] and eng.stats().kernel_used == 2, w.name
            _check_solved(sia, eng, ref, w.name)


@pytest.mark.parametrize("group", ["big_cash", "big_f5"])
def test_whole_solves_large_magnitudes(sia, oracle, monkeypatch, group):
    """The three kernels of the store-all tests: the automatic one, the row kernel without its shortcuts (F3 / F4: pairs and
    uniform-key trips off; F5: the one-point kernel), the generic one."""
    off = {"big_cash": ("SDPGPU_CASH_PAIR", "SDPGPU_CASH_UNI"), "big_f5": ("SDPGPU_CASH_OD_PAIR",)}[group]
    seen = set()
    for w in pp.instances(group):
        ref = pp.reference(oracle, w)
        for variant in ("auto", "no-shortcuts", "generic"):
            for k in off:
                monkeypatch.delenv(k, raising=False)
                if variant == "no-shortcuts":
                    monkeypatch.setenv(k, "0")
            with sia.SdpEngine(pp.ping_pong_desc(w, 1 if variant == "generic" else 0), w.pmf, w.overhead()) as eng:
                eng.solve()
                used = eng.stats().kernel_used
                assert used == (1 if variant == "generic" else 2), f"{w.name} {variant}: kernel {used}"
                if variant != "generic":
                    seen.add(used)
                assert eng.stats().cells_evaluated == ref["cells"], w.name
                _check_solved(sia, eng, ref, f"{w.name} {variant}")
    assert seen == {2}


# ---- 2. every period, stale rows poisoned -------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", pp.POISONS, ids=lambda p: str(p))
@pytest.mark.parametrize("group", pp.FAMILIES + pp.OTHER_GROUPS)
def test_every_period_with_stale_rows_poisoned(sia, oracle, group, poison):
    """Automatic kernel: V_t of EVERY period against the oracle's, the destination table and the tail behind V_{t+1} overwritten
    before each period.  All three poisons must give the oracle's tables: a kernel that reads a stale entry under a zero weight
    fails the NaN run alone, one that selects or accumulates it fails both."""
    seen = set()
    for w in pp.instances(group):
        seen |= pp.run_ping_pong(sia, oracle, w, poison=poison)
    assert 2 in seen, seen


@pytest.mark.parametrize("family", pp.FAMILIES)
def test_every_period_generic_kernel_nan_poison(sia, oracle, family):
    for w in pp.instances(family)[:4]:
        assert pp.run_ping_pong(sia, oracle, w, kernel=1, poison="nan") == {1}


# ---- 3. user text -------------------------------------------------------------------------------------------------------------
def _first_T3(family, n):
    out = [w for w in (fz.make_instance(family, s) for s in range(16 if family == 5 else 40)) if w.T >= 3][:n]
    assert len(out) == n
    return out


@pytest.mark.parametrize("fused", [False, True], ids=["three-functions", "fused"])
@pytest.mark.parametrize("family", [3, 4, 5, 6])
def test_cash_families_as_user_text(sia, oracle, family, fused):
    """The cash families as user lambdas (tests/test_custom_functor.py proves on the CPU that the texts restate them), three
    seeds with T >= 3 each, every period against the built-in oracle under the NaN poison."""
    for w in _first_T3(family, 3):
        assert pp.run_ping_pong(sia, oracle, w, poison="nan", custom=cs.cash_text(w, fused=fused)) == {1}  # (the generic loop)


@pytest.mark.parametrize("family,text", [(1, cs.BACKORDER_UNCLAMPED), (2, cs.LEADTIME_UNCLAMPED)], ids=["backorder", "leadtime"])
def test_unclamped_user_text_on_growing_grids(sia, oracle, family, text):
    """Per-period grids grown from the initial state (P.cur != P.next in c_next_index): every V_t is shorter than the stale
    V_{t+2} it is written over."""
    from test_custom_functor import _params_backorder
    growing = [w for w in pp.instances(family) if not w.functor.clampInventory and pp.grid_grows(pp.states_per_period(w))][:2]
    assert len(growing) == 2
    for w in growing:
        assert pp.run_ping_pong(sia, oracle, w, poison="nan", custom=(text, _params_backorder(w.functor))) == {1}


# ---- 4. slabs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", pp.FAMILIES)
def test_ragged_slabs(sia, oracle, family):
    """The instances of test_gpu_fuzz.test_random_instances_sharded_bit_exact (seeds 700.., worlds 2, 3, 5, 7, one issuing thread
    or one per rank) with two tables on every rank."""
    instances = [fz.make_instance(family, 700 + s) for s in range(6)]
    if family != 5:
        instances += [fz.make_stepped_instance(family, 720 + s, 2) for s in range(2)]
    instances += [fz.make_shaped_instance(family, 730, shape) for shape in ("one_inventory_level", "one_demand", "pmf_129_points")]
    for i, w in enumerate(instances):
        world = (2, 3, 5, 7)[i % 4]
        ref = pp.reference(oracle, w)
        engs = []
        try:
            for r in range(world):
                d = pp.ping_pong_desc(w)
                d.rank, d.world_size, d.device = r, world, 0
                engs.append(sia.SdpEngine(d, w.pmf, w.overhead()))
            sia.SdpEngine.solve_multi(engs, sync=True, gather_first=True, threads=bool(i % 2))
            total = 0
            for r, e in enumerate(engs):
                total += int(e.stats().cells_evaluated)
                _check_solved(sia, e, ref, f"{w.name} rank {r}/{world}", slab=True)
            assert total == ref["cells"], w.name
        finally:
            for e in engs:
                e.close()


# ---- 5. read-outs -------------------------------------------------------------------------------------------------------------
def _readout_instances(group):
    ws = [w for w in pp.instances(group) if w.T >= 3]
    out = ws[:2] + ws[-2:]  # (for a family: two seeds of the generator, then the two lengthened instances)
    assert len(out) == 4 and len({w.name for w in out}) == 4
    return out


def _same_result(a, b, what):
    assert (a.n_paths, a.n_valid, a.n_lost) == (b.n_paths, b.n_valid, b.n_lost), what
    for name in ("mean", "m2"):
        assert np.float64(getattr(a, name)).tobytes() == np.float64(getattr(b, name)).tobytes(), (what, name)


@pytest.mark.parametrize("family", pp.FAMILIES)
def test_read_outs_of_a_ping_pong_handle(sia, oracle, family):
    """Reachable sets, the table rollout and the evaluation of period-1 states (on and between grid points: it reads V_2) against
    the oracle's loops, as test_gpu_fuzz.test_random_instances_read_out_bit_exact forms them; the sampled rollout against the same
    call on a handle that keeps every table."""
    for w in _readout_instances(family):
        f = w.functor
        rng = pp.instance_rng(w, "read-out")
        ref = pp.reference(oracle, w)
        P, V, pol = ref["P"], ref["V"], ref["pol"]
        with sia.SdpEngine(pp.ping_pong_desc(w), w.pmf, w.overhead()) as eng, sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as keep:
            eng.solve()
            keep.solve()
            reach = P.reachable()
            for t in range(1, w.T + 1):
                assert np.array_equal(eng.reachable(t), reach[t - 1]), f"{w.name} t={t}: reachable"
            n = 64
            dem = np.stack([rng.choice(np.asarray(w.pmf[t])[:, 0], size=n) for t in range(w.T)], axis=1)
            gamma = getattr(f, "discountFactor", 1.0) if w.desc().family in (3, 4) else 1.0
            disc = np.array([math.pow(gamma, t) for t in range(w.T)])
            ini = (getattr(f, "iniInventory", 0.0), getattr(f, "iniCash", 0.0) or 0.0, getattr(f, "iniPreQ", 0.0) or 0.0)
            gs, gv = eng.simulate(dem, disc, *ini)
            os_, ov = P.simulate(V, pol, dem, disc, *ini)
            assert np.array_equal(gv, ov), f"{w.name}: rollout validity"
            assert np.array_equal(gs[gv.astype(bool)], os_[ov.astype(bool)]), f"{w.name}: rollout sums"
            # period-1 states between grid points (and on them)
            x, cash, preq = P.state_arrays(1)
            pick = rng.choice(len(x), size=min(40, len(x)), replace=False)
            qc = cash[pick] + (rng.integers(0, 3, size=len(pick)) * 0.013 if family in (3, 4, 5, 6) else 0.0)
            kw = dict(cash=qc if family in (3, 4, 5, 6) else None, preq=preq[pick] if family in (2, 5) else None)
            if family == 2 and w.desc().lead_time == 2:
                kw["preq2"] = P.preq2_array(1)[pick]
            ov_, oa_ = P.eval_states(1, V[1], x[pick], **kw)
            gv_, ga_ = eng.eval_states(1, x[pick], **kw)
            assert np.array_equal(ga_, oa_) and np.array_equal(gv_, ov_), f"{w.name}: eval_states(1)"
            # sampled rollouts, from the grid start and (cash families) from a start between cash keys: its action is formed from V_2
            starts = [ini] + ([(ini[0], ini[1] + 0.37, ini[2])] if family in (3, 4, 5, 6) else [])
            for start in starts:
                for mode in ("lhs", "random"):
                    a = eng.simulate_sampled(257, 20241020, *start, mode=mode, discount=disc, want_sums=True)
                    b = keep.simulate_sampled(257, 20241020, *start, mode=mode, discount=disc, want_sums=True)
                    what = f"{w.name}: simulate_sampled {mode} from {start}"
                    _same_result(a[0], b[0], what)
                    assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]), what


def test_xr_rollout_of_a_ping_pong_handle(sia, oracle):
    for w in _readout_instances("xr"):
        ref = pp.reference(oracle, w)
        disc = np.array([math.pow(w.functor.discountFactor, t) for t in range(w.T)])
        x, R = float(w.functor.iniInventory), float(w.functor.iniCash)
        with sia.SdpEngine(pp.ping_pong_desc(w), w.pmf, w.overhead()) as eng, sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as keep:
            eng.solve()
            keep.solve()
            for start in ((x, R), (x, R + 0.25)):  # (the second: R between cash keys, the first action is formed from V_2)
                for mode in ("lhs", "random"):
                    a = eng.xr_simulate(257, 20241020, *start, mode=mode, discount=disc, want_sums=True, want_demands=True)
                    b = keep.xr_simulate(257, 20241020, *start, mode=mode, discount=disc, want_sums=True, want_demands=True)
                    what = f"{w.name}: xr_simulate {mode} from {start}"
                    _same_result(a[0][0], b[0][0], what)
                    assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]), what
                    if start == (x, R):
                        want, valid = ref["P"].simulate(ref["V"], ref["pol"], a[2], disc, x, R)
                        assert valid.all() and a[1][0].tobytes() == want.tobytes(), what


def test_user_text_rollout_of_a_ping_pong_handle(sia, oracle):
    """CashOverdraftLimit's lambdas (outside the built-in families), T = 4: the tables against the oracle running the same text,
    custom_simulate from the grid start and from a start off the grid against a handle that keeps every table."""
    from test_gpu_custom_functor import _overdraft_limit_case
    shape, params, pmf = _overdraft_limit_case(sia)
    T = len(pmf)

    def desc(store_all):
        d = shape.to_desc(T, sia.OptDirection.MAX)
        d.discount_factor = 0.98
        d.store_all_values = store_all
        return d

    with oracle.custom_functor(cs.OVERDRAFT_LIMIT, params):
        V, pol, _ = oracle.Problem(desc(1), pmf).solve(nthreads=4)
    rng = np.random.default_rng(4)
    dem = np.stack([rng.choice(np.asarray(pmf[t])[:, 0], size=65) for t in range(T)], axis=1)
    disc = np.array([math.pow(0.98, t) for t in range(T)])
    with sia.SdpEngine(desc(0), pmf, custom_source=cs.OVERDRAFT_LIMIT, custom_params=params) as eng, \
            sia.SdpEngine(desc(1), pmf, custom_source=cs.OVERDRAFT_LIMIT, custom_params=params) as keep:
        eng.solve()
        keep.solve()
        _check_solved(sia, eng, {"V": V, "pol": pol}, "overdraft-limit")
        for ini in ((0.0, 10.0, 0.0), (0.5, 10.37, 0.0)):
            a, b = eng.custom_simulate(dem, disc, *ini), keep.custom_simulate(dem, disc, *ini)
            assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), ini
            assert np.array_equal(eng.last_sim_flags, keep.last_sim_flags), ini


# ---- 6. bookkeeping: which V_t a handle still holds ---------------------------------------------------------------------------
def _bookkeeping_cases():
    return [("f1_T3", lambda: fz.make_instance(1, 2)), ("f1_T4", lambda: fz.make_instance(1, 1)), ("f3_T4", lambda: fz.make_instance(3, 0))]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "after-two-graph-replays"])
@pytest.mark.parametrize("name,make", _bookkeeping_cases(), ids=[c[0] for c in _bookkeeping_cases()])
def test_a_period_run_again_invalidates_what_it_overwrites(sia, oracle, monkeypatch, name, make, graph):
    """Period T run a second time (after a whole sweep) writes V_T into table (T & 1), over V_2 (T = 4) or V_1 (T = 3): that table
    is refused from then on -- by values, by eval_states and an off-grid rollout start (which read V_2), by run_period(1) -- until
    the periods below T have been stepped again, which restores everything.  (With T = 3 it is V_1 that goes: V_2 stays valid, so
    period 1 may be run from it at once; that in turn overwrites V_3, and period 2 is refused.)  Before the flags of the whole
    parity were cleared, values(2) / values(1) returned V_T's numbers with status OK."""
    if graph:
        monkeypatch.setenv("SDPGPU_GRAPH", "1")
    else:
        monkeypatch.delenv("SDPGPU_GRAPH", raising=False)
    w = make()
    T, f = w.T, w.functor
    assert (name, T, w.desc().family) in (("f1_T3", 3, 1), ("f1_T4", 4, 1), ("f3_T4", 4, 3))
    ref = pp.reference(oracle, w)
    P, V = ref["P"], ref["V"]
    cash_family = w.desc().family == 3
    x, cash, _ = P.state_arrays(1)
    q1 = dict(cash=cash[:5] + 0.013) if cash_family else {}
    x2, cash2, _ = P.state_arrays(2)
    q2 = dict(cash=cash2[:5]) if cash_family else {}
    ini = (float(f.iniInventory), float(getattr(f, "iniCash", 0.0)), 0.0)
    off_grid = (ini[0], ini[1] + 0.37, 0.0)
    dem = np.stack([np.full(3, np.asarray(w.pmf[t])[0, 0]) for t in range(T)], axis=1)
    disc = np.ones(T)
    with sia.SdpEngine(pp.ping_pong_desc(w), w.pmf, w.overhead()) as eng:
        eng.solve()
        _check_solved(sia, eng, ref, f"{name}: first solve")
        eng.solve()
        _check_solved(sia, eng, ref, f"{name}: second solve")
        if graph:
            eng.solve()
            assert eng.stats().graph_replays == 2
            _check_solved(sia, eng, ref, f"{name}: second replay")
        _refused(sia, eng.eval_states, 2, x2[:5], **q2)  # needs V_3
        want1 = P.eval_states(1, V[1], x[:5], **q1)
        got1 = eng.eval_states(1, x[:5], **q1)
        assert np.array_equal(got1[0], want1[0]) and np.array_equal(got1[1], want1[1])
        if cash_family:
            assert eng.simulate(dem, disc, *off_grid)[0].shape == (3,)  # accepted while V_2 exists

        eng.run_period(T)  # (a period stepped by hand: it also drops a captured sweep)
        assert np.array_equal(eng.values(T), V[T - 1]), f"{name}: V_{T} run again"
        if T == 4:
            _refused(sia, eng.values, 2)
            assert np.array_equal(eng.values(1), V[0])  # table 1 is untouched
            _refused(sia, eng.eval_states, 1, x[:5], **q1)
            if cash_family:
                _refused(sia, eng.simulate, dem, disc, *off_grid)
            _refused(sia, eng.run_period, 1)
            _refused(sia, eng.run_period, 2)  # V_3 is gone as well
        else:
            _refused(sia, eng.values, 1)
            assert np.array_equal(eng.values(2), V[1])  # table 0 is untouched: with T = 3 nothing that reads V_2 is stale,
            eng.run_period(1)                           # and period 1 may be run from it at once
            assert np.array_equal(eng.values(1), V[0]) and np.array_equal(eng.policy(1), ref["pol"][0])
            _refused(sia, eng.values, 3)                # ... which in turn overwrote V_3
            _refused(sia, eng.run_period, 2)
            eng.run_period(T)
            _refused(sia, eng.values, 1)
        for t in range(T - 1, 0, -1):
            eng.run_period(t)
            assert np.array_equal(eng.values(t), V[t - 1]), f"{name}: V_{t} stepped again"
        _check_solved(sia, eng, ref, f"{name}: stepped T-1..1 again")
        if graph:
            eng.solve()  # the hand-stepped periods dropped the captured sweep: this one is eager
            assert eng.stats().graph_replays == 2
            _check_solved(sia, eng, ref, f"{name}: eager sweep after the hand-stepped periods")
        assert eng.stats().cells_evaluated == ref["cells"]
