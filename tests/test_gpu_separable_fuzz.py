"""Randomised parity of the opt-in separable mode (desc.kernel = 3), every handle on kernel 3:

  * F1 (separable_f1_kernel) BIT FOR BIT against its numpy twin (tests/separable_twin.py) -- values and policy of every period on
    the seeded random, coarser-grid (steps 2 and 4), level-fuzz and degenerate family-1 instances: MIN and MAX, clamped and not,
    gapped supports, weights that do not sum to 1.  The mode's own statement against the oracle (values to 1e-9 relative; the
    oracle-order Q-value of the chosen action to 1e-9 relative of the oracle's optimum, at every state) is applied to the GPU's
    tables too.  Then rank slabs ragged against the 64-state tile, ping-pong value rows, and the two refusals.
  * F2 (separable_f2_table_kernel / _expand_kernel) and F5 (one cash row per level + level_fill_kernel) bit for bit against the
    ORACLE, from period 1, policy included, on the random, coarser-grid and degenerate instances, F2 also on rank slabs.
Sizes are those of test_gpu_fuzz.py: seconds per test."""
import numpy as np
import pytest

import separable_twin as st
import test_gpu_fuzz as tf
import test_gpu_parity as tp

pytestmark = pytest.mark.gpu


def _sep_desc(sia, w, **kw):
    d = w.desc()
    d.kernel = sia._abi.KERNEL_SEPARABLE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _solve_separable(sia, w, **kw):
    """Tables of periods 1 .. T of the separable mode on one rank."""
    with sia.SdpEngine(_sep_desc(sia, w, **kw), w.pmf, w.overhead()) as eng:
        eng.solve()
        assert eng.stats().kernel_used == 3, w.name
        return [eng.values(t) for t in range(1, w.T + 1)], [eng.policy(t) for t in range(1, w.T + 1)]


def _assert_tables(values, policy, V, pol, what):
    for t, (v, p) in enumerate(zip(values, policy), start=1):
        assert np.array_equal(p, pol[t - 1]), f"{what}: policy of period {t}"
        assert np.array_equal(v, V[t - 1]), f"{what}: values of period {t}"


def _solve_slabs(sia, w, world, threads=False):
    """sdpgpu_solve_multi over `world` rank handles of one device, V_1 gathered too: ([whole value tables of every rank],
    concatenated policy slabs)."""
    engs = []
    try:
        for r in range(world):
            engs.append(sia.SdpEngine(_sep_desc(sia, w, rank=r, world_size=world, device=0), w.pmf, w.overhead()))
        sia.SdpEngine.solve_multi(engs, sync=True, gather_first=True, threads=threads)
        values, slabs = [], [[] for _ in range(w.T)]
        for e in engs:
            assert e.stats().kernel_used == 3, w.name
            values.append([e.values(t) for t in range(1, w.T + 1)])
            for t in range(1, w.T + 1):
                _, lo, hi = e.slab(t)
                assert sum(len(s) for s in slabs[t - 1]) == lo   # the slabs follow one another
                slabs[t - 1].append(e.policy(t))
        return values, [np.concatenate(s) for s in slabs]
    finally:
        for e in engs:
            e.close()


# ---------------------------------------------------------------------------------------------------------------
# F1: the twin's bits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", st.F1_GROUPS)
def test_f1_bit_exact_against_the_twin(sia, oracle, group):
    worst_v = worst_q = 0.0
    for (w, P, V, pol, tV, tpol) in st.solved(oracle, group):
        gv, gp = _solve_separable(sia, w)
        _assert_tables(gv, gp, tV, tpol, w.name)
        v, q = st.oracle_side(w, P, V, gv, gp)
        assert v <= st.REL_TOL, f"{w.name}: values {v}"
        assert q <= st.REL_TOL, f"{w.name}: oracle-order Q of the chosen action {q}"
        worst_v, worst_q = max(worst_v, v), max(worst_q, q)
    print(f"{group}: worst value difference from the oracle {worst_v:.3g}, worst Q difference {worst_q:.3g}")


# (group, index): MIN clamped on seven tiles; MAX; unclamped, period 1 has ONE state; step 4, MAX; unclamped with 256 actions and a
# 129-point gapped support, 891 states; weights that do not sum to 1 on 95 states (two tiles: more ranks than tiles)
_SLAB_CASES = [("random", 22), ("random", 1), ("random", 39), ("step4", 16), ("level", 15), ("shapes", 19)]


@pytest.mark.parametrize("group,index", _SLAB_CASES, ids=[f"{g}-{i}" for g, i in _SLAB_CASES])
def test_f1_slabs_bit_exact_against_the_twin(sia, oracle, group, index):
    """2, 3, 5 and 7 ranks: slab bounds that are no multiple of the 64-state tile, more ranks than tiles (and than states).  Every
    rank ends with the twin's whole value tables; the policy slabs concatenate to the twin's."""
    w, P, V, pol, tV, tpol = st.solved(oracle, group)[index]
    if (group, index) == ("shapes", 19):
        assert w.name.endswith("zero_probabilities")
    for n, world in enumerate((2, 3, 5, 7)):
        values, policy = _solve_slabs(sia, w, world, threads=bool(n % 2))
        for r, v in enumerate(values):
            _assert_tables(v, tpol, tV, tpol, f"{w.name} rank {r}/{world}")
        _assert_tables(tV, policy, tV, tpol, f"{w.name} on {world} ranks")


def test_f1_ping_pong_value_rows(sia, oracle):
    """store_all_values = 0: V_1, V_2 and the policy of every period are those of the run that keeps every table (the twin's)."""
    for group, index in _SLAB_CASES:
        w, P, V, pol, tV, tpol = st.solved(oracle, group)[index]
        full_v, full_p = _solve_separable(sia, w)
        with sia.SdpEngine(_sep_desc(sia, w, store_all_values=0), w.pmf, w.overhead()) as eng:
            eng.solve()
            assert eng.stats().kernel_used == 3
            for t in range(1, min(w.T, 2) + 1):
                assert np.array_equal(eng.values(t), full_v[t - 1]) and np.array_equal(eng.values(t), tV[t - 1]), f"{w.name}: V_{t}"
            for t in range(1, w.T + 1):
                assert np.array_equal(eng.policy(t), full_p[t - 1]) and np.array_equal(eng.policy(t), tpol[t - 1]), f"{w.name}: policy {t}"


@pytest.mark.parametrize("A,D,message", [(6001, 2, "action range exceeds the LDS tile"),
                                         (5001, 3950, "action + demand range exceeds the LDS tile")],
                         ids=["6001-actions", "5001-actions-3950-demands"])
def test_f1_refuses_what_does_not_fit_the_lds(sia, A, D, message):
    """More than 6000 actions, and (64 + A + D - 1) window slots of 16 B + (64 + A) levels of 8 B beyond a compute unit's 160 KiB:
    SDPGPU_ERR_UNSUPPORTED, nothing launched."""
    from stochastic_inventory_amd.functors import BackorderFunctor
    from stochastic_inventory_amd.states import OptDirection
    from stochastic_inventory_amd.workloads import Workload
    f = BackorderFunctor(fixedOrderingCost=5, variOrderingCost=1, holdingCost=1, penaltyCost=4, minInventory=-10, maxInventory=80,
                         maxOrderQuantity=A - 1, iniInventory=0)
    tile = np.stack([np.arange(D, dtype=np.float64), np.full(D, 1.0 / D)], axis=1)
    w = Workload(f"sep_refuse_{A}x{D}", f, OptDirection.MIN, [tile, tile])
    with sia.SdpEngine(_sep_desc(sia, w), w.pmf, w.overhead()) as eng:
        with pytest.raises(sia.SdpgpuError) as e:
            eng.solve()
        assert e.value.code == 4 and message in e.value.message


# ---------------------------------------------------------------------------------------------------------------
# F2: the oracle's bits
# ---------------------------------------------------------------------------------------------------------------
def _f2_group(name):
    if name == "random":
        return [tf.make_instance(2, seed) for seed in range(40)]
    if name in ("step2", "step4"):
        return [tf.make_stepped_instance(2, 300 + seed, int(name[4:])) for seed in range(24)]
    if name == "window":   # the row-window kernel's generator: rows, action counts and pmfs far wider than the groups above
        import test_gpu_f2_window_fuzz as wf
        return wf.instances()
    return [tf.make_shaped_instance(2, 40 + seed, shape) for shape in tf.SHAPES if not shape.startswith("pmf_") for seed in range(3)]


@pytest.mark.parametrize("group", ["random", "step2", "step4", "shapes", "window"])
def test_f2_bit_exact_against_the_oracle(sia, oracle, group):
    ws = _f2_group(group)
    if group == "shapes":   # the instances without orders (one action, one pipeline plane) take part
        assert sum(1 for w in ws if w.functor.maxOrderQuantity == 0 and w.name.endswith("no_orders")) == 3
    lead2 = 0
    for w in ws:
        if group == "window":
            import test_gpu_f2_window_fuzz as wf
            V, pol, _ = wf.solved(oracle, w)    # (solved once for every test of that generator)
        else:
            V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=4)
        gv, gp = _solve_separable(sia, w)
        _assert_tables(gv, gp, V, pol, w.name)
        lead2 += w.desc().lead_time == 2
    assert lead2 > 0 and (group == "shapes" or lead2 < len(ws))   # both pipeline depths


# lead time 2, clamped, four periods; lead time 1 without the clamp (period 1 has one inventory level); step 2 with lead time 2; no
# orders (one action, one pipeline plane)
_F2_SLAB_CASES = [lambda: tf.make_instance(2, 3), lambda: tf.make_instance(2, 12), lambda: tf.make_stepped_instance(2, 315, 2),
                  lambda: tf.make_shaped_instance(2, 40, "no_orders")]


def test_f2_slabs_bit_exact_against_the_oracle(sia, oracle):
    """2, 3 and 5 ranks: every rank builds the whole table G and expands its slab."""
    ws = [make() for make in _F2_SLAB_CASES]
    assert {w.desc().lead_time for w in ws} == {1, 2} and {w.desc().step for w in ws} == {1.0, 2.0} and all(w.T > 2 for w in ws)
    for w in ws:
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=4)
        for world in (2, 3, 5):
            values, policy = _solve_slabs(sia, w, world)
            for r, v in enumerate(values):
                _assert_tables(v, pol, V, pol, f"{w.name} rank {r}/{world}")
            _assert_tables(V, policy, V, pol, f"{w.name} on {world} ranks")


# ---------------------------------------------------------------------------------------------------------------
# F5: the oracle's bits, or the one refusal
# ---------------------------------------------------------------------------------------------------------------
def _f5_exact_or_refused(sia, oracle, w):
    """The mode's tables are the oracle's.  It refuses (SDPGPU_ERR_UNSUPPORTED, "does not fit the cash row kernel") exactly where
    sdpgpu_run_period says it does: the pipeline axis has one plane (no orders), or the period is not eligible for the cash row
    kernel -- which the automatic path shows by running the generic kernel (kernel_used == 1) on the same instance (for these
    instances eligibility does not change from period to period: the cash axis and the pmf widths decide it).  Returns whether it ran."""
    P = oracle.Problem(w.desc(), w.pmf, w.overhead())
    V, pol, _ = P.solve(nthreads=8)
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as auto:
        auto.solve()
        auto_kernel = auto.stats().kernel_used
    may_refuse = P.grids[0].nq == 1 or auto_kernel == 1
    with sia.SdpEngine(_sep_desc(sia, w), w.pmf, w.overhead()) as eng:
        if may_refuse:
            with pytest.raises(sia.SdpgpuError) as e:
                eng.solve()
            assert e.value.code == 4 and "does not fit the cash row kernel" in e.value.message, w.name
            return False
        eng.solve()
        assert eng.stats().kernel_used == 3, w.name
        _assert_tables([eng.values(t) for t in range(1, w.T + 1)], [eng.policy(t) for t in range(1, w.T + 1)], V, pol, w.name)
        return True


def test_f5_random_instances_bit_exact_or_refused(sia, oracle):
    ran = [_f5_exact_or_refused(sia, oracle, tf.make_instance(5, seed)) for seed in range(16)]
    print(f"the separable mode ran on {sum(ran)} of {len(ran)} instances")
    assert not ran[9]                 # seed 9 has no orders: one pipeline plane
    assert sum(ran) >= len(ran) // 2  # the mode took part


@pytest.mark.parametrize("name", [n for n, _ in tp._od_cases()])
def test_f5_pair_kernel_cases_bit_exact(sia, oracle, name):
    """The cases of test_overdraft_pair_kernel_variants.  Four are the cash + lead-time family: exact, none refused.  The two
    overdraft instances (family 4, no pipeline) are outside the mode: refused by name."""
    w = dict(tp._od_cases())[name]
    if w.desc().family == 5:
        assert _f5_exact_or_refused(sia, oracle, w)
        return
    with sia.SdpEngine(_sep_desc(sia, w), w.pmf, w.overhead()) as eng:
        with pytest.raises(sia.SdpgpuError) as e:
            eng.solve()
        assert e.value.code == 4 and "backorder, lead-time and cash + lead-time families only" in e.value.message


def test_f5_large_magnitude_bit_exact(sia, oracle):
    """Balances around +-1e6 in hundredths on rows of 1500 - 4000 points (the two-point kernel, levels only): none refused."""
    for seed in range(9):
        assert _f5_exact_or_refused(sia, oracle, tf.make_large_magnitude_f5_instance(seed))
