"""CPU side of the separable mode's checks (no GPU): the numpy twin of separable_f1_kernel (tests/separable_twin.py) against
the oracle on the seeded random, coarser-grid, level-fuzz and degenerate family-1 instances -- the mode's own statement, 1e-9
relative on the values, and at EVERY state the oracle-order Q-value of the action the twin chose within 1e-9 relative of the
oracle's optimum (no cap on how many actions differ: on the random group 27 of 18 778 states differ, every one an exact tie in
the oracle's own arithmetic, and one instance differs on 4 % of its states).  Measured worst: 2.0e-15 on the values, 0 on the
Q-values.  tests/test_gpu_separable_fuzz.py then holds the GPU's tables against the twin bit for bit.

And the premise of the exact members of the mode (F2: separable_f2_*; F5: one cash row per level + level_fill_kernel): the
oracle's tables are equal on all states that share x + preQ (and q2 with lead time 2, and the cash point for F5)."""
import numpy as np
import pytest

import separable_twin as st
import test_gpu_fuzz as tf


@pytest.mark.parametrize("group", st.F1_GROUPS)
def test_oracle_order_q_reproduces_the_oracle(oracle, group):
    """oracle_order_q at the oracle's own policy is the oracle's V, bit for bit: the yardstick of the Q-check is the oracle's
    arithmetic, not a third one."""
    for (w, P, V, pol, _, _) in st.solved(oracle, group):
        for t in range(1, P.T + 1):
            q = st.oracle_order_q(w, P, t, V[t] if t < P.T else None, pol[t - 1])
            assert np.array_equal(q, V[t - 1]), f"{w.name} t={t}"


@pytest.mark.parametrize("group", st.F1_GROUPS)
def test_twin_within_the_modes_tolerance_of_the_oracle(oracle, group):
    worst_v = worst_q = 0.0
    differing = states = 0
    for (w, P, V, pol, tV, tpol) in st.solved(oracle, group):
        v, q = st.oracle_side(w, P, V, tV, tpol)
        assert v <= st.REL_TOL, f"{w.name}: values {v}"
        assert q <= st.REL_TOL, f"{w.name}: oracle-order Q of the twin's action {q}"
        worst_v, worst_q = max(worst_v, v), max(worst_q, q)
        differing += sum(int((a != b).sum()) for a, b in zip(tpol, pol))
        states += sum(len(a) for a in pol)
    print(f"{group}: worst value difference {worst_v:.3g}, worst Q difference {worst_q:.3g}, "
          f"{differing} of {states} actions differ")


def test_the_instances_cover_what_the_kernel_branches_on():
    ws = [w for g in st.F1_GROUPS for w in st.f1_group(g)]
    assert {w.desc().direction for w in ws} == {0, 1}
    assert {bool(w.desc().clamp_inventory) for w in ws} == {True, False}
    assert {w.desc().step for w in ws} == {1.0, 2.0, 4.0}
    assert any(np.any(np.diff(t[:, 0]) > w.desc().step) for w in ws for t in w.pmf)            # gapped supports
    sums = [float(np.sum(t[:, 1])) for w in ws for t in w.pmf]
    assert any(abs(s - 1.0) > 0.05 for s in sums) and any(s == 1.0 for s in sums)              # weights that do not sum to 1
    n_states = [int((w.desc().max_inventory - w.desc().min_inventory) / w.desc().step) + 1 for w in ws if w.desc().clamp_inventory]
    assert min(n_states) == 1 and max(n_states) > 4 * 64                                        # one state .. several tiles


def test_weights_that_do_not_sum_to_one_need_the_weight_sum(oracle):
    """The three family-1 zero_probabilities instances (weights zeroed without renormalising): with the weight sum the twin is
    the oracle's to rounding; c(a) + G(x + a), the mode before it carried the weight sum, is off by 1.7, 0.68 and 1.2 relative
    and chooses other actions on up to 45 % of the states -- these instances tell the two apart."""
    for seed, off in ((40, 1.7), (41, 0.68), (42, 1.2)):
        w = tf.make_shaped_instance(1, seed, "zero_probabilities")
        P = oracle.Problem(w.desc(), w.pmf, w.overhead())
        V, pol, _ = P.solve()
        assert max(st.oracle_side(w, P, V, *st.twin_solve(w, P))) <= st.REL_TOL
        v, q = st.oracle_side(w, P, V, *st.twin_solve(w, P, weight_sum=False))
        print(f"{w.name}: without the weight sum, values off by {v:.3g}, Q of the chosen actions by {q:.3g}")
        assert 0.9 * off < v < 1.1 * off


# ---------------------------------------------------------------------------------------------------------------
# The exact members: the tables depend on the level only
# ---------------------------------------------------------------------------------------------------------------
def f2_instances():
    ws = [tf.make_instance(2, seed) for seed in range(40)]
    ws += [tf.make_stepped_instance(2, 300 + seed, step) for step in (2, 4) for seed in range(24)]
    ws += [tf.make_shaped_instance(2, 40 + seed, shape) for shape in tf.SHAPES if not shape.startswith("pmf_") for seed in range(3)]
    return ws


def f5_instances():
    import test_gpu_parity as tp
    ws = [tf.make_instance(5, seed) for seed in range(16)]
    ws += [tf.make_shaped_instance(5, 40 + seed, shape) for shape in tf.SHAPES if not shape.startswith("pmf_") for seed in range(3)]
    ws += [w for _, w in tp._od_cases() if w.desc().family == 5]
    return ws + [tf.make_large_magnitude_f5_instance(seed) for seed in range(9)]


def _level_violations(P, V, pol):
    bad = states = 0
    for t in range(1, P.T + 1):
        g = P.grids[t - 1]
        x, _, preq = P.state_arrays(t)
        idx = np.arange(len(x))
        iq2 = idx // (g.nc * g.nx) // g.nq1
        ic = idx % g.nc
        level = np.round((x + preq - (g.x_lo)) / P.desc.step).astype(np.int64)
        key = (iq2 * (g.nx + g.nq1) + level) * g.nc + ic
        order = np.argsort(key, kind="stable")
        k, v, a = key[order], V[t - 1][order], pol[t - 1][order]
        same = k[1:] == k[:-1]
        bad += int((same & ((v[1:] != v[:-1]) | (a[1:] != a[:-1]))).sum())
        states += len(x)
    return bad, states


@pytest.mark.parametrize("family", [2, 5])
def test_tables_depend_on_the_level_only(oracle, family):
    """Every state of one level x + preQ (same q2 with lead time 2, same cash point for F5) has the oracle's value and action of
    the level's other states, bit for bit: what lets the F2 and F5 members evaluate one representative and copy it.  The
    seeded random, coarser-grid (F2; F5 takes step 1 only) and degenerate instances of test_gpu_fuzz.py, and for F5 also the
    pair-kernel cases of test_gpu_parity.py and the large balances: 190 402 and 3 649 305 states, no violation."""
    bad = states = 0
    lead2 = 0
    for w in (f2_instances() if family == 2 else f5_instances()):
        P = oracle.Problem(w.desc(), w.pmf, w.overhead())
        V, pol, _ = P.solve(nthreads=8)
        b, s = _level_violations(P, V, pol)
        assert b == 0, w.name
        bad, states = bad + b, states + s
        lead2 += P.desc.lead_time == 2
    print(f"family {family}: {bad} violations in {states} states")
    assert states > 100_000 and (family == 5 or lead2 > 10)
