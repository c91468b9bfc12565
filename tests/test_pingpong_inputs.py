"""CPU side of the ping-pong tests (tests/pingpong.py): the conditions on the selected instances that keep
tests/test_gpu_pingpong.py from being vacuous, on the oracle's layout alone.  A table is reused only from the third period on, and
a stale TAIL exists only where a period has fewer states than the one two periods later."""
import numpy as np
import pytest

import pingpong as pp
import test_gpu_fuzz as fz


def _T3(ws):
    return [w for w in ws if w.T >= 3]


@pytest.mark.parametrize("family", pp.FAMILIES)
def test_enough_instances_reuse_a_table(family):
    """Per family at least 6 selected instances have T >= 3 (a table is written a second time).  Among make_instance's seeds
    0..39 (F5: 0..15) 24 / 19 / 22 / 19 / 5 / 18 have; F5 reaches the bound through the lengthened instances."""
    n = 16 if family == 5 else 40
    have = sum(fz.make_instance(family, s).T >= 3 for s in range(n))
    assert have == {1: 24, 2: 19, 3: 22, 4: 19, 5: 5, 6: 18}[family]
    selected = _T3(pp.instances(family))
    print(f"family {family}: {len(selected)} selected instances with T >= 3")
    assert len(selected) >= 6
    names = [w.name for w in pp.instances(family)]
    assert len(set(names)) == len(names)  # (pingpong.reference is keyed by name)


@pytest.mark.parametrize("family,at_least", [(1, 7), (2, 4)])
def test_growing_grids_are_selected(family, at_least):
    """F1 has 7 and F2 has 4 seeds below 40 with T >= 3 and S[t+2] > S[t] for some t (an unclamped grid: V_t is written over a
    longer V_{t+2}); every one of them is selected, and the lengthened unclamped instance grows over all of its periods."""
    seeds = [s for s in range(pp.GROWING_BELOW)
             if fz.make_instance(family, s).T >= 3 and pp.grid_grows(pp.states_per_period(fz.make_instance(family, s)))]
    assert len(seeds) == at_least, seeds
    growing = [w for w in pp.instances(family) if pp.grid_grows(pp.states_per_period(w))]
    names = {w.name for w in growing}
    assert all(fz.make_instance(family, s).name in names for s in seeds)
    assert len(growing) >= at_least + 1
    long = pp.lengthened(family)[0]
    S = pp.states_per_period(long)
    assert not long.functor.clampInventory and long.T == 5 and all(b > a for a, b in zip(S, S[1:])), S


def test_cash_families_have_no_growing_grid():
    """The cash families are clamped: every period has the same grid, the stale row has the length of the new one."""
    for group in (3, 4, 5, 6) + pp.OTHER_GROUPS:
        for w in pp.instances(group):
            assert len(set(pp.states_per_period(w))) == 1, w.name


@pytest.mark.parametrize("family", pp.FAMILIES)
def test_lengthened_instances_solve_on_the_oracle(oracle, family):
    """Horizons 5 and 6 (F5: 5): the pmf tiles and overheads cycle, every period has a tile and an overhead, and the oracle's
    sweep finds every successor on the grid (it fails otherwise)."""
    ws = pp.lengthened(family)
    assert [w.T for w in ws] == [T for _, T in pp.LENGTHENED[family]] and len(ws) == 2
    assert {w.T for w in ws} == ({5} if family == 5 else {5, 6})
    for (seed, T), w in zip(pp.LENGTHENED[family], ws):
        base = fz.make_instance(family, seed)
        assert base.T < T and len(w.pmf) == T
        for t in range(T):
            assert np.array_equal(w.pmf[t], base.pmf[t % base.T])
        oh = w.overhead()
        if oh is not None:
            assert len(oh) == T and list(oh[:base.T]) == list(base.overhead())
        ref = pp.reference(oracle, w)  # raises on a successor off the grid
        assert len(ref["V"]) == T and ref["cells"] > 0
        assert all(len(ref["V"][t]) == ref["P"].S[t] for t in range(T))


def test_other_generators_counts():
    assert [len(pp.instances(g)) for g in pp.OTHER_GROUPS] == [8, 4, 3, 3]
    for g in pp.OTHER_GROUPS:
        assert len(_T3(pp.instances(g))) >= 1, g
