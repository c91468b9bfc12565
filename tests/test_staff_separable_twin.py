"""The premise of the STAFF family's separable mode, on the CPU: tests/staff_separable_twin.py (the numpy restatement of
csrc/sdp_staff_sep.hpp) against oracle/staffref.c, and the launch plan a kernel = SEPARABLE workforce handle reports.

The mode reassociates the reference's sum, so its values agree with the oracle's to rounding, 1e-9 relative, and the hire count
may differ only where two actions tie to that rounding: wherever it differs, the twin's action -- evaluated in the REFERENCE's
operation order on the oracle's own V_{t+1} -- costs the oracle's V to 1e-9.  That holds for every instance; the share of
such states is capped per named case and over the fuzz as a whole."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import staff_block_cases as sb  # noqa: E402
import staff_cases  # noqa: E402
import staff_separable_twin as twin  # noqa: E402

REL_TOL = 1e-9
NAMED = [m.__name__ for m in staff_cases.ALL] + ["clamped_mid", "long_rows", "ragged_rows", "growing"]


@functools.lru_cache(maxsize=None)
def _case(name):
    return getattr(staff_cases, name)() if hasattr(staff_cases, name) else getattr(sb, name)()


def _rel(a, b):
    """Worst relative difference (an exact pair of zeros counts as no difference)."""
    r = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    r[(a == 0) & (b == 0)] = 0.0
    return float(r.max()) if len(r) else 0.0


def _against_oracle(c):
    """-> (worst relative value difference, states whose action differs, states); asserts the tie claim on every such state."""
    from oracle import staffref
    staffref.build()
    P = c.oracle_problem(staffref)
    V, pol, _ = P.solve(nthreads=8)
    tV, tpol = twin.solve(c, P)
    worst, differ, states = 0.0, 0, 0
    for t in range(1, c.T + 1):
        assert np.isfinite(tV[t - 1]).all(), (c.name, t)
        worst = max(worst, _rel(tV[t - 1], V[t - 1]))
        off = np.nonzero(tpol[t - 1] != pol[t - 1])[0]
        if len(off):
            q = twin.oracle_order_q(c, P, t, V[t] if t < c.T else None, tpol[t - 1])
            assert _rel(q[off], V[t - 1][off]) <= REL_TOL, (c.name, t, off[:5])
        differ += len(off)
        states += len(pol[t - 1])
    return worst, differ, states


@pytest.mark.parametrize("name", NAMED)
def test_named_cases_against_the_oracle(name):
    worst, differ, states = _against_oracle(_case(name))
    print(f"{name}: worst relative difference {worst:.3g}, {differ} of {states} states hire differently")
    assert worst <= REL_TOL
    assert differ <= 0.02 * states


def test_ties_are_the_oracles_bits():
    """fixCost = unitVariCost = salary = 0: c(a) = 0 and w is the bare penalty, so no rounding differs from the reference's."""
    from oracle import staffref
    staffref.build()
    c = _case("ties")
    P = c.oracle_problem(staffref)
    V, pol, _ = P.solve(nthreads=8)
    tV, tpol = twin.solve(c, P)
    for t in range(c.T):
        assert np.array_equal(tV[t], V[t]) and np.array_equal(tpol[t], pol[t]), t + 1


def test_fuzz_against_the_oracle():
    worst, differ, states, per = 0.0, 0, 0, []
    for c in twin.fuzz_cases():
        w, d, s = _against_oracle(c)
        worst, differ, states = max(worst, w), differ + d, states + s
        per.append(d / s)
    print(f"fuzz: worst relative difference {worst:.3g}, {differ} of {states} states hire differently, "
          f"{max(per):.3%} at worst in one instance")
    assert worst <= REL_TOL
    assert differ <= 0.02 * states


def test_oracle_order_q_is_the_oracles_value():
    """The yardstick of the tie claim itself: on the oracle's own actions it returns the oracle's V, bit for bit."""
    from oracle import staffref
    staffref.build()
    for name in ("staff_rates", "staff_testing_small", "staff_short_rows"):
        c = _case(name)
        P = c.oracle_problem(staffref)
        V, pol, _ = P.solve()
        for t in range(1, c.T + 1):
            assert np.array_equal(twin.oracle_order_q(c, P, t, V[t] if t < c.T else None, pol[t - 1]), V[t - 1]), (name, t)


def test_slab_rows_are_pieces_of_the_whole_rows():
    """A rank's G and P over the levels its slab reaches are the whole rows' entries (each level is its own serial sum)."""
    from oracle import staffref
    staffref.build()
    c = _case("staff_wide_actions")
    P = c.oracle_problem(staffref)
    V, _, _ = P.solve()
    n_actions = c.functor.maxHireNum + 1
    G, Ps = twin.g_rows(c, P, 1, V[1])
    for lo, hi in ((0, 31), (31, 61), (61, 91)):
        g, ps = twin.g_rows(c, P, 1, V[1], lo, hi)
        assert np.array_equal(g, G[lo: hi + n_actions - 1]) and np.array_equal(ps, Ps[lo: hi + n_actions - 1])


@pytest.mark.parametrize("name,states", [("staff_wide_actions", 91), ("clamped_wide", 8200)])
def test_plan_of_a_separable_handle(sia, name, states):
    """sdpgpu_plan_period, host arithmetic only: kernel = 3, one 64-state workgroup of the scan launch per tile, its static
    LDS (256 partial values and actions); an AUTO handle of the same instance keeps reporting the cell-by-cell form."""
    c = _case(name)
    d = c.functor.to_desc(c.T)
    d.kernel = sia._abi.KERNEL_SEPARABLE
    with sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len) as eng:
        for t in range(1, c.T + 1):
            pl = eng.plan(t)
            assert pl.kernel == 3
            assert (pl.r, pl.s, pl.chunks, pl.chunk_blocks) == (1, 1, 1, 0)
            assert pl.tiles == pl.tasks == -(-states // 64)
            assert pl.lds_bytes == 256 * 12 and pl.workgroups_per_cu == 0
    with sb.engine(sia, c) as eng:
        assert eng.plan(c.T).kernel == 1


def test_plan_of_a_separable_slab(sia):
    """Rank slabs: every rank reports the workgroups of its own slab."""
    c = sb.clamped_wide()
    tiles = []
    for rank in range(3):
        d = c.functor.to_desc(c.T)
        d.kernel, d.rank, d.world_size = sia._abi.KERNEL_SEPARABLE, rank, 3
        with sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len) as eng:
            _, lo, hi = eng.slab(c.T)
            pl = eng.plan(c.T)
            assert pl.kernel == 3 and pl.tiles == pl.tasks == -(-(hi - lo) // 64)
            tiles.append(pl.tiles)
    assert sum(tiles) >= -(-8200 // 64)
