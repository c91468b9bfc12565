"""The rollouts of one handle share one grow-only scratch block, one counter-zeroing step and one pair of timing events (the
host frame of csrc/sdpgpu_sim_host.hpp).  Calls of different entry points, path counts and rule counts, interleaved on ONE
handle, must not disturb each other: every output equals, bit for bit, what the same call returns on a FRESH handle -- also
where the block is larger than the call needs and stale partials, counters and sums of a larger call lie beyond the used range.
Path counts: the wave edges 63, 64, 65 and a call of several workgroups per rule (1025)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
import staff_cases  # noqa: E402
from test_cash_rule_host import SEED, setup_of  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(res):
    """The fields of the result records that a call determines (kernel_ms is a timing)."""
    res = res if isinstance(res, (list, tuple)) else [res]
    assert all(r.kernel_ms > 0 for r in res)
    return [(r.n_paths, r.n_valid, r.n_lost, np.float64(r.mean).tobytes(), np.float64(r.m2).tobytes()) for r in res]


def same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), what
        else:
            assert g == w, what


def test_cash_calls_interleaved_on_one_handle_equal_fresh_handles(sia):
    s = setup_of(cases.f3_testing)

    def engine():
        d = s.w.desc()
        d.device = 0
        return sia.SdpEngine(d, s.w.pmf, s.w.overhead())

    def table(eng):  # sdpgpu_simulate_sampled
        res, sums, flags = eng.simulate_sampled(65, SEED, *s.ini, discount=s.disc, want_sums=True)
        return bits(res) + [sums, flags]

    def rules(eng, n, which):  # sdpgpu_cash_rule_simulate
        res, sums = eng.cash_rule_simulate(n, SEED, *s.ini, s.forms[which], s.rules[which], c1_tab=s.c1[which], c2_tab=s.c2[which],
                                           discount=s.disc, want_sums=True, **s.scalars)
        assert sums.shape == (len(which), n)
        return bits(res) + [sums]

    def draws(eng):  # sdpgpu_sample_demands
        return list(eng.sample_demands(64, SEED))

    steps = [("simulate_sampled, n = 65", table, True), ("five rules, n = 1025 (the block grows)", lambda e: rules(e, 1025, list(range(5))), False),
             ("simulate_sampled, n = 65, again", table, True), ("two rules, n = 63 (stale parts beyond)", lambda e: rules(e, 63, [1, 3]), False),
             ("sample_demands, n = 64", draws, False), ("two rules, n = 63, again", lambda e: rules(e, 63, [1, 3]), False)]
    want = []
    for what, call, solved in steps:  # each call alone on a handle of its own
        with engine() as fresh:
            if solved:
                fresh.solve(sync=True)
            want.append(call(fresh))
    with engine() as eng:
        eng.solve(sync=True)
        got = [call(eng) for _, call, _ in steps]
    for (what, _, _), g, w in zip(steps, got, want):
        same(g, w, what)
    same(got[0], got[2], "steps 1 and 3")
    same(got[3], got[5], "steps 4 and 6")
    assert got[1][0][1] == 1025 and got[3][0][1] == 63 and got[0][0][1] > 0  # (n_valid: the rollouts ran on live paths)


def test_staff_calls_interleaved_on_one_handle_equal_fresh_handles(sia):
    c = staff_cases.staff_single()
    T = len(c.functor.minStaffNum)
    tree = (65,) + (1,) * (T - 1)
    ss = np.array([[m + 1.75, m + 4.25] for m in c.functor.minStaffNum])
    two = np.stack([ss, ss + 2.0])

    def engine():
        d = c.functor.to_desc(T)
        d.device = 0
        eng = sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len)
        eng.solve(sync=True)
        return eng

    def run(eng, levels):  # sdpgpu_staff_simulate
        res, sums, valid, dem = eng.staff_simulate(tree, SEED, c.functor.iniStaffNum, levels, want_sums=True, want_demands=True)
        assert sums.shape == (1 if levels is None else 2, 65)
        return bits(res) + [sums, valid, dem]

    steps = [("the table rule", None), ("two level rules", two), ("the table rule, again", None)]
    want = []
    for _, levels in steps:
        with engine() as fresh:
            want.append(run(fresh, levels))
    with engine() as eng:
        got = [run(eng, levels) for _, levels in steps]
    for (what, _), g, w in zip(steps, got, want):
        same(g, w, what)
    same(got[0], got[2], "steps 1 and 3")
