"""The screen of the F1 level kernel (window_f1_level_kernel<..., CUT>, csrc/sdp_window.hpp "THE SCREEN"): a level
block whose predecessor stopped at the cut-off is first walked from step screen_start with its sums started at +0.0 -- a
lower bound of every cell, enough to prove the block beaten -- and walked again from step 0 when that fails.  Here, without a
GPU: the lemma the bound rests on, in fp64 as the device adds, and the host's rule for screen_start.  The device tests are in
tests/test_gpu_level_screen.py."""
import numpy as np

import test_level_cutoff as tc
from stochastic_inventory_amd import workloads

MASS = 2.0 ** -16  # kF1ScreenMass (csrc/sdpgpu_internal.hpp)


def _sum_in_order(xs):
    acc = 0.0
    for x in xs:
        acc = acc + float(x)
    return acc


def test_lemma_dropping_addends_never_raises_an_in_order_sum():
    """Round-to-nearest addition is monotone in both operands and fl(x + 0) = x: replace any addends of a non-negative
    sequence by +0.0 and the in-order fp64 sum cannot grow.  Seeded random sequences, some with addends spread over 40 orders
    of magnitude (where nearly every addition rounds); suffixes -- what a screened block sums -- and arbitrary subsequences."""
    rng = np.random.default_rng(20240611)
    checked = 0
    for case in range(300):
        n = int(rng.integers(2, 400))
        if case % 3 == 0:
            xs = rng.random(n)
        elif case % 3 == 1:
            xs = 10.0 ** rng.uniform(-20.0, 20.0, size=n)
        else:  # a pmf-like head of tiny weights in front of the mass, times costs of mixed size
            xs = np.exp(-0.5 * ((np.arange(n) - 0.6 * n) / (0.05 * n + 1)) ** 2) * 10.0 ** rng.uniform(-3.0, 6.0, size=n)
            xs[rng.random(n) < 0.1] = 0.0
        whole = _sum_in_order(xs)
        for start in sorted({0, 1, n // 3, n // 2, n - 1} | set(int(v) for v in rng.integers(0, n, size=4))):
            assert _sum_in_order(xs[start:]) <= whole
            checked += 1
        for _ in range(4):
            keep = rng.random(n) < rng.uniform(0.05, 0.95)
            assert _sum_in_order(xs[keep]) <= whole
            assert _sum_in_order(np.where(keep, xs, 0.0)) == _sum_in_order(xs[keep])  # adding +0.0 changes nothing
            checked += 1
    assert checked >= 3000


def _rule(tile, S=8, mass=MASS):
    """The host's rule, written again: the largest multiple of S whose leading steps carry at most `mass` of the probability,
    0 below S.  `tile` is [[d, p_d]] on unit-stride demands."""
    p = tile[:, 1]
    bound = mass * _sum_in_order(p)
    head, n = 0.0, 0
    while n < len(p) and head + p[n] <= bound:
        head += p[n]
        n += 1
    start = n // S * S
    return start if S <= start < len(p) else 0


def test_screen_start_rule_on_the_target_tiles(sia, monkeypatch):
    """The six demand tiles of the target grid (Poisson, means 122, 122, 100, 78, 78, 100 on 200 points): the library's
    screen_start, the rule written again above, and the figures themselves -- under the bound 2^-24 (64, 64, 48, 32, 32, 48)
    and under the bound the library ships, 2^-16, one block of 8 steps further."""
    w = workloads.target_grid()
    for log2, want in ((24, [64, 64, 48, 32, 32, 48]), (None, [72, 72, 56, 40, 40, 56]), (32, [56, 56, 40, 24, 24, 40])):
        monkeypatch.delenv("SDPGPU_F1_SCREEN_LOG2", raising=False)
        if log2 is not None:
            monkeypatch.setenv("SDPGPU_F1_SCREEN_LOG2", str(log2))
        with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
            got = [eng.f1_screen_start(t) for t in range(1, w.T + 1)]
            assert eng.f1_screen(1) == (0,) * 6  # nothing has run
        assert got == [_rule(t, mass=MASS if log2 is None else 2.0 ** -log2) for t in w.pmf]
        assert got == want, f"bound 2^-{log2 or 16}"


def test_screen_start_rule_edges(sia, monkeypatch):
    """A first step that carries 1/16 of the mass (the dyadic pmf of test_cutoff_ties_where_blocks_stop), a pmf too short for
    one block of S steps, and a support with gaps (laid out on unit-stride steps, probability 0 in the gaps): 0, 0, and the
    rule on the laid-out steps.  The two-period grid of tests/test_gpu_level_prefetch.py has Poisson(100) tiles: 56 (under
    2^-24 it would be 48: 56 leading steps carry more than that)."""
    monkeypatch.delenv("SDPGPU_F1_SCREEN_LOG2", raising=False)
    pmf = [np.column_stack([np.arange(24.0), np.full(24, 1.0 / 32)]) for _ in range(2)]
    for t in pmf:
        t[:8, 1] = 2.0 / 32
    d = np.concatenate([[0.0, 3.0], np.arange(17.0, 51.0)])
    gaps = np.column_stack([d, np.concatenate([[1e-12, 1e-11], np.full(len(d) - 2, 1.0 / (len(d) - 2))])])
    dense = np.column_stack([np.arange(51.0), np.zeros(51)])
    dense[gaps[:, 0].astype(int), 1] = gaps[:, 1]
    w = tc._grid(1200, 400, 24, T=2)
    for tiles, want in ((pmf, [0, 0]), ([workloads.truncated_poisson_tile(3.0, 7)] * 2, [0, 0]), ([gaps, gaps], [16, 16])):
        w.pmf = tiles
        with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
            assert [eng.f1_screen_start(t) for t in (1, 2)] == want
    assert _rule(dense) == 16
    w2 = tc._grid(26000, 300, 200, T=2, lo=-300, h=0.2)
    with sia.SdpEngine(w2.desc(), w2.pmf, w2.overhead()) as eng:
        assert [eng.f1_screen_start(t) for t in (1, 2)] == [56, 56]
    p = w2.pmf[0][:, 1]
    assert _sum_in_order(p[:48]) <= 2.0 ** -24 * _sum_in_order(p) < _sum_in_order(p[:56]) <= MASS * _sum_in_order(p)
