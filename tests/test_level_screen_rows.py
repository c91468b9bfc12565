"""The screen rows of the F1 level kernel (window_f1_level_kernel<..., CUT, RS>, csrc/sdp_window.hpp "THE SCREEN ROWS", DESIGN
4): a screened pass proves cells beaten and nothing else, and under the cut-off's gate the in-order sums of one lane and one
level are non-decreasing in the action -- so it walks RS of the block's R = 4 action rows and holds each row's sum against the
thresholds of every row it stands for.  Here, without a GPU: the lemma, in fp64 in the kernel's order of operations; a numpy
twin of the collapsed test that must never stop a block holding a cell that can win or tie, next to a deliberately wrong
variant (the base row's threshold only) that must; and the arithmetic that prices screened steps in sdpgpu_stats.  The device
tests are in tests/test_gpu_level_screen_rows.py."""
import numpy as np

import test_level_cutoff as tc
import test_level_screen as ts

R, S, NA = 4, 8, 256


def _m_cost(m, h, pi):
    """M(m): holding and penalty cost of level m, h max(m, 0) + pi max(-m, 0)."""
    m = np.asarray(m, dtype=np.float64)
    return h * np.maximum(m, 0.0) + pi * np.maximum(-m, 0.0)


def _walk(levels, c0, p, V, lo, n_states, h, pi, start=0):
    """Running sums of the cells (level y, action k) from step `start`, in the kernel's order: per step j ascending,
    acc += p_j (c0[k] + M(y - j)), then acc += p_j V(clamp(y - j)) where V is given; from +0.0.  Yields (j + 1, acc) after
    every step -- acc[y, k], the same for every action at one level but for the operand c0[k]."""
    acc = np.zeros((len(levels), len(c0)))
    for j in range(start, len(p)):
        m = levels - j
        acc = acc + p[j] * (c0[None, :] + _m_cost(m, h, pi)[:, None])
        if V is not None:
            acc = acc + (p[j] * V[np.clip(m - lo, 0, n_states - 1)])[:, None]
        yield j + 1, acc


def _c0(n, K, v):
    a = np.arange(n, dtype=np.float64)
    return np.where(a > 0, K, 0.0) + v * a


def test_lemma_in_order_sums_do_not_fall_with_the_action():
    """Random instances under the cut-off's gate -- K, v, h, pi >= 0 (K = 0 and v = 0 among them), p_j >= 0 with zeros,
    V_{t+1} >= 0 or absent or all zero, levels on both sides of 0, costs over many orders of magnitude: after EVERY step the
    in-order sum of action k + 1 at a level is >= that of action k (hence of every k' >= k), from step 0 and from a later
    start (a screened pass)."""
    rng = np.random.default_rng(20250320)
    checked = 0
    for case in range(60):
        n_act, D, n_states = int(rng.integers(2, 70)), int(rng.integers(3, 60)), int(rng.integers(20, 90))
        lo = -int(rng.integers(0, n_states + 30))
        K = 0.0 if case % 4 == 0 else float(10.0 ** rng.uniform(-3, 6))
        v = 0.0 if case % 5 == 0 else float(10.0 ** rng.uniform(-6, 3))
        h, pi = float(10.0 ** rng.uniform(-4, 3)), float(10.0 ** rng.uniform(-4, 4))
        p = rng.random(D) * np.exp(-0.5 * ((np.arange(D) - 0.5 * D) / (0.1 * D + 1)) ** 2)
        p[rng.random(D) < 0.2] = 0.0
        V = None if case % 3 == 0 else (np.zeros(n_states) if case % 3 == 1 and case % 2 else
                                        rng.random(n_states) * 10.0 ** rng.uniform(-2, 7, size=n_states))
        levels = np.arange(lo, lo + n_states + n_act - 1)
        for start in (0, D // 3):
            for _, acc in _walk(levels, _c0(n_act, K, v), p, V, lo, n_states, h, pi, start):
                assert np.all(acc[:, 1:] >= acc[:, :-1])
                checked += acc.size
    assert checked > 10 ** 6


# ---------------------------------------------------------------------------------------------------------------
# The numpy twin: every level block (S levels x one block of 64 R actions) of a small grid, screened from the host's
# screen_start with the cut-off's test every S steps (no test schedule, no mode rule, thresholds U(i) = Q(i, 0) as the slots
# start -- a slot only falls afterwards, which makes every rule stop earlier alike).  A lane holds actions
# kb + lane + 64 r; screen row q of RS stands for rows q G .. (q + 1) G - 1 and carries the c0 of its lowest live action.
# ---------------------------------------------------------------------------------------------------------------
def _carrier(n_pad, G):
    """For every padded action index: the action whose c0 its screen row carries."""
    k = np.arange(n_pad)
    kb, lane, r = k // NA * NA, k % 64, k % NA // 64
    base = kb + lane + 64 * (r // G * G)
    return np.where((base == 0) & (G > 1), 64, base)  # lane 0 of action block 0 skips action 0


def _twin(w, rules):
    """Per period (last first) and rule: the blocks each rule stops, and those of them that hold a live cell whose exact
    Q(i, k) does not exceed U(i) -- one that can still win or tie -- or that is the state's strict winner."""
    f, T = w.functor, w.T
    lo, n_states, A = int(f.minInventory), int(f.maxInventory - f.minInventory + 1), int(f.maxOrderQuantity + 1)
    K, v, h, pi = f.fixedOrderingCost, f.variOrderingCost, f.holdingCost, f.penaltyCost
    n_pad = -(-A // NA) * NA
    levels = np.arange(lo, lo + n_states + A - 1)
    state = levels[:, None] - np.arange(n_pad)[None, :] - lo  # state index of cell (level, action)
    real = (np.arange(n_pad)[None, :] < A) & (state >= 0) & (state < n_states)
    live = real & (np.arange(n_pad)[None, :] > 0)
    st = np.clip(state, 0, n_states - 1)
    c0 = _c0(n_pad, K, v)
    n_blk = -(-len(levels) // S)

    def by_block(cells):  # any() over the cells of every (level block, action block)
        pad = np.zeros((n_blk * S, n_pad), dtype=bool)
        pad[:len(levels)] = cells
        return pad.reshape(n_blk, S, n_pad // NA, NA).any(axis=(1, 3))

    out, V = [], None
    for t in range(T, 0, -1):
        p = np.zeros(-(-len(w.pmf[t - 1]) // S) * S)
        p[:len(w.pmf[t - 1])] = w.pmf[t - 1][:, 1]
        start = ts._rule(w.pmf[t - 1])
        assert start >= S
        for _, Q in _walk(levels, c0, p, V, lo, n_states, h, pi):
            pass
        Vt = np.full(n_states, np.inf)
        np.minimum.at(Vt, st[real], Q[real])
        U = Q[np.arange(n_states), 0]  # level i - lo + 0: cell (state i, action 0)
        assert np.all(Vt <= U)
        th = np.where(real, U[st], -np.inf)
        can_win = live & (Q <= th)
        wins = live & (Q == Vt[st]) & (Q < th)
        tests = range(start + S, len(p), S)
        first = {name: np.full(Q.shape, np.inf) for name in rules}  # per cell: the first test step at which it reads beaten
        for j, acc in _walk(levels, c0, p, V, lo, n_states, h, pi, start):
            if j not in tests:
                continue
            for name, (G, naive) in rules.items():
                car = _carrier(n_pad, G)
                mine = acc[:, car]  # the sum the cell's screen row carries
                if naive:  # WRONG on purpose: a screen row tested against its base row's threshold alone
                    beaten = np.where((np.arange(n_pad) == car)[None, :], mine > th, True)
                else:
                    beaten = mine > th
                first[name] = np.where(beaten & np.isinf(first[name]), j, first[name])
        res = {}
        for name in rules:
            stop = np.where(live, first[name], 0.0).reshape(-1, n_pad)
            pad = np.zeros((n_blk * S, n_pad))
            pad[:len(levels)] = stop
            blk = pad.reshape(n_blk, S, n_pad // NA, NA).max(axis=(1, 3))  # inf: the block runs to the end
            stopped = np.isfinite(blk) & by_block(live)
            steps = np.where(stopped, blk, len(p)) - start
            res[name] = (stopped, stopped & by_block(can_win), stopped & by_block(wins), int(steps[by_block(live)].sum()))
        out.append(res)
        V = Vt
    return out


_RULES = {"full": (1, False), "two rows": (2, False), "one row": (4, False), "naive one row": (4, True)}
_TWIN = {}


def _twin_grid():
    """700 states from -120, 300 actions, 200 demands, two periods, h = 0.2: the ordering region is a fifth of the states."""
    if not _TWIN:
        w = tc._grid(700, 300, 200, T=2, lo=-120, h=0.2)
        _TWIN["w"], _TWIN["res"] = w, _twin(w, _RULES)
    return _TWIN["w"], _TWIN["res"]


def test_collapsed_rules_never_stop_a_block_that_can_win():
    """RS = 4 (the full test), 2 and 1: blocks are stopped in every period, and no stopped block holds a live cell whose
    exact sum is <= its threshold.  The collapsed rules stop a subset of what the full test stops by the same step, at a
    few per cent more steps."""
    _, res = _twin_grid()
    for period, r in zip((2, 1), res):
        full = r["full"]
        for name in ("full", "two rows", "one row"):
            stopped, can_win, wins, steps = r[name]
            print(f"period {period}, {name}: {int(stopped.sum())} blocks stopped, {steps} screened steps")
            assert stopped.sum() > 0
            assert not can_win.any() and not wins.any(), f"period {period}, {name}"
            assert not (stopped & ~full[0]).any()  # a collapsed sum is <= the row's own: it proves no more
            assert full[3] <= steps <= 1.05 * full[3]
        assert r["full"][3] <= r["two rows"][3] <= r["one row"][3]


def test_the_naive_one_row_rule_is_wrong_on_this_grid():
    """The base row's threshold alone: it stops at least one block that holds the strict winner of a state -- what the
    device parity test on grids with levels below 0 is there to catch."""
    _, res = _twin_grid()
    bad = sum(int(r["naive one row"][2].sum()) for r in res)
    print("blocks with a winning cell that the naive rule stops, per period (last first):",
          [int(r["naive one row"][2].sum()) for r in res])
    assert bad >= 1
    assert all(r["naive one row"][3] < r["one row"][3] for r in res)  # it stops earlier, which is the point


# ---------------------------------------------------------------------------------------------------------------
# The operation model (sdpgpu_f1_level_ops_model, what sdpgpu_stats_get charges a level period that counted its steps)
# ---------------------------------------------------------------------------------------------------------------
def test_ops_model_prices_exact_and_screened_steps_separately(sia):
    lib = sia._abi.load()
    ops3 = 3.0 + 1.0 / S + 1.0 / (64.0 * R)  # with a future term
    ops2 = 2.0 + 1.0 / S  # period T
    planned, run, scr, tests = 10_000_000, 4_321_000, 3_900_000, 123_456

    def model(ops, future, rs, screened=scr):
        return lib.sdpgpu_f1_level_ops_model(ops, future, R, S, rs, planned, run, screened, tests)

    for ops, future in ((ops3, 1), (ops2, 0)):
        # RS = R is the figure from before the collapse, whatever part of the steps was screened: bit for bit
        today = ops * (run / planned) + tests / planned
        assert model(ops, future, 4) == today == model(ops, future, 4, 0)
        per = 3 if future else 2
        got = []
        for rs in (2, 1):
            lane_ops = rs * S * per + rs + (S / 64.0 if future else 0.0)  # of a screened step, over R S nominal cells
            want = (ops * (run - scr) + lane_ops / (R * S) * scr + tests) / planned
            got.append(model(ops, future, rs))
            assert abs(got[-1] - want) <= 4 * np.finfo(float).eps * want
            assert model(ops, future, rs, 0) == today  # nothing screened: nothing cheaper
        assert today > got[0] > got[1] > ops * ((run - scr) / planned)
    for bad in ((ops3, 1, R, S, 3, planned, run, scr, tests), (ops3, 1, R, S, 2, planned, run, run + 1, tests),
                (0.0, 1, R, S, 2, planned, run, scr, tests), (ops3, 1, R, S, 2, 0, 0, 0, 0)):
        assert lib.sdpgpu_f1_level_ops_model(*bad) == -1.0


def test_screen_rows_switch_is_read_at_create_time(sia, monkeypatch):
    """SDPGPU_F1_SCREEN_ROWS: 1, 2 and 4 are taken, unset is 2, anything else is refused with a reason (no device needed)."""
    import pytest
    w = tc._grid(700, 130, 16)
    for value, want in ((None, 2), ("1", 1), ("2", 2), ("4", 4)):
        monkeypatch.delenv("SDPGPU_F1_SCREEN_ROWS", raising=False)
        if value is not None:
            monkeypatch.setenv("SDPGPU_F1_SCREEN_ROWS", value)
        with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
            assert eng.f1_screen_rows(1) == (0, want)
    for value in ("3", "0", "8", "two", "", "2x"):
        monkeypatch.setenv("SDPGPU_F1_SCREEN_ROWS", value)
        with pytest.raises(sia._abi.SdpgpuError, match="SDPGPU_F1_SCREEN_ROWS"):
            sia.SdpEngine(w.desc(), w.pmf, w.overhead())
