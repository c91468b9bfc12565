"""The lead-time family on SCRAMBLED successor tables (tests/scrambled.py).  A lead-time-1 state enters the lambdas through
x + preQ alone, so a solved V_{t+1}[plane k][index i] is a function of i + k: a row-window kernel whose plane base and row offset
slip against each other (plane k + 1, index i - 1) still gives the oracle's table on every parity test that solves a recursion
(tests/test_scrambled_inputs.py measures it: no state changes).  Here every period below T is evaluated on a V_{t+1} of pairwise
distinct values and compared, bit for bit, with the oracle's evaluation of the same period on the same table, where that slip
changes most states: the (instance, period) pairs of scrambled.KEPT_F2 -- the row-window generator of
tests/test_gpu_f2_window_fuzz.py under its switch sets, and the named workloads of tests/test_gpu_parity.py's row-window tests
under theirs.  Every case asserts which kernel ran."""
import pytest

import scrambled
import test_gpu_f2_window_fuzz as wf
import test_gpu_parity as tp
from scrambled import run_scrambled

pytestmark = pytest.mark.gpu

GENERIC, WINDOW, EXACT_LEVELS = 1, 2, 3
_SWITCHES = ("SDPGPU_WIN_R", "SDPGPU_WIN_S", "SDPGPU_WIN_NCH")


def _set(monkeypatch, env):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _generator(sia, oracle, kernel):
    used = {}
    for seed, periods in sorted(scrambled.kept("window_fuzz", scrambled.KEPT_F2).items()):
        w = wf.make_row_window_instance(seed)
        used[w.name] = run_scrambled(sia, oracle, w, kernel=kernel, periods=periods)
    assert len(used) >= scrambled.MIN_KEPT
    return used


@pytest.mark.parametrize("env", wf.SWITCH_SETS, ids=wf._ids)
def test_row_window_plans(sia, oracle, monkeypatch, env):
    """The automatic plan and the forced S / R / chunk counts of test_row_window_plans_bit_exact."""
    _set(monkeypatch, env)
    used = _generator(sia, oracle, 0)
    assert set(used.values()) == {WINDOW}, used


@pytest.mark.parametrize("kernel", [GENERIC, EXACT_LEVELS], ids=["generic", "exact-level-mode"])
def test_other_kernels(sia, oracle, monkeypatch, kernel):
    _set(monkeypatch, {})
    used = _generator(sia, oracle, kernel)
    assert set(used.values()) == {kernel}, used


# ---------------------------------------------------------------------------------------------------------------
# The named workloads and switch lists of tests/test_gpu_parity.py's row-window tests (imported, not copied)
# ---------------------------------------------------------------------------------------------------------------
_NAMED = scrambled.f2_named_cases()


def _named(sia, oracle, prefix):
    keep = scrambled.kept("named", scrambled.KEPT_F2)
    names = [n for n in _NAMED if n.startswith(prefix)]
    assert names and all(n in keep for n in names)
    for n in names:
        assert run_scrambled(sia, oracle, _NAMED[n], periods=keep[n]) == WINDOW, n


@pytest.mark.parametrize("win_s", scrambled.parametrize_values(tp.test_f2_row_window_states_per_lane, "win_s"),
                         ids=lambda s: f"S{s}" if s else "planned")
def test_row_window_states_per_lane(sia, oracle, monkeypatch, win_s):
    _set(monkeypatch, {"SDPGPU_WIN_S": win_s} if win_s else {})
    _named(sia, oracle, "lanes:")


@pytest.mark.parametrize("env", scrambled.parametrize_values(tp.test_f2_row_window_block_plans, "env"), ids=wf._ids)
def test_row_window_block_plans(sia, oracle, monkeypatch, env):
    _set(monkeypatch, env)
    _named(sia, oracle, "blocks:")


# ---------------------------------------------------------------------------------------------------------------
# The padding between a table's S states and its slab belongs to the caller: nothing may depend on it
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [0.0, float("nan")], ids=["zeros", "nans"])
@pytest.mark.parametrize("lead", [1, 2])
def test_padding_of_the_callers_arena_is_not_read(sia, oracle, monkeypatch, lead, poison):
    """As test_gpu_scrambled_successor.test_padding_of_the_callers_arena_is_not_read: zeros or NaNs behind the last state of a
    V_{t+1} in the caller's arena, the handle the LAST rank of the smallest odd world that leaves some V_{t+1} ragged; the first
    kept instance of each lead time whose row-window launches are chunked (the last tile of the last plane borders the padding)."""
    _set(monkeypatch, {})
    for seed, periods in sorted(scrambled.kept("window_fuzz", scrambled.KEPT_F2).items()):
        w = wf.make_row_window_instance(seed)
        if w.functor.leadTime == lead and w.functor.maxOrderQuantity >= 16:
            break
    else:
        raise AssertionError("no instance")
    S = scrambled.reference(oracle, w)["P"].S
    world = next(n for n in (3, 5, 7, 11, 13) if any(S[t] % n for t in range(1, w.T)))
    assert run_scrambled(sia, oracle, w, poison=poison, periods=periods, rank=world - 1, world=world) == WINDOW
