"""The cash kernels on SCRAMBLED successor tables (tests/scrambled.py): every period below T is evaluated on a V_{t+1} of
pairwise distinct values and compared, bit for bit, with the oracle's evaluation of the same period on the same table.  On the
tables the recursion itself produces a gather that reads a neighbouring cash key is mostly invisible;
here it changes most states.  Only the (instance, period) pairs that tests/test_scrambled_inputs.py shows to be sensitive
(scrambled.KEPT) are run.  Every case also asserts which kernel ran, as the parity test of its generator does."""
import pytest

import scrambled
import test_gpu_fuzz as fz
import test_gpu_parity as tp
from scrambled import run_scrambled

pytestmark = pytest.mark.gpu

GENERIC, SPECIALISED = 1, 2


def _ids(env):
    return ",".join(f"{k[7:]}={v}" for k, v in env.items()) or "default"


def _group(sia, oracle, group, make, kernel=0):
    """run_scrambled over the kept pairs of one generator; the kernels that ran, by instance name."""
    used = {}
    for seed, periods in sorted(scrambled.kept(group).items()):
        w = make(seed)
        used[w.name] = run_scrambled(sia, oracle, w, kernel=kernel, periods=periods)
    assert used
    return used


@pytest.mark.parametrize("kernel", [0, 1], ids=["auto", "generic"])
@pytest.mark.parametrize("family", [3, 4, 5, 6])
def test_random_instances(sia, oracle, family, kernel):
    used = _group(sia, oracle, f"fuzz_f{family}", lambda s: fz.make_instance(family, s), kernel)
    if kernel:
        assert set(used.values()) == {GENERIC}, used
    else:  # (as test_random_instances_bit_exact: the specialised kernels took part; narrow rows stay on the generic one)
        assert SPECIALISED in used.values() and set(used.values()) <= {GENERIC, SPECIALISED}, used


@pytest.mark.parametrize("kernel", [0, 1], ids=["auto", "generic"])
def test_random_xr_instances(sia, oracle, kernel):
    used = _group(sia, oracle, "xr", fz.make_xr_instance, kernel)
    if kernel:
        assert set(used.values()) == {GENERIC}, used
    else:  # (test_random_xr_instances_bit_exact sees both: rows under 32 points are the generic kernel's)
        assert SPECIALISED in used.values() and set(used.values()) <= {GENERIC, SPECIALISED}, used


@pytest.mark.parametrize("env", [{}, {"SDPGPU_CASH_DIAG": "0"}, {"SDPGPU_CASH_DIAG_S": "2"}, {"SDPGPU_CASH_SHIFT": "0"},
                                 {"SDPGPU_CASH_SHIFT": "0", "SDPGPU_CASH_PAIR": "0"}], ids=_ids)
def test_wide_cash_rows(sia, oracle, monkeypatch, env):
    """The diagonal and per-cell forms of the uniform-shift kernel, and the pair / row kernels behind them."""
    monkeypatch.setenv("SDPGPU_CASH_DIAG_CHECK", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    used = _group(sia, oracle, "wide_cash", fz.make_wide_cash_instance)
    assert set(used.values()) == {SPECIALISED}, used


@pytest.mark.parametrize("env,kernel", [({}, 0), ({"SDPGPU_CASH_PAIR": "0"}, 0), ({"SDPGPU_CASH_PAIR": "0", "SDPGPU_CASH_UNI": "0"}, 0),
                                        ({"SDPGPU_CASH_PAIR_S": "2"}, 0), ({}, 1)],
                         ids=["auto", "PAIR=0", "PAIR=0,UNI=0", "PAIR_S=2", "generic"])
def test_large_magnitude_cash(sia, oracle, monkeypatch, env, kernel):
    """The integer-domain clamp, the uniform-key trips and the LEAN elisions near the 5e8 admission bound, on tables where a slip
    of one key shows (on the solved tables of these instances it changes no state at all)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    used = _group(sia, oracle, "big_cash", fz.make_large_magnitude_cash_instance, kernel)
    assert set(used.values()) == {GENERIC if kernel else SPECIALISED}, used


def test_large_magnitude_cash_past_the_limit(sia, oracle):
    used = _group(sia, oracle, "big_cash_past_limit", lambda s: fz.make_large_magnitude_cash_instance(s, past_limit=True))
    assert set(used.values()) == {GENERIC}, used  # (the launcher falls back)


@pytest.mark.parametrize("env,kernel", [({}, 0), ({"SDPGPU_CASH_OD_PAIR": "0"}, 0), ({"SDPGPU_CASH_RW": "1"}, 0),
                                        ({"SDPGPU_CASH_DIAG_ORDER": "0"}, 0), ({}, 1)],
                         ids=["auto", "OD_PAIR=0", "RW=1", "DIAG_ORDER=0", "generic"])
def test_large_magnitude_f5(sia, oracle, monkeypatch, env, kernel):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    used = _group(sia, oracle, "big_f5", fz.make_large_magnitude_f5_instance, kernel)
    assert set(used.values()) == {GENERIC if kernel else SPECIALISED}, used


# ---------------------------------------------------------------------------------------------------------------
# The named cases and switch lists of tests/test_gpu_parity.py's kernel-variant tests (imported, not copied)
# ---------------------------------------------------------------------------------------------------------------
_NAMED = scrambled.named_cases()
_OD_ENVS = [e for e in scrambled.parametrize_values(tp.test_overdraft_pair_kernel_variants, "env")
            if e in ({}, {"SDPGPU_CASH_OD_PAIR": "0"}, {"SDPGPU_CASH_PAIR_S": "2"}, {"SDPGPU_CASH_RW": "1"})]
assert len(_OD_ENVS) == 4


def _named(sia, oracle, monkeypatch, prefix, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    keep = scrambled.kept("named")
    names = [n for n in _NAMED if n.startswith(prefix)]
    assert names and all(n in keep for n in names)
    for n in names:
        assert run_scrambled(sia, oracle, _NAMED[n], periods=keep[n]) == SPECIALISED, f"{n} {env}"


@pytest.mark.parametrize("env", scrambled.parametrize_values(tp.test_cash_row_kernel_variants, "env"), ids=_ids)
def test_cash_row_kernel_variants(sia, oracle, monkeypatch, env):
    _named(sia, oracle, monkeypatch, "row:", env)


@pytest.mark.parametrize("env", _OD_ENVS, ids=_ids)
def test_overdraft_pair_kernel_variants(sia, oracle, monkeypatch, env):
    _named(sia, oracle, monkeypatch, "od:", env)


@pytest.mark.parametrize("env", scrambled.parametrize_values(tp.test_cash_diag_kernel_variants, "env"), ids=_ids)
def test_cash_diag_kernel_variants(sia, oracle, monkeypatch, env):
    _named(sia, oracle, monkeypatch, "diag:", env)


# ---------------------------------------------------------------------------------------------------------------
# The padding between a table's S states and its slab belongs to the caller: nothing may depend on it
# ---------------------------------------------------------------------------------------------------------------
def _padding_instances():
    out = [(f"fuzz_f{f}", (lambda s, f=f: fz.make_instance(f, s))) for f in (3, 4, 5, 6)]
    return out + [("wide_cash", fz.make_wide_cash_instance), ("big_cash", fz.make_large_magnitude_cash_instance),
                  ("big_f5", fz.make_large_magnitude_f5_instance)]


@pytest.mark.parametrize("poison", [0.0, float("nan")], ids=["zeros", "nans"])
@pytest.mark.parametrize("group,make", _padding_instances(), ids=[g for g, _ in _padding_instances()])
def test_padding_of_the_callers_arena_is_not_read(sia, oracle, group, make, poison):
    """With sdpgpu_attach_values the library does not own the arena: zeros or NaNs between a table's last state and the end of
    its slab must give the same tables (one instance per family and per wide-row generator, automatic kernel).  A table is
    padded to a multiple of the world size, so the handle is the LAST rank (the one whose slab borders the padding) of the
    smallest odd world that leaves some V_{t+1} ragged."""
    seed, periods = sorted(scrambled.kept(group).items())[0]
    w = make(seed)
    S = scrambled.reference(oracle, w)["P"].S
    world = next(n for n in (3, 5, 7, 11, 13) if any(S[t] % n for t in range(1, w.T)))
    used = run_scrambled(sia, oracle, w, poison=poison, periods=periods, rank=world - 1, world=world)
    assert used in (GENERIC, SPECIALISED)
    if group in ("wide_cash", "big_cash", "big_f5"):
        assert used == SPECIALISED
