"""Ping-pong value tables (store_all_values = 0): helpers of tests/test_pingpong_inputs.py (CPU) and tests/test_gpu_pingpong.py
(GPU).  No test lives here.

With two tables instead of T, V_t lives in table (t & 1) and both tables have the longest period's length.  On a grid that
grows with t the row of V_t is written over the longer V_{t+2}, and V_{t+1} is read from a table whose tail still holds
V_{t+3}: a kernel that touches a row's tail, or that assumes a clean destination, can only go wrong in this mode.  A whole
solve() shows V_1, V_2 and the policies alone, so run_ping_pong steps the periods by hand, compares EVERY V_t with the oracle's
while it exists, and overwrites what is stale before each period."""
import zlib

import numpy as np

# what stands in for the stale entries: nothing, NaN (any read shows, even one under a zero weight), or finite values of both
# signs that swamp every sum and win every arg-min / arg-max (a read under a zero weight does NOT show: the two tell the causes
# apart)
POISONS = (None, "nan", "finite")
BIG = 1e300


def poison_values(n, poison):
    """n entries of the poison (host array)."""
    if poison == "nan":
        return np.full(n, np.nan)
    if poison == "finite":
        out = np.full(n, BIG)
        out[1::2] = -BIG
        return out
    raise ValueError(poison)


_REFERENCES = {}


def reference(oracle, w):
    """The oracle's problem and its solved tables of an instance: computed once, shared, never changed."""
    key = (w.name, bytes(w.desc()), tuple(np.asarray(t).tobytes() for t in w.pmf))
    ref = _REFERENCES.get(key)
    if ref is None:
        P = oracle.Problem(w.desc(), w.pmf, w.overhead())
        V, pol, cells = P.solve(nthreads=8)
        for arr in list(V) + list(pol):
            arr.setflags(write=False)
        ref = _REFERENCES[key] = {"P": P, "V": V, "pol": pol, "cells": cells}
    return ref


def ping_pong_desc(w, kernel=0):
    d = w.desc()
    d.store_all_values = 0
    d.kernel = kernel
    return d


def run_ping_pong(sia, oracle, w, kernel=0, poison=None, custom=None):
    """One instance on the GPU on two value tables, the periods stepped T..1 by hand; returns the set of stats().kernel_used
    seen after the periods.  custom: (text, params) -- a USER-TEXT handle of a text that restates w's family
    (tests/custom_sources.py); the reference stays the built-in oracle.

    The arena is the caller's (sdpgpu_attach_values): table k starts at k * (arena / 2).  For t < T, values(t + 1) has been
    read, so the deferred read-out is flushed and the row of V_{t+1} is final.  With `poison`, before run_period(t):
    the WHOLE of table (t & 1) -- the destination, which holds the stale V_{t+2} -- and the tail of table ((t + 1) & 1) behind
    the S_{t+1} states of V_{t+1}, each out to the table's end, are overwritten.  After the period values(t) and policy(t) must
    be the oracle's (np.array_equal: same operation order, no tolerance), and the destination table behind its S_t states still
    holds the poison: the period wrote its own row and nothing else."""
    import torch
    ref = reference(oracle, w)
    T = w.T
    kw = {} if custom is None else dict(custom_source=custom[0], custom_params=custom[1])
    seen = set()
    with sia.SdpEngine(ping_pong_desc(w, kernel), w.pmf, w.overhead(), **kw) as eng:
        buf = torch.zeros(eng.values_bytes() // 8, dtype=torch.float64, device="cuda")
        eng.attach_values(buf.data_ptr(), buf.numel() * 8)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        table = buf.numel() // 2
        assert buf.numel() == 2 * table and table >= max(eng.num_states(t) for t in range(1, T + 1))
        for t in range(T, 0, -1):
            if t < T:
                assert np.array_equal(eng.values(t + 1), ref["V"][t]), f"{w.name} kernel {kernel}: V_{t + 1} before period {t}"
            off = (eng.values_device_ptr(t) - buf.data_ptr()) // 8
            assert off == (t & 1) * table and eng.num_states(t) == len(ref["V"][t - 1])
            if poison is not None:
                buf[off:off + table].copy_(torch.from_numpy(poison_values(table, poison)))
                if t < T:
                    nxt, S1 = ((t + 1) & 1) * table, eng.num_states(t + 1)
                    assert nxt != off and S1 <= table
                    if S1 < table:
                        buf[nxt + S1:nxt + table].copy_(torch.from_numpy(poison_values(table - S1, poison)))
            eng.run_period(t)
            gv, ga = eng.values(t), eng.policy(t)
            want_v, want_a = ref["V"][t - 1], ref["pol"][t - 1]
            what = f"{w.name} kernel {kernel} poison {poison} t={t} of {T}"
            assert np.array_equal(ga, want_a), f"{what}: policy ({int(np.sum(ga != want_a))} of {len(ga)} states)"
            assert np.array_equal(gv, want_v), f"{what}: values ({int(np.sum(gv != want_v))} of {len(gv)} states)"
            if poison is not None:  # the poison was there, and the period wrote its S_t states and nothing behind them
                S = len(want_v)
                tail = buf[off + S:off + table].cpu().numpy()
                assert tail.tobytes() == poison_values(table, poison)[S:].tobytes(), f"{what}: entries behind the row were written"
            seen.add(int(eng.stats().kernel_used))
    seen.discard(0)  # (what stats() reports is period 1's kernel: nothing before that period has run)
    return seen


def lengthen(w, T):
    """`w` with horizon T: the pmf tiles, and overheadCosts where the functor has them, cycled out to T periods (the counterpart
    of _one_period in tests/test_gpu_fuzz.py)."""
    tiles = list(w.pmf)
    w.pmf = [tiles[t % len(tiles)] for t in range(T)]
    f = w.functor
    if getattr(f, "overheadCosts", None) is not None:
        oh = list(f.overheadCosts)
        f.overheadCosts = [oh[t % len(oh)] for t in range(T)]
    w.name = f"{w.name}_T{T}"
    return w


def grid_grows(S):
    """Some V_t is written into the table that holds a LONGER V_{t+2} (S: states per period, period 1 first)."""
    return len(S) >= 3 and any(S[t + 2] > S[t] for t in range(len(S) - 2))


def states_per_period(w):
    """S_1 .. S_T by the oracle's layout (host arithmetic)."""
    from oracle import sdpref
    sdpref.build()
    return list(sdpref.Problem(w.desc(), w.pmf, w.overhead()).S)


FAMILIES = (1, 2, 3, 4, 5, 6)
OTHER_GROUPS = ("xr", "wide_cash", "big_cash", "big_f5")
BASE_SEEDS = 12                    # make_instance(family, 0 .. 11)
GROWING_BELOW = 40                 # F1 / F2: every seed below this with T >= 3 and a growing grid
STEPPED_SEEDS = (300, 301)         # make_stepped_instance(family, seed, 2); not F5 (the engine refuses a coarser pipeline grid)
SHAPES = ("one_inventory_level", "negative_demands", "demands_beyond_grid", "pmf_129_points")
SHAPE_SEED = 40
# (seed, T): seeds of make_instance lengthened; for F1 and F2 the first is UNCLAMPED (its grid grows over all T periods)
# (F2's second is a lead-time-2 instance, always clamped)
LENGTHENED = {1: ((4, 5), (1, 6)), 2: ((4, 5), (3, 6)), 3: ((0, 5), (3, 6)), 4: ((0, 5), (1, 6)), 5: ((2, 5), (5, 5)),
              6: ((0, 5), (1, 6))}


def lengthened(family):
    import test_gpu_fuzz as fz
    return [lengthen(fz.make_instance(family, seed), T) for seed, T in LENGTHENED[family]]


def instances(group):
    """The workloads of the ping-pong tests: group = a family 1..6 of tests/test_gpu_fuzz.py's generators, or one of
    OTHER_GROUPS."""
    import test_gpu_fuzz as fz
    if group == "xr":
        return [fz.make_xr_instance(s) for s in range(8)]
    if group == "wide_cash":
        return [fz.make_wide_cash_instance(s) for s in range(4)]
    if group == "big_cash":
        return [fz.make_large_magnitude_cash_instance(s) for s in range(3)]
    if group == "big_f5":
        return [fz.make_large_magnitude_f5_instance(s) for s in range(3)]
    family = int(group)
    out = [fz.make_instance(family, s) for s in range(BASE_SEEDS)]
    if family in (1, 2):
        for s in range(BASE_SEEDS, GROWING_BELOW):
            w = fz.make_instance(family, s)
            if w.T >= 3 and grid_grows(states_per_period(w)):
                out.append(w)
    if family != 5:
        out += [fz.make_stepped_instance(family, s, 2) for s in STEPPED_SEEDS]
    out += [fz.make_shaped_instance(family, SHAPE_SEED, shape) for shape in SHAPES]
    out += lengthened(family)
    return out


def instance_rng(w, what=""):
    return np.random.default_rng(zlib.crc32(f"{w.name}:{what}".encode()))
