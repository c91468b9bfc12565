"""Scrambled successor tables: helpers of tests/test_scrambled_inputs.py (CPU) and tests/test_gpu_scrambled_successor.py /
tests/test_gpu_survival_wide.py / tests/test_gpu_f2_scrambled_successor.py / tests/test_gpu_custom_scrambled.py (GPU).  No test lives here.

The value tables the recursion itself produces are almost constant along the cash axis for the cash families (V(x, cash) is an
expected cash INCREMENT: it does not depend on the balance while the order constraint is slack; survival probabilities are
plateaus of 0, gamma^k and 1), so a kernel that gathers V_{t+1} at a wrong cash key still gives the oracle's table.  Here a
period is evaluated on a V_{t+1} of pairwise distinct values instead, and compared with the oracle's evaluation of the same
period on the same table.

The lead-time family hides a different slip: a solved lead-time-1 table is a function of plane + index alone, so a gather that is
one plane up and one index down reads the same value (slip_antidiagonal, KEPT_F2)."""
import zlib

import numpy as np

THRESHOLD = 0.5      # an (instance, period) pair is kept when a slip of one key changes at least this share of its states
MAX_DROPPED = 1 / 3  # of a generator's tables
MIN_KEPT = 8         # tables of a generator
MIN_MEDIAN = 0.75    # of the kept tables' sensitivities, per generator


def scramble(n, lo, hi, rng):
    """n pairwise distinct finite values in [lo, lo + max(hi - lo, 1)): a random permutation of a jittered arithmetic
    progression.  lo, hi: the range of the solved table, so that the future terms keep the magnitude of the immediate values
    and both signs appear where they do in the solved table."""
    span = max(float(hi) - float(lo), 1.0)
    perm = rng.permutation(n).astype(np.float64)
    u = rng.uniform(0.25, 0.75, size=n)
    out = float(lo) + (perm + u) * (span / n)
    assert np.all(np.isfinite(out)) and len(np.unique(out)) == n
    return out


def slip(v, nc):
    """Every row of `v` (rows of nc cash keys) shifted by one key, last column kept: what a gather whose key is off by one reads."""
    rows = np.asarray(v, dtype=np.float64).reshape(-1, nc)
    out = rows.copy()
    out[:, :-1] = rows[:, 1:]
    return out.reshape(-1)


def slip_antidiagonal(v, grid):
    """The table whose entry (plane q, index i) is the entry (q + 1, i - 1) of `v`, the last plane and index 0 kept: what a
    gather of the lead-time family reads whose plane base and row offset slip against each other (grid: the oracle's Grid of the
    table's period, planes of nx inventory points).  A solved V_{t+1} of lead time 1 depends on q + i alone, so there the
    slipped table is the table itself away from its edges."""
    planes = np.asarray(v, dtype=np.float64).reshape(int(grid.nq), int(grid.nx))
    out = planes.copy()
    out[:-1, 1:] = planes[1:, :-1]
    return out.reshape(-1)


def antidiagonal_sensitivity(P, t, v_next, nthreads=8):
    """Share of the states of period t (family 2) whose value changes when V_{t+1} = v_next is read one plane up, one index down."""
    a = P.period(t, v_next, nthreads=nthreads)[0]
    b = P.period(t, slip_antidiagonal(v_next, P.grids[t]), nthreads=nthreads)[0]
    return float(np.mean(a != b))


def row_length(P, period):
    """Length of the fastest axis (the cash axis) of a cash family's table: the index of the first change of x in flat-index
    order.  (Not len(unique(cash)): the (x, R) state's second entry is R = cash + variCost * x.)"""
    x = P.state_arrays(period)[0]
    change = np.nonzero(x != x[0])[0]
    return int(change[0]) if len(change) else len(x)


def table_rng(name, t):
    """The generator of the table that stands in for V_{t+1} when period t of instance `name` is evaluated."""
    return np.random.default_rng(zlib.crc32(f"{name}:{t}".encode()))


def slip_sensitivity(P, t, v_next, nthreads=8):
    """Share of the states of period t whose value changes when every gather of V_{t+1} = v_next slips by one cash key."""
    a = P.period(t, v_next, nthreads=nthreads)[0]
    b = P.period(t, slip(v_next, row_length(P, t + 1)), nthreads=nthreads)[0]
    return float(np.mean(a != b))


_REFERENCES = {}


def reference(oracle, w):
    """The oracle's side of run_scrambled, computed once per instance and shared by every kernel variant: the problem, the
    solved tables, and per period t < T the scrambled V_{t+1} with the oracle's (values, policy) of period t on it."""
    key = (w.name, bytes(w.desc()), tuple(np.asarray(t).tobytes() for t in w.pmf))
    ref = _REFERENCES.get(key)
    if ref is None:
        P = oracle.Problem(w.desc(), w.pmf, w.overhead())
        V, pol, cells = P.solve(nthreads=8)
        ref = {"P": P, "V": V, "pol": pol, "cells": cells, "scrambled": {}}
        for t in range(w.T - 1, 0, -1):
            table = scramble(P.S[t], V[t].min(), V[t].max(), table_rng(w.name, t))
            v, a, _ = P.period(t, table, nthreads=8)
            for arr in (table, v, a):
                arr.setflags(write=False)
            ref["scrambled"][t] = (table, v, a)
        _REFERENCES[key] = ref
    return ref


def run_scrambled(sia, oracle, w, kernel=0, poison=None, periods=None, rank=0, world=1, custom=None, slabs=None):
    """One instance on the GPU, every period below T on a scrambled V_{t+1}; returns stats().kernel_used.
    custom: (text, params) -- the handle is a USER-TEXT handle (sdpgpu_create_custom) of a text that restates w's family
    (tests/custom_sources.py; tests/test_custom_functor.py proves on the CPU that it does), nothing else changes: the reference
    stays the built-in oracle.  slabs: a list that receives (t, lo, hi) of every period the handle ran.
    rank, world: the handle is that rank's slab of a sharded sweep (a table is padded to a multiple of `world` states: with one
    rank there is no padding); the whole V_{t+1} is written here, so no exchange is needed, and the slab's states are compared.

    The value arena is the caller's (sdpgpu_attach_values), the periods run T downwards (run_period refuses any other order).
    Period T is compared with the oracle's.  Then for t = T-1 .. 1: values(t + 1) flushes the deferred read-out, so that
    period t reads the fp64 row and not a key row; the scrambled table is copied over the row of V_{t+1} in the arena (with
    `poison`, the padding between its S states and its slab is filled with that value); run_period(t); values(t) and policy(t)
    against oracle.period(t, scrambled) with np.array_equal -- same operation order, no tolerance.
    periods: the t to compare (the pairs the sensitivity condition kept); the others still run, on their scrambled table.

    Not reached this way: with a caller's arena the F1 cut-off gate is off below T (values_external), and the keyed-input form
    of the window kernels is never taken (the flush above).  Both have their own twins and tests.  For a user-text handle a
    caller's arena turns nothing off: the generic loop has one form per launch size, chosen by the slab alone."""
    import torch
    ref = reference(oracle, w)
    d = w.desc()
    d.kernel = kernel
    d.rank, d.world_size = rank, world
    T = w.T
    kw = {} if custom is None else dict(custom_source=custom[0], custom_params=custom[1])
    with sia.SdpEngine(d, w.pmf, w.overhead(), **kw) as eng:
        buf = torch.zeros(eng.values_bytes() // 8, dtype=torch.float64, device="cuda")
        eng.attach_values(buf.data_ptr(), buf.numel() * 8)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.run_period(T)
        _, lo, hi = eng.slab(T)
        if slabs is not None:
            slabs.append((T, lo, hi))
        assert np.array_equal(eng.policy(T), ref["pol"][T - 1][lo:hi]), f"{w.name} kernel {kernel} t={T}: policy"
        assert np.array_equal(eng.values(T)[lo:hi], ref["V"][T - 1][lo:hi]), f"{w.name} kernel {kernel} t={T}: values"
        for t in range(T - 1, 0, -1):
            table, want_v, want_a = ref["scrambled"][t]
            eng.values(t + 1)
            off = (eng.values_device_ptr(t + 1) - buf.data_ptr()) // 8
            S, padded = eng.num_states(t + 1), eng.slab(t + 1)[0]
            assert S == len(table) and 0 <= off and off + max(S, padded) <= buf.numel()
            buf[off:off + S].copy_(torch.from_numpy(table))
            if poison is not None and padded > S:
                buf[off + S:off + padded] = poison
            eng.run_period(t)
            _, lo, hi = eng.slab(t)
            if slabs is not None:
                slabs.append((t, lo, hi))
            gv, ga = eng.values(t)[lo:hi], eng.policy(t)
            want_v, want_a = want_v[lo:hi], want_a[lo:hi]
            if periods is None or t in periods:
                what = f"{w.name} kernel {kernel} t={t} on a scrambled V_{t + 1}"
                assert np.array_equal(ga, want_a), f"{what}: policy ({int(np.sum(ga != want_a))} of {len(ga)} states)"
                assert np.array_equal(gv, want_v), f"{what}: values ({int(np.sum(gv != want_v))} of {len(gv)} states)"
        return int(eng.stats().kernel_used)


# ---------------------------------------------------------------------------------------------------------------
# The instances and the (instance, period) pairs the GPU tests run
# ---------------------------------------------------------------------------------------------------------------
def generators():
    """name -> (make(seed), seeds): the generators and seed lists of the scrambled GPU tests."""
    import test_gpu_fuzz as fz
    import test_gpu_survival_wide as sw
    out = {f"fuzz_f{f}": ((lambda s, f=f: fz.make_instance(f, s)), range(8 if f == 5 else 12)) for f in (3, 4, 5, 6)}
    out["xr"] = (fz.make_xr_instance, range(12))
    out["wide_cash"] = (fz.make_wide_cash_instance, range(12))
    out["big_cash"] = (fz.make_large_magnitude_cash_instance, range(8))
    out["big_cash_past_limit"] = ((lambda s: fz.make_large_magnitude_cash_instance(s, past_limit=True)), range(8))  # (0-3 alone leave 7 tables)
    out["big_f5"] = (fz.make_large_magnitude_f5_instance, range(6))
    out["wide_survival"] = (sw.make_wide_survival_instance, sw.SEEDS)
    return out


def named_cases():
    """name -> workload: the named cases of tests/test_gpu_parity.py's kernel-variant tests, as those tests build them."""
    import cases
    import test_gpu_parity as tp
    out = {}
    for make in parametrize_values(tp.test_cash_row_kernel_variants, "make"):
        w = make()
        if make is cases.f3_testing or make is cases.f3_xr:  # (as that test does: two-point kernels need the wider row)
            w.functor.maxCashState = 700.0
        out[f"row:{w.name}"] = w
    for name, w in tp._od_cases():
        out[f"od:{name}"] = w
    for make in parametrize_values(tp.test_cash_diag_kernel_variants, "make"):
        w = make()
        out[f"diag:{w.name}"] = w
    return out


def parametrize_values(test_function, argname):
    """The value list of one @pytest.mark.parametrize of an existing test (imported, not copied)."""
    for mark in test_function.pytestmark:
        if mark.name == "parametrize" and mark.args[0] == argname:
            return list(mark.args[1])
    raise KeyError(argname)


def custom_wide_cases():
    """name -> workload: the large-state instances of tests/test_gpu_custom_scrambled.py (cases.CUSTOM_WIDE)."""
    import cases
    return {w.name: w for w in (make() for make in cases.CUSTOM_WIDE)}


def f2_named_cases():
    """name -> workload: the named workloads of tests/test_gpu_parity.py's row-window tests, as those tests build them."""
    import test_gpu_parity as tp
    out = {f"lanes:{w.name}": w for w in (tp._f2_lane_workload(False), tp._f2_lane_workload(True))}
    w = tp._f2_block_workload()
    out[f"blocks:{w.name}"] = w
    return out


def f2_groups():
    """group -> [(key, workload)]: the lead-time instances of the scrambled tests (keys as in KEPT_F2)."""
    import test_gpu_f2_window_fuzz as wf
    return {"window_fuzz": [(seed, wf.make_row_window_instance(seed)) for seed in range(wf.N_INSTANCES)],
            "named": list(f2_named_cases().items())}


def measure_f2(oracle, instances):
    """[(key, t, sensitivity)] as measure(), for the anti-diagonal slip of the lead-time family."""
    out = []
    for key, w in instances:
        ref = reference(oracle, w)
        for t in range(1, w.T):
            out.append((key, t, antidiagonal_sensitivity(ref["P"], t, ref["scrambled"][t][0])))
    return out


def measure(oracle, instances):
    """[(key, t, sensitivity)] for every period with a future of every (key, workload) in `instances`."""
    out = []
    for key, w in instances:
        ref = reference(oracle, w)
        for t in range(1, w.T):
            out.append((key, t, slip_sensitivity(ref["P"], t, ref["scrambled"][t][0])))
    return out


def kept_prefix(group, n=None):
    """{seed: set of periods} of the first seeds of KEPT[group], in ascending order, that together cover at least n (default
    MIN_KEPT) pairs."""
    n = MIN_KEPT if n is None else n
    out, pairs = {}, 0
    for key, periods in sorted(kept(group).items()):
        if pairs >= n:
            break
        out[key] = periods
        pairs += len(periods)
    assert pairs >= n, group
    return out


def kept(group, table=None):
    """{seed or case name: set of periods} of a group of KEPT (table: KEPT_F2 for the lead-time family)."""
    out = {}
    for key, t in (KEPT if table is None else table).get(group, ()):
        out.setdefault(key, set()).add(t)
    return out


# (seed, t) -- or (case name, t) for "named" -- at or above THRESHOLD; tests/test_scrambled_inputs.py asserts that this is exactly
# what the oracle yields
KEPT = {
    "fuzz_f3": [(0, 1), (0, 2), (0, 3), (1, 1), (2, 1), (3, 1), (3, 2), (3, 3), (4, 1), (5, 1), (7, 1), (7, 2), (7, 3), (8, 1), (8, 3),
                (9, 1), (10, 1), (10, 2), (10, 3)],
    "fuzz_f4": [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (4, 1), (4, 2), (4, 3), (5, 1), (5, 2), (5, 3), (7, 1), (7, 2), (8, 1),
                (8, 2), (9, 1), (9, 2), (9, 3), (10, 1), (11, 1)],
    "fuzz_f5": [(0, 1), (2, 1), (2, 2), (3, 1), (5, 1), (5, 2), (6, 1), (7, 1), (7, 2)],
    "fuzz_f6": [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (3, 1), (6, 1), (6, 2), (6, 3), (7, 1), (9, 1), (10, 1),
                (10, 2), (10, 3), (11, 1), (11, 2)],
    "xr": [(0, 1), (0, 2), (1, 1), (1, 2), (1, 3), (4, 1), (4, 2), (4, 3), (5, 1), (5, 2), (5, 3), (6, 1), (6, 2), (8, 1), (9, 1), (9, 2),
           (9, 3), (10, 1)],
    "wide_cash": [(0, 1), (0, 2), (1, 1), (1, 2), (3, 1), (3, 2), (4, 1), (4, 2), (5, 1), (5, 2), (6, 1), (7, 1), (7, 2), (8, 1), (9, 1),
                  (10, 1), (10, 2), (11, 1)],
    "big_cash": [(0, 1), (1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (6, 1), (6, 2), (7, 1)],
    "big_cash_past_limit": [(0, 1), (1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (6, 1), (6, 2), (7, 1)],
    "big_f5": [(0, 1), (1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2), (5, 1), (5, 2)],
    "wide_survival": [(0, 1), (0, 2), (0, 3), (1, 1), (3, 1), (3, 2), (4, 1), (4, 2), (6, 1), (7, 1), (9, 1), (9, 2), (9, 3), (10, 1),
                      (11, 1), (11, 2), (11, 3), (13, 1), (13, 2), (13, 3), (14, 1), (14, 2), (14, 3), (16, 1)],
    "named": [("row:f3_grid_prices", 1), ("row:f3_grid_prices", 2), ("row:f3_half_grid_prices", 1), ("row:f3_half_grid_prices", 2),
              ("row:f3_testing", 1), ("row:f3_testing", 2), ("row:f3_testing", 3), ("row:f3_xr", 1), ("row:f3_xr", 2),
              ("od:f5_spl_shape", 1), ("od:f5_spl_shape", 2), ("od:f5_deposit_interest", 1), ("od:f5_deposit_interest", 2),
              ("od:f5_interest_free_band_half_grid_price", 1), ("od:f5_interest_free_band_half_grid_price", 2),
              ("od:f5_off_grid_price", 1), ("od:f5_off_grid_price", 2), ("od:f4_tenths", 1), ("od:f4_tenths", 2),
              ("od:f4_hundredths_fixed_cost_deposit", 1), ("od:f4_hundredths_fixed_cost_deposit", 2),
              ("diag:cfg3_cash_24x700x70x30x3", 1), ("diag:cfg3_cash_24x700x70x30x3", 2), ("diag:f3_dyadic_wide", 1),
              ("diag:f3_dyadic_wide", 2), ("diag:f3_dyadic_wide_min", 1), ("diag:f3_dyadic_wide_min", 2),
              ("diag:f3_dyadic_big_fixed", 1), ("diag:f3_dyadic_big_fixed", 2)],
    # cases.CUSTOM_WIDE: EVERY period with a future (test_custom_wide_pairs_are_all_sensitive)
    "custom_wide": [("f3_custom_wide", 1), ("f3_custom_wide", 2), ("f5_custom_wide", 1), ("f5_custom_wide", 2),
                    ("f6_custom_wide", 1), ("f6_custom_wide", 2)],
}

# The lead-time family (the row-window kernel): (seed, t) of test_gpu_f2_window_fuzz.make_row_window_instance, (case name, t) of
# f2_named_cases(), at or above THRESHOLD under slip_antidiagonal; asserted by test_kept_f2_pairs_are_the_sensitive_ones
KEPT_F2 = {
    "window_fuzz": [(1, 1), (1, 2), (3, 1), (3, 2), (4, 1), (4, 2), (5, 1), (6, 1), (12, 1), (13, 1), (14, 1), (15, 1), (15, 2), (18, 1),
                    (20, 1), (22, 1), (23, 1), (23, 2), (24, 1), (24, 2), (25, 1), (25, 2), (28, 1), (28, 2), (29, 1), (30, 1), (30, 2),
                    (33, 1), (33, 2), (34, 1), (34, 2), (36, 1), (37, 1), (38, 1), (38, 2), (41, 1), (41, 2), (44, 1), (45, 1), (46, 1)],
    "named": [("lanes:cfg4_leadtime_300x37q_37x30x3", 1), ("lanes:cfg4_leadtime_300x37q_37x30x3", 2),
              ("lanes:cfg4_pipeline_300x10q1x10q2_10x22x3", 1), ("lanes:cfg4_pipeline_300x10q1x10q2_10x22x3", 2),
              ("blocks:cfg4_leadtime_140x43q_43x120x2", 1)],
}
