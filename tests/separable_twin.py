"""Two plain numpy restatements for the opt-in separable F1 mode (separable_f1_kernel, csrc/sdp_window.hpp), written from
the kernel's and the oracle's descriptions with none of the library's code:

  * oracle_order_q: the Q-value of ONE given action per state in the REFERENCE's operation order -- imm = ((fixed + vari) +
    hold) + pen; `acc += p * imm` and then `acc += p * V_{t+1}[clamp]` as two rounded operations, demand ascending; the upper
    clamp, then the lower.  Vectorised over the states this is the oracle's arithmetic bit for bit: evaluated at the oracle's own
    policy it returns the oracle's V (tests/test_separable_twin.py asserts that), so it answers "what is the action the mode
    chose worth in the reference's own arithmetic".
  * twin_solve: the kernel itself.  Per period, G over the levels y = x_lo + e * step, e < S + A - 1, as `g += p * M(y - d)` and
    then `g += p * V_{t+1}[idx]`, demand ascending, with the kernel's window slots, clamp and index formula; P_t = the weights
    added in ascending order from 0.0; q = ((a > 0 ? K : 0) + v * a) * P_t + G(x + a); the lowest index among exactly equal
    optima (the kernel's four action slots each keep their first best and merge by value, then index), MIN or MAX.  The
    twin's own V_{t+1} feeds period t.  Every level is an exact multiple of the step and the library is built without FMA
    contraction, so the GPU's tables equal these bit for bit, whichever 64-state tile or rank slab formed them.

f1_group() gives the instances both the CPU and the GPU file run; solved() keeps oracle and twin tables of an instance."""
import numpy as np

REL_TOL = 1e-9   # the F1 mode's own parity statement (include/sdpgpu.h)


def rel(a, b):
    r = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    r[(a == 0) & (b == 0)] = 0.0
    return r


def _pos(a):
    """Math.max(a, 0) (a zero of either sign gives +0.0)."""
    return np.where(a > 0.0, a, 0.0)


def _n_actions(d):
    return int(d.max_order_quantity / d.step) + 1


def oracle_order_q(w, P, period, V_next, actions):
    """Q(state, actions[state]) of every grid state of `period` in the reference's operation order.  V_next: the table of
    period + 1 on the oracle's grid of that period (ignored for the last period)."""
    d = P.desc
    assert d.family == 1
    x = P.state_arrays(period)[0]
    k = np.asarray(actions, dtype=np.int64)
    assert k.shape == x.shape and k.min() >= 0 and k.max() < _n_actions(d)
    a = k.astype(np.float64) * d.step
    fixed = np.where(a > 0, d.fixed_order_cost, 0.0)
    vari = d.unit_order_cost * a
    future = period < P.T
    if future:
        gn = P.grids[period]
        V_next = np.asarray(V_next, dtype=np.float64)
        assert V_next.shape == (gn.nx,)
    acc = np.zeros(len(x))
    for dem, p in np.asarray(w.pmf[period - 1], dtype=np.float64):
        lev = x + a - dem
        hold = d.holding_cost * _pos(lev)
        pen = d.penalty_cost * _pos(-lev)
        imm = fixed + vari + hold + pen
        acc += p * imm
        if future:
            nx = lev
            if d.clamp_inventory:
                nx = np.where(nx > d.max_inventory, d.max_inventory, nx)
                nx = np.where(nx < d.min_inventory, d.min_inventory, nx)
            q = (nx - gn.x_lo) / d.step
            idx = q.astype(np.int64)
            assert np.all(idx == q) and idx.min() >= 0 and idx.max() < gn.nx   # (the oracle fails on a state off the grid)
            acc += p * V_next[idx]
    return acc


def twin_period(d, x, tile, next_x_lo, V_next, weight_sum=True):
    """One period of separable_f1_kernel.  x: the period's inventory levels; tile: [[demand, weight]]; V_next: V_{t+1} on the
    grid that starts at next_x_lo, None for the last period.  weight_sum=False is the mode as it was before it carried P_t
    (c(a) + G(x + a): WRONG when the weights do not sum to 1; never set by a test that compares with the GPU)."""
    step, inv_step = d.step, 1.0 / d.step
    S, A = len(x), _n_actions(d)
    x_lo = float(x[0])
    dem, p = tile[:, 0], tile[:, 1]
    d_min = float(dem[0])
    d_range = int((float(dem[-1]) - d_min) / step)
    span = S + A - 1
    # slot e of the window <-> level lev_lo + e * step, lev_lo = x_lo - d_max
    lev_lo = x_lo - (d_min + float(d_range) * step)
    lev = lev_lo + np.arange(span + d_range, dtype=np.float64) * step
    M = d.holding_cost * _pos(lev) + d.penalty_cost * _pos(-lev)
    if V_next is not None:
        nx = lev
        if d.clamp_inventory:
            nx = np.where(nx > d.max_inventory, d.max_inventory, nx)
            nx = np.where(nx < d.min_inventory, d.min_inventory, nx)
        idx = ((nx - next_x_lo) * inv_step).astype(np.int32)     # (int): towards zero
        idx = np.where(idx > len(V_next) - 1, len(V_next) - 1, idx)
        idx = np.where(idx < 0, 0, idx)
        Vw = V_next[idx]
    g = np.zeros(span)
    p_sum = 0.0
    for j in range(len(p)):
        pj = float(p[j])
        jd = int((float(dem[j]) - d_min) * inv_step)
        lo = d_range - jd
        g += pj * M[lo:lo + span]
        if V_next is not None:
            g += pj * Vw[lo:lo + span]
        p_sum += pj
    k = np.arange(A)
    a = k.astype(np.float64) * step
    c = (np.where(a > 0, d.fixed_order_cost, 0.0) + d.unit_order_cost * a) * (p_sum if weight_sum else 1.0)
    q = c[None, :] + g[np.arange(S)[:, None] + k[None, :]]
    best = q.argmax(axis=1) if d.direction == 1 else q.argmin(axis=1)   # the first of equal optima: the lowest index
    return q[np.arange(S), best], best.astype(np.int32)


def twin_solve(w, P, weight_sum=True):
    """(values, policy) of periods 1 .. T as separable_f1_kernel forms them, the twin's own V_{t+1} feeding period t."""
    d = P.desc
    assert d.family == 1
    V, pol = [None] * P.T, [None] * P.T
    for period in range(P.T, 0, -1):
        x = P.state_arrays(period)[0]
        future = period < P.T
        V[period - 1], pol[period - 1] = twin_period(d, x, np.asarray(w.pmf[period - 1], dtype=np.float64),
                                                     float(P.grids[period].x_lo) if future else 0.0,
                                                     V[period] if future else None, weight_sum)
    return V, pol


# ---------------------------------------------------------------------------------------------------------------
# The instances of tests/test_separable_twin.py (CPU) and tests/test_gpu_separable_fuzz.py (GPU)
# ---------------------------------------------------------------------------------------------------------------
F1_GROUPS = ("random", "step2", "step4", "level", "shapes")


def f1_group(name):
    import test_gpu_fuzz as tf
    import test_gpu_level_fuzz as tl
    if name == "random":
        return [tf.make_instance(1, seed) for seed in range(40)]
    if name in ("step2", "step4"):
        return [tf.make_stepped_instance(1, 300 + seed, int(name[4:])) for seed in range(24)]
    if name == "level":
        return [tl.make_level_instance(seed) for seed in range(36)]
    assert name == "shapes"
    return [tf.make_shaped_instance(1, 40 + seed, shape) for shape in tf.SHAPES for seed in range(3)]


_SOLVED = {}


def solved(oracle, group):
    """[(w, P, oracle V, oracle policy, twin V, twin policy)] of a group, computed once per session."""
    if group not in _SOLVED:
        out = []
        for w in f1_group(group):
            P = oracle.Problem(w.desc(), w.pmf, w.overhead())
            V, pol, _ = P.solve(nthreads=4)
            tV, tpol = twin_solve(w, P)
            out.append((w, P, V, pol, tV, tpol))
        _SOLVED[group] = out
    return _SOLVED[group]


def oracle_side(w, P, V, values, policy):
    """The two statements of the F1 mode against the oracle, for tables `values` / `policy` of periods 1 .. T (the twin's or
    the GPU's): (worst relative difference of the values, worst relative difference between the oracle's V and the
    oracle-order Q of the action the tables chose)."""
    worst_v = worst_q = 0.0
    for t in range(1, P.T + 1):
        worst_v = max(worst_v, float(rel(values[t - 1], V[t - 1]).max()))
        q = oracle_order_q(w, P, t, V[t] if t < P.T else None, policy[t - 1])
        worst_q = max(worst_q, float(rel(q, V[t - 1]).max()))
    return worst_v, worst_q
