"""Plain Python / numpy twins of the structure checks, written from the reference and independently of the C++:

  * check    -- sdp.inventory.CheckKConvexity.check   (CheckKConvexity.java:39-68)
  * check_ck -- sdp.inventory.CheckKConvexity.checkCK (CheckKConvexity.java:6-36)
  * gy       -- the expected cost of standing at level y in period t: the second Recursion of capacitated.CLSPforDraw.main
                (CLSPforDraw.java:147-170: fixedCost 0, variableCost v * y, level y - d) summed as Recursion.java:138-143 sums,
                for any period

Only the innermost index is vectorised, and every fp64 step of the reference's expression is its own elementwise numpy
operation (numpy contracts nothing into an FMA), so each number is rounded exactly as the Java double arithmetic rounds it.
A row is g[0 .. n) at consecutive grid points; the reference's xLength is n for such rows.

Results are tuples (holds, i0, i1, i2, lhs, rhs): (1, -1, -1, -1, 0.0, 0.0) when no triple violates, else the FIRST violating
triple in loop order with the two numbers the reference prints there.
"""
import numpy as np

HOLDS = (1, -1, -1, -1, 0.0, 0.0)


def _first_violation(lhs, rhs0):
    """Index of the first element with !(lhs > rhs0 - 0.1), or -1.  (NaN compares false: a violation.)"""
    with np.errstate(all="ignore"):
        ok = lhs > rhs0 - 0.1
    bad = np.flatnonzero(~ok)
    return int(bad[0]) if len(bad) else -1


def check(g, K):
    g = np.asarray(g, dtype=np.float64)
    n = len(g)
    K = np.float64(K)
    with np.errstate(all="ignore"):
        for a in range(n):
            for b in range(a):
                if b == 0:
                    continue  # no c
                c = np.arange(b)
                t = g[b] - g[c]
                t = np.float64(a - b) * t
                t = t / (b - c).astype(np.float64)
                rhs0 = g[b] + t
                lhs = np.full(b, g[a] + K)
                k = _first_violation(lhs, rhs0)
                if k >= 0:
                    return (0, a, b, k, float(lhs[k]), float(rhs0[k]))
    return HOLDS


def check_ck(g, K, capacity):
    g = np.asarray(g, dtype=np.float64)
    n = len(g)
    K = np.float64(K)
    with np.errstate(all="ignore"):
        for y in range(n):
            for z in range(max(capacity, 0)):
                if y + z >= n:
                    break  # every b is skipped from here on
                # b = 1 .. capacity - 1 with y - b > 0
                b = np.arange(1, min(capacity, y))
                if len(b) == 0:
                    break
                t = g[y] - g[y - b]
                t = np.float64(z) * t
                t = t / b.astype(np.float64)
                rhs0 = g[y] + t
                lhs = np.full(len(b), g[y + z] + K)
                k = _first_violation(lhs, rhs0)
                if k >= 0:
                    return (0, y, z, int(b[k]), float(lhs[k]), float(rhs0[k]))
    return HOLDS


def run(kind, g, K, capacity=0):
    return check(g, K) if kind == 0 else check_ck(g, K, capacity)


def gy(pmf_t, v_next, x_min, x_max, step, v, h, pi):
    """G_t(y) for every y of the grid x_min, x_min + step, ..., x_max.  pmf_t: rows [demand, probability] of period t;
    v_next: V_{t+1} on the same grid, or None for the last period (no future term, Recursion.java:140)."""
    nx = int((x_max - x_min) / step) + 1
    y = x_min + np.arange(nx, dtype=np.float64) * step
    acc = np.zeros(nx)
    for d, p in np.asarray(pmf_t, dtype=np.float64):
        lev = y - d
        imm = ((0.0 + v * y) + h * np.maximum(lev, 0.0)) + pi * np.maximum(-lev, 0.0)
        acc = acc + p * imm
        if v_next is not None:
            nxt = np.where(lev > x_max, x_max, lev)  # CLSPforDraw.java:150-151: upper bound first, then lower
            nxt = np.where(nxt < x_min, x_min, nxt)
            idx = ((nxt - x_min) / step).astype(np.int64)
            acc = acc + p * np.asarray(v_next)[idx]
    return acc


def bits(x):
    """fp64 -> its 64 bits, so that comparisons see NaN payloads and the sign of zero."""
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Two result tuples equal by bits."""
    return tuple(int(v) for v in a[:4]) == tuple(int(v) for v in b[:4]) and np.array_equal(bits([a[4], a[5]]), bits([b[4], b[5]]))
