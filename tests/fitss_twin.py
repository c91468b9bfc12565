"""Independent twin of the (s, S) level rules ("Batched (s, S) level rules"): plain Python / numpy written from the
definition -- levelIndex, the three fits with the closed-form minSquare, the three rule rollouts -- with none of the
library's code.  Rows are [period, x, Q]; every function also records which BRANCH of the definition it took (`trace`), so a
test can assert that its cases reach all of them."""
import numpy as np


def level_index(rows, max_q):
    """Walk j ascending with mark = false: Q_j < maxQ and not mark -> mark; else Q_j == maxQ and mark and j != n - 1 ->
    clear, append j; then Q_j == 0 -> append j, stop; then j == n - 1 -> append j."""
    out, mark, n = [], False, len(rows)
    for j in range(n):
        q = rows[j][2]
        if q < max_q and not mark:
            mark = True
        elif q == max_q and mark and j != n - 1:
            mark = False
            out.append(j)
        if q == 0:
            out.append(j)
            break
        if j == n - 1:
            out.append(j)
    return out


def min_square(lb, up_index, rows, max_q, trace=None):
    low = 0
    for i in range(len(rows)):
        if rows[i][2] != max_q:
            low = i
            break
    terms = [rows[low][1] + rows[low][2]]
    for i in range(low + 1, up_index + 1):
        if rows[i][2] != max_q:
            terms.append(rows[i][1] + rows[i][2])
    total = 0.0
    for v in terms:  # ascending i, fp64
        total += v
    m = total / len(terms)
    if trace is not None:
        trace.add("minsq_below_lb" if m < lb else ("minsq_above_ub" if m > 10000.0 else "minsq_inside"))
        if len(terms) > 1:
            trace.add("minsq_many_terms")
    return min(max(m, lb), 10000.0)


def _period_rows(table, t):
    return [r for r in table if r[0] == t + 1]


def fit(levels, T, max_q, table, trace=None):
    """getSinglesS / getTwosS / getThreesS (levels 1 / 2 / 3): [T][2 * levels]."""
    table = [[float(v) for v in r] for r in np.asarray(table, dtype=np.float64)]
    tr = trace if trace is not None else set()
    out = np.zeros((T, 2 * levels))
    x0, q0 = table[0][1], table[0][2]
    for b in range(levels):
        out[0][2 * b] = x0 + 1
        out[0][2 * b + 1] = x0 + q0
    for t in range(1, T):
        rows = _period_rows(table, t)
        n = len(rows)
        idx = level_index(rows, max_q)
        o = out[t]
        x = lambda k: rows[k][1]
        S = lambda k: rows[k - 1][1] + rows[k - 1][2]
        at_limit = lambda k: k == n - 1 and rows[k][2] == max_q
        if len(idx) == 1 and idx[0] != 0:
            tr.add(f"L{levels}:one")
            o[0], o[1] = x(idx[0]), S(idx[0])
            if at_limit(idx[0]):
                tr.add(f"L{levels}:one_at_limit")
                o[0], o[1] = x(idx[0]) + 1, x(idx[0]) + rows[idx[0]][2]
            for b in range(1, levels):
                o[2 * b], o[2 * b + 1] = o[0], o[1]
        elif len(idx) == 1 and idx[0] == 0:
            tr.add(f"L{levels}:zero_row")
            o[:] = x(0)
        elif len(idx) == 0:  # (dead: the list is never empty)
            for b in range(levels):
                o[2 * b], o[2 * b + 1] = x(n - 1), max_q * 10
        elif levels == 1:
            tr.add("L1:minsq")
            k = idx[-1]
            o[0] = x(k)
            o[1] = min_square(o[0], k, rows, max_q, tr)
        elif len(idx) == 2:
            tr.add(f"L{levels}:two")
            o[0], o[1], o[2], o[3] = x(idx[0]), S(idx[0]), x(idx[1]), S(idx[1])
            if at_limit(idx[1]):
                tr.add(f"L{levels}:two_at_limit")
                o[2], o[3] = x(idx[1]) + 1, x(idx[1]) + rows[idx[1]][2]
            if levels == 3:
                o[4], o[5] = o[2], o[3]
        elif levels == 2:
            tr.add("L2:minsq")
            k2, k1 = idx[-1], idx[-2]
            o[2], o[3] = x(k2), S(k2)
            o[0] = x(k1)
            o[1] = min_square(o[0], k1, rows, max_q, tr)
        elif len(idx) == 3:
            tr.add("L3:three")
            o[0], o[1], o[2], o[3], o[4], o[5] = x(idx[0]), S(idx[0]), x(idx[1]), S(idx[1]), x(idx[2]), S(idx[2])
            if at_limit(idx[2]):
                tr.add("L3:three_at_limit")
                o[4], o[5] = x(idx[2]) + 1, x(idx[2]) + rows[idx[2]][2]
        else:
            tr.add("L3:minsq")
            k3, k2, k1 = idx[-1], idx[-2], idx[-3]
            o[4], o[5] = x(k3), S(k3)
            o[2], o[3] = x(k2), S(k2)
            o[0] = x(k1)
            o[1] = min_square(o[0], k1, rows, max_q, tr)
    return out


# every live branch of the three methods (the `length == 0` branch is dead code)
LIVE_BRANCHES = {"L1:one", "L1:one_at_limit", "L1:zero_row", "L1:minsq",
                 "L2:one", "L2:one_at_limit", "L2:zero_row", "L2:two", "L2:two_at_limit", "L2:minsq",
                 "L3:one", "L3:one_at_limit", "L3:zero_row", "L3:two", "L3:two_at_limit", "L3:three", "L3:three_at_limit", "L3:minsq",
                 "minsq_below_lb", "minsq_inside", "minsq_many_terms"}


def order_quantity(levels, t, x, ini, o, max_q):
    """The order of period index t in state x under the rule row o (SimulateFitsS's band tests as written)."""
    if t == 0:
        return o[1] - ini  # not capped
    if levels == 1:
        return 0.0 if x >= o[0] else min(max_q, o[1] - x)
    if x < o[0]:
        return min(max_q, o[1] - x)
    if o[0] <= x and x < o[2]:
        return min(max_q, o[3] - x)
    if levels == 3 and o[2] <= x and x < o[4]:
        return min(max_q, o[5] - x)
    return 0.0


def rollout(levels, ss, demands, ini, max_q, K, v, h, pi, lo, hi):
    """Path sums of one instance: ss [T][2 * levels], demands [n_paths][T]; the F1 immediateValue / stateTransition
    (ThreeLevelFitsSTest.java:98-115) in fp64, one operation at a time."""
    ss = np.asarray(ss, dtype=np.float64)
    out = np.empty(len(demands))
    for p, row in enumerate(np.asarray(demands, dtype=np.float64)):
        total, x = 0.0, float(ini)
        for t, d in enumerate(row):
            d = float(d)
            a = float(order_quantity(levels, t, x, float(ini), [float(z) for z in ss[t]], float(max_q)))
            fixed = K if a > 0 else 0.0
            var = v * a
            level = (x + a) - d
            total += ((fixed + var) + h * max(level, 0.0)) + pi * max(-level, 0.0)
            nxt = hi if level > hi else level
            x = lo if nxt < lo else nxt
        out[p] = total
    return out
