"""Plain Python-float restatements for the G(y) rows of the STAFF family (csrc/sdp_staff_structure.hpp; DESIGN 4, "Workforce
structure rows"): the definition, the loop of the reference's drawing recursion, and the condition under which the two agree.

    gy_level / gy_row   the definition: one serial sum per level against a given V_{t+1}
    second_recursion    StaffRecursion.java:127-172 over the lambdas of WorkforcePlanning.java:171-195, with that loop applied
                        at EVERY period (an action whose level x + a is not a row of the table is skipped, :148-149; no clamp,
                        :171-174).  In the Java text the inner call at :161 has one argument and so resolves to the method of
                        :81-118; the loop restated here is the one the condition below refers to.
    condition           no state of periods 2 .. T that the sums of second_recursion reach has x + policy(x) > n_rows - 1
"""
import sys

MAX_VALUE = sys.float_info.max


def row_of(case, t, y):
    """p_row of level y in period t (1-based): a list of Python floats."""
    n = y + 1 if case.row_len is None else int(case.row_len[y])
    return [float(p) for p in case.table[t - 1, y, :n]]


def gy_level(case, t, y, v_next, next_x_lo):
    """G_t(y); v_next (None: period T) is indexed by nn - next_x_lo."""
    f = case.functor
    v, salary, pen_u, ms = float(f.unitVariCost), float(f.salary), float(f.unitPenalty), int(f.minStaffNum[t - 1])
    g = 0.0
    for j, p in enumerate(row_of(case, t, y)):
        n = y - j
        pen = 0.0 if n > ms else pen_u * float(ms - n)
        g += p * (((0.0 + v * float(y)) + salary * float(n)) + pen)
        if v_next is not None:
            nn = n
            if f.clampStaff:
                nn = f.maxX if nn > f.maxX else nn
                nn = f.minX if nn < f.minX else nn
            g += p * float(v_next[nn - next_x_lo])
    return g


def gy_row(case, t, v_next, next_x_lo, y_lo=0, y_hi=None):
    rows = case.table.shape[1]
    y_hi = rows - 1 if y_hi is None else y_hi
    return [gy_level(case, t, y, v_next, next_x_lo) for y in range(y_lo, y_hi + 1)]


def second_recursion(case):
    """-> (G_1(y) for y = 0 .. n_rows - 1, the set of (period, x) the sums reached in periods 2 .. T)."""
    f = case.functor
    T, rows = case.T, case.table.shape[1]
    K, v, salary, pen_u = float(f.fixCost), float(f.unitVariCost), float(f.salary), float(f.unitPenalty)
    memo = {}

    def value(period, x):
        key = (period, x)
        if key in memo:
            return memo[key]
        ms = int(f.minStaffNum[period - 1])
        best = MAX_VALUE
        # (in period 1 the lambdas ignore the action: every action gives the same sum, one is formed)
        for a in ([0] if period == 1 else range(f.maxHireNum + 1)):
            y = x if period == 1 else x + a
            if y >= rows:
                continue
            q = 0.0
            for j, p in enumerate(row_of(case, period, y)):
                if period == 1:
                    fix, vari, n = 0.0, v * float(x), x - j
                else:
                    fix, vari, n = (K if a > 0 else 0.0), v * float(a), x + a - j
                pen = 0.0 if n > ms else pen_u * float(ms - n)
                q += p * (fix + vari + salary * float(n) + pen)
                if period < T:
                    q += p * value(period + 1, n)
            if q < best:
                best = q
        memo[key] = best
        return best

    g1 = [value(1, y) for y in range(rows)]
    return g1, {k for k in memo if k[0] >= 2}


def reached(case):
    """The (period, x) of periods 2 .. T the sums of second_recursion reach, without evaluating them."""
    f = case.functor
    rows = case.table.shape[1]
    lens = [y + 1 if case.row_len is None else int(case.row_len[y]) for y in range(rows)]
    out = set()
    cur = {y - j for y in range(rows) for j in range(lens[y])}
    for period in range(2, case.T + 1):
        out |= {(period, x) for x in cur}
        nxt = set()
        for x in cur:
            for a in range(f.maxHireNum + 1):
                if x + a >= rows:
                    break
                nxt |= {x + a - j for j in range(lens[x + a])}
        cur = nxt
    return out


def condition(case, policy, x_lo):
    """True iff no reached state of periods 2 .. T has x + policy(x) > n_rows - 1.  policy[t - 1][x - x_lo[t - 1]]: the
    solved hire count; a reached state outside the solved grid breaks the condition as well."""
    rows = case.table.shape[1]
    for period, x in reached(case):
        i = x - int(x_lo[period - 1])
        if i < 0 or i >= len(policy[period - 1]):
            return False
        if x + int(policy[period - 1][i]) > rows - 1:
            return False
    return True
