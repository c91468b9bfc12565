"""An independent restatement, from the Java, of what the cash structure entry points compute: the three G kinds of the drivers'
second and third CashRecursion (SingleCrossTesting.java:110-165, CashConstraintDraw.java:193-283) summed as
CashRecursion.java:110-122 sums, and every table method of CashRecursion.java:227-404.  Plain Python floats (IEEE doubles, no
FMA), loops as the reference writes them; numpy only for the arrays that go in and out.

The lambdas of the drawn period are the handle's own (formula 1 of CashConstraintTesting.java:117-148: overhead per period,
salvage at T, the penalty statement, max(0, level), both clamps, Math.round) with `action` struck out as the drivers strike it:
fixedCost = 0, variableCost = 0 (G) or variCost * iniInventory (GA, GB), and for GB `nextCash - fixOrderCost` before the
clamps."""
import math

import numpy as np

INT_MAX, INT_MIN = 2147483647, -2147483648


def java_int(x):
    """(int) of a double: NaN -> 0, saturating, truncation toward zero."""
    if x != x:
        return 0
    if x >= 2147483647.0:
        return INT_MAX
    if x <= -2147483648.0:
        return INT_MIN
    return int(x)


def wrap(n):
    """int arithmetic wraps."""
    return (n + 2**31) % 2**32 - 2**31


def java_div(a, b):
    """a / b of two doubles (no exception on zero)."""
    if b == 0:
        if a == 0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def canon(x):
    """A NaN that is stored is the one NaN of Double.doubleToLongBits (Java defines no other)."""
    return math.nan if x != x else x


def java_round(x):
    """Math.round as an integer-valued double: floor(x + 1/2) with ties up, computed without the addition's rounding."""
    f = math.floor(x)
    return f + 1.0 if x - f >= 0.5 else float(f)


# ---- the G kinds -------------------------------------------------------------------------------------------------------
def g_entry(kind, f, T, period, pmf_t, overhead, v_next, nc, x_lo_next, k_lo, R, y):
    """Entry (R, y) of period `period`: f a CashFunctor-shaped object (attributes only), pmf_t rows [demand, prob], v_next the
    flat V_{period+1} laid out [ix * nc + ic] (None at period T).  kind 0 = G (stored minus variCost * y), 1 = GA, 2 = GB."""
    variCost, fixOrderCost = float(f.variCost), float(f.fixOrderCost)
    thisQValue = 0.0
    for row in pmf_t:
        randomDemand, dProb = float(row[0]), float(row[1])
        revenue = f.price * min(y, randomDemand)
        fixedCost = 0.0
        variableCost = 0.0 if kind == 0 else variCost * y
        inventoryLevel = y - randomDemand
        holdCosts = f.holdingCost * max(inventoryLevel, 0.0)
        cashIncrement = revenue - fixedCost - variableCost - holdCosts - overhead
        salValue = f.salvageValue * max(inventoryLevel, 0.0) if period == T else 0.0
        cashIncrement += salValue
        endCash = R + cashIncrement
        if endCash < 0:
            cashIncrement += f.penaltyCost * endCash
        thisQValue += dProb * cashIncrement
        if period < T:
            nextInventory = max(0.0, inventoryLevel)
            nextCash = R + cashIncrement
            if kind == 2:
                nextCash = nextCash - fixOrderCost
            nextCash = f.maxCashState if nextCash > f.maxCashState else nextCash
            nextCash = f.minCashState if nextCash < f.minCashState else nextCash
            nextInventory = f.maxInventoryState if nextInventory > f.maxInventoryState else nextInventory
            nextInventory = f.minInventoryState if nextInventory < f.minInventoryState else nextInventory
            nextCash = java_round(nextCash * 1.0)
            idx = int(nextInventory - x_lo_next) * nc + (int(nextCash) - k_lo)
            thisQValue += dProb * f.discountFactor * float(v_next[idx])
    return thisQValue - variCost * y if kind == 0 else thisQValue


def g_table(kind, f, T, period, pmf_t, overhead, v_next, nc, x_lo_next, k_lo, x_lo, n_x, cash_lo, n_r):
    out = np.empty((n_r, n_x), dtype=np.float64)
    for i in range(n_r):
        for j in range(n_x):
            out[i, j] = g_entry(kind, f, T, period, pmf_t, overhead, v_next, nc, x_lo_next, k_lo, float(cash_lo) + i, float(x_lo) + j)
    return out


# ---- CashRecursion.java:227-404 ----------------------------------------------------------------------------------------
class IndexOutOfBounds(Exception):
    """Where Java throws ArrayIndexOutOfBoundsException; carries (i, j, k)."""


def getMinusGAGB(resultGA, resultGB, minCash, fixCost, variCost):
    RLength, xLength = len(resultGA), len(resultGA[0])
    values = np.zeros((RLength, xLength))
    for i in range(RLength):
        cash = minCash + float(i)
        Qbound = max(0, java_int(java_div(cash - fixCost, variCost)))
        for j in range(xLength):
            optimalGB = float(resultGB[i][j])
            k = j
            while k < min(wrap(wrap(j + Qbound) + 1), xLength):
                if float(resultGB[i][k]) > optimalGB:
                    optimalGB = float(resultGB[i][k])
                k += 1
            values[i][j] = canon(optimalGB - float(resultGA[i][j]) - fixCost)
    return values


def getMinusFG(resultG, resultF, minCash, fixCost, variCost):
    RLength, xLength = len(resultG), len(resultG[0])
    values = np.zeros((RLength, xLength))
    for i in range(RLength):
        for j in range(xLength):
            values[i][j] = canon(float(resultF[i][j]) - float(resultG[i][j]) - variCost * float(j))
    return values


def getH(resultG, minCash, fixCost, variCost, with_index=False):
    RLength, xLength = len(resultG), len(resultG[0])
    values = np.zeros((RLength, xLength))
    opt = np.zeros((RLength, xLength), dtype=np.int32)
    for i in range(RLength):
        cash = minCash + float(i)
        for j in range(xLength):
            ybound = min(xLength - 1, wrap(j + max(0, java_int(java_div(cash - fixCost, variCost)))))
            optimalIncre = -fixCost
            optyIndex = j
            for k in range(j + 1, ybound + 1):
                cashIndex = java_int(cash - fixCost - variCost * float(k - j))
                if cashIndex < 0:
                    continue
                if cashIndex >= RLength:
                    raise IndexOutOfBounds((i, j, k))
                if float(resultG[cashIndex][k]) - float(resultG[i][j]) - fixCost > optimalIncre:
                    optimalIncre = float(resultG[cashIndex][k]) - float(resultG[i][j]) - fixCost
                    optyIndex = k
            values[i][j] = canon(optimalIncre)
            opt[i][j] = optyIndex
    return (values, opt) if with_index else values


def getH3Column(resultG, minCash, fixCost, variCost):
    RLength, xLength = len(resultG), len(resultG[0])
    H = getH(resultG, minCash, fixCost, variCost)
    values = np.zeros((RLength * xLength, 3))
    index = 0
    for i in range(RLength):
        for j in range(xLength):
            values[index][0] = resultG[i][0]
            values[index][1] = resultG[0][j]
            values[index][2] = H[i][j]
            index += 1
    return values


HOLDS = (1, -1, -1, -1, -1, 0.0)


def checkSingleCrossing(resultH):
    """-> the verdict tuple (holds, i, j, i1, j1, value): `return false` with the loop variables at that moment."""
    RLength, xLength = len(resultH), len(resultH[0])
    lastColumnEnd = 0
    for i in range(RLength):
        for j in range(xLength - 1, -1, -1):
            if float(resultH[i][j]) > -0.1:
                for i1 in range(i, RLength):
                    for j1 in range(lastColumnEnd, j + 1):
                        if float(resultH[i1][j1]) > -0.1:
                            continue
                        return (0, i, j, i1, j1, canon(float(resultH[i1][j1])))
                lastColumnEnd = j + 1
                break
    return HOLDS


def checkNonIncreasing(arr):
    RLength, xLength = len(arr), len(arr[0])
    for i in range(RLength):
        for j in range(xLength - 1):
            if float(arr[i][j + 1]) - float(arr[i][j]) < 0.1:
                continue
            return (0, i, j, i, j + 1, canon(float(arr[i][j + 1]) - float(arr[i][j])))
    return HOLDS


def checkNonDecreasing(arr):
    RLength, xLength = len(arr), len(arr[0])
    for j in range(xLength):
        for i in range(RLength - 1):
            if float(arr[i + 1][j]) - float(arr[i][j]) > -0.1:
                continue
            return (0, i, j, i + 1, j, canon(float(arr[i + 1][j]) - float(arr[i][j])))
    return HOLDS


def same_verdict(a, b):
    """Indices equal and the doubles equal by bits (NaN == NaN here)."""
    return tuple(a[:5]) == tuple(b[:5]) and np.float64(a[5]).tobytes() == np.float64(b[5]).tobytes()
