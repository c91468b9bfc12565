"""Host twin of the two-product rollout (sdpgpu_multi_policy_simulate): the lambdas of the three families and the simulators'
loop over a memo dict, in plain Python floats.  Written from the reference's lines and keeping their statement order:

    MultiItemCash.java:79-118            immediateValue / stateTransition of CashRecursionMulti      ("multicash")
    MultiItemCashXR.java:108-148         ... of CashRecursionMultiXR, state (x1, x2, R)              ("multixr")
    MultiProductLeadtime.java:162-223    ... of CashRecursionMultiLead, state with preQ1, preQ2      ("multilead")
    CashSimulationMulti.java:71-84, CashSimulationMultiXR.java:72-83    the loop over a path

It shares no code with the kernels or with stochastic_inventory_amd.  A state is the memo's key (period, i1, i2, q1, q2,
cash-or-R) and the memo a dict from it to the action pair -- what recursion.getAction(state) answers; where the memo holds
no such state the reference would re-enter its recursion, the twin ends the path there: its sum is NaN and it is not valid.
The keyword arguments are those of multilead_solve / multicash_solve / multixr_solve."""
import itertools
import math

import numpy as np


def jint(v):
    """Java's (int) of a double inside the int range: truncation toward zero."""
    return float(int(v))


def lambdas(kind, kw, depositeRate=0.0):
    """-> (immediateValue(state, action, demand), stateTransition(state, action, demand)) of the family."""
    T = kw["T"]
    price, variCost = [float(v) for v in kw["price"]], [float(v) for v in kw["vari_cost"]]
    minInventoryState, maxInventoryState = float(kw["min_inventory"]), float(kw["max_inventory"])
    minCashState, maxCashState = float(kw["min_cash"]), float(kw["max_cash"])

    if kind == "multicash":
        salPrice = [float(v) for v in kw["sal_price"]]

        def immediateValue(s, a, d):  # MultiItemCash.java:79-99
            period, i1, i2, _, _, cash = s
            action1, action2 = float(a[0]), float(a[1])
            demand1, demand2 = d
            endInventory1 = max(0.0, i1 + action1 - demand1)
            endInventory2 = max(0.0, i2 + action2 - demand2)
            revenue1 = price[0] * (i1 + action1 - endInventory1)
            revenue2 = price[1] * (i2 + action2 - endInventory2)
            revenue = revenue1 + revenue2
            orderingCost1 = variCost[0] * action1
            orderingCost2 = variCost[1] * action2
            orderingCosts = orderingCost1 + orderingCost2
            salValue = 0.0
            if period == T:
                salValue = salPrice[0] * endInventory1 + salPrice[1] * endInventory2
            return revenue - orderingCosts + salValue

        def stateTransition(s, a, d):  # MultiItemCash.java:103-118
            period, i1, i2, _, _, cash = s
            endInventory1 = i1 + float(a[0]) - d[0]
            endInventory1 = max(0.0, endInventory1)
            endInventory2 = i2 + float(a[1]) - d[1]
            endInventory2 = max(0.0, endInventory2)
            nextCash = cash + immediateValue(s, a, d)
            nextCash = maxCashState if nextCash > maxCashState else nextCash
            nextCash = minCashState if nextCash < minCashState else nextCash
            endInventory1 = maxInventoryState if endInventory1 > maxInventoryState else endInventory1
            endInventory2 = minInventoryState if endInventory2 < minInventoryState else endInventory2
            nextCash = jint(nextCash)
            endInventory1 = jint(endInventory1)
            endInventory2 = jint(endInventory2)
            return (period + 1, endInventory1, endInventory2, 0.0, 0.0, nextCash)

        return immediateValue, stateTransition

    if kind == "multixr":
        salPrice = [float(v) for v in kw["sal_price"]]

        def immediateValue(s, a, d):  # MultiItemCashXR.java:108-128
            period, x1, x2, _, _, R = s
            action1, action2 = float(a[0]), float(a[1])
            demand1, demand2 = d
            endInventory1 = max(0.0, action1 - demand1)
            endInventory2 = max(0.0, action2 - demand2)
            revenue1 = price[0] * (action1 - endInventory1)
            revenue2 = price[1] * (action2 - endInventory2)
            revenue = revenue1 + revenue2
            initialCash = R - variCost[0] * x1 - variCost[1] * x2
            orderingCostY1 = variCost[0] * action1
            orderingCostY2 = variCost[1] * action2
            orderingCostsY = orderingCostY1 + orderingCostY2
            salValue = 0.0
            if period == T:
                salValue = salPrice[0] * endInventory1 + salPrice[1] * endInventory2
            return revenue + (1 - depositeRate) * (R - orderingCostsY) + salValue - initialCash

        def stateTransition(s, a, d):  # MultiItemCashXR.java:132-148
            period, x1, x2, _, _, R = s
            endInventory1 = float(a[0]) - d[0]
            endInventory1 = max(0.0, endInventory1)
            endInventory2 = float(a[1]) - d[1]
            endInventory2 = max(0.0, endInventory2)
            initialCash = R - variCost[0] * x1 - variCost[1] * x2
            nextCash = initialCash + immediateValue(s, a, d)
            nextCash = maxCashState if nextCash > maxCashState else nextCash
            nextCash = minCashState if nextCash < minCashState else nextCash
            endInventory1 = maxInventoryState if endInventory1 > maxInventoryState else endInventory1
            endInventory2 = minInventoryState if endInventory2 < minInventoryState else endInventory2
            nextCash = jint(nextCash)
            endInventory1 = jint(endInventory1)
            endInventory2 = jint(endInventory2)
            nextR = jint(nextCash) + variCost[0] * endInventory1 + variCost[1] * endInventory2
            return (period + 1, endInventory1, endInventory2, 0.0, 0.0, nextR)

        return immediateValue, stateTransition

    if kind != "multilead":
        raise ValueError(kind)
    salValueUnit = [float(v) for v in kw["sal_value"]]
    overheadCost = [float(v) for v in kw["overhead"]]
    r0, r1, r2 = float(kw["r0"]), float(kw["r1"]), float(kw["r2"])
    limit, interestFreeAmount = float(kw["limit"]), float(kw["interest_free"])
    cash_int_cast = bool(kw.get("cash_int_cast", False))

    def immediateValue(s, a, d):  # MultiProductLeadtime.java:162-198
        period, i1, i2, preQ1, preQ2, iniCash = s
        action1, action2 = float(a[0]), float(a[1])
        demand1, demand2 = d
        endInventory1 = max(0.0, i1 + preQ1 - demand1)
        endInventory2 = max(0.0, i2 + preQ2 - demand2)
        revenue1 = price[0] * min(demand1, i1 + preQ1)
        revenue2 = price[1] * min(i2 + preQ2, demand2)
        revenue = revenue1 + revenue2
        orderingCost1 = variCost[0] * action1
        orderingCost2 = variCost[1] * action2
        orderingCosts = orderingCost1 + orderingCost2
        salValue = 0.0
        if period == T:
            salValue = salValueUnit[0] * endInventory1 + salValueUnit[1] * endInventory2
        t = period - 1
        cashBalanceBefore = iniCash - orderingCosts - overheadCost[t]
        if cashBalanceBefore >= 0:
            interest = -r0 * cashBalanceBefore
        elif cashBalanceBefore >= -interestFreeAmount:
            interest = 0.0
        elif cashBalanceBefore >= -limit:
            interest = r1 * (-cashBalanceBefore - interestFreeAmount)
        else:
            interest = r2 * (-cashBalanceBefore - limit) + r1 * (limit - interestFreeAmount)
        cashBalanceAfter = cashBalanceBefore - interest + revenue + salValue
        cashIncrement = cashBalanceAfter - iniCash
        return cashIncrement

    def stateTransition(s, a, d):  # MultiProductLeadtime.java:202-223
        period, i1, i2, preQ1, preQ2, iniCash = s
        nextPreQ1, nextPreQ2 = float(a[0]), float(a[1])
        endInventory1 = i1 + preQ1 - d[0]
        endInventory1 = max(0.0, endInventory1)
        endInventory2 = i2 + preQ2 - d[1]
        endInventory2 = max(0.0, endInventory2)
        nextCash = iniCash + immediateValue(s, a, d)
        nextCash = maxCashState if nextCash > maxCashState else nextCash
        nextCash = minCashState if nextCash < minCashState else nextCash
        endInventory1 = maxInventoryState if endInventory1 > maxInventoryState else endInventory1
        endInventory2 = minInventoryState if endInventory2 < minInventoryState else endInventory2
        if cash_int_cast:
            nextCash = jint(nextCash)  # :219, commented out in the file as it stands
        endInventory1 = jint(endInventory1)
        endInventory2 = jint(endInventory2)
        return (period + 1, endInventory1, endInventory2, nextPreQ1, nextPreQ2, nextCash)

    return immediateValue, stateTransition


def initial_state(kw):
    return (1, float(kw["ini_i1"]), float(kw["ini_i2"]), 0.0, 0.0, float(kw["ini_cash"]))


def memo_dict(rows):
    """{(period, i1, i2, q1, q2, cash): (a1, a2)} of memo rows {period, i1, i2, q1, q2, cash, value, a1, a2}."""
    return {(int(r[0]), float(r[1]), float(r[2]), float(r[3]), float(r[4]), float(r[5])): (int(r[7]), int(r[8])) for r in np.asarray(rows).tolist()}


def tiles(kind, kw):
    """Per period the joint tile as the recursion reads it: rows {d1, d2, p} in list order.  CashRecursionMulti and
    CashRecursionMultiLead cast the demands to int (`new Demands((int) ..., (int) ...)`), CashRecursionMultiXR keeps them;
    multilead: the product list i1 * n2 + i2 with p = p1 * p2, the same every period (GetPmfMulti.java:157-172)."""
    if kind == "multilead":
        (v1, v2), (p1, p2) = kw["values"], kw["probs"]
        tile = np.array([[jint(a), jint(b), float(pa) * float(pb)] for a, pa in zip(v1, p1) for b, pb in zip(v2, p2)])
        return [tile.copy() for _ in range(kw["T"])]
    out = []
    for t in kw["pmf"]:
        t = np.array(t, dtype=np.float64).reshape(-1, 3)
        if kind == "multicash":
            t[:, 0], t[:, 1] = [jint(v) for v in t[:, 0]], [jint(v) for v in t[:, 1]]
        out.append(t)
    return out


def support_paths(tl):
    """Every path through the tiles: (d1[n, T], d2[n, T], probability[n] as the product in period order)."""
    d1, d2, pr = [], [], []
    for combo in itertools.product(*[range(len(t)) for t in tl]):
        d1.append([tl[t][j, 0] for t, j in enumerate(combo)])
        d2.append([tl[t][j, 1] for t, j in enumerate(combo)])
        p = 1.0
        for t, j in enumerate(combo):
            p = p * tl[t][j, 2]
        pr.append(p)
    return np.array(d1), np.array(d2), np.array(pr)


def rollout(kind, kw, memo, d1, d2, disc, depositeRate=0.0):
    """(sums[n], valid[n]) of the memo's policy along the demand pairs d1 / d2 [n, T]; disc[t] = Math.pow(discountFactor, t)."""
    immediateValue, stateTransition = lambdas(kind, kw, depositeRate)
    T = kw["T"]
    n = len(d1)
    sums, valid = np.empty(n), np.zeros(n, dtype=bool)
    for i in range(n):
        total = 0.0
        state = initial_state(kw)
        ok = True
        for t in range(T):
            actions = memo.get(state)
            if actions is None:
                ok = False
                break
            randomDemands = (float(d1[i][t]), float(d2[i][t]))
            total += float(disc[t]) * immediateValue(state, actions, randomDemands)
            state = stateTransition(state, actions, randomDemands)
        sums[i] = total if ok else math.nan
        valid[i] = ok
    return sums, valid
