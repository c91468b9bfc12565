"""Forward simulation of the computed policy: the step immediately AFTER the hot path
 and the reference's only validation idiom.

Mirrors `sdp.inventory.Simulation` (src/sdp/inventory/Simulation.java:33-107) and the SDP part of
`sdp.cash.CashSimulation` (src/sdp/cash/CashSimulation.java:85-118): sample demand paths, round
them to integers (`Math.round`, Simulation.java:64), and per path walk
`getAction(state) -> immediateValue -> stateTransition` through the horizon.  Here the walk is a
batched table-lookup rollout on the device (`sdpgpu_simulate`, one path per lane) over the policy
tables the sweep left in HBM; only the sampling and the final mean stay on the host.

Differences, both deliberate:
* the reference's latin-hypercube sampler draws its jitter from `Math.random()`
  (Sampling.java:94) and is therefore not reproducible; this one takes a seed.
* `Arrays.stream(simuValues).sum()` is a compensated sum in Java; the mean here uses math.fsum.
  Per-path sums are accumulated on the device in period order exactly as the reference's
  `sum += ...`, so they are bit-identical to the CPU oracle's.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np

from . import _abi
from .functors import java_round


class Sampling:
    """sdp.sampling.Sampling: latin hypercube / plain random sampling through inverseF."""

    def __init__(self, seed: int = 12345):
        self.rng = np.random.default_rng(seed)

    def generateLHSamples(self, distributions: Sequence, sampleNum: int) -> np.ndarray:
        """Sampling.java:86-103: one stratum [j/n, (j+1)/n) per sample and period, then a shuffle of the rows."""
        T = len(distributions)
        samples = np.empty((sampleNum, T), dtype=np.float64)
        for i in range(T):
            u = (np.arange(sampleNum) + self.rng.random(sampleNum)) / float(sampleNum)
            samples[:, i] = [distributions[i].inverseF(float(p)) for p in u]
        # Sampling.shuffle (Sampling.java:326-335): every period column is shuffled on its own, each
        # position swapped with a uniformly drawn one
        for i in range(T):
            marks = self.rng.integers(0, sampleNum, size=sampleNum)
            col = samples[:, i]
            for j in range(sampleNum):
                m = marks[j]
                col[j], col[m] = col[m], col[j]
        return samples

    def generateRanSamples(self, distributions: Sequence, sampleNum: int) -> np.ndarray:
        """Sampling.java:49-60."""
        T = len(distributions)
        samples = np.empty((sampleNum, T), dtype=np.float64)
        for i in range(T):
            samples[:, i] = [distributions[i].inverseF(float(p)) for p in self.rng.random(sampleNum)]
        return samples


def round_demands(samples: np.ndarray) -> np.ndarray:
    """`Math.round(samples[i][t])` element-wise (Simulation.java:64)."""
    return np.array([[float(java_round(float(v))) for v in row] for row in samples], dtype=np.float64)


def _check_sampler(sampler: str) -> str:
    if sampler not in ("host", "device"):
        raise ValueError(f"sampler {sampler!r}: 'host' or 'device'")
    return sampler


def _hand_samplers(recursion, distributions):
    """sampler="device": every distribution to the engine's sampler of its period index; None keeps the pmf tile."""
    T = recursion.T
    if distributions is not None and len(distributions) != T:
        raise ValueError(f"{len(distributions)} distributions, the horizon is {T}")
    for t in range(T):
        recursion.engine.set_sampler(t, None if distributions is None else distributions[t])


def _is_custom(recursion) -> bool:
    """The recursion's functor is a CustomFunctor: its handle takes the user-functor rollouts."""
    from .functors import CustomFunctor
    return isinstance(recursion.functor, CustomFunctor)


def merge_moments(na: int, mean_a: float, m2_a: float, nb: int, mean_b: float, m2_b: float):
    """(n, mean, M2) of the union of two samples from theirs (Chan, Golub, LeVeque: "Updating formulae and a pairwise algorithm
    for computing sample variances", 1979): M2 = sum of squared deviations from the mean."""
    if na == 0:
        return nb, mean_b, m2_b
    if nb == 0:
        return na, mean_a, m2_a
    n = na + nb
    delta = mean_b - mean_a
    return n, mean_a + delta * (nb / n), m2_a + m2_b + delta * delta * (na * nb / n)


class Simulation:
    """sdp.inventory.Simulation(distributions, sampleNum, recursion) -- also serves the cash classes
    (CashSimulation adds `Math.pow(discountFactor, t)` weights and `+ iniCash`, :108,114)."""

    def __init__(self, distributions: Sequence, sampleNum: int, recursion, discountFactor: float = 1.0,
                 seed: int = 12345, sampler: str = "host"):
        """sampler="host" (the default): sample through inverseF in Python, upload, roll on the device.  sampler="device":
        sample, roll and reduce on the device in one call (SdpEngine.simulate_sampled; seeded and reproducible) --
        each distribution goes to the engine's sampler of its period; a None entry, or distributions=None, draws that
        period from the recursion's own pmf tile."""
        self.sampler = _check_sampler(sampler)
        self.distributions = None if distributions is None else list(distributions)
        self.sampleNum = int(sampleNum)
        self.recursion = recursion
        self.discountFactor = float(discountFactor)
        self.stateTransition = recursion.getStateTransitionFunction()
        self.immediateValue = recursion.getImmediateValueFunction()
        self.seed = int(seed)
        self.sampling = Sampling(seed)
        self.last_values = None
        self.last_result = None
        if self.sampler == "device":
            _hand_samplers(recursion, self.distributions)

    def setSampleNum(self, n: int):
        self.sampleNum = int(n)

    def _rollout(self, iniState, demands: np.ndarray) -> np.ndarray:
        rec = self.recursion
        rec.getExpectedValue(iniState)  # solves on first use, as Simulation.java:62 does
        T = rec.T
        disc = np.array([math.pow(self.discountFactor, t) for t in range(T)], dtype=np.float64)
        x, cash, preq = rec.functor.tuple_of(iniState)
        # (a recursion over user lambdas rolls through their compiled text: SdpEngine.custom_simulate)
        roll = rec.engine.custom_simulate if _is_custom(rec) else rec.engine.simulate
        sums, valid = roll(demands, disc, x, cash, preq)
        if not valid.all():
            raise RuntimeError(f"{int((~valid).sum())} sample paths left the state grid (demand outside the PMF support "
                               "of an unclamped family); the reference would re-enter the recursion there")
        return sums

    def _discount(self):
        return np.array([math.pow(self.discountFactor, t) for t in range(self.recursion.T)], dtype=np.float64)

    def _device_call(self, iniState, n: int, mode: str, first_path: int = 0):
        """One sample-and-roll call on the device; raises as _rollout does when paths left the grid."""
        rec = self.recursion
        rec.getExpectedValue(iniState)  # solves on first use, as Simulation.java:62 does
        x, cash, preq = rec.functor.tuple_of(iniState)
        roll = rec.engine.custom_simulate_sampled if _is_custom(rec) else rec.engine.simulate_sampled
        res, sums, _ = roll(n, self.seed, x, cash, preq, mode=mode, first_path=first_path, discount=self._discount(), want_sums=True)
        if res.n_valid != res.n_paths:
            raise RuntimeError(f"{res.n_paths - res.n_valid} sample paths left the state grid (demand outside the PMF support "
                               "of an unclamped family); the reference would re-enter the recursion there")
        self.last_result = res
        return res, sums

    def simulateSDPGivenSamplNum(self, iniState) -> float:
        """Simulation.java:53-74: mean of the simulated totals over `sampleNum` LHS paths."""
        if self.sampler == "device":
            res, sums = self._device_call(iniState, self.sampleNum, "lhs")
            self.last_values = sums
            mean = res.mean
            if hasattr(iniState, "getIniCash"):  # CashSimulation.java:114
                mean += iniState.getIniCash()
            return mean
        samples = self.sampling.generateLHSamples(self.distributions, self.sampleNum)
        sums = self._rollout(iniState, round_demands(samples))
        self.last_values = sums
        mean = math.fsum(sums.tolist()) / len(sums)
        if hasattr(iniState, "getIniCash"):  # CashSimulation.java:114
            mean += iniState.getIniCash()
        return mean

    def simulateSDPwithErrorConfidence(self, iniState, error: float, confidence: float, batch: int = 1000,
                                       maxRuns: int = 1000000):
        """Simulation.java:76-107: keep sampling until the normal confidence radius is below error * mean
        (at least 1000 runs).  Paths are rolled in batches on the device."""
        from scipy import stats as _st
        z = float(_st.norm.ppf(0.5 + confidence / 2.0))
        if self.sampler == "device":
            # rounds of plain-random paths continuing ONE stream (first_path = paths drawn so far); the rounds' (n, mean, m2)
            # merged by the pairwise update of Chan, Golub and LeVeque
            n, mean, m2 = 0, 0.0, 0.0
            chunks = []
            center, radius = 0.0, math.inf
            while n < 1000 or (radius >= center * error and n < maxRuns):
                res, sums = self._device_call(iniState, batch, "random", first_path=n)
                n, mean, m2 = merge_moments(n, mean, m2, res.n_paths, res.mean, res.m2)
                chunks.append(sums)
                center = mean
                radius = z * math.sqrt(m2 / (n - 1)) / math.sqrt(n) if n > 1 else math.inf
            self.last_values = np.concatenate(chunks)
            return [center, radius]
        vals = np.empty(0)
        center, radius = 0.0, math.inf
        while len(vals) < 1000 or (radius >= center * error and len(vals) < maxRuns):
            samples = self.sampling.generateRanSamples(self.distributions, batch)
            vals = np.concatenate([vals, self._rollout(iniState, round_demands(samples))])
            center = float(vals.mean())
            radius = z * float(vals.std(ddof=1)) / math.sqrt(len(vals))
        self.last_values = vals
        return [center, radius]

    def simulateOnHost(self, iniState, demands: np.ndarray) -> np.ndarray:
        """The reference's loop verbatim (Simulation.java:59-69), one path at a time through the host
        lambdas and getAction -- for cross-checking the device rollout on a few paths."""
        out = np.empty(len(demands))
        for i, row in enumerate(demands):
            total, state = 0.0, iniState
            for t, d in enumerate(row):
                self.recursion.getExpectedValue(state)
                optQ = self.recursion.getAction(state)
                total += math.pow(self.discountFactor, t) * self.immediateValue(state, optQ, float(d))
                state = self.stateTransition(state, optQ, float(d))
            out[i] = total
        return out


CASH_RULE_M = 10000.0  # `int M = 10000` (CashSimulation.java:1004): C2 of an inventory level without an entry


def cash_rule_rows(form: int, optsCS) -> np.ndarray:
    """The reference's optsCS as the (T, 4) rows (s, c1, c2, S) of sdpgpu_cash_rule_simulate: form 0 has the four columns
    already (CashSimulation.java:1011-1028); the three columns [s, C, S] of forms 1 and 2 (:1064-1079, :1113-1120) become
    (s, C, 0, S).  Four columns are taken as they are."""
    rows = np.asarray(optsCS, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] not in (3, 4) or (form == _abi.RULE_SC12S and rows.shape[1] != 4):
        raise ValueError(f"optsCS of shape {rows.shape}: [T, 4] for (s, C1, C2, S), [T, 3] for (s, C, S)")
    if rows.shape[1] == 3:
        rows = np.stack([rows[:, 0], rows[:, 1], np.zeros(len(rows)), rows[:, 2]], axis=1)
    return np.ascontiguousarray(rows)


def cash_rule_table_index(x: float, min_inventory: float, step: float, nx: int):
    """Index of the table entry whose key IS the double x (key of entry ix: min_inventory + ix * step), or None -- the lookup
    of DESIGN 4, "Cash rule rollout"."""
    fi = float(np.rint((x - min_inventory) * (1.0 / step)))
    if not (0.0 <= fi < nx):
        return None
    i = int(fi)
    return i if min_inventory + i * step == x else None


def pack_cash_rule_table(cache, T: int, min_inventory: float, step: float, nx: int) -> np.ndarray:
    """A cacheC1Values / cacheC2Values map {(period, x): value} (period 1-based, as State.getPeriod(); a State key works too)
    as the dense (T, NX) table: NaN where no key is present; a key off the grid or outside the horizon can never be hit and is
    dropped."""
    tab = np.full((T, nx), np.nan)
    for key, v in (cache or {}).items():
        period, x = (key.getPeriod(), key.getIniInventory()) if hasattr(key, "getPeriod") else key
        ix = cash_rule_table_index(float(x), min_inventory, step, nx)
        if ix is not None and 1 <= int(period) <= T and int(period) == period:
            tab[int(period) - 1, ix] = float(v)
    return tab


def cash_rule_order(form: int, t: int, row, c1_row, c2_row, x: float, cash: float, minCashRequired: float, maxQ: float,
                    fixOrderCost: float, variCost: float, grid) -> float:
    """optQ of one period (CashSimulation.java:1009-1031, :1062-1082, :1111-1123).  row = (s, c1, c2, S); c1_row / c2_row:
    the period's dense table rows or None; grid = (min_inventory, step, nx)."""
    from .functors import _d2i
    s, c1, c2, S = (float(v) for v in row)
    m = max(0.0, (cash - minCashRequired - fixOrderCost) / variCost)
    if t == 0:
        q = S - x if x < s else 0.0
        return min(q, m) if form == _abi.RULE_SC1S else q
    if form == _abi.RULE_SC12S:
        m = float(_d2i(m))
    m = min(m, maxQ)
    if not x < s:
        return 0.0

    def lookup(tab_row, absent):
        ix = None if tab_row is None else cash_rule_table_index(x, *grid)
        return absent if ix is None or tab_row[ix] != tab_row[ix] else float(tab_row[ix])

    if form != _abi.RULE_SMEANCS:
        c1 = lookup(c1_row, 0.0)
    if form == _abi.RULE_SC12S:
        c2 = lookup(c2_row, CASH_RULE_M)
    orders = cash > c1 and (form != _abi.RULE_SC12S or cash < c2)
    return min(m, S - x) if orders else 0.0


def overdraft_rule_rows(form: int, opts, T: int) -> np.ndarray:
    """The reference's arrays as the (T, 4) rows (s, C, S, S2) of sdpgpu_custom_rule_simulate: optsS [T, 2] = (s, S) of
    simulatesSOD, optsCS [T, 3] = (s, C, S) of simulatesCSDraft, optsCS [T, 4] = (s, C, S1, S2) of simulatesSOD2.  Four columns
    are taken as they are."""
    rows = np.asarray(opts, dtype=np.float64)
    want = {_abi.ORULE_SS: 2, _abi.ORULE_SCS: 3, _abi.ORULE_SCS1S2: 4}.get(form)
    if want is None:
        raise ValueError(f"form {form}: ORULE_SS 0, ORULE_SCS 1, ORULE_SCS1S2 2")
    if rows.ndim != 2 or rows.shape[0] != T or rows.shape[1] not in (want, 4):
        raise ValueError(f"rule of shape {rows.shape} for form {form}: [{T}, {want}] (or the four columns s, C, S, S2)")
    z = np.zeros(T)
    if rows.shape[1] == 2:
        rows = np.stack([rows[:, 0], z, rows[:, 1], z], axis=1)
    elif rows.shape[1] == 3:
        rows = np.stack([rows[:, 0], rows[:, 1], rows[:, 2], z], axis=1)
    return np.ascontiguousarray(rows)


def overdraft_rule_order(form: int, t: int, row, x: float, cash: float, iniX: float, minCashRequired: float, maxQ: float, fixOrderCost: float,
                         variCost: float) -> float:
    """optQ of one period (CashSimulation.java:1152-1165, :1191-1202, :1228-1240); row = (s, C, S, S2)."""
    s, c, S, S2 = (float(v) for v in row)
    if form == _abi.ORULE_SCS1S2:
        if t == 0:
            return S - iniX
        if not x < s:
            return 0.0
        return S - x if cash <= c + 0.1 else S2 - x
    if t == 0:
        return S if form == _abi.ORULE_SS else S - s
    m = min(max(0.0, (cash - minCashRequired - fixOrderCost) / variCost), maxQ)
    orders = x < s and (form == _abi.ORULE_SS or cash > c)
    return min(m, S - x) if orders else 0.0


class CashSimulation(Simulation):
    """sdp.cash.CashSimulation(distributions, sampleNum, recursion, discountFactor): the SDP simulation of Simulation plus the
    rollouts of an (s, C, S) ordering rule -- simulatesCS in its two forms and simulatesMeanCS (CashSimulation.java:996-1134),
    the twelve extra columns of CashConstraintTesting.main.  sampler="device" (the default here): demand paths are drawn, every
    rule rolled and the means reduced on the device in one call (SdpEngine.cash_rule_simulate; DESIGN 4, "Cash rule rollout"); a
    rule needs no solve.  sampler="host": the same rules through the recursion's Python lambdas on host-sampled demands.
    The rule is an argument (FindsCS is not mirrored).  Over a CustomFunctor recursion (user lambdas) the overdraft drivers' rules
    -- simulatesSOD, simulatesCSDraft, simulatesSOD2, several at once: simulateOverdraftRules -- run through the compiled text
    (SdpEngine.custom_rule_simulate; DESIGN 4, "User-functor rollouts"); fitss.FindsSOverDraft reads them off the table."""

    def __init__(self, distributions: Sequence, sampleNum: int, recursion, discountFactor: float = 1.0, seed: int = 12345,
                 sampler: str = "device"):
        super().__init__(distributions, sampleNum, recursion, discountFactor, seed, sampler)
        self.last_results = None

    def _grid(self):
        f = self.recursion.functor
        return (float(f.minInventoryState), float(f.stepSize), self.recursion.engine.rule_table_points())

    def _pack(self, rules):
        """rules: (form, optsCS[, cacheC1Values[, cacheC2Values]]) each -> forms[R], rows[R, T, 4], c1_tab, c2_tab (None when no
        rule brings that map)."""
        T, grid = self.recursion.T, self._grid()
        forms, rows, c1, c2 = [], [], [], []
        for rule in rules:
            form, opts = int(rule[0]), rule[1]
            r = cash_rule_rows(form, opts)
            if r.shape[0] != T:
                raise ValueError(f"optsCS has {r.shape[0]} periods, the horizon is {T}")
            forms.append(form)
            rows.append(r)
            c1.append(rule[2] if len(rule) > 2 else None)
            c2.append(rule[3] if len(rule) > 3 else None)

        def tabs(maps):
            if all(m is None for m in maps):
                return None
            return np.stack([pack_cash_rule_table(m, T, *grid) for m in maps])

        return np.asarray(forms, dtype=np.int32), np.stack(rows), tabs(c1), tabs(c2)

    def simulateRulesOnDemands(self, iniState, rules, demands, minCashRequired, maxQ, fixOrderCost, variCost) -> np.ndarray:
        """The reference's loops through the recursion's lambdas (sampler="host" and the cross-check of the device rollout):
        path sums [R, n] of the rules along demands[n, T]."""
        forms, rows, c1, c2 = self._pack(rules)
        grid, disc = self._grid(), self._discount()
        out = np.empty((len(forms), len(demands)))
        for r, form in enumerate(forms.tolist()):
            for i, path in enumerate(demands):
                total, state = 0.0, iniState
                for t, d in enumerate(path):
                    q = cash_rule_order(form, t, rows[r, t], None if c1 is None else c1[r, t], None if c2 is None else c2[r, t],
                                        state.getIniInventory(), state.getIniCash(), minCashRequired, maxQ, fixOrderCost, variCost, grid)
                    total += disc[t] * self.immediateValue(state, q, float(d))
                    state = self.stateTransition(state, q, float(d))
                out[r, i] = total
        return out

    def simulateRules(self, iniState, rules, minCashRequired, maxQ, fixOrderCost, variCost) -> np.ndarray:
        """Several rules along the SAME demand paths in one call: rules = [(form, optsCS[, cacheC1Values[, cacheC2Values]]),
        ...], form one of _abi.RULE_SC12S / RULE_SC1S / RULE_SMEANCS.  Returns mean + iniCash per rule; last_values holds the
        path sums [R, n], last_results the device's results."""
        if self.sampler == "device":
            forms, rows, c1, c2 = self._pack(rules)
            res, sums = self.recursion.engine.cash_rule_simulate(
                self.sampleNum, self.seed, iniState.getIniInventory(), iniState.getIniCash(), forms, rows, c1_tab=c1, c2_tab=c2,
                min_cash_required=minCashRequired, max_q=maxQ, fix_order_cost=fixOrderCost, vari_cost=variCost, mode="lhs",
                discount=self._discount(), want_sums=True)
            self.last_results, self.last_values = res, sums
            return np.array([r.mean + iniState.getIniCash() for r in res])
        samples = self.sampling.generateLHSamples(self.distributions, self.sampleNum)
        sums = self.simulateRulesOnDemands(iniState, rules, round_demands(samples), minCashRequired, maxQ, fixOrderCost, variCost)
        self.last_results, self.last_values = None, sums
        return np.array([math.fsum(s.tolist()) / len(s) + iniState.getIniCash() for s in sums])

    def simulatesCS(self, iniState, optsCS, cacheC1Values, *rest) -> float:
        """Both reference overloads: (iniState, optsCS, cacheC1Values, cacheC2Values, minCashRequired, maxQ, fixOrderCost,
        variCost) is the (s, C1, C2, S) rule (CashSimulation.java:996-1042); without cacheC2Values -- (iniState, optsCS,
        cacheC1Values, overheadCost, maxQ, fixOrderCost, variCost) -- the (s, C1, S) rule (:1050-1093)."""
        if len(rest) == 5:
            return float(self.simulateRules(iniState, [(_abi.RULE_SC12S, optsCS, cacheC1Values, rest[0])], *rest[1:])[0])
        if len(rest) == 4:
            return float(self.simulateRules(iniState, [(_abi.RULE_SC1S, optsCS, cacheC1Values)], *rest)[0])
        raise TypeError("simulatesCS(iniState, optsCS, cacheC1Values, [cacheC2Values,] minCashRequired, maxQ, fixOrderCost, variCost)")

    def simulatesMeanCS(self, iniState, optsCS, minCashRequired, maxQ, fixOrderCost, variCost) -> float:
        """CashSimulation.java:1101-1134: the (s, C, S) rule with one C per period."""
        return float(self.simulateRules(iniState, [(_abi.RULE_SMEANCS, optsCS)], minCashRequired, maxQ, fixOrderCost, variCost)[0])

    # ---- the overdraft drivers' rules over a CustomFunctor recursion ("User-functor rollouts") ----------------------
    def simulateOverdraftRulesOnDemands(self, iniState, rules, demands, minCashRequired=0.0, maxQ=0.0, fixOrderCost=0.0,
                                        variCost=1.0) -> np.ndarray:
        """The reference's loops (CashSimulation.java:1142-1250) through the recursion's Python lambdas: path sums [R, n] of the
        rules along demands[n, T] (sampler="host" and the cross-check of the device rollout)."""
        T, disc = self.recursion.T, self._discount()
        x0 = iniState.getIniInventory()
        out = np.empty((len(rules), len(demands)))
        for r, (form, opts) in enumerate(rules):
            rows = overdraft_rule_rows(int(form), opts, T)
            for i, path in enumerate(demands):
                total, state = 0.0, iniState
                for t, d in enumerate(path):
                    q = overdraft_rule_order(int(form), t, rows[t], state.getIniInventory(), state.getIniCash(), x0, minCashRequired, maxQ,
                                             fixOrderCost, variCost)
                    total += disc[t] * self.immediateValue(state, q, float(d))
                    if t + 1 < T:
                        state = self.stateTransition(state, q, float(d))
                out[r, i] = total
        return out

    def simulateOverdraftRules(self, iniState, rules, minCashRequired=0.0, maxQ=0.0, fixOrderCost=0.0, variCost=1.0) -> np.ndarray:
        """Several overdraft rules along the SAME demand paths in one call: rules = [(form, opts), ...], form one of
        _abi.ORULE_SS (opts [T, 2] = (s, S)), ORULE_SCS ([T, 3] = (s, C, S)), ORULE_SCS1S2 ([T, 4] = (s, C, S1, S2)).  Returns
        mean + iniCash per rule; last_values holds the path sums [R, n], last_results the device's results."""
        T = self.recursion.T
        if self.sampler == "device":
            forms = np.array([int(f) for f, _ in rules], dtype=np.int32)
            rows = np.stack([overdraft_rule_rows(int(f), o, T) for f, o in rules])
            res, sums = self.recursion.engine.custom_rule_simulate(
                self.sampleNum, self.seed, iniState.getIniInventory(), iniState.getIniCash(), forms, rows, min_cash_required=minCashRequired,
                max_q=maxQ, fix_order_cost=fixOrderCost, vari_cost=variCost, mode="lhs", discount=self._discount(), want_sums=True)
            self.last_results, self.last_values = res, sums
            return np.array([r.mean + iniState.getIniCash() for r in res])
        samples = self.sampling.generateLHSamples(self.distributions, self.sampleNum)
        sums = self.simulateOverdraftRulesOnDemands(iniState, rules, round_demands(samples), minCashRequired, maxQ, fixOrderCost, variCost)
        self.last_results, self.last_values = None, sums
        return np.array([math.fsum(s.tolist()) / len(s) + iniState.getIniCash() for s in sums])

    def simulatesSOD(self, iniState, optsS, minCashRequired, maxQ, fixOrderCost, variCost) -> float:
        """CashSimulation.java:1180-1211: the (s, S) rule under overdraft."""
        return float(self.simulateOverdraftRules(iniState, [(_abi.ORULE_SS, optsS)], minCashRequired, maxQ, fixOrderCost, variCost)[0])

    def simulatesCSDraft(self, iniState, optsCS, minCashRequired, maxQ, fixOrderCost, variCost) -> float:
        """CashSimulation.java:1142-1173: the (s, C, S) rule under an overdraft limit."""
        return float(self.simulateOverdraftRules(iniState, [(_abi.ORULE_SCS, optsCS)], minCashRequired, maxQ, fixOrderCost, variCost)[0])

    def simulatesSOD2(self, iniState, optsCS) -> float:
        """CashSimulation.java:1218-1250: the (s, C, S1, S2) rule; it reads no scalar."""
        return float(self.simulateOverdraftRules(iniState, [(_abi.ORULE_SCS1S2, optsCS)])[0])


class CashSimulationXR(Simulation):
    """sdp.cash.CashSimulationXR(distributions, sampleNum, recursionXR, discountFactor, fixOrderCost, price, variOrderCost,
    holdCost, salvageValue) (CashSimulationXR.java:48-62): the validation steps of cash.singleItem.CashConstraintXR.main on the
    (x, R) state -- simulateSDPGivenSamplNum (:91-113), simulateSDPwithErrorConfidence (:115-147) and simulateAStar (:153-173),
    the rollout of Chao's a* levels (RecursionG.getOptY).  sampler="device" (the default here): demand paths are drawn, rolled
    and the means reduced on the device in one call (SdpEngine.xr_simulate; DESIGN 4, "(x, R) rollout"); the a* rollout needs
    no solve.  sampler="host": the reference's loops through the recursion's Python lambdas on host-sampled demands.  Of the
    five cost arguments only variOrderCost is read (:162), as in the reference."""

    def __init__(self, distributions: Sequence, sampleNum: int, recursionXR, discountFactor: float = 1.0, fixOrderCost: float = 0.0,
                 price: float = 0.0, variOrderCost: float = 1.0, holdCost: float = 0.0, salvageValue: float = 0.0, seed: int = 12345,
                 sampler: str = "device"):
        super().__init__(distributions, sampleNum, recursionXR, discountFactor, seed, sampler)
        self.fixOrderCost, self.price, self.variOrderCost = float(fixOrderCost), float(price), float(variOrderCost)
        self.holdCost, self.salvageValue = float(holdCost), float(salvageValue)
        self.last_results = None
        self.last_demands = None

    @staticmethod
    def _levels(optY) -> np.ndarray:
        lv = np.asarray(optY, dtype=np.float64)
        if lv.ndim not in (1, 2):
            raise ValueError(f"optY of shape {lv.shape}: (T,) for one rule, (R, T) for several")
        return lv

    def simulateOnDemands(self, iniState, demands, optY=None) -> np.ndarray:
        """The reference's loops through the recursion's lambdas (sampler="host" and the cross-check of the device rollout)
        along demands[n, T]: optY None -- the policy table (getAction, :101-105), path sums [n]; optY of shape (T,) -- the a*
        rule (:161-165), [n]; of shape (R, T) -- [R, n]."""
        disc = self._discount()
        if optY is None:
            out = np.empty(len(demands))
            for i, path in enumerate(demands):
                total, state = 0.0, iniState
                for t, d in enumerate(path):
                    self.recursion.getExpectedValue(state)
                    optQ = self.recursion.getAction(state)
                    total += disc[t] * self.immediateValue(state, optQ, float(d))
                    state = self.stateTransition(state, optQ, float(d))
                out[i] = total
            return out
        lv = self._levels(optY)
        rows = lv[None] if lv.ndim == 1 else lv
        out = np.empty((len(rows), len(demands)))
        c = self.variOrderCost
        for r, row in enumerate(rows.tolist()):
            for i, path in enumerate(demands):
                total, state = 0.0, iniState
                for t, d in enumerate(path):
                    thisY = row[t] if state.getIniR() > c * row[t] else state.getIniR() / c  # :162
                    total += disc[t] * self.immediateValue(state, thisY, float(d))
                    state = self.stateTransition(state, thisY, float(d))
                out[r, i] = total
        return out[0] if lv.ndim == 1 else out

    def _xr_call(self, iniState, n: int, mode: str, first_path: int = 0, levels=None):
        rec = self.recursion
        if levels is None:
            rec.getExpectedValue(iniState)  # solves on first use, as :101 does
        res, sums, dem = rec.engine.xr_simulate(n, self.seed, iniState.getIniInventory(), iniState.getIniR(), levels,
                                                vari_cost=self.variOrderCost, mode=mode, first_path=first_path,
                                                discount=self._discount(), want_sums=True, want_demands=True)
        self.last_results, self.last_result, self.last_demands = res, res[0], dem
        if res[0].n_valid != res[0].n_paths:
            raise RuntimeError(f"{res[0].n_paths - res[0].n_valid} sample paths left the state grid after period 1 (a start whose inventory "
                               "is no grid value); the reference would re-enter the recursion there")
        return res, sums

    @staticmethod
    def _host_demands(samples) -> np.ndarray:
        """`Math.round(Math.max(0, samples[i][t]))` (:103, :130, :163)."""
        return round_demands(np.maximum(0.0, samples))

    def simulateSDPGivenSamplNum(self, iniState) -> float:
        """:91-113: mean of the table policy's totals over sampleNum LHS paths, + iniR."""
        if self.sampler == "device":
            res, sums = self._xr_call(iniState, self.sampleNum, "lhs")
            self.last_values = sums[0]
            return res[0].mean + iniState.getIniR()
        samples = self.sampling.generateLHSamples(self.distributions, self.sampleNum)
        sums = self.simulateOnDemands(iniState, self._host_demands(samples))
        self.last_values = sums
        return math.fsum(sums.tolist()) / len(sums) + iniState.getIniR()

    def simulateSDPwithErrorConfidence(self, iniState, error: float, confidence: float, batch: int = 1000, maxRuns: int = 1000000):
        """:115-147: plain-random paths until the normal confidence radius is below error * mean (at least 1000 runs);
        returns [centre + iniR, radius]."""
        from scipy import stats as _st
        z = float(_st.norm.ppf(0.5 + confidence / 2.0))
        center, radius = 0.0, math.inf
        if self.sampler == "device":
            n, mean, m2 = 0, 0.0, 0.0
            chunks = []
            while n < 1000 or (radius >= center * error and n < maxRuns):
                res, sums = self._xr_call(iniState, batch, "random", first_path=n)
                n, mean, m2 = merge_moments(n, mean, m2, res[0].n_paths, res[0].mean, res[0].m2)
                chunks.append(sums[0])
                center = mean
                radius = z * math.sqrt(m2 / (n - 1)) / math.sqrt(n) if n > 1 else math.inf
            self.last_values = np.concatenate(chunks)
            return [center + iniState.getIniR(), radius]
        vals = np.empty(0)
        while len(vals) < 1000 or (radius >= center * error and len(vals) < maxRuns):
            samples = self.sampling.generateRanSamples(self.distributions, batch)
            vals = np.concatenate([vals, self.simulateOnDemands(iniState, self._host_demands(samples))])
            center = float(vals.mean())
            radius = z * float(vals.std(ddof=1)) / math.sqrt(len(vals))
        self.last_values = vals
        return [center + iniState.getIniR(), radius]

    def simulateAStar(self, optY, iniState):
        """:153-173: the a* rule y = R > variOrderCost * a_t ? a_t : R / variOrderCost over sampleNum LHS paths, + iniR.  optY
        of shape (T,): a float; of shape (R, T): R rules on the SAME demand paths in one call, an array."""
        lv = self._levels(optY)
        if self.sampler == "device":
            res, sums = self._xr_call(iniState, self.sampleNum, "lhs", levels=lv)
            self.last_values = sums[0] if lv.ndim == 1 else sums
            out = np.array([r.mean + iniState.getIniR() for r in res])
        else:
            samples = self.sampling.generateLHSamples(self.distributions, self.sampleNum)
            sums = self.simulateOnDemands(iniState, self._host_demands(samples), lv)
            self.last_values = sums
            out = np.array([math.fsum(s.tolist()) / len(s) + iniState.getIniR() for s in np.atleast_2d(sums)])
        return float(out[0]) if lv.ndim == 1 else out


class RiskSimulation:
    """sdp.cash.RiskSimulation(distributions, sampleNum, recursion): `simulateLostSale` (RiskSimulation.java:206-241),
    the validation run of the survival-probability recursion -- roll the policy along LHS demand paths, count the
    paths that ever hold negative cash and the paths that ever lose a demand.  The walk runs on the device
    (`sdpgpu_simulate`, family SURVIVAL); sampling and the two ratios stay on the host."""

    def __init__(self, distributions: Sequence, sampleNum: int, recursion, seed: int = 12345, sampler: str = "host"):
        """sampler="device": sampling, walk and both counts on the device in one call (see Simulation)."""
        self.sampler = _check_sampler(sampler)
        self.distributions = None if distributions is None else list(distributions)
        self.sampleNum = int(sampleNum)
        self.recursion = recursion
        self.seed = int(seed)
        self.sampling = Sampling(seed)
        self.last_flags = None
        self.last_result = None
        if self.sampler == "device":
            _hand_samplers(recursion, self.distributions)

    def simulateLostSale(self, iniState, immediateValue=None):
        """Returns [simulated survival probability, lost-sale rate] (RiskSimulation.java:237-240)."""
        if self.sampler == "device":
            rec = self.recursion
            rec.getSurvProb(iniState)
            x, cash, _ = rec.functor.tuple_of(iniState)
            res, _, flags = rec.engine.simulate_sampled(self.sampleNum, self.seed, x, cash, 0.0, mode="lhs", want_sums=True)
            if res.n_valid != res.n_paths:
                raise RuntimeError("a sample path left the state grid")
            self.last_flags = flags
            self.last_result = res
            return [1 - res.mean, res.n_lost / float(self.sampleNum)]
        samples = self.sampling.generateLHSamples(self.distributions, self.sampleNum)
        return self.simulateLostSaleOnDemands(iniState, round_demands(samples))

    def simulateLostSaleOnDemands(self, iniState, demands: np.ndarray):
        rec = self.recursion
        rec.getSurvProb(iniState)
        x, cash, _ = rec.functor.tuple_of(iniState)
        went_bankrupt, valid = rec.engine.simulate(demands, np.ones(rec.T), x, cash, 0.0)
        if not valid.all():
            raise RuntimeError("a sample path left the state grid")
        flags = rec.engine.last_sim_flags
        self.last_flags = flags
        lost = int(((flags >> 1) & 1).sum())
        sim_final = 1 - math.fsum(went_bankrupt.tolist()) / float(len(went_bankrupt))
        return [sim_final, lost / float(self.sampleNum)]

    def simulateOnHost(self, iniState, demands: np.ndarray):
        """The reference's loop verbatim through the host lambdas and getAction, for a few paths."""
        rec = self.recursion
        bankrupt = np.zeros(len(demands))
        lost = 0
        for i, row in enumerate(demands):
            state = iniState
            countBefore, countBeforeBankrupt = False, state.getBankruptBefore()
            for d in row:
                rec.getSurvProb(state)
                optQ = rec.getAction(state)
                if state.getIniCash() < 0:
                    optQ = 0.0
                if state.getIniInventory() + optQ < d and not countBefore:
                    lost += 1
                    countBefore = True
                thisValue = state.getIniCash() + rec.immediateValue(state, optQ, float(d))
                state = rec.stateTransition(state, optQ, float(d))
                if thisValue < 0 and not countBeforeBankrupt:
                    bankrupt[i] = 1
                    countBeforeBankrupt = True
        return [1 - bankrupt.sum() / float(len(demands)), lost / float(len(demands))]


class SimulationBatch:
    """`new Simulation(distributions, sampleNum, recursion).simulateSDPGivenSamplNum(initialState)` for every instance of
    a sweep at once (CLSPTesting.java:120-124): `distributions_per_instance[i]` are instance i's T demand distributions
    (None = draw from the instance's own pmf tiles), `recursion_batch` a RecursionBatch of either kind (one grid shape, or
    ragged: every path then moves on its instance's own grid).  Sampling (latin hypercube,
    seeded) and rollout happen on the device in one launch (SdpBatch.simulate_sampled); there is no host sampling."""

    def __init__(self, distributions_per_instance, sampleNum: int, recursion_batch, seed: int = 12345):
        self.recursion = recursion_batch
        self.sampleNum = int(sampleNum)
        self.seed = int(seed)
        self.last_values = None
        batch = recursion_batch.batch
        if distributions_per_instance is not None:
            if len(distributions_per_instance) != len(recursion_batch):
                raise ValueError(f"{len(distributions_per_instance)} distribution lists but {len(recursion_batch)} instances")
            for i, dists in enumerate(distributions_per_instance):
                if dists is None:
                    continue
                if len(dists) != recursion_batch.T:
                    raise ValueError(f"instance {i}: {len(dists)} distributions, the horizon is {recursion_batch.T}")
                for t, d in enumerate(dists):
                    batch.set_sampler(i, t, d)

    def setSampleNum(self, n: int):
        self.sampleNum = int(n)

    def simulateSDPGivenSamplNum(self, iniStates=None, want_sums: bool = False) -> np.ndarray:
        """The n means (Simulation.java:53-74 per instance).  iniStates: None = every functor's iniInventory, or one
        State per instance."""
        self.recursion._solve()
        ini = None if iniStates is None else [s.getIniInventory() for s in iniStates]
        out = self.recursion.batch.simulate_sampled(self.sampleNum, self.seed, ini_x=ini, want_sums=want_sums)
        if want_sums:
            self.last_values = out[1]
            return out[0]
        return out

    def _simulate_rule(self, levels: int, iniStates, optsS, want_sums: bool):
        if optsS is None:
            self.recursion._solve()  # the rule is fitted on the device from the solved tables
        ini = None if iniStates is None else [s.getIniInventory() for s in iniStates]
        out = self.recursion.batch.simulate_ss_sampled(levels, self.sampleNum, self.seed, ss=optsS, ini_x=ini, want_sums=want_sums)
        if want_sums:
            self.last_values = out[1]
            return out[0]
        return out

    def simulateSinglesS(self, iniStates=None, optsS=None, want_sums: bool = False) -> np.ndarray:
        """SimulateFitsS.simulateSinglesS (SimulateFitsS.java:32-54) for every instance: the n means of the one-level rule
        optsS [n, T, 2] (None = FitsS.getSinglesS of every instance, fitted on the device), along the SAME demand paths as
        simulateSDPGivenSamplNum (same seed: common random numbers)."""
        return self._simulate_rule(1, iniStates, optsS, want_sums)

    def simulateTwosS(self, iniStates=None, optsS=None, want_sums: bool = False) -> np.ndarray:
        """SimulateFitsS.simulateTwosS (SimulateFitsS.java:63-91): optsS [n, T, 4] or None = getTwosS on the device."""
        return self._simulate_rule(2, iniStates, optsS, want_sums)

    def simulateThreesS(self, iniStates=None, optsS=None, want_sums: bool = False) -> np.ndarray:
        """SimulateFitsS.simulateThreesS (SimulateFitsS.java:100-130): optsS [n, T, 6] or None = getThreesS on the device."""
        return self._simulate_rule(3, iniStates, optsS, want_sums)


class SimulateFitsS:
    """capacitated.fitss.SimulateFitsS(distributions, sampleNum, recursion) for ONE backorder-family Recursion: the three
    reference methods, signature (iniState, optsS, maxOrderQuantity).  Internally a batch of one built from the recursion's
    functor and pmf; the rule is explicit, so nothing is solved a second time.  distributions: T demand distributions, or
    None / None entries = the recursion's own pmf tiles.  Sampling is the seeded latin hypercube of the device
    (SdpBatch.simulate_ss_sampled); `last_values` holds the path sums of the last call."""

    def __init__(self, distributions: Sequence, sampleNum: int, recursion, seed: int = 12345):
        from .functors import BackorderFunctor
        if not isinstance(recursion.functor, BackorderFunctor):
            raise TypeError("SimulateFitsS rolls the (s, S) rules of the backorder family (a Recursion over a BackorderFunctor)")
        self.distributions = None if distributions is None else list(distributions)
        if self.distributions is not None and len(self.distributions) != recursion.T:
            raise ValueError(f"{len(self.distributions)} distributions, the horizon is {recursion.T}")
        self.sampleNum = int(sampleNum)
        self.recursion = recursion
        self.seed = int(seed)
        self.last_values = None
        self._batch, self._batch_maxq = None, None

    def _one(self, maxOrderQuantity):
        """The batch of one; rebuilt when the caller's maxOrderQuantity is not the functor's (the rule's cap is an argument
        in the reference, SimulateFitsS.java:32)."""
        from .batch import SdpBatch
        if self._batch is None or self._batch_maxq != float(maxOrderQuantity):
            if self._batch is not None:
                self._batch.close()
            d = self.recursion.functor.to_desc(self.recursion.T, self.recursion.optDirection)
            d.max_order_quantity = float(maxOrderQuantity)
            self._batch = SdpBatch([d], [self.recursion.pmf], ragged=True, device=int(self.recursion.engine.desc.device))
            self._batch_maxq = float(maxOrderQuantity)
            if self.distributions is not None:
                for t, dist in enumerate(self.distributions):
                    if dist is not None:
                        self._batch.set_sampler(0, t, dist)
        return self._batch

    def _simulate(self, levels: int, iniState, optsS, maxOrderQuantity) -> float:
        rule = np.ascontiguousarray(optsS, dtype=np.float64)
        if rule.shape != (self.recursion.T, 2 * levels):
            raise ValueError(f"optsS of shape {rule.shape}: expected [{self.recursion.T}, {2 * levels}]")
        mean, sums = self._one(maxOrderQuantity).simulate_ss_sampled(levels, self.sampleNum, self.seed, ss=rule[None],
                                                                      ini_x=[iniState.getIniInventory()], want_sums=True)
        self.last_values = sums[0]
        return float(mean[0])

    def simulateSinglesS(self, iniState, optsS, maxOrderQuantity) -> float:
        return self._simulate(1, iniState, optsS, maxOrderQuantity)

    def simulateTwosS(self, iniState, optsS, maxOrderQuantity) -> float:
        return self._simulate(2, iniState, optsS, maxOrderQuantity)

    def simulateThreesS(self, iniState, optsS, maxOrderQuantity) -> float:
        return self._simulate(3, iniState, optsS, maxOrderQuantity)

    def close(self):
        if self._batch is not None:
            self._batch.close()
            self._batch = None
