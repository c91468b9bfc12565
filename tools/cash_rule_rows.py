"""What the four (s, C, S) rule rollouts of the cash sweep's loop body cost on the device, beside the solve and the table rollout.

One handle of CashConstraintTesting.main's own shape (CashConstraintTesting.java:49-73, its first instance: T = 10, Poisson(15)
truncated at the 0.999 quantile, K = 10, v = 1, p = 5, h = 0, B0 = 3 so iniCash = 13, overhead 0, order limit 150, inventory
0 .. 200, integer cash -100 .. 1500, formula 1), the loop body of CashConstraintTesting.java:153-244 in Python:

    solve -> simulateSDPGivenSamplNum -> simulatesCS (s, C1, C2, S) -> simulatesCS (s, C1, S) -> simulatesMeanCS -> simulatesCS (MIP)

The rule is not fitted as FindsCS fits it (out of scope); it is read off the solved policy table by this recipe, per
period t: a state "orders" when its policy entry is above 0;
    s_t    = 1 + the largest inventory at which any cash level orders (0.5 when none does)
    S_t    = the most frequent order-up-to level x + q among the ordering states (s_t when none orders)
    C1_t(x) = (the smallest cash that orders at inventory x) - 1, C2_t(x) = (the largest cash that orders at x) + 1; absent where
              no cash orders at x
    C_t    = the mean of the present C1_t(x) (0 when none)
Four rules of mixed forms on the same 100 000 latin-hypercube paths: (s, C1(x), C2(x), S), (s, C1(x), S), (s, C, S), and -- standing
in for the MIP's rule, which arrives as an array too -- (s, C1(x), S + 1).

Medians and ranges of --samples samples, after one warm-up each:
  a   the solve sweep (sdpgpu_stats: solve_ms, HIP events)
  b   the four rules in ONE sdpgpu_cash_rule_simulate call -- kernel_ms: the rollout and both reductions of all four
  c   sdpgpu_simulate_sampled (the table policy) on the same handle and paths -- kernel_ms
  d   the host route: CashSimulation(sampler="host").simulateRules on --host-paths paths (Python sampling and lambdas), wall
      time scaled to 100 000 paths
No speed threshold is set: nobody has measured this, and (b) is expected to be a small fraction of (a).

    python tools/cash_rule_rows.py [--samples 7] [--paths 100000] [--host-paths 1000] [--seed 12345] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import stochastic_inventory_amd as sia  # noqa: E402
from stochastic_inventory_amd import _abi  # noqa: E402


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def rule_from_table(eng, T):
    """The recipe of the module text -> rows[T, 4] = (s, C, 0, S), c1[T, NX], c2[T, NX]."""
    nx = eng.rule_table_points()
    rows, c1, c2 = np.zeros((T, 4)), np.full((T, nx), np.nan), np.full((T, nx), np.nan)
    for t in range(T):
        x_lo, gx, nc, _ = eng.grid(t + 1)
        assert gx == nx
        pol = eng.policy(t + 1).reshape(nx, nc)
        cash = np.array([eng.cash_value(ic) for ic in range(nc)])
        orders = pol > 0
        xs = np.nonzero(orders.any(axis=1))[0]
        s = float(x_lo + xs.max() + 1) if len(xs) else 0.5
        S = s
        if len(xs):
            ix, ic = np.nonzero(orders)
            levels, counts = np.unique(x_lo + ix + pol[ix, ic], return_counts=True)
            S = float(levels[np.argmax(counts)])
            for i in xs:
                at = np.nonzero(orders[i])[0]
                c1[t, i], c2[t, i] = cash[at.min()] - 1.0, cash[at.max()] + 1.0
        rows[t] = (s, float(np.nanmean(c1[t])) if len(xs) else 0.0, 0.0, S)
    return rows, c1, c2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--paths", type=int, default=100000)
    ap.add_argument("--host-paths", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "cash_rule_rows.json"))
    args = ap.parse_args()
    import torch
    T, n = 10, max(args.samples, 1)
    K, v, price, B0, overhead, max_q = 10.0, 1.0, 5.0, 3.0, 0.0, 150.0
    ini_cash = K + overhead + v * B0
    f = sia.CashFunctor(price=price, fixOrderCost=K, variCost=v, holdingCost=0, overheadCost=overhead, salvageValue=0.5, penaltyCost=0,
                        maxOrderQuantity=max_q, minInventoryState=0, maxInventoryState=200, minCashState=-100, maxCashState=1500,
                        cashRoundMult=1.0, cashRoundDiv=1.0, cashRoundIntDiv=True, cashFormula=1, iniInventory=0, iniCash=ini_cash)
    dists = [sia.PoissonDist(15.0)] * T
    pmf = sia.GetPmf(dists, 0.999, 1).getpmf()
    rec = sia.CashRecursion(sia.OptDirection.MAX, pmf, functor=f, discountFactor=1.0, device=0)
    initial = sia.CashState(1, 0.0, ini_cash)
    final_value = rec.getExpectedValue(initial) + ini_cash  # solves
    eng = rec.engine
    A = []
    for _ in range(n):
        eng.solve(sync=True)
        A.append(eng.stats().solve_ms)
    rows, c1, c2 = rule_from_table(eng, T)
    mip = rows.copy()
    mip[:, 3] += 1.0
    forms = [_abi.RULE_SC12S, _abi.RULE_SC1S, _abi.RULE_SMEANCS, _abi.RULE_SC1S]
    rules = np.stack([rows, rows, rows, mip])
    tabs1, tabs2 = np.stack([c1] * 4), np.stack([c2] * 4)
    kw = dict(min_cash_required=overhead, max_q=max_q, fix_order_cost=K, vari_cost=v, c1_tab=tabs1, c2_tab=tabs2)
    first = eng.cash_rule_simulate(args.paths, args.seed, 0.0, ini_cash, forms, rules, **kw)  # warm-up
    B = []
    for _ in range(n):
        res = eng.cash_rule_simulate(args.paths, args.seed, 0.0, ini_cash, forms, rules, **kw)
        B.append(res[0].kernel_ms)
        assert [r.mean for r in res] == [r.mean for r in first], "the rollout is not reproducible"
    table = eng.simulate_sampled(args.paths, args.seed, 0.0, ini_cash)  # warm-up
    Cs = []
    for _ in range(n):
        Cs.append(eng.simulate_sampled(args.paths, args.seed, 0.0, ini_cash).kernel_ms)
    # the host route, as the reference runs it: sampling through inverseF, every path through the lambdas, four times
    cache1 = {(t + 1, float(ix)): float(c1[t, ix]) for t in range(T) for ix in range(c1.shape[1]) if not np.isnan(c1[t, ix])}
    cache2 = {(t + 1, float(ix)): float(c2[t, ix]) for t in range(T) for ix in range(c2.shape[1]) if not np.isnan(c2[t, ix])}
    host = sia.CashSimulation(dists, args.host_paths, rec, 1.0, seed=args.seed, sampler="host")
    host_rules = [(forms[0], rows, cache1, cache2), (forms[1], rows[:, [0, 1, 3]], cache1), (forms[2], rows[:, [0, 1, 3]]),
                  (forms[3], mip[:, [0, 1, 3]], cache1)]
    t0 = time.perf_counter()
    host_means = host.simulateRules(initial, host_rules, overhead, max_q, K, v)
    host_s = time.perf_counter() - t0
    out = {
        "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": n, "seed": args.seed,
        "workload": "CashConstraintTesting.main[0]: T = 10, Poisson(15) at the 0.999 quantile, K = 10, v = 1, p = 5, h = 0, B0 = 3, "
                    "order limit 150, 201 x 1601 states",
        "paths": args.paths, "rules": ["(s, C1(x), C2(x), S)", "(s, C1(x), S)", "(s, C, S)", "(s, C1(x), S + 1) in the MIP's place"],
        "final_value": final_value, "rule_rows_s_C_0_S": rows.tolist(),
        "sim_table_plus_ini_cash": table.mean + ini_cash,
        "sim_rules_plus_ini_cash": [r.mean + ini_cash for r in first],
        "gap_rules_percent": [(final_value - (r.mean + ini_cash)) * 100 / final_value for r in first],
        "a_solve_ms_hip_events": summary(A),
        "b_four_rules_one_call_kernel_ms": summary(B),
        "c_simulate_sampled_kernel_ms": summary(Cs),
        "d_host_route": {"paths": args.host_paths, "wall_s": host_s, "scaled_to_paths_s": host_s * args.paths / args.host_paths,
                         "means_plus_ini_cash": [float(m) for m in host_means]},
    }
    rec.engine.close()
    print(json.dumps({k: (v["median"] if isinstance(v, dict) and "median" in v else v) for k, v in out.items() if k != "rule_rows_s_C_0_S"}),
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
