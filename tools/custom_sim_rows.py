"""What the validation half of an overdraft driver costs on the device when its lambdas are USER TEXT, beside the solve.

One user-functor handle of CashOverdraftTesting.main's own shape (CashOverdraftTesting.java:33-69, its first instance: T = 6,
Poisson(7) truncated at the 0.999 quantile, K = 10, v = 1, h = 1, p = 10, B0 = 0, b = 0.05, order limit 50, inventory 0 .. 150,
cash -100 .. 800 in tenths: 151 x 9001 states, discount 0.95), the lambdas of :78-120 as the text of
tests/custom_overdraft_sources.py, and the loop body of :125-149 in Python:

    solve -> getOptTable -> FindsSOverDraft.getsS -> simulatesSOD          (and simulateSDPGivenSamplNum, CashOverdraftLimit.main:122)

Medians and ranges of --samples samples, after one warm-up each; kernel time by HIP events, the host side (argument checks,
uploads, read-back) EXCLUDED:
  a   the solve sweep (sdpgpu_stats: solve_ms)
  b   sdpgpu_custom_simulate_sampled, --paths latin-hypercube paths -- kernel_ms: draws, table rollout, both reductions
  c   sdpgpu_custom_rule_simulate with simulatesSOD's rule from getsS, --paths paths -- kernel_ms: draws, rule rollout, reductions
  d   the host route, the only route before these entry points existed: CashSimulation(sampler="host").simulatesSOD on
      --host-paths paths (Python sampling and lambdas), wall time, SCALED to --paths paths and labelled so
and, once, the wall time of the handle's first rollout call against a later one: the hipRTC compile of the rollout program.
No ratio is fixed in advance; the expectation is only that (b) and (c) are a small fraction of (a).

    python tools/custom_sim_rows.py [--samples 7] [--paths 10000] [--host-paths 1000] [--seed 12345] [--json PATH]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stochastic_inventory_amd as sia  # noqa: E402
from stochastic_inventory_amd import _abi  # noqa: E402
import custom_overdraft_sources as co  # noqa: E402


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def python_lambdas(price, K, v, h, rate, maxQ, mcr, minI, maxI, minC, maxC):
    """CashOverdraftTesting.java:78-120 on the mirror's CashState."""

    def feasible(s):
        m = int(min(maxQ, max(0, (s.getIniCash() - mcr - K) / v)))
        return [float(k) for k in range(m + 1)]

    def imm(s, action, d):
        revenue = price * min(s.getIniInventory() + action, d)
        fixedCost = K if action > 0 else 0
        level = s.getIniInventory() + action - d
        before = s.getIniCash() + revenue - fixedCost - v * action - h * max(level, 0)
        return before - rate * max(-before, 0) - s.getIniCash()

    def trans(s, action, d):
        nx = max(0, s.getIniInventory() + action - d)
        revenue = price * min(s.getIniInventory() + action, d)
        fixedCost = K if action > 0 else 0
        nc = s.getIniCash() + revenue - fixedCost - v * action - h * max(nx, 0)
        nc = nc - max(-nc, 0) * rate
        nc = maxC if nc > maxC else nc
        nc = minC if nc < minC else nc
        nx = maxI if nx > maxI else nx
        nx = minI if nx < minI else nx
        return sia.CashState(s.getPeriod() + 1, float(nx), sia.java_round(nc * 10) / 10.0)

    return feasible, trans, imm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--paths", type=int, default=10000)
    ap.add_argument("--host-paths", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "custom_sim_rows.json"))
    args = ap.parse_args()
    import torch
    T, n = 6, max(args.samples, 1)
    price, K, v, h, rate, maxQ, mcr, gamma, ini_cash = 10.0, 10.0, 1.0, 1.0, 0.05, 50.0, -1000.0, 0.95, 0.0
    params = [price, K, v, h, rate, maxQ, mcr, 0.0, 150.0, -100.0, 800.0]
    shape = sia.OverdraftFunctor(price=price, fixOrderCost=K, variCost=v, maxOrderQuantity=maxQ, minInventoryState=0, maxInventoryState=150,
                                 minCashState=-100, maxCashState=800, cashRoundMult=10.0, cashRoundDiv=10.0, cashRoundIntDiv=False,
                                 iniInventory=0, iniCash=ini_cash)
    dists = [sia.PoissonDist(7.0)] * T
    pmf = sia.GetPmf(dists, 0.999, 1).getpmf()
    feasible, trans, imm = python_lambdas(*params)
    functor = sia.CustomFunctor(shape=shape, source=co.OVERDRAFT_TESTING, params=params, getFeasibleAction=feasible, stateTransitionFn=trans,
                                immediateValueFn=imm)
    rec = sia.CashRecursion(sia.OptDirection.MAX, pmf, feasible, trans, imm, gamma, functor=functor, device=0)
    initial = sia.CashState(1, 0.0, ini_cash)
    final_value = rec.getExpectedValue(initial) + ini_cash  # solves
    eng = rec.engine
    states = [eng.num_states(t) for t in range(1, T + 1)]
    A = []
    for _ in range(n):
        eng.solve(sync=True)
        A.append(eng.stats().solve_ms)
    disc = np.array([gamma ** t for t in range(T)])
    # the one-time compile: the first rollout call of the handle against a later one, wall clock
    t0 = time.perf_counter()
    table = eng.custom_simulate_sampled(args.paths, args.seed, 0.0, ini_cash, discount=disc)
    first_call_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    eng.custom_simulate_sampled(args.paths, args.seed, 0.0, ini_cash, discount=disc)
    later_call_s = time.perf_counter() - t0
    B = []
    for _ in range(n):
        res = eng.custom_simulate_sampled(args.paths, args.seed, 0.0, ini_cash, discount=disc)
        B.append(res.kernel_ms)
        assert res.mean == table.mean and res.n_valid == res.n_paths, "the rollout is not reproducible"
    # simulatesSOD's rule, as the driver finds it
    finder = sia.FindsSOverDraft(T, ini_cash)
    try:
        optsS = finder.getsS(rec.getOptTable())
        rule_note = "FindsSOverDraft.getsS(getOptTable())"
    except IndexError as e:  # the reference's ArrayIndexOutOfBoundsException on this table: a rule near it, so that (c) is still timed
        optsS = np.array([[0.0, 20.0]] + [[8.0, 20.0]] * (T - 1))
        rule_note = f"getsS raised ({e}); a fixed (s, S) = (8, 20) in its place"
    rows = sia.simulation.overdraft_rule_rows(_abi.ORULE_SS, optsS, T)
    kw = dict(min_cash_required=mcr, max_q=maxQ, fix_order_cost=K, vari_cost=v, discount=disc)
    first = eng.custom_rule_simulate(args.paths, args.seed, 0.0, ini_cash, [_abi.ORULE_SS], rows, **kw)  # warm-up
    Cs = []
    for _ in range(n):
        res = eng.custom_rule_simulate(args.paths, args.seed, 0.0, ini_cash, [_abi.ORULE_SS], rows, **kw)
        Cs.append(res[0].kernel_ms)
        assert res[0].mean == first[0].mean, "the rule rollout is not reproducible"
    # the host route: sampling through inverseF, every path through the Python lambdas
    host = sia.CashSimulation(dists, args.host_paths, rec, gamma, seed=args.seed, sampler="host")
    t0 = time.perf_counter()
    host_value = host.simulatesSOD(initial, optsS, mcr, maxQ, K, v)
    host_s = time.perf_counter() - t0
    sim_rule = first[0].mean + ini_cash
    out = {
        "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": n, "seed": args.seed,
        "workload": "CashOverdraftTesting.main[0] as user text: T = 6, Poisson(7) at the 0.999 quantile, K = 10, v = 1, h = 1, p = 10, "
                    "B0 = 0, b = 0.05, order limit 50, discount 0.95, 151 x 9001 states",
        "states_per_period": states, "pmf_points": [len(t) for t in pmf], "paths": args.paths,
        "timing": "kernel time by HIP events (solve_ms, kernel_ms); the host side of a call is excluded",
        "final_value": final_value, "rule": rule_note, "optsS": np.asarray(optsS).tolist(),
        "sim_table_plus_ini_cash": table.mean + ini_cash, "sim_sS_plus_ini_cash": sim_rule,
        "gap_sS_percent": (final_value - sim_rule) * 100 / final_value,
        "a_solve_ms_hip_events": summary(A),
        "b_custom_simulate_sampled_kernel_ms": summary(B),
        "c_custom_rule_simulate_sS_kernel_ms": summary(Cs),
        "d_host_route": {"paths": args.host_paths, "wall_s": host_s, "scaled_to_paths_s": host_s * args.paths / args.host_paths,
                         "label": f"measured on {args.host_paths} paths, scaled linearly to {args.paths}", "value_plus_ini_cash": host_value},
        "rollout_program_first_call_wall_s": first_call_s, "rollout_program_later_call_wall_s": later_call_s,
        "rollout_program_compile_and_load_wall_s": first_call_s - later_call_s,
    }
    rec.engine.close()
    print(json.dumps({k: (v["median"] if isinstance(v, dict) and "median" in v else v) for k, v in out.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
