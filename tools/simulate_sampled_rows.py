"""What the validation step after a solve costs, with the demand paths sampled on the host and on the device.

Two shapes, each a single handle:

  cash   cash.singleItem.CashConstraintTesting.main's own first instance (CashConstraintTesting.java:49-73, 96, 170): inventory
         0..200, integer cash -100..1500, Q <= 150, the ten Poisson(15) periods of demand pattern 1 through GetPmf at the 0.999
         quantile, K = 10, v = 1, price 5, B0 = 3 (iniCash 13), sampleNum = 100000
  clsp   capacitated.CLSPTesting.main's first instance (workloads.clsp_testing_sweep): x in [-500, 500], orders 0..500, T = 8,
         NormalDist(mean, coeVar * mean) demands, 10000 paths (CLSPTesting.java:120-124)

Medians and ranges of --samples samples (b and c after one warm-up; a, seconds of Python, without) of

  a   Simulation(sampler="host").simulateSDPGivenSamplNum: wall time.  Sampling through inverseF in Python, the upload, the
      rollout (sdpgpu_simulate), the mean on the host -- the code of the commit before the device sampler, so the baseline
  b   the same with sampler="device": wall time, and kernel_ms (HIP events around the rollout and both reductions)
  c   the solve sweep of the same handle (sdpgpu_stats: solve_ms, HIP events)

    python tools/simulate_sampled_rows.py [--shapes cash,clsp] [--samples 5] [--seed 12345] [--host-paths-cap 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import stochastic_inventory_amd as sia  # noqa: E402
from stochastic_inventory_amd import pmf, workloads  # noqa: E402
from stochastic_inventory_amd.simulation import Simulation  # noqa: E402


def cash_constraint_testing():
    means = [15.0] * 10
    dists = [pmf.PoissonDist(m) for m in means]
    tiles = pmf.GetPmf(dists, 0.999, 1).getpmf()
    f = sia.CashFunctor(price=5, fixOrderCost=10, variCost=1, holdingCost=0, salvageValue=0.5, penaltyCost=0, overheadCost=0,
                        maxOrderQuantity=150, minInventoryState=0, maxInventoryState=200, minCashState=-100, maxCashState=1500,
                        cashRoundMult=1.0, cashRoundDiv=1.0, cashRoundIntDiv=True, cashFormula=1, iniInventory=0, iniCash=13)
    rec = sia.CashRecursion(sia.OptDirection.MAX, tiles, functor=f, discountFactor=1.0, device=0)
    return ("CashConstraintTesting.main, first instance: 201 x 1601 states, Q <= 150, T = 10, Poisson(15)", dists, rec,
            sia.CashState(1, 0.0, 13.0), 100000, 1.0)


def clsp_testing():
    w = workloads.clsp_testing_sweep(patterns=(1,))[0]
    dists = [pmf.NormalDist(float(m), w.coeVar * m) for m in workloads.CLSP_TESTING_DEMANDS[w.pattern - 1]]
    rec = sia.Recursion(sia.OptDirection.MIN, w.pmf, functor=w.functor, device=0)
    return (f"CLSPTesting.main, first instance ({w.name}): 1001 states x 501 actions, T = 8", dists, rec,
            sia.State(1, w.functor.iniInventory), 10000, 1.0)


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def measure(make, samples, seed, host_cap):
    what, dists, rec, ini, n, gamma = make()
    value = rec.getExpectedValue(ini)  # solves
    eng = rec.engine
    C = []
    for _ in range(samples):
        eng.solve(sync=True)
        C.append(eng.stats().solve_ms)
    dev = Simulation(dists, n, rec, discountFactor=gamma, seed=seed, sampler="device")
    sim_dev = dev.simulateSDPGivenSamplNum(ini)  # warm-up
    B, Bk = [], []
    for _ in range(samples):
        t0 = time.perf_counter()
        again = dev.simulateSDPGivenSamplNum(ini)
        B.append((time.perf_counter() - t0) * 1e3)
        Bk.append(dev.last_result.kernel_ms)
        assert again == sim_dev, "the device sampler is not reproducible"
    n_host = n if host_cap <= 0 else min(n, host_cap)
    for t in range(rec.T):
        eng.set_sampler(t, None)
    host = Simulation(dists, n_host, rec, discountFactor=gamma, seed=seed)
    A, sim_host = [], None
    for _ in range(samples):  # (no warm-up: seconds of Python against a rollout that (b) has warmed already)
        t0 = time.perf_counter()
        sim_host = host.simulateSDPGivenSamplNum(ini)
        A.append((time.perf_counter() - t0) * 1e3)
        print(f"  host sampler, {n_host} paths: {A[-1]:.0f} ms", file=sys.stderr, flush=True)
    out = {
        "workload": what, "paths": n, "periods": rec.T, "quantiles": n * rec.T, "seed": seed,
        "value_V1": value + (ini.getIniCash() if hasattr(ini, "getIniCash") else 0.0),
        "simValue_host_sampler": sim_host, "simValue_device_sampler": sim_dev,
        "a_host_sampler_wall_ms": summary(A), "a_paths": n_host, "a_is_scaled": n_host != n,
        "b_device_sampler_wall_ms": summary(B), "b_device_sampler_kernel_ms": summary(Bk),
        "c_solve_ms_hip_events": summary(C),
    }
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cash,clsp")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--host-paths-cap", type=int, default=0, help="run (a) on at most this many paths (0: all; a capped run is marked)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sim_sampled_rows.json"))
    args = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": args.samples, "rows": {}}
    table = {"cash": cash_constraint_testing, "clsp": clsp_testing}
    for name in args.shapes.split(","):
        row = measure(table[name], max(args.samples, 1), args.seed, args.host_paths_cap)
        res["rows"][name] = row
        print(json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
        with open(args.json, "w") as fh:  # (written after every shape: a long run leaves what it has)
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
