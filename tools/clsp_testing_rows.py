"""capacitated.CLSPTesting.main as ONE batch: solve the 540 instances (SdpBatch.solve), simulate their policies along 10000
latin-hypercube demand paths each, drawn on the device from NormalDist(mean, coeVar * mean) as the reference does
(SdpBatch.simulate_sampled; CLSPTesting.java:120-124), and print the rows of the reference's result file
(CLSPTesting.java:30, 122-140):

    K, v, h, I0, pai, coeVar, DemandPatt, OpValue, Time, simValue

`Time` is the batch's solve time divided by the number of instances, in seconds (the reference times each Recursion on its
own; a batch has one sweep).  Times are measured too, medians of --samples after a warm-up:

  B   simulate_sampled alone: HIP events on the batch's stream around the rollout and mean kernels (SdpBatch.simulate_ms)
  B'  wall time of everything a driver pays: create, pmfs, samplers, solve, V_1(ini), simulate, means on the host
  A   the same rows WITHOUT the batched simulation: one SdpEngine per instance, solved, demands sampled on the host
      (simulation.Sampling.generateLHSamples + round_demands), SdpEngine.simulate.  Host sampling takes seconds per
      instance, so A runs on --baseline-instances instances spread over the sweep and is SCALED to all of them.

    python tools/clsp_testing_rows.py [--patterns 1,7] [--paths 10000] [--seed 12345] [--samples 5] [--baseline-instances 4]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import stochastic_inventory_amd as sia
from stochastic_inventory_amd import pmf, workloads
from stochastic_inventory_amd.simulation import Sampling, round_demands


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="", help="subset of the demand patterns 1..10 (default: all: 540 instances)")
    ap.add_argument("--paths", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--baseline-instances", type=int, default=4, help="instances the per-handle path A is run on (0: skip A)")
    ap.add_argument("--csv", default=os.path.join(ROOT, "profiles", "batch_clsp_testing_rows.csv"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "batch_clsp_testing_sim.json"))
    args = ap.parse_args()
    patterns = tuple(int(x) for x in args.patterns.split(",")) if args.patterns else None
    ws = workloads.clsp_testing_sweep(patterns)
    n = len(ws)
    dists = [[pmf.NormalDist(float(m), w.coeVar * m) for m in workloads.CLSP_TESTING_DEMANDS[w.pattern - 1]] for w in ws]

    def descs():
        out = [w.desc() for w in ws]
        for d in out:
            d.device = 0
        return out

    def whole():
        """B': (OpValue[n], simValue[n], batch) from nothing"""
        b = sia.SdpBatch(descs(), [w.pmf for w in ws])
        for i in range(n):
            for t, d in enumerate(dists[i]):
                b.set_sampler(i, t, d)
        b.solve(sync=False)
        op, _ = b.initial()
        sim = b.simulate_sampled(args.paths, args.seed)
        return op, sim, b

    op, sim, batch = whole()  # warm-up; these are the rows
    solve_ms = batch.stats().solve_ms
    B, S = [], []
    for _ in range(max(args.samples, 1)):
        again = batch.simulate_sampled(args.paths, args.seed)
        assert np.array_equal(again, sim), "simulate_sampled is not reproducible"
        B.append(batch.simulate_ms())
        batch.solve(sync=True)
        S.append(batch.stats().solve_ms)
    batch.close()
    B1 = []
    for _ in range(max(args.samples, 1)):
        t0 = time.perf_counter()
        _, _, b = whole()
        b.close()
        B1.append((time.perf_counter() - t0) * 1e3)

    # ---- A: what the same rows cost through handles and host sampling --------------------------------------------------------
    A, picked = [], []
    if args.baseline_instances > 0:
        picked = sorted({int(round(k)) for k in np.linspace(0, n - 1, args.baseline_instances)})

        def handles():
            out = []
            for i in picked:
                w = ws[i]
                d = w.desc()
                d.device = 0
                with sia.SdpEngine(d, w.pmf) as eng:
                    eng.solve(sync=True)
                    v1 = eng.values(1)[int(w.functor.iniInventory - w.functor.minInventory)]
                    dem = round_demands(Sampling(args.seed).generateLHSamples(dists[i], args.paths))
                    sums, _ = eng.simulate(dem, np.ones(w.T), w.functor.iniInventory, 0.0, 0.0)
                    out.append((v1, math.fsum(sums.tolist()) / len(sums)))
            return out

        first = handles()
        for (v1, _), i in zip(first, picked):
            assert v1 == op[i], "handle and batch disagree on OpValue"
        for _ in range(max(args.samples, 1)):
            t0 = time.perf_counter()
            handles()
            A.append((time.perf_counter() - t0) * 1e3)

    os.makedirs(os.path.dirname(os.path.abspath(args.csv)), exist_ok=True)
    lines = ["K,v,h,I0,pai,coeVar,DemandPatt,OpValue,Time,simValue"]
    for i, w in enumerate(ws):
        f = w.functor
        lines.append(f"{f.fixedOrderingCost:g},{f.variOrderingCost:g},{f.holdingCost:g},{f.iniInventory:g},{f.penaltyCost:g},{w.coeVar:g},"
                     f"{w.pattern},{op[i]!r},{solve_ms / n / 1e3:.9f},{sim[i]!r}")
    with open(args.csv, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[:4]) + f"\n... {n} rows -> {os.path.relpath(args.csv, ROOT)}")

    def summary(xs):
        return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)} if xs else None

    import torch
    rel = np.abs(sim - op) / op
    res = {
        "workload": f"CLSPTesting.main, {n} instances of 1001 states x 501 actions, T = 8, {args.paths} paths each",
        "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "",
        "instances": n, "paths": args.paths, "seed": args.seed, "path_steps": n * args.paths * 8,
        "B_simulate_sampled_ms_hip_events": summary(B),
        "solve_ms_hip_events": summary(S),
        "B_inclusive_wall_ms": summary(B1),
        "A_handles_host_sampling_wall_ms_subset": summary(A),
        "A_subset_instances": picked,
        "A_scaled_to_all_instances_ms": (statistics.median(A) * n / len(picked)) if A else None,
        "A_is_scaled_from_a_subset": bool(A) and len(picked) < n,
        "largest_rel_gap_sim_vs_op": float(rel.max()),
    }
    with open(args.json, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in res.items() if k not in ("workload", "device")}))


if __name__ == "__main__":
    main()
