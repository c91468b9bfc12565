"""What the simulation step of the workforce drivers' loop body costs on the device, beside the solve.

One handle of WorkforceTesting.main[0]'s shape (WorkforceTesting.java:43-107: T = 8, maxHireNum 1000, no clamp, one turnover
rate, a 1001-row binomial table), the loop body of WorkforceTesting.java:112-165 in Python:

    solve -> getOptTable -> FitsS(2**31 - 1, T).getSinglesS -> SimulatesS.simulatesS, twice

Medians and ranges of --samples samples, after one warm-up each, by HIP events, of

  a   the solve sweep (sdpgpu_stats: solve_ms)
  b   SimulatesS.simulatesS with TWO rules in one call on the default tree 10, 10, 10, 10, 1, 1, 1, 1 (10000 leaves): the rule
      fitted to the SDP table and a second one standing in for the MIP's (the fitted levels moved up by one) -- kernel_ms of the
      call: the rollout and both reductions of both rules
  c   SimulatesS.simulateTable on the same tree -- kernel_ms

No ratio is set in advance; the only expectation is that (b) is short against (a).

    python tools/staff_sim_rows.py [--samples 7] [--seed 12345] [--rate 0.1]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import stochastic_inventory_amd as sia  # noqa: E402
from stochastic_inventory_amd.pmf import staff_level_pmf  # noqa: E402


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "staff_sim_rows.json"))
    args = ap.parse_args()
    import torch
    T, n = 8, max(args.samples, 1)
    f = sia.StaffFunctor(fixCost=50, unitVariCost=20, salary=30, unitPenalty=50, minStaffNum=[40] * T, maxHireNum=1000, clampStaff=False,
                         iniStaffNum=0)
    rec = sia.StaffRecursion(pmf=np.repeat(staff_level_pmf([args.rate], 1001), T, axis=0), T=T, functor=f, device=0)
    initial = sia.StaffState(1, 0)
    opt = rec.getExpectedValue(initial)  # solves
    eng = rec.engine
    A = []
    for _ in range(n):
        eng.solve(sync=True)
        A.append(eng.stats().solve_ms)
    fitted = np.asarray(sia.FitsS(2 ** 31 - 1, T).getSinglesS(rec.getOptTable()), dtype=np.float64)
    rules = np.stack([fitted, fitted + 1.0])
    sim = sia.SimulatesS(rec, T, [args.rate] * T, seed=args.seed)
    means = sim.simulatesS(initial, rules)  # warm-up
    B = []
    for _ in range(n):
        again = sim.simulatesS(initial, rules)
        B.append(sim.last_results[0].kernel_ms)
        assert np.array_equal(again, means), "the rollout is not reproducible"
    table_mean = sim.simulateTable(initial)  # warm-up
    Cs = []
    for _ in range(n):
        assert sim.simulateTable(initial) == table_mean
        Cs.append(sim.last_results[0].kernel_ms)
    out = {
        "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": n, "seed": args.seed,
        "workload": f"WorkforceTesting.main[0]: T = {T}, maxHireNum 1000, no clamp, turnover rate {args.rate}, 1001-row table",
        "tree": sim.defaultSampleNums(), "leaves": int(np.prod(sim.defaultSampleNums())),
        "value_V1": opt, "levels_fitted": fitted.tolist(),
        "sim_fitted_rule": float(means[0]), "gap_fitted_percent": (float(means[0]) - opt) * 100 / opt,
        "sim_second_rule": float(means[1]), "sim_table": table_mean, "gap_table_percent": (table_mean - opt) * 100 / opt,
        "a_solve_ms_hip_events": summary(A),
        "b_simulatesS_two_rules_kernel_ms": summary(B),
        "c_simulateTable_kernel_ms": summary(Cs),
    }
    rec.close()
    print(json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in out.items()}), flush=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
