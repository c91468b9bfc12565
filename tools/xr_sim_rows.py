"""What the validation steps of cash.singleItem.CashConstraintXR.main cost on the device, beside its solve.

The driver's own instance (tests/cases.py: xr_main_instance -- four periods, Gamma(8, rate 2) demand truncated at the 0.99
quantile, price 4, unit cost 2, salvage 1, inventory 0 .. 500, integer cash -100 .. 2000, start (x, R) = (0, 30)) and its own
10 000 latin-hypercube paths (CashConstraintXR.java:133), drawn from the handle's pmf tiles:

    solve -> simulateSDPGivenSamplNum -> RecursionG.getOptY -> simulateAStar

Medians and ranges of --samples samples, after one warm-up each:
  a   the solve sweep (sdpgpu_stats: solve_ms, HIP events)
  b   the table rollout: sdpgpu_xr_simulate with levels NULL -- kernel_ms: the rollout and both reductions
  c   the a* rollout with the levels RecursionG returns -- kernel_ms
and, once: the wall time of RecursionG.getOptY on the host, the a* levels, the three values and the a* gap to V_1.
No ratio is set in advance: nobody has measured this; the expectation is only that (b) and (c) are short against (a).

    python tools/xr_sim_rows.py [--samples 7] [--paths 10000] [--seed 12345] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
import stochastic_inventory_amd as sia  # noqa: E402


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--paths", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "xr_sim_rows.json"))
    args = ap.parse_args()
    import torch
    n = max(args.samples, 1)
    w = cases.xr_main_instance()
    f = w.functor
    rec = sia.CashRecursionXR(w.direction, w.pmf, functor=f, discountFactor=f.discountFactor, device=0)
    ini = sia.CashStateXR(1, f.iniInventory, f.iniCash, f.variCost)
    v1 = rec.getExpectedValue(ini)  # solves
    eng = rec.engine
    A = []
    for _ in range(n):
        eng.solve(sync=True)
        A.append(eng.stats().solve_ms)
    x, R = float(f.iniInventory), float(f.iniCash)
    first_b = eng.xr_simulate(args.paths, args.seed, x, R)[0]  # warm-up
    B = []
    for _ in range(n):
        res = eng.xr_simulate(args.paths, args.seed, x, R)[0]
        B.append(res.kernel_ms)
        assert res.mean == first_b.mean, "the table rollout is not reproducible"
    t0 = time.perf_counter()
    optY = sia.RecursionG(w.pmf, None, f.price, f.variCost, f.depositeRate, f.salvageValue).getOptY()
    opt_s = time.perf_counter() - t0
    first_c = eng.xr_simulate(args.paths, args.seed, x, R, optY, vari_cost=f.variCost)[0]  # warm-up
    Cs = []
    for _ in range(n):
        res = eng.xr_simulate(args.paths, args.seed, x, R, optY, vari_cost=f.variCost)[0]
        Cs.append(res.kernel_ms)
        assert res.mean == first_c.mean, "the a* rollout is not reproducible"
    final = R + v1
    out = {
        "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": n, "seed": args.seed,
        "workload": "CashConstraintXR.main: T = 4, Gamma(8, 2) at the 0.99 quantile, price 4, cost 2, salvage 1, 501 x 2101 states",
        "paths": args.paths, "final_value": final, "opt_y": [float(a) for a in optY], "opt_y_host_wall_s": opt_s,
        "sim_table_plus_ini_r": first_b.mean + R, "sim_a_star_plus_ini_r": first_c.mean + R,
        "gap_a_star_percent": (final - (first_c.mean + R)) * 100 / final,
        "a_solve_ms_hip_events": summary(A),
        "b_table_rollout_kernel_ms": summary(B),
        "c_a_star_rollout_kernel_ms": summary(Cs),
    }
    rec.engine.close()
    print(json.dumps({k: (v["median"] if isinstance(v, dict) and "median" in v else v) for k, v in out.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
