"""What validating the solve of cash.multiItem.MultiItemCashXR.main costs on the device, beside the solve itself.

The driver's own instance (tests/multicash_cases.py: xr_main_instance -- two periods, Poisson demands with means {20, 10}
truncated at the 0.99 quantile: 352 demand pairs a period, prices {5, 10}, unit costs {1, 2}, Qbound 50, start (0, 0, R = 0);
71 767 period-2 states) and the 10 000 paths CashSimulationMultiXR rolls (MultiItemCashUniform.java:151-153), drawn from the
joint tiles ("Two-product rollout"):

    solve with the memo read back -> policy object (hash table over the memo) -> sampled rollout

Medians and ranges of --samples samples, after one warm-up each:
  a   the solve (gpu_ms of sdpgpu_multixr_solve: HIP events around the forward and backward passes)
  b   sdpgpu_multicash_policy_create: HIP events on the null stream around the call -- the copies of the records and tiles,
      the slot array's fill and multi_policy_insert_kernel -- and its wall time
  c   sdpgpu_multi_policy_simulate_sampled, 10 000 latin-hypercube paths -- kernel_ms: the rollout and both reductions
and, once: the host route -- the same paths walked state by state through CashRecursionMultiXR's read-back memo
(_MultiRecursionBase._lookup) and the lambdas of tests/multi_sim_twin.py, timed on --host-paths paths and scaled to --paths --
its path sums against the device's, and |mean + iniR - finalValue| in standard errors sqrt(m2 / n) / sqrt(n).
No time is set in advance: nobody has measured this.

    python tools/multi_sim_rows.py [--samples 7] [--paths 10000] [--host-paths 1000] [--seed 12345] [--json PATH]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multicash_cases  # noqa: E402
import multi_sim_twin as twin  # noqa: E402
import stochastic_inventory_amd as sia  # noqa: E402
from stochastic_inventory_amd import multiitem  # noqa: E402


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--paths", type=int, default=10000)
    ap.add_argument("--host-paths", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "multi_sim_rows.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    n = max(args.samples, 1)
    kw = multicash_cases.xr_main_instance()
    functor = {k: v for k, v in kw.items() if k not in ("pmf", "ini_cash", "ini_i1", "ini_i2", "T", "discount")}
    rec = sia.CashRecursionMultiXR(kw["discount"], kw["pmf"], TLength=kw["T"], functor=functor)
    ini = sia.CashStateMultiXR(1, kw["ini_i1"], kw["ini_i2"], kw["ini_cash"])
    v1 = rec.getExpectedValue(ini)  # solves, reads the memo back
    final = kw["ini_cash"] + v1
    rows = rec.result.table
    A = [multiitem.multixr_solve(0.0, **kw).gpu_ms for _ in range(n + 1)][1:]
    B, B_wall = [], []
    for i in range(n + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        pol = rec.policy()
        e1.record()
        torch.cuda.synchronize()
        if i:
            B.append(e0.elapsed_time(e1))
            B_wall.append((time.perf_counter() - t0) * 1e3)
        if i < n:
            pol.close()
    first, sums, valid = pol.simulate_sampled(args.paths, args.seed, want_sums=True)  # warm-up
    assert valid.all(), "a drawn path left the memo"
    Cs = []
    for _ in range(n):
        res = pol.simulate_sampled(args.paths, args.seed)
        Cs.append(res.kernel_ms)
        assert res.mean == first.mean and res.m2 == first.m2, "the rollout is not reproducible"
    # the host route: getAction by _lookup, the lambdas in Python
    m = min(args.host_paths, args.paths)
    d1, d2, _ = pol.sample(args.paths, args.seed)
    pol.close()
    immediateValue, stateTransition = twin.lambdas("multixr", kw, 0.0)
    host = np.empty(m)
    t0 = time.perf_counter()
    for p in range(m):
        state, total = twin.initial_state(kw), 0.0
        for t in range(kw["T"]):
            y = rec.getAction(sia.CashStateMultiXR(state[0], state[1], state[2], state[5]))
            d = (float(d1[p, t]), float(d2[p, t]))
            total += kw["discount"] ** t * immediateValue(state, y, d)
            state = stateTransition(state, y, d)
        host[p] = total
    host_s = time.perf_counter() - t0
    assert (host.view(np.uint64) == sums[:m].view(np.uint64)).all(), "the host route and the device disagree"
    se = math.sqrt(first.m2 / args.paths) / math.sqrt(args.paths)
    out = {
        "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": n, "seed": args.seed,
        "workload": "MultiItemCashXR.main: T = 2, Poisson {20, 10} at the 0.99 quantile (352 pairs a period), Qbound 50",
        "memo_rows": int(len(rows)), "paths": args.paths, "final_value": final, "sim_plus_ini_r": first.mean + kw["ini_cash"],
        "standard_error": se, "distance_in_standard_errors": abs(first.mean + kw["ini_cash"] - final) / se,
        # GetPmfMulti's truncated tile is not normalised: the recursion weighs with it as it is, the sampler's running sum
        # saturates at 1 -- the distance above carries that, not sampling error alone
        "tile_probability_sums": [float(np.sum(np.asarray(t)[:, 2])) for t in kw["pmf"]],
        "a_solve_gpu_ms_hip_events": summary(A),
        "b_create_ms_hip_events": summary(B), "b_create_wall_ms": summary(B_wall),
        "c_rollout_kernel_ms": summary(Cs),
        "host_route_paths": m, "host_route_wall_s": host_s, "host_route_scaled_to_paths_s": host_s * args.paths / m,
        "host_route_sums_equal_the_device_bit_for_bit": True,
    }
    print(json.dumps({k: (v["median"] if isinstance(v, dict) and "median" in v else v) for k, v in out.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
