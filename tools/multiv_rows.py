"""What cash.multiItem.MultiItemYR.main's solve costs on the device (sdpgpu_multiv_solve, DESIGN 4 "V / Pi recursion").

The driver's own instance (MultiItemYR.java:45-98): T = 2, prices {5, 10}, unit costs {1, 2}, salvage half the cost, no
deposit, Qbound 50, start (0, 0, cash 10), bounds inventory 0 .. 200 and cash 0 .. 10000, TRUNC10 rounding, gamma demands
GammaDist(20 * 10, 10) and GammaDist(10 * 1, 1) through the project's GammaDist, tiled as GetPmfMulti.getPmf does for gammas
(GetPmfMulti.java:72-105: supports (int) inverseF(1 - q) .. (int) inverseF(q) at q = 0.9999, step 1, cdf differences over
(2 q - 1)^2).

  a   gpu_ms of sdpgpu_multiv_solve (HIP events around the forward and the backward pass), --samples samples after one
      warm-up: median and range; states / distinct R / Pi entries per period, cells, cells per second
  b   once: the host twin (tests/multiv_twin.py, the memoised restatement of CashRecursionV) on a reduced box (--host-q), its
      wall time per (Pi entry, demand pair) cell scaled to the cells of (a); V_1, the action and y* of the reduced box are
      compared with the device's on that box, bit for bit
No time is set in advance: nobody has measured this workload.

    python tools/multiv_rows.py [--samples 7] [--host-q 6] [--json PATH]
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

import numpy as np  # noqa: E402

import multiv_twin as twin  # noqa: E402
import stochastic_inventory_amd as sia  # noqa: E402


def gamma_joint_pmf(d1, d2, q=0.9999, step=1):
    """GetPmfMulti.getPmf for two GammaDists (GetPmfMulti.java:72-105)."""
    lb = [int(d.inverseF(1 - q)) for d in (d1, d2)]
    ub = [int(d.inverseF(q)) for d in (d1, d2)]
    n1, n2 = int((ub[0] - lb[0] + 1) / step), int((ub[1] - lb[1] + 1) / step)
    psum = (2 * q - 1) * (2 * q - 1)
    rows = []
    for i in range(n1):
        for j in range(n2):
            a, b = float(lb[0] + i * step), float(lb[1] + j * step)
            rows.append([a, b, (d1.cdf(a + 0.5 * step) - d1.cdf(a - 0.5 * step)) * (d2.cdf(b + 0.5 * step) - d2.cdf(b - 0.5 * step)) / psum])
    return np.array(rows)


def yr_main_instance(q_bound=50):
    tile = gamma_joint_pmf(sia.GammaDist(20 * 10, 10), sia.GammaDist(10 * 1, 1))
    return dict(T=2, q_bound=q_bound, rounding="trunc10", price=[5, 10], vari_cost=[1, 2], sal_price=[0.5, 1.0], deposit_rate=0.0,
                ini_cash=10, ini_i1=0, ini_i2=0, min_inventory=0, max_inventory=200, min_cash=0, max_cash=10000, pmf=[tile, tile])


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--host-q", type=int, default=6)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "multiv_rows.json"))
    args = ap.parse_args()
    import torch
    n = max(args.samples, 1)
    kw = yr_main_instance()
    runs = [sia.multiv_solve(**kw) for _ in range(n + 1)][1:]
    first = runs[0]
    assert all((r.value, r.action, r.yStar, r.alpha) == (first.value, first.action, first.yStar, first.alpha) for r in runs)
    ms = [r.gpu_ms for r in runs]
    # the host twin on a reduced box, against the device on the same box
    small = yr_main_instance(args.host_q)
    t0 = time.perf_counter()
    tw, value, action, ystar = twin.drive(small)
    host_s = time.perf_counter() - t0
    host_cells = sum(len(small["pmf"][k[0] - 1]) for k in tw.cacheValuesPai)
    dev = sia.multiv_solve(**small)
    assert (dev.value, tuple(dev.action), tuple(dev.yStar)) == (value, action, ystar), "the twin and the device disagree"
    med = statistics.median(ms)
    out = {
        "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": n,
        "workload": "MultiItemYR.main: T = 2, GammaDist(200, 10) x GammaDist(10, 1) at the 0.9999 quantile, Qbound 50, cash 10",
        "pairs_per_period": [int(len(t)) for t in kw["pmf"]],
        "value": first.value, "action": first.action, "y_star": first.yStar, "constrained": first.constrained, "alpha": first.alpha,
        "states_per_period": first.statesPerPeriod, "r_per_period": first.rPerPeriod, "entries_per_period": first.entriesPerPeriod,
        "cells": first.cells, "a_solve_gpu_ms_hip_events": summary(ms), "cells_per_second": first.cells / (med * 1e-3),
        "host_twin_q_bound": args.host_q, "host_twin_wall_s": host_s, "host_twin_cells": host_cells,
        "host_twin_scaled_to_cells_s": host_s / host_cells * first.cells,
        "host_twin_equals_the_device_on_its_box": True,
    }
    print(json.dumps({k: (v["median"] if isinstance(v, dict) and "median" in v else v) for k, v in out.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
