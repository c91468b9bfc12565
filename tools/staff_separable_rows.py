"""The workforce family's opt-in separable mode beside its cell-by-cell kernels: the solve sweep and every period of it.

Two shapes, each solved by an AUTO handle (the cell-by-cell kernels launch_staff chooses: the yardstick) and by a
kernel = SDPGPU_KERNEL_SEPARABLE handle (one G(y) row per period, then the scan):

  WorkforceTesting.main[0]   WorkforceTesting.java:43-107: T = 8, maxHireNum 1000, no clamp, a 1001-row binomial table
  WorkforcePlanning.main     WorkforcePlanning.java:33-50: T = 3, staff 0..600, hires 0..500, clamped, a 601-row table

Per handle: solve_ms of --samples sweeps after one warm-up (sdpgpu_stats, HIP events), then the same number of profiled sweeps
for sdpgpu_period_ms of every period.  Between the two handles: the worst relative difference of the value tables and the
number of states whose hire count differs.  No ratio is set in advance; what is required is that the separable median lies
below the cell-by-cell minimum and the two ranges do not overlap.

    python tools/staff_separable_rows.py [--samples 7] [--json profiles/staff_separable_rows.json]
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


def sweep(rec, T, n):
    """-> (solve_ms summary, per-period summaries, value tables, policies) of one StaffRecursion."""
    eng = rec.engine
    eng.solve(sync=True)  # warm-up: lazy allocations, table uploads
    solve = []
    for _ in range(n):
        eng.solve(sync=True)
        solve.append(eng.stats().solve_ms)
    eng.set_profiling(True)
    eng.solve(sync=True)
    per = [[] for _ in range(T)]
    for _ in range(n):
        eng.solve(sync=True)
        for t in range(1, T + 1):
            per[t - 1].append(eng.period_ms(t))
    eng.set_profiling(False)
    kernel_used = eng.stats().kernel_used
    return (summary(solve), [summary(p) for p in per], [eng.values(t) for t in range(1, T + 1)],
            [eng.policy(t) for t in range(1, T + 1)], kernel_used)


def shape_rows(name, functor, table, T, n):
    out = {"workload": name}
    tables = {}
    for label, separable in (("cell_by_cell", False), ("separable", True)):
        rec = sia.StaffRecursion(pmf=table, T=T, functor=functor, device=0, separable=separable)
        solve, per, V, pol, used = sweep(rec, T, n)
        rec.close()
        out[label] = {"kernel_used": used, "solve_ms": solve, "period_ms": per}
        tables[label] = (V, pol)
    (V0, p0), (V1, p1) = tables["cell_by_cell"], tables["separable"]
    worst = 0.0
    for a, b in zip(V1, V0):
        r = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
        r[(a == 0) & (b == 0)] = 0.0
        worst = max(worst, float(r.max()))
    out["states"] = int(sum(len(v) for v in V0))
    out["worst_relative_value_difference"] = worst
    out["states_hiring_differently"] = int(sum(np.count_nonzero(a != b) for a, b in zip(p1, p0)))
    cc, sp = out["cell_by_cell"]["solve_ms"], out["separable"]["solve_ms"]
    out["ratio_of_medians"] = cc["median"] / sp["median"]
    out["ranges_apart"] = bool(sp["max"] < cc["min"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "staff_separable_rows.json"))
    args = ap.parse_args()
    import torch
    n = max(args.samples, 1)
    T = 8
    testing = sia.StaffFunctor(fixCost=50, unitVariCost=20, salary=30, unitPenalty=50, minStaffNum=[40] * T, maxHireNum=1000,
                               clampStaff=False, iniStaffNum=0)
    rows = [shape_rows(f"WorkforceTesting.main[0]: T = {T}, maxHireNum 1000, no clamp, turnover rate {args.rate}, 1001-row table",
                       testing, np.repeat(staff_level_pmf([args.rate], 1001), T, axis=0), T, n)]
    planning = sia.StaffFunctor(fixCost=100, unitVariCost=10, salary=20, unitPenalty=80, minStaffNum=[40, 40, 40], maxHireNum=500,
                                minX=0, maxX=600, clampStaff=True, iniStaffNum=0)
    rows.append(shape_rows("WorkforcePlanning.main: T = 3, staff 0..600, hires 0..500, clamped, turnover rate 0.5, 601-row table",
                           planning, staff_level_pmf([0.5, 0.5, 0.5], 601), 3, n))
    out = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": n,
           "yardstick": "cell_by_cell: the kernels of csrc/sdp_staff.hpp as launch_staff chooses them (kernel AUTO)", "rows": rows}
    for r in rows:
        print(json.dumps({"workload": r["workload"], "cell_by_cell_solve_ms": r["cell_by_cell"]["solve_ms"]["median"],
                          "separable_solve_ms": r["separable"]["solve_ms"]["median"], "ratio": r["ratio_of_medians"],
                          "ranges_apart": r["ranges_apart"], "worst_rel": r["worst_relative_value_difference"],
                          "hire_differently": r["states_hiring_differently"], "states": r["states"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
