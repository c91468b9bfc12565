"""What the cash drivers' structure analysis costs on the device, beside the solve it follows.

The 30 instances of SingleCrossTesting.main (workloads.single_cross_testing: 10 demand patterns x 3 prices, T = 2, K = 10, v = 1,
inventory 0 .. 200 x cash -100 .. 1500, window levels 0 .. 30 x cash 0 .. 40) and CheckFG.main's instance (workloads.check_fg:
T = 3, inventory 0 .. 500 x cash -100 .. 2000, window 0 .. 100 x 0 .. 90), each through

    solve -> sdpgpu_cash_structure (source 0, every request: G, GA, GB, F, H, GB - GA - K, F - G - v j and the seven checks)

Per instance: the verdicts, the solve sweep (sdpgpu_stats: solve_ms, HIP events) and the structure call's kernels (kernel_ms: HIP
events around the G launch, the derived tables and the checks), medians and ranges of --samples samples after one warm-up each.
Then ONE whole-grid G table of SingleCrossTesting's grid (201 levels x 1601 cash points) of the first instance: the kernels of a
source-0 call asking for F - G - v j alone (the G launch, the gather of F and one elementwise kernel), the wall time of
sdpgpu_cash_g_table (launch, copy of 2.5 MB to the host, synchronise), next to the handle's period-1 kernel time.
No speed threshold is set: nobody has measured this.

    python tools/cash_structure_rows.py [--samples 7] [--json PATH]
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
from stochastic_inventory_amd import _abi, workloads  # noqa: E402


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def verdict_rows(res):
    return {k: {"holds": bool(v[0]), "i": v[1], "j": v[2], "i1": v[3], "j1": v[4], "value": v[5]} for k, v in res.verdicts.items()}


def run_instance(w, n):
    d = w.desc()
    d.device = 0
    x_lo, x_hi, c_lo, c_hi = w.window
    with sia.SdpEngine(d, w.pmf, w.overhead()) as eng:
        eng.solve(sync=True)  # warm-up
        solve = []
        for _ in range(n):
            eng.solve(sync=True)
            solve.append(eng.stats().solve_ms)
        first = eng.cash_structure(_abi.CSTRUCT_ALL, w.period, x_lo, x_hi, c_lo, c_hi, want_tables=False)  # warm-up
        struct = []
        for _ in range(n):
            res = eng.cash_structure(_abi.CSTRUCT_ALL, w.period, x_lo, x_hi, c_lo, c_hi, want_tables=False)
            struct.append(res.kernel_ms)
            assert [v[:5] for v in res.verdicts.values()] == [v[:5] for v in first.verdicts.values()], "the verdicts are not reproducible"
        return {"name": w.name, "states": eng.num_states(1), "window": list(w.window), "verdicts": verdict_rows(first),
                "solve_ms_hip_events": summary(solve), "structure_kernel_ms": summary(struct)}


def whole_grid(w, n):
    d = w.desc()
    d.device = 0
    f = w.functor
    win = (int(f.minInventoryState), int(f.maxInventoryState), int(f.minCashState), int(f.maxCashState))
    with sia.SdpEngine(d, w.pmf, w.overhead()) as eng:
        eng.set_profiling(True)
        eng.solve(sync=True)
        eng.solve(sync=True)
        period_ms = eng.period_ms(1)
        eng.cash_structure(_abi.CSTRUCT_FG, 1, *win, want_tables=False)  # warm-up
        kern, wall = [], []
        for _ in range(n):
            kern.append(eng.cash_structure(_abi.CSTRUCT_FG, 1, *win, want_tables=False).kernel_ms)
        g = eng.cash_g_table(_abi.CASH_G, 1, *win)  # warm-up
        for _ in range(n):
            t0 = time.perf_counter()
            eng.cash_g_table(_abi.CASH_G, 1, *win)
            wall.append((time.perf_counter() - t0) * 1e3)
        return {"name": w.name, "points": int(g.size), "shape_cash_x_levels": list(g.shape), "demand_points_period_1": len(w.pmf[0]),
                "g_f_fg_kernels_ms_hip_events": summary(kern), "cash_g_table_call_wall_ms": summary(wall),
                "period_1_kernel_ms_same_handle": period_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "cash_structure_rows.json"))
    args = ap.parse_args()
    import torch
    n = max(args.samples, 1)
    singles = workloads.single_cross_testing()
    rows = [run_instance(w, n) for w in singles]
    fg = run_instance(workloads.check_fg(), n)
    out = {
        "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": n,
        "requests": "mask 0x3ff: H, GB - GA - K, F - G - v j, checkSingleCrossing on H, checkNonIncreasing and checkNonDecreasing on each",
        "single_cross_testing": rows, "check_fg": fg, "whole_grid_g_table": whole_grid(singles[0], n),
        "single_crossing_holds": sum(r["verdicts"]["single_crossing"]["holds"] for r in rows),
    }
    print(json.dumps({"instances": len(rows), "single_crossing_holds": out["single_crossing_holds"],
                      "solve_ms_median_of_medians": statistics.median(r["solve_ms_hip_events"]["median"] for r in rows),
                      "structure_ms_median_of_medians": statistics.median(r["structure_kernel_ms"]["median"] for r in rows),
                      "check_fg_structure_ms": fg["structure_kernel_ms"]["median"],
                      "whole_grid_kernels_ms": out["whole_grid_g_table"]["g_f_fg_kernels_ms_hip_events"]["median"],
                      "period_1_kernel_ms": out["whole_grid_g_table"]["period_1_kernel_ms_same_handle"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
