"""What the workforce family's G(y) rows and their K-convexity check cost on the device, beside the solve they inspect.

  (a) workloads.workforce_planning() (WorkforcePlanning.main: T = 3, 601 levels, hires 0 .. 500, clamped): the three rows
      G_1 .. G_3 over 0 .. 600 (three sdpgpu_staff_gy calls) and ONE CheckKConvexity.check(yG, fixCost) on G_1
      (sdpgpu_staff_check_convexity), each beside that handle's solve.
  (b) workloads.workforce_testing_sweep() (WorkforceTesting.main: 216 instances, T = 8): all 216 x 8 rows in the ONE launch the
      first sdpgpu_batch_staff_gy after a solve makes, beside the batch's solve measured in the same run.
  (c) the one-thread host entry sdpgpu_staff_gy_host on the rows of (a) and on one instance's eight rows of (b) (wall clock).

The solves are the library's own HIP-event times (sdpgpu_stats / sdpgpu_batch_stats: solve_ms).  The ABI records no event pair
around a G or check call, and each is synchronous (it returns once its stream has drained), so its figure is the WALL time of the
call: the device block, the uploads of the row records, the launch, the copy back -- an upper bound on its kernels.  Medians and
ranges of --samples samples after one warm-up each, in one process.  No bar is set: nobody has measured this before.

    python tools/staff_gy_rows.py [--samples 7] [--json PATH] [--instances N]
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
from stochastic_inventory_amd import workloads  # noqa: E402


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def timed(fn):
    """Wall time of a synchronous call in ms (it returns once its stream has drained), and what it returned."""
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def host_rows(lib, functor, table2d, T, values, x_los, min_staff):
    """Wall time of the host entry for the rows G_1 .. G_T over every level of the table."""
    import ctypes as C
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rows = table2d.shape[0]
    out = np.empty(rows)
    t0 = time.perf_counter()
    for t in range(1, T + 1):
        vn = values[t + 1] if t < T else None  # (values and x_los are keyed by their own period)
        rc = lib.sdpgpu_staff_gy_host(float(functor.unitVariCost), float(functor.salary), float(functor.unitPenalty), int(min_staff[t - 1]),
                                      dp(table2d), None, rows, table2d.shape[1], None if vn is None else dp(vn), int(x_los[t + 1]) if t < T else 0,
                                      0 if vn is None else len(vn), 1 if functor.clampStaff else 0, int(functor.minX), int(functor.maxX), 0, rows, dp(out))
        assert rc == 0, lib.sdpgpu_batch_last_error(None).decode()
    return (time.perf_counter() - t0) * 1e3


def planning(n):
    w = workloads.workforce_planning()
    d = w.desc()
    d.device = 0
    with sia.SdpEngine(d, None, w.overhead(), level_pmf=w.level_pmf) as eng:
        eng.solve(sync=True)
        solve = []
        for _ in range(n):
            eng.solve(sync=True)
            solve.append(eng.stats().solve_ms)
        rows3 = lambda: [eng.staff_gy(t, 0, 600) for t in (1, 2, 3)]  # noqa: E731
        check = lambda: eng.staff_check_convexity(0, "gy", 1, 0, 600)  # noqa: E731
        rows3(), check()
        g_ms = [timed(rows3)[0] for _ in range(n)]
        c_ms, verdict = [], None
        for _ in range(n):
            ms, verdict = timed(check)
            c_ms.append(ms)
        values = {t: eng.values(t) for t in (2, 3)}
        x_los = {t: eng.grid(t)[0] for t in (2, 3)}
        host = [host_rows(eng._lib, w.functor, np.ascontiguousarray(w.level_pmf[0]), 3, values, x_los, w.functor.minStaffNum) for _ in range(n)]
    s, g, c = statistics.median(solve), statistics.median(g_ms), statistics.median(c_ms)
    return {"name": w.name, "levels": 601, "solve_ms_hip_events": summary(solve), "three_g_rows_call_wall_ms": summary(g_ms),
            "one_check_call_wall_ms": summary(c_ms), "check_holds": bool(verdict["holds"]), "three_g_rows_over_solve": g / s,
            "one_check_over_solve": c / s, "host_entry_three_rows_wall_ms": summary(host)}


def sweep(n, instances):
    ws = workloads.workforce_testing_sweep()[:instances]
    with sia.StaffRecursionBatch([w.functor for w in ws], [w.level_pmf for w in ws], device=0) as rb:
        b = rb.batch
        b.solve(sync=True)
        b.staff_gy(0, 1, 0, 0)
        solve, fill = [], []
        for _ in range(n):
            b.solve(sync=True)  # (drops the kept rows: the next request forms them all again)
            solve.append(b.stats().solve_ms)
            fill.append(timed(lambda: b.staff_gy(0, 1, 0, 0))[0])
        kept = [timed(lambda: b.staff_gy(len(ws) - 1, 8, 0, 1000))[0] for _ in range(n)]
        values = {t: b.values(0, t) for t in range(2, 9)}
        x_los = {t: b.grid(0, t)[0] for t in range(2, 9)}
        host = [host_rows(b._lib, ws[0].functor, np.ascontiguousarray(ws[0].level_pmf[0]), 8, values, x_los, ws[0].functor.minStaffNum) for _ in range(n)]
    s, f = statistics.median(solve), statistics.median(fill)
    return {"instances": len(ws), "periods": 8, "rows": len(ws) * 8, "levels_per_row": 1001, "pool_tables": rb.num_tables,
            "batch_solve_ms_hip_events": summary(solve), "all_rows_first_request_wall_ms": summary(fill), "all_rows_over_solve": f / s,
            "kept_row_request_wall_ms": summary(kept), "host_entry_eight_rows_of_one_instance_wall_ms": summary(host)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--instances", type=int, default=216)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "staff_gy_rows.json"))
    args = ap.parse_args()
    import torch
    n = max(args.samples, 1)
    out = {"device": torch.cuda.get_device_name(0), "samples": n, "workforce_planning": planning(n),
           "workforce_testing_sweep": sweep(n, args.instances)}
    a, b = out["workforce_planning"], out["workforce_testing_sweep"]
    print(json.dumps({"planning_solve_ms": a["solve_ms_hip_events"]["median"], "planning_three_rows_ms": a["three_g_rows_call_wall_ms"]["median"],
                      "planning_check_ms": a["one_check_call_wall_ms"]["median"], "planning_rows_over_solve": a["three_g_rows_over_solve"],
                      "planning_check_over_solve": a["one_check_over_solve"], "planning_host_ms": a["host_entry_three_rows_wall_ms"]["median"],
                      "sweep_solve_ms": b["batch_solve_ms_hip_events"]["median"], "sweep_all_rows_ms": b["all_rows_first_request_wall_ms"]["median"],
                      "sweep_rows_over_solve": b["all_rows_over_solve"], "sweep_host_one_instance_ms": b["host_entry_eight_rows_of_one_instance_wall_ms"]["median"]}),
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
