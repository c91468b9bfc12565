"""The sweep of workforce.WorkforceTesting.main (216 instances, workloads.workforce_testing_sweep) solved two ways, in one process:

  A   one separable handle after another (SdpEngine, kernel = SDPGPU_KERNEL_SEPARABLE): 216 x 16 launches -- the existing path
  B   one batch solve (StaffBatch): 16 launches for all instances

B runs first and stays alive; the handles of A are created, solved, compared and destroyed in chunks (a handle keeps pmfs[t]
once per period on the host: 64 MB each).  Per sample, A is the SUM over the 216 handles of sdpgpu_stats.solve_ms (HIP events
around each handle's own 16 launches: the gaps between handles are NOT counted, which favours A) and, beside it, the wall time
of the loop; B is sdpgpu_batch_stats.solve_ms.  --samples samples each after one warm-up solve, median and range.  Then A' / B':
wall time including create, table upload, the first solve and the read-out of V_1(0), measured once each.  Then every one of
the 216 x 8 value and policy tables of A against B, bit for bit.  Required: B's range below A's, and all tables equal.

    python tools/staff_batch_rows.py [--samples 7] [--chunk 27] [--json profiles/staff_batch_rows.json]
    python tools/staff_batch_rows.py --batch-only --lib path/to/libsdpgpu.so     # B alone, on another build of the library

--lib loads another build of the library, e.g. one made with build.build(extra_flags=["-DSDP_STAFF_BATCH_R=1"]) (instance blocks
off) or other read-ahead depths (-DSDP_STAFF_BATCH_U1=.., -DSDP_STAFF_BATCH_UR=..): how the kept form of the G kernel was chosen.
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

import stochastic_inventory_amd as sia  # noqa: E402
from stochastic_inventory_amd import workloads  # noqa: E402


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def make_batch(sweep):
    rec = sia.StaffRecursionBatch([w.functor for w in sweep], [w.level_pmf for w in sweep], sweep[0].T, device=0)
    return rec


def handle(w):
    d = w.desc()
    d.kernel, d.device = sia._abi.KERNEL_SEPARABLE, 0
    return sia.SdpEngine(d, None, w.overhead(), level_pmf=w.level_pmf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=27, help="handles alive at a time")
    ap.add_argument("--instances", type=int, default=0, help="only the first N instances of the sweep (0: all 216)")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--lib", default="", help="another build of libsdpgpu.so")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "staff_batch_rows.json"))
    args = ap.parse_args()
    if args.lib:
        sia._abi.LIB_PATH = os.path.abspath(args.lib)
    import torch
    n = max(args.samples, 1)
    sweep = workloads.workforce_testing_sweep()
    if args.instances:
        sweep = sweep[:args.instances]
    N, T = len(sweep), sweep[0].T
    out = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": n, "instances": N,
           "library": args.lib or "the tree's own", "build_id": sia._abi.load().sdpgpu_build_id().decode()}

    # ---- B: one batch ----
    t0 = time.perf_counter()
    rec = make_batch(sweep)
    b = rec.batch
    b.solve(sync=True)
    ini_b = b.initial()
    out["B_prime_wall_ms"] = (time.perf_counter() - t0) * 1e3
    b_ms, b_wall = [], []
    for _ in range(n):
        t1 = time.perf_counter()
        b.solve(sync=True)
        b_wall.append((time.perf_counter() - t1) * 1e3)
        b_ms.append(b.stats().solve_ms)
    st = b.stats()
    plans = [b.plan(t) for t in range(1, T + 1)]
    out["B"] = {"solve_ms": summary(b_ms), "wall_ms": summary(b_wall), "period_launches": st.period_launches,
                "cells_evaluated": st.cells_evaluated, "pool_tables": rec.num_tables,
                "plan": [{"period": t + 1, "tables": p.tables, "r": p.r, "u": p.u, "blocks": p.blocks, "g_tasks": p.g_tasks,
                          "scan_workgroups": p.scan_workgroups, "levels": p.levels, "states": p.states, "longest_row": p.longest_row}
                         for t, p in enumerate(plans)]}
    b.set_profiling(True)
    b.solve(sync=True)
    out["B"]["period_ms"] = [b.period_ms(t) for t in range(1, T + 1)]
    b.set_profiling(False)
    print(json.dumps({"B_solve_ms": out["B"]["solve_ms"], "B_prime_wall_ms": out["B_prime_wall_ms"], "r": [p.r for p in plans]}), flush=True)

    if not args.batch_only:
        # ---- A: handle after handle, in chunks ----
        a_ms, a_wall = [0.0] * n, [0.0] * n
        a_prime = 0.0
        cells = 0
        unequal = []
        ini_unequal = 0
        for c0 in range(0, N, args.chunk):
            part = sweep[c0:c0 + args.chunk]
            t0 = time.perf_counter()
            engs = []
            for k, w in enumerate(part):
                e = handle(w)
                e.solve(sync=True)
                v1, p1 = e.values(1), e.policy(1)  # (period 1 holds the one state iniStaffNum)
                if v1[0] != ini_b[0][c0 + k] or p1[0] != ini_b[1][c0 + k]:
                    ini_unequal += 1
                engs.append(e)
            a_prime += (time.perf_counter() - t0) * 1e3
            for s in range(n):
                t1 = time.perf_counter()
                ms = 0.0
                for e in engs:
                    e.solve(sync=True)
                    ms += e.stats().solve_ms
                a_wall[s] += (time.perf_counter() - t1) * 1e3
                a_ms[s] += ms
            for k, e in enumerate(engs):
                cells += e.stats().cells_evaluated
                for t in range(1, T + 1):
                    if not (np.array_equal(e.values(t), b.values(c0 + k, t)) and np.array_equal(e.policy(t), b.policy(c0 + k, t))):
                        unequal.append([c0 + k, t])
                e.close()
            print(json.dumps({"handles_done": c0 + len(part), "tables_unequal": len(unequal)}), flush=True)
        out["A_prime_wall_ms"] = a_prime
        out["A"] = {"solve_ms": summary(a_ms), "wall_ms": summary(a_wall), "launches": N * 2 * T, "cells_evaluated": cells}
        out["tables_compared"] = N * T
        out["tables_unequal"] = unequal
        out["initial_unequal"] = ini_unequal
        out["cells_agree"] = bool(cells == st.cells_evaluated)
        out["ratio_of_medians"] = out["A"]["solve_ms"]["median"] / out["B"]["solve_ms"]["median"]
        out["ranges_apart"] = bool(out["B"]["solve_ms"]["max"] < out["A"]["solve_ms"]["min"])
        out["ratio_prime"] = out["A_prime_wall_ms"] / out["B_prime_wall_ms"]
        print(json.dumps({"A_solve_ms": out["A"]["solve_ms"], "A_wall_ms": out["A"]["wall_ms"], "A_prime_wall_ms": a_prime,
                          "ratio": out["ratio_of_medians"], "ranges_apart": out["ranges_apart"], "ratio_prime": out["ratio_prime"],
                          "tables_unequal": len(unequal), "initial_unequal": ini_unequal, "cells_agree": out["cells_agree"]}), flush=True)
    rec.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
