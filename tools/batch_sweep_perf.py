"""CLSPTesting's 540 instances (workloads.clsp_testing_sweep): the looped single-handle path against the batched solve.

One process, one stream of its own, HIP events beside a host clock.

  A   540 pre-created SdpEngines (pmfs set, one warm-up solve each); timed: 540 x solve(sync=False) + one synchronize
  A'  the same including create / set_pmf / read-out of V_1(ini) and its action: what a driver's sweep loop pays
  B   SdpBatch.solve
  B'  SdpBatch including create / set_pmf / initial()

A sample is as many back-to-back sweeps as fill half a second, divided by their number; samples alternate A, B, A, B, ...
Before anything is timed the two paths are compared bit for bit (initial values and actions, all period-1 tables).

    python tools/batch_sweep_perf.py [--samples 7] [--inclusive-samples 3] [--patterns 1,7] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import stochastic_inventory_amd as sia
from stochastic_inventory_amd import workloads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--inclusive-samples", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="least length of a timed window, seconds")
    ap.add_argument("--patterns", default="", help="subset of the demand patterns 1..10 (default: all: 540 instances)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "batch_clsp_testing_sweep.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it has no CPU path")
    torch.cuda.set_device(0)
    patterns = tuple(int(x) for x in args.patterns.split(",")) if args.patterns else None
    ws = workloads.clsp_testing_sweep(patterns)
    n = len(ws)
    stream = torch.cuda.Stream()
    sptr = stream.cuda_stream

    def descs():
        out = [w.desc() for w in ws]
        for d in out:
            d.device = 0
        return out

    def make_engines():
        engines = []
        for w, d in zip(ws, descs()):
            e = sia.SdpEngine(d, w.pmf)
            e.set_stream(sptr)
            engines.append(e)
        return engines

    def make_batch(profiling=False):
        b = sia.SdpBatch(descs(), [w.pmf for w in ws])
        b.set_stream(sptr)
        b.set_profiling(profiling)
        return b

    def timed(fn, sweeps):
        """(host ms, device ms) per sweep of `sweeps` back-to-back calls of fn, which only enqueues."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        for _ in range(sweeps):
            fn()
        e1.record(stream)
        stream.synchronize()
        host = (time.perf_counter() - t0) * 1e3 / sweeps
        return host, e0.elapsed_time(e1) / sweeps

    # ---- the two paths, warmed up, and their results compared at the size that is timed ------------------------------
    engines = make_engines()
    for e in engines:
        e.solve(sync=False)
    stream.synchronize()
    batch = make_batch()
    batch.solve(sync=True)
    bst = batch.stats()
    ini_v, ini_k = batch.initial()
    ix = [int((w.functor.iniInventory - w.functor.minInventory) / w.functor.stepSize) for w in ws]
    identical = True
    cells_handles = 0
    for i, e in enumerate(engines):
        v1, p1 = e.values(1), e.policy(1)
        identical &= bool(np.array_equal(batch.values(i, 1), v1) and np.array_equal(batch.policy(i, 1), p1))
        identical &= bool(ini_v[i] == v1[ix[i]] and ini_k[i] == p1[ix[i]])
        cells_handles += e.stats().cells_evaluated
    if not identical:
        raise SystemExit("the batch and the looped handles DIFFER: nothing is timed")
    cells = int(bst.cells_evaluated)
    assert cells == cells_handles

    def run_a():
        for e in engines:
            e.solve(sync=False)

    def run_b():
        batch.solve(sync=False)

    sweeps_a = max(1, int(np.ceil(args.window * 1e3 / timed(run_a, 1)[0])))
    sweeps_b = max(1, int(np.ceil(args.window * 1e3 / timed(run_b, 3)[0])))
    A, B = [], []
    for _ in range(args.samples):
        A.append(timed(run_a, sweeps_a))
        B.append(timed(run_b, sweeps_b))

    # per-period launch times of the batch (events between the launches: a run of its own)
    prof = make_batch(profiling=True)
    prof.solve(sync=True)
    prof.solve(sync=True)
    period_ms = [prof.period_ms(t) for t in range(1, prof.T + 1)]
    prof.close()

    # ---- inclusive: what a driver pays ---------------------------------------------------------------------------------
    def incl_a():
        es = make_engines()
        for e in es:
            e.solve(sync=False)
        out = []
        for e, k in zip(es, ix):  # getExpectedValue / getAction of the initial state (the first read waits for the sweep)
            out.append((e.values(1)[k], e.policy(1)[k]))
        for e in es:
            e.close()
        return out

    def incl_b():
        b = make_batch()
        b.solve(sync=False)
        out = b.initial()
        b.close()
        return out

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    for e in engines:
        e.close()
    batch.close()
    A1, B1 = [], []
    for _ in range(args.inclusive_samples):
        A1.append(wall(incl_a))
        B1.append(wall(incl_b))

    def summary(xs):
        return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}

    a_host, b_host = [x[0] for x in A], [x[0] for x in B]
    res = {
        "workload": f"CLSPTesting.main, {n} instances of 1001 states x 501 actions, T = 8",
        "device": torch.cuda.get_device_name(0),
        "instances": n,
        "cells_per_sweep": cells,
        "bit_identical_to_looped_handles": identical,
        "plan": {"r": bst.window_r, "s": bst.window_s, "chunks": bst.window_chunks, "lds_bytes": int(bst.lds_bytes),
                 "period_launches": bst.period_launches, "finalize_launches": bst.finalize_launches,
                 "win_s_override": os.environ.get("SDPGPU_WIN_S", "")},
        "sweeps_per_sample": {"A": sweeps_a, "B": sweeps_b},
        "A_ms_per_sweep_host": summary(a_host), "A_ms_per_sweep_device": summary([x[1] for x in A]),
        "B_ms_per_sweep_host": summary(b_host), "B_ms_per_sweep_device": summary([x[1] for x in B]),
        "A_inclusive_ms": summary(A1) if A1 else None, "B_inclusive_ms": summary(B1) if B1 else None,
        "A_over_B": statistics.median(a_host) / statistics.median(b_host),
        "A_inclusive_over_B_inclusive": statistics.median(A1) / statistics.median(B1) if A1 else None,
        "B_cells_per_s": cells / (statistics.median(b_host) * 1e-3),
        "B_period_ms": period_ms,
        "max_B_below_min_A": max(b_host) < min(a_host),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("instances", "plan", "A_over_B", "A_inclusive_over_B_inclusive", "B_cells_per_s",
                                          "max_B_below_min_A")}))
    print("A  ms/sweep (host)", res["A_ms_per_sweep_host"])
    print("B  ms/sweep (host)", res["B_ms_per_sweep_host"])
    print("A' ms", res["A_inclusive_ms"])
    print("B' ms", res["B_inclusive_ms"])
    print("B per-period ms", period_ms)
    return 0 if res["max_B_below_min_A"] else 1


if __name__ == "__main__":
    sys.exit(main())
