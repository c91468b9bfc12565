"""ThreeLevelFitsSTest's 810 instances (workloads.fitss_sweep): the sweep as 27 batches of one shape against ONE ragged batch.

One process, one stream of its own, HIP events beside a synchronised host clock.

  A   27 pre-created SdpBatches, one per order limit (today's only route; each is small enough to be chunked: key rows, a
      key reset and a finalize pass per batch); timed: 27 x solve(sync=False) + one synchronize
  B   one SdpBatch(..., ragged=True) of all 810: solve alone
  C   B's solve + simulate_sampled(10000) + initial(): what the driver's loop body asks of every instance
  D   the WHOLE loop body of ThreeLevelFitsSTest.main (:120-145): B's solve + initial() + simulate_sampled(10000) (the table
      policy) + simulate_ss_sampled(levels, 10000) with the rule fitted on the device + the 810 gaps
      (simFinalValue - finalValue) / finalValue; the fit and rule-rollout kernels by HIP events (simulate_ms).  Beside it the
      only route the batch offered before for the fit and the rule rollout: read the policy rows back (sdpgpu_batch_policy),
      fit with the plain-Python twin of tests/fitss_twin.py and roll the rule out in numpy, path-vectorised, on demands from
      sample_demands -- on every `--host-stride`-th instance, scaled to 810
  E   D + check_convexity(kind=1, source="values", period=1, x_lo=0, x_hi=100): the loop body through :159, the CSV row's
      last column (CheckKConvexity.checkCK on V_1(x), x = 0 .. 100) included

The same run times a heavy case of its own: CheckKConvexity.check over the WHOLE grid (1101 points, 2.2e8 triples a row), on
G, for all six periods of all 810 instances -- six launches, by HIP events -- and beside it the host route: sdpgpu_batch_gy
read-back plus sdpgpu_check_convexity in one thread, on every `--host-stride`-th instance, scaled to 810.  Its samples go to
`--convexity-out` (profiles/batch_convexity.json).

A sample is as many back-to-back sweeps as fill the window, divided by their number; samples alternate A, B, C, D, E, A, ...
after a warm-up.  Before anything is timed the two routes are compared bit for bit (initial values and actions of all 810, the
period-1 tables of one instance per shape).

    python tools/fitss_sweep_rows.py [--samples 7] [--out profiles/batch_fitss_sweep.json]

Under `rocprofv3 --kernel-trace --stats -- python tools/fitss_sweep_rows.py --trace-b` only B runs (three sweeps, nothing
written).

UNIFORM BATCHES MUST NOT PAY.  `--uniform FILE` times SdpBatch.solve of CLSPTesting's 540 instances (the batch of one shape)
and writes its samples to FILE; it uses nothing newer than SdpBatch itself, so the same file runs from a checkout of the
parent commit.  Run it from both trees in one session, alternating, then hand the files to the main run:
`--uniform-parent P1.json,P2.json --uniform-new N1.json,N2.json`.  The verdict in the output: the new median lies within the
parent's own min-to-max spread, or within 1 % of its median where that spread is tighter than 1 %.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import stochastic_inventory_amd as sia
from stochastic_inventory_amd import workloads


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def timed(stream, fn, sweeps):
    """(host ms, device ms) per sweep of `sweeps` back-to-back calls of fn."""
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


def numpy_rule_rollout(levels, rule, dem, ini, max_q, K, v, h, pi, lo, hi):
    """SimulateFitsS.simulateSinglesS / TwosS / ThreesS for ONE instance, all paths at once: rule [T, 2 * levels], dem [n, T]."""
    x = np.full(dem.shape[0], float(ini))
    total = np.zeros(dem.shape[0])
    for t in range(dem.shape[1]):
        o = rule[t]
        if t == 0:
            a = np.full_like(x, o[1] - ini)
        elif levels == 1:
            a = np.where(x >= o[0], 0.0, np.minimum(max_q, o[1] - x))
        else:
            a = np.zeros_like(x)
            lower = -np.inf
            for b in range(levels):
                band = (x < o[0]) if b == 0 else ((lower <= x) & (x < o[2 * b]))
                a = np.where(band, np.minimum(max_q, o[2 * b + 1] - x), a)
                lower = o[2 * b]
        level = (x + a) - dem[:, t]
        total += ((np.where(a > 0, K, 0.0) + v * a) + h * np.maximum(level, 0.0)) + pi * np.maximum(-level, 0.0)
        x = np.maximum(np.minimum(level, hi), lo)
    return total


def host_route(ragged, ws, idx, levels, paths, seed, tw):
    """What the batch offered before for the fit and the rule rollout, on the instances `idx`: -> (seconds, rules, path sums)."""
    t0 = time.perf_counter()
    rules, sums = [], []
    T = ragged.T
    for i in idx:
        f = ws[i].functor
        rows = []
        for period in range(1, T + 1):
            lo, hi = ragged.reachable(i, period)
            pol = ragged.policy(i, period)
            k = np.arange(lo, hi + 1)
            rows.append(np.stack([np.full(len(k), float(period)), f.minInventory + k.astype(np.float64), pol[k].astype(np.float64)], axis=1))
        rule = tw.fit(levels, T, int(f.maxOrderQuantity), np.concatenate(rows))
        dem, _ = ragged.sample_demands(i, paths, seed)
        sums.append(numpy_rule_rollout(levels, rule, dem, f.iniInventory, float(int(f.maxOrderQuantity)), f.fixedOrderingCost,
                                       f.variOrderingCost, f.holdingCost, f.penaltyCost, f.minInventory, f.maxInventory))
        rules.append(rule)
    return time.perf_counter() - t0, np.stack(rules), np.stack(sums)


def descs_of(ws):
    out = [w.desc() for w in ws]
    for d in out:
        d.device = 0
    return out


def uniform(args, stream):
    ws = workloads.clsp_testing_sweep()
    b = sia.SdpBatch(descs_of(ws), [w.pmf for w in ws])
    b.set_stream(stream.cuda_stream)
    b.solve(sync=True)
    run = lambda: b.solve(sync=False)
    sweeps = max(1, int(np.ceil(args.window * 1e3 / timed(stream, run, 3)[0])))
    timed(stream, run, sweeps)  # warm-up
    S = [timed(stream, run, sweeps) for _ in range(args.samples)]
    st = b.stats()
    res = {"workload": f"CLSPTesting.main, {len(ws)} instances of one shape, SdpBatch.solve", "tree": ROOT,
           "device": torch.cuda.get_device_name(0), "sweeps_per_sample": sweeps,
           "plan": {"r": st.window_r, "s": st.window_s, "chunks": st.window_chunks, "lds_bytes": int(st.lds_bytes)},
           "ms_per_sweep_host": summary([x[0] for x in S]), "ms_per_sweep_device": summary([x[1] for x in S])}
    b.close()
    with open(args.uniform, "w") as f:
        json.dump(res, f, indent=1)
    print("uniform", ROOT, res["ms_per_sweep_host"])
    return 0


def uniform_verdict(parent_files, new_files):
    def pool(files):
        runs = [json.load(open(p)) for p in files]
        return runs, [x for r in runs for x in r["ms_per_sweep_host"]["samples"]]
    pr, p = pool(parent_files)
    nr, n = pool(new_files)
    pm, nm = statistics.median(p), statistics.median(n)
    spread = (max(p) - min(p)) / pm
    ok = (min(p) <= nm <= max(p)) if spread >= 0.01 else abs(nm - pm) <= 0.01 * pm
    return {"workload": pr[0]["workload"], "order": "parent and new processes alternating in one session",
            "parent_ms_per_sweep_host": summary(p), "new_ms_per_sweep_host": summary(n),
            "parent_spread_relative": spread, "new_over_parent_median": nm / pm,
            "rule": "new median within the parent's min..max, or within 1 % of its median where that spread is below 1 %",
            "new_median_within_rule": bool(ok), "parent_plan": pr[0]["plan"], "new_plan": nr[0]["plan"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3, help="least length of a timed window, seconds")
    ap.add_argument("--paths", type=int, default=10000, help="sample paths per instance of row C (Simulation's sampleNum)")
    ap.add_argument("--levels", type=int, default=3, help="row D: the driver (1, 2, 3: One-, Two-, ThreeLevelFitsSTest)")
    ap.add_argument("--host-stride", type=int, default=30, help="row D's host route runs on every n-th instance and is scaled")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_fitss_sweep.json"))
    ap.add_argument("--convexity-out", default=os.path.join(ROOT, "profiles", "batch_convexity.json"))
    ap.add_argument("--trace-b", action="store_true", help="run B three times and leave (for a kernel trace)")
    ap.add_argument("--uniform", default="", help="time CLSPTesting's uniform batch only and write the samples to this file")
    ap.add_argument("--uniform-parent", default="", help="comma-separated --uniform files of the parent commit")
    ap.add_argument("--uniform-new", default="", help="comma-separated --uniform files of this tree")
    args = ap.parse_args()
    if args.samples < 5:
        raise SystemExit("at least 5 samples")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it has no CPU path")
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    sptr = stream.cuda_stream
    if args.uniform:
        return uniform(args, stream)

    ws = workloads.fitss_sweep()
    n = len(ws)
    descs, pmfs = descs_of(ws), [w.pmf for w in ws]
    ragged = sia.SdpBatch(descs, pmfs, ragged=True)
    ragged.set_stream(sptr)
    ragged.solve(sync=True)
    if args.trace_b:
        for _ in range(3):
            ragged.solve(sync=True)
        ragged.close()
        return 0
    groups = {}
    for i, w in enumerate(ws):
        groups.setdefault(int(w.functor.maxOrderQuantity), []).append(i)
    shaped = []
    for q, idx in sorted(groups.items()):
        g = sia.SdpBatch([descs[i] for i in idx], [pmfs[i] for i in idx])
        g.set_stream(sptr)
        g.solve(sync=True)
        shaped.append((q, idx, g))

    # ---- the two routes compared at the size that is timed -------------------------------------------------------------
    rst = ragged.stats()
    ini_v, ini_k = ragged.initial()
    identical, cells_a, launches_a, others_a, chunks_a = True, 0, 0, 0, []
    for q, idx, g in shaped:
        gv, gk = g.initial()
        identical &= bool(np.array_equal(ini_v[idx], gv) and np.array_equal(ini_k[idx], gk))
        identical &= bool(np.array_equal(ragged.values(idx[0], 1), g.values(0, 1)) and np.array_equal(ragged.policy(idx[0], 1), g.policy(0, 1)))
        st = g.stats()
        cells_a += int(st.cells_evaluated)
        launches_a += st.period_launches
        others_a += st.finalize_launches
        chunks_a.append(st.window_chunks)
    if not identical:
        raise SystemExit("the ragged batch and the batches by shape DIFFER: nothing is timed")
    assert cells_a == int(rst.cells_evaluated)

    def run_a():
        for _, _, g in shaped:
            g.solve(sync=False)

    def run_b():
        ragged.solve(sync=False)

    def run_c():
        ragged.solve(sync=False)
        ragged.simulate_sampled(args.paths, 12345)
        ragged.initial()

    gaps = {}

    def run_d():
        ragged.solve(sync=False)
        final, _ = ragged.initial()
        table_mean = ragged.simulate_sampled(args.paths, 12345)
        rule_mean = ragged.simulate_ss_sampled(args.levels, args.paths, 12345)
        gaps["rule"] = (rule_mean - final) / final
        gaps["table"] = (table_mean - final) / final

    verdict = {}

    def run_e():
        run_d()
        verdict["ck"] = ragged.check_convexity(1, source="values", period=1, x_lo=0.0, x_hi=100.0)

    runs = (("A", run_a), ("B", run_b), ("C", run_c), ("D", run_d), ("E", run_e))
    sweeps = {k: max(1, int(np.ceil(args.window * 1e3 / timed(stream, f, 2)[0]))) for k, f in runs}
    rows = {k: [] for k, _ in runs}
    for k, f in runs:  # warm-up at the timed length
        timed(stream, f, sweeps[k])
    for _ in range(args.samples):
        for k, f in runs:
            rows[k].append(timed(stream, f, sweeps[k]))
    run_c()
    sim_ms = ragged.simulate_ms()
    fit_rule_ms = []
    for _ in range(args.samples):
        run_d()
        fit_rule_ms.append(ragged.simulate_ms())

    # row D's other side: policy rows to the host, the twin's fit, a numpy rollout -- on a subset, checked against the device
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fitss_twin as tw
    sub = list(range(0, n, max(1, args.host_stride)))
    dev_rules = ragged.fit_ss(args.levels)
    _, dev_sums = ragged.simulate_ss_sampled(args.levels, args.paths, 12345, want_sums=True)
    host_route(ragged, ws, sub[:2], args.levels, args.paths, 12345, tw)  # warm-up
    host_s = []
    for _ in range(args.samples):
        sec, h_rules, h_sums = host_route(ragged, ws, sub, args.levels, args.paths, 12345, tw)
        host_s.append(sec * 1e3 * n / len(sub))
    rules_equal = bool(np.array_equal(h_rules, dev_rules[sub]))
    sums_equal = bool(np.array_equal(h_sums, dev_sums[sub]))

    # ---- the heavy case: check over the whole grid, on G, all periods of all instances ----------------------------------
    from stochastic_inventory_amd.structure import check_row
    T = ragged.T
    heavy_res = {}

    def heavy():
        for t in range(1, T + 1):
            heavy_res[t] = ragged.check_convexity(0, source="gy", period=t)

    nx = ragged.num_states_of(0)
    row_triples = nx * (nx - 1) * (nx - 2) // 6
    timed(stream, heavy, 1)  # warm-up (the G rows are made here)
    heavy_s = [timed(stream, heavy, 1) for _ in range(args.samples)]
    heavy_holds = int(sum(int(heavy_res[t]["holds"].sum()) for t in heavy_res))
    heavy_first = sorted({(int(r["i0"]), int(r["i1"]), int(r["i2"])) for t in heavy_res for r in heavy_res[t] if not r["holds"]})
    # A check ends at its first violation, so only a row that HOLDS costs all its triples.  The rate comes from the same six
    # launches with K = 1e12 for every instance: every row holds, every triple is evaluated.
    full_res = {}

    def full():
        for t in range(1, T + 1):
            full_res[t] = ragged.check_convexity(0, source="gy", period=t, K=1.0e12)

    timed(stream, full, 1)
    full_s = [timed(stream, full, 1) for _ in range(args.samples)]
    full_holds = int(sum(int(full_res[t]["holds"].sum()) for t in full_res))
    triples = n * T * row_triples
    # the host route: the G rows back, one thread of sdpgpu_check_convexity; a sample = one instance's six rows, scaled
    heavy_host, heavy_equal = [], True
    for i in sub:
        t0 = time.perf_counter()
        own = [check_row(0, ragged.gy(i, t), ws[i].functor.fixedOrderingCost) for t in range(1, T + 1)]
        heavy_host.append((time.perf_counter() - t0) * 1e3 * n)
        for t, r in enumerate(own, start=1):
            d = heavy_res[t][i]
            heavy_equal &= (r.holds, r.i0, r.i1, r.i2) == (d["holds"], d["i0"], d["i1"], d["i2"]) and \
                np.array_equal(np.array([r.lhs, r.rhs]).view(np.uint64), np.array([d["lhs"], d["rhs"]]).view(np.uint64))
    heavy_dev = statistics.median(x[1] for x in heavy_s)
    full_dev = statistics.median(x[1] for x in full_s)
    conv = {
        "workload": f"CheckKConvexity.check over the whole grid ({nx} points) on G_t, t = 1 .. {T}, of {n} instances: {T} launches",
        "device": torch.cuda.get_device_name(0), "rows": n * T, "triples_per_row": row_triples,
        "with_each_instances_K": {
            "rows_that_hold": heavy_holds, "triples_of_the_rows_that_hold": heavy_holds * row_triples,
            "distinct_first_violations": len(heavy_first), "first_violations_sample": heavy_first[:8],
            "ms_device_events": summary([x[1] for x in heavy_s]), "ms_host_clock": summary([x[0] for x in heavy_s]),
            "host_route": {"what": "sdpgpu_batch_gy read-back + sdpgpu_check_convexity, one thread; one sample = one instance's six rows x "
                                   "the instance count", "instances_run": len(sub), "scaled_to": n, "ms_scaled": summary(heavy_host),
                           "equal_the_device_results": bool(heavy_equal)},
            "host_route_over_device": statistics.median(heavy_host) / heavy_dev},
        "with_K_1e12_every_row_holds": {
            "rows_that_hold": full_holds, "triples": triples, "ms_device_events": summary([x[1] for x in full_s]),
            "ms_host_clock": summary([x[0] for x in full_s]),
            "triples_per_s_device": triples / (full_dev * 1e-3) if full_holds == n * T else None},
        "row_E_last_column": {"what": "checkCK on V_1(x), x = 0 .. 100, K and capacity of the instance (ThreeLevelFitsSTest.java:146-159)",
                              "rows_that_hold": int(verdict["ck"]["holds"].sum()), "rows": n},
    }
    with open(args.convexity_out, "w") as f:
        json.dump(conv, f, indent=1)

    # per-period launch times of the ragged batch (events between the launches: a run of its own)
    prof = sia.SdpBatch(descs, pmfs, ragged=True)
    prof.set_stream(sptr)
    prof.set_profiling(True)
    prof.solve(sync=True)
    prof.solve(sync=True)
    period_ms = [prof.period_ms(t) for t in range(1, prof.T + 1)]
    plans = [prof.plan(t) for t in range(1, prof.T + 1)]
    prof.close()

    host = {k: [x[0] for x in v] for k, v in rows.items()}
    cells = int(rst.cells_evaluated)
    res = {
        "workload": f"ThreeLevelFitsSTest.main, {n} instances of 1101 states, {len(groups)} order limits 26 .. 288, T = 6",
        "device": torch.cuda.get_device_name(0),
        "instances": n,
        "cells_per_sweep": cells,
        "bit_identical_A_and_B": identical,
        "A_route": {"batches": len(shaped), "period_launches": launches_a, "other_launches": others_a,
                    "chunks_min": min(chunks_a), "chunks_max": max(chunks_a)},
        "B_plan": {"r": rst.window_r, "s": rst.window_s, "chunks": rst.window_chunks, "lds_bytes": int(rst.lds_bytes),
                   "period_launches": rst.period_launches, "other_launches": rst.finalize_launches,
                   "tasks_per_period": [int(p.tasks) for p in plans], "chunk_blocks": [p.chunk_blocks for p in plans]},
        "sweeps_per_sample": sweeps,
        "A_ms_per_sweep_host": summary(host["A"]), "A_ms_per_sweep_device": summary([x[1] for x in rows["A"]]),
        "B_ms_per_sweep_host": summary(host["B"]), "B_ms_per_sweep_device": summary([x[1] for x in rows["B"]]),
        "C_ms_per_sweep_host": summary(host["C"]), "C_ms_per_sweep_device": summary([x[1] for x in rows["C"]]),
        "C_paths_per_instance": args.paths, "C_simulate_kernels_ms": sim_ms,
        "D_ms_per_sweep_host": summary(host["D"]), "D_ms_per_sweep_device": summary([x[1] for x in rows["D"]]),
        "D_levels": args.levels, "D_paths_per_instance": args.paths,
        "D_fit_and_rule_rollout_kernels_ms": summary(fit_rule_ms),
        "D_minus_C_ms_host": statistics.median(host["D"]) - statistics.median(host["C"]),
        "D_gap_rule": {"median": float(np.median(gaps["rule"])), "min": float(gaps["rule"].min()), "max": float(gaps["rule"].max())},
        "D_gap_table_policy_same_paths": {"median": float(np.median(gaps["table"])), "min": float(gaps["table"].min()),
                                          "max": float(gaps["table"].max())},
        "D_host_route": {"what": "sdpgpu_batch_policy of the six periods, the plain-Python fit of tests/fitss_twin.py, sample_demands and a "
                                 "path-vectorised numpy rollout, per instance; fit + rule rollout ONLY (no solve, no table rollout)",
                         "instances_run": len(sub), "scaled_to": n, "ms_scaled": summary(host_s),
                         "rules_equal_the_device_fit": rules_equal, "path_sums_equal_the_device_rollout": sums_equal},
        "E_ms_per_sweep_host": summary(host["E"]), "E_ms_per_sweep_device": summary([x[1] for x in rows["E"]]),
        "E_minus_D_ms_host": statistics.median(host["E"]) - statistics.median(host["D"]),
        "E_rows_that_hold": int(verdict["ck"]["holds"].sum()),
        "D_host_route_over_fit_and_rule_part_of_D": statistics.median(host_s) / max(statistics.median(host["D"]) - statistics.median(host["C"]), 1e-9),
        "A_over_B": statistics.median(host["A"]) / statistics.median(host["B"]),
        "B_cells_per_s": cells / (statistics.median(host["B"]) * 1e-3),
        "B_period_ms": period_ms,
        "max_B_below_min_A": max(host["B"]) < min(host["A"]),
    }
    if args.uniform_parent and args.uniform_new:
        res["uniform_batch_against_parent"] = uniform_verdict(args.uniform_parent.split(","), args.uniform_new.split(","))
    for _, _, g in shaped:
        g.close()
    ragged.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("instances", "A_route", "B_plan", "A_over_B", "B_cells_per_s", "max_B_below_min_A")}))
    for k in "ABCDE":
        print(k, "ms/sweep (host)", res[f"{k}_ms_per_sweep_host"])
    print("B per-period ms", period_ms)
    print("D fit + rule rollout kernels ms", res["D_fit_and_rule_rollout_kernels_ms"], "host route (scaled) ms", res["D_host_route"]["ms_scaled"],
          "rules equal", rules_equal, "sums equal", sums_equal, "gap", res["D_gap_rule"])
    print("heavy case:", conv["workload"])
    print(" each instance's K:", json.dumps(conv["with_each_instances_K"]))
    print(" K = 1e12:", json.dumps(conv["with_K_1e12_every_row_holds"]))
    if "uniform_batch_against_parent" in res:
        print("uniform", json.dumps(res["uniform_batch_against_parent"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
