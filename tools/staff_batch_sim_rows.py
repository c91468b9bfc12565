"""Steps 2-5 of WorkforceTesting.main's loop body (216 instances, workloads.workforce_testing_sweep; two level rules each on the
default tree of 10 000 leaves) two ways, in one process:

  A   one separable handle per instance, each calling sdpgpu_staff_simulate with n_rules = 2: 216 rollout launches
  B   one sdpgpu_batch_staff_simulate call on the solved batch: one rollout launch
  C   B plus sdpgpu_batch_staff_fit_ss
  D   solve + fit + rollout + initial(): the whole loop body on the batch

The batch is made and solved first and stays alive; its fitted levels are rule 0 of every instance, the same levels + 1 (a stand-in
for the MIP's) rule 1.  The handles of A live in chunks (a handle keeps pmfs[t] once per period on the host: 64 MB each) and are
NOT solved: a level rule needs the device tables only.  Per sample, A is the SUM over the 216 handles of the call's kernel_ms
(HIP events around each call's own launches: the gaps between handles are not counted, which favours A) and, beside it, the wall
time of the loop; the create + table upload of the 216 handles (create, and a first call on a one-leaf tree that uploads) is
reported apart.  B is the kernel_ms of its one call, and its wall time.  --samples samples each after one warm-up, median and
range.  Asserted: every leaf sum and every mean of A equals B's by bits.  Reported, not tuned: whether the range of B's kernel_ms
lies above the range of A's summed kernel_ms.

    python tools/staff_batch_sim_rows.py [--samples 7] [--chunk 27] [--json profiles/staff_batch_sim_rows.json]
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

SEED = 12345


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": list(xs)}


def handle(w):
    d = w.desc()
    d.kernel, d.device = sia._abi.KERNEL_SEPARABLE, 0
    return sia.SdpEngine(d, None, w.overhead(), level_pmf=w.level_pmf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=27, help="handles alive at a time")
    ap.add_argument("--instances", type=int, default=0, help="only the first N instances of the sweep (0: all 216)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "staff_batch_sim_rows.json"))
    args = ap.parse_args()
    import torch
    n = max(args.samples, 1)
    sweep = workloads.workforce_testing_sweep()
    if args.instances:
        sweep = sweep[:args.instances]
    N, T = len(sweep), sweep[0].T
    out = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "", "samples": n, "instances": N, "rules": 2,
           "build_id": sia._abi.load().sdpgpu_build_id().decode()}

    rec = sia.StaffRecursionBatch([w.functor for w in sweep], [w.level_pmf for w in sweep], T, device=0)
    b = rec.batch
    tree = rec.defaultSampleNums()
    leaves = int(np.prod(tree))
    out["tree"], out["leaves"] = tree, leaves
    b.solve(sync=True)
    levels = b.fit_ss(2 ** 31 - 1)
    rules = np.ascontiguousarray(np.stack([levels, levels + 1.0], axis=1))  # (N, 2, T, 2)

    # ---- B, C, D on the batch ----
    b.staff_simulate(tree, SEED, 0, rules)  # warm-up: the scratch block, the code objects
    b_ms, b_wall, c_wall, d_wall, fit_wall = [], [], [], [], []
    for _ in range(n):
        t0 = time.perf_counter()
        res_b, sums_b, valid_b = b.staff_simulate(tree, SEED, 0, rules, want_sums=True)
        b_wall.append((time.perf_counter() - t0) * 1e3)
        b_ms.append(res_b[0][0].kernel_ms)
    for _ in range(n):
        t0 = time.perf_counter()
        b.staff_simulate(tree, SEED, 0, rules)
        b_nosum = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        lv = b.fit_ss(2 ** 31 - 1)
        fit_wall.append((time.perf_counter() - t0) * 1e3)
        c_wall.append(b_nosum + fit_wall[-1])
        assert lv.tobytes() == levels.tobytes()
    for _ in range(n):
        t0 = time.perf_counter()
        b.solve(sync=False)
        lv = b.fit_ss(2 ** 31 - 1)
        res_d = b.staff_simulate(tree, SEED, 0, np.ascontiguousarray(np.stack([lv, lv + 1.0], axis=1)))
        ini_v, ini_a = b.initial()
        d_wall.append((time.perf_counter() - t0) * 1e3)
        assert [r.mean for row in res_d for r in row] == [r.mean for row in res_b for r in row]
    assert valid_b.all() and all(r.n_valid == leaves for row in res_b for r in row)
    out["B_kernel_ms"], out["B_wall_ms"] = summary(b_ms), summary(b_wall)
    out["C_fit_wall_ms"], out["C_wall_ms"] = summary(fit_wall), summary(c_wall)
    out["D_wall_ms"] = summary(d_wall)
    out["solve_ms"] = float(b.stats().solve_ms)

    # ---- A: one handle per instance, in chunks ----
    a_ms, a_wall = [0.0] * n, [0.0] * n
    create_wall = 0.0
    sums_equal = means_equal = 0
    one_leaf = [1] * T
    for c0 in range(0, N, max(args.chunk, 1)):
        idx = list(range(c0, min(N, c0 + max(args.chunk, 1))))
        t0 = time.perf_counter()
        engs = [handle(sweep[i]) for i in idx]
        for e, i in zip(engs, idx):
            e.staff_simulate(one_leaf, SEED, 0, rules[i])  # (uploads the tables; also the warm-up of this handle)
        create_wall += (time.perf_counter() - t0) * 1e3
        for s in range(n):
            t0 = time.perf_counter()
            got = [e.staff_simulate(tree, SEED, 0, rules[i], want_sums=True) for e, i in zip(engs, idx)]
            a_wall[s] += (time.perf_counter() - t0) * 1e3
            a_ms[s] += sum(res[0].kernel_ms for res, _, _ in got)
            if s == 0:
                for (res, sums, valid), i in zip(got, idx):
                    assert sums.tobytes() == sums_b[i].tobytes(), f"leaf sums of instance {i} differ between A and B"
                    sums_equal += sums.size
                    for r in range(2):
                        assert np.float64(res[r].mean).tobytes() == np.float64(res_b[i][r].mean).tobytes(), (i, r, res[r].mean, res_b[i][r].mean)
                        assert np.float64(res[r].m2).tobytes() == np.float64(res_b[i][r].m2).tobytes() and res[r].n_valid == res_b[i][r].n_valid
                        means_equal += 1
        for e in engs:
            e.close()
    out["A_kernel_ms_sum"], out["A_wall_ms"] = summary(a_ms), summary(a_wall)
    out["A_create_upload_wall_ms"] = create_wall
    out["leaf_sums_equal_by_bits"], out["means_equal_by_bits"] = sums_equal, means_equal
    out["B_range_above_A_range"] = bool(min(b_ms) > max(a_ms))
    rec.close()

    print(f"{N} instances x 2 rules x {leaves} leaves, {n} samples (median [min .. max], ms)")
    for key in ("A_kernel_ms_sum", "A_wall_ms", "B_kernel_ms", "B_wall_ms", "C_fit_wall_ms", "C_wall_ms", "D_wall_ms"):
        v = out[key]
        print(f"  {key:18s} {v['median']:10.3f} [{v['min']:.3f} .. {v['max']:.3f}]")
    print(f"  A create + upload  {create_wall:10.1f} (once)")
    print(f"  equal by bits: {sums_equal} leaf sums, {means_equal} means; B's range above A's: {out['B_range_above_A_range']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
