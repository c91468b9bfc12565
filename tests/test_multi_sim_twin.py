"""CPU: the host twin of the two-product rollout (tests/multi_sim_twin.py) against the oracle's literal recursion.  The
policy of the oracle's memo, rolled by the twin along EVERY support path of an instance, must reproduce the value the
recursion computed: sum over paths of probability x path sum = V_1 = final_value - ini_cash.  That pins the twin's lambdas,
its loop and its reading of the memo to the reference; it needs no device and passes without the rollout's kernels.

Tolerance 1e-12 relative to max(1, |V_1|): the two sides add the same products in different orders (the recursion nests the
periods, the test sums whole paths) and nothing else differs.  What the identity gives on these 50 instances with the
oracle's memo is a few 1e-16 (at most 3.9e-16); no path leaves the memo."""
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multi_sim_cases as cases  # noqa: E402


def weighted_identity(ref):
    """|sum_p prob_p x sum_p - V_1| / max(1, |V_1|)."""
    v1 = ref["final_value"] - float(ref["kw"]["ini_cash"])
    est = math.fsum(float(p) * float(s) for p, s in zip(ref["prob"], ref["sums"]))
    return abs(est - v1) / max(1.0, abs(v1))


@pytest.mark.parametrize("cid", cases.ALL)
def test_twin_reproduces_the_recursions_value(oracle, cid):
    ref = cases.reference(oracle, cid)
    n = len(ref["prob"])
    assert ref["valid"].all(), "a support path left the oracle's memo"
    assert abs(math.fsum(ref["prob"].tolist()) - 1.0) < 1e-12
    err = weighted_identity(ref)
    print(f"{cid}: {n} paths, T = {ref['kw']['T']}, {len(ref['rows'])} memo rows, identity {err:.3g}")
    assert err <= 1e-12


def test_path_counts():
    """The sizes the GPU tests lean on: at most 486 paths for a random instance, 81 for KAT-1, 64 for KAT-2 with Qbound 12."""
    import multi_sim_twin as twin
    counts = {}
    for cid in cases.ALL:
        kind, kw, _ = cases.case(cid)
        counts[cid] = math.prod(len(t) for t in twin.tiles(kind, kw))
    assert max(v for k, v in counts.items() if k[:2] in ("mc", "xr")) <= 486
    assert counts["kat1"] == 81 and counts["kat2-q12"] == 64
    assert all(cases.case(c)[1]["T"] == 1 for c in cases.ONE_PERIOD)
