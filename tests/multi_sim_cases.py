"""The instances the two-product rollout is tested on (tests/test_multi_sim_twin.py on the CPU, tests/test_gpu_multi_sim.py on
the GPU): the 24 random MultiItemCash instances, the 24 random MultiItemCashXR ones, and the lead-time family's KAT-1 and
KAT-2 with its action box cut to 12 (64 support paths).  Every case is (id, kind, keyword arguments of the solver, deposit
rate); the oracle's memo and the twin's path sums of a case are computed once per session and shared."""
import functools
import json
import os

import numpy as np

import multicash_cases
import multi_sim_twin as twin

HERE = os.path.dirname(os.path.abspath(__file__))
LEAD_KEYS = ("T", "q_bound", "price", "vari_cost", "sal_value", "ini_cash", "ini_i1", "ini_i2", "r0", "r1", "r2", "limit",
             "interest_free", "min_inventory", "max_inventory", "min_cash", "max_cash", "discount", "overhead", "values",
             "probs")


@functools.lru_cache(maxsize=None)
def _kats():
    return json.load(open(os.path.join(HERE, "golden", "kat_reference.json")))


def case(cid):
    """'mc-<seed>', 'xr-<seed>', 'kat1', 'kat2-q12', 'kat1-stocked' -> (kind, kw, deposit rate)."""
    if cid.startswith("mc-"):
        return "multicash", multicash_cases.random_instance(int(cid[3:])), 0.0
    if cid.startswith("xr-"):
        dep, kw = multicash_cases.xr_random_instance(int(cid[3:]))
        return "multixr", kw, dep
    if cid == "kat1":
        k = _kats()["kat1"]
        return "multilead", {n: k[n] for n in LEAD_KEYS}, 0.0
    if cid == "kat2-q12":
        k = _kats()["kat2_slow"]
        return "multilead", dict({n: k[n] for n in LEAD_KEYS}, q_bound=12), 0.0
    if cid == "kat1-stocked":  # more stock than the largest demand: a demand above the support leaves the memo in period 1
        k = _kats()["kat1"]
        return "multilead", dict({n: k[n] for n in LEAD_KEYS}, ini_i1=45.0, ini_i2=25.0, q_bound=12), 0.0
    raise KeyError(cid)


ALL = [f"mc-{s}" for s in range(24)] + [f"xr-{s}" for s in range(24)] + ["kat1", "kat2-q12"]
ONE_PERIOD = ["mc-11", "mc-14", "mc-21", "mc-23"]  # the T = 1 seeds: no transition is taken


def discount_weights(kw):
    """Math.pow(discountFactor, t), t = 0 .. T-1."""
    return [float(kw["discount"]) ** t for t in range(kw["T"])]


def oracle_memo(oracle, cid):
    """((final value, ...), memo rows) of the oracle's literal recursion."""
    kind, kw, dep = case(cid)
    if kind == "multixr":
        return oracle.memo_table("multixr", dep, **kw)
    return oracle.memo_table(kind, **kw)


_REF = {}


def reference(oracle, cid):
    """Once per session: the oracle's memo of the case, all its support paths and the twin's sums along them."""
    if cid not in _REF:
        kind, kw, dep = case(cid)
        res, rows = oracle_memo(oracle, cid)
        d1, d2, prob = twin.support_paths(twin.tiles(kind, kw))
        sums, valid = twin.rollout(kind, kw, twin.memo_dict(rows), d1, d2, discount_weights(kw), dep)
        for a in (rows, d1, d2, prob, sums, valid):
            a.setflags(write=False)
        _REF[cid] = dict(kind=kind, kw=kw, dep=dep, final_value=res[0], rows=rows, d1=d1, d2=d2, prob=prob, sums=sums, valid=valid)
    return _REF[cid]


def solve(sia, cid):
    """The GPU solve of the case with its memo: MultiLeadResult."""
    from stochastic_inventory_amd import multiitem
    kind, kw, dep = case(cid)
    if kind == "multixr":
        return multiitem.multixr_solve(dep, table=True, **kw)
    return {"multicash": multiitem.multicash_solve, "multilead": multiitem.multilead_solve}[kind](table=True, **kw)


def policy(sia, cid, rows, capacity_log2=0):
    from stochastic_inventory_amd.multiitem import MultiPolicy
    kind, kw, dep = case(cid)
    return MultiPolicy(kind, rows, capacity_log2, depositeRate=dep, **kw) if kind == "multixr" else MultiPolicy(kind, rows, capacity_log2, **kw)
