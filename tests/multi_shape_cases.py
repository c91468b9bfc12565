"""Instances of the three two-product recursions built to reach the shape-dependent code of csrc/sdpgpu_sparse.hip that
random small instances never enter.  Every builder is named after the edge it reaches and says so in `claims`; the
claims are checked from the ORACLE's memo and host arithmetic (preconditions()), never from the engine.

No GPU here.  `python tests/multi_shape_cases.py --check` runs the oracle over every instance and prints its cells, its
time, the states per period and the preconditions (committed as profiles/multi_shape_cases.txt).  The budget is a
condition: an instance costs the oracle at most 1.5e8 (state, action, demand pair) cells.

All data are integers or dyadic fractions.  The cash instances serve both CashRecursionMulti ("multicash") and
CashRecursionMultiXR ("multixr"); their unit costs are integers, so the XR form is eligible for the lattice path too.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_CELLS = 150_000_000

# backward_fact_kernel (csrc/sdpgpu_sparse.hip): threads of a workgroup, order pairs a lane carries through a pass, pairs of
# a run taken together; backward_lead_wave_kernel: chunks of 64 order pairs a pass; backward_kernel: order pairs a lane
FACT_THREADS, FACT_NI, FACT_CH = 512, 5, 4
LEAD_CHUNKS = 10
ACT_PER_LANE = 10
LDS_BYTES = 160 * 1024


class Case:
    def __init__(self, name, family, kw, claims=None, deposit=0.0):
        self.name, self.family, self.kw, self.claims, self.deposit = name, family, kw, dict(claims or {}), deposit

    @property
    def kinds(self):
        return ("multicash", "multixr") if self.family == "cash" else ("multilead",)

    def __repr__(self):
        return self.name


# ---- host arithmetic restated ------------------------------------------------------------------------------------
def fact_index_words(rows):
    """The index word of every pair of a period's list as the launcher forms it: k1 | k2 << 16, k = position of the
    demand among the list's distinct first / second demands in order of first appearance."""
    u1, u2, idx = [], [], []
    for d1, d2 in ((float(r[0]), float(r[1])) for r in rows):
        if d1 not in u1:
            u1.append(d1)
        if d2 not in u2:
            u2.append(d2)
        idx.append(u1.index(d1) | (u2.index(d2) << 16))
    return idx, len(u1), len(u2)


def fact_run(idx):
    """csrc/sdpgpu_sparse.hip: fact_run -- the length of the list's runs of one first index when the list is made of
    runs of equal length, 0 otherwise."""
    if not idx:
        return 0
    run = 1
    while run < len(idx) and (idx[run] & 0xffff) == (idx[0] & 0xffff):
        run += 1
    if len(idx) % run != 0:
        return 0
    for j in range(0, len(idx), run):
        for c in range(1, run):
            if (idx[j + c] & 0xffff) != (idx[j] & 0xffff):
                return 0
    return run


def fact_lds_bytes(q_bound, nd, n_distinct, last, mark=False):
    """csrc/sdpgpu_sparse.hip: fact_lds_bytes."""
    qn = 0 if mark else min(q_bound * q_bound, FACT_THREADS * FACT_NI)
    return qn * 8 + nd * 12 + q_bound * n_distinct * (16 if last else 24) + (q_bound + 1) * 4 + (FACT_THREADS * FACT_NI // 64) * 8 + 32


def pass_boundary(kind, q_bound):
    """First position (in the order the kernel walks a state's actions) of the second pass of backward_fact_kernel."""
    if kind == "multixr" and q_bound <= FACT_THREADS:
        return (FACT_THREADS // q_bound) * q_bound * FACT_NI
    return FACT_THREADS * FACT_NI


def best_positions(kind, kw, table):
    """Per state of the oracle's memo: (position of its best action in the order its actions are walked, number of
    actions it is offered).  multicash walks the OFFERED pairs (variCost . (i, j) < cash + 0.1, MultiItemCash.java:66-76),
    i outer and j inner; multixr the whole box, and the memo holds order-up-to levels."""
    qb = kw["q_bound"]
    i1, i2, cash, a1, a2 = (table[:, c] for c in (1, 2, 5, 7, 8))
    if kind == "multixr":
        q1, q2 = a1 - np.trunc(i1), a2 - np.trunc(i2)
        return (q1 * qb + q2).astype(np.int64), np.full(len(table), qb * qb, np.int64)
    c1, c2 = float(kw["vari_cost"][0]), float(kw["vari_cost"][1])
    rows = np.arange(qb, dtype=np.float64)
    cost = (c1 * rows)[:, None] + (c2 * rows)[None, :]  # orderingCost1 + orderingCost2 of (i, j)
    pos, n_off = np.zeros(len(table), np.int64), np.zeros(len(table), np.int64)
    for lo in range(0, len(table), 1024):
        hi = min(lo + 1024, len(table))
        off = cost[None, :, :] < (cash[lo:hi] + 0.1)[:, None, None]  # [state][i][j]
        per_row = off.sum(axis=2)
        before = np.concatenate([np.zeros((hi - lo, 1), np.int64), np.cumsum(per_row, axis=1)], axis=1)
        n_off[lo:hi] = before[:, qb]
        pos[lo:hi] = before[np.arange(hi - lo), a1[lo:hi].astype(np.int64)] + a2[lo:hi].astype(np.int64)
    return pos, n_off


# ---- builders: the two cash families -----------------------------------------------------------------------------
def dyadic(rng, n, denom):
    """n positive probabilities k / denom (denom a power of two) that sum to one."""
    w = np.ones(n, np.int64) + rng.multinomial(denom - n, np.ones(n) / n)
    return (w / float(denom)).tolist()


def product_list(rng, v1, v2, denom=256):
    """The list GetPmfMulti builds: the second product's demands under every first one."""
    p = dyadic(rng, len(v1) * len(v2), denom)
    return [[float(a), float(b), p[i * len(v2) + j]] for i, a in enumerate(v1) for j, b in enumerate(v2)]


def cash_kw(T, q_bound, pmf, **over):
    kw = dict(T=T, q_bound=q_bound, price=[5.0, 10.0], vari_cost=[1.0, 2.0], sal_price=[0.5, 1.0], ini_cash=30.0,
              ini_i1=0.0, ini_i2=0.0, min_inventory=0.0, max_inventory=12.0, min_cash=0.0, max_cash=150.0, discount=1.0,
              pmf=[np.array(t, dtype=np.float64) for t in pmf])
    kw.update(over)
    return kw


def solver_kw(case, kind):
    """The keyword arguments of the solver / the oracle for `kind` (multixr takes R of the period-1 state as ini_cash)."""
    kw = dict(case.kw)
    if kind == "multixr":
        kw["ini_cash"] = kw["ini_cash"] + kw["vari_cost"][0] * kw["ini_i1"] + kw["vari_cost"][1] * kw["ini_i2"]
    return kw


RUN_SHAPES = [(n1, n2) for n2 in (4, 5, 7, 8, 9) for n1 in (1, 2, 3)]  # (first-demand count, second-demand count)


def runs():
    """Product lists whose runs of one first demand are 4, 5, 7, 8 and 9 pairs long under 1, 2 and 3 first demands: the
    grouped walk of a run (CH = 4 pairs at a time) with tails of 0, 1 and 3 pairs.  Every one of the 15 shapes is the
    list of some period; the last instance has three periods."""
    out = []
    shapes = list(RUN_SHAPES)
    groups = [shapes[2 * k:2 * k + 2] for k in range(6)] + [shapes[12:15]]
    for g, group in enumerate(groups):
        rng = np.random.default_rng(7100 + g)
        T = len(group)
        pmf = []
        for n1, n2 in group:
            v1 = np.sort(rng.choice(np.arange(0, 9), size=n1, replace=False))
            v2 = np.sort(rng.choice(np.arange(0, 10), size=n2, replace=False))
            pmf.append(product_list(rng, v1, v2))
        q_bound = 4 if T == 3 else int(rng.integers(5, 9))
        kw = cash_kw(T, q_bound, pmf, ini_cash=float(rng.integers(12, 40)), ini_i1=float(rng.integers(0, 3)),
                     ini_i2=float(rng.integers(0, 3)), max_inventory=float(rng.integers(4, 10)), discount=[1.0, 0.9375][g % 2])
        name = "runs-" + "+".join(f"{a}x{b}" for a, b in group)
        out.append(Case(name, "cash", kw, {"fact_run": [n2 for _, n2 in group]}))
    return out


def irregular_lists():
    """Lists that are not made of equal runs (fact_run = 0: the pair-by-pair walk that reloads the first product's
    entries when the first index changes), and one of equal runs in which a first demand comes back."""
    out = []

    def add(name, rows, run, seed, q_bound):
        rng = np.random.default_rng(seed)
        rows = [list(map(float, r)) for r in rows]
        kw = cash_kw(2, q_bound, [rows, rows], ini_cash=float(rng.integers(15, 40)), ini_i1=float(rng.integers(0, 3)),
                     ini_i2=float(rng.integers(0, 3)), max_inventory=float(rng.integers(5, 10)))
        out.append(Case(name, "cash", kw, {"fact_run": [run, run]}))

    rng = np.random.default_rng(7200)
    full = product_list(rng, [1, 3, 4], [0, 2, 5, 6], denom=128)
    # (a) one pair of a product list removed, its probability moved to the first pair
    holed = [list(r) for r in full]
    gone = holed.pop(6)
    holed[0][2] += gone[2]
    add("irregular-pair-removed", holed, 0, 7201, 7)
    # (b) the product list shuffled (the first permutation that is not itself made of equal runs)
    for seed in range(7210, 7300):
        order = np.random.default_rng(seed).permutation(len(full))
        shuffled = [full[i] for i in order]
        if fact_run(fact_index_words(shuffled)[0]) == 0:
            break
    add("irregular-shuffled", shuffled, 0, 7202, 6)
    # (c) a first demand that comes back after another one: (1, .), (1, .), (2, .), (2, .), (1, .) -- unequal runs ...
    p = dyadic(rng, 5, 64)
    add("irregular-first-demand-recurs", [[1, 0, p[0]], [1, 2, p[1]], [2, 0, p[2]], [2, 2, p[3]], [1, 3, p[4]]], 0, 7203, 8)
    # ... and equal runs of two pairs, (1, .), (2, .), (1, .): the run walk must reload at every run, not at every NEW demand
    p = dyadic(rng, 6, 64)
    add("irregular-first-demand-recurs-equal-runs",
        [[1, 0, p[0]], [1, 2, p[1]], [2, 0, p[2]], [2, 2, p[3]], [1, 3, p[4]], [1, 5, p[5]]], 2, 7204, 8)
    # (d) a (d1, d2) row listed twice with its probability split (the reference walks the list literally)
    twice = product_list(rng, [2, 4], [1, 3, 5], denom=64)
    half = twice[4][2] / 2
    twice[4][2] = half
    twice.append([twice[4][0], twice[4][1], half])
    add("irregular-row-repeated", twice, 0, 7205, 7)
    return out


def two_passes():
    """More order pairs than one pass of backward_fact_kernel carries (512 lanes x 5): the `> val + 0.1` scan carries its
    value and best action into the second pass.  The first product's demands sit at the top of the action box, so that a
    state without stock of it orders the cap (its best action lies in the second pass) and a state with stock orders
    less (first pass).  Qbound 65: more than 64 rows in multicash's offered-row prefix sum; Qbound 53: idle lanes in
    multixr's lane layout (9 x 53 = 477 of 512).  (T = 2: period T's kernel takes its two passes on every state, the
    not-last forms on the root state alone -- a third period at these action counts is beyond the oracle's budget.)"""
    out = []
    for q_bound, d1, d2, ini_cash, ini_i1, max_inv in ((51, (46, 50), (12, 16), 200.0, 0.0, 8.0), (53, (48, 52), (14, 18), 210.0, 12.0, 20.0),
                                                       (65, (60, 64), (20, 26), 260.0, 35.0, 40.0)):
        rng = np.random.default_rng(7300 + q_bound)
        pmf = [product_list(rng, d1, d2, denom=16) for _ in range(2)]
        # (a root with stock of its own reaches period-2 states with enough of it to order less than the cap)
        kw = cash_kw(2, q_bound, pmf, ini_cash=ini_cash, ini_i1=ini_i1, max_inventory=max_inv, max_cash=400.0)
        out.append(Case(f"two-passes-q{q_bound}", "cash", kw,
                        {"fact_run": [2, 2], "two_passes": True, "root_offered_beyond_one_pass": True}))
    return out


def wide_list():
    """23 x 23 = 529 demand pairs, more than the 512 threads that stage the list (and its index words) into LDS: once as
    the list of period 1 (forward marking, a not-last backward pass), once as the list of period T."""
    out = []
    for where in (0, 1):
        rng = np.random.default_rng(7400 + where)
        wide = product_list(rng, range(23), range(23), denom=4096)
        small = product_list(rng, [3, 9], [2, 7], denom=16)
        pmf = [wide, small] if where == 0 else [small, wide]
        kw = cash_kw(2, 12, pmf, ini_cash=40.0, max_inventory=9.0)
        out.append(Case(f"wide-list-period{where + 1}", "cash", kw, {"fact_run": [23, 2] if where == 0 else [2, 23], "wide_period": where}))
    return out


def tables_beyond_lds():
    """Period 1 lists 170 first demands under one second demand: Qbound 40 x 171 distinct demands x 24 B of factored tables
    do not fit the 160 KiB of LDS, so the launcher itself leaves backward_fact_kernel (both as the marking pass and as the
    backward pass) for lattice_mark_kernel / backward_kernel in that period; period 2 (a 2 x 2 list) stays factored."""
    rng = np.random.default_rng(7500)
    first = product_list(rng, range(170), [3], denom=1024)
    second = product_list(rng, [5, 20], [4, 15], denom=16)
    kw = cash_kw(2, 40, [first, second], ini_cash=60.0, max_inventory=10.0, max_cash=250.0)
    return [Case("tables-beyond-lds", "cash", kw, {"fact_run": [1, 2], "beyond_lds_period": 0})]


# ---- builders: the lead-time family ------------------------------------------------------------------------------
def lead_kw(T, q_bound, values, probs, **over):
    kw = dict(T=T, q_bound=q_bound, price=(5.0, 10.0), vari_cost=(1.0, 2.5), sal_value=(0.5, 1.25), ini_cash=10.0,
              ini_i1=1.0, ini_i2=0.0, r0=0.0078125, r1=0.125, r2=1.5, limit=40.0, interest_free=3.0, min_inventory=0.0,
              max_inventory=9.0, min_cash=-120.0, max_cash=400.0, discount=1.0, overhead=[4.0 + 3 * t for t in range(T)],
              values=[[float(v) for v in values[0]], [float(v) for v in values[1]]], probs=probs, cash_int_cast=False)
    kw.update(over)
    return kw


def lead_chunk_edges():
    """Action counts on and around the edges of backward_lead_wave_kernel's walk: Qbound 8 (NA = 64, one full chunk), 9 (81),
    25 (625, under one pass of 10 chunks), 26 (676, two passes), 36 (1296: three passes, the last chunk partial), 64 (4096,
    the wave kernel's limit) and 65 (4225: backward_kernel by itself, one action at a time)."""
    out = []
    for q_bound in (8, 9, 25, 26, 36, 64, 65):
        rng = np.random.default_rng(7600 + q_bound)
        n1, n2 = (2, 1) if q_bound >= 64 else (2, 2)
        hi = max(3, q_bound // 2)
        v1 = np.sort(rng.choice(np.arange(1, hi + 1), size=n1, replace=False))
        v2 = np.sort(rng.choice(np.arange(1, hi + 1), size=n2, replace=False))
        kw = lead_kw(2, q_bound, [v1, v2], [dyadic(rng, n1, 16), dyadic(rng, n2, 16)], discount=[1.0, 0.9375][q_bound % 2],
                     cash_int_cast=bool(q_bound % 2))
        out.append(Case(f"lead-chunk-edges-q{q_bound}", "lead", kw, {"na": q_bound * q_bound}))
    return out


def lead_deep_passes():
    """Three periods at Qbound 26 (676 order pairs: two passes of the wave kernel, lead_actions<3> of the workgroup form):
    a narrow cash box with the (int) cast, inventories of at most 2 and large demands keep the reachable set small, so
    periods 2 and 3 hold many states that each take two passes -- the not-last passes on more than one state."""
    out = []
    for n_pairs in (1, 2):
        rng = np.random.default_rng(7700 + n_pairs)
        values = [[27], [30]] if n_pairs == 1 else [[27, 29], [30]]
        probs = [dyadic(rng, len(values[0]), 8), [1.0]]
        kw = lead_kw(3, 26, values, probs, max_inventory=2.0, min_cash=-5.0, max_cash=5.0, ini_cash=2.0, cash_int_cast=True,
                     overhead=[1.0, 2.0, 1.0], limit=4.0, interest_free=1.0)
        out.append(Case(f"lead-deep-passes-{n_pairs}pair", "lead", kw, {"na": 676, "deep": True}))
    return out


def lead_wide_list():
    """64, 65 and 72 demand pairs (8 x 8, 13 x 5, 9 x 8): a wave stages its state's demand terms 64 pairs at a time."""
    out = []
    for (n1, n2), T, q_bound in (((8, 8), 2, 6), ((13, 5), 3, 2), ((9, 8), 2, 5), ((9, 8), 3, 2)):
        rng = np.random.default_rng(7800 + n1 * 16 + n2 + T)
        v1 = np.sort(rng.choice(np.arange(0, 16), size=n1, replace=False))
        v2 = np.sort(rng.choice(np.arange(0, 12), size=n2, replace=False))
        over = dict(cash_int_cast=True, min_cash=-20.0, max_cash=40.0, max_inventory=4.0) if T == 3 else {}
        kw = lead_kw(T, q_bound, [v1, v2], [dyadic(rng, n1, 64), dyadic(rng, n2, 32)], **over)
        out.append(Case(f"lead-wide-list-{n1}x{n2}-T{T}", "lead", kw, {"na": q_bound * q_bound, "pairs": n1 * n2}))
    return out


def lead_workgroup_form():
    """backward_kernel's lead-time branches (SDPGPU_MULTI_WAVE=0): NA / 256 order pairs a lane -- Qbound 16 (lead_actions<1>,
    exactly 256), 17 (<2>), 50 (<10>, 2500 of 2560) and 51 (2601: beyond 2560, one action at a time)."""
    out = []
    for q_bound in (16, 17, 50, 51):
        rng = np.random.default_rng(7900 + q_bound)
        hi = q_bound // 2
        v1 = np.sort(rng.choice(np.arange(1, hi + 1), size=2, replace=False))
        v2 = np.sort(rng.choice(np.arange(1, hi + 1), size=2, replace=False))
        kw = lead_kw(2, q_bound, [v1, v2], [dyadic(rng, 2, 16), dyadic(rng, 2, 16)], cash_int_cast=bool(q_bound % 2))
        out.append(Case(f"lead-workgroup-form-q{q_bound}", "lead", kw, {"na": q_bound * q_bound}))
    return out


BUILDERS = {"runs": runs, "irregular_lists": irregular_lists, "two_passes": two_passes, "wide_list": wide_list,
            "tables_beyond_lds": tables_beyond_lds, "lead_chunk_edges": lead_chunk_edges, "lead_deep_passes": lead_deep_passes,
            "lead_wide_list": lead_wide_list, "lead_workgroup_form": lead_workgroup_form}


def cases_of(builder):
    """[(case, kind)] of a builder: a cash instance once per family."""
    return [(c, k) for c in BUILDERS[builder]() for k in c.kinds]


# ---- the forms a solve can be put under, and the launch sites each must go through ---------------------------------
SWITCHES = ("SDPGPU_MULTI_LATTICE", "SDPGPU_MULTI_I32", "SDPGPU_MULTI_DENSE_GB", "SDPGPU_MULTI_FACT", "SDPGPU_MULTI_WAVE",
            "SDPGPU_MULTI_TRIPLES")
CASH_FORMS = {
    "default": {},
    "lattice": {"SDPGPU_MULTI_LATTICE": "1"},
    "lattice-64bit": {"SDPGPU_MULTI_LATTICE": "1", "SDPGPU_MULTI_I32": "0"},
    "lattice-ranks": {"SDPGPU_MULTI_LATTICE": "1", "SDPGPU_MULTI_DENSE_GB": "0"},
    "lattice-ranks-64bit": {"SDPGPU_MULTI_LATTICE": "1", "SDPGPU_MULTI_DENSE_GB": "0", "SDPGPU_MULTI_I32": "0"},
    "per-cell": {"SDPGPU_MULTI_FACT": "0"},
    "lattice-per-cell": {"SDPGPU_MULTI_LATTICE": "1", "SDPGPU_MULTI_FACT": "0"},
    "lattice-triples": {"SDPGPU_MULTI_LATTICE": "1", "SDPGPU_MULTI_TRIPLES": "1"},  # (multixr only)
}
LEAD_FORMS = {"default": {}, "workgroup": {"SDPGPU_MULTI_WAVE": "0"}}


def forms_of(case, kind):
    if case.family == "lead":
        return dict(LEAD_FORMS)
    return {n: e for n, e in CASH_FORMS.items() if kind == "multixr" or "SDPGPU_MULTI_TRIPLES" not in e}


def expected_forms(case, kind, env, bits):
    """The SDPGPU_MULTI_FORM_* mask (bits: name -> bit, _abi.MULTI_FORMS) a solve of `case` under the switches `env` must
    report: read off the launcher's rules (sparse_solve) for instances whose candidates stay below 2^31 a period, whose
    lattice box allows 32-bit index words and fits the dense-table budget -- every instance here."""
    kw = case.kw
    T, qb = kw["T"], kw["q_bound"]
    m = 0
    if case.family == "lead":
        wave = env.get("SDPGPU_MULTI_WAVE") != "0" and qb * qb <= 4096
        return bits["SORTED_FORWARD"] | (bits["LEAD_WAVE"] if wave else bits["BACKWARD"])
    lattice = env.get("SDPGPU_MULTI_LATTICE") == "1"
    fact = env.get("SDPGPU_MULTI_FACT") != "0"
    width = bits["FACT_I64"] if env.get("SDPGPU_MULTI_I32") == "0" else bits["FACT_I32"]
    dense = env.get("SDPGPU_MULTI_DENSE_GB") != "0"
    triples = env.get("SDPGPU_MULTI_TRIPLES") == "1" and kind == "multixr"
    beyond = case.claims.get("beyond_lds_period", -1)
    for t in range(T - 1):  # forward
        if not lattice:
            m |= bits["SORTED_FORWARD"]
        elif triples:
            m |= bits["TRIPLES_MARK"]
        elif fact and t != beyond:
            m |= bits["FACT_MARK"] | width
        else:
            m |= bits["LATTICE_MARK"]
    for t in range(T):  # backward
        if not fact or t == beyond:
            m |= bits["BACKWARD"]
        elif t == T - 1:
            m |= bits["FACT_LAST"]
        elif not lattice:
            m |= bits["FACT_UID"]
        elif dense:
            m |= bits["DENSE_SCATTER"] | bits["FACT_DENSE"] | width
        else:
            m |= bits["FACT_RANK"] | width
    return m


# ---- the oracle and the preconditions ----------------------------------------------------------------------------
def oracle_memo(oracle, case, kind):
    """-> (final value, action pair, states per period, cells, memo rows) of the oracle's literal memoised recursion."""
    kw = solver_kw(case, kind)
    if kind == "multilead":
        (fv, a1, a2, _, cells), table = oracle.memo_table("multilead", **kw)
    elif kind == "multicash":
        (fv, a1, a2, _, cells), table = oracle.memo_table("multicash", **kw)
    else:
        (fv, a1, a2, _, cells), table = oracle.memo_table("multixr", case.deposit, **kw)
    states = [int((table[:, 0] == t + 1).sum()) for t in range(kw["T"])]
    return fv, (a1, a2), states, cells, table


def preconditions(case, kind, states, cells, table):
    """{name: (holds, figures)}: what the builder's name claims, from the oracle's memo and host arithmetic."""
    kw, cl = case.kw, case.claims
    qb = kw["q_bound"]
    out = {"within_budget": (cells <= BUDGET_CELLS, f"{cells:.3g} cells")}
    if case.family == "lead":
        na, nd = qb * qb, len(kw["values"][0]) * len(kw["values"][1])
        out["na"] = (na == cl["na"], f"NA {na}: {-(-na // 64)} chunks, {-(-na // (64 * LEAD_CHUNKS))} wave passes, "
                                     f"{'one at a time' if na > 256 * ACT_PER_LANE else f'lead_actions<{-(-na // 256)}>'} in the workgroup form")
        if "pairs" in cl:
            out["pairs"] = (nd == cl["pairs"] and nd >= 64, f"{nd} demand pairs")
        if cl.get("deep"):
            multi = [s for s in states[1:-1] if s > 1]
            out["deep"] = (na > 64 * LEAD_CHUNKS and kw["T"] >= 3 and len(multi) > 0, f"not-last periods after the first hold {states[1:-1]} states of {na} actions")
        return out
    runs_ = [fact_run(fact_index_words(t)[0]) for t in kw["pmf"]]
    out["fact_run"] = (runs_ == cl["fact_run"], f"fact_run per period {runs_}")
    lds = []
    for t, rows in enumerate(kw["pmf"]):
        _, nu1, nu2 = fact_index_words(rows)
        lds.append((fact_lds_bytes(qb, len(rows), nu1 + nu2, t == kw["T"] - 1), fact_lds_bytes(qb, len(rows), nu1 + nu2, False, True)))
    if "beyond_lds_period" in cl:
        t = cl["beyond_lds_period"]
        ok = all((lds[u][0] > LDS_BYTES and lds[u][1] > LDS_BYTES) == (u == t) for u in range(kw["T"]))
        out["tables_beyond_lds"] = (ok, f"factored tables (backward, marking) per period {lds} B against {LDS_BYTES}")
    else:
        out["tables_fit_lds"] = (all(max(b) <= LDS_BYTES for b in lds), f"factored tables at most {max(max(b) for b in lds)} B")
    if "wide_period" in cl:
        nd = len(kw["pmf"][cl["wide_period"]])
        out["wide_list"] = (nd > FACT_THREADS, f"{nd} pairs in period {cl['wide_period'] + 1}")
    if cl.get("two_passes"):
        bound = pass_boundary(kind, qb)
        pos, n_off = best_positions(kind, kw, table)
        two = n_off > bound
        beyond, inside = int((two & (pos >= bound)).sum()), int((two & (pos < bound)).sum())
        out["two_passes"] = (beyond > 0 and inside > 0,
                             f"pass boundary {bound}: {int(two.sum())} states take two passes, best action beyond it for {beyond}, inside for {inside}")
        root = table[:, 0] == 1
        out["root"] = (kind != "multicash" or int(n_off[root][0]) > FACT_THREADS * FACT_NI,
                       f"root state offered {int(n_off[root][0])} pairs, best at position {int(pos[root][0])}")
        if kind == "multicash":
            out["carry_rows"] = (True, f"{qb} rows in the offered-row prefix sum ({'more than' if qb > 64 else 'within'} 64)")
        else:
            ts = (FACT_THREADS // qb) * qb
            out["idle_lanes"] = (True, f"{FACT_THREADS - ts} idle lanes of {FACT_THREADS}")
    return out


def check():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import sdpref
    sdpref.build()
    bad = 0
    for builder in BUILDERS:
        print(f"== {builder}: {BUILDERS[builder].__doc__.split(':')[0].strip().splitlines()[0]}")
        for case, kind in cases_of(builder):
            t0 = time.perf_counter()
            fv, act, states, cells, table = oracle_memo(sdpref, case, kind)
            dt = time.perf_counter() - t0
            pre = preconditions(case, kind, states, cells, table)
            ok = all(v[0] for v in pre.values())
            bad += not ok
            print(f"{case.name} [{kind}]: {cells} cells ({cells / BUDGET_CELLS:.2f} of the budget), {dt:.1f} s, states {states}, "
                  f"value {fv!r}, action {act} -- {'ok' if ok else 'PRECONDITION FAILS'}")
            for name, (holds, what) in pre.items():
                print(f"    {'ok  ' if holds else 'FAIL'} {name}: {what}")
    print("every instance within budget, every precondition true" if not bad else f"{bad} instances fail")
    return 1 if bad else 0


if __name__ == "__main__":
    if "--check" in sys.argv:
        sys.exit(check())
    print(__doc__)
