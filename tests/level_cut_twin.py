"""Independent twin of the cut-off of the F1 level kernel (window_f1_level_kernel<4, 8, ..., CUT>, DESIGN 4, "The level
kernel's cut-off"): plain numpy written from the kernel's description, with none of the library's code.  Scope: the
built-in CLSP costs, MIN, step 1, the default clamp, a unit-stride support from 0 -- the instances of _grid() in
test_level_cutoff.py.

One period at a time, from the instance, V_{t+1} (None for period T) and the plan (band, action blocks, padded demand
steps).  A task is (band of `band` levels, block of 256 actions) and walks its level blocks of 8 levels in order; the twin
walks all tasks of a slab of bands together, vectorised over levels and actions, one demand step after the other:

  * U(i) = Q(i, 0), every sum from +0.0 with j ascending, `acc += p * imm` and then `acc += p * V` as two rounded operations,
    padded steps with p = 0;
  * the test schedule of a task -- cut_start = max(8, D // 2 // 8 * 8), a test every 8 steps from cut_at on, cut_dec,
    cut_first and cut_once carried from one level block to the next exactly as the kernel carries them;
  * the test itself: every cell that is a real action other than action 0 must be STRICTLY above its state's slot; the slots
    start at U(i), or at -inf where they belong to no state of the slab;
  * a block that stops is dropped with its epilogue -- the twin does not compute its remaining steps either; a block that
    runs to the end goes into the slots under the strict <, level after level (for one state that is action ascending);
  * the pieces of a state are merged across tasks by the reference's rule, the lowest action among equal values.

What comes out are the period's tables, the steps run and the tests made per task, and how the stops are spread over the
blocks of a task.  The three keyword switches of twin_period() turn the twin into a kernel that is WRONG in one known way
(they are never set by a test that compares with the GPU): they show that the step count tells such a kernel apart."""
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np

LV = 8          # levels per level block, and steps between two tests
NA = 256        # actions per task
INT_MAX = 2**31 - 1
DBL_MAX = 1.7976931348623157e308


def plan_geometry(pl, S, A, D):
    """(band, action blocks, padded demand steps) of a level plan as sdpgpu_plan_period reports it: the band is the
    multiple of 8 whose number of bands over the S + A - 1 levels is `tiles`."""
    assert pl.chunk_blocks == 0 and (pl.r, pl.s) == (4, LV), "not a level plan"
    nb = -(-A // NA)
    assert pl.tasks == pl.tiles * nb
    ny = S + A - 1
    band = -(-(-(-ny // pl.tiles)) // LV) * LV
    while -(-ny // band) != pl.tiles:
        band -= LV
        assert band > 0
    return band, nb, -(-D // LV) * LV


def planned_steps(S, A, band, nb, d_pad):
    """The host's count: level blocks of every band x action blocks x padded steps."""
    ny = S + A - 1
    blocks = sum(-(-(min(yb + band, ny) - yb) // LV) for yb in range(0, ny, band))
    return blocks * nb * d_pad


def _level_cost(level, h, pi):
    return h * np.maximum(level, 0.0) + pi * np.maximum(-level, 0.0)


def u_row(S, x_lo, h, pi, p, v_next):
    """U(i) = Q(i, 0): action 0 costs c0 = +0.0, the level cost of i - j, then the future value, j ascending."""
    i = np.arange(S)
    acc = np.zeros(S)
    for j, pj in enumerate(p):
        m = i - j
        acc += pj * (0.0 + _level_cost(x_lo + m.astype(np.float64), h, pi))
        if v_next is not None:
            acc += pj * v_next[np.clip(m, 0, S - 1)]
    return acc


@dataclass
class PeriodTwin:
    values: np.ndarray
    policy: np.ndarray
    steps: np.ndarray          # [bands, action blocks]: steps run by the task
    tests: np.ndarray          # [bands, action blocks]: tests made by the task
    planned: int
    blocks: int = 0            # level blocks walked or stopped
    stopped: int = 0           # ... that stopped
    stopped_later: int = 0     # ... that stopped and were not the first block of their task
    stopped_second_table: int = 0   # ... that stopped at step 64 or later (the second product table)
    rearmed_tasks: int = 0     # tasks in which a block ran to the end after an earlier block of the task had stopped
    never_stopped_tasks: int = 0
    always_stopped_tasks: int = 0
    stop_hist: dict = field(default_factory=dict)

    @property
    def run(self):
        return int(self.steps.sum())


def _slab(args):
    (b0, b1, ab, S, A, x_lo, K, v, h, pi, pp, v_next, U, band, d_pad, cut_start, slot_shift, keep_once, edge_fill) = args
    ny = S + A - 1
    kb = ab * NA
    width = min(NA, A - kb)
    k = kb + np.arange(width)
    c0 = np.where(k > 0, K, 0.0) + v * k.astype(np.float64)
    live = k != 0                                # (every k here is a real action)
    nB = b1 - b0
    yb = (b0 + np.arange(nB)) * band
    ye = np.minimum(yb + band, ny)
    nblk = -(-(ye - yb) // LV)
    n_slot = ye - yb + NA - 1
    # slot q of a task holds state i_min + q; one spare slot past the end for the slot_shift switch
    i_slot = (yb - kb - NA + 1)[:, None] + np.arange(band + NA + 1)[None, :]
    in_slab = (i_slot >= 0) & (i_slot < S)
    outside = -np.inf if edge_fill is None else U[np.clip(i_slot, 0, S - 1)]
    sval = np.where(in_slab, U[np.clip(i_slot, 0, S - 1)], outside)
    sval[:, band + NA] = 0.0
    sidx = np.zeros(sval.shape, dtype=np.int32)
    cut_first = np.full(nB, cut_start, dtype=np.int64)
    cut_dec = np.full(nB, LV, dtype=np.int64)
    cut_once = np.zeros(nB, dtype=bool)
    steps = np.zeros(nB, dtype=np.int64)
    tests = np.zeros(nB, dtype=np.int64)
    had_stop = np.zeros(nB, dtype=bool)
    had_run = np.zeros(nB, dtype=bool)
    rearmed = np.zeros(nB, dtype=bool)
    stat = dict(blocks=0, stopped=0, later=0, second=0)
    hist = {}
    s_ar = np.arange(LV)
    a_ar = np.arange(width)
    for q in range(int(nblk.max())):
        tk = np.flatnonzero(nblk > q)            # the tasks that have this level block
        n = len(tk)
        y0 = yb[tk] + LV * q
        q_of = LV * q + s_ar[:, None] - a_ar[None, :] + NA - 1      # slot of cell (s, a)
        slot = sval[tk][:, q_of + slot_shift]                       # [n, 8, width]
        # level m = y0 + s - j runs over y0 - d_pad + 1 .. y0 + 7: column u holds level y0 - d_pad + 1 + u
        lev = (y0 - d_pad + 1)[:, None] + np.arange(d_pad + LV - 1)[None, :]
        m_cost = _level_cost(x_lo + lev.astype(np.float64), h, pi)
        v_lev = None if v_next is None else v_next[np.clip(lev, 0, S - 1)]
        acc = np.zeros((n, LV, width))
        cur = np.arange(n)                       # rows of acc <-> tasks tk[cur] still walking
        cut_at = cut_first[tk].copy()
        once = cut_once[tk]
        fail = np.zeros(n, dtype=np.int64)
        stop = np.full(n, -1, dtype=np.int64)
        for jj in range(0, d_pad, LV):
            testing = np.flatnonzero(jj >= cut_at[cur])
            if len(testing):
                g = cur[testing]
                tests[tk[g]] += 1
                beaten = ((acc[testing] > slot[g]) | ~live).all(axis=(1, 2))
                stop[g[beaten]] = jj
                gf = g[~beaten]
                fail[gf] += 1
                cut_at[gf] = np.where(once[gf], INT_MAX, jj + LV)
                if beaten.any():
                    keep = np.ones(len(cur), dtype=bool)
                    keep[testing[beaten]] = False
                    cur = cur[keep]
                    acc = acc[keep]
                    if not len(cur):
                        break
            for j in range(jj, jj + LV):
                pj = pp[j]
                u0 = d_pad - 1 - j
                imm = c0[None, None, :] + m_cost[cur, u0:u0 + LV][:, :, None]
                imm *= pj
                acc += imm
                if v_lev is not None:
                    acc += (pj * v_lev[cur, u0:u0 + LV])[:, :, None]
        ran = stop < 0
        steps[tk] += np.where(ran, d_pad, stop)
        stat["blocks"] += n
        stat["stopped"] += int((~ran).sum())
        stat["second"] += int((stop >= 64).sum())
        if q > 0:
            stat["later"] += int((~ran).sum())
        for sv, cnt in zip(*np.unique(stop[~ran], return_counts=True)):
            hist[int(sv)] = hist.get(int(sv), 0) + int(cnt)
        rearmed[tk] |= ran & had_stop[tk]
        had_stop[tk] |= ~ran
        had_run[tk] |= ran
        dec = np.where(ran, LV, np.where(fail == 0, np.minimum(2 * cut_dec[tk], 8 * LV), LV))
        cut_dec[tk] = dec
        cut_first[tk] = np.where(ran, max(LV, d_pad - LV), np.maximum(LV, stop - dec))
        cut_once[tk] = np.where(ran, True, once if keep_once else False)
        # the epilogue of the blocks that ran to the end: level after level, strict <
        g = tk[cur]
        for s in range(LV):
            qs = q_of[s]
            state = (y0[cur] + s)[:, None] - k[None, :]
            old = sval[g[:, None], qs[None, :]]
            new = acc[:, s, :]
            upd = (state >= 0) & (state < S) & (new < old)
            sval[g[:, None], qs[None, :]] = np.where(upd, new, old)
            sidx[g[:, None], qs[None, :]] = np.where(upd, k[None, :], sidx[g[:, None], qs[None, :]])
    # the pieces: every state of the task's range that has a real action here
    kf = np.maximum(kb, yb[:, None] - i_slot)
    piece = in_slab & (kf < A) & (np.arange(band + NA + 1)[None, :] < n_slot[:, None])
    return (b0, ab, i_slot, piece, sval, sidx, steps, tests, stat, hist, int(rearmed.sum()), int((~had_stop).sum()),
            int((~had_run).sum()))


def twin_period(S, A, x_lo, K, v, h, pi, p, v_next, band, n_ablocks, d_pad, *, threads=8, slot_shift=0, keep_once=False,
                edge_fill=None):
    """One period of the level kernel with the cut-off.  p: the probabilities of demands 0 .. D - 1; v_next: V_{t+1} over the
    same S states, None for period T.  slot_shift / keep_once / edge_fill: see the module's docstring."""
    p = np.asarray(p, dtype=np.float64)
    D = len(p)
    assert d_pad == -(-D // LV) * LV and band % LV == 0 and n_ablocks == -(-A // NA)
    pp = np.concatenate([p, np.zeros(d_pad - D)])
    if v_next is not None:
        v_next = np.ascontiguousarray(v_next, dtype=np.float64)
        assert v_next.shape == (S,)
    U = u_row(S, x_lo, h, pi, p, v_next)
    ny = S + A - 1
    n_bands = -(-ny // band)
    cut_start = max(LV, D // 2 // LV * LV)
    jobs = []
    for ab in range(n_ablocks):
        width = min(NA, A - ab * NA)
        per = max(1, (1 << 17) // (LV * width))   # bands per slab: arrays of about 1 MiB
        for b0 in range(0, n_bands, per):
            jobs.append((b0, min(b0 + per, n_bands), ab, S, A, x_lo, K, v, h, pi, pp, v_next, U, band, d_pad, cut_start,
                         slot_shift, keep_once, edge_fill))
    if threads > 1 and len(jobs) > 1:
        with ThreadPoolExecutor(threads) as pool:
            done = list(pool.map(_slab, jobs))
    else:
        done = [_slab(j) for j in jobs]
    out = PeriodTwin(values=np.full(S, DBL_MAX), policy=np.zeros(S, dtype=np.int32),
                     steps=np.zeros((n_bands, n_ablocks), dtype=np.int64), tests=np.zeros((n_bands, n_ablocks), dtype=np.int64),
                     planned=planned_steps(S, A, band, n_ablocks, d_pad))
    # merge in action order: action blocks ascending, bands ascending; a later piece wins only when strictly lower
    for (b0, ab, i_slot, piece, sval, sidx, steps, tests, stat, hist, rearmed, never, always) in sorted(done, key=lambda r: (r[1], r[0])):
        nB = len(steps)
        out.steps[b0:b0 + nB, ab] = steps
        out.tests[b0:b0 + nB, ab] = tests
        out.blocks += stat["blocks"]
        out.stopped += stat["stopped"]
        out.stopped_later += stat["later"]
        out.stopped_second_table += stat["second"]
        out.rearmed_tasks += rearmed
        out.never_stopped_tasks += never
        out.always_stopped_tasks += always
        for sv, cnt in hist.items():
            out.stop_hist[sv] = out.stop_hist.get(sv, 0) + cnt
        for r in range(nB):
            sel = piece[r]
            i = i_slot[r][sel]
            val = sval[r][sel]
            better = val < out.values[i]
            out.values[i[better]] = val[better]
            out.policy[i[better]] = sidx[r][sel][better]
    return out


@dataclass
class SolveTwin:
    periods: list              # PeriodTwin of period 1 .. T
    band: int
    n_ablocks: int
    d_pad: int

    @property
    def planned(self):
        return sum(p.planned for p in self.periods)

    @property
    def run(self):
        return sum(p.run for p in self.periods)

    @property
    def walked(self):
        return self.run / self.planned

    @property
    def blocks_per_task(self):
        return self.band // LV

    @property
    def carried_share(self):
        """The share of the stopped blocks that were not the first block of their task."""
        stopped = sum(p.stopped for p in self.periods)
        return sum(p.stopped_later for p in self.periods) / stopped if stopped else 0.0

    @property
    def rearmed_tasks(self):
        return sum(p.rearmed_tasks for p in self.periods)


def twin_solve(w, pl, V, **kw):
    """Every period of workload `w` (a BackorderFunctor inside the twin's scope) under the level plan `pl`, each from the
    given row V[t] of the period above (V: the reference's values of periods 1 .. T)."""
    f = w.functor
    S = int(f.maxInventory - f.minInventory) + 1
    A = int(f.maxOrderQuantity) + 1
    geo = None
    periods = []
    for t in range(w.T):
        tile = np.asarray(w.pmf[t], dtype=np.float64)
        D = len(tile)
        assert np.array_equal(tile[:, 0], np.arange(D)), "the twin's scope: demands 0, 1, .., D - 1"
        g = plan_geometry(pl, S, A, D)
        assert geo in (None, g), "one plan for every period"
        geo = g
        periods.append(twin_period(S, A, float(f.minInventory), float(f.fixedOrderingCost), float(f.variOrderingCost),
                                   float(f.holdingCost), float(f.penaltyCost), tile[:, 1], V[t + 1] if t + 1 < w.T else None,
                                   *geo, **kw))
    return SolveTwin(periods, *geo)


# ---------------------------------------------------------------------------------------------------------------
# The grids of the cut-off tests, with what the twin counts on them (tests/test_level_cut_twin.py checks every figure on the
# CPU; the GPU tests of test_level_cutoff.py / test_gpu_level_fuzz.py hold the device counters against the same figures).
# S states x A actions x D demands, T periods of seasonal_pmf, inventory from `lo` up, costs K / v / h / pi.
# blocks: level blocks per task of the plan; run: steps run, period 1 .. T.
# ---------------------------------------------------------------------------------------------------------------
def _case(id, S, A, D, T, lo, K, h, blocks, run, v=1.0, pi=10.0):
    return dict(id=id, S=S, A=A, D=D, T=T, lo=lo, K=K, v=v, h=h, pi=pi, blocks=blocks, run=run)


# One level block per task (the grids of test_cutoff_fires_and_changes_nothing): nothing is carried from block to block.
ONE_BLOCK_GRIDS = [
    _case("A500-D200", 1601, 500, 200, 3, 0, 500.0, 2.0, 1, [72200, 53744, 58424]),
    _case("A300-D40", 900, 300, 40, 3, 0, 500.0, 2.0, 1, [8656, 6336, 6784]),
    _case("A130-D16", 700, 130, 16, 3, 0, 500.0, 2.0, 1, [1664, 1352, 1448]),
    _case("A300-D21-neg", 2000, 300, 21, 3, -700, 500.0, 2.0, 1, [11824, 10112, 10320]),
]

# Several level blocks per task.  The holding cost is small against K / i, so that blocks of high inventory stop, early or
# late with the level; the slab reaches below zero, where orders win and blocks run to the end.
MULTI_BLOCK_GRIDS = [
    # ragged last band: 19 levels, the third block of its tasks has three levels of the slab
    _case("40000x300x24", 40000, 300, 24, 2, -200, 500.0, 0.2, 5, [222664, 205168]),
    # one action block, half of its lanes real
    _case("66000x130x16", 66000, 130, 16, 2, -200, 500.0, 0.01, 5, [111328, 90256]),
    # a third action block with one real lane
    _case("30000x513x24", 30000, 513, 24, 2, -400, 500.0, 0.25, 6, [243616, 218360]),
    # a second action block with one real lane (20000 states plan three blocks per task: 26000 for the four asked for)
    _case("26000x257x9", 26000, 257, 9, 3, -150, 500.0, 0.5, 4, [94312, 52816, 59048]),
    # lanes of r = 0 only
    _case("50000x64x17", 50000, 64, 17, 3, -50, 500.0, 0.15, 4, [110336, 97128, 98072]),
    # D > 64: blocks stop in the second product table (j0 = 64)
    _case("25000x300x100", 25000, 300, 100, 2, -300, 500.0, 0.2, 4, [393656, 379496]),
    # a third of the slab below zero: bands that never stop, bands that always do
    _case("36000x300x32-deep", 36000, 300, 32, 2, -12000, 500.0, 0.1, 5, [236032, 230400]),
]
