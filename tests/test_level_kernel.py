"""The action-major F1 level kernel (window_f1_level_kernel, SDPGPU_WIN_LEVEL): its plans, the task -> cell mapping (host
arithmetic, no GPU), and its tables against the state-major window_f1_kernel and the oracle on odd shapes (GPU)."""
import numpy as np
import pytest

from stochastic_inventory_amd import workloads
from stochastic_inventory_amd.functors import BackorderFunctor
from stochastic_inventory_amd.states import OptDirection

_SWITCHES = ("SDPGPU_WIN_R", "SDPGPU_WIN_S", "SDPGPU_WIN_NCH", "SDPGPU_WIN_LEVEL")


def _grid(S, A, D, T=3, direction=OptDirection.MIN, flat=False, K=500.0, lo=0):
    if flat:
        f = BackorderFunctor(fixedOrderingCost=0, variOrderingCost=0, holdingCost=0, penaltyCost=0,
                             minInventory=lo, maxInventory=lo + S - 1, maxOrderQuantity=A - 1, iniInventory=lo)
    else:
        f = BackorderFunctor(fixedOrderingCost=K, variOrderingCost=1, holdingCost=2, penaltyCost=10,
                             minInventory=lo, maxInventory=lo + S - 1, maxOrderQuantity=A - 1, iniInventory=lo)
    return workloads.Workload(f"lvl_{S}x{A}x{D}x{T}", f, direction, workloads.seasonal_pmf(T, D), "level kernel test")


def _engine(sia, w, monkeypatch, level, world=1, rank=0, **kw):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if level is not None:
        monkeypatch.setenv("SDPGPU_WIN_LEVEL", str(level))
    d = w.desc()
    d.world_size, d.rank = world, rank
    if "custom_source" in kw:
        return sia.SdpEngine(d, w.pmf, **kw)
    return sia.SdpEngine(d, w.pmf, w.overhead(), **kw)


def _cells(S, A, pl):
    """The kernel's task -> cell map, as window_f1_level_kernel computes it: (state, action) of every real cell of every
    task, and the chunk row the task's piece of each state goes to (plus the rows it marks as holding no piece)."""
    R, band, nb = pl.r, None, pl.tasks // pl.tiles
    assert pl.chunk_blocks == 0 and nb == -(-A // (64 * R))
    ny = S + A - 1
    band = -(-ny // pl.tiles)
    band = -(-band // pl.s) * pl.s
    # the plan's band is the one whose count of bands is `tiles`; search the multiple of S that gives it
    while -(-ny // band) != pl.tiles or band % pl.s:
        band -= pl.s
        assert band > 0
    seen = np.zeros((S, A), dtype=np.int32)
    rows = {}  # state -> {row: (lowest action, highest action)}
    nan_rows = {}
    for task in range(pl.tasks):
        ab, b = task % nb, task // nb
        kb = ab * 64 * R
        yb, ye = b * band, min((b + 1) * band, ny)
        # cell (lane, r, s) of level block y0: level y0 + s, action kb + lane + 64 r
        y = np.arange(yb, yb + -(-(ye - yb) // pl.s) * pl.s)[:, None]
        k = (kb + np.arange(64 * R))[None, :]
        i = y - k
        real = (k < A) & (i >= 0) & (i < S)
        assert np.all(y[np.any(real, axis=1)] < ye)
        np.add.at(seen, (np.broadcast_to(i, real.shape)[real], np.broadcast_to(k, real.shape)[real]), 1)
        for i in range(yb - kb - 64 * R + 1, ye - kb):
            kf = max(kb, yb - i)
            if not (0 <= i < S) or kf >= A:
                continue
            c = (b - i // band) + ab
            kl = min(kb + 64 * R - 1, ye - 1 - i, A - 1)
            assert c < pl.chunks and c not in rows.setdefault(i, {})
            rows[i][c] = (kf, kl)
            if kb > 0 and yb - i == kb:
                nan_rows.setdefault(i, set()).add(c - 1)
    return seen, rows, nan_rows


@pytest.mark.parametrize("S,A,D", [(300, 37, 13), (2000, 300, 21), (1601, 500, 200), (5000, 777, 9)])
def test_level_task_map_covers_every_pair_once(sia, monkeypatch, S, A, D):
    """Every (state, action) pair of the slab is one cell of one task; a state's pieces sit in chunk rows whose order is
    their action order, starting at row 0, and a row skipped between two pieces is marked (NaN) by the later piece."""
    w = _grid(S, A, D, T=2)
    with _engine(sia, w, monkeypatch, 1) as eng:
        pl = eng.plan(1)
    assert pl.kernel == 2 and pl.chunk_blocks == 0 and (pl.r, pl.s) == (4, 8) and pl.chunks >= 2
    assert pl.lds_bytes <= 65536 and pl.workgroups_per_cu >= 2
    seen, rows, nan_rows = _cells(S, A, pl)
    assert seen.min() == 1 and seen.max() == 1
    for i in range(S):
        got = sorted(rows[i].items())
        assert got[0][0] == 0 and got[0][1][0] == 0 and got[-1][1][1] == A - 1
        for (c0, (a0, b0)), (c1, (a1, b1)) in zip(got, got[1:]):
            assert a1 == b0 + 1  # consecutive action runs in ascending rows
            assert set(range(c0 + 1, c1)) <= nan_rows.get(i, set())


def test_level_plan_choice(sia, monkeypatch):
    """The planner takes the level kernel for the target grid by itself, and keeps window_f1_kernel where it cannot run
    (ping-pong tables, ranks of a sharded slab) or does not win (small grids, SDPGPU_WIN_LEVEL=0, forced blocks)."""
    with _engine(sia, workloads.target_grid(T=2), monkeypatch, None) as eng:
        pl = eng.plan(1)
    assert pl.chunk_blocks == 0 and (pl.r, pl.s) == (4, 8) and pl.tasks % 2 == 0 and pl.tasks <= 4096
    assert pl.lds_bytes <= 65536 and pl.workgroups_per_cu == 2
    with _engine(sia, workloads.target_grid(T=2), monkeypatch, 0) as eng:
        assert eng.plan(1).chunk_blocks > 0
    with _engine(sia, workloads.cfg2_clsp(T=2), monkeypatch, None) as eng:
        assert eng.plan(1).chunk_blocks > 0
    for rank in range(2):
        with _engine(sia, _grid(3000, 300, 20), monkeypatch, 1, world=2, rank=rank) as eng:
            assert eng.plan(1).chunk_blocks > 0
    w = workloads.cfg5_scaled(S=1601, T=2)
    d = w.desc()
    d.store_all_values = 0
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDPGPU_WIN_LEVEL", "1")
    with sia.SdpEngine(d, w.pmf, w.overhead()) as eng:
        assert eng.plan(1).chunk_blocks > 0


def _tables(eng, T):
    return [(eng.values(t), eng.policy(t)) for t in range(1, T + 1)]


def _check_pair(sia, oracle, monkeypatch, w, with_oracle=True, **kw):
    out = {}
    for level in (1, 0):
        with _engine(sia, w, monkeypatch, level, **kw) as eng:
            assert (eng.plan(1).chunk_blocks == 0) == (level == 1)
            eng.solve(sync=True)
            out[level] = _tables(eng, w.T)
    for t, ((v1, p1), (v0, p0)) in enumerate(zip(out[1], out[0]), start=1):
        assert np.array_equal(v1, v0) and np.array_equal(p1, p0), f"{w.name} period {t}: level kernel != window_f1_kernel"
    if with_oracle:
        V, pol, _ = oracle.Problem(w.desc(), w.pmf, w.overhead()).solve(nthreads=8)
        for t in range(w.T):
            assert np.array_equal(out[1][t][0], V[t]) and np.array_equal(out[1][t][1], pol[t]), f"{w.name} period {t + 1}"


@pytest.mark.gpu
@pytest.mark.parametrize("S,A,D,direction,flat,lo", [
    (300, 37, 13, OptDirection.MIN, False, 0),        # A < 64, D not a multiple of 8
    (2000, 300, 21, OptDirection.MIN, False, -700),   # A not a multiple of 256, backorders below 0
    (2000, 300, 21, OptDirection.MAX, False, 0),      # MAX
    (1601, 500, 200, OptDirection.MIN, False, 0),     # the target's actions and demands, ragged slab
    (900, 130, 16, OptDirection.MIN, True, 0),        # flat costs: every action ties
    (900, 130, 16, OptDirection.MAX, True, -300),
], ids=["A37-D13", "A300-D21-neg", "A300-D21-max", "A500-D200", "flat-min", "flat-max"])
def test_level_kernel_matches_window_kernel_and_oracle(sia, oracle, monkeypatch, S, A, D, direction, flat, lo):
    _check_pair(sia, oracle, monkeypatch, _grid(S, A, D, direction=direction, flat=flat, lo=lo))


@pytest.mark.gpu
def test_level_kernel_low_fixed_cost_ties(sia, oracle, monkeypatch):
    """No fixed cost and a zero variable cost on a flat pmf tail: many exact ties between actions of one state."""
    f = BackorderFunctor(fixedOrderingCost=0, variOrderingCost=0, holdingCost=1, penaltyCost=1, minInventory=0,
                         maxInventory=1199, maxOrderQuantity=399, iniInventory=0)
    pmf = [np.column_stack([np.arange(8.0), np.full(8, 0.125)]) for _ in range(3)]
    w = workloads.Workload("lvl_ties_1200x400x8x3", f, OptDirection.MIN, pmf, "ties")
    _check_pair(sia, oracle, monkeypatch, w)


@pytest.mark.gpu
def test_level_kernel_level_shape_tables(sia, monkeypatch):
    """User lambdas of the level shape (m_tab / c_tab) on the level kernel against the same text on window_f1_kernel."""
    w = workloads.custom_clsp_level(T=3, S=3000, A=300, D=40)
    _check_pair(sia, None, monkeypatch, w, with_oracle=False, custom_source=w.custom_source, custom_params=w.custom_params)


@pytest.mark.gpu
def test_level_kernel_target_period(sia, monkeypatch):
    """The target's full-size shape (1e6 x 500 x 200), two periods: the automatic plan (the level kernel) against
    window_f1_kernel, every state bit for bit."""
    w = workloads.target_grid(T=2)
    out = {}
    for level in (None, 0):
        with _engine(sia, w, monkeypatch, level) as eng:
            assert (eng.plan(1).chunk_blocks == 0) == (level is None)
            eng.solve(sync=True)
            out[level] = _tables(eng, w.T)
    for (v1, p1), (v0, p0) in zip(out[None], out[0]):
        assert np.array_equal(v1, v0) and np.array_equal(p1, p0)
