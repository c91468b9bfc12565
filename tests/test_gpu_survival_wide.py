"""The survival family (F6) on WIDE cash rows: 1024-2600 cash points (16 and more 64-point tiles: the band numbering and the
band interleave of the cash row kernel), all four quantisers -- (mult 1, long division), (10, double division), (10, long
division: the INTDIV instantiation, whose key is not the rounded balance) and (100, double division: `dead = key < 0` on a key
that is not the balance in units) -- with an order bound that binds over much of the row.  make_instance(6, ...) of
tests/test_gpu_fuzz.py stays on integer cash and rows of at most 131 points."""
import math
import zlib

import numpy as np
import pytest

import scrambled
from stochastic_inventory_amd.functors import SurvivalFunctor
from stochastic_inventory_amd.states import OptDirection
from stochastic_inventory_amd.workloads import Workload

pytestmark = pytest.mark.gpu

QUANTISERS = [(1.0, True), (10.0, False), (10.0, True), (100.0, False)]  # (mult = div, long division), by seed % 4


def make_wide_survival_instance(seed):
    """T = 2-4; quantiser by seed % 4; 1024-2600 cash points, the axis reaching below zero in two seeds of three; 10-39 orders;
    variCost ~ maxCash / (U(2, 4) * maxQ), so that the cash bound on the order binds over much of the row; price = variCost *
    U(1.5, 3); a demand support whose top lies in maxQ / 2 .. maxQ (with gaps in one instance of three); a period's overhead
    = (price - variCost) * E[d] * U(0.7, 1.3), so that survival is neither certain nor hopeless; fixed cost, holding cost, deposit
    rate 0 / 0.02 and gamma 1 / 0.97 at random.  All money in hundredths."""
    rng = np.random.default_rng(660000 + seed)
    T = int(rng.integers(2, 5))
    mult, long_div = QUANTISERS[seed % 4]
    per_unit = 1.0 if long_div else mult  # cash keys per unit of money
    nc = int(rng.integers(1024, 2601))
    below = int(nc * rng.uniform(0.05, 0.25)) if seed % 3 else 0
    min_cash, max_cash = -below / per_unit, (nc - 1 - below) / per_unit
    cents = lambda v: float(max(round(v * 100), 0)) / 100  # noqa: E731
    max_q = int(rng.integers(10, 40))
    vari = max(0.01, cents(max_cash / (rng.uniform(2, 4) * max_q)))
    price = cents(vari * rng.uniform(1.5, 3))
    pmf, overheads = [], []
    for _ in range(T):
        top = int(rng.integers(max_q // 2, max_q + 1))
        n = int(rng.integers(4, min(top + 1, 24) + 1))
        if seed % 3 == 1:
            d = np.append(np.sort(rng.choice(np.arange(top), size=n - 1, replace=False)), top).astype(np.float64)
        else:
            d = np.arange(top - n + 1, top + 1, dtype=np.float64)
        p = rng.random(n) + 0.05
        p /= p.sum()
        pmf.append(np.stack([d, p], axis=1))
        overheads.append(cents((price - vari) * float(np.dot(d, p)) * rng.uniform(0.7, 1.3)))
    f = SurvivalFunctor(price=price, fixOrderCost=float(rng.choice([0.0, cents(rng.uniform(0, 3 * vari))])), variCost=vari,
                        holdingCost=float(rng.choice([0.0, cents(rng.uniform(0, 0.2 * vari))])),
                        depositeRate=float(rng.choice([0, 0.02])), salvageValue=cents(rng.uniform(0, 0.5 * vari)),
                        discountFactor=float(rng.choice([1.0, 0.97])), maxOrderQuantity=float(max_q), minInventoryState=0.0,
                        maxInventoryState=float(rng.integers(3, 9)), minCashState=min_cash, maxCashState=max_cash,
                        iniInventory=0.0, iniCash=math.floor(max_cash * rng.uniform(0.2, 0.5) * per_unit) / per_unit,
                        cashRoundMult=mult, cashRoundDiv=mult, cashRoundIntDiv=long_div, overheadCosts=overheads)
    return Workload(f"fuzz_wide_f6_{seed}", f, OptDirection.MAX, pmf)


# twelve of the seeds 0-19 that meet _reference's condition, three per quantiser (2, 5, 8, 12, 15 and 18 do not: fewer than 16
# distinct values in V_1, or under 5 % of the period-1 states ordering)
SEEDS = [0, 1, 3, 4, 6, 7, 9, 10, 11, 13, 14, 16]
FOUR = [0, 1, 10, 11]  # one per quantiser, 7 or 8 inventory rows: neither 3 nor 5 slabs end on a row


def _reference(oracle, seed):
    """The oracle's tables (shared through scrambled.reference) of an instance that meets the condition on the instances kept:
    in period 1 at least 5 % of the states order something and V_1 has at least 16 distinct values."""
    w = make_wide_survival_instance(seed)
    ref = scrambled.reference(oracle, w)
    assert 1024 <= ref["P"].grids[0].nc <= 2600, w.name
    assert np.mean(ref["pol"][0] > 0) >= 0.05 and len(np.unique(ref["V"][0])) >= 16, w.name
    return w, ref


VARIANTS = [("auto", {}), ("generic", {}), ("row-major", {"SDPGPU_CASH_BANDS": "0"}), ("three-bands", {"SDPGPU_CASH_BANDS": "3"}),
            ("contiguous-bands", {"SDPGPU_CASH_BAND_INTERLEAVE": "0"})]


@pytest.mark.parametrize("seed", SEEDS)
def test_wide_survival_rows_bit_exact(sia, oracle, monkeypatch, seed):
    """Whole solves: the cash row kernel (banded with interleaved bands, row-major, three bands per XCD, contiguous bands) and
    the generic kernel against the oracle, every table bit for bit, and the cell count."""
    w, ref = _reference(oracle, seed)
    for name, env in VARIANTS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            d = w.desc()
            d.kernel = 1 if name == "generic" else 0
            with sia.SdpEngine(d, w.pmf, w.overhead()) as eng:
                eng.solve()
                assert eng.stats().kernel_used == (1 if name == "generic" else 2), f"{w.name} {name}"
                assert eng.stats().cells_evaluated == ref["cells"], f"{w.name} {name}"
                for period in range(1, w.T + 1):
                    assert np.array_equal(eng.policy(period), ref["pol"][period - 1]), f"{w.name} {name} t={period}: policy"
                    assert np.array_equal(eng.values(period), ref["V"][period - 1]), f"{w.name} {name} t={period}: values"


@pytest.mark.parametrize("kernel", [0, 1], ids=["auto", "generic"])
@pytest.mark.parametrize("seed", sorted(scrambled.kept("wide_survival")))
def test_wide_survival_rows_on_scrambled_successor_tables(sia, oracle, seed, kernel):
    w, _ = _reference(oracle, seed)
    used = scrambled.run_scrambled(sia, oracle, w, kernel=kernel, periods=scrambled.kept("wide_survival")[seed])
    assert used == (1 if kernel else 2), w.name


@pytest.mark.parametrize("world", [3, 5])
@pytest.mark.parametrize("seed", FOUR)
def test_wide_survival_rows_in_slabs(sia, oracle, seed, world):
    """sdpgpu_solve_multi with 3 and 5 ranks: the cuts fall inside rows and inside tiles."""
    w, ref = _reference(oracle, seed)
    engs = []
    try:
        for r in range(world):
            d = w.desc()
            d.rank, d.world_size, d.device = r, world, 0
            engs.append(sia.SdpEngine(d, w.pmf, w.overhead()))
        sia.SdpEngine.solve_multi(engs, sync=True, gather_first=True)
        cuts = set()
        for r, e in enumerate(engs):
            assert e.stats().kernel_used == 2, f"{w.name} rank {r}/{world}"
            for period in range(1, w.T + 1):
                _, lo, hi = e.slab(period)
                cuts.add(lo % ref["P"].grids[period - 1].nc)
                assert np.array_equal(e.values(period), ref["V"][period - 1]), f"{w.name} rank {r}/{world}: V_{period}"
                assert np.array_equal(e.policy(period), ref["pol"][period - 1][lo:hi]), f"{w.name} rank {r}/{world}: policy of period {period}"
        assert any(c % 64 for c in cuts), cuts  # (a cut inside a row and inside a 64-point tile)
    finally:
        for e in engs:
            e.close()


@pytest.mark.parametrize("seed", FOUR)
def test_wide_survival_rows_read_out(sia, oracle, seed):
    """Reachable set and rollout flags against the oracle's literal loops (as test_random_instances_read_out_bit_exact), and no
    bankrupt state is ever visited -- also on the long-division quantisers, where a balance of -0.3 rounds to key 0 and is alive."""
    w, ref = _reference(oracle, seed)
    P, f = ref["P"], w.functor
    rng = np.random.default_rng(zlib.crc32(w.name.encode()))
    with sia.SdpEngine(w.desc(), w.pmf, w.overhead()) as eng:
        eng.solve()
        assert eng.stats().kernel_used == 2
        reach = P.reachable()
        for period in range(1, w.T + 1):
            assert np.array_equal(eng.reachable(period), reach[period - 1]), f"{w.name} t={period}: reachable"
            assert not reach[period - 1][P.state_arrays(period)[1] < 0].any(), f"{w.name} t={period}: a bankrupt state is visited"
        assert sum(int(r.sum()) for r in reach) > w.T
        dem = np.stack([rng.choice(np.asarray(w.pmf[t])[:, 0], size=64) for t in range(w.T)], axis=1)
        disc = np.ones(w.T)
        gs, gv = eng.simulate(dem, disc, f.iniInventory, f.iniCash, 0.0)
        os_, ov = P.simulate(ref["V"], ref["pol"], dem, disc, f.iniInventory, f.iniCash, 0.0)
        assert np.array_equal(eng.last_sim_flags, P.last_sim_flags), f"{w.name}: rollout flags"
        assert np.array_equal(gv, ov) and np.array_equal(gs[gv], os_[ov]), f"{w.name}: rollout sums"
