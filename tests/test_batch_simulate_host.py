"""The batched simulation (sdpgpu_batch_simulate*, sdpgpu_sample_table; DESIGN 4 "Batched simulation") as far as it goes
without a GPU: the new symbols, validation (every bad argument its code and a text naming instance / field, before any
device call), the threshold tables against 50-digit cdfs, and the sampler's CONSTRUCTION checked on the independent host
twin (tests/sampler_twin.py): sigma a bijection, one u per stratum, uncorrelated columns, table search = rounded quantile."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_twin as tw  # noqa: E402

SEED = 20240607
NS = (1, 2, 63, 64, 65, 1537, 10000)
RTOL, ATOL_CDF_DIFFERENCE = 1e-13, 4e-16  # tests/test_pmf_reference.py holds the same cdf code to these
NEW_SYMBOLS = ("sdpgpu_batch_simulate", "sdpgpu_batch_set_sampler", "sdpgpu_batch_simulate_sampled",
               "sdpgpu_batch_sample_demands", "sdpgpu_batch_simulate_ms", "sdpgpu_sample_table")


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _batch(sia, lib, n=3, T=3, step=1.0, with_pmf=True):
    arr = (sia.SdpgpuDesc * n)()
    for i in range(n):
        d = sia.desc_defaults()
        d.periods, d.step = T, step
        d.min_inventory, d.max_inventory, d.max_order_quantity = -20.0, 30.0, 12.0
        d.fixed_order_cost, d.unit_order_cost, d.holding_cost, d.penalty_cost = 10.0 + i, float(i % 2), 1.0, 5.0 + i
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(sia.SdpgpuDesc))
    b = C.c_void_p()
    assert lib.sdpgpu_batch_create(arr, n, C.byref(b)) == 0, lib.sdpgpu_batch_last_error(None)
    if with_pmf:
        dem = np.arange(4, dtype=np.float64) * step
        p = np.full(4, 0.25)
        for i in range(n):
            for t in range(T):
                assert lib.sdpgpu_batch_set_pmf(b, i, t, _dp(dem), _dp(p), 4) == 0
    return b


def _spec(sia, kind, a, b):
    s = sia._abi.SdpgpuDistSpec()
    s.kind, s.a, s.b = kind, a, b
    return s


def test_the_new_symbols_are_declared_and_exported(sia, lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdpgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in sia._abi.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert lib.sdpgpu_abi_version() == 6  # additive
    assert "SimulationBatch" in sia.__all__ and hasattr(sia.SdpBatch, "simulate_sampled")


def test_simulate_validates_before_any_device_call(sia, lib):
    b = _batch(sia, lib)
    err = lambda: lib.sdpgpu_batch_last_error(b).decode()
    try:
        dem = np.zeros((5, 3))
        mean = np.zeros(3)
        sums = np.zeros((3, 5))
        assert lib.sdpgpu_batch_simulate(None, 5, _dp(dem), 0, None, _dp(mean), None) == 1
        assert lib.sdpgpu_batch_simulate(b, 5, _dp(dem), 0, None, None, None) == 1 and "out_mean" in err()
        assert lib.sdpgpu_batch_simulate(b, 5, None, 0, None, _dp(mean), None) == 1 and "demand" in err()
        assert lib.sdpgpu_batch_simulate(b, 0, _dp(dem), 0, None, _dp(mean), None) == 1 and "n_paths = 0" in err()
        assert lib.sdpgpu_batch_simulate(b, -3, _dp(dem), 0, None, _dp(mean), None) == 1 and "n_paths" in err()
        assert lib.sdpgpu_batch_simulate(b, 5, _dp(dem), 7, None, _dp(mean), None) == 1 and "instance_stride" in err()
        for bad in (31.0, -21.0, 0.5, float("nan")):
            ini = np.array([0.0, 3.0, bad])
            assert lib.sdpgpu_batch_simulate(b, 5, _dp(dem), 0, _dp(ini), _dp(mean), None) == 1
            assert "instance 2" in err() and "ini_x" in err(), err()
            assert lib.sdpgpu_batch_simulate_sampled(b, 5, 1, _dp(ini), _dp(mean), None) == 1 and "instance 2" in err()
        assert lib.sdpgpu_batch_simulate_sampled(b, 0, 1, None, _dp(mean), None) == 1 and "n_paths = 0" in err()
        assert lib.sdpgpu_batch_simulate_sampled(b, 5, 1, None, None, None) == 1 and "out_mean" in err()
        # valid arguments, nothing solved
        assert lib.sdpgpu_batch_simulate(b, 5, _dp(dem), 0, None, _dp(mean), _dp(sums)) == 2 and "before sdpgpu_batch_solve" in err()
        assert lib.sdpgpu_batch_simulate_sampled(b, 5, 1, None, _dp(mean), _dp(sums)) == 2 and "before sdpgpu_batch_solve" in err()
        assert lib.sdpgpu_batch_simulate_ms(b) == -1.0
    finally:
        lib.sdpgpu_batch_destroy(b)


def test_sampler_and_sample_demands_validation(sia, lib):
    b = _batch(sia, lib)
    err = lambda: lib.sdpgpu_batch_last_error(b).decode()
    try:
        ok = _spec(sia, sia._abi.DIST_NORMAL, 3.0, 0.9)
        assert lib.sdpgpu_batch_set_sampler(b, 3, 0, C.byref(ok)) == 1 and "instance 3" in err()
        assert lib.sdpgpu_batch_set_sampler(b, 0, 3, C.byref(ok)) == 1 and "period index 3" in err()
        bad = _spec(sia, sia._abi.DIST_NORMAL, 3.0, -1.0)
        assert lib.sdpgpu_batch_set_sampler(b, 1, 2, C.byref(bad)) == 1
        assert "instance 1" in err() and "period 3" in err() and "spec" in err()
        assert lib.sdpgpu_batch_set_sampler(b, 1, 2, C.byref(_spec(sia, 9, 1.0, 1.0))) == 1 and "kind 9" in err()
        wide = _spec(sia, sia._abi.DIST_UNIFORM_INT, 0.0, 1.0e6)  # over the documented cap on the table length
        assert lib.sdpgpu_batch_set_sampler(b, 0, 0, C.byref(wide)) == 4 and "SDPGPU_SAMPLE_TABLE_CAP" in err()
        assert lib.sdpgpu_batch_set_sampler(b, 0, 0, C.byref(ok)) == 0 and err() == ""
        assert lib.sdpgpu_batch_set_sampler(b, 0, 0, None) == 0  # back to the pmf tile
        out = np.zeros((5, 3))
        assert lib.sdpgpu_batch_sample_demands(b, 3, 5, 1, _dp(out), None) == 1 and "instance 3" in err()
        assert lib.sdpgpu_batch_sample_demands(b, 0, 0, 1, _dp(out), None) == 1 and "n_paths = 0" in err()
        assert lib.sdpgpu_batch_sample_demands(b, 0, 5, 1, None, None) == 1 and "out_demand" in err()
    finally:
        lib.sdpgpu_batch_destroy(b)
    b = _batch(sia, lib, with_pmf=False)
    try:  # the tile samplers need the tiles
        out = np.zeros((5, 3))
        assert lib.sdpgpu_batch_sample_demands(b, 0, 5, 1, _dp(out), None) == 2
        assert b"instance 0, period 1" in lib.sdpgpu_batch_last_error(b)
    finally:
        lib.sdpgpu_batch_destroy(b)


def test_sampled_mode_needs_a_unit_step(sia, lib):
    b = _batch(sia, lib, step=2.0)
    try:
        mean, out = np.zeros(3), np.zeros((5, 3))
        ok = _spec(sia, sia._abi.DIST_NORMAL, 3.0, 0.9)
        for rc in (lib.sdpgpu_batch_simulate_sampled(b, 5, 1, None, _dp(mean), None), lib.sdpgpu_batch_set_sampler(b, 0, 0, C.byref(ok)),
                   lib.sdpgpu_batch_sample_demands(b, 0, 5, 1, _dp(out), None)):
            assert rc == 4 and b"step == 1" in lib.sdpgpu_batch_last_error(b)
        assert lib.sdpgpu_batch_simulate(b, 5, _dp(np.zeros((5, 3))), 0, None, _dp(mean), None) == 2  # explicit demands: any step
    finally:
        lib.sdpgpu_batch_destroy(b)


def test_valid_arguments_without_a_device_are_a_device_error(sia, lib):
    """sample_demands needs the tiles and a device, not a solve: with valid arguments the only thing that can be missing here
    is the device (SDPGPU_ERR_DEVICE with the runtime's text); where there is one, the call succeeds."""
    has_gpu = False
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        pass
    b = _batch(sia, lib)
    try:
        out = np.zeros((5, 3))
        rc = lib.sdpgpu_batch_sample_demands(b, 0, 5, 1, _dp(out), _dp(out.copy()))
        if has_gpu:
            assert rc == 0 and set(np.unique(out)) <= {0.0, 1.0, 2.0, 3.0}
        else:
            assert rc == 3 and lib.sdpgpu_batch_last_error(b) != b""
    finally:
        lib.sdpgpu_batch_destroy(b)


def test_sample_table_argument_errors(sia, lib):
    k, n = C.c_int32(), C.c_int32()
    ok = _spec(sia, sia._abi.DIST_NORMAL, 10.0, 3.0)
    assert lib.sdpgpu_sample_table(None, C.byref(k), None, 0, C.byref(n)) == 1
    assert lib.sdpgpu_sample_table(C.byref(ok), None, None, 0, C.byref(n)) == 1
    assert lib.sdpgpu_sample_table(C.byref(ok), C.byref(k), None, 4, C.byref(n)) == 1
    assert lib.sdpgpu_sample_table(C.byref(ok), C.byref(k), None, 0, C.byref(n)) == 0 and n.value > 0
    small = np.zeros(2)
    assert lib.sdpgpu_sample_table(C.byref(ok), C.byref(k), _dp(small), 2, C.byref(n)) == 1
    assert b"capacity" in lib.sdpgpu_last_error(None)
    assert lib.sdpgpu_sample_table(C.byref(_spec(sia, sia._abi.DIST_GAMMA, -1.0, 1.0)), C.byref(k), None, 0, C.byref(n)) == 1
    assert lib.sdpgpu_sample_table(C.byref(_spec(sia, sia._abi.DIST_NORMAL, 0.0, 1.0e7)), C.byref(k), None, 0, C.byref(n)) == 4
    # a distribution narrower than one integer: no threshold inside (2^-64, 1), every u gives round(mean)
    assert lib.sdpgpu_sample_table(C.byref(_spec(sia, sia._abi.DIST_NORMAL, 3.0, 1e-9)), C.byref(k), None, 0, C.byref(n)) == 0
    assert (k.value, n.value) == (3, 0)


def _mp_cdf(kind, a, b, x):
    import mpmath as mp
    mp.mp.dps = 50
    x = mp.mpf(x)
    if kind == "normal":
        return mp.erfc(-(x - mp.mpf(a)) / (mp.mpf(b) * mp.sqrt(2))) / 2
    if kind == "gamma":
        return mp.gammainc(mp.mpf(a), 0, mp.mpf(b) * x, regularized=True) if x > 0 else mp.mpf(0)
    if kind == "poisson":
        return mp.gammainc(mp.floor(x) + 1, mp.mpf(a), mp.inf, regularized=True) if x >= 0 else mp.mpf(0)
    n = mp.mpf(b) - mp.mpf(a) + 1
    return (mp.floor(x) - mp.mpf(a) + 1) / n


TABLE_CASES = [("normal", 54.0, 54 * 0.3), ("normal", 3.0, 3 * 0.3), ("normal", 10.0, 10 * 0.1), ("normal", 51.0, 51 * 0.2),
               ("normal", 2.0, 2 * 0.1), ("poisson", 20.0, 0.0), ("poisson", 3.5, 0.0), ("poisson", 180.0, 0.0),
               ("gamma", 25.0, 0.5), ("gamma", 2.0, 0.1), ("uniform_int", 0.0, 10.0), ("uniform_int", -3.0, 40.0)]


@pytest.mark.parametrize("kind,a,b", TABLE_CASES)
def test_sample_table_against_fifty_digit_cdfs(sia, kind, a, b):
    from stochastic_inventory_amd import pmf
    make = {"normal": pmf.NormalDist, "gamma": pmf.GammaDist, "poisson": lambda a, b: pmf.PoissonDist(a),
            "uniform_int": lambda a, b: pmf.UniformIntDist(int(a), int(b))}
    k_lo, thr, strict = pmf.sample_table(make[kind](a, b))
    assert strict == (kind in ("poisson", "uniform_int"))
    assert len(thr) > 0 and np.all(np.diff(thr) >= 0), "ascending"
    assert thr[0] > 2.0 ** -64 and thr[-1] < 1.0, "inside (2^-64, 1)"
    half = 0.0 if strict else 0.5
    want = np.array([float(_mp_cdf(kind, a, b, k_lo + q + half)) for q in range(len(thr))])
    err = np.abs(thr - want)
    assert np.all(err <= RTOL * want + ATOL_CDF_DIFFERENCE), (float(np.max(err / want)), int(np.argmax(err / want)))
    # the table is complete: the k below k_lo has a threshold <= 2^-64 (or none), the k after the last one a threshold of 1 in fp64
    if kind != "uniform_int":
        assert float(_mp_cdf(kind, a, b, k_lo - 1 + half)) <= 2.0 ** -64 * (1 + 1e-9)
        assert float(_mp_cdf(kind, a, b, k_lo + len(thr) + half)) >= 1.0 - 2.3e-16
    else:
        assert k_lo == int(a) and len(thr) == int(b - a)
    if kind == "normal" and (a, b) == (54.0, 54 * 0.3):
        assert 270 <= len(thr) <= 290  # about 17 standard deviations: CLSPTesting's widest period


@pytest.mark.parametrize("n", NS)
def test_sigma_is_a_bijection_and_every_stratum_holds_one_u(n):
    for inst, t in ((0, 0), (5, 3), (539, 7)):
        j, u = tw.strata_and_uniforms(n, SEED, inst, t)
        assert np.array_equal(np.sort(j), np.arange(n)), (n, inst, t)
        assert np.all((u >= j / n) & (u <= (j + 1) / n))
        assert np.array_equal(np.minimum(np.floor(np.sort(u) * n), n - 1), np.arange(n)) or n == 1
        if n >= 63:
            assert not np.array_equal(j, np.arange(n)), "sigma must not be the identity"
    if n >= 63:
        assert not np.array_equal(tw.sigma(n, SEED, 0, 0), tw.sigma(n, SEED, 0, 1))
        assert not np.array_equal(tw.sigma(n, SEED, 0, 0), tw.sigma(n, SEED + 1, 0, 0))


def test_philox_known_answers():
    """Random123's published vectors for Philox4x32-10."""
    assert tw.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    m = 0xFFFFFFFF
    assert tw.philox4x32_10((m, m, m, m), (m, m)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert tw.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_the_stratum_columns_of_two_periods_are_uncorrelated():
    """|Spearman rho| < 4 / sqrt(n - 1) (four standard deviations under independence), n = 10000, the seeds the tests use."""
    from scipy.stats import spearmanr
    n = 10000
    bound = 4.0 / np.sqrt(n - 1)
    for seed in (SEED, 12345):
        for inst, ta, tb in ((0, 0, 1), (0, 1, 2), (17, 0, 7), (539, 3, 4)):
            rho = spearmanr(tw.sigma(n, seed, inst, ta), tw.sigma(n, seed, inst, tb))[0]
            assert abs(rho) < bound, (seed, inst, ta, tb, rho)
        rho = spearmanr(tw.sigma(n, seed, 0, 0), tw.sigma(n, seed, 1, 0))[0]  # and of two instances
        assert abs(rho) < bound
        rho = spearmanr(np.arange(n), tw.sigma(n, seed, 0, 0))[0]  # and against the path index itself
        assert abs(rho) < bound


def test_table_search_equals_the_rounded_quantile():
    """Twin demands of a CLSPTesting instance (pattern 10, coeVar 0.3) against Math.round(norm.ppf(u)): 10000 x 8 samples; the
    two may differ only where the ppf sample lies within 1e-9 of a half-integer (expected number of such samples: none)."""
    from scipy.stats import norm
    from stochastic_inventory_amd import pmf, workloads
    means = workloads.CLSP_TESTING_DEMANDS[9]
    tables = [pmf.sample_table(pmf.NormalDist(float(m), 0.3 * m)) for m in means]
    dem, u = tw.sample(10000, SEED, 537, tables)
    differ = 0
    for t, m in enumerate(means):
        x = norm.ppf(u[:, t], loc=float(m), scale=0.3 * m)
        want = np.floor(x + 0.5)  # Math.round
        off = dem[:, t] != want
        near = np.abs((x - 0.5) - np.round(x - 0.5)) < 1e-9
        assert not np.any(off & ~near), (t, dem[off & ~near, t][:5], x[off & ~near][:5])
        differ += int(off.sum())
    assert differ <= 2
