"""Sampled simulation on a handle (sdpgpu_set_sampler, sdpgpu_simulate_sampled, sdpgpu_sample_demands; DESIGN 4 "Sampled
simulation on a handle") as far as it goes without a GPU: the new symbols, every argument error and refusal with a text naming
the argument BEFORE any device call, and the host twin of RANDOM mode, written from its definition over
tests/sampler_twin.py's Philox (the LHS twin is sampler_twin itself at inst = 0)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
import sampler_twin as tw  # noqa: E402

NEW_SYMBOLS = ("sdpgpu_set_sampler", "sdpgpu_simulate_sampled", "sdpgpu_sample_demands")
OK, ERR_ARG, ERR_STATE, ERR_DEVICE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4
LHS, RANDOM = 0, 1


# ---- the twin of RANDOM mode ------------------------------------------------------------------------------------------------
def random_uniforms(n, seed, t, first_path=0):
    """u[p] of path P = first_path + p in period index t: (w0, w1, ., .) = Philox4x32-10 at counter (P mod 2^32, t, P div 2^32, 2)
    under the seed, u = ((w0 * 2^32 + w1) >> 11) * 2^-53."""
    P = np.array([first_path + p for p in range(n)], dtype=np.uint64)
    lo, hi = P & np.uint64(tw.M32), P >> np.uint64(32)
    u = np.empty(n)
    for h in np.unique(hi):  # (_philox_vec takes one value of word 2 at a time)
        at = hi == h
        w0, w1, _, _ = tw._philox_vec(lo[at], t, int(h), 2, tw._key(seed))
        u[at] = (((w0 << np.uint64(32)) | w1) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return u


def tile_demands(tile, u):
    """Demand of u from a pmf tile [[demand, prob], ...]: thresholds = the running fp64 sum, the last one +infinity; the demand
    is the tile's q-th VALUE, q = #{c <= u} (a tile may have gaps)."""
    tile = np.asarray(tile, dtype=np.float64)
    thr = np.cumsum(tile[:, 1], dtype=np.float64)
    thr[-1] = np.inf
    return tile[:, 0][np.searchsorted(thr, u, side="right")]


def spec_demands(table, u):
    k_lo, thr, strict = table
    return tw.demand_of(u, k_lo, thr, strict)


def twin_sample(n, seed, mode, first_path, draw):
    """(demand[n, T], u[n, T]); draw[t] maps the uniforms of period index t to demands."""
    T = len(draw)
    dem, uu = np.empty((n, T)), np.empty((n, T))
    for t in range(T):
        u = random_uniforms(n, seed, t, first_path) if mode == RANDOM else tw.strata_and_uniforms(n, seed, 0, t)[1]
        uu[:, t] = u
        dem[:, t] = draw[t](u)
    return dem, uu


def reduction_chain(n):
    """L(n) of DESIGN 4: 6 butterfly levels in a wave, C = ceil(W / 1024) partials per thread, 10 tree levels."""
    W = (n + 63) // 64
    return 6 + (W + 1023) // 1024 + 10


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _spec(sia, kind, a, b):
    s = sia._abi.SdpgpuDistSpec()
    s.kind, s.a, s.b = kind, a, b
    return s


def _engine(sia, make=cases.f1_small, **changes):
    w = make()
    d = w.desc()
    for k, v in changes.items():
        setattr(d, k, v)
    return sia.SdpEngine(d, w.pmf, w.overhead()), w


def _sim(lib, eng, n=5, seed=1, mode=LHS, first_path=0, result=True, disc=None):
    from stochastic_inventory_amd._abi import SdpgpuSimResult
    res = SdpgpuSimResult()
    rc = lib.sdpgpu_simulate_sampled(eng._h, n, seed, mode, first_path, None if disc is None else _dp(disc), 0.0, 0.0, 0.0,
                                     C.byref(res) if result else None, None, None)
    return rc, lib.sdpgpu_last_error(eng._h).decode()


def _draw(lib, eng, n=5, seed=1, mode=LHS, first_path=0, out=True):
    dem = np.zeros((max(n, 1), eng.T))
    rc = lib.sdpgpu_sample_demands(eng._h, n, seed, mode, first_path, _dp(dem) if out else None, None)
    return rc, lib.sdpgpu_last_error(eng._h).decode()


def test_the_new_symbols_are_declared_exported_and_listed(sia, lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdpgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in sia._abi.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert "sdpgpu_sim_result" in header and "SDPGPU_SAMPLE_RANDOM" in header
    assert lib.sdpgpu_abi_version() == 6  # additive
    for m in ("set_sampler", "simulate_sampled", "sample_demands"):
        assert hasattr(sia.SdpEngine, m)
    r = sia._abi.SdpgpuSimResult
    assert [f[0] for f in r._fields_] == ["n_paths", "n_valid", "n_lost", "reserved", "mean", "m2", "kernel_ms"] and C.sizeof(r) == 40
    import inspect
    from stochastic_inventory_amd import simulation
    for cls in (simulation.Simulation, simulation.RiskSimulation):
        assert inspect.signature(cls.__init__).parameters["sampler"].default == "host"


def test_argument_errors_name_the_argument_before_any_device_call(sia, lib):
    eng, _ = _engine(sia)
    with eng:
        assert lib.sdpgpu_simulate_sampled(None, 5, 1, LHS, 0, None, 0.0, 0.0, 0.0, None, None, None) == ERR_ARG
        assert lib.sdpgpu_sample_demands(None, 5, 1, LHS, 0, None, None) == ERR_ARG
        assert lib.sdpgpu_set_sampler(None, 0, None) == ERR_ARG
        for call in (_sim, _draw):
            rc, err = call(lib, eng, n=0)
            assert rc == ERR_ARG and "n_paths = 0" in err
            rc, err = call(lib, eng, n=-4)
            assert rc == ERR_ARG and "n_paths" in err
            rc, err = call(lib, eng, n=(1 << 24) + 1)
            assert rc == ERR_UNSUPPORTED and "n_paths" in err and str(1 << 24) in err
            rc, err = call(lib, eng, mode=2)
            assert rc == ERR_ARG and "mode = 2" in err
            rc, err = call(lib, eng, mode=LHS, first_path=7)
            assert rc == ERR_ARG and "first_path" in err
        rc, err = _sim(lib, eng, result=False)
        assert rc == ERR_ARG and "result" in err
        rc, err = _draw(lib, eng, out=False)
        assert rc == ERR_ARG and "out_demand" in err
        # valid arguments (both modes, a first_path above 2^32), nothing solved
        for mode, fp in ((LHS, 0), (RANDOM, 0), (RANDOM, (1 << 40) + 3)):
            rc, err = _sim(lib, eng, mode=mode, first_path=fp, disc=np.ones(eng.T))
            assert rc == ERR_STATE and "nothing has been solved" in err
        assert _sim(lib, eng, n=1 << 24)[0] == ERR_STATE


def test_set_sampler_validation(sia, lib):
    eng, _ = _engine(sia)
    err = lambda: lib.sdpgpu_last_error(eng._h).decode()
    with eng:
        ok = _spec(sia, sia._abi.DIST_NORMAL, 3.0, 0.9)
        assert lib.sdpgpu_set_sampler(eng._h, eng.T, C.byref(ok)) == ERR_ARG and f"period index {eng.T}" in err()
        assert lib.sdpgpu_set_sampler(eng._h, -1, None) == ERR_ARG and "period index -1" in err()
        assert lib.sdpgpu_set_sampler(eng._h, 2, C.byref(_spec(sia, sia._abi.DIST_NORMAL, 3.0, -1.0))) == ERR_ARG
        assert "period 3" in err() and "spec" in err()
        assert lib.sdpgpu_set_sampler(eng._h, 2, C.byref(_spec(sia, 9, 1.0, 1.0))) == ERR_ARG and "kind 9" in err()
        wide = _spec(sia, sia._abi.DIST_UNIFORM_INT, 0.0, 1.0e6)
        assert lib.sdpgpu_set_sampler(eng._h, 0, C.byref(wide)) == ERR_UNSUPPORTED and "SDPGPU_SAMPLE_TABLE_CAP" in err()
        for kind, a, b in ((sia._abi.DIST_NORMAL, 3.0, 0.9), (sia._abi.DIST_POISSON, 20.0, 0.0), (sia._abi.DIST_GAMMA, 25.0, 0.5),
                           (sia._abi.DIST_UNIFORM_INT, 0.0, 10.0)):
            assert lib.sdpgpu_set_sampler(eng._h, 1, C.byref(_spec(sia, kind, a, b))) == OK and err() == ""
        assert lib.sdpgpu_set_sampler(eng._h, 1, None) == OK  # back to the pmf tile
        eng.set_sampler(0, sia.PoissonDist(4.0))  # the Python face of the same call
        eng.set_sampler(0, None)
        with pytest.raises(sia.SdpgpuError):
            eng.set_sampler(eng.T, None)


def test_a_spec_needs_a_unit_step_and_a_tile_does_not(sia, lib):
    w = cases.f1_small()  # (its tiles 0 .. 7 hold odd demands: doubled for the handle of step 2)
    d = w.desc()
    d.step, d.min_inventory, d.max_inventory, d.max_order_quantity, d.ini_inventory = 2.0, -12.0, 16.0, 8.0, 2.0
    tiles = [np.stack([t[:, 0] * 2.0, t[:, 1]], axis=1) for t in w.pmf]
    with sia.SdpEngine(d, tiles) as eng:
        ok = _spec(sia, sia._abi.DIST_NORMAL, 3.0, 0.9)
        assert lib.sdpgpu_set_sampler(eng._h, 0, C.byref(ok)) == ERR_UNSUPPORTED
        assert "step == 1" in lib.sdpgpu_last_error(eng._h).decode()
        assert lib.sdpgpu_set_sampler(eng._h, 0, None) == OK
        # the tile sampler passes validation at step 2: what is missing is the solve, resp. (below) only the device
        rc, err = _sim(lib, eng)
        assert rc == ERR_STATE and "nothing has been solved" in err
        rc, err = _draw(lib, eng)
        assert rc in (OK, ERR_DEVICE) and "step" not in err


def test_refusals_are_those_of_sdpgpu_simulate(sia, lib):
    from stochastic_inventory_amd.pmf import staff_level_pmf
    # the (x, R) state of cash_formula 2
    eng, _ = _engine(sia, cases.f3_xr)
    with eng:
        for call in (_sim, _draw):
            rc, err = call(lib, eng)
            assert rc == ERR_UNSUPPORTED and "CashConstraintXR" in err
    # a rank of several
    eng, _ = _engine(sia, world_size=2, rank=0)
    with eng:
        for call in (_sim, _draw):
            rc, err = call(lib, eng)
            assert rc == ERR_STATE and "world_size 1" in err
    # STAFF
    f = sia.StaffFunctor(fixCost=100, unitVariCost=10, salary=20, unitPenalty=80, minStaffNum=[8, 8, 8], maxHireNum=20,
                         minX=0, maxX=30, clampStaff=True, iniStaffNum=0)
    with sia.SdpEngine(f.to_desc(3), None, [8.0] * 3, level_pmf=staff_level_pmf([0.5] * 3, 31)) as eng:
        for call in (_sim, _draw):
            rc, err = call(lib, eng)
            assert rc == ERR_UNSUPPORTED and "SimulatesS" in err
    # user functors
    from stochastic_inventory_amd import workloads
    w = cases.f1_small()
    with sia.SdpEngine(w.desc(), w.pmf, custom_source=workloads.CLSP_LAMBDAS_HIP, custom_params=workloads.clsp_lambda_params(w)) as eng:
        for call in (_sim, _draw):
            rc, err = call(lib, eng)
            assert rc == ERR_UNSUPPORTED and "user functor" in err


def test_tile_samplers_need_the_tiles(sia, lib):
    d = cases.f1_small().desc()
    h = C.c_void_p()
    assert lib.sdpgpu_create(C.byref(d), C.byref(h)) == OK
    try:
        out = np.zeros((5, d.periods))
        assert lib.sdpgpu_sample_demands(h, 5, 1, LHS, 0, _dp(out), None) == ERR_STATE
        assert b"pmf of period 1" in lib.sdpgpu_last_error(h)
        # with a spec on every period the tiles are not needed: only the device can be missing
        for t in range(d.periods):
            assert lib.sdpgpu_set_sampler(h, t, C.byref(_spec(sia, sia._abi.DIST_POISSON, 4.0, 0.0))) == OK
        assert lib.sdpgpu_sample_demands(h, 5, 1, LHS, 0, _dp(out), None) in (OK, ERR_DEVICE)
    finally:
        lib.sdpgpu_destroy(h)


def test_valid_arguments_without_a_device_are_a_device_error(sia, lib):
    """sample_demands needs the tiles and a device, not a solve: with valid arguments the only thing that can be missing here is
    the device (SDPGPU_ERR_DEVICE with the runtime's text); where there is one, the call succeeds."""
    has_gpu = False
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        pass
    eng, w = _engine(sia)
    with eng:
        for mode, fp in ((LHS, 0), (RANDOM, 0), (RANDOM, (1 << 33) + 5)):
            out = np.full((5, eng.T), -1.0)
            rc = lib.sdpgpu_sample_demands(eng._h, 5, 1, mode, fp, _dp(out), _dp(out.copy()))
            if has_gpu:
                assert rc == OK and set(np.unique(out)) <= set(np.asarray(w.pmf[0])[:, 0])
            else:
                assert rc == ERR_DEVICE and lib.sdpgpu_last_error(eng._h) != b""
        if not has_gpu:
            with pytest.raises(sia.SdpgpuError) as e:
                eng.sample_demands(5, 1, mode="random", first_path=9)
            assert e.value.code == ERR_DEVICE
        with pytest.raises(ValueError):
            eng.sample_demands(5, 1, mode="sobol")


def test_random_twin_known_answers():
    """The words behind u: Philox4x32-10 (its published vectors are held in tests/test_batch_simulate_host.py) at the counter
    (P mod 2^32, t, P div 2^32, 2); the vectorised twin against the scalar one, and two values worked out by hand from it."""
    seed = 20240607
    key = tw._key(seed)
    for P, t in ((0, 0), (1, 0), (5, 3), ((1 << 32) - 1, 2), (1 << 32, 2), ((1 << 40) + 12345, 7)):
        w = tw.philox4x32_10((P & tw.M32, t, P >> 32, 2), key)
        want = float(((w[0] << 32) | w[1]) >> 11) * 2.0 ** -53
        assert random_uniforms(1, seed, t, first_path=P)[0] == want
        assert 0.0 <= want < 1.0
    # word 3 keeps the stream apart from the latin hypercube's uniforms (0) and shuffle keys (1)
    assert tw.philox4x32_10((0, 0, 0, 2), key) != tw.philox4x32_10((0, 0, 0, 0), key) != tw.philox4x32_10((0, 0, 0, 1), key)
    assert tw.philox4x32_10((0, 0, 0, 2), (0, 0)) == KAT_ZERO_KEY
    assert random_uniforms(1, 0, 0)[0] == float(((KAT_ZERO_KEY[0] << 32) | KAT_ZERO_KEY[1]) >> 11) * 2.0 ** -53


KAT_ZERO_KEY = (0xDD2FC514, 0xADF5A0DB, 0xE6F70B22, 0xD3B4CA74)


def test_random_stream_continues_across_calls():
    """(first_path, n) = (0, a) then (a, b) draw what (0, a + b) draws -- also across a multiple of 2^32."""
    seed = 7
    for base in (0, (1 << 32) - 700, (1 << 45) + 1):
        for a, b in ((1, 1), (1000, 537), (64, 1000)):
            for t in (0, 3):
                whole = random_uniforms(a + b, seed, t, base)
                assert np.array_equal(whole[:a], random_uniforms(a, seed, t, base))
                assert np.array_equal(whole[a:], random_uniforms(b, seed, t, base + a))
    u = random_uniforms(20000, seed, 0)
    assert abs(u.mean() - 0.5) < 4 / np.sqrt(12 * 20000) and len(np.unique(u)) == 20000
    assert not np.array_equal(u, random_uniforms(20000, seed, 1)) and not np.array_equal(u, random_uniforms(20000, seed + 1, 0))


def test_tile_lookup_returns_the_tiles_values():
    tile = cases.f1_gapped().pmf[0]  # {2, 5, 9} with probabilities 1/4, 1/2, 1/4
    u = np.array([0.0, 0.2499, 0.25, 0.5, 0.7499999, 0.75, 0.999999, 1.0 - 2.0 ** -53])
    assert tile_demands(tile, u).tolist() == [2.0, 2.0, 5.0, 5.0, 5.0, 9.0, 9.0, 9.0]
    assert reduction_chain(10000) == 17 and reduction_chain(1 << 24) == 6 + 256 + 10 and reduction_chain(1) == 17


def test_merge_moments_is_the_pairwise_update():
    from stochastic_inventory_amd.simulation import merge_moments
    rng = np.random.default_rng(3)
    x = rng.normal(100.0, 7.0, size=5000)
    n, mean, m2 = 0, 0.0, 0.0
    for part in np.split(x, [1, 64, 1000, 3000]):
        n, mean, m2 = merge_moments(n, mean, m2, len(part), float(part.mean()), float(((part - part.mean()) ** 2).sum()))
    assert n == 5000 and abs(mean - x.mean()) < 1e-12 * abs(x.mean())
    assert abs(m2 - ((x - x.mean()) ** 2).sum()) < 1e-11 * m2
