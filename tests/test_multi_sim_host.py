"""Two-product rollout (sdpgpu_multi_policy_*, multiitem.MultiPolicy, CashSimulationMulti, CashSimulationMultiXR; DESIGN 4
"Two-product rollout") as far as it goes without a GPU: the eight symbols in the header, in _abi.EXPORTS and in the library,
ABI 6, every refusal of `create` with its code and a text naming the argument BEFORE any device call, the exception barrier,
and what a valid call answers without a device (SDPGPU_ERR_DEVICE, as the other rollouts).  The refusals of simulate* need a
policy object, which needs a device: tests/test_gpu_multi_sim.py has them."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_sim_cases as cases  # noqa: E402

OK, ERR_ARG, ERR_STATE, ERR_DEVICE, ERR_UNSUPPORTED, ERR_ALLOC, ERR_INTERNAL = 0, 1, 2, 3, 4, 5, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdpgpu_multilead_policy_create": 4, "sdpgpu_multicash_policy_create": 6, "sdpgpu_multi_policy_destroy": 1,
           "sdpgpu_multi_policy_lookup": 11, "sdpgpu_multi_policy_simulate": 8, "sdpgpu_multi_policy_simulate_sampled": 9,
           "sdpgpu_multi_policy_sample": 8}
NAN = float("nan")


@pytest.fixture(scope="module")
def lib(sia):
    return sia._abi.load()


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _create(sia, lib, cid, rows, capacity_log2=0, table_edit=None, kw_edit=None, xr=None, dep=None, null_memo=False):
    """-> (rc, error text); a policy that was created is destroyed again."""
    from stochastic_inventory_amd import multiitem
    kind, kw, dep0 = cases.case(cid)
    kw = dict(kw, **(kw_edit or {}))
    t, arrs = multiitem.table_from_rows(rows)
    if table_edit:
        table_edit(t, arrs)
    h = C.c_void_p()
    memo = None if null_memo else C.byref(t)
    if kind == "multilead":
        k = multiitem.fill_multilead(sia._abi.SdpgpuMultilead(), **kw)
        rc = lib.sdpgpu_multilead_policy_create(C.byref(k), memo, capacity_log2, C.byref(h))
    else:
        k = multiitem.fill_multicash(sia._abi.SdpgpuMulticash(), **kw)
        rc = lib.sdpgpu_multicash_policy_create(C.byref(k), (1 if kind == "multixr" else 0) if xr is None else xr,
                                                dep0 if dep is None else dep, memo, capacity_log2, C.byref(h))
    err = lib.sdpgpu_multilead_last_error().decode()
    if h:
        assert rc == OK
        lib.sdpgpu_multi_policy_destroy(h)
    else:
        assert rc != OK
    return rc, err


def test_the_symbols_and_classes_exist(sia, lib):
    header = open(os.path.join(ROOT, "include", "sdpgpu.h")).read()
    assert "typedef struct sdpgpu_multi_policy sdpgpu_multi_policy;" in header  # (the eighth name: the handle's type)
    for name, nargs in SYMBOLS.items():
        assert name in sia._abi.EXPORTS and hasattr(lib, name) and name + "(" in header, name
        assert len(sia._abi.EXPORTS[name][1]) == nargs, name
    assert lib.sdpgpu_abi_version() == 6  # additive
    assert "CashSimulationMulti.java" in header and "CashSimulationMultiXR.java" in header and '"Two-product rollout"' in header
    from stochastic_inventory_amd import multiitem
    for name in ("MultiPolicy", "CashSimulationMulti", "CashSimulationMultiXR"):
        assert getattr(sia, name) is getattr(multiitem, name) and name in sia.__all__
    for m in ("lookup", "simulate", "simulate_sampled", "sample", "close"):
        assert callable(getattr(multiitem.MultiPolicy, m))
    assert inspect.signature(multiitem._MultiRecursionBase.policy).parameters["capacity_log2"].default == 0
    # the reference's constructor shape (CashSimulationMulti.java:37-44, CashSimulationMultiXR.java:38-46)
    for cls in (multiitem.CashSimulationMulti, multiitem.CashSimulationMultiXR):
        assert list(inspect.signature(cls.__init__).parameters)[1:7] == ["sampleNum", "distributions", "discountFactor", "recursion",
                                                                        "stateTransition", "immediateValue"]
        assert callable(cls.setSampleNum) and callable(cls.simulateSDPGivenSamplNum)
    assert callable(multiitem.CashSimulationMulti.simulateSDPGivenSamplNumMulti)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**Two-product rollout:**" in design and "generateLHSamplesMultiProd" in design


@pytest.mark.parametrize("cid", ["mc-0", "xr-0", "kat1"])
def test_create_refusals_come_before_any_device_call_and_name_the_argument(sia, lib, oracle, cid):
    rows = np.array(cases.reference(oracle, cid)["rows"])
    n = len(rows)
    T = cases.case(cid)[1]["T"]
    assert n >= 3 and rows[0, 0] == 1 and (rows[1:, 0] > 1).all()

    def expect(code, *words, **kw):
        rc, err = _create(sia, lib, cid, kw.pop("rows", rows), **kw)
        assert rc == code, (rc, err)
        for w in words:
            assert w in err, (w, err)

    # the descriptor, as the solves check it
    expect(ERR_ARG, "bad descriptor", kw_edit=dict(q_bound=0))
    expect(ERR_ARG, "bad descriptor", kw_edit=dict(q_bound=257))
    if cid == "mc-0":
        expect(ERR_UNSUPPORTED, "negative cash", kw_edit=dict(min_cash=-1.0))
        expect(ERR_ARG, "xr = 2", xr=2)
    if cid == "xr-0":
        expect(ERR_ARG, "deposit_rate", dep=NAN)
    # the memo
    expect(ERR_ARG, "memo is null", null_memo=True)
    expect(ERR_ARG, "memo->rows", "memo->capacity", table_edit=lambda t, a: setattr(t, "capacity", n - 1))
    expect(ERR_ARG, "memo->rows = 0", table_edit=lambda t, a: setattr(t, "rows", 0))
    for col in ("period", "i1", "i2", "q1", "q2", "cash", "value", "a1", "a2"):
        expect(ERR_ARG, "column of memo is null", table_edit=lambda t, a, col=col: setattr(t, col, None))
    # the capacity: 2^k must exceed the row count
    k_tight = n.bit_length()  # the smallest k with 2^k > n
    assert (1 << k_tight) > n >= (1 << (k_tight - 1))
    expect(ERR_ARG, "capacity_log2", capacity_log2=k_tight - 1)
    expect(ERR_ARG, "capacity_log2", capacity_log2=-1)
    expect(ERR_ARG, "capacity_log2", capacity_log2=32)
    # the rows: periods within 1 .. T, finite tuples, action pairs of the descriptor, ONE period-1 row equal to the initial state
    for bad in (0, T + 1):
        r = rows.copy()
        r[n - 1, 0] = bad
        expect(ERR_ARG, f"memo->period[{n - 1}] = {bad}", rows=r)
    r = rows.copy()
    r[1, 5] = NAN
    expect(ERR_ARG, "memo->cash[1]", "not finite", rows=r)
    r = rows.copy()
    r[2, 7] = -1
    expect(ERR_ARG, "a1 / a2[2]", "q_bound", rows=r)
    r = rows.copy()
    r[2, 8] += 300
    expect(ERR_ARG, "a1 / a2[2]", "q_bound", rows=r)
    r = rows.copy()
    r[1, 0] = 1
    expect(ERR_ARG, "rows 0 and 1 are both of period 1", rows=r)
    if T > 1:
        r = rows.copy()
        r[0, 0] = 2
        expect(ERR_ARG, "no row of period 1", rows=r)
    r = rows.copy()
    r[0, 5] += 1.0
    expect(ERR_ARG, "memo row 0", "not the descriptor's initial state", rows=r)
    r = rows.copy()
    r[0, 1] += 1.0
    r[0, 7] += 1.0 if cid == "xr-0" else 0.0  # (the XR family's levels move with x)
    expect(ERR_ARG, "memo row 0", "not the descriptor's initial state", rows=r)


def test_null_handles_and_out_pointers(sia, lib):
    from stochastic_inventory_amd._abi import SdpgpuSimResult
    res = SdpgpuSimResult()
    z = np.zeros(4)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.sdpgpu_multi_policy_simulate(None, 1, dp, dp, None, C.byref(res), None, None) == ERR_ARG
    assert "policy is null" in lib.sdpgpu_multilead_last_error().decode()
    assert lib.sdpgpu_multi_policy_simulate_sampled(None, 1, 0, 0, 0, None, C.byref(res), None, None) == ERR_ARG
    assert lib.sdpgpu_multi_policy_sample(None, 1, 0, 0, 0, dp, dp, None) == ERR_ARG
    assert lib.sdpgpu_multi_policy_lookup(None, 0, None, None, None, None, None, None, None, None, None) == ERR_ARG
    lib.sdpgpu_multi_policy_destroy(None)  # a no-op
    kind, kw, _ = cases.case("mc-0")
    from stochastic_inventory_amd import multiitem
    k = multiitem.fill_multicash(sia._abi.SdpgpuMulticash(), **kw)
    t, _arrs = multiitem.table_from_rows(np.zeros((1, 9)))
    assert lib.sdpgpu_multicash_policy_create(C.byref(k), 0, 0.0, C.byref(t), 0, None) == ERR_ARG
    assert "out is null" in lib.sdpgpu_multilead_last_error().decode()
    assert lib.sdpgpu_multilead_policy_create(None, C.byref(t), 0, C.byref(C.c_void_p())) == ERR_ARG
    assert "bad descriptor" in lib.sdpgpu_multilead_last_error().decode()


@pytest.mark.parametrize("what,code,text", [("bad_alloc", ERR_ALLOC, "host allocation failed"), ("runtime", ERR_INTERNAL, "injected"),
                                            ("other", ERR_INTERNAL, "unknown exception")])
def test_no_exception_crosses_the_new_entry_points(sia, lib, oracle, monkeypatch, what, code, text):
    """The engine's barrier (ml_guard; SDPGPU_TEST_THROW throws at the top of the guarded region, no device needed)."""
    from stochastic_inventory_amd._abi import SdpgpuSimResult
    rows = cases.reference(oracle, "mc-0")["rows"]
    monkeypatch.setenv("SDPGPU_TEST_THROW", what)
    rc, err = _create(sia, lib, "mc-0", rows)
    assert rc == code and text in err and "sdpgpu_multicash_policy_create" in err
    rc, err = _create(sia, lib, "kat1", cases.reference(oracle, "kat1")["rows"])
    assert rc == code and text in err and "sdpgpu_multilead_policy_create" in err
    res = SdpgpuSimResult()
    assert lib.sdpgpu_multi_policy_simulate_sampled(None, 1, 0, 0, 0, None, C.byref(res), None, None) == code
    assert lib.sdpgpu_multi_policy_simulate(None, 1, None, None, None, C.byref(res), None, None) == code
    assert lib.sdpgpu_multi_policy_sample(None, 1, 0, 0, 0, None, None, None) == code
    assert lib.sdpgpu_multi_policy_lookup(None, 0, None, None, None, None, None, None, None, None, None) == code
    assert text in lib.sdpgpu_multilead_last_error().decode()


@pytest.mark.parametrize("cid", ["mc-0", "xr-0", "kat1"])
def test_a_valid_memo_without_a_device_is_a_device_error(sia, lib, oracle, cid):
    has_gpu = _has_gpu()
    rows = cases.reference(oracle, cid)["rows"]
    rc, err = _create(sia, lib, cid, rows)
    assert rc == (OK if has_gpu else ERR_DEVICE) and (has_gpu or "no HIP device" in err)
    if not has_gpu:
        with pytest.raises(sia.SdpgpuError) as e:
            cases.policy(sia, cid, rows)
        assert e.value.code == ERR_DEVICE
    with pytest.raises(ValueError):
        sia.MultiPolicy("multistaff", rows)
