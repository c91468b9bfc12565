"""GPU: the three two-product recursions at the shapes where the kernels of csrc/sdpgpu_sparse.hip take another path
(tests/multi_shape_cases.py), under every launch form, against the oracle's literal memoised recursion: the root value and
action, the states per period, the cells and the WHOLE memo, bit for bit.  Every run also reports which kernel forms it
launched (sdpgpu_multi_forms_used -> result.forms), and the test asserts that those are exactly the ones the shape and the
switches are meant to reach -- a forced form that silently did not run would otherwise pass for free.

One test per instance and family: the oracle runs once, the forms are looped inside."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multi_shape_cases as msc  # noqa: E402

pytestmark = pytest.mark.gpu


def _ids(pairs):
    return [f"{c.name}-{k}" for c, k in pairs]


def _solve(sia, case, kind):
    from stochastic_inventory_amd.multiitem import multilead_solve
    kw = msc.solver_kw(case, kind)
    if kind == "multilead":
        return multilead_solve(table=True, **kw)
    if kind == "multicash":
        return sia.multicash_solve(table=True, **kw)
    return sia.multixr_solve(case.deposit, table=True, **kw)


def run_case(sia, oracle, monkeypatch, case, kind):
    """The oracle once, its preconditions, then every form: -> {form name: forms mask}."""
    from stochastic_inventory_amd._abi import MULTI_FORMS, multi_form_names
    fv, act, states, cells, want = msc.oracle_memo(oracle, case, kind)
    for name, (holds, what) in msc.preconditions(case, kind, states, cells, want).items():
        print(f"{case.name} [{kind}] {name}: {what}")
        assert holds, (case.name, kind, name, what)
    seen = {}
    for form, env in msc.forms_of(case, kind).items():
        for var in msc.SWITCHES:
            monkeypatch.delenv(var, raising=False)
        for var, val in env.items():
            monkeypatch.setenv(var, val)
        r = _solve(sia, case, kind)
        where = (case.name, kind, form)
        assert r.finalValue == fv and (r.firstAction, r.secondAction) == act, where
        assert r.statesPerPeriod == states and r.cells == cells, where
        assert r.table.shape == want.shape == (sum(states), 9), where
        differ = np.flatnonzero((r.table != want).any(axis=1))
        assert differ.size == 0, (where, f"{differ.size} of {len(want)} memo rows differ, the first: engine "
                                         f"{r.table[differ[0]].tolist()} oracle {want[differ[0]].tolist()}")
        expect = msc.expected_forms(case, kind, env, MULTI_FORMS)
        assert r.forms == expect, (where, "launched", multi_form_names(r.forms), "expected", multi_form_names(expect))
        seen[form] = r.forms
    for var in msc.SWITCHES:
        monkeypatch.delenv(var, raising=False)
    return seen


@pytest.mark.parametrize("case,kind", msc.cases_of("runs"), ids=_ids(msc.cases_of("runs")))
def test_runs(sia, oracle, monkeypatch, case, kind):
    """Runs of 4, 5, 7, 8 and 9 pairs: the grouped walk of a run and its tail."""
    run_case(sia, oracle, monkeypatch, case, kind)


@pytest.mark.parametrize("case,kind", msc.cases_of("irregular_lists"), ids=_ids(msc.cases_of("irregular_lists")))
def test_irregular_lists(sia, oracle, monkeypatch, case, kind):
    """Lists that are not made of equal runs: the pair-by-pair walk."""
    run_case(sia, oracle, monkeypatch, case, kind)


@pytest.mark.parametrize("case,kind", msc.cases_of("two_passes"), ids=_ids(msc.cases_of("two_passes")))
def test_two_passes(sia, oracle, monkeypatch, case, kind):
    """Qbound 51, 53, 65: a second pass of the action range, best actions on both sides of the pass boundary."""
    run_case(sia, oracle, monkeypatch, case, kind)


@pytest.mark.parametrize("case,kind", msc.cases_of("wide_list"), ids=_ids(msc.cases_of("wide_list")))
def test_wide_list(sia, oracle, monkeypatch, case, kind):
    """529 demand pairs: more than one trip of the staging loops."""
    run_case(sia, oracle, monkeypatch, case, kind)


@pytest.mark.parametrize("case,kind", msc.cases_of("tables_beyond_lds"), ids=_ids(msc.cases_of("tables_beyond_lds")))
def test_tables_beyond_lds(sia, oracle, monkeypatch, case, kind):
    """The launcher leaves the factored kernels BY ITSELF in the period whose tables outgrow the LDS: backward_kernel (never
    otherwise run for these two families) and, on the lattice, lattice_mark_kernel -- no switch names them."""
    from stochastic_inventory_amd._abi import MULTI_FORMS as F
    seen = run_case(sia, oracle, monkeypatch, case, kind)
    assert seen["default"] & F["BACKWARD"] and seen["default"] & F["FACT_LAST"]
    assert seen["lattice"] & F["BACKWARD"] and seen["lattice"] & F["LATTICE_MARK"] and not seen["lattice"] & F["FACT_MARK"]


@pytest.mark.parametrize("case,kind", msc.cases_of("lead_chunk_edges"), ids=_ids(msc.cases_of("lead_chunk_edges")))
def test_lead_chunk_edges(sia, oracle, monkeypatch, case, kind):
    """NA = 64, 81, 625, 676, 1296, 4096, 4225: chunk and pass edges of the wave kernel; with no switch set, Qbound 64 is the
    wave kernel's and Qbound 65 backward_kernel's (one action at a time)."""
    from stochastic_inventory_amd._abi import MULTI_FORMS as F
    seen = run_case(sia, oracle, monkeypatch, case, kind)
    if case.kw["q_bound"] == 65:
        assert seen["default"] & F["BACKWARD"] and not seen["default"] & F["LEAD_WAVE"]
    else:
        assert seen["default"] & F["LEAD_WAVE"] and not seen["default"] & F["BACKWARD"]


@pytest.mark.parametrize("case,kind", msc.cases_of("lead_deep_passes"), ids=_ids(msc.cases_of("lead_deep_passes")))
def test_lead_deep_passes(sia, oracle, monkeypatch, case, kind):
    """Three periods at 676 order pairs: the not-last two-pass walk on many states."""
    run_case(sia, oracle, monkeypatch, case, kind)


@pytest.mark.parametrize("case,kind", msc.cases_of("lead_wide_list"), ids=_ids(msc.cases_of("lead_wide_list")))
def test_lead_wide_list(sia, oracle, monkeypatch, case, kind):
    """64, 65 and 72 demand pairs: a wave's staging loop beyond its first trip."""
    run_case(sia, oracle, monkeypatch, case, kind)


@pytest.mark.parametrize("case,kind", msc.cases_of("lead_workgroup_form"), ids=_ids(msc.cases_of("lead_workgroup_form")))
def test_lead_workgroup_form(sia, oracle, monkeypatch, case, kind):
    """Qbound 16, 17, 50, 51 under SDPGPU_MULTI_WAVE=0: lead_actions<1>, <2>, <10> and the loop beyond 2560 order pairs."""
    from stochastic_inventory_amd._abi import MULTI_FORMS as F
    seen = run_case(sia, oracle, monkeypatch, case, kind)
    assert seen["workgroup"] == F["SORTED_FORWARD"] | F["BACKWARD"]


def test_every_form_bit_is_expected_by_some_case():
    """Every bit of the forms mask is in the expected set of at least one (instance, form) above."""
    from stochastic_inventory_amd._abi import MULTI_FORMS
    union = 0
    for builder in msc.BUILDERS:
        for case, kind in msc.cases_of(builder):
            for env in msc.forms_of(case, kind).values():
                union |= msc.expected_forms(case, kind, env, MULTI_FORMS)
    assert union == sum(MULTI_FORMS.values()), [n for n, b in MULTI_FORMS.items() if not union & b]
