"""CPU: the instance builders of tests/multi_shape_cases.py -- what they claim that needs no memo (list shapes, LDS
arithmetic, action counts), the oracle-side preconditions on the cheap instances, and that the forms a GPU run is put under
expect every bit of the forms mask somewhere.  (The full check, every instance through the oracle, is
`python tests/multi_shape_cases.py --check`; its output is profiles/multi_shape_cases.txt.)"""
import multi_shape_cases as msc


def test_list_shapes_are_what_the_builders_claim():
    shapes = set()
    for case in msc.runs():
        for rows, run in zip(case.kw["pmf"], case.claims["fact_run"]):
            idx, nu1, nu2 = msc.fact_index_words(rows)
            assert msc.fact_run(idx) == run == nu2 and len(rows) == nu1 * nu2 and case.kw["q_bound"] <= 8
            shapes.add((nu1, nu2))
    assert shapes == set(msc.RUN_SHAPES) and any(c.kw["T"] == 3 for c in msc.runs())
    irregular = msc.irregular_lists()
    assert sum(c.claims["fact_run"] == [0, 0] for c in irregular) >= 4
    for case in irregular + msc.two_passes() + msc.wide_list() + msc.tables_beyond_lds():
        assert [msc.fact_run(msc.fact_index_words(t)[0]) for t in case.kw["pmf"]] == case.claims["fact_run"], case.name
    assert sorted(c.kw["q_bound"] for c in msc.two_passes()) == [51, 53, 65]
    assert all(len(c.kw["pmf"][c.claims["wide_period"]]) == 529 and c.kw["q_bound"] <= 12 for c in msc.wide_list())
    (beyond,) = msc.tables_beyond_lds()
    _, nu1, nu2 = msc.fact_index_words(beyond.kw["pmf"][0])
    assert (beyond.kw["q_bound"], nu1 + nu2) == (40, 171) and 40 * 171 * 24 > msc.LDS_BYTES
    assert msc.fact_lds_bytes(40, 170, 171, False) > msc.LDS_BYTES < msc.fact_lds_bytes(40, 170, 171, False, mark=True)


def test_lead_time_shapes():
    assert [c.kw["q_bound"] ** 2 for c in msc.lead_chunk_edges()] == [64, 81, 625, 676, 1296, 4096, 4225]
    assert all(c.kw["T"] == 2 for c in msc.lead_chunk_edges())
    assert all(c.kw["T"] == 3 and c.kw["q_bound"] == 26 for c in msc.lead_deep_passes())
    wide = msc.lead_wide_list()
    assert {c.claims["pairs"] for c in wide} == {64, 65, 72} and {c.kw["T"] for c in wide} == {2, 3}
    assert all(c.kw["q_bound"] <= 6 for c in wide)
    assert [c.kw["q_bound"] for c in msc.lead_workgroup_form()] == [16, 17, 50, 51]


def test_pass_boundaries():
    assert msc.pass_boundary("multicash", 51) == 2560 and msc.pass_boundary("multixr", 51) == 2550
    assert msc.pass_boundary("multixr", 53) == 2385 and msc.pass_boundary("multixr", 65) == 2275


def test_preconditions_hold_on_the_cheap_instances(oracle):
    for builder in ("runs", "irregular_lists", "lead_wide_list", "lead_deep_passes"):
        for case, kind in msc.cases_of(builder):
            _, _, states, cells, table = msc.oracle_memo(oracle, case, kind)
            for name, (holds, what) in msc.preconditions(case, kind, states, cells, table).items():
                assert holds, (case.name, kind, name, what)


def test_every_form_bit_is_expected_by_some_case(sia):
    from stochastic_inventory_amd._abi import MULTI_FORMS
    union = 0
    for builder in msc.BUILDERS:
        for case, kind in msc.cases_of(builder):
            for env in msc.forms_of(case, kind).values():
                union |= msc.expected_forms(case, kind, env, MULTI_FORMS)
    assert union == sum(MULTI_FORMS.values()), [n for n, b in MULTI_FORMS.items() if not union & b]
