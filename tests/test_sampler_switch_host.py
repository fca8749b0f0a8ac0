"""The sampler switch against its recorded answers (tests/golden/sampler_switch.json, written by tools/make_sampler_switch_golden.py before
the switch became one table): the whole grid of tests/sampler_switch_cases.py, through the two check functions chained the way
``interface._run`` chained them and through ``sampler.resolve_sampler``.  Every row is compared; none is skipped."""
import json
import os

from layoutllm_t2i_amd import interface as itf
from layoutllm_t2i_amd import sampler as smp

import sampler_switch_cases as sc

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_switch.json")))


def _chained(sampler, ddim_eta, ddim_discretize, dpm_order, dpm_discretize):
    sampler_args = itf.check_sampler_args(sampler, ddim_eta, ddim_discretize)
    return sampler_args + itf.check_dpm_args(sampler_args[0], dpm_order, dpm_discretize, *sampler_args[1:])


def _resolved(row):
    spec, values = smp.resolve_sampler(row)
    assert spec is smp.SAMPLER_TABLE[values["sampler"]] and set(values) == set(sc.KEYS)
    kwargs = spec.kwargs(values)
    assert list(kwargs) == [k.kwarg for k in spec.keys] and all(kwargs[k.kwarg] is values[k.name] for k in spec.keys)
    return [values[k] for k in sc.KEYS]


def test_the_golden_holds_the_whole_grid():
    rows = sc.rows()
    assert GOLD["keys"] == list(sc.KEYS) and GOLD["axes"] == [[repr(v) for v in axis] for axis in sc.AXES]
    assert len(rows) == len(GOLD["rows"]) == 5 * 6 * 3 * 5 * 4
    kinds = {o[0] for o in GOLD["outcomes"]}
    assert kinds == {"ok", "raises"} and {o[1] for o in GOLD["outcomes"] if o[0] == "raises"} == {"ValueError"}
    assert sorted(set(GOLD["rows"])) == list(range(len(GOLD["outcomes"])))


def test_every_row_answers_as_recorded_through_the_check_functions_and_through_the_resolver():
    wrong = []
    for n, (row, want) in enumerate(zip(sc.rows(), (GOLD["outcomes"][i] for i in GOLD["rows"]))):
        for how, fn in (("check_sampler_args + check_dpm_args", lambda: _chained(**row)), ("resolve_sampler", lambda: _resolved(row))):
            got = sc.outcome(fn)
            if got != want:
                wrong.append((n, row, how, got, want))
    assert not wrong, f"{len(wrong)} differences, the first: {wrong[0]}"


def test_the_table_is_what_the_callers_read():
    assert itf.SAMPLERS is smp.SAMPLERS == ("plms", "ddim", "dpmpp_2m") and smp.DEFAULT_SAMPLER == "plms"
    assert smp.SAMPLER_KEYS == sc.KEYS
    assert [s.cls for s in smp.SAMPLER_TABLE.values()] == [smp.PLMSSampler, smp.DDIMSampler, smp.DPMSolverSampler]
    spec, values = smp.resolve_sampler({})
    assert spec.name == "plms" and spec.kwargs(values) == {}
    assert values == dict(sampler="plms", ddim_eta=0.0, ddim_discretize="uniform", dpm_order=2, dpm_discretize="logsnr")
    spec, values = smp.resolve_sampler(dict(sampler="ddim", ddim_eta=1, steps=4))          # a whole args dict will do; eta comes back a float
    assert spec.kwargs(values) == dict(eta=1.0, discretize="uniform") and isinstance(values["ddim_eta"], float)
    spec, values = smp.resolve_sampler(dict(sampler="dpmpp_2m", dpm_order=1))
    assert spec.kwargs(values) == dict(order=1, discretize="logsnr")
