"""GPU test (-m gpu; it launches only the parameter packing): the launch plans and the packed parameters of both engines are what
tests/golden/plan_manifest.json.gz (gzip-compressed JSON) records -- op names, kinds, order, exact flops, cost slots, side branches, the detection-only
tail and which of its entries are the dense ops themselves, the keys of plan.named and the layout of eng.P.  The record was made by
tools/gen_golden_plan_manifest.py before the RPN stage of the two plan builders was put on shared steps; the two cases with an
``engine_bf16`` knob off (plan_manifest.KNOBS) were added to it before the backbone was put on one DLA walk, with the one rename the
tool's docstring states.  There is no tolerance and no skipped field."""
import gzip
import json
import os

import pytest

import plan_manifest
from gpu_common import GOLDEN, _dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(GOLDEN, "plan_manifest.json.gz"), "rt") as f:
        return json.load(f)


def test_the_record_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(plan_manifest.CASES)


@pytest.mark.parametrize("case", list(plan_manifest.CASES))
def test_plan_and_packed_parameters_match_the_record(case, golden):
    _dev()
    got = json.loads(json.dumps(plan_manifest.dump_case(case)))           # (tuples -> lists, as the record was written)
    want = golden[case]
    assert sorted(got) == sorted(want)
    for field in ("branches", "tail_start", "tail", "tail_is_dense", "named"):
        assert got[field] == want[field], field
    assert [op[:2] for op in got["ops"]] == [op[:2] for op in want["ops"]]
    for g, w in zip(got["ops"], want["ops"]):
        assert g == w, (g, w)
    assert sorted(got["P"]) == sorted(want["P"])
    for k in want["P"]:
        assert got["P"][k] == want["P"][k], k
    assert got == want
