"""GPU test (-m gpu; it launches only the parameter packing): the launch plans and the packed parameters of both engines are what
tests/golden/plan_manifest.json.gz (gzip-compressed JSON) records -- op names, kinds, order, exact flops, cost slots, side branches, the detection-only
tail and which of its entries are the dense ops themselves, the keys of plan.named and the layout of eng.P, and of every conv / head
/ tail descriptor each integer and float field by value and each pointer field as null or not.  The record was made by
tools/gen_golden_plan_manifest.py before the RPN stage of the two plan builders was put on shared steps; the two cases with an
``engine_bf16`` knob off (plan_manifest.KNOBS) were added to it before the backbone was put on one DLA walk, with the one rename the
tool's docstring states; the descriptor fields, the benchmark's fp32 shape with the ``engine`` knobs and the batch of 20 were added
before the fp32 conv planner was split into one route per kernel family (the tool's docstring names the commit).  There is no
tolerance and no skipped field."""
import gzip
import json
import os
import re

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


# one pattern per place where the fp32 conv planner appends an op: each must match the kind of a recorded op
FP32_CONV_ROUTES = [
    r"touch", r"wino44<16,16>", r"wino44<16,32>", r"wino44<16,16,splitk\d+>", r"wino44<16,16,kpair>",
    r"wino_lds<64,32,16>", r"wino_wave<32,32>",
    r"conv_wave", r"conv_wave<deform>", r"conv_wave<wgsplit\d+>", r"conv_wave<deform,wgsplit\d+>", r"conv_wave<splitk\d+>",
    r"conv_wave<deform,splitk\d+>",
    r"igemm<\d+,\d+,\d+>", r"igemm<\d+,\d+,\d+,splitk\d+>", r"igemm<\d+,\d+,\d+,deform>", r"igemm<\d+,\d+,\d+,deform,splitk\d+>",
    r"igemm<\d+,\d+,\d+,per_image>",
]


def test_the_record_reaches_every_route_of_the_fp32_conv_planner(golden):
    kinds = {op[1] for case in golden.values() for op in case["ops"]}
    for route in FP32_CONV_ROUTES:
        assert any(re.fullmatch(route, k) for k in kinds), route
    # the wave kernel on fragment-ordered per-image weights: the logits GEMM of the unfused ANAB chain of the batch of 20
    logits = next(op for op in golden["f32-anab_fullalign-b20-160x192"]["ops"] if op[0] == "anab.logits")
    assert logits[1] == "conv_wave" and logits[4]["wgt_img_stride"] > 0, logits
    # a folded touch and a touch launch of its own: fewer touch launches than F(4x4) layers, and one per layer with a span of 0
    for case, own in (("f32-anab_fullalign-b8-384x1280", False), ("f32-anab_fullalign-b8-384x1280-WINO44_TOUCH_SPAN=0", True)):
        k = [op[1] for op in golden[case]["ops"]]
        n44, ntouch = sum(x.startswith("wino44<") for x in k), k.count("touch")
        assert 0 < ntouch and (ntouch == n44 if own else ntouch < n44), (case, n44, ntouch)


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
        assert g[:4] == w[:4], (g, w)
        assert (g[4] is None) == (w[4] is None) and sorted(g[4] or ()) == sorted(w[4] or ()), (g, w)
        for field in w[4] or ():
            assert g[4][field] == w[4][field], (g[:2], field, g[4][field], w[4][field])
    assert sorted(got["P"]) == sorted(want["P"])
    for k in want["P"]:
        assert got["P"][k] == want["P"][k], k
    assert got == want
