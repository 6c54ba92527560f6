"""The route of m3d_conv_bf16_forward on the host: which of its eight kernels the library names for a descriptor
(m3d_conv_bf16_variant; one function in csrc/bf16_conv.hip decides it for the query and for the launch).  The query reads no
memory behind the descriptor's pointers, so tests/bf16_conv_routes.py fills them with made-up addresses and nothing runs on a GPU.

  * the 124 416 descriptors of the grid answer what tests/golden/bf16_conv_routes.json.gz records (made before the two chains
    became one: tools/gen_golden_bf16_conv_routes.py);
  * the shapes the GPU tests pin a `variant=` on answer that variant;
  * each M3D_BF16_* knob moves the routes it names and no other (one fresh process per setting: a knob is read once);
  * engine_bf16.conv_bf16_kind labels the eight codes and refuses the rest.
"""
import collections
import gzip
import json
import os
import subprocess
import sys

import pytest

import bf16_conv_routes as R
from m3dssd_amd import _hip

C = {name[len("M3D_BF16_CONV_"):]: value for name, value in _hip.CONSTANTS.items() if name.startswith("M3D_BF16_CONV_")}


def test_the_header_names_the_codes():
    assert C == {"IGEMM": 0, "HALO16": 1, "HALO32": 2, "DCN_PATCH8": 3, "DCN_PATCH16": 4, "WIDE": 5, "DCN1X1": 6, "C64": 8}
    assert _hip.CONSTANTS["M3D_ABI_VERSION"] == 5


def test_null_descriptor():
    assert R.lib().m3d_conv_bf16_variant(None) == -1


def test_grid_equals_the_record():
    with gzip.open(R.RECORD, "rt") as f:
        record = json.load(f)
    assert record["grid"] == json.loads(json.dumps([[name, values] for name, values in R.GRID]))
    want = record["codes"]
    assert len(want) == 124416
    counts = collections.Counter(want)
    assert set(counts) == {str(v) for v in C.values()}
    assert min(counts.values()) >= 12, counts           # the grid cannot silently lose a route
    got = R.grid_codes()
    assert len(got) == len(want)
    assert got == want, "first difference at descriptor %d" % next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)


def _rup32(c):
    return (c + 31) // 32 * 32


def test_shapes_of_the_gpu_tests_answer_their_variant():
    import test_gpu_bf16 as T
    import test_gpu_poison as P
    halo = [R.code(n, c, h, w, _rup32(co), cout=co, out_mode=om, sigmoid_from=sg) for n, c, h, w, co, _, _, sg, om, _ in T.HALO_CASES]
    assert halo == [case[-1] for case in T.HALO_CASES] == [1, 1, 0, 1, 1, 0, 1, 1, 2, 2, 1]
    for n, c, h, w, co, _, _, _ in T.WIDE_CASES:
        assert R.code(n, c, h, w, _rup32(co), cout=co, wgt_wave=1) == C["WIDE"]
    names, cases = T.test_conv_bf16_c64_persistent_kernel_matches_torch_and_the_halo_tile.pytestmark[0].args
    assert names.split(",")[:3] == ["n", "h", "w"] and len(cases) == 3
    for n, h, w, *_ in cases:
        assert R.code(n, 64, h, w, 64) == C["C64"]
    assert sorted(P.BF16_CONV_SHAPES) == sorted(C.values())
    for variant, (n, c, h, w, co) in P.BF16_CONV_SHAPES.items():           # as test_gpu_poison._bf16_conv_args describes them
        deform = variant in (C["DCN_PATCH8"], C["DCN_PATCH16"], C["DCN1X1"])
        got = R.code(n, c, h, w, _rup32(co), cout=co, k=1 if variant == C["DCN1X1"] else 3, deform=deform,
                     patch=deform and variant != C["DCN1X1"], wgt_wave=variant == C["WIDE"], out_mode=1 if variant == C["HALO32"] else 0)
        assert got == variant, (variant, got)


# the codes of R.PROBES under each setting; what a knob moves is what differs from the first row
PROBE_CODES = {
    "": [8, 1, 2, 5, 6, 3, 4, 0, 4],
    "M3D_BF16_C64=0": [1, 1, 2, 5, 6, 3, 4, 0, 4],
    "M3D_BF16_HALO=0": [8, 0, 0, 5, 6, 3, 4, 0, 4],
    "M3D_BF16_HALO=2": [8, 1, 1, 5, 6, 3, 4, 0, 4],
    "M3D_BF16_WIDE=0": [8, 1, 2, 1, 6, 3, 4, 0, 4],
    "M3D_BF16_DCN1X1=0": [8, 1, 2, 5, 0, 3, 4, 0, 4],
    "M3D_BF16_DCN_PATCH=0": [8, 1, 2, 5, 6, 0, 0, 0, 0],
}


def test_each_knob_moves_the_routes_it_names():
    assert R.probe_codes() == PROBE_CODES[""]
    children = {}
    for setting in PROBE_CODES:                            # plain CPU processes, all started before the first is waited for
        env = dict(os.environ, **dict([setting.split("=")] if setting else []))
        children[setting] = subprocess.Popen([sys.executable, R.__file__], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for setting, child in children.items():
        out, err = child.communicate(timeout=120)
        assert child.returncode == 0, (setting, err[-2000:])
        assert [int(v) for v in out.split()] == PROBE_CODES[setting], setting


def test_kind_labels():
    from m3dssd_amd.engine_bf16 import BF16_CONV_KINDS, conv_bf16_kind
    assert sorted(BF16_CONV_KINDS) == sorted(C.values())
    assert conv_bf16_kind(C["IGEMM"], 32, False) == "bf16_conv<32>"
    assert conv_bf16_kind(C["IGEMM"], 192, False) == "bf16_conv<64>"
    assert conv_bf16_kind(C["IGEMM"], 128, True) == "bf16_conv<128,deform>"
    assert conv_bf16_kind(C["HALO16"], 256, False) == "bf16_halo<128,16>"
    assert conv_bf16_kind(C["HALO16"], 32, False) == "bf16_halo<32,16>"
    assert conv_bf16_kind(C["HALO32"], 64, False) == "bf16_halo<64,32>"
    assert conv_bf16_kind(C["DCN_PATCH8"], 128, True) == "bf16_dcn_patch<8>"
    assert conv_bf16_kind(C["DCN_PATCH16"], 128, True) == "bf16_dcn_patch<16>"
    assert conv_bf16_kind(C["WIDE"], 128, False) == "bf16_wide<128,128>"
    assert conv_bf16_kind(C["DCN1X1"], 128, True) == "bf16_dcn1x1"
    assert conv_bf16_kind(C["C64"], 64, False) == "bf16_c64"
    for code in (7, 9, -1):
        with pytest.raises(ValueError):
            conv_bf16_kind(code, 128, False)
