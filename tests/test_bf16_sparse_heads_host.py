"""CPU tests of the bf16 sparse heads' C ABI: the row-list forms of the fused bf16 head and of the one-launch bf16 attention are
declared in the public header, bound in ``_hip.SIGNATURES`` and exported by the built library."""
import os
import re

from m3dssd_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("m3d_head_mlp2_bf16_forward_rows", "m3d_anab_attend_bf16_rows")


def test_bf16_row_list_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "m3dssd_hip.h")).read()
    L = _hip.lib()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name          # a declaration, not a mention in a comment
        assert name in _hip.SIGNATURES, name
        assert getattr(L, name) is not None, name
    # the argument lists: the dense call's, then the list and its device-side length in front of the stream
    for dense, rows in (("m3d_head_mlp2_bf16_forward", NAMES[0]), ("m3d_anab_attend_bf16", NAMES[1])):
        (rd, ad), (rr, ar) = _hip.SIGNATURES[dense], _hip.SIGNATURES[rows]
        assert rr is rd and len(ar) == len(ad) + 2 and list(ar[:len(ad) - 1]) == list(ad[:-1])
    # additive under ABI 5
    assert "m3d_head_mlp2_bf16_forward_rows, m3d_anab_attend_bf16_rows (additive)" in header
    assert L.m3d_abi_version() == 5
