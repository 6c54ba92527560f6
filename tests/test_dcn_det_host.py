"""CPU tests of the deterministic DCNv2 backward's host side: the four entry points in the header, its additive list and the
binding; the two workspace queries (pure host arithmetic) against the float form's; the mode switch of ops and the CPU refusal."""
import re

import pytest
import torch

from m3dssd_amd import _hip
from test_gpu_dcn_backward import PARITY_CASES

NAMES = ("m3d_dcn_v2_backward_det", "m3d_dcn_v2_backward_det_bf16", "m3d_dcn_v2_backward_det_workspace_bytes",
         "m3d_dcn_v2_backward_det_workspace_bytes_bf16")


def test_entry_points_are_declared_listed_and_bound():
    text = open(_hip.HEADER).read()
    assert re.search(r"#define\s+M3D_ABI_VERSION\s+5\b", text)
    additive = text[text.index("added under 5"):text.index("#define M3D_ABI_VERSION")]
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name + " is not declared"
        assert re.search(r"\b%s\b" % name, additive), name + " is not in the additive list"
        assert name in _hip.SIGNATURES, name
    # the argument lists of the two existing backward entries and of their queries
    for new, old in (("m3d_dcn_v2_backward_det", "m3d_dcn_v2_backward"), ("m3d_dcn_v2_backward_det_bf16", "m3d_dcn_v2_backward_bf16"),
                     ("m3d_dcn_v2_backward_det_workspace_bytes", "m3d_dcn_v2_backward_workspace_bytes"),
                     ("m3d_dcn_v2_backward_det_workspace_bytes_bf16", "m3d_dcn_v2_backward_workspace_bytes_bf16")):
        assert _hip.SIGNATURES[new] == _hip.SIGNATURES[old], new
    L = _hip.lib()                                                       # resolves every declared name
    assert L.m3d_abi_version() == 5
    for name in NAMES:
        assert getattr(L, name) is not None


def test_workspace_queries_answer_on_the_host_and_cover_the_float_form():
    L = _hip.lib()
    pairs = ((L.m3d_dcn_v2_backward_det_workspace_bytes, L.m3d_dcn_v2_backward_workspace_bytes, False),
             (L.m3d_dcn_v2_backward_det_workspace_bytes_bf16, L.m3d_dcn_v2_backward_workspace_bytes_bf16, True))
    for det, flt, bf16 in pairs:
        for (n, c, co, h, w, k, stride, pad, dil, G, _, _) in PARITY_CASES:
            q = (n, c, h, w, co, k, k, stride, pad, dil, G)
            have, base = det(*q), flt(*q)
            if base <= 0:                                                # (bf16: the dilated row)
                assert bf16 and dil != 1 and have <= 0, q
                continue
            assert have >= base and have % 256 == 0, q
            # the staging buffer of grad_input doubles: at least 4 more bytes per padded input element
            assert have - base >= n * h * w * ((c // G + 63) // 64 * 64) * 4, q
        # what the float queries refuse
        for q in ((2, 24, 10, 12, 8, 3, 3, 1, 1, 1, 5), (2, 24, 10, 12, 8, 3, 3, 1, 1, 1, 0), (0, 24, 10, 12, 8, 3, 3, 1, 1, 1, 1),
                  (2, 24, 10, 12, 8, 3, 3, 0, 1, 1, 1)):
            assert flt(*q) <= 0 and det(*q) <= 0, q
        q = (2, 24, 10, 12, 8, 3, 3, 1, 2, 2, 1)                         # dilation 2: fp32 only
        assert (flt(*q) <= 0) == bf16 and (det(*q) <= 0) == bf16
        assert det(4, 24, 10, 12, 8, 3, 3, 1, 1, 1, 3) > det(2, 24, 10, 12, 8, 3, 3, 1, 1, 1, 3)


def test_mode_follows_the_pytorch_flag_and_overrides_it():
    from m3dssd_amd.host import ops
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    assert ops.set_dcn_deterministic(None) is None                       # the default
    try:
        torch.use_deterministic_algorithms(False)
        assert ops.dcn_deterministic() is False
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert ops.dcn_deterministic() is True
        torch.use_deterministic_algorithms(True)
        assert ops.dcn_deterministic() is True
        assert ops.set_dcn_deterministic(False) is None and ops.dcn_deterministic() is False
        torch.use_deterministic_algorithms(False)
        assert ops.set_dcn_deterministic(True) is False and ops.dcn_deterministic() is True
        assert ops.set_dcn_deterministic(None) is True and ops.dcn_deterministic() is False
        with pytest.raises(TypeError):
            ops.set_dcn_deterministic(1)
        assert ops.set_dcn_deterministic(None) is None
    finally:
        ops.set_dcn_deterministic(None)
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_tensors_are_refused(dtype):
    from m3dssd_amd.host import ops
    x = torch.zeros(1, 8, 5, 5, dtype=dtype)
    off, m = torch.zeros(1, 18, 5, 5), torch.ones(1, 9, 5, 5)
    wt = torch.zeros(4, 8, 3, 3)
    for det in (None, True, False):
        with pytest.raises(NotImplementedError):
            ops.dcn_v2_backward(x, off, m, wt, torch.zeros(1, 4, 5, 5, dtype=dtype), 1, 1, deterministic=det)
    prev = ops.set_dcn_deterministic(True)
    try:
        with pytest.raises(NotImplementedError):
            ops.dcn_v2(x, off, m, wt, torch.zeros(4), 1, 1)
    finally:
        ops.set_dcn_deterministic(prev)
