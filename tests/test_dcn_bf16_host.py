"""CPU tests of the bf16 DCNv2 operator's host side: the four entry points in the header, its additive list and the binding, the
workspace queries (pure host arithmetic), the CPU refusal, and the legitimacy of the exact-arithmetic backward cases that
tests/test_gpu_dcn_bf16.py compares bit for bit."""
import re

import pytest
import torch

from m3dssd_amd import _hip
import dcn_bf16_cases as C
import dcn_grad_ref as R
import exact_inputs as X

NAMES = ("m3d_dcn_v2_forward_bf16", "m3d_dcn_v2_workspace_bytes_bf16", "m3d_dcn_v2_backward_bf16",
         "m3d_dcn_v2_backward_workspace_bytes_bf16")


def test_entry_points_are_declared_listed_and_bound():
    text = open(_hip.HEADER).read()
    assert re.search(r"#define\s+M3D_ABI_VERSION\s+5\b", text)
    additive = text[text.index("added under 5"):text.index("#define M3D_ABI_VERSION")]
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name + " is not declared"
        assert re.search(r"\b%s\b" % name, additive), name + " is not in the additive list"
        assert name in _hip.SIGNATURES, name
    assert _hip.SIGNATURES["m3d_dcn_v2_workspace_bytes_bf16"][1] == [_hip.c_int] * 11
    assert _hip.SIGNATURES["m3d_dcn_v2_backward_workspace_bytes_bf16"][1] == [_hip.c_int] * 11


def test_workspace_queries_answer_on_the_host():
    L = _hip.lib()
    assert L.m3d_abi_version() == 5
    for q in (L.m3d_dcn_v2_workspace_bytes_bf16, L.m3d_dcn_v2_backward_workspace_bytes_bf16):
        n1 = q(2, 24, 10, 12, 8, 3, 3, 1, 1, 1, 3)
        assert n1 > 0 and n1 % 256 == 0
        assert q(2, 24, 10, 12, 8, 3, 3, 1, 1, 1, 5) == -1          # 5 does not divide 24
        assert q(2, 24, 10, 12, 8, 3, 3, 1, 1, 1, 0) == -1
        assert q(2, 24, 10, 12, 8, 3, 3, 1, 2, 2, 1) == -1          # dilation 2: not on the bf16 path
        assert q(4, 24, 10, 12, 8, 3, 3, 1, 1, 1, 3) > n1           # grows with the batch
        assert q(2, 24, 10, 12, 8, 3, 3, 2, 1, 1, 3) < n1           # stride 2: a quarter of the output pixels


def test_cpu_tensors_are_refused():
    from m3dssd_amd.host import ops
    x = torch.zeros(1, 8, 5, 5, dtype=torch.bfloat16)
    off, m = torch.zeros(1, 18, 5, 5), torch.ones(1, 9, 5, 5)
    wt, b = torch.zeros(4, 8, 3, 3), torch.zeros(4)
    with pytest.raises(NotImplementedError):
        ops.dcn_v2_forward(x, off, m, wt, b, 1, 1)
    with pytest.raises(NotImplementedError):
        ops.dcn_v2_backward(x, off, m, wt, torch.zeros(1, 4, 5, 5, dtype=torch.bfloat16), 1, 1)
    with pytest.raises(NotImplementedError):
        ops.dcn_v2(x, off, m, wt, b, 1, 1)


@pytest.mark.parametrize("spec", C.EXACT_BWD_CASES)
def test_exact_backward_cases_are_legitimate(spec):
    """The premise of the bit-for-bit backward test: the float64 gradients are what float32 arithmetic gives as well, and the two
    intermediates the kernel may keep narrow survive a bf16 round trip."""
    ops, go, ts, args = C.exact_bwd_case(spec)
    assert spec[5] <= 16 and set(go.unique().tolist()) <= {-2.0, -1.0, 1.0, 2.0}
    out64, g64 = R.ref_grads(ts, go, args, dt=torch.float64)
    out32, g32 = R.ref_grads(ts, go, args, dt=torch.float32)
    assert torch.equal(out64, out32.double())
    for name, a, b in zip(("input", "offset", "mask", "weight", "bias"), g64, g32):
        assert torch.equal(a, b.double()), name
        assert a.abs().max() > 0, name
    # the forward of the restatement is the forward of exact_inputs (two independent statements of the operator)
    assert torch.equal(out64, X.dcn_ref(ops))
    col, gcol = C.col_gcol64(ops, go)
    assert torch.equal(col, X._rt(col, X.BF16)) and col.abs().max() > 0
    assert torch.equal(gcol, X._rt(gcol, X.BF16))
    assert float(gcol.abs().max()) <= 64 and torch.equal(gcol * 2, torch.round(gcol * 2))


@pytest.mark.parametrize("shape", C.EXACT_FWD_CASES)
def test_exact_forward_cases_are_legitimate(shape):
    n, c, h, w, co, k, pad, dg = shape
    ops = X.dcn_operands(sum(shape), n, c, h, w, co, k, pad, dg)
    X.assert_exact_under(X.dcn_ref, ops, X.BF16)
