"""CPU checks of the DCNv2 backward: the C ABI carries the two new entry points, the workspace rule answers without a GPU, the
float64 autograd yardstick of the GPU tests (tests/dcn_grad_ref.py) is pinned against the forward oracle and gradcheck, and
the host layer still refuses CPU tensors."""
import re

import pytest
import torch

from m3dssd_amd import _hip

import dcn_grad_ref as R


def _prototype_arg_count(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(_hip.HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
    assert m, "%s is not declared in include/m3dssd_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_library_and_binding_carry_the_backward_entry_points():
    L = _hip.lib()
    for name, nargs in (("m3d_dcn_v2_backward", 27), ("m3d_dcn_v2_backward_workspace_bytes", 11)):
        assert _prototype_arg_count(name) == nargs
        assert hasattr(L, name), name
        assert name in _hip.SIGNATURES
        assert len(_hip.SIGNATURES[name][1]) == nargs
    assert L.m3d_abi_version() == 5


def test_backward_workspace_rule():
    L = _hip.lib()
    f = L.m3d_dcn_v2_backward_workspace_bytes
    assert f(2, 6, 12, 10, 5, 3, 3, 1, 1, 1, 4) == -1            # 4 does not divide 6
    assert f(2, 6, 12, 10, 5, 3, 3, 1, 1, 1, 0) == -1
    for shape in ((128, 48, 160, 128, 3, 3, 1, 1, 1, 1), (6, 12, 10, 5, 3, 3, 1, 2, 2, 3), (128, 16, 40, 128, 1, 1, 1, 0, 1, 1)):
        sizes = [f(b, *shape) for b in (1, 2, 3, 4, 8)]
        assert all(s > 0 for s in sizes), sizes
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes


# batch, channels, height, width, channels_out, kernel_h, kernel_w, stride, pad, dilation, deformable_group ->
# m3d_dcn_v2_workspace_bytes_grouped, m3d_dcn_v2_backward_workspace_bytes, m3d_dcn_v2_workspace_bytes_bf16,
# m3d_dcn_v2_backward_workspace_bytes_bf16
WORKSPACE_PINS = [
    ((1, 24, 10, 12, 8, 3, 3, 1, 1, 1, 3), (110336, 1101568, 35328, 858880)),                      # 3x3, three deformable groups
    ((2, 32, 13, 17, 128, 3, 3, 1, 1, 1, 1), (480000, 4901888, 386304, 4075520)),                  # Co % 128 == 0: the wide fp32 tile
    ((1, 8, 10, 12, 72, 3, 3, 2, 1, 1, 2), (183808, 808960, 47616, 603904)),                       # stride 2, two groups, Co = 72
    ((2, 16, 7, 9, 16, 1, 1, 1, 0, 1, 1), (34560, 212992, 18432, 156416)),                         # 1x1 pad 0
    ((1, 6, 12, 10, 5, 3, 3, 1, 2, 2, 3), (110336, 1101568, -1, -1)),                              # dilation 2 pad 2: no bf16 form
    ((4, 256, 24, 80, 256, 3, 3, 1, 1, 1, 1), (18948096, 236819456, 13836288, 159341568)),         # network size: 256 -> 256 at 24x80
    ((2, 6, 12, 10, 5, 3, 3, 1, 1, 1, 4), (-1, -1, -1, -1)),                                       # 4 does not divide 6
    ((3, 20, 11, 13, 72, 3, 3, 1, 1, 1, 1), (374272, 4827136, 260864, 4020992)),                   # odd everything, Co = 72
    ((1, 72, 5, 7, 12, 3, 3, 1, 1, 1, 1), (240640, 961536, 88576, 720128)),                        # C past one wave, 35 pixels
]


@pytest.mark.parametrize("shape,expected", WORKSPACE_PINS)
def test_workspace_queries_are_pinned(shape, expected):
    """The four workspace queries of the DCNv2 operator are ABI: callers size their buffers by them and the M3D_E_WORKSPACE
    messages quote them.  The expected byte counts were taken from the library built at commit e8e42fb, the last one with a
    separate fp32 and bf16 workspace planner (the queries are host arithmetic and ran on a machine without a GPU); they are not
    recomputed from the code under test."""
    L = _hip.lib()
    got = tuple(int(f(*shape)) for f in (L.m3d_dcn_v2_workspace_bytes_grouped, L.m3d_dcn_v2_backward_workspace_bytes,
                                         L.m3d_dcn_v2_workspace_bytes_bf16, L.m3d_dcn_v2_backward_workspace_bytes_bf16))
    assert got == expected


@pytest.mark.parametrize("spec", R.PIN_CASES)
def test_yardstick_forward_matches_the_oracle(spec):
    """The float32 forward of the restatement against oracle.dcn.dcn_v2_forward: <= 2e-6 * (1 + |ref|) (measured 7.5e-7)."""
    from oracle import dcn as odcn
    ts, go, args = R.make_case(*spec)
    with torch.no_grad():
        got = R.dcn_ref(*ts, *args)
    ref = odcn.dcn_v2_forward(*ts, *args)
    err = float(((got - ref).abs() / (1 + ref.abs())).max())
    print("yardstick forward vs oracle %s: %.2e" % (spec, err))
    assert err <= 2e-6


def test_yardstick_float32_gradients_agree_with_float64():
    """Room the 2e-4 bound of the GPU tests leaves: the restatement's own float32 gradients against its float64 ones (measured
    5.2e-5 at worst, grad_weight of the largest shape)."""
    worst = 0.0
    for spec in R.PIN_CASES[:4]:
        ts, go, args = R.make_case(*spec)
        _, g32 = R.ref_grads(ts, go, args, torch.float32)
        _, g64 = R.ref_grads(ts, go, args, torch.float64)
        for a, b in zip(g32, g64):
            worst = max(worst, float(((a.double() - b).abs() / (1 + b.abs())).max()))
    print("yardstick fp32 vs fp64 gradients: %.2e" % worst)
    assert worst <= 2e-4


def test_yardstick_passes_gradcheck():
    """torch.autograd.gradcheck in float64 on a tiny case; the sampling coordinates are kept 0.1 away from integers (the
    derivative jumps there) and in float64 (gradcheck's perturbations are below float32 resolution)."""
    g = torch.Generator().manual_seed(5)
    n, c, co, h, w, k, G = 1, 4, 3, 5, 6, 3, 2
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    frac = 0.1 + 0.8 * torch.rand(n, G * 2 * k * k, h, w, generator=g, dtype=torch.float64)
    off = torch.randint(-3, 3, (n, G * 2 * k * k, h, w), generator=g).double() + frac
    m = torch.sigmoid(torch.randn(n, G * k * k, h, w, generator=g, dtype=torch.float64))
    wt = torch.randn(co, c, k, k, generator=g, dtype=torch.float64) / 6.0
    b = torch.randn(co, generator=g, dtype=torch.float64)
    ts = [t.requires_grad_(True) for t in (x, off, m, wt, b)]
    assert torch.autograd.gradcheck(lambda *a: R.dcn_ref(*a, 1, 1, 1, G, coord32=False), ts, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_cpu_tensors_are_refused_with_and_without_grad():
    from m3dssd_amd.host import ops
    from m3dssd_amd.host.dcn import DCNv2, DCNv2Function
    x = torch.zeros(1, 4, 4, 4, requires_grad=True)
    off, m = torch.zeros(1, 18, 4, 4, requires_grad=True), torch.zeros(1, 9, 4, 4, requires_grad=True)
    w, b = torch.zeros(4, 4, 3, 3, requires_grad=True), torch.zeros(4, requires_grad=True)
    with pytest.raises(NotImplementedError):
        DCNv2Function(1, 1)(x, off, m, w, b)
    with pytest.raises(NotImplementedError):
        DCNv2(4, 4, 3, 1, 1)(x, off, m)
    with pytest.raises(NotImplementedError):
        ops.dcn_v2(x, off, m, w, b, 1, 1)
    with pytest.raises(NotImplementedError):
        ops.dcn_v2_backward(x.detach(), off.detach(), m.detach(), w.detach(), torch.zeros(1, 4, 4, 4), 1, 1)
