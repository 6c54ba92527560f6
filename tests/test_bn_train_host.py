"""Host-side checks of the fused BatchNorm + residual + activation training operator: the guarantee of the case builder
(tests/bn_train_ref.py), the C ABI declarations, ``train.set_fused_batchnorm`` on a CPU-built net and the host-tensor refusal of
``ops.bn_act_train``.  No GPU."""
import re

import pytest
import torch
from torch import nn

from m3dssd_amd import _hip, synth
from m3dssd_amd.host import ops, train
from m3dssd_amd.host.dla import BasicBlock, Root

import bn_train_ref as R

FUNCTIONS = ("m3d_bn_act_train_workspace_bytes", "m3d_bn_act_train_chunks", "m3d_bn_act_train_forward", "m3d_bn_act_train_backward")


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.IDS)
def test_builder_keeps_pre_activations_away_from_zero(i):
    B, C, H, W, has_res, slope = R.CASES[i]
    c = R.make_case(i)
    assert c.shape == (B, C, H, W) and (c.residual is not None) == has_res and c.slope == slope
    assert all(t.dtype == torch.float32 and not t.is_cuda for t in (c.x, c.gamma, c.beta, c.running_mean, c.running_var, c.grad_y))
    if C > 1:
        assert (c.gamma > 0).any() and (c.gamma < 0).any()
    z64 = R.pre_activation(c.x, c.residual, c.gamma, c.beta)
    z32 = R.pre_activation(c.x, c.residual, c.gamma, c.beta, torch.float32)
    print("case", i, R.CASES[i], "passes", c.passes, "min|z64| %.3e" % z64.abs().min().item())
    if slope < 1.0:
        assert z64.abs().min().item() >= R.Z_MIN
        assert torch.equal(z32 > 0, z64 > 0), "the float32 composition has another sign pattern than the float64 one"
    # the references leave the cached case as it is
    before = [t.clone() for t in (c.x, c.gamma, c.beta, c.running_mean, c.running_var)]
    ref = R.ref_grads(c, torch.float64, "cpu")
    assert all(torch.equal(a, b) and not b.requires_grad for a, b in zip(before, (c.x, c.gamma, c.beta, c.running_mean, c.running_var)))
    assert (ref["grad_residual"] is not None) == has_res
    assert not torch.equal(ref["running_mean"].float(), c.running_mean) and not torch.equal(ref["running_var"].float(), c.running_var)


def test_case_5_has_several_chunks_and_a_ragged_last_one():
    B, C, H, W = R.make_case(5).shape
    assert B * H * W > 4096 and (B * H * W) % 4096 != 0          # (the chunk of csrc/bn_train.hip; the GPU test asks the library)


def test_header_declares_the_entry_points():
    with open(_hip.HEADER) as f:
        text = f.read()
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _hip.SIGNATURES, name
        assert re.search(r"added under 5:.*\b%s\b" % name, text, flags=re.S), name + " is not in the list of additive names"
    assert _hip.CONSTANTS["M3D_ABI_VERSION"] == 5
    res, args = _hip.SIGNATURES["m3d_bn_act_train_forward"]
    assert res is _hip.c_int and len(args) == 19
    res, args = _hip.SIGNATURES["m3d_bn_act_train_backward"]
    assert res is _hip.c_int and len(args) == 18
    assert _hip.SIGNATURES["m3d_bn_act_train_workspace_bytes"] == (_hip.c_ll, [_hip.c_int] * 4)
    assert _hip.SIGNATURES["m3d_bn_act_train_chunks"] == (_hip.c_int, [_hip.c_int] * 4)


def _cpu_net():
    from model.M3d_inference_align import build
    flags = synth.config_flags("anab_fullalign")
    conf = synth.synth_conf((64, 128), 0, batch_size=2, device="cpu", **flags)
    return build(conf, "train")


def test_set_fused_batchnorm_on_a_cpu_built_net():
    net = _cpu_net()
    bns = [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
    keys = list(net.state_dict().keys())
    assert len(bns) > 50
    assert not any(getattr(m, "fused_train", False) for m in bns), "the flag must default to off"
    assert train.set_fused_batchnorm(net) == len(bns)
    assert all(m.fused_train is True for m in bns)
    assert list(net.state_dict().keys()) == keys
    assert train.set_fused_batchnorm(net, False) == len(bns)
    assert not any(m.fused_train for m in bns)
    assert list(net.state_dict().keys()) == keys


def test_flagged_sites_keep_their_torch_layers_on_host_tensors():
    """A host tensor never reaches the operator: the flagged modules compute what the unflagged ones do, bit for bit."""
    torch.manual_seed(3)
    block, root = BasicBlock(8, 8).train(), Root(16, 8, 1, True).train()
    head = nn.Sequential(nn.Conv2d(8, 8, 1), nn.BatchNorm2d(8), nn.LeakyReLU(inplace=True), nn.Conv2d(8, 4, 1)).train()
    x = torch.randn(2, 8, 5, 7)

    def run():
        torch.manual_seed(4)
        for m in list(block.modules()) + list(root.modules()) + list(head.modules()):
            if isinstance(m, nn.BatchNorm2d):
                m.reset_running_stats()
        a = block(x)
        return a, root(a, x), train.seq_forward(head, a)

    plain = run()
    assert torch.equal(plain[2], head(plain[0]))
    n = sum(train.set_fused_batchnorm(m) for m in (block, root, head))
    assert n == 4
    for a, b in zip(plain, run()):
        assert torch.equal(a, b)
    assert int(block.bn1.num_batches_tracked) == 1


def test_bn_act_train_refuses_host_tensors():
    c = R.make_case(2)
    with pytest.raises(NotImplementedError):
        ops.bn_act_train(c.x, c.residual, c.gamma, c.beta, c.running_mean.clone(), c.running_var.clone(), R.MOMENTUM, R.EPS, c.slope)
    with pytest.raises(NotImplementedError):
        ops.bn_act_train_forward(c.x, None, c.gamma, c.beta, None, None, R.MOMENTUM, R.EPS, c.slope)
