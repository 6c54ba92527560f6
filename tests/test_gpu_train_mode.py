"""GPU tests (-m gpu) of training mode: RPN.forward with grad enabled (the differentiable forward of m3dssd_amd/host/train.py)
against the engine, the wiring of the gradients, whole-network gradients against the float32 torch compositions of
tests/anab_train_ref.py in place of the two HIP operators, and one full iteration net(x) -> RPN_3D_loss -> backward -> SGD step ->
eval.  128x320 frames unless stated."""
import pytest
import torch
from torch import nn

from gpu_common import _dev, _log, _relerr
from m3dssd_amd import synth
from m3dssd_amd.host import ops, train
from m3dssd_amd.host.dla import Tree

import anab_train_ref as R
import rpn_loss_ref as RR

pytestmark = pytest.mark.gpu


def _build(config, back_bone, crop, B, phase="train", conf=None):
    from model.M3d_inference_align import build
    flags = synth.config_flags(config)
    if conf is None:
        conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0", back_bone=back_bone, **flags)
    net = build(conf, phase)
    net.load_state_dict(synth.synth_state_dict(0, back_bone=back_bone, **flags), strict=True)
    return net.to(_dev()), conf


class _Top1:
    """Records the top-1 anchor indices of every align stage of a train-mode forward (a forward pre-hook on the align modules:
    the indices are recomputed from the probabilities the stage was handed, by the kernel the stage uses)."""

    def __init__(self, net):
        self.ind, self.handles = [], []
        for name in ("shape_align", "center_align2d", "center_align3d"):
            m = getattr(net, name, None)
            if m is not None:
                self.handles.append(m.register_forward_pre_hook(lambda mod, args: self.ind.append(train._top1(args[-1].detach())[0])))

    def close(self):
        for h in self.handles:
            h.remove()


# ------------------------------------------------------------------------------------ 6. the train-mode forward equals the engine
@pytest.mark.parametrize("config,back_bone", [("anab_fullalign", "dla34"), ("base", "dla34"), ("anab_fullalign", "dla102")])
def test_train_forward_equals_the_engine(config, back_bone):
    crop, B = (128, 320), 2
    net, conf = _build(config, back_bone, crop, B)
    x = synth.synth_frames(B, crop, 1234).to(_dev())
    net.eval()
    with torch.no_grad():
        ref = [t.clone() for t in net(x)]
    sel = net.engine().plan_for(B, *crop).named.get("sel_idx")
    net.train()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eval()
    rec = _Top1(net)
    out = net(x)
    rec.close()
    assert len(out) == 5 and out[0].grad_fn is not None
    # precondition: both runs chose the same anchors
    for ind in rec.ind:
        n_diff = (ind.reshape(-1) != sel.reshape(-1).long()).sum().item()
        assert n_diff == 0, "top-1 anchors differ at %d pixels: choose another seed" % n_diff
    cls, prob, b2, b3, fs = (t.detach().cpu() for t in out)
    o_cls, o_prob, o_b2, o_b3, o_fs = (t.cpu() for t in ref[:5])
    rep = dict(cls_rel=_relerr(cls, o_cls), prob=(prob - o_prob).abs().max().item(), bbox_2d=(b2 - o_b2).abs().max().item(),
               bbox_3d=(b3 - o_b3).abs().max().item())
    print("train forward vs engine", config, back_bone, rep)
    _log("train_forward_vs_engine", dict(config=config, back_bone=back_bone, **rep))
    assert rep["cls_rel"] < 1e-3 and rep["prob"] < 1e-4 and rep["bbox_2d"] < 1e-3 and rep["bbox_3d"] < 1e-3, rep
    assert torch.equal(fs, o_fs)


# ------------------------------------------------------------------------------------ 7. wiring
def _weighted_sum(out, seed):
    g = torch.Generator().manual_seed(seed)
    return sum((t * torch.randn(t.shape, generator=g).to(t.device)).sum() for t in out[:4])


def test_every_parameter_gets_a_gradient_and_the_detach_points_hold():
    crop, B = (128, 320), 2
    net, conf = _build("anab_fullalign", "dla34", crop, B)
    x = synth.synth_frames(B, crop, 1234).to(_dev())
    _weighted_sum(net(x), 5).backward()
    # the reference computes these and drops them: the unused projection of shape_align, and the projection of a Tree of more than
    # one level (its tree1 is a Tree and computes its own residual)
    dropped = {"shape_align.proj.weight"}
    for name, m in net.named_modules():
        if isinstance(m, Tree) and m.levels > 1 and m.project is not None:
            dropped |= {"%s.project.%s" % (name, k) for k, _ in m.project.named_parameters()}
    assert len(dropped) > 1
    for name, p in net.named_parameters():
        if name in dropped:
            assert p.grad is None, name
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
    # a loss on bbox_w alone (the head's own output, taken by a forward hook: a slice of the concatenated bbox_2d would hand the
    # other heads zeros, not None).  bbox_w reads feats_align2d, whose offsets come from bbox_x.detach() / bbox_y.detach(): nothing
    # reaches those two heads.
    net.zero_grad(set_to_none=True)
    taken = []
    h = net.bbox_w.register_forward_hook(lambda mod, args, out: taken.append(out))
    net(x)
    h.remove()
    taken[0].sum().backward()
    assert all(p.grad is None for p in net.bbox_x.parameters()) and all(p.grad is None for p in net.bbox_y.parameters())
    assert all(p.grad is not None and p.grad.any() for p in net.bbox_w.parameters())
    assert all(p.grad is not None and p.grad.any() for p in net.center_align2d.parameters())
    assert all(p.grad is None for p in net.cls.parameters()) and all(p.grad is None for p in net.center_align3d.parameters())


# ------------------------------------------------------------------------------------ 8. whole-network gradients
# Every parameter gradient with the HIP operators against the same module with ops.dcn_v2 / ops.anab_attention swapped for the
# float32 torch compositions of tests/anab_train_ref.py (64x128, B = 2, anab_fullalign, DLA-34, BatchNorm with batch
# statistics); per tensor max|diff| / max|ref|.
#
# Two things make the figure a property of the gradients under test and of nothing else:
#   * torch.use_deterministic_algorithms for the length of the test.  Without it two passes of the same code differ (the first
#     difference is 1e-7 in a convolution of the backbone), with it they are bit-identical.
#   * the swapped operators return the VALUE of the HIP forward and take their GRADIENT from autograd through the composition
#     (_value_of_hip_gradient_of).  The two forwards differ by 1e-6, which is what tests 1, 4, 5 and 6 bound; here it would put a
#     handful of the 10^5 LeakyReLU inputs of a head on the other side of zero, and one such flip changes a row of a weight
#     gradient by several per cent of its maximum -- a discontinuity of the network, not an error of a gradient.  With equal
#     forwards both runs differentiate the same piecewise-linear function at the same point.
# Largest per-tensor figures measured on the MI355X (GRAD_MEASURED, by parameter); the bound is 4 x the largest, the convention of
# tests/test_gpu_bf16.py.  A bound above 1e-2 would mean a wiring error, not rounding.
GRAD_MEASURED = {"center_align3d.align.bias": 6.19e-6, "base.base.base_layer.1.bias": 2.47e-6, "base.base.level2.tree2.bn2.bias": 2.18e-6,
                 "base.base.level2.tree1.bn1.weight": 2.12e-6, "base.base.level3.tree2.tree1.bn1.weight": 1.85e-6,
                 "base.base.base_layer.0.weight": 1.79e-6, "base.base.level0.0.weight": 1.76e-6,
                 "base.base.level2.project.0.weight": 1.76e-6}          # the eight largest of 319 tensors; median 2.7e-7
GRAD_BOUND = 4 * max(GRAD_MEASURED.values())                             # 2.5e-5


def _value_of_hip_gradient_of(hip_forward, composition):
    class Swapped(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *ts):
            ctx.save_for_backward(*ts)
            return hip_forward(*ts)

        @staticmethod
        def backward(ctx, go):
            ts = [t.detach().requires_grad_(True) for t in ctx.saved_tensors]
            with torch.enable_grad():
                out = composition(*ts)
            return torch.autograd.grad(out, ts, go)

    return Swapped.apply


def _torch_anab(q, k, v, gates, B, H, W):
    return _value_of_hip_gradient_of(lambda *ts: ops.anab_attention_forward(*ts, B, H, W),
                                     lambda *ts: R.anab_core(*ts, B, H, W))(q, k, v, gates)


def _torch_dcn(inp, offset, mask, weight, bias, stride, padding, dilation=1, deformable_groups=1):
    conf = (stride, padding, dilation, deformable_groups)
    return _value_of_hip_gradient_of(lambda *ts: ops.dcn_v2_forward(*ts, *conf), lambda *ts: R.dcn_ref(*ts, *conf))(
        inp, offset, mask, weight, bias)


def _biases_in_front_of_batchnorm(net):
    """Their gradient is exactly zero (the mean subtraction removes a constant), and so is that of center_align2d's bias, whose
    output feeds 1x1 convolutions in front of a BatchNorm only."""
    from m3dssd_amd.host.dla import BasicBlock, DeformConv
    names = {"center_align2d.align.bias"}
    for name, m in net.named_modules():
        if isinstance(m, BasicBlock):
            names |= {name + ".conv1.bias", name + ".conv2.bias"}
        elif isinstance(m, DeformConv):
            names.add(name + ".conv.bias")
        elif isinstance(m, nn.Sequential) and len(m) == 7 and isinstance(m[1], nn.BatchNorm2d):      # a head: conv BN act conv BN act conv
            names |= {name + ".0.bias", name + ".3.bias"}
    return names


@pytest.fixture
def deterministic_torch():
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
              torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.use_deterministic_algorithms(before[0], warn_only=before[1])
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before[2], before[3]


def test_whole_network_gradients(monkeypatch, deterministic_torch):
    crop, B = (64, 128), 2
    net, conf = _build("anab_fullalign", "dla34", crop, B)
    x = synth.synth_frames(B, crop, 77).to(_dev())

    def run():
        net.zero_grad(set_to_none=True)
        rec = _Top1(net)
        out = net(x)
        _weighted_sum(out, 9).backward()
        rec.close()
        return {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, rec.ind, [t.detach() for t in out[:4]]

    got, ind_a, out_a = run()
    monkeypatch.setattr(ops, "dcn_v2", _torch_dcn)
    monkeypatch.setattr(ops, "anab_attention", _torch_anab)
    ref, ind_b, out_b = run()
    monkeypatch.undo()
    assert len(ind_a) == 3 and all(torch.equal(a, b) for a, b in zip(ind_a, ind_b)), "top-1 anchors differ: choose another seed"
    assert all(torch.equal(a, b) for a, b in zip(out_a, out_b)), "the two forwards are not the same function value"
    assert got.keys() == ref.keys()
    # A bias whose gradient is exactly zero holds the rounding residue of sum(dy) - sum(dy) in either run: its own maximum is
    # no scale.  Those tensors are measured on the scale of their layer's weight gradient; every other tensor on its own.
    zero = _biases_in_front_of_batchnorm(net)
    assert all(n in got for n in zero)

    def scale(n):
        return ref[n[:-len("bias")] + "weight" if n in zero else n].abs().max().clamp_min(1e-30)

    errs = {n: ((got[n] - ref[n]).abs().max() / scale(n)).item() for n in got}
    order = sorted(errs.items(), key=lambda kv: -kv[1])
    fig = dict(worst=order[:8], median=order[len(order) // 2][1], tensors=len(order))
    print("whole-network gradients:", fig)
    _log("train_whole_network_gradients", fig)
    assert GRAD_BOUND <= 1e-2
    assert order[0][1] <= GRAD_BOUND, order[:8]


# ------------------------------------------------------------------------------------ 9. one iteration
def test_one_training_iteration_then_eval():
    from lib.loss.rpn_3d import RPN_3D_loss
    crop, B = (128, 320), 2
    conf = RR.loss_conf(crop, 0, device="cuda:0")
    conf.update(synth.config_flags("anab_fullalign"))
    conf.batch_size = B
    net, _ = _build("anab_fullalign", "dla34", crop, B, conf=conf)
    x = synth.synth_frames(B, crop, 1234).to(_dev())
    imobjs = RR.make_case(31, crop, B, 6)[4]
    net.eval()
    with torch.no_grad():
        before = [t.clone() for t in net(x)]
    net.train()
    with torch.no_grad(), pytest.raises(NotImplementedError):
        net(x)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9)
    crit = RPN_3D_loss(conf)
    cls, prob, b2, b3, fs = net(x)
    loss, stats = crit(cls, prob, b2, b3, imobjs, fs)
    assert torch.isfinite(loss)
    opt.zero_grad()
    loss.backward()
    opt.step()
    net.eval()
    with torch.no_grad():
        after = [t.clone() for t in net(x)]
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[3], before[3])
    fresh, _ = _build("anab_fullalign", "dla34", crop, B, phase="test", conf=conf)
    fresh.load_state_dict(net.state_dict(), strict=True)
    fresh = fresh.to(_dev()).eval()
    with torch.no_grad():
        want = fresh(x)
    for a, b in zip(after, want):
        assert torch.equal(a, b)
