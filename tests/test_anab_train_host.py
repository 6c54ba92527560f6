"""CPU checks of the train-mode pieces: the yardstick of the GPU tests (tests/anab_train_ref.py) is pinned against the forward
oracle and gradcheck, the C ABI carries the new entry points, the host operator refuses what it does not run, build(conf, 'train')
builds, and entering training mode drops the packed engine."""
import re

import pytest
import torch

from m3dssd_amd import _hip, synth
from oracle import model_cpu

import anab_train_ref as R


def _prototype_arg_count(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(_hip.HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
    assert m, "%s is not declared in include/m3dssd_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_library_and_binding_carry_the_entry_points():
    L = _hip.lib()
    for name, nargs in (("m3d_anab_attention_forward", 18), ("m3d_anab_attention_backward", 26),
                        ("m3d_anab_attention_workspace_bytes", 6)):
        assert _prototype_arg_count(name) == nargs
        assert hasattr(L, name), name
        assert name in _hip.SIGNATURES
        assert len(_hip.SIGNATURES[name][1]) == nargs
    assert L.m3d_abi_version() == 5


def test_workspace_rule_follows_the_support_set():
    f = _hip.lib().m3d_anab_attention_workspace_bytes
    for ck, cv in ((64, 128), (128, 128), (168, 128), (168, 256)):
        for h, w in ((8, 16), (16, 40), (48, 160), (5, 128), (1, 128)):
            fwd, bwd = f(2, h, w, ck, cv, 0), f(2, h, w, ck, cv, 1)
            assert 0 < fwd < bwd, (ck, cv, h, w, fwd, bwd)
    assert f(1, 5, 7, 168, 128, 1) == -1               # HW % 128
    assert f(1, 8, 16, 168, 64, 1) == -1               # Cv
    assert f(1, 8, 16, 64, 256, 1) == -1               # Cv = 256 is built for Ck = 168
    assert f(1, 8, 16, 160, 128, 0) == -1
    assert f(0, 8, 16, 168, 128, 0) == -1


@pytest.mark.parametrize("B,H,W", [(2, 8, 16), (1, 5, 7), (1, 32, 4), (1, 16, 8), (1, 128, 1), (2, 64, 2)])     # and the narrow maps
def test_composition_equals_the_forward_oracle(B, H, W):
    g = torch.Generator().manual_seed(3)
    C = 16
    x = torch.randn(B, C, H, W, generator=g)
    sd = {"a.query_conv.weight": torch.randn(168, C, 1, 1, generator=g) * 0.2, "a.key_conv.weight": torch.randn(168, C, 1, 1, generator=g) * 0.2,
          "a.value_conv.weight": torch.randn(C, C, 1, 1, generator=g) * 0.2, "a.spatial_conv.weight": torch.randn(4, C, 1, 1, generator=g) * 0.2}
    want = model_cpu.anab(sd, "a", x)
    got = R.anab_module(x, sd["a.query_conv.weight"], sd["a.key_conv.weight"], sd["a.value_conv.weight"], sd["a.spatial_conv.weight"])
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    got64 = R.anab_module(*(t.double() for t in (x, sd["a.query_conv.weight"], sd["a.key_conv.weight"], sd["a.value_conv.weight"],
                                                   sd["a.spatial_conv.weight"])))
    assert (got64 - want.double()).abs().max().item() <= 1e-5 * want.abs().max().item()


@pytest.mark.parametrize("B,H,W", [(1, 5, 7), (1, 8, 16), (1, 8, 2), (1, 20, 1)])
def test_gradcheck_of_the_composition(B, H, W):
    g = torch.Generator().manual_seed(7)
    n = B * H * W
    q = (torch.randn(n, 6, generator=g, dtype=torch.float64) * 0.5).requires_grad_(True)
    k = torch.randn(n, 6, generator=g, dtype=torch.float64).requires_grad_(True)
    v = torch.randn(n, 5, generator=g, dtype=torch.float64).requires_grad_(True)
    gates = torch.sigmoid(torch.randn(n, 4, generator=g, dtype=torch.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda *a: R.anab_core(*a, B, H, W), (q, k, v, gates), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_host_operator_refusals():
    from m3dssd_amd.host import ops
    n = 128
    q, k, v, g = torch.zeros(n, 168), torch.zeros(n, 168), torch.zeros(n, 128), torch.zeros(n, 4)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ops.anab_attention(q, k, v, g, 1, 8, 16)
    with pytest.raises(NotImplementedError):
        ops.anab_attention_backward(q, k, v, g, torch.zeros(n, 128), 1, 8, 16)
    # the shape and type rules are checked in front of any launch: a "meta" tensor passes for a device tensor here
    def fake(t):
        class T(torch.Tensor):
            is_cuda = True
        return t.as_subclass(T)
    with pytest.raises(RuntimeError, match="float32"):
        ops._anab_prepare("anab_attention", fake(q.double()), fake(k), fake(v), fake(g), 1, 8, 16)
    with pytest.raises(RuntimeError, match="HW % 128"):
        ops._anab_prepare("anab_attention", *(fake(t[:35]) for t in (q, k, v, g)), 1, 5, 7)
    with pytest.raises(RuntimeError, match=r"\(Ck, Cv\)"):
        ops._anab_prepare("anab_attention", fake(q[:, :160]), fake(k[:, :160]), fake(v), fake(g), 1, 8, 16)
    with pytest.raises(RuntimeError, match=r"\(Ck, Cv\)"):
        ops._anab_prepare("anab_attention", fake(q[:, :64]), fake(k[:, :64]), fake(torch.zeros(n, 256)), fake(g), 1, 8, 16)
    assert ops._anab_prepare("anab_attention", fake(q), fake(k), fake(v), fake(g), 1, 8, 16)[:2] == (168, 128)


def test_aligned_copies_what_the_kernels_cannot_read():
    """ops._anab_aligned hands q / grad_out on as they are only where 16-byte row loads are possible AND the rows do not overlap:
    autograd's grad_out behind ``.sum(0)`` has strides (0, 1), behind ``.sum()`` (0, 0), and the C ABI refuses go_cs < Cv."""
    from m3dssd_amd.host import ops
    n, c = 640, 128
    g = torch.Generator().manual_seed(5)
    dense = torch.randn(n, c, generator=g)
    assert dense.data_ptr() % 16 == 0
    assert ops._anab_aligned(dense) is dense
    wide = torch.randn(n, c + 8, generator=g)
    assert ops._anab_aligned(wide[:, 4:4 + c]).data_ptr() == wide.data_ptr() + 16            # an aligned column slice: as it is
    row = torch.randn(c, generator=g)
    for view in (row.expand(n, c), torch.randn((), generator=g).expand(n, c), row[:1].expand(n, c), wide[:, 3:3 + c],
                 torch.randn(n, c + 2, generator=g)[:, :c], dense.t().contiguous().t()):
        got = ops._anab_aligned(view)
        assert got.stride() == (c, 1) and got.data_ptr() % 16 == 0, view.stride()
        assert torch.equal(got, view)
    x = torch.randn(n, c, generator=g, requires_grad=True)                 # the strides autograd really hands over
    seen = []
    x.register_hook(lambda t: seen.append(t.stride()))
    x.sum(0).backward(row)
    x.sum().backward()
    assert seen == [(0, 1), (0, 0)]


@pytest.mark.parametrize("config", ["anab_fullalign", "base"])
def test_build_train_on_the_cpu(config):
    from model.M3d_inference_align import build
    conf = synth.synth_conf((128, 320), 0, batch_size=2, device="cpu", **synth.config_flags(config))
    net = build(conf, "train")
    assert net.training and all(m.training for m in net.modules())
    with pytest.raises(NotImplementedError):           # no CPU path, with or without grad
        net(torch.zeros(2, 3, 128, 320))


def test_train_drops_the_packed_engine_and_eval_does_not():
    from model.M3d_inference_align import build
    conf = synth.synth_conf((128, 320), 0, batch_size=2, device="cpu")
    net = build(conf, "test")
    fake = object()
    net._engine, net._param_sig = fake, "sig"
    net.__dict__["_device_engines"] = {"cuda:1": fake}
    net.eval()
    assert net._engine is fake and "_device_engines" in net.__dict__
    net.train(False)
    assert net._engine is fake
    net.train()
    assert net._engine is None and net._param_sig is None and "_device_engines" not in net.__dict__
    net._engine = fake
    net.eval()
    assert net._engine is fake
