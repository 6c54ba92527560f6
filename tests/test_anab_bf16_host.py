"""The bf16 ANAB attention operator without a device: the exactness premise of tests/test_gpu_anab_bf16.py's exact comparison, the
declaration of the three entry points, the CPU refusal, and set_bf16_attention."""
import re

import pytest
import torch

from m3dssd_amd import _hip

import anab_bf16_cases as C
import anab_train_ref as R
import exact_inputs as X

NEW = {"m3d_anab_attention_workspace_bytes_bf16": 6, "m3d_anab_attention_forward_bf16": 18, "m3d_anab_attention_backward_bf16": 26}


@pytest.mark.parametrize("shape", C.EXACT_SHAPES, ids=["b2_cv128", "b1_cv256"])
def test_exact_operands_round_nowhere(shape):
    """The emulation with the operator's rounding points (bf16 khat / vhat / P / dS / outputs, fp32 accumulation in a scrambled
    order) changes no bit, it is the float64 composition of anab_train_ref, and the rows are what the docstring promises: one-hot
    and two-hot softmax rows with a gap of at least 1024, targets in every key tile and at all four scales."""
    B, H, W, Ck, Cv = shape
    ts, go, target = C.exact_case(B, Ck, Cv, seed=7)
    ops = {"ts": ts, "go": go, "dims": (B, H, W)}
    flat = X.assert_exact_under(C.emulate, ops, torch.bfloat16)
    ref64 = R.core_grads(ts, go, B, H, W, torch.float64, "cpu")
    for name, a, b in zip(C.NAMES, C.split(flat, Ck, Cv), ref64):
        assert torch.equal(a, b), name + ": the emulation is not the float64 composition"
    q, k, _, g = (t.double() for t in ts)
    S = R.anab_logits(q, k, g, B, H, W).reshape(B * H * W, 337)
    top = S.max(-1, keepdim=True)[0]
    hot = S == top
    two = target[:, 1] >= 0
    assert torch.equal(hot.sum(-1), 1 + two.long())
    rows = torch.arange(S.shape[0])
    assert hot[rows, target[:, 0]].all() and hot[rows[two], target[two, 1]].all()
    assert (top - S)[~hot].min().item() >= 1024.0 and top.min().item() > 1024.0
    keys = torch.cat([target[:, 0], target[two, 1]])
    assert set((keys // 32).tolist()) == set(range(11)), "a key tile of 32 has no target"
    assert {0}.issubset(keys.tolist()) and ((keys >= 1) & (keys < 17)).any() and ((keys >= 17) & (keys < 81)).any() and (keys >= 81).any()
    assert int(two.sum()) >= 32
    # the two-hot rows make grad_q, grad_k and the k-term of grad_gates non-zero; the one-hot rows leave grad_q at zero
    assert ref64[1][two].abs().sum() > 0 and ref64[2].abs().sum() > 0 and not ref64[1][~two].any()
    for t in ref64:
        assert torch.isfinite(t).all()


def test_entry_points_are_declared_additive_and_bound():
    hdr = open(_hip.HEADER).read()
    assert re.search(r"#define\s+M3D_ABI_VERSION\s+5\b", hdr)
    history = hdr[hdr.index("added under 5"):hdr.index("#define M3D_ABI_VERSION")]
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _hip.lib()
    for name, nargs in NEW.items():
        assert re.search(r"\b%s\b" % name, history), name + " is not in the additive list"
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, body)
        assert m, name + " is not declared in include/m3dssd_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_hip.SIGNATURES[name][1]), name
        assert hasattr(L, name)
    # the same argument lists as the fp32 entry points
    for name in NEW:
        assert _hip.SIGNATURES[name] == _hip.SIGNATURES[name[:-len("_bf16")]]


def test_workspace_rule_answers_without_a_gpu():
    L = _hip.lib()
    for Ck, Cv in ((64, 128), (128, 128), (168, 128), (168, 256)):
        fwd, bwd = (L.m3d_anab_attention_workspace_bytes_bf16(2, 16, 40, Ck, Cv, b) for b in (0, 1))
        assert 0 < fwd < bwd and fwd % 256 == 0 and bwd % 256 == 0
    assert L.m3d_anab_attention_workspace_bytes_bf16(1, 5, 7, 168, 128, 1) == -1          # HW % 128
    assert L.m3d_anab_attention_workspace_bytes_bf16(1, 8, 16, 160, 128, 1) == -1         # (Ck, Cv)
    assert L.m3d_anab_attention_workspace_bytes_bf16(1, 8, 16, 64, 256, 0) == -1


def test_cpu_tensors_are_refused():
    from m3dssd_amd.host import ops
    q, k, v, g = (torch.zeros(128, c, dtype=torch.bfloat16) for c in (168, 168, 128, 4))
    with pytest.raises(NotImplementedError):
        ops.anab_attention_bf16(q, k, v, g, 1, 8, 16)
    with pytest.raises(NotImplementedError):
        ops.anab_attention_forward_bf16(q, k, v, g, 1, 8, 16)


def test_set_bf16_attention_reaches_every_anab_and_nothing_else():
    from torch import nn
    from m3dssd_amd.host import train
    from m3dssd_amd.host.attention import ANAB
    assert ANAB.bf16_attention is False

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = ANAB(32, 1)
            self.seq = nn.Sequential(nn.Conv2d(3, 8, 1), ANAB(16, 1), nn.ModuleList([ANAB(8, 1)]))
            self.other = nn.Linear(4, 4)

    net = Net()
    before = {n: dict(vars(m)) for n, m in net.named_modules() if not isinstance(m, ANAB)}
    assert train.set_bf16_attention(net, True) == 3
    assert all(m.bf16_attention is True for m in net.modules() if isinstance(m, ANAB))
    for n, m in net.named_modules():
        if not isinstance(m, ANAB):
            assert not hasattr(m, "bf16_attention") and vars(m).keys() == before[n].keys(), n
    assert ANAB.bf16_attention is False and ANAB(8, 1).bf16_attention is False           # the class default stands
    assert train.set_bf16_attention(net, False) == 3
    assert not any(m.bf16_attention for m in net.modules() if isinstance(m, ANAB))
    assert train.set_bf16_attention(nn.Linear(2, 2), True) == 0
    # a built network: the one ANAB of the fullalign configuration
    from m3dssd_amd import synth
    from model.M3d_inference_align import build
    conf = synth.synth_conf((64, 128), 0, batch_size=2, device="cpu", back_bone="dla34", **synth.config_flags("anab_fullalign"))
    built = build(conf, "train")
    blocks = [m for m in built.modules() if isinstance(m, ANAB)]
    assert len(blocks) >= 1 and train.set_bf16_attention(built, True) == len(blocks)
    assert all(m.bf16_attention for m in blocks)
    assert [n for n, m in built.named_modules() if "bf16_attention" in vars(m)] == [n for n, m in built.named_modules() if isinstance(m, ANAB)]
