"""GPU tests (-m gpu) of the base / anab model configurations and of every flag combination of the reference model file
(M3d_inference_align.py:138-168,241-277): the fp32 and bf16 plans against the composed CPU oracle (tests/config_oracle.py),
the reference's own outputs (tests/golden/model_{base,anab}_128x320_b2.npz), graph replay, batch invariance, the uint8 input
path and the detection stage in all its forms.  Bounds are the fullalign ones of test_gpu_network.py / test_gpu_bf16.py."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import config_oracle
from gpu_common import GOLDEN, _dev, _log, _relerr
from m3dssd_amd import synth
from m3dssd_amd.config import model_flags

pytestmark = pytest.mark.gpu

CONFIGS = ["base", "anab"]
COMBOS = [(sa, ca, at) for sa, ca, at in itertools.product((False, True), (False, True), ("ANAB", None))]
ALIGN_KINDS = ("align", "anab_pool", "anab_attend", "softmax", "softmax_bf16", "bf16_anab", "bf16_qkvs")


def _flags(config):
    if isinstance(config, str):
        return synth.config_flags(config)
    sa, ca, at = config
    return dict(shape_align=sa, center_align=ca, attention=at)


@functools.lru_cache(maxsize=None)
def _net(config, crop, B, dtype="f32"):
    from model.M3d_inference_align import build
    flags = _flags(config)
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0", **flags)
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, **flags), strict=True)
    net.set_compute_dtype(dtype)
    return net.to(_dev()), conf


def _forward(net, x):
    with torch.no_grad():
        return [t.clone() for t in net(x.to(_dev()))]


def _oracle(config, crop, B, x, plan=None):
    """Composed oracle; with `plan` the engine's top-1 anchor / hard-mask decisions are injected into its align stages."""
    flags = _flags(config)
    cconf = synth.synth_conf(crop, 0, batch_size=B, device="cpu", **flags)
    sd = synth.synth_state_dict(0, **flags)
    inject = None
    if plan is not None:
        fh, fw = crop[0] // 8, crop[1] // 8
        ind = plan.named["sel_idx"].view(B, 1, fh, fw).long().cpu()
        hard = (plan.named["sel_prob"].view(B, 1, fh, fw).cpu() > 0.5).float()
        inject = {"sel": {"ind": ind, "hard": hard}}
    taps = {}
    with torch.no_grad():
        out = config_oracle.rpn_forward(sd, cconf, x, taps, inject)
    return out, taps


def _assert_matches_oracle(out, ref):
    """The fullalign bounds (test_gpu_network.py::test_forward_matches_oracle)."""
    cls, prob, b2, b3, fs, rois = (t.cpu() for t in out)
    o_cls, o_prob, o_b2, o_b3, o_fs, o_rois = ref
    assert _relerr(cls, o_cls) < 1e-3
    assert (prob - o_prob).abs().max().item() < 1e-4
    assert (b2 - o_b2).abs().max().item() < 1e-3
    assert (b3 - o_b3).abs().max().item() < 1e-3
    assert torch.equal(rois, o_rois) and torch.equal(fs, o_fs)
    return dict(cls_rel=_relerr(cls, o_cls), prob=(prob - o_prob).abs().max().item(), bbox_2d=(b2 - o_b2).abs().max().item(),
                bbox_3d=(b3 - o_b3).abs().max().item())


# ------------------------------------------------------------------------------------ fp32 forward
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "sa%d-ca%d-%s" % c)
def test_fp32_every_flag_combination_matches_composed_oracle(combo):
    crop, B = (128, 320), 2
    net, conf = _net(combo, crop, B)
    x = synth.synth_frames(B, crop, 1234)
    out = _forward(net, x)
    plan = net.engine().plan_for(B, *crop)
    with_shape, with_center, with_anab = model_flags(conf)
    if with_shape or with_center:
        # the engine's decisions against the free-running oracle's: they may differ at exact near-ties only
        (_, _, _, _, _, _), free_taps = _oracle(combo, crop, B, x)
        fh, fw = crop[0] // 8, crop[1] // 8
        ind = plan.named["sel_idx"].view(B, 1, fh, fw).long().cpu()
        prob_sel = plan.named["sel_prob"].view(B, 1, fh, fw).cpu()
        o_mask, o_ind = free_taps["fg_prob"].max(dim=1, keepdim=True)
        assert (prob_sel - torch.gather(free_taps["fg_prob"], 1, ind)).abs().max().item() < 1e-4
        near = (o_mask - torch.gather(free_taps["fg_prob"], 1, ind)).abs() < 1e-4
        assert near[o_ind != ind].all()
    ref, taps = _oracle(combo, crop, B, x, plan)
    rep = _assert_matches_oracle(out, ref)
    for name in ("feats0", "feats", "feats_align2d", "feats_align3d", "feats_gl"):
        assert _relerr(plan.named[name].torch_nchw().cpu(), taps[name]) < 2e-3, name
    # an absent stage publishes the map that stands in for it under the reference's name
    n = plan.named
    assert (n["feats"] is n["feats0"]) == (not with_shape)
    assert (n["feats_align3d"] is n["feats"]) == (not with_center)
    assert (n["feats_gl"] is n["feats_align3d"]) == (not with_anab)
    kinds = {op[1] for op in plan.ops}
    assert ("align" in kinds) == (with_shape or with_center)
    assert any(k.startswith("anab") for k in kinds) == with_anab
    _log("configs_fp32_oracle", dict(combo=list(combo), **rep))


@pytest.mark.parametrize("config", CONFIGS)
def test_fp32_matches_reference_golden(config):
    g = np.load(os.path.join(GOLDEN, "model_%s_128x320_b2.npz" % config))
    crop, B = (128, 320), 2
    net, conf = _net(config, crop, B)
    out = [t.cpu() for t in _forward(net, synth.synth_frames(B, crop, 1234))]
    rs = int(g["row_stride"])
    cls, prob, b2, b3, fs, rois = out
    assert _relerr(cls[:, ::rs], g["cls"]) < 1e-3
    assert np.abs(prob[:, ::rs].numpy() - g["prob"]).max() < 1e-4
    assert np.abs(b2[:, ::rs].numpy() - g["bbox_2d"]).max() < 1e-3
    assert np.abs(b3[:, ::rs].numpy() - g["bbox_3d"]).max() < 1e-3
    assert np.array_equal(fs.numpy(), g["feat_size"])
    for name, t in (("cls", cls), ("prob", prob), ("bbox_2d", b2), ("bbox_3d", b3)):
        chk = g["chk." + name]
        assert abs(t.double().abs().sum().item() - chk[1]) <= 1e-4 * chk[1], name
    plan = net.engine().plan_for(B, *crop)
    for key in g.files:
        if key.startswith("tap."):
            got = plan.named[key[4:]].torch_nchw().cpu()[:, ::8].numpy()
            assert _relerr(got, g[key]) < 2e-3, key


@pytest.mark.parametrize("config", CONFIGS)
def test_fp32_full_size_matches_composed_oracle(config):
    crop, B = (384, 1280), 1
    net, conf = _net(config, crop, B)
    x = synth.synth_frames(B, crop, 1234, pad_right_third=True)
    out = _forward(net, x)
    ref, _ = _oracle(config, crop, B, x)
    rep = _assert_matches_oracle(out, ref)
    _log("configs_fp32_full_size", dict(config=config, **rep))


@pytest.mark.parametrize("config", CONFIGS)
def test_plan_has_only_the_configured_stages(config):
    """base: no align / ANAB launch, the 11 box heads in one launch; anab: ANAB on feats0, the z3d head behind it.  Both dtypes."""
    crop, B = (128, 320), 2
    for dtype in ("f32", "bf16"):
        net, conf = _net(config, crop, B, dtype)
        _forward(net, synth.synth_frames(B, crop, 1234))
        plan = net.engine().plan_for(B, *crop)
        names = [op[0] for op in plan.ops]
        kinds = [op[1] for op in plan.ops]
        assert not any("align" in nm for nm in names), (dtype, names)
        assert "align" not in kinds and not any(k.startswith("dcn") and "align" in nm for k, nm in zip(kinds, names))
        box = [nm for nm in names if nm.startswith("bbox_")]
        if config == "base":
            assert not any(nm.startswith("anab") for nm in names) and not set(kinds) & set(ALIGN_KINDS), (dtype, kinds)
            assert box == ["+".join(net.engine().box_heads) + ".mlp"], (dtype, box)
            assert not plan.branches
        else:
            assert any(nm.startswith("anab") for nm in names)
            assert "bbox_z3d.mlp" in box and len(box) == (2 if dtype == "f32" else 3), (dtype, box)
            if dtype == "bf16":
                # ANAB reads feats0: the side branch starts where it is ready, the z3d head is its last launch
                b0, b1, join = plan.branches[0]
                assert b0 == plan.named["planar_first_op"] and names[b1 - 1] == "bbox_z3d.mlp" and join == len(names) - 1
        # the detection stage's ordering contract (PipelinedDetector._check_no_write_beside_detect)
        first = plan.named["planar_first_op"]
        assert plan.named["score_bits_first_write_op"] >= first and names[-1] == "bundle_outputs"


# ------------------------------------------------------------------------------------ replay, batch, input path
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("config", CONFIGS)
def test_graph_replay_matches_eager(config, dtype):
    from lib.rpn_util import detect_batch
    crop, B = (128, 320), 2
    net, conf = _net(config, crop, B, dtype)
    dev = _dev()
    x = synth.synth_frames(B, crop, 3).to(dev)
    with torch.no_grad():
        eager = [t.clone() for t in net(x)[:4]]
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        detect_batch(net, x, conf)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            gd, gc = detect_batch(net, x, conf)
    torch.cuda.current_stream().wait_stream(s)
    x2 = synth.synth_frames(B, crop, 4).to(dev)
    e1, n1 = detect_batch(net, x2, conf)
    e1, n1 = e1.clone(), n1.clone()
    with torch.no_grad():
        eager2 = [t.clone() for t in net(x2)[:4]]
    x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gd, e1) and torch.equal(gc, n1)
    with torch.no_grad():
        again = [t.clone() for t in net(x)[:4]]
    for u, v in zip(again, eager2):
        assert torch.equal(u, v)
    assert not torch.equal(eager[3], eager2[3])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("config", CONFIGS)
def test_batch_invariance_and_uint8_frames(config, dtype):
    from m3dssd_amd.host.preprocess import preprocess
    crop = (128, 320)
    net2, conf = _net(config, crop, 2, dtype)
    net1, _ = _net(config, crop, 1, dtype)
    x = synth.synth_frames(2, crop, 77)
    both = _forward(net2, x)
    for i in range(2):
        single = _forward(net1, x[i:i + 1])
        for u, s in zip(both[:4], single[:4]):
            if dtype == "bf16":           # the bf16 kernels are batch-invariant by construction (test_gpu_bf16.py)
                assert torch.equal(u[i:i + 1], s)
            else:                         # the fp32 bound of test_gpu_network.py::test_batch_invariance_and_determinism
                assert (u[i:i + 1] - s).abs().max().item() < 1e-4
    rng = np.random.RandomState(5)
    frames = torch.from_numpy(rng.randint(0, 256, size=(2, 120, 310, 3)).astype(np.uint8)).to(_dev())
    a = _forward(net2, frames)
    b = _forward(net2, preprocess(frames, conf.crop_size, conf.image_means, conf.image_stds))
    for u, v in zip(a[:4], b[:4]):
        assert torch.equal(u, v)


def test_data_parallel_wrapper_and_engine_refresh():
    from torch import nn
    crop, B = (128, 320), 2
    net, conf = _net("anab", crop, B)
    x = synth.synth_frames(B, crop, 1234)
    ref = _forward(net, x)
    dp = nn.DataParallel(net, device_ids=[0])
    with torch.no_grad():
        got = [t.clone() for t in dp(x.to(_dev()))]
    for u, v in zip(got[:4], ref[:4]):
        assert torch.equal(u, v)
    net.refresh_engine()
    for u, v in zip(_forward(net, x)[:4], ref[:4]):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------ detection
@pytest.mark.parametrize("config", CONFIGS)
def test_detection_matches_reference_rows(config):
    """im_detect_3d / detect_batch on the HIP path against the rows the reference's im_detect_3d produced for image 0
    (tools/gen_golden_configs.py): kept anchors / classes identical, every column within 2e-3 * (1 + |ref|)."""
    from lib.rpn_util import detect_batch, im_detect_3d
    crop, B = (128, 320), 2
    net, conf = _net(config, crop, B)
    x = synth.synth_frames(B, crop, 1234)
    ref = np.load(os.path.join(GOLDEN, "model_%s_128x320_b2.npz" % config))["aboxes"]
    ab = im_detect_3d(x[0], net, conf)
    assert ab.shape == ref.shape
    assert np.array_equal(ab[:, 13], ref[:, 13]) and np.array_equal(ab[:, 5], ref[:, 5])
    err = np.abs(ab - ref) / (1.0 + np.abs(ref))
    assert err.max() < 2e-3
    dets, counts = detect_batch(net, x.to(_dev()), conf)
    k = int(counts[0])
    assert k == min(len(ref), conf.nms_topN_post)
    d0 = dets[0, :k].cpu().numpy()
    assert np.array_equal(d0[:, 13], ref[:k, 13]) and (np.abs(d0 - ref[:k]) <= 2e-3 * (1.0 + np.abs(ref[:k]))).all()
    _log("configs_detect_golden", dict(config=config, max_rel=float(err.max()), rows=int(ref.shape[0])))


@pytest.mark.parametrize("planar", [True, False])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("config", CONFIGS)
def test_pipelined_detector_equals_detect_batch(config, dtype, planar):
    from lib.rpn_util import detect_batch
    from m3dssd_amd.pipeline import PipelinedDetector
    dev = _dev()
    net, conf = _net(config, (128, 320), 2, dtype)
    xs = [synth.synth_frames(2, (128, 320), 40 + i).to(dev) for i in range(4)]
    ref = []
    for x in xs:
        d, c = detect_batch(net, x, conf)
        ref.append((d.clone(), c.clone()))
    pipe = PipelinedDetector(net, conf, 2, 128, 320, planar=planar)
    got = []
    for x in xs:
        r = pipe.step(x)
        if r is not None:
            got.append((r[0].clone(), r[1].clone()))
    r = pipe.flush()
    got.append((r[0].clone(), r[1].clone()))
    assert len(got) == len(ref)
    for (gd, gc), (rd, rc) in zip(got, ref):
        assert torch.equal(gc, rc) and torch.equal(gd, rd)


# ------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize("config", CONFIGS)
def test_bf16_matches_fp32_engine_within_fullalign_bounds(config):
    """bf16 plan vs the fp32 plan of the same configuration, per output column (max, p99.9, rms) within the fullalign bounds of
    test_gpu_bf16.py (1.3 x measured).  Neither configuration has a discrete decision inside the network: no injection."""
    from test_gpu_bf16 import BF16_COLS, BF16_GUARD, BF16_MEASURED, BF16_PROB_MEASURED
    crop, B = (128, 320), 2
    x = synth.synth_frames(B, crop, 1234)
    n32, _ = _net(config, crop, B, "f32")
    n16, _ = _net(config, crop, B, "bf16")
    a = [t.cpu() for t in _forward(n32, x)]
    b = [t.cpu() for t in _forward(n16, x)]
    assert type(n16.engine()).__name__ == "EngineBF16"
    assert torch.isfinite(b[3]).all() and torch.isfinite(b[0]).all()
    rep = {"config": config, "prob": (a[1] - b[1]).abs().max().item()}
    for nm, j in (("bbox_2d", 2), ("bbox_3d", 3)):
        e = (a[j] - b[j]).abs().view(-1, a[j].shape[-1])
        rep[nm + "_cols"] = {c: [e[:, k].max().item(), torch.quantile(e[:, k].float(), 0.999).item(),
                                 e[:, k].pow(2).mean().sqrt().item()] for k, c in enumerate(BF16_COLS[nm])}
    _log("configs_bf16_vs_fp32", rep)
    assert rep["prob"] <= BF16_GUARD * BF16_PROB_MEASURED + 0.01, rep
    for nm, cols in BF16_COLS.items():
        for c in cols:
            mx, p999, rms = rep[nm + "_cols"][c]
            tmx, tp, tr = (BF16_GUARD * v for v in BF16_MEASURED[nm][c])
            assert mx <= tmx and p999 <= tp and rms <= tr, (nm, c, (mx, p999, rms), (tmx, tp, tr))
