"""GPU tests (-m gpu) of the DLA-102 backbone (the reference's shipped configurations, scripts/config/kitti_3d_*.py) on the fp32
plan: every flag combination stage by stage against the composed CPU oracle (tests/dla102_oracle.py), the reference's own outputs
and detections (tests/golden/model_dla102_*_128x320_b2.npz), a full-size forward, graph replay, batch invariance, the pipelined
detector, and the two kernel forms DLA-102 adds (the three-layer head with Cin = 256, the attention with Cv = 256) through the
C ABI against torch in float64.  Bounds are the ones of tests/test_gpu_configs.py."""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dla102_oracle
from gpu_common import GOLDEN, _dev, _log, _relerr
from m3dssd_amd import _hip, synth
from m3dssd_amd.config import model_flags

pytestmark = pytest.mark.gpu

CONFIGS = ["anab_fullalign", "base"]
COMBOS = [(sa, ca, at) for sa, ca, at in itertools.product((False, True), (False, True), ("ANAB", None))]
STAGES = ("level0", "level1", "level2", "level3", "level4", "level5", "feats0", "feats", "feats_align2d", "feats_align3d",
          "feats_gl")


def _flags(config):
    if isinstance(config, str):
        return synth.config_flags(config)
    sa, ca, at = config
    return dict(shape_align=sa, center_align=ca, attention=at)


@functools.lru_cache(maxsize=None)
def _net(config, crop, B):
    from model.M3d_inference_align import build
    flags = _flags(config)
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0", back_bone="dla102", **flags)
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, back_bone="dla102", **flags), strict=True)
    return net.to(_dev()), conf


def _forward(net, x):
    with torch.no_grad():
        return [t.clone() for t in net(x.to(_dev()))]


def _oracle(config, crop, B, x, plan=None):
    """Composed oracle; with `plan` the engine's top-1 anchor / hard-mask decisions are injected into its align stages."""
    flags = _flags(config)
    cconf = synth.synth_conf(crop, 0, batch_size=B, device="cpu", back_bone="dla102", **flags)
    sd = synth.synth_state_dict(0, back_bone="dla102", **flags)
    inject = None
    if plan is not None:
        fh, fw = crop[0] // 8, crop[1] // 8
        ind = plan.named["sel_idx"].view(B, 1, fh, fw).long().cpu()
        hard = (plan.named["sel_prob"].view(B, 1, fh, fw).cpu() > 0.5).float()
        inject = {"sel": {"ind": ind, "hard": hard}}
    taps = {}
    with torch.no_grad():
        out = dla102_oracle.rpn_forward(sd, cconf, x, taps, inject)
    return out, taps


def _assert_matches_oracle(out, ref):
    cls, prob, b2, b3, fs, rois = (t.cpu() for t in out)
    o_cls, o_prob, o_b2, o_b3, o_fs, o_rois = ref
    rep = dict(cls_rel=_relerr(cls, o_cls), prob=(prob - o_prob).abs().max().item(), bbox_2d=(b2 - o_b2).abs().max().item(),
               bbox_3d=(b3 - o_b3).abs().max().item())
    assert rep["cls_rel"] < 1e-3 and rep["prob"] < 1e-4 and rep["bbox_2d"] < 1e-3 and rep["bbox_3d"] < 1e-3, rep
    assert torch.equal(rois, o_rois) and torch.equal(fs, o_fs)
    return rep


# ------------------------------------------------------------------------------------ fp32 forward
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "sa%d-ca%d-%s" % c)
def test_every_flag_combination_matches_composed_oracle_stage_by_stage(combo):
    crop, B = (128, 320), 2
    net, conf = _net(combo, crop, B)
    x = synth.synth_frames(B, crop, 1234)
    out = _forward(net, x)
    plan = net.engine().plan_for(B, *crop)
    ref, taps = _oracle(combo, crop, B, x, plan)
    rep = _assert_matches_oracle(out, ref)
    for name in STAGES:
        got = plan.named[name].torch_nchw().cpu()
        assert got.shape == taps[name].shape, name
        rep[name] = _relerr(got, taps[name])
        assert rep[name] < 2e-3, (name, rep)
    assert plan.named["feats0"].c == 256 and plan.named["level5"].c == 1024
    # the 1x1 heads run as fused three-layer launches, the attention as one launch
    kinds = [op[1] for op in plan.ops]
    heads = [(op[0], op[1]) for op in plan.ops if op[0].endswith(".mlp") and op[0] != "cls.mlp"]
    assert heads and all(k.startswith("head_mlp<3,") for _, k in heads), heads
    assert ("anab_attend" in kinds) == model_flags(conf)[2]
    _log("dla102_fp32_oracle", dict(combo=list(combo), **rep))


@pytest.mark.parametrize("config", CONFIGS)
def test_matches_reference_golden(config):
    g = np.load(os.path.join(GOLDEN, "model_dla102_%s_128x320_b2.npz" % config))
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
    ts = int(g["tap_stride"])
    for key in g.files:
        if key.startswith("tap."):
            got = plan.named[key[4:]].torch_nchw().cpu()[:, ::ts].numpy()
            assert _relerr(got, g[key]) < 2e-3, key


@pytest.mark.parametrize("config", CONFIGS)
def test_detection_matches_reference_rows(config):
    from lib.rpn_util import detect_batch, im_detect_3d
    crop, B = (128, 320), 2
    net, conf = _net(config, crop, B)
    x = synth.synth_frames(B, crop, 1234)
    ref = np.load(os.path.join(GOLDEN, "model_dla102_%s_128x320_b2.npz" % config))["aboxes"]
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
    _log("dla102_detect_golden", dict(config=config, max_rel=float(err.max()), rows=int(ref.shape[0])))


def test_full_size_matches_composed_oracle():
    crop, B = (384, 1280), 1
    net, conf = _net("anab_fullalign", crop, B)
    x = synth.synth_frames(B, crop, 1234, pad_right_third=True)
    out = _forward(net, x)
    ref, _ = _oracle("anab_fullalign", crop, B, x, net.engine().plan_for(B, *crop))
    rep = _assert_matches_oracle(out, ref)
    _log("dla102_fp32_full_size", rep)


def test_shipped_conf_with_pre_train_runs():
    """A conf with the shipped fields (back_bone = 'dla102', pre_train = True) builds with a warning, strict-loads the checkpoint
    and computes exactly what the module built from the synthetic conf computes."""
    from model.M3d_inference_align import build
    crop, B = (128, 320), 2
    ref_net, _ = _net("anab_fullalign", crop, B)
    flags = _flags("anab_fullalign")
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0", back_bone="dla102", **flags)
    conf.pre_train = True
    with pytest.warns(UserWarning, match="not downloaded"):
        net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, back_bone="dla102", **flags), strict=True)
    net = net.to(_dev())
    x = synth.synth_frames(B, crop, 1234)
    for u, v in zip(_forward(net, x)[:4], _forward(ref_net, x)[:4]):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------ replay, batch, pipeline
def test_graph_replay_matches_eager():
    from lib.rpn_util import detect_batch
    crop, B = (128, 320), 2
    net, conf = _net("anab_fullalign", crop, B)
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


def test_batch_invariance():
    crop = (128, 320)
    net2, _ = _net("anab_fullalign", crop, 2)
    net1, _ = _net("anab_fullalign", crop, 1)
    x = synth.synth_frames(2, crop, 77)
    both = _forward(net2, x)
    for i in range(2):
        single = _forward(net1, x[i:i + 1])
        for u, s in zip(both[:4], single[:4]):
            assert (u[i:i + 1] - s).abs().max().item() < 1e-4


@pytest.mark.parametrize("planar", [True, False])
def test_pipelined_detector_equals_detect_batch(planar):
    from lib.rpn_util import detect_batch
    from m3dssd_amd.pipeline import PipelinedDetector
    dev = _dev()
    net, conf = _net("anab_fullalign", (128, 320), 2)
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


# ------------------------------------------------------------------------------------ kernels through the C ABI
def _head256_case(seed, cout, cpad, dev, n=2, h=13, w=21):
    """One three-layer head 256 -> 256 -> 256 -> cout: (MlpDesc, device output, float64 reference, keep-alive list)."""
    from m3dssd_amd.engine import pack_frag
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, 256 + 8, generator=g)                  # an NHWC slice of a wider buffer
    ref = x[..., :256].permute(0, 3, 1, 2).double()
    d = _hip.MlpDesc()
    xd = x.contiguous().to(dev)
    keep = [xd]
    d.inp, d.in_cs, d.M, d.Cin = xd.data_ptr(), 256 + 8, n * h * w, 256
    chans = [256, 256, 256, cout]
    for li, slot in enumerate("123"):
        ci, co = chans[li], chans[li + 1]
        last = li == 2
        wt = torch.randn(co, ci, generator=g) / ci ** 0.5
        b = torch.randn(co, generator=g) * 0.1
        if last:
            sc, sh = torch.ones(co), b
        else:
            gam, bet = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.2
            mean, var = torch.randn(co, generator=g) * 0.2, torch.rand(co, generator=g) + 0.5
            sc = gam / torch.sqrt(var + 1e-5)
            sh = (b - mean) * sc + bet
        ref = torch.einsum("oc,nchw->nohw", wt.double(), ref) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
        if not last:
            ref = F.leaky_relu(ref, 0.01)
        wp = pack_frag(wt, cpad if last else 256, dev)
        scd, shd = sc.contiguous().to(dev), sh.contiguous().to(dev)
        keep += [wp, scd, shd]
        setattr(d, "w" + slot, wp.data_ptr())
        setattr(d, "s" + slot, scd.data_ptr())
        setattr(d, "t" + slot, shd.data_ptr())
    out = torch.zeros(n, cout, h * w, device=dev)
    d.Cout, d.Cout_pad, d.out, d.out_img_stride, d.HW = cout, cpad, out.data_ptr(), cout * h * w, h * w
    return d, out, ref.reshape(n, cout, h * w), keep


def test_head_mlp_cin256_three_layers_batched():
    """m3d_head_mlp_forward_batched with Cin = 256 and w1 (the DLA-102 heads): four heads of one launch, Cout 36 / 1 / 17 on the
    64-channel output tile, each within 2e-4 (1 + |ref|) of the float64 chain and bit-identical to its single-head launch; the
    256-channel output tile (cls: 144 of 256) on its own; a launch that mixes Cin 128 and 256 is refused."""
    L, dev = _hip.lib(), _dev()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = [_head256_case(300 + i, co, 64, dev) for i, co in enumerate([36, 36, 1, 17])]
    arr = (_hip.MlpDesc * len(cases))(*[c[0] for c in cases])
    _hip.check(L.m3d_head_mlp_forward_batched(arr, len(cases), st))
    torch.cuda.synchronize()
    batched = [c[1].clone() for c in cases]
    for (d, out, ref, _), got in zip(cases, batched):
        assert _relerr(got.cpu(), ref) < 2e-4
        out.zero_()
        _hip.check(L.m3d_head_mlp_forward(d, st))
        torch.cuda.synchronize()
        assert torch.equal(out, got)
    wide = _head256_case(400, 144, 256, dev, n=1, h=11, w=37)
    _hip.check(L.m3d_head_mlp_forward(ctypes.byref(wide[0]), st))
    torch.cuda.synchronize()
    assert _relerr(wide[1].cpu(), wide[2]) < 2e-4
    mixed = _hip.MlpDesc.from_buffer_copy(cases[1][0])
    mixed.Cin = 128
    assert L.m3d_head_mlp_forward_batched((_hip.MlpDesc * 2)(cases[0][0], mixed), 2, st) != 0


@pytest.mark.parametrize("B,h,w,keys,res_mode,affine", [(2, 8, 16, 337, 1, True), (1, 16, 40, 337, 0, False),
                                                         (1, 16, 40, 85, 0, True), (1, 48, 160, 337, 1, True)])
def test_anab_attend_f32_cv256_matches_torch(B, h, w, keys, res_mode, affine):
    """m3d_anab_attend_f32 with Cv = 256 (two value-channel halves per pixel tile) against torch in float64: 2e-5 (1 + |ref|);
    both residual modes, with and without the BN affine, a ragged key tile, untouched neighbours of the output slice."""
    L, dev = _hip.lib(), _dev()
    g = torch.Generator().manual_seed(B * 1000 + keys + h)
    HW, cv, ck = h * w, 256, 168
    kcs, kp, qcs = ck + 24, (keys + 31) // 32 * 32, ck + 8
    q = torch.randn(B * HW, ck, generator=g) * 0.5
    khat = torch.randn(B, keys, ck, generator=g) * 0.3
    vhat = torch.randn(B, cv, keys, generator=g)
    res = torch.randn(B * HW, cv, generator=g)
    scale, shift = torch.rand(cv, generator=g) + 0.5, torch.randn(cv, generator=g) * 0.1
    S = torch.einsum("bpc,bkc->bpk", q.view(B, HW, ck).double(), khat.double())
    ref = torch.einsum("bpk,bck->bpc", torch.softmax(S, dim=-1), vhat.double()).reshape(B * HW, cv)
    sc, sh = (scale.double(), shift.double()) if affine else (torch.ones(cv, dtype=torch.float64), torch.zeros(cv, dtype=torch.float64))
    ref = (ref + res.double()) * sc + sh if res_mode else ref * sc + sh + res.double()
    ref = F.leaky_relu(ref, 0.01)
    dq = torch.full((B * HW, qcs), 3.0)
    dq[:, :ck] = q
    dk = torch.full((B, kp, kcs), 7.0)
    dk[:, :keys, :ck] = khat
    dv = torch.full((B, cv, kp), 7.0)
    dv[:, :, :keys] = vhat
    dq, dk, dv, dr = (t.contiguous().to(dev) for t in (dq, dk, dv, res))
    dsc, dsh = scale.to(dev), shift.to(dev)
    out = torch.full((B * HW, cv + 4), 512.0, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _hip.check(L.m3d_anab_attend_f32(dq.data_ptr(), qcs, dk.data_ptr(), kcs, dv.data_ptr(), B, HW, ck, keys, kp, cv, dr.data_ptr(), cv,
                                     res_mode, dsc.data_ptr() if affine else None, dsh.data_ptr() if affine else None, 1,
                                     out.data_ptr(), cv + 4, st))
    torch.cuda.synchronize()
    assert (out[:, cv:] == 512.0).all()
    got = out[:, :cv].cpu().double()
    assert ((got - ref).abs() <= 2e-5 * (1.0 + ref.abs())).all(), (got - ref).abs().max().item()
    # Cv = 256 is built for Ck = 168 only
    assert L.m3d_anab_attend_f32(dq.data_ptr(), qcs, dk.data_ptr(), kcs, dv.data_ptr(), B, HW, 128, keys, kp, cv, None, 0, 0, None,
                                 None, 0, out.data_ptr(), cv + 4, st) != 0
