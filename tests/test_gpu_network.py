"""GPU tests (-m gpu; every check goes through the C ABI of libm3dssd_hip.so) of the whole forward: stage-wise and end-to-end parity against the oracle and the reference goldens,
batch invariance, determinism soaks, hipGraph replay, the benched configurations, uint8 input path.
Re-filed by component in round 5 (before: per-round files); tolerances are stated at the checks."""
import collections
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from m3dssd_amd import _hip, synth
from gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("crop,B,pad", [((128, 320), 2, False), ((384, 1280), 1, True)])
def test_forward_matches_oracle(crop, B, pad):
    net, plan, out, free, inj, taps_free, taps_inj, ind, prob_sel = _run_both(crop, B, pad)
    b3 = out[3].cpu()
    m, n_idx, n_flip = _forward_parity((net, plan, out, free, inj, taps_free, taps_inj, ind, prob_sel))
    o_b3 = inj[3]
    # free-running oracle (its own decisions): every row away from a differing decision must agree too -- unconditional;
    # the z3d column sits behind ANAB's global pooling, so a differing pixel can move it everywhere, slightly
    assert n_idx + n_flip <= 8, (n_idx, n_flip)
    ok = _clean_rows(taps_free, ind, prob_sel, b3.shape[1] // (ind.shape[2] * ind.shape[3]))
    assert ok.float().mean().item() > 0.9
    e_free = (b3 - free[3]).abs()
    cols = [0, 1, 3, 4, 5, 6]
    e_clean = e_free[:, :, cols][ok].max().item()
    e_z = e_free[:, :, 2][ok].max().item()
    feats_gl_err = _relerr(plan.named["feats_gl"].torch_nchw().cpu(), taps_inj["feats_gl"])
    _parity_log("forward_matches_oracle", dict(crop=list(crop), B=B, n_idx=n_idx, n_flip=n_flip, clean_frac=ok.float().mean().item(),
                                               bbox3d_free_clean=e_clean, z3d_free_clean=e_z,
                                               bbox3d_inj=(b3 - o_b3).abs().max().item(), feats_gl_rel=feats_gl_err))
    assert e_clean < 1e-3
    assert e_z < (1e-3 if n_idx + n_flip == 0 else 5e-3)


def test_forward_matches_reference_golden_samples():
    """Against the vectors dumped from the reference itself (tools/gen_golden.py), full size."""
    net, plan, out, free, inj, taps_free, taps_inj, ind, prob_sel = _run_both((384, 1280), 1, True)
    g = np.load(os.path.join(GOLDEN, "model_384x1280_b1.npz"))
    st = int(g["stride"])
    cls = out[0].cpu()
    assert cls.shape == (1, 276480, 4)
    assert np.abs(cls[:, ::st].numpy() - g["cls"]).max() < 1e-3
    n_idx, n_flip = _check_decisions(taps_free, ind, prob_sel)
    # unconditional: the sampled rows away from any differing discrete decision must match the REFERENCE's own numbers
    # (prob is upstream of the decisions: every sampled row); the counts are bounded and logged
    assert n_idx + n_flip <= 8, (n_idx, n_flip)
    ok = _clean_rows(taps_free, ind, prob_sel, 36)[:, ::st].numpy()
    assert ok.mean() > 0.9
    e3 = np.abs(out[3].cpu()[:, ::st].numpy() - g["bbox_3d"])
    e2 = np.abs(out[2].cpu()[:, ::st].numpy() - g["bbox_2d"])
    _parity_log("forward_matches_reference_golden", dict(n_idx=n_idx, n_flip=n_flip, rows=int(ok.sum()), rows_total=int(ok.size),
                                                         bbox3d=float(e3[ok].max()), bbox2d=float(e2[ok].max())))
    assert np.abs(out[1].cpu()[:, ::st].numpy() - g["prob"]).max() < 1e-4
    assert e3[:, :, [0, 1, 3, 4, 5, 6]][ok].max() < 1e-3 and e2[ok].max() < 1e-3
    assert e3[:, :, 2][ok].max() < (1e-3 if n_idx + n_flip == 0 else 5e-3)


def test_batch_invariance_and_determinism():
    """Images are independent units: image i of a batch == the same image alone; two runs are bit-identical."""
    from model.M3d_inference_align import build
    dev = _dev()
    conf = synth.synth_conf((128, 320), 0, batch_size=3, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0))
    net = net.to(dev)
    x = synth.synth_frames(3, (128, 320), 77).to(dev)
    with torch.no_grad():
        a = [t.clone() for t in net(x)[:4]]
        b = [t.clone() for t in net(x)[:4]]
        single = [t.clone() for t in net(x[1:2])[:4]]
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for u, s in zip(a, single):
        assert (u[1:2] - s).abs().max().item() < 1e-4


# ------------------------------------------------------------------------------------ standalone modules
def test_standalone_modules_match_oracle():
    from model.module.attention import ANAB
    from model.module.feturealign_mgpu import center_align, shape_align
    from model.pose_dla_dcn import DeformConv
    from oracle import model_cpu
    dev = _dev()
    sd = synth.synth_state_dict(0)
    conf = synth.synth_conf((128, 320), 0, device="cuda:0")
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 128, 16, 40, generator=g)
    # DeformConv
    p = "base.ida_up.node_1"
    dc = DeformConv(128, 128).eval()
    dc.load_state_dict({k[len(p) + 1:]: v for k, v in sd.items() if k.startswith(p + ".")})
    ref = model_cpu.deform_conv(sd, p, x)
    assert _relerr(dc.to(dev)(x.to(dev)).cpu(), ref) < 5e-4
    # ANAB
    an = ANAB(128, 1).eval()
    an.load_state_dict({k[len("bbox_z3d_gl.0."):]: v for k, v in sd.items() if k.startswith("bbox_z3d_gl.0.")})
    ref = model_cpu.anab(sd, "bbox_z3d_gl.0", x)
    assert _relerr(an.to(dev)(x.to(dev)).cpu(), ref) < 5e-4
    # align modules (distinct fg probabilities -> unambiguous top-1)
    fg = torch.rand(2, 36, 16, 40, generator=g)
    anchors = torch.from_numpy(conf.anchors)
    sa = shape_align(128, anchors, 8, [16, 40]).eval()
    sa.load_state_dict({k[len("shape_align."):]: v for k, v in sd.items() if k.startswith("shape_align.")})
    ref = model_cpu.shape_align(sd, "shape_align", x, fg, conf.anchors, 8)
    assert _relerr(sa.to(dev)(x.to(dev), fg.to(dev)).cpu(), ref) < 5e-4
    bx, by = torch.randn(2, 36, 16, 40, generator=g), torch.randn(2, 36, 16, 40, generator=g)
    ca = center_align(128, anchors, conf.bbox_means[0][0:2], conf.bbox_stds[0][0:2], 8, [16, 40]).eval()
    ca.load_state_dict({k[len("center_align2d."):]: v for k, v in sd.items() if k.startswith("center_align2d.")})
    ref = model_cpu.center_align(sd, "center_align2d", x, bx, by, fg, conf.anchors, conf.bbox_means[0][0:2],
                                 conf.bbox_stds[0][0:2], 8)
    got = ca.to(dev)(x.to(dev), bx.to(dev), by.to(dev), fg.to(dev)).cpu()
    assert _relerr(got, ref) < 5e-4


def test_dlaseg_standalone_matches_oracle():
    from model.pose_dla_dcn import DLASeg
    from oracle import model_cpu
    dev = _dev()
    sd = synth.synth_state_dict(0)
    conf = synth.synth_conf((128, 320), 0, device="cuda:0")
    m = DLASeg("dla34", False, 8, 1, 5, 256, conf).eval()
    m.load_state_dict({k[len("base."):]: v for k, v in sd.items() if k.startswith("base.")})
    x = synth.synth_frames(1, (128, 320), 5)
    ref = model_cpu.dla_seg(sd, "base", x)
    got = m.to(dev)(x.to(dev)).cpu()
    assert got.shape == ref.shape == (1, 128, 16, 40)
    assert _relerr(got, ref) < 1e-3


def test_graph_replay_matches_eager():
    """The whole step (forward + bundle + top-k + decode + NMS) captured in a hipGraph replays bit-identically."""
    from lib.rpn_util import detect_batch
    from model.M3d_inference_align import build
    dev = _dev()
    conf = synth.synth_conf((128, 320), 0, batch_size=2, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0))
    net = net.to(dev)
    x = synth.synth_frames(2, (128, 320), 3).to(dev)
    d0, c0 = detect_batch(net, x, conf)
    d0, c0 = d0.clone(), c0.clone()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        detect_batch(net, x, conf)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            gd, gc = detect_batch(net, x, conf)
    torch.cuda.current_stream().wait_stream(s)
    x2 = synth.synth_frames(2, (128, 320), 4).to(dev)
    e1, n1 = detect_batch(net, x2, conf)
    e1, n1 = e1.clone(), n1.clone()
    x.copy_(x2)                       # the graph reads the captured input buffer
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gd, e1) and torch.equal(gc, n1)
    assert not torch.equal(e1, d0)


def test_full_size_batch8_uses_wave_kernels_and_matches_batch1():
    """At bs=8 / 1280x384 the plan picks the wave-granular kernels (enough waves), at bs=1 the LDS-tiled ones (oracle-checked
    above): image i of the batch must equal the same image alone, so the two kernel families cross-check at full size."""
    from model.M3d_inference_align import build
    dev = _dev()
    conf = synth.synth_conf((384, 1280), 0, batch_size=8, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0))
    net = net.to(dev)
    x = synth.synth_frames(8, (384, 1280), 4321).to(dev)
    with torch.no_grad():
        full = [t.clone() for t in net(x)[:4]]
        kinds8 = {op[1] for op in net.engine().plan_for(8, 384, 1280).ops}
        one = [t.clone() for t in net(x[5:6])[:4]]
        kinds1 = {op[1] for op in net.engine().plan_for(1, 384, 1280).ops}
    assert any(k.startswith("wino44") for k in kinds8) and any(k.startswith("conv_wave") for k in kinds8)
    assert "wino_wave<32,32>" not in kinds1 and "wino44<16,32>" not in kinds1
    for name, u, s_, tol in zip(("cls", "prob", "bbox_2d", "bbox_3d"), full, one, (1e-3, 1e-4, 1e-3, 1e-3)):
        err = (u[5:6] - s_).abs().max().item()
        assert err < tol, (name, err)


def test_config4_shard_size_batch32_properties():
    """BASELINE.json config 4 shards 32 images per GPU: at that size (1280x384) image i of the batch equals the same image alone,
    two runs are bit-identical, and the detections of the batch equal those of its two halves (size-independent properties)."""
    from lib.rpn_util import detect_batch
    from model.M3d_inference_align import build
    dev = _dev()
    conf = synth.synth_conf((384, 1280), 0, batch_size=32, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0))
    net = net.to(dev)
    x = synth.synth_frames(32, (384, 1280), 99).to(dev)
    with torch.no_grad():
        a = [t.clone() for t in net(x)[:4]]
        b = [t.clone() for t in net(x)[:4]]
        one = [t.clone() for t in net(x[17:18])[:4]]
        dets, counts = (t.clone() for t in detect_batch(net, x, conf))
        d0, c0 = (t.clone() for t in detect_batch(net, x[:16], conf))
        d1, c1 = (t.clone() for t in detect_batch(net, x[16:], conf))
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for name, u, s_, tol in zip(("cls", "prob", "bbox_2d", "bbox_3d"), a, one, (1e-3, 1e-4, 1e-3, 1e-3)):
        assert (u[17:18] - s_).abs().max().item() < tol, name
    assert torch.equal(counts, torch.cat([c0, c1]))
    dref = torch.cat([d0, d1])                                         # decoded pixels / metres of the same kept anchors:
    assert ((dets - dref).abs() <= 2e-4 * (1.0 + dref.abs())).all()    # the batch-32 and batch-16 plans run the same kernels
    assert torch.equal(dets[:, :, 13], torch.cat([d0, d1])[:, :, 13])  # identical anchor ids row by row


# ------------------------------------------------------------------------------------ test-time input path (8f row 4)
def test_preprocess_u8_bit_exact_and_fused_stem():
    """m3d_preprocess_u8 == oracle.preprocess == the reference golden, bit for bit (IEEE division, numpy's operation order);
    the stem fed with uint8 frames (m3d_stem_conv7x7_u8) == the stem fed with the preprocessed float image, bit for bit."""
    import ctypes
    from m3dssd_amd import _hip
    from m3dssd_amd.host.preprocess import preprocess
    from oracle.preprocess import preprocess as opre
    dev = _dev()
    L = _hip.lib()
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "preprocess.npz"))
    mean, stds = g["mean"], g["stds"]
    for n in "abc":
        got = preprocess(torch.from_numpy(g["in_" + n]).to(dev), tuple(g["size_" + n]), mean, stds).cpu().numpy()[0]
        assert np.array_equal(got, g["out_" + n])
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, size=(3, 50, 70, 3)).astype(np.uint8)            # batch of 3, padded to 64x96
    want = np.stack([opre(f, (64, 96), mean, stds) for f in frames])
    xf = preprocess(torch.from_numpy(frames).to(dev), (64, 96), mean, stds)
    assert np.array_equal(xf.cpu().numpy(), want)
    with pytest.raises(RuntimeError):
        preprocess(torch.from_numpy(frames).to(dev), (32, 96), mean, stds)         # frame taller than the target
    with pytest.raises(NotImplementedError):
        preprocess(torch.from_numpy(frames), (64, 96), mean, stds)                 # host tensor
    # fused stem
    w = torch.randn(7 * 7 * 3 * 16, device=dev) * 0.1
    sc, sh = torch.rand(16, device=dev) + 0.5, torch.randn(16, device=dev) * 0.1
    o1, o2 = torch.zeros(3 * 64 * 96 * 16, device=dev), torch.zeros(3 * 64 * 96 * 16, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    m3, s3 = (ctypes.c_float * 3)(*mean.tolist()), (ctypes.c_float * 3)(*stds.tolist())
    fr = torch.from_numpy(frames).to(dev)
    _hip.check(L.m3d_stem_conv7x7(xf.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), o1.data_ptr(), 16, 3, 64, 96, st))
    _hip.check(L.m3d_stem_conv7x7_u8(fr.data_ptr(), 50, 70, m3, s3, w.data_ptr(), sc.data_ptr(), sh.data_ptr(), o2.data_ptr(), 16,
                                     3, 64, 96, st))
    assert torch.equal(o1, o2)


def test_network_accepts_uint8_frames():
    """net(uint8 BGR frames) == net(Preprocess(frames)) exactly: the input path runs inside the stem kernel."""
    from m3dssd_amd.host.preprocess import preprocess
    from model.M3d_inference_align import build
    dev = _dev()
    conf = synth.synth_conf((128, 320), 0, batch_size=2, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0))
    net = net.to(dev)
    rng = np.random.RandomState(5)
    frames = torch.from_numpy(rng.randint(0, 256, size=(2, 120, 310, 3)).astype(np.uint8)).to(dev)
    with torch.no_grad():
        a = [t.clone() for t in net(frames)[:4]]
        x = preprocess(frames, conf.crop_size, conf.image_means, conf.image_stds)
        b = [t.clone() for t in net(x)[:4]]
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert float(a[3].abs().max()) > 0


def test_fp32_forward_without_f4x4_is_bit_identical_over_40_runs(monkeypatch):
    """The F(2x2,3x3) wave kernel (and its split-K form) serves the 3x3 layers wherever the F(4x4) kernel does not apply or is
    switched off (M3D_WINO44=0): same soak on that plan."""
    import m3dssd_amd.engine as E
    monkeypatch.setattr(E, "USE_WINO44", False)
    bad, nbuf, kinds = _soak("f32", 8, (384, 1280), 40)
    assert "wino_wave" in kinds and "wino44" not in kinds, kinds
    assert not bad, bad[:3]


def test_bf16_forward_is_bit_identical_over_40_runs_at_batch_64():
    bad, nbuf, kinds = _soak("bf16", 64, (384, 1280), 40)
    assert {"bf16_halo", "bf16_conv", "bf16_head2", "bf16_frontend2", "bf16_anab", "bf16_dcn_patch"} <= kinds, kinds
    assert not bad, bad[:3]

