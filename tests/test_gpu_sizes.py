"""GPU tests (-m gpu) of the fp32 and bf16 engines at the image sizes of tests/size_cases.py: sizes that steer the plan builder into
the branches the two benched sizes never take (Engine._conv thresholds, the three forms of ANAB, the two poolings, odd level-4 /
level-5 maps, fewer anchors than nms_topN_pre, the bf16 engine's refusal).  What is under test is the engine's own work -- the
selection, the View.slice / channel-stride arithmetic of the concat buffers, the workspace sizing -- since the kernels behind the
branches have their own tests.  Bounds: those of test_gpu_network.test_forward_matches_oracle (gpu_common._forward_parity) and
of test_gpu_bf16._assert_bf16_report, unchanged.  tests/test_sizes_host.py pins on the CPU that the oracle has no near-tie
at the first five sizes, so that every row is compared there."""
import pytest
import torch

import size_cases as SC
from gpu_common import _clean_rows, _detect_vs_oracle, _dev, _forward_parity, _net_dt, _parity_log, _run_both
from m3dssd_amd import synth

pytestmark = pytest.mark.gpu

FP32_MFMA_KINDS = ("igemm", "wino", "conv_wave", "head_mlp")


def _kinds(plan):
    return {op[0]: op[1] for op in plan.ops if op[1] != "touch"}


def _conv_kinds(plan):
    """name -> kind of every launch that went through Engine._conv."""
    return {n: k for n, k in _kinds(plan).items() if k.startswith(("igemm", "wino_", "wino44<", "conv_wave"))}


def _assert_steers(case, plan):
    """The plan really took the branches the case was chosen for (names and kind strings of plan.ops)."""
    kinds = _kinds(plan)
    crop, HW = case.crop, (case.crop[0] // 8) * (case.crop[1] // 8)
    unfused = {"anab.logits", "anab.softmax", "anab.pv"}
    lv5 = [k for n, k in kinds.items() if n.startswith("base.base.level5.") and n.endswith((".tree1.conv2", ".tree2.conv1", ".tree2.conv2"))]
    assert len(lv5) == 3, kinds
    if crop in ((96, 224), (160, 416), (32, 64)):
        # HW no multiple of 128 and too few waves (or HW no multiple of 32) for the wave kernel: igemm, row softmax, igemm
        assert unfused <= set(kinds) and "anab.attend" not in kinds, kinds
        assert kinds["anab.logits"].startswith("igemm") and kinds["anab.pv"].startswith("igemm"), kinds
        # the igemm takes per-image weights in one launch only where no tile straddles two images
        assert kinds["anab.logits"].endswith(",per_image>") == (HW % 64 != 0), kinds
    if crop in ((96, 256), (64, 128), (256, 256)):
        assert HW % 128 == 0 and "anab.attend" in kinds and not (unfused & set(kinds)), kinds
    if crop == (160, 192):
        assert unfused <= set(kinds) and "anab.attend" not in kinds, kinds
        assert kinds["anab.logits"].startswith("conv_wave"), kinds["anab.logits"]
    if crop == (256, 256):
        assert "anab.pool_nested" in kinds and "anab.pool_partial" not in kinds
    else:
        assert "anab.pool_partial" in kinds and "anab.pool_finish" in kinds and "anab.pool_nested" not in kinds
    if (crop[0] // 32) % 2 or (crop[1] // 32) % 2:
        # an odd level-5 map: F(2x2,3x3) works on 2x2 output tiles and is refused
        assert not any(k.startswith(("wino_wave", "wino_lds")) for k in lv5), lv5
    # the two Winograd forms work on 4x4 / 2x2 output tiles and take no ragged map: a level-4 map of 6x14 or a level-5 map of 3x7
    # must reach neither (m3d_wino44_applicable refuses H % 4 or W % 4, Engine._conv refuses odd maps for F(2x2))
    for op in plan.ops:
        if op[1].startswith("wino44<"):
            assert op[4].H % 4 == 0 and op[4].W % 4 == 0, op[:2]
        if op[1].startswith(("wino_wave", "wino_lds")):
            assert op[4].H % 2 == 0 and op[4].W % 2 == 0, op[:2]


@pytest.mark.parametrize("case", SC.SIZE_CASES, ids=SC.case_id)
def test_forward_matches_oracle_at_size(case):
    """The checks and bounds of test_forward_matches_oracle at a size that steers other plan branches.  Where the oracle has no
    near-tie (tests/test_sizes_host.py) the engine must take the oracle's decisions at every pixel, and every row of bbox_3d, all
    seven columns, is compared with the free-running oracle at 1e-3: no clean-row mask, no relaxed z3d.  Where it has a few, the
    scheme of test_forward_matches_oracle holds, and every differing decision must sit on one of those near-tie pixels.
    (32, 64) and (64, 128): the hard mask is off at every pixel with the synthetic weights (asserted in test_sizes_host.py), so
    these two cases do not cover the gated branch of the alignments; the other five do."""
    crop, B = case.crop, case.B
    run = _run_both(crop, B, False, case.seed)
    net, plan, out, free, inj, taps_free, taps_inj, ind, prob_sel = run
    _parity_log("sizes_plan_kinds", dict(crop=list(crop), B=B, conv_kinds=_conv_kinds(plan),
                                         other={n: k for n, k in _kinds(plan).items() if n not in _conv_kinds(plan)}))
    _assert_steers(case, plan)
    m, n_idx, n_flip = _forward_parity(run)
    b3 = out[3].cpu()
    e_free = (b3 - free[3]).abs()
    fg = taps_free["fg_prob"]
    near = SC.near_tie_mask(fg)
    o_mask, o_ind = fg.max(dim=1, keepdim=True)
    differs = (o_ind != ind) | ((o_mask > 0.5) != (prob_sel > 0.5))
    ok = _clean_rows(taps_free, ind, prob_sel, b3.shape[1] // (ind.shape[2] * ind.shape[3]))
    cols = [0, 1, 3, 4, 5, 6]
    rec = dict(crop=list(crop), B=B, seed=case.seed, n_idx=n_idx, n_flip=n_flip, near_ties=int(near.sum()),
               clean_frac=ok.float().mean().item(), bbox3d_free_all=e_free.max().item(),
               bbox3d_free_clean=e_free[:, :, cols][ok].max().item(), z3d_free_clean=e_free[:, :, 2][ok].max().item(), **m)
    print("sizes_forward", rec)
    _parity_log("sizes_forward_matches_oracle", rec)
    assert not (differs & ~near).any(), "a decision differs at a pixel that is no near-tie of the oracle"
    if case.near_ties == 0:
        assert int(near.sum()) == 0
        assert n_idx + n_flip == 0, (n_idx, n_flip)
        assert rec["bbox3d_free_all"] < 1e-3
        return
    assert ok.float().mean().item() > 0.9
    assert rec["bbox3d_free_clean"] < 1e-3
    assert rec["z3d_free_clean"] < (1e-3 if n_idx + n_flip == 0 else 5e-3)


def test_batch_invariance_and_determinism_at_96x224():
    """Image 1 of the batch of 2 == the same image alone (1e-4, as test_batch_invariance_and_determinism); two runs of the batch
    are bit-identical.  HW = 336: the unfused ANAB chain with per-image key / value weights."""
    case = SC.by_crop((96, 224))
    net, conf = _net_dt(case.crop, case.B, "f32")
    x = synth.synth_frames(case.B, case.crop, case.seed).to(_dev())
    with torch.no_grad():
        a = [t.clone() for t in net(x)[:4]]
        b = [t.clone() for t in net(x)[:4]]
        single = [t.clone() for t in net(x[1:2])[:4]]
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for u, s in zip(a, single):
        assert (u[1:2] - s).abs().max().item() < 1e-4


@pytest.mark.parametrize("n,h,w", [(2, 13, 21), (3, 4, 24), (2, 8, 24)])
def test_standalone_anab_on_maps_that_are_no_multiple_of_128(n, h, w):
    """The stand-alone ANAB module (bound: test_standalone_modules_match_oracle's 5e-4) on maps that go through the unfused chain:
    H*W = 273 (odd) and 96 (a multiple of 32 only): one igemm launch per image; 192 (a multiple of 64): one igemm launch that
    takes every 64-row tile's weights from the tile's image."""
    from model.module.attention import ANAB
    from oracle import model_cpu
    sd = synth.synth_state_dict(0)
    x = torch.randn(n, 128, h, w, generator=torch.Generator().manual_seed(11))
    an = ANAB(128, 1).eval()
    an.load_state_dict({k[len("bbox_z3d_gl.0."):]: v for k, v in sd.items() if k.startswith("bbox_z3d_gl.0.")})
    ref = model_cpu.anab(sd, "bbox_z3d_gl.0", x)
    got = an.to(_dev())(x.to(_dev())).cpu()
    err = ((got - ref).abs() / (1.0 + ref.abs())).max().item()
    _parity_log("sizes_standalone_anab", dict(n=n, h=h, w=w, relerr=err))
    assert err < 5e-4


# ------------------------------------------------------------------------------------ detection
DETECT_CROPS = [(96, 224), (32, 64)]


@pytest.mark.parametrize("crop", DETECT_CROPS, ids=lambda c: "%dx%d" % c)
def test_detect_matches_oracle_at_size(crop):
    """detect_batch / im_detect_3d against the oracle's detection path on the engine's own outputs.  (32, 64): 36 * 32 = 1152
    anchors, fewer than nms_topN_pre = 3000 -- every row goes through the decode and the NMS."""
    case = SC.by_crop(crop)
    n_kept, n_pre = _detect_vs_oracle(crop, case.B, None, case.seed)
    conf = synth.synth_conf(crop, 0, batch_size=case.B, device="cuda:0")
    R = 36 * (crop[0] // 8) * (crop[1] // 8)
    assert n_pre == min(int(conf.nms_topN_pre), R) and n_kept > 0
    if crop == (32, 64):
        assert R == 1152 < int(conf.nms_topN_pre) and n_pre == R


@pytest.mark.parametrize("k", [None, 100])
@pytest.mark.parametrize("crop", DETECT_CROPS, ids=lambda c: "%dx%d" % c)
def test_detectors_equal_detect_batch_at_size(crop, k):
    """FrameDetector and PipelinedDetector, dense and with the detection-only tail (sparse_heads on), against the eager
    detect_batch on four batches in a row: identical detections, as test_gpu_sparse_heads demands at 128x320.  k: nms_topN_pre
    (None: the configuration's 3000; 100: a list that leaves pixels out)."""
    from lib.rpn_util import detect_batch
    from m3dssd_amd.pipeline import FrameDetector
    from test_gpu_sparse_heads import _run_detectors
    case = SC.by_crop(crop)
    B, HW = case.B, (crop[0] // 8) * (crop[1] // 8)
    net, conf = _net_dt(crop, B, "f32")
    if k:
        conf.nms_topN_pre = k
    xs = [synth.synth_frames(B, crop, s).to(_dev()) for s in (case.seed, 11, 12, 13)]
    ref = []
    for x in xs:
        d, c = detect_batch(net, x, conf)
        ref.append((d.clone(), c.clone()))
    assert all(int(c.sum()) > 0 for _, c in ref)
    eng = net.engine()
    plan = eng.plan_for(B, *crop)
    assert plan.tail is not None
    for sparse in (False, True):
        got_p, got_f, n = _run_detectors(net, conf, xs, crop=crop, sparse_heads=sparse)
        for got in (got_p, got_f):
            assert len(got) == len(ref)
            for (gd, gc), (rd, rc) in zip(got, ref):
                assert torch.equal(gc, rc) and torch.equal(gd, rd), (crop, k, sparse)
        if sparse:
            _parity_log("sizes_sparse_n_rows", dict(crop=list(crop), k=int(conf.nms_topN_pre), n_rows=list(n), pixels=B * HW))
            assert all(0 < v <= B * HW for v in n), n
            assert plan.named["sparse_k"][0] == min(int(conf.nms_topN_pre), 36 * HW)
    # sparse_heads=None follows the plan-time rule: min(k, HW) rows can touch at most that many pixels
    want = min(int(conf.nms_topN_pre), HW) <= 0.5 * HW
    assert eng.sparse_heads_default(plan, conf.nms_topN_pre) is want
    assert FrameDetector(net, conf, *crop, batch=B).sparse_heads is want
    if k is None:
        assert want is False           # 3000 rows (or all 1152 of the 4x8 map) can touch every pixel: dense


# ------------------------------------------------------------------------------------ bf16 engine
@pytest.mark.parametrize("crop", [(96, 224), (160, 416)], ids=lambda c: "%dx%d" % c)
def test_bf16_engine_refuses_maps_that_are_no_multiple_of_128_and_caches_nothing(crop):
    """H*W/64 no multiple of 128: the bf16 module raises from plan construction, before any launch; the same module then runs
    (96, 256) and matches a fresh module bit for bit -- no half-built plan is kept."""
    from test_gpu_bf16 import _net
    dev = _dev()
    case, good = SC.by_crop(crop), SC.by_crop((96, 256))
    net, conf = _net(crop, case.B, "bf16")
    x = synth.synth_frames(case.B, crop, case.seed).to(dev)
    for _ in range(2):
        with pytest.raises(RuntimeError, match="multiple of 128"):
            net(x)
    eng = net.engine()
    assert type(eng).__name__ == "EngineBF16" and (case.B,) + crop not in eng.plans
    xg = synth.synth_frames(good.B, good.crop, good.seed).to(dev)
    fresh, _ = _net(good.crop, good.B, "bf16")
    with torch.no_grad():
        a = [t.clone() for t in eng.forward(xg, fresh=True)]
        b = [t.clone() for t in fresh.engine().forward(xg, fresh=True)]
    assert list(eng.plans) == [(good.B,) + good.crop]
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)


@pytest.mark.parametrize("crop", [(96, 256), (64, 128), (256, 256)], ids=lambda c: "%dx%d" % c)
def test_bf16_network_matches_fp32_oracle_at_size(crop):
    """test_bf16_network_matches_fp32_oracle_within_stated_tolerance at the sizes the bf16 engine accepts: the same report, the
    same bounds (1.3 x the largest value seen at 1280x384, held by the smaller maps too)."""
    from test_gpu_bf16 import BF16_P999_MEASURED_AT, _assert_bf16_report, _bf16_vs_oracle, _log, _net
    case = SC.by_crop(crop)
    B = case.B
    net, conf = _net(crop, B, "bf16")
    x = synth.synth_frames(B, crop, case.seed)
    with torch.no_grad():
        outs = [t.cpu() for t in net(x.to(_dev()))[:4]]
    eng = net.engine()
    assert type(eng).__name__ == "EngineBF16"
    plan = eng.plan_for(B, *crop)
    kinds = _kinds(plan)
    assert all(not k.startswith(FP32_MFMA_KINDS) for k in kinds.values()), "fp32 MFMA kernel in the bf16 plan"
    assert "anab.attend" in kinds and ("anab.pool_nested" in kinds) == (crop == (256, 256)), kinds
    rep = _bf16_vs_oracle(net, plan, x, outs, list(range(B)), crop)
    print("sizes_bf16", rep)
    rep["kinds"] = kinds
    _log("sizes_bf16_network", rep)
    _assert_bf16_report(rep, full_size=False, p999_measured=BF16_P999_MEASURED_AT.get(crop))
