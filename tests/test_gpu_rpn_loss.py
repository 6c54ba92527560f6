"""GPU tests (-m gpu) of RPN_3D_loss on the device: m3d_rpn_targets + m3d_rpn_loss behind lib.loss.rpn_3d.RPN_3D_loss.

Yardstick: tests/rpn_loss_ref.py in float64 (pinned on the CPU against the reference's own numbers by
tests/test_rpn_loss_host.py).  Labels, the gt index of every regression target and the sampled masks must be EQUAL on every
anchor of every case; normalised targets within rpn_loss_ref.target_tolerance; loss, each stat and the three gradients within
rpn_loss_ref.DEVICE_BOUNDS (4 x the float32-vs-float64 error of the restatement, measured on the CPU).  Cases: the five golden
files and two seeded full-size batches (384x1280, B = 4 with 12 and B = 8 with 32 ground truths per image) that pass the
generator's uniqueness checks."""
import os

import numpy as np
import pytest
import torch

from m3dssd_amd.host import loss as hl
from m3dssd_amd.host import ops
from gpu_common import _dev, _log, _net_dev, CROP
import rpn_loss_ref as RR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _case(name):
    if name in RR.FULL_CASES:
        seed, B, ng = RR.FULL_CASES[name]
        return RR.loss_conf((384, 1280), 0), RR.make_case(seed, (384, 1280), B, ng)
    return RR.golden_case(np.load(os.path.join(GOLDEN, "rpn_loss_%s.npz" % name)))


def _run_device(conf, case, grads=True):
    dev = _dev()
    cls, prob, b2, b3, imobjs, fs = case
    crit = hl.RPN_3D_loss(conf)
    ins = [t.to(dev).requires_grad_(grads) for t in (cls, b2, b3)]
    loss, stats = crit(ins[0], prob.to(dev), ins[1], ins[2], imobjs, fs)
    out = dict(loss_t=loss, loss=float(loss.detach()), stats=stats, crit=crit)
    for k in ("labels", "gt_index", "targets", "sampled"):
        out[k] = crit.last[k].cpu().numpy()
    if grads:
        loss.backward()
        for k, t in zip(("g_cls", "g_bbox_2d", "g_bbox_3d"), ins):
            out[k] = t.grad.double().cpu().numpy()
    return out


def _compare(name, conf, d, r, check_grads=True, g2d_bound=None):
    """Exact on every anchor: labels, gt index, sampled.  Bounded: targets, loss, stats, gradients.  Prints each figure first."""
    assert np.array_equal(d["labels"].astype(np.int64), r["labels"]), "labels differ on %d anchors" % (d["labels"] != r["labels"]).sum()
    assert np.array_equal(d["gt_index"].astype(np.int64), r["gt_index"])
    assert np.array_equal(d["sampled"], r["sampled"]), "sampled masks differ on %d anchors" % (d["sampled"] != r["sampled"]).sum()
    terr = np.abs(d["targets"].astype(np.float64) - r["targets"])
    tol = RR.target_tolerance(r["targets"], conf)
    fig = {"targets_not_identical": int((terr > 0).sum()), "targets_max_err_over_tol": float((terr / np.maximum(tol, 1e-300)).max())}
    fig["loss"] = abs(d["loss"] - r["loss"]) / abs(r["loss"]) if np.isfinite(r["loss"]) and r["loss"] != 0 else float(d["loss"] != r["loss"])
    names_d, names_r = [RR.stat_key(s) for s in d["stats"]], [RR.stat_key(s) for s in r["stats"]]
    fig["stat"] = 0.0
    for a, b in zip(d["stats"], r["stats"]):
        if np.isfinite(b["val"]):
            fig["stat"] = max(fig["stat"], abs(a["val"] - b["val"]) / max(abs(b["val"]), 1e-30))
    if check_grads:
        for k in ("g_cls", "g_bbox_2d", "g_bbox_3d"):
            fig[k] = RR.rel(d[k], r[k])
    print("device vs float64 restatement %s: %s" % (name, fig))
    _log("rpn_loss_" + name, fig)
    assert names_d == names_r, (names_d, names_r)
    assert (terr <= tol).all()
    for k, v in fig.items():
        if k.startswith("targets"):
            continue
        bound = g2d_bound if (k == "g_bbox_2d" and g2d_bound is not None) else RR.DEVICE_BOUNDS[k]
        assert v <= bound, (k, v, bound)
    for s in d["stats"]:
        assert set(s) == {"name", "val", "format", "group"}


@pytest.mark.parametrize("name", RR.GOLDEN_CASES + tuple(RR.FULL_CASES))
def test_loss_matches_the_float64_restatement(name):
    conf, case = _case(name)
    r = RR.rpn_3d_loss(conf, *case, dtype=torch.float64)
    if name in RR.FULL_CASES:
        assert RR.nearest_threshold_gap(r["overlaps"], conf) > 1e-9 and all(lo != hi for lo, hi in r["margins"])
    d = _run_device(conf, case)
    assert d["loss_t"].dtype == torch.float32 and d["loss_t"].dim() == 0 and d["loss_t"].is_cuda and d["loss_t"].grad_fn is not None
    _compare(name, conf, d, r, g2d_bound=RR.G2D_CASE_BOUNDS.get(name))
    if name not in RR.FULL_CASES:        # and the reference's own labels / masks, anchor by anchor
        G = np.load(os.path.join(GOLDEN, "rpn_loss_%s.npz" % name))
        assert np.array_equal(d["labels"], G["labels"])
        assert np.array_equal(d["sampled"], RR.unpack_sampled(G, d["sampled"].shape))


def test_fg_fraction_none_with_all_boxes():
    conf, case = _case("shipped")
    conf.update(fg_fraction=None, box_samples=float("inf"))
    r = RR.rpn_3d_loss(conf, *case, dtype=torch.float64)
    _compare("fg_fraction_none", conf, _run_device(conf, case), r)


def test_hard_negatives_off_with_all_boxes_draws_nothing():
    conf, case = _case("shipped")
    conf.update(hard_negatives=False, box_samples=float("inf"))
    ref = RR.loss_conf((128, 320), 0, box_samples=float("inf"))
    _compare("all_boxes_no_hard_negatives", conf, _run_device(conf, case), RR.rpn_3d_loss(ref, *case, dtype=torch.float64))


def test_twenty_calls_are_bitwise_identical():
    conf, case = _case("full_b4")
    dev = _dev()
    cls, prob, b2, b3, imobjs, fs = case
    crit = hl.RPN_3D_loss(conf)
    ins = [t.to(dev) for t in (cls, prob, b2, b3)]
    first = None
    for i in range(20):
        loss, stats = crit(*ins, imobjs, fs)
        got = [loss.cpu().numpy().tobytes(), crit.last["stats"].cpu().numpy().tobytes()] + \
              [g.cpu().numpy().tobytes() for g in crit.last["grads"]] + \
              [crit.last[k].cpu().numpy().tobytes() for k in ("labels", "gt_index", "targets", "sampled")]
        if first is None:
            first = got
        assert got == first, "call %d differs from call 0" % i


def _gt(cls, box, vis=1.0, z=20.0):
    x, y, w, h = box
    return RR.Conf(cls=cls, ign=False, visibility=vis, bbox_full=np.array([x, y, w, h], dtype=np.float64),
                   bbox_3d=[x + w / 2, y + h / 2, z, 1.6, 1.5, 3.9, 0.3, 0.0, 1.0, z])


def _im(gts):
    return RR.Conf(gts=gts, p2=np.eye(4), p2_inv=np.eye(4), scale_factor=1.0)


def test_no_fg_in_the_batch_leaves_the_cls_term():
    """A valid ground truth no anchor shape fits (12 : 1) has no fg anchor: bg rows are sampled, only `cls` and the acc stats."""
    conf = RR.loss_conf((128, 320), 0)
    cls, prob, b2, b3, _, fs = RR.make_case(31)
    imobjs = [_im([_gt("Car", (5.0, 40.0, 300.0, 25.0))]), _im([_gt("Pedestrian", (10.0, 50.0, 290.0, 24.5))])]
    case = (cls, prob, b2, b3, imobjs, fs)
    r = RR.rpn_3d_loss(conf, *case, dtype=torch.float64)
    assert r["fg_num"] == 0 and r["bg_num"] > 0 and [RR.stat_key(s) for s in r["stats"]] == ["acc_bg", "loss_cls"]
    d = _run_device(conf, case)
    _compare("no_fg", conf, d, r)
    assert not d["g_bbox_2d"].any() and not d["g_bbox_3d"].any()


def test_batch_without_any_valid_gt_is_zero():
    """Every image is skipped (ignore regions only): loss 0, no sampled anchor, zero gradients, only the bg accuracy."""
    conf = RR.loss_conf((128, 320), 0)
    cls, prob, b2, b3, _, fs = RR.make_case(32)
    imobjs = [_im([_gt("Van", (30.0, 20.0, 60.0, 50.0))]), _im([])]
    case = (cls, prob, b2, b3, imobjs, fs)
    r = RR.rpn_3d_loss(conf, *case, dtype=torch.float64, grads=False)
    d = _run_device(conf, case)
    assert d["loss"] == 0.0 and r["loss"] == 0.0 and not d["sampled"].any()
    assert [RR.stat_key(s) for s in d["stats"]] == [RR.stat_key(s) for s in r["stats"]] == ["acc_bg"]
    assert d["stats"][0]["val"] == r["stats"][0]["val"]
    assert not d["g_cls"].any() and not d["g_bbox_2d"].any() and not d["g_bbox_3d"].any()
    assert not d["labels"].any() and not d["targets"].any()


def test_a_disjoint_predicted_box_gives_inf_and_finite_gradients():
    """The reference returns +inf (and NaN gradients in that row); the device returns +inf, a zero IoU-term gradient for that row
    and the restatement's gradients everywhere else."""
    conf, case = _case("shipped")
    cls, prob, b2, b3, imobjs, fs = case
    r0 = RR.rpn_3d_loss(conf, *case, dtype=torch.float64)
    b, row = np.argwhere(r0["sampled"] == 1)[0]
    b2 = b2.clone()
    b2[b, row, 0] = 200.0                      # the decoded box moves ~100 widths away
    case = (cls, prob, b2, b3, imobjs, fs)
    r = RR.rpn_3d_loss(conf, *case, dtype=torch.float64)
    d = _run_device(conf, case)
    assert r["loss"] == float("inf") and d["loss"] == float("inf")
    assert np.isfinite(d["g_cls"]).all() and np.isfinite(d["g_bbox_2d"]).all() and np.isfinite(d["g_bbox_3d"]).all()
    assert not d["g_bbox_2d"][b, row].any()
    assert not np.isfinite(r["g_bbox_2d"][b, row]).all()
    keep = np.ones(d["sampled"].shape, dtype=bool)
    keep[b, row] = False
    assert np.array_equal(d["sampled"], r["sampled"])
    for k in ("g_cls", "g_bbox_2d", "g_bbox_3d"):
        assert RR.rel(d[k][keep], r[k][keep]) <= RR.DEVICE_BOUNDS[k], k
    vals = {RR.stat_key(s): s["val"] for s in d["stats"]}
    assert vals["loss_iou"] == float("inf") and np.isfinite(vals["loss_cls"]) and np.isfinite(vals["acc_iou"])


def test_more_ground_truths_than_the_cap_is_an_argument_error():
    conf = RR.loss_conf((128, 320), 0)
    cls, prob, b2, b3, _, fs = RR.make_case(33)
    rng = np.random.Generator(np.random.PCG64(5))
    many = [_gt("Car", (float(rng.uniform(0, 250)), float(rng.uniform(0, 60)), 40.0, 50.0)) for _ in range(hl.MAX_GT + 1)]
    dev = _dev()
    with pytest.raises(RuntimeError, match="M3D_RPN_MAX_GT"):
        hl.RPN_3D_loss(conf)(cls.to(dev), prob.to(dev), b2.to(dev), b3.to(dev), [_im(many), _im(many[:3])], fs)
    # exactly the cap runs (64 valid + 64 ignore regions) and agrees with the restatement
    full = many[:64] + [_gt("Van", tuple(g.bbox_full)) for g in many[64:128]]
    case = (cls, prob, b2, b3, [_im(full), _im(many[:3])], fs)
    r = RR.rpn_3d_loss(conf, *case, dtype=torch.float64)
    if RR.nearest_threshold_gap(r["overlaps"], conf) > 1e-9 and all(lo != hi for lo, hi in r["margins"]):
        _compare("at_the_cap", conf, _run_device(conf, case), r, check_grads=False)
    else:
        pytest.fail("the at-the-cap case is not unique; choose another seed")


def test_bad_inputs_are_rejected_with_a_message():
    conf, case = _case("shipped")
    dev = _dev()
    cls, prob, b2, b3 = [t.to(dev) for t in case[:4]]
    imobjs, fs = case[4], case[5]
    crit = hl.RPN_3D_loss(conf)
    with pytest.raises(RuntimeError, match="contiguous"):
        crit(cls.transpose(0, 1).contiguous().transpose(0, 1), prob, b2, b3, imobjs, fs)
    with pytest.raises(RuntimeError, match="bbox_2d has shape"):
        crit(cls, prob, b3, b3, imobjs, fs)
    with pytest.raises(RuntimeError, match="shape"):
        crit(cls[:, :-1], prob[:, :-1], b2[:, :-1], b3[:, :-1], imobjs, fs)
    with pytest.raises(RuntimeError, match="float32"):
        crit(cls.double(), prob, b2, b3, imobjs, fs)
    with pytest.raises(RuntimeError, match="imobjs"):
        crit(cls, prob, b2, b3, imobjs[:1], fs)
    with pytest.raises(NotImplementedError):
        crit(cls.cpu(), prob, b2, b3, imobjs, fs)
    for bad in (dict(bbox_3d_proj_lambda=1.0), dict(hard_negatives=False)):
        with pytest.raises(NotImplementedError):
            hl.RPN_3D_loss(RR.loss_conf(**bad))
    with pytest.raises(NotImplementedError):
        hl.RPN_3D_loss_smp(conf)


def test_ops_layer_and_grad_output_scaling():
    conf, case = _case("shipped")
    dev = _dev()
    cls, prob, b2, b3, imobjs, fs = case
    vec = hl.pack_conf(conf.bbox_means, conf.bbox_stds, conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo, conf.bg_thresh_hi,
                       conf.best_thresh, conf.box_samples, conf.fg_fraction, conf.focal_loss, conf.cls_2d_lambda, conf.iou_2d_lambda,
                       conf.bbox_2d_lambda, conf.bbox_3d_lambda, conf.feat_stride)
    table = hl.pack_gts(imobjs, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
    anchors = torch.from_numpy(np.asarray(conf.anchors, dtype=np.float64)).to(dev)
    r = RR.rpn_3d_loss(conf, *case, dtype=torch.float64)
    labels, gidx, targets, scores = ops.rpn_targets(cls.to(dev), prob.to(dev), anchors, vec, table, fs)
    assert np.array_equal(labels.cpu().numpy().astype(np.int64), r["labels"]) and np.array_equal(gidx.cpu().numpy().astype(np.int64), r["gt_index"])
    act = r["labels"] != RR.IGN_FLAG
    want = np.take_along_axis(prob.numpy(), np.where(act, r["labels"], 0)[..., None], axis=2)[..., 0]
    assert np.array_equal(scores.cpu().numpy()[act], want[act])
    ins = [t.to(dev).requires_grad_(True) for t in (cls, b2, b3)]
    loss, stats = ops.rpn_loss(ins[0], prob.to(dev), ins[1], ins[2], anchors, vec, table, fs)
    assert stats.shape == (len(hl.STAT_NAMES),) and stats.dtype == torch.float64 and not stats.requires_grad
    (loss * 3.0).backward()
    for k, t in zip(("g_cls", "g_bbox_2d", "g_bbox_3d"), ins):
        assert RR.rel(t.grad.double().cpu().numpy() / 3.0, r[k]) <= RR.DEVICE_BOUNDS[k], k


def test_loss_on_the_eval_mode_rpn_outputs():
    """The validation loss of a checkpoint at engine speed: the eval-mode RPN (DLA-34, synthetic weights) feeds the loss."""
    from m3dssd_amd import synth
    net, nconf = _net_dev(0, 2)
    x = synth.synth_frames(2, CROP, 1234).to(_dev())
    with torch.no_grad():
        cls, prob, b2, b3, fs, _rois = net(x)
    conf = RR.loss_conf(CROP, 0)
    imobjs = RR.make_case(11)[4]
    crit = hl.RPN_3D_loss(conf)
    loss, stats = crit(cls.contiguous(), prob.contiguous(), b2.contiguous(), b3.contiguous(), imobjs, fs)
    case = (cls.cpu(), prob.cpu(), b2.cpu(), b3.cpu(), imobjs, [int(fs[0]), int(fs[1])])
    r = RR.rpn_3d_loss(conf, *case, dtype=torch.float64, grads=False)
    unique = RR.nearest_threshold_gap(r["overlaps"], conf) > 1e-9 and all(lo != hi for lo, hi in r["margins"])
    d = dict(loss=float(loss), stats=stats)
    for k in ("labels", "gt_index", "targets", "sampled"):
        d[k] = crit.last[k].cpu().numpy()
    if not unique:          # equal scores at the cut: the documented tie rule (lower row first) is the restatement's rule too
        print("eval-mode outputs: equal scores at a cut; the tie rule decides")
    _compare("eval_rpn_outputs", conf, d, r, check_grads=False)


def _head_run(device, dtype_ref, steps=5):
    """Five SGD steps of a 1x1-conv head (ATen) on a fixed feature map; the loss is the device one (device='cuda') or the
    restatement in `dtype_ref` (CPU).  Returns the loss trajectory."""
    conf = RR.loss_conf((128, 320), 0)
    imobjs, fs = RR.make_case(11)[4:6]
    g = torch.Generator().manual_seed(3)
    A, C = 36, 4
    feat = torch.randn(2, 16, fs[0], fs[1], generator=g)
    head = torch.nn.Conv2d(16, A * (C + 4 + 7), 1)
    with torch.no_grad():
        head.weight.copy_(torch.randn(head.weight.shape, generator=g) * 0.1)
        head.bias.zero_()
    if device == "cuda":
        head, feat = head.to(_dev()), feat.to(_dev())
        crit = hl.RPN_3D_loss(conf)
    opt = torch.optim.SGD(head.parameters(), lr=1e-3)
    traj = []
    for _ in range(steps):
        o = head(feat)                                                   # [B, A*15, H, W], channel = k*A + a
        o = o.view(2, C + 11, A, fs[0], fs[1]).permute(0, 2, 3, 4, 1).reshape(2, A * fs[0] * fs[1], C + 11)
        cls, b2, b3 = o[..., :C].contiguous(), o[..., C:C + 4].contiguous(), o[..., C + 4:].contiguous()
        prob = torch.softmax(cls, dim=2).detach()
        opt.zero_grad()
        if device == "cuda":
            loss, _ = crit(cls, prob, b2, b3, imobjs, fs)
            loss.backward()
            traj.append(float(loss))
        else:
            r = RR.rpn_3d_loss(conf, cls.detach(), prob, b2.detach(), b3.detach(), imobjs, fs, dtype=dtype_ref)
            gs = [torch.from_numpy(r[k]).float() for k in ("g_cls", "g_bbox_2d", "g_bbox_3d")]
            torch.autograd.backward([cls, b2, b3], gs)
            traj.append(r["loss"])
        opt.step()
    return np.asarray(traj)


# five SGD steps: |loss_k(device) - loss_k(float64 restatement)| / loss_k.  Bound = 4 x the same figure between the float32 and
# the float64 restatement driving the same float32 head on the CPU (_head_run("cpu", torch.float32) against
# _head_run("cpu", torch.float64)) [measured 1.09e-7, at step 3].
SGD_BOUND = 5.0e-7


def test_five_sgd_steps_follow_the_restatement():
    ref = _head_run("cpu", torch.float64)
    dev = _head_run("cuda", None)
    err = np.abs(dev - ref) / np.abs(ref)
    print("SGD trajectory: restatement %s device %s rel err %s" % (ref, dev, err))
    _log("rpn_loss_sgd", {"ref": ref.tolist(), "dev": dev.tolist()})
    assert ref[-1] < ref[0], "the loss must go down"
    assert (err <= SGD_BOUND).all()
