"""GPU tests (-m gpu) of RPN_3D_loss_smp on the device: m3d_rpn_loss_smp (ingest launch + the select / loss / finish launches
of m3d_rpn_loss) and m3d_rpn_precompute_targets behind lib.loss.rpn_3d.RPN_3D_loss_smp.

Yardsticks: tests/rpn_loss_smp_ref.py in float64 (pinned on the CPU against the reference's own numbers by
tests/test_rpn_loss_smp_host.py) within rpn_loss_ref.DEVICE_BOUNDS, the reference's own labels and sampled masks
(tests/golden/rpn_loss_smp_*.npz) anchor by anchor, and RPN_3D_loss on the device BIT FOR BIT: the same kernels get the same
bits and add in a fixed order."""
import os

import numpy as np
import pytest
import torch

from m3dssd_amd.host import loss as hl
from m3dssd_amd.host import ops
from gpu_common import _dev, _log
import poison
import rpn_loss_ref as RR
import rpn_loss_smp_ref as SR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _smp_conf(conf):
    conf.device = "cuda:0"
    return conf


def _vec(conf):
    return hl.pack_conf(conf.bbox_means, conf.bbox_stds, conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo, conf.bg_thresh_hi,
                        conf.best_thresh, conf.box_samples, conf.fg_fraction, conf.focal_loss, conf.cls_2d_lambda, conf.iou_2d_lambda,
                        conf.bbox_2d_lambda, conf.bbox_3d_lambda, conf.feat_stride)


def _precompute(conf, imobjs, fs):
    table = hl.pack_gts(imobjs, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
    return ops.rpn_precompute_targets(np.asarray(conf.anchors, dtype=np.float64), _vec(conf), table, fs, _dev()), table


def _bits(crit, loss):
    """Everything a call computed, as bytes."""
    d = crit.last
    return {"loss": loss.detach().cpu().numpy().tobytes(), "sampled": d["sampled"].cpu().numpy().tobytes(),
            "labels": d["labels"].cpu().numpy().tobytes(), "targets": d["targets"].cpu().numpy().tobytes(),
            "scores": d["scores"].cpu().numpy().tobytes(), "stats": d["stats"].cpu().numpy()[:len(hl.STAT_NAMES)].tobytes(),
            "g_cls": d["grads"][0].cpu().numpy().tobytes(), "g_bbox_2d": d["grads"][1].cpu().numpy().tobytes(),
            "g_bbox_3d": d["grads"][2].cpu().numpy().tobytes()}


def _run(crit, case, target, grads=True):
    dev = _dev()
    cls, prob, b2, b3, _imobjs, fs = case
    ins = [t.to(dev).requires_grad_(grads) for t in (cls, b2, b3)]
    loss, stats = crit(ins[0], prob.to(dev), ins[1], ins[2], target, fs)
    out = dict(loss_t=loss, loss=float(loss.detach()), stats=stats, bits=_bits(crit, loss))
    for k in ("labels", "targets", "sampled"):
        out[k] = crit.last[k].cpu().numpy()
    if grads and loss.grad_fn is not None:
        loss.backward()
        for k, t in zip(("g_cls", "g_bbox_2d", "g_bbox_3d"), ins):
            out[k] = t.grad.double().cpu().numpy()
            assert t.grad.cpu().numpy().tobytes() == out["bits"][k]            # grad_output = 1: the stored gradients themselves
    return out


@pytest.mark.parametrize("name", tuple(SR.GOLDEN_CASES))
def test_golden_cases_from_the_loaders_host_dict(name):
    """The reference-layout dict (host tensors, int64 labels) through pinned staging: labels and sampled masks equal the
    reference's on every anchor, stats names and order equal the reference's, numbers within DEVICE_BOUNDS of float64."""
    G = np.load(os.path.join(GOLDEN, "rpn_loss_smp_%s.npz" % name))
    conf, case = SR.golden_case(name)
    fs = case[5]
    target = SR.make_target(conf, case[4], fs)
    assert target["labels"].dtype == torch.int64 and not target["labels"].is_cuda
    r = SR.rpn_3d_loss_smp(conf, *case[:4], target, fs, dtype=torch.float64)
    crit = hl.RPN_3D_loss_smp(_smp_conf(conf))
    d = _run(crit, case, target)
    assert d["loss_t"].dtype == torch.float32 and d["loss_t"].dim() == 0 and d["loss_t"].is_cuda and d["loss_t"].grad_fn is not None
    assert np.array_equal(d["labels"], G["labels"]) and np.array_equal(d["labels"].astype(np.int64), r["labels"])
    want = RR.unpack_sampled(G, d["sampled"].shape)
    assert np.array_equal(d["sampled"], want), "sampled masks differ on %d anchors" % (d["sampled"] != want).sum()
    assert np.array_equal(d["sampled"], r["sampled"])
    assert d["targets"].tobytes() == r["targets"].tobytes()                     # passed through, bit for bit
    assert [RR.stat_key(s) for s in d["stats"]] == list(G["stat_names"]) == [RR.stat_key(s) for s in r["stats"]]
    fig = {"loss": abs(d["loss"] - r["loss"]) / abs(r["loss"]), "stat": 0.0}
    for a, b in zip(d["stats"], r["stats"]):
        assert set(a) == {"name", "val", "format", "group"}
        fig["stat"] = max(fig["stat"], abs(a["val"] - b["val"]) / max(abs(b["val"]), 1e-30))
    for k in ("g_cls", "g_bbox_2d", "g_bbox_3d"):
        fig[k] = RR.rel(d[k], r[k])
    fig["loss_vs_reference_f32"] = abs(d["loss"] - float(G["loss"])) / abs(float(G["loss"]))
    print("smp device vs float64 restatement %s: %s" % (name, fig))
    _log("rpn_loss_smp_" + name, fig)
    for k, bound in RR.DEVICE_BOUNDS.items():
        assert fig[k] <= bound, (k, fig[k], bound)


def _full_call(conf, case):
    dev = _dev()
    cls, prob, b2, b3, imobjs, fs = case
    crit = hl.RPN_3D_loss(conf)
    loss, _ = crit(cls.to(dev), prob.to(dev), b2.to(dev), b3.to(dev), imobjs, fs)
    return crit, _bits(crit, loss)


def _same_bits(got, want, what, keys=("loss", "sampled", "g_cls", "g_bbox_2d", "g_bbox_3d", "labels", "targets", "scores", "stats")):
    for k in keys:
        assert got[k] == want[k], "%s: %s differs from RPN_3D_loss" % (what, k)


def _dict_from_last(crit_full, table):
    """The target dict from what an RPN_3D_loss call left in crit.last: int16 labels, the packed targets split."""
    t = crit_full.last["targets"]
    any_val = torch.from_numpy((table[:, 0, 0] > 0).astype(np.int32)).to(t.device)
    return dict(labels=crit_full.last["labels"], bbox_2d=t[..., :4].contiguous(), bbox_3d=t[..., 4:].contiguous(), meta=dict(any_val=any_val))


@pytest.mark.parametrize("name", RR.GOLDEN_CASES)
def test_bit_equality_with_rpn_3d_loss(name):
    """Fed rpn_precompute_targets(...), and separately the labels / targets of an RPN_3D_loss call: loss, sampled, the three
    gradients (and labels, targets, scores, the stat block) are bitwise those of RPN_3D_loss on the same inputs."""
    conf, case = RR.golden_case(np.load(os.path.join(GOLDEN, "rpn_loss_%s.npz" % name)))
    crit_full, want = _full_call(conf, case)
    pre, table = _precompute(conf, case[4], case[5])
    crit = hl.RPN_3D_loss_smp(_smp_conf(conf))
    _same_bits(_run(crit, case, pre)["bits"], want, name + " / precomputed")
    _same_bits(_run(crit, case, _dict_from_last(crit_full, table))["bits"], want, name + " / crit.last")


@pytest.mark.parametrize("name", ("shipped", "emptyimg", "odd"))
def test_precompute_targets_equal_rpn_targets(name):
    conf, case = SR.golden_case(name)
    cls, prob, _b2, _b3, imobjs, fs = case
    pre, table = _precompute(conf, imobjs, fs)
    dev = _dev()
    anchors = torch.from_numpy(np.asarray(conf.anchors, dtype=np.float64)).to(dev)
    labels, gidx, targets, _scores = ops.rpn_targets(cls.to(dev), prob.to(dev), anchors, _vec(conf), table, fs)
    assert pre["labels"].dtype == pre["gt_index"].dtype == torch.int16 and pre["meta"]["any_val"].dtype == torch.int32
    assert torch.equal(pre["labels"], labels) and torch.equal(pre["gt_index"], gidx)
    assert pre["bbox_2d"].cpu().numpy().tobytes() == targets[..., :4].contiguous().cpu().numpy().tobytes()
    assert pre["bbox_3d"].cpu().numpy().tobytes() == targets[..., 4:].contiguous().cpu().numpy().tobytes()
    assert pre["meta"]["any_val"].cpu().tolist() == [int(v > 0) for v in table[:, 0, 0]]
    # and the loader's dict: what _targets stores, row by row ((0 - mean) / std where a row is not fg)
    host = SR.make_target(conf, imobjs, fs)
    assert np.array_equal(pre["labels"].cpu().numpy().astype(np.int64), host["labels"].numpy())
    t = np.concatenate([pre["bbox_2d"].cpu().numpy(), pre["bbox_3d"].cpu().numpy()], axis=2).astype(np.float64)
    want = np.concatenate([host["bbox_2d"].numpy(), host["bbox_3d"].numpy()], axis=2)
    assert (np.abs(t - want) <= RR.target_tolerance(want, conf)).all()
    nonfg = host["labels_fg"].numpy() == 0
    assert np.array_equal(t[nonfg], want[nonfg].astype(np.float64))


def _gt(cls, box, z=20.0):
    x, y, w, h = box
    return RR.Conf(cls=cls, ign=False, visibility=1.0, bbox_full=np.array([x, y, w, h], dtype=np.float64),
                   bbox_3d=[x + w / 2, y + h / 2, z, 1.6, 1.5, 3.9, 0.3, 0.0, 1.0, z])


def _sliver_case():
    """40x72, B = 3: the middle image has ONE valid gt, three pixels wide -- below best_thresh for every anchor, no fg and no
    ignored row (the reference's branch lib/loss/rpn_3d.py:961-987); the outer images are those of the `odd` golden case."""
    conf, (cls, prob, b2, b3, imobjs, fs) = SR.golden_case("odd")
    sliver = RR.Conf(gts=[_gt("Car", (30.0, 5.0, 3.0, 30.0))], p2=np.eye(4), p2_inv=np.eye(4), scale_factor=1.0)
    return conf, (cls, prob, b2, b3, [imobjs[0], sliver, imobjs[2]], fs)


def test_valid_gt_without_fg_or_ignored_row_equals_rpn_3d_loss():
    conf, case = _sliver_case()
    host = SR.make_target(conf, case[4], case[5])
    assert host["meta"]["any_val"].tolist() == [1, 1, 1] and not host["labels"][1].any()          # valid gt, every row bg
    crit_full, want = _full_call(conf, case)
    assert crit_full.last["sampled"][1].any()
    pre, _table = _precompute(conf, case[4], case[5])
    crit = hl.RPN_3D_loss_smp(_smp_conf(conf))
    _same_bits(_run(crit, case, pre)["bits"], want, "sliver / precomputed")
    got = _run(crit, case, host)["bits"]
    _same_bits(got, want, "sliver / host dict", keys=("loss", "sampled", "g_cls", "g_bbox_2d", "g_bbox_3d", "labels", "scores", "stats"))


def test_label_forms_give_identical_bits():
    """int64 / int16, host / device, and int64 labels at an address that is no multiple of 16 (the one-label-per-load path)."""
    conf, case = SR.golden_case("odd")
    fs, dev = case[5], _dev()
    host = SR.make_target(conf, case[4], fs)
    crit = hl.RPN_3D_loss_smp(_smp_conf(conf))
    want = _run(crit, case, host)["bits"]
    on_dev = dict(labels=host["labels"].to(dev), bbox_2d=host["bbox_2d"].to(dev), bbox_3d=host["bbox_3d"].to(dev),
                  meta=dict(any_val=host["meta"]["any_val"].to(dev)))
    assert _run(crit, case, on_dev)["bits"] == want
    assert _run(crit, case, dict(on_dev, labels=host["labels"].to(torch.int16)))["bits"] == want
    assert _run(crit, case, dict(on_dev, labels=on_dev["labels"].to(torch.int16), meta=dict(any_val=[1, 0, 1])))["bits"] == want
    B, R = host["labels"].shape
    for dtype in (torch.int64, torch.int16):
        store = torch.zeros(B * R + 1, dtype=dtype, device=dev)
        store[1:] = host["labels"].to(dev).to(dtype).reshape(-1)
        shifted = store[1:].view(B, R)
        assert shifted.is_contiguous() and shifted.data_ptr() % (2 * shifted.element_size()) != 0
        assert _run(crit, case, dict(on_dev, labels=shifted))["bits"] == want, dtype
    pinned = dict(host, labels=host["labels"].pin_memory())
    assert _run(crit, case, pinned)["bits"] == want


@pytest.mark.parametrize("bad", ("C", -1, 2999))
def test_a_label_outside_the_allowed_set_raises_and_changes_nothing_else(bad, monkeypatch):
    """The row is counted and treated as ignored: with every allocation NaN-poisoned, all outputs are those of the same call
    with that row labelled 3000."""
    conf, case = SR.golden_case("odd")
    fs, dev = case[5], _dev()
    host = SR.make_target(conf, case[4], fs)
    ins = [t.to(dev) for t in case[:4]]
    crit = hl.RPN_3D_loss_smp(_smp_conf(conf))
    value = crit.num_classes if bad == "C" else bad
    rows = [(0, 7), (2, 1619), (1, 800)]                # an image's first workgroup, the very last row, the image without a valid gt
    labels_bad, labels_ign = host["labels"].clone(), host["labels"].clone()
    for b, r in rows:
        labels_bad[b, r], labels_ign[b, r] = value, RR.IGN_FLAG
    loss, _ = crit(*ins, dict(host, labels=labels_ign), fs)
    want = _bits(crit, loss)
    with poison.poisoned_allocations("nan", monkeypatch=monkeypatch) as st:
        with pytest.raises(RuntimeError, match="%d labels are outside" % len(rows)):
            crit(*ins, dict(host, labels=labels_bad), fs)
    assert st.from_file("m3dssd_amd/host/loss.py") >= 9
    d = crit.last
    assert float(d["stats"][hl.SMP_STAT_BAD_LABELS]) == len(rows)
    for k, t in (("sampled", d["sampled"]), ("labels", d["labels"]), ("targets", d["targets"]), ("scores", d["scores"]),
                 ("g_cls", d["grads"][0]), ("g_bbox_2d", d["grads"][1]), ("g_bbox_3d", d["grads"][2])):
        assert t.cpu().numpy().tobytes() == want[k], k
    assert d["stats"].cpu().numpy()[:len(hl.STAT_NAMES)].tobytes() == want["stats"]          # (slot 0 is the loss)


def test_bad_targets_are_rejected_with_a_message():
    conf, case = SR.golden_case("odd")
    fs, dev = case[5], _dev()
    host = SR.make_target(conf, case[4], fs)
    ins = [t.to(dev) for t in case[:4]]
    crit = hl.RPN_3D_loss_smp(_smp_conf(conf))
    B, R = host["labels"].shape
    for change, msg in ((dict(labels=host["labels"][:, :-1]), r"target\['labels'\] has shape"),
                        (dict(labels=host["labels"].to(torch.int32)), "int64 or torch.int16"),
                        (dict(bbox_2d=host["bbox_3d"]), r"target\['bbox_2d'\] has shape"),
                        (dict(bbox_3d=host["bbox_3d"].double()), "float32"),
                        (dict(bbox_3d=host["bbox_3d"].transpose(0, 1).contiguous().transpose(0, 1)), "contiguous"),
                        (dict(labels=host["labels"].t().contiguous().t()), "contiguous"),
                        (dict(labels_fg=host["labels_fg"][:1]), r"target\['labels_fg'\] has shape"),
                        (dict(meta=dict(any_val=host["meta"]["any_val"][:2])), "any_val"),
                        (dict(meta=dict(any_val=host["meta"]["any_val"], rois=host["meta"]["rois"][:, :-1])), "rois"),
                        (dict(meta=dict()), "any_val")):
        with pytest.raises(RuntimeError, match=msg):
            crit(*ins, dict(host, **change), fs)
    with pytest.raises(RuntimeError, match="no 'bbox_3d'"):
        crit(*ins, {k: v for k, v in host.items() if k != "bbox_3d"}, fs)
    with pytest.raises(RuntimeError, match="dict"):
        crit(*ins, case[4], fs)                                     # a list of imobjs: RPN_3D_loss' argument
    with pytest.raises(RuntimeError, match="bbox_2d has shape"):
        crit(ins[0], ins[1], ins[3], ins[3], host, fs)
    with pytest.raises(NotImplementedError):
        crit(ins[0].cpu(), ins[1], ins[2], ins[3], host, fs)
    vec, L = _vec(conf), hl._hip.lib()
    with pytest.raises(RuntimeError, match="label_bytes"):          # refused before any pointer is looked at
        hl._hip.check(L.m3d_rpn_loss_smp(1, 36, fs[0], fs[1], vec.ctypes.data, hl.CONF_COUNT, B, 1, 4, 1, 1, 1, 1, 1, 1, 1, 4,
                                         1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1 << 30, None))


def test_ops_layer_grad_output_scaling_and_five_identical_calls():
    conf, case = SR.golden_case("odd")
    cls, prob, b2, b3, imobjs, fs = case
    dev = _dev()
    host = SR.make_target(conf, imobjs, fs)
    anchors = torch.from_numpy(np.asarray(conf.anchors, dtype=np.float64)).to(dev)
    first = None
    for i in range(5):
        ins = [t.to(dev).requires_grad_(True) for t in (cls, b2, b3)]
        loss, stats, det = ops.rpn_loss_smp(ins[0], prob.to(dev), ins[1], ins[2], host, anchors, _vec(conf), fs, return_details=True)
        assert stats.shape == (hl.SMP_STAT_COUNT,) and stats.dtype == torch.float64 and not stats.requires_grad
        assert float(stats[hl.SMP_STAT_BAD_LABELS]) == 0.0
        (loss * 3.0).backward()
        for t, g in zip(ins, det["grads"]):
            assert torch.equal(t.grad, g * 3.0)
        got = [loss.detach().cpu().numpy().tobytes(), stats.cpu().numpy().tobytes()] + [t.grad.cpu().numpy().tobytes() for t in ins] + \
              [det[k].cpu().numpy().tobytes() for k in ("labels", "targets", "scores", "sampled")]
        if first is None:
            first = got
        assert got == first, "call %d differs from call 0" % i


def test_one_training_step_equals_the_step_with_rpn_3d_loss():
    """net.train(), net(x), RPN_3D_loss_smp on rpn_precompute_targets (made ahead of the forward), backward, SGD step -- at
    64x128, the smallest crop of the training tests; the loss is that of RPN_3D_loss on the same forward, bit for bit."""
    from lib.loss.rpn_3d import RPN_3D_loss, RPN_3D_loss_smp
    from m3dssd_amd import synth
    from model.M3d_inference_align import build
    crop, B = (64, 128), 2
    conf = RR.loss_conf(crop, 0, device="cuda:0")
    conf.update(synth.config_flags("anab_fullalign"))
    conf.batch_size = B
    net = build(conf, "train")
    net.load_state_dict(synth.synth_state_dict(0, back_bone="dla34", **synth.config_flags("anab_fullalign")), strict=True)
    net = net.to(_dev()).train()
    x = synth.synth_frames(B, crop, 1234).to(_dev())
    imobjs = RR.make_case(31, crop, B, 6)[4]
    fs = [crop[0] // 8, crop[1] // 8]
    target, table = _precompute(conf, imobjs, fs)
    assert table[:, 0, 0].min() > 0 and bool(((target["labels"] > 0) & (target["labels"] != RR.IGN_FLAG)).any())
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9)
    cls, prob, b2, b3, fs_net = net(x)
    assert [int(fs_net[0]), int(fs_net[1])] == fs
    with torch.no_grad():
        want, _ = RPN_3D_loss(conf)(cls, prob, b2, b3, imobjs, fs_net)
    loss, stats = RPN_3D_loss_smp(conf)(cls, prob, b2, b3, target, fs_net)
    assert torch.isfinite(loss) and loss.detach().cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert [RR.stat_key(s) for s in stats][-1] == "loss_ttloss"
    before = [p.detach().clone() for p in net.parameters()]
    opt.zero_grad()
    loss.backward()
    opt.step()
    assert any(not torch.equal(a, b) for a, b in zip(before, net.parameters()))
