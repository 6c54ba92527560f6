"""CPU checks of RPN_3D_loss_smp: the yardstick of the GPU tests (tests/rpn_loss_smp_ref.py) is pinned against the reference's own
numbers (tests/golden/rpn_loss_smp_*.npz, tools/gen_golden_rpn_loss_smp.py), and the host layer is checked: the shim, the
constructor and its ``conf.device`` rule, refusals, the C ABI's new names."""
import os
import re

import numpy as np
import pytest
import torch

from m3dssd_amd import _hip
from m3dssd_amd.host import loss as hl

import rpn_loss_ref as RR
import rpn_loss_smp_ref as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", tuple(SR.GOLDEN_CASES))
def test_restatement_matches_the_reference(name):
    """Labels, any_val, sampled masks and fg targets of EVERY anchor equal the reference's; loss, stats and gradients within
    REF32_BOUND, the float32 bound test_rpn_loss_host.py uses for its restatement."""
    G = np.load(os.path.join(GOLDEN, "rpn_loss_smp_%s.npz" % name))
    conf, (cls, prob, b2, b3, imobjs, fs) = SR.golden_case(name)
    target = SR.make_target(conf, imobjs, fs)
    o = SR.rpn_3d_loss_smp(conf, cls, prob, b2, b3, target, fs, dtype=torch.float32)
    assert float(G["threshold_gap"]) > 1e-9
    assert np.array_equal(o["labels"], G["labels"].astype(np.int64))
    assert np.array_equal(target["meta"]["any_val"].numpy(), G["any_val"])
    assert np.array_equal(o["sampled"], RR.unpack_sampled(G, o["sampled"].shape))
    fr = G["fg_rows"]
    assert np.array_equal(np.argwhere((o["labels"] > 0) & (o["labels"] != RR.IGN_FLAG)), fr)
    assert np.array_equal(o["targets"][fr[:, 0], fr[:, 1]], G["fg_targets"])
    for k, t in (("labels_fg", o["labels"] > 0), ("labels_bg", o["labels"] == 0), ("labels_ign", o["labels"] == RR.IGN_FLAG)):
        want = (t & (o["labels"] != RR.IGN_FLAG)) if k == "labels_fg" else t
        assert np.array_equal(target[k].numpy().astype(bool), want), k
    worst = abs(o["loss"] - float(G["loss"])) / abs(float(G["loss"]))
    assert [RR.stat_key(s) for s in o["stats"]] == list(G["stat_names"])
    assert list(G["stat_names"])[-1] == "loss_ttloss" and "loss_bbox3d" in G["stat_names"] and "loss_bbox_2d" not in G["stat_names"]
    for s, v in zip(o["stats"], G["stat_vals"]):
        worst = max(worst, abs(s["val"] - v) / max(abs(v), 1e-30))
    for k in ("g_cls", "g_bbox_2d", "g_bbox_3d"):
        cs, sm = RR.grad_summary(o[k])
        worst = max(worst, RR.rel(sm, G[k + "_sample"]), RR.rel(cs, G[k + "_sum"]))
    print("smp restatement(float32) vs reference %s: %.2e" % (name, worst))
    assert worst <= RR.REF32_BOUND


FIELDS = ("num_classes", "num_anchors", "anchors", "bbox_means", "bbox_stds", "feat_stride", "fg_fraction", "box_samples", "ign_thresh",
          "nms_thres", "fg_thresh", "bg_thresh_lo", "bg_thresh_hi", "best_thresh", "hard_negatives", "focal_loss", "crop_size",
          "cls_2d_lambda", "iou_2d_lambda", "bbox_2d_lambda", "bbox_3d_lambda", "bbox_3d_proj_lambda", "lbls", "ilbls", "min_gt_vis",
          "min_gt_h", "max_gt_h", "device")


def test_constructs_for_a_rocm_device_without_a_gpu_and_carries_the_fields():
    crit = hl.RPN_3D_loss_smp(RR.loss_conf(device="cuda:0"))
    assert isinstance(crit, torch.nn.Module)
    for f in FIELDS:
        assert hasattr(crit, f), f
    assert crit.num_classes == 4 and crit.num_anchors == 36 and crit.box_samples == 0.2 and crit.device == "cuda:0"
    assert crit._anchors_dev is None and crit.last is None                     # nothing uploaded before the first forward
    hl.RPN_3D_loss_smp(RR.loss_conf(device=torch.device("cuda", 1)))
    hl.RPN_3D_loss_smp(RR.loss_conf(device="cuda:0", bbox_2d_lambda=1))           # supported here (NameError in the reference)


def test_the_shim_exports_the_same_class():
    import lib.loss.rpn_3d as shim
    from lib.loss.rpn_3d import RPN_3D_loss_smp
    assert shim.RPN_3D_loss_smp is hl.RPN_3D_loss_smp is RPN_3D_loss_smp


def test_host_tensors_and_unsupported_settings_raise():
    from m3dssd_amd.host import ops
    conf = RR.loss_conf(device="cuda:0")
    cls, prob, b2, b3, imobjs, fs = RR.make_case(11)
    target = SR.make_target(conf, imobjs, fs)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        hl.RPN_3D_loss_smp(conf)(cls, prob, b2, b3, target, fs)
    vec = hl.pack_conf(conf.bbox_means, conf.bbox_stds, 0.5, 0.5, 0, 0.5, 0.35, 0.2, 0.2, 0, 1, 1, 0, 1, 8)
    with pytest.raises(NotImplementedError):
        ops.rpn_loss_smp(cls, prob, b2, b3, target, conf.anchors, vec, fs)
    table = hl.pack_gts(imobjs, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ops.rpn_precompute_targets(conf.anchors, vec, table, fs, "cpu")
    with pytest.raises(NotImplementedError, match=r"RPN_3D_loss_smp: conf.device=cpu: no CPU fallback"):
        hl.RPN_3D_loss_smp(RR.loss_conf())
    with pytest.raises(NotImplementedError, match="RPN_3D_loss_smp: bbox_3d_proj_lambda"):
        hl.RPN_3D_loss_smp(RR.loss_conf(device="cuda:0", bbox_3d_proj_lambda=1.0))
    with pytest.raises(NotImplementedError, match="RPN_3D_loss_smp: random sampling"):
        hl.RPN_3D_loss_smp(RR.loss_conf(device="cuda:0", hard_negatives=False))
    hl.RPN_3D_loss_smp(RR.loss_conf(device="cuda:0", hard_negatives=False, box_samples=float("inf")))


def test_smp_stats_list_names_order_and_presence():
    key = lambda lst: [(d["group"], d["name"]) for d in lst]      # noqa: E731
    full = [("acc", "fg"), ("acc", "bg"), ("loss", "cls"), ("loss", "bbox3d"), ("misc", "z"), ("misc", "ry"), ("acc", "iou"),
            ("loss", "iou"), ("loss", "ttloss")]
    block = np.arange(17.0) + 1
    lst = hl.stats_list_smp(block, 1, 1, 1)
    assert key(lst) == full and lst[-1]["val"] == block[0] and all(set(d) == {"name", "val", "format", "group"} for d in lst)
    assert key(hl.stats_list_smp(block, 1, 0, 0)) == [k for k in full if k not in (("loss", "bbox3d"), ("loss", "iou"))]
    none = np.zeros(17)
    lst = hl.stats_list_smp(none, 1, 1, 1)                      # no fg, no bg, nothing sampled: 'bg' alone, NaN like the reference's
    assert key(lst) == [("acc", "bg")] and np.isnan(lst[0]["val"])
    assert hl.stats_list_smp(none, 0, 1, 1) == []


def test_header_signature_table_and_library_agree_on_the_new_names():
    L = _hip.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(_hip.HEADER).read(), flags=re.S)
    for name, nargs in (("m3d_rpn_precompute_targets", 17), ("m3d_rpn_loss_smp", 29)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
        assert hasattr(L, name) and name in _hip.SIGNATURES
        assert len(_hip.SIGNATURES[name][1]) == nargs
    assert L.m3d_abi_version() == 5                                 # additive: the number does not move
    consts = dict(re.findall(r"\b(M3D_RPN_[A-Z0-9_]+)\s*=?\s+(\d+)", hdr))
    assert int(consts["M3D_RPN_SMP_STAT_BAD_LABELS"]) == hl.SMP_STAT_BAD_LABELS == int(consts["M3D_RPN_STAT_COUNT"]) == len(hl.STAT_NAMES)
    assert int(consts["M3D_RPN_SMP_STAT_COUNT"]) == hl.SMP_STAT_COUNT == hl.SMP_STAT_BAD_LABELS + 1
