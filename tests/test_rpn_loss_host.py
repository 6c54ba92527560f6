"""CPU checks of RPN_3D_loss: the yardstick of the GPU tests (tests/rpn_loss_ref.py) is pinned against the reference's own
numbers (tests/golden/rpn_loss_*.npz, tools/gen_golden_rpn_loss.py), its float32-vs-float64 error -- the source of the device
bounds -- is measured, and the host layer is checked: shims, constructor fields, refusals, the C ABI's new names, gt packing."""
import os
import re

import numpy as np
import pytest
import torch

from m3dssd_amd import _hip
from m3dssd_amd.host import loss as hl

import rpn_loss_ref as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return np.load(os.path.join(GOLDEN, "rpn_loss_%s.npz" % name))


@pytest.mark.parametrize("name", RR.GOLDEN_CASES)
def test_restatement_matches_the_reference(name):
    """Labels, sampled masks and fg targets of EVERY anchor equal the reference's; loss, stats and gradients within REF32_BOUND
    (measured 0.0: bit-identical on the build machine)."""
    G = _load(name)
    conf, case = RR.golden_case(G)
    o = RR.rpn_3d_loss(conf, *case, dtype=torch.float32)
    assert float(G["threshold_gap"]) > 1e-9
    assert np.array_equal(o["labels"], G["labels"].astype(np.int64))
    assert np.array_equal(o["sampled"], RR.unpack_sampled(G, o["sampled"].shape))
    fr = G["fg_rows"]
    assert np.array_equal(np.argwhere(o["gt_index"] >= 0), fr)
    assert np.array_equal(o["targets"][fr[:, 0], fr[:, 1]], G["fg_targets"])
    worst = abs(o["loss"] - float(G["loss"])) / abs(float(G["loss"]))
    assert [RR.stat_key(s) for s in o["stats"]] == list(G["stat_names"])
    for s, v in zip(o["stats"], G["stat_vals"]):
        worst = max(worst, abs(s["val"] - v) / max(abs(v), 1e-30))
    for k in ("g_cls", "g_bbox_2d", "g_bbox_3d"):
        cs, sm = RR.grad_summary(o[k])
        worst = max(worst, RR.rel(sm, G[k + "_sample"]), RR.rel(cs, G[k + "_sum"]))
    print("restatement(float32) vs reference %s: %.2e" % (name, worst))
    assert worst <= RR.REF32_BOUND


def _f32_vs_f64(conf, case):
    o32 = RR.rpn_3d_loss(conf, *case, dtype=torch.float32)
    o64 = RR.rpn_3d_loss(conf, *case, dtype=torch.float64)
    assert np.array_equal(o32["labels"], o64["labels"]) and np.array_equal(o32["sampled"], o64["sampled"])
    assert np.array_equal(o32["targets"], o64["targets"])                       # dtype-independent: target_tolerance's premise
    out = {"loss": abs(o32["loss"] - o64["loss"]) / abs(o64["loss"]), "stat": 0.0}
    for a, b in zip(o32["stats"], o64["stats"]):
        out["stat"] = max(out["stat"], abs(a["val"] - b["val"]) / max(abs(b["val"]), 1e-30))
    for k in ("g_cls", "g_bbox_2d", "g_bbox_3d"):
        out[k] = RR.rel(o32[k], o64[k])
    return out, o64


@pytest.mark.parametrize("name", RR.GOLDEN_CASES + tuple(RR.FULL_CASES))
def test_device_bounds_come_from_the_float32_error_of_the_restatement(name):
    """DEVICE_BOUNDS are 4 x the float32-vs-float64 error measured here; this run's own measurement must stay inside them (the
    factor is the room another torch build's summation order gets)."""
    if name in RR.FULL_CASES:
        seed, B, ng = RR.FULL_CASES[name]
        conf, case = RR.loss_conf((384, 1280), 0), RR.make_case(seed, (384, 1280), B, ng)
    else:
        conf, case = RR.golden_case(_load(name))
    err, o64 = _f32_vs_f64(conf, case)
    print("float32 vs float64 restatement %s: %s" % (name, ", ".join("%s %.2e" % kv for kv in err.items())))
    if name in RR.FULL_CASES:          # the generator's uniqueness checks, on the cases that have no golden file
        assert RR.nearest_threshold_gap(o64["overlaps"], conf) > 1e-9
        assert all(lo != hi for lo, hi in o64["margins"])
    for k, v in err.items():
        bound = RR.G2D_CASE_BOUNDS.get(name, RR.DEVICE_BOUNDS[k]) if k == "g_bbox_2d" else RR.DEVICE_BOUNDS[k]
        assert v <= bound, (k, v, bound)


def test_shims_import_and_constructor_fields():
    import lib.loss.rpn_3d as shim
    from lib.loss.rpn_3d import RPN_3D_loss
    assert shim.RPN_3D_loss is hl.RPN_3D_loss
    conf = RR.loss_conf()
    crit = RPN_3D_loss(conf)
    assert isinstance(crit, torch.nn.Module)
    for f in ("num_classes", "num_anchors", "anchors", "bbox_means", "bbox_stds", "feat_stride", "fg_fraction", "box_samples",
              "ign_thresh", "nms_thres", "fg_thresh", "bg_thresh_lo", "bg_thresh_hi", "best_thresh", "hard_negatives", "focal_loss",
              "crop_size", "cls_2d_lambda", "iou_2d_lambda", "bbox_2d_lambda", "bbox_3d_lambda", "bbox_3d_proj_lambda", "lbls",
              "ilbls", "min_gt_vis", "min_gt_h", "max_gt_h", "device"):
        assert hasattr(crit, f), f
    assert crit.num_classes == 4 and crit.num_anchors == 36 and crit.box_samples == 0.2


def test_cpu_tensors_and_unsupported_settings_raise():
    from m3dssd_amd.host import ops
    conf = RR.loss_conf()
    cls, prob, b2, b3, imobjs, fs = RR.make_case(11)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        hl.RPN_3D_loss(conf)(cls, prob, b2, b3, imobjs, fs)
    vec = hl.pack_conf(conf.bbox_means, conf.bbox_stds, 0.5, 0.5, 0, 0.5, 0.35, 0.2, 0.2, 0, 1, 1, 0, 1, 8)
    table = hl.pack_gts(imobjs, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
    with pytest.raises(NotImplementedError):
        ops.rpn_loss(cls, prob, b2, b3, conf.anchors, vec, table, fs)
    with pytest.raises(NotImplementedError):
        ops.rpn_targets(cls, prob, conf.anchors, vec, table, fs)
    with pytest.raises(NotImplementedError, match="bbox_3d_proj_lambda"):
        hl.RPN_3D_loss(RR.loss_conf(bbox_3d_proj_lambda=1.0))
    with pytest.raises(NotImplementedError, match="random sampling"):
        hl.RPN_3D_loss(RR.loss_conf(hard_negatives=False))
    hl.RPN_3D_loss(RR.loss_conf(hard_negatives=False, box_samples=float("inf")))       # nothing is drawn: supported
    with pytest.raises(NotImplementedError, match="RPN_3D_loss_smp"):
        hl.RPN_3D_loss_smp(conf)
    crit = hl.RPN_3D_loss(conf)
    crit.bbox_3d_proj_lambda = 0.5                                                     # changed after construction
    with pytest.raises(NotImplementedError, match="bbox_3d_proj_lambda"):
        crit(cls, prob, b2, b3, imobjs, fs)
    with pytest.raises(ValueError, match="fg_fraction=None"):
        hl.pack_conf(conf.bbox_means, conf.bbox_stds, 0.5, 0.5, 0, 0.5, 0.35, 0.2, None, 0, 1, 1, 0, 1, 8)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(_hip.HEADER).read(), flags=re.S)


def test_header_signature_table_and_library_agree_on_the_new_names():
    L, hdr = _hip.lib(), _header()
    for name, nargs in (("m3d_rpn_loss_workspace_bytes", 2), ("m3d_rpn_targets", 19), ("m3d_rpn_loss", 25)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
        assert hasattr(L, name) and name in _hip.SIGNATURES
        assert len(_hip.SIGNATURES[name][1]) == nargs
    assert L.m3d_abi_version() == 5
    consts = dict(re.findall(r"\b(M3D_RPN_[A-Z0-9_]+)\s*=?\s+(\d+)", hdr))
    assert int(consts["M3D_RPN_MAX_GT"]) == hl.MAX_GT >= 64
    assert int(consts["M3D_RPN_GT_COLS"]) == hl.GT_COLS
    assert int(consts["M3D_RPN_CONF_COUNT"]) == hl.CONF_COUNT
    assert int(consts["M3D_RPN_STAT_COUNT"]) == len(hl.STAT_NAMES)
    for i, n in enumerate(hl.STAT_NAMES):
        assert int(consts["M3D_RPN_STAT_" + n.upper()]) == i
    src = open(os.path.join(_hip.CSRC, "Makefile")).read()
    assert "rpn_loss.hip" in src.split("SRCS")[1].split("\n")[0]


def test_workspace_rule_answers_without_a_gpu():
    f = _hip.lib().m3d_rpn_loss_workspace_bytes
    assert f(0, 100) == -1 and f(2, 0) == -1
    sizes = [f(b, 276480) for b in (1, 2, 4, 8)]
    assert all(s > 0 for s in sizes) and all(b > a for a, b in zip(sizes, sizes[1:]))


@pytest.mark.parametrize("name", ("shipped", "emptyimg"))
def test_gt_packing_matches_the_reference_tables(name):
    """determine_ignores, class lookup and XYWH -> corners of the product against the table the reference's helpers gave."""
    G = _load(name)
    conf, case = RR.golden_case(G)
    table = hl.pack_gts(case[4], conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
    assert table.dtype == np.float64 and np.array_equal(table, G["gt_table"])
    plain = [dict(gts=[dict(g) for g in im.gts], p2=im.p2, p2_inv=im.p2_inv, scale_factor=1.0) for im in case[4]]
    assert np.array_equal(hl.pack_gts(plain, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h), table)
    if name == "emptyimg":
        assert table[1, 0, 0] == 0 and table[1, 0, 1] > 0          # no valid gt, but ignore regions
    igns, rmvs = hl.determine_ignores(case[4][0].gts, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
    assert rmvs.tolist() == [g.cls == "Tram" for g in case[4][0].gts]
    assert igns.tolist() == [g.cls == "Van" or g.visibility < conf.min_gt_vis or g.bbox_full[3] < conf.min_gt_h for g in case[4][0].gts]
    stats = hl.stats_list(np.arange(16.0) + 1, 1, 0, 1, 1)
    assert [(d["group"], d["name"]) for d in stats] == [("acc", "fg"), ("acc", "bg"), ("loss", "cls"), ("loss", "bbox_3d"),
                                                        ("misc", "z"), ("misc", "ry"), ("acc", "iou"), ("loss", "iou")]
