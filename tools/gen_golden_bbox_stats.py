#!/usr/bin/env python
"""Generate tests/golden/bbox_stats.npz by running the REFERENCE's own generate_anchors (lib/rpn_util.py:25-164),
compute_bbox_stats (lib/rpn_util.py:732-889) and, per image, compute_targets (lib/rpn_util.py:430-532) on a synthetic imdb.

Build-container only, like tools/gen_golden_rpn_loss_smp.py, whose import stubs (tools/gen_golden.py) it reuses.

The imdb: test_scale = [32, 1280] at stride 8 -- a map 4 rows high and about 160 wide, so that roi coordinates reach 1 280,
where a float32 roi differs from the float64 one compute_bbox_stats uses.  4 scales x 3 ratios = 12 anchors (R about 7.7 k).
Eight images with imH 30-32 and four different feature widths (155, 156, 159, 160); seven ground truths per image whose shapes cycle over the
anchors' (the reference raises on an unused anchor); the classes include an ignore class (Van) and an unlisted one (Tram); one
low-visibility box; image 4 has no gts; every ground truth of image 6 is ignored.

Stored (data only): the imdb as plain arrays, the conf scalars, the reference's anchors, bbox_means, bbox_stds, and per image
n_fg and, per column over the fg rows, sum t, sum |t|, max |t| of the reference's float32 transforms (added in longdouble, cast
to float64).

The generator FAILS unless the reference finishes, tests/bbox_stats_ref.py restates it bit for bit, and no overlap lies within
1e-9 of fg_thresh, bg_thresh_hi, best_thresh, ign_thresh or the 0.2 of generate_anchors: a last-bit difference cannot flip a label.

Run:  python tools/gen_golden_bbox_stats.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

SIZES = [(32, 1280), (31, 1225), (30, 1165), (32, 1275), (31, 1230), (30, 1160), (32, 1280), (31, 1225)]      # (imH, imW)
N_GT = 7
EMPTY_IMAGE, IGNORED_IMAGE = 4, 6
SEED = 3


def make_conf(EasyDict):
    conf = EasyDict()
    conf.feat_stride = 8
    conf.test_scale = [32, 1280]
    conf.min_gt_h, conf.max_gt_h = 4.0, 24.0
    conf.min_gt_vis = 0.65
    conf.lbls, conf.ilbls = ['Car', 'Pedestrian', 'Cyclist'], ['Van', 'ignore']
    conf.has_3d, conf.cluster_anchors = True, 0
    base = (24.0 / 6.0) ** (1 / 3)
    conf.anchor_scales = np.array([6.0 * (base ** i) for i in range(4)])
    conf.anchor_ratios = np.array([0.5, 1.0, 1.5])
    conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo, conf.bg_thresh_hi, conf.best_thresh = 0.5, 0.5, 0, 0.5, 0.35
    conf.anchors = conf.bbox_means = conf.bbox_stds = None
    return conf


def make_imdb(conf, EasyDict):
    rng = np.random.RandomState(SEED)
    imdb, n_anchor = [], len(conf.anchor_scales) * len(conf.anchor_ratios)
    for i, (h, w) in enumerate(SIZES):
        im = EasyDict(imH=h, imW=w, scale=1, gts=[])
        for g in range(0 if i == EMPTY_IMAGE else N_GT):
            a = (i * N_GT + g) % n_anchor
            sh = conf.anchor_scales[a // 3] * rng.uniform(0.9, 1.1) * h / conf.test_scale[0]
            sw = sh * conf.anchor_ratios[a % 3] * rng.uniform(0.9, 1.1)
            x, y = rng.uniform(0, w - sw), rng.uniform(0, max(h - sh, 1))
            cls = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Tram'][rng.randint(0, 5) if g > 4 else g % 3]
            if i == IGNORED_IMAGE:
                cls = ['Van', 'Tram', 'Car'][g % 3]
            gt = EasyDict(bbox_full=np.array([x, y, sw, sh]), cls=cls, ign=bool((g == 6 and i % 2) or (i == IGNORED_IMAGE and g % 3 == 2)),
                          visibility=0.3 if (i == 1 and g == 3) else 1.0)
            gt.bbox_3d = np.array([x + sw / 2 + rng.normal(0, 1), y + sh / 2 + rng.normal(0, 1), rng.uniform(5, 60), rng.uniform(0.5, 2),
                                   rng.uniform(1.2, 2), rng.uniform(0.8, 4.5), rng.uniform(-3.1, 3.1)])
            im.gts.append(gt)
        imdb.append(im)
    return imdb


def main():
    gen_golden._install_stubs()
    sys.path.append(os.path.join(gen_golden.REPO, "tests"))
    from easydict import EasyDict
    import bbox_stats_ref as BR
    import lib.rpn_util as ref_rpn
    import lib.core as ref_core
    assert ref_rpn.__file__.startswith(gen_golden.REF)

    conf = make_conf(EasyDict)
    imdb = make_imdb(conf, EasyDict)
    ref_rpn.generate_anchors(conf, imdb, None)
    ref_rpn.compute_bbox_stats(conf, imdb, None)
    anchors, means, stds = conf.anchors, conf.bbox_means, conf.bbox_stds
    assert anchors.dtype == np.float64 and anchors.shape == (12, 9) and means.shape == stds.shape == (1, 11) and means.dtype == np.float64
    assert np.isfinite(means).all() and np.isfinite(stds).all() and (stds > 0).all()

    # the restatement, from the arrays the fixture stores
    arrays = dict(BR.imdb_to_arrays(imdb), **BR.conf_to_arrays(conf))
    conf2, imdb2 = BR.conf_from_arrays(arrays), BR.imdb_from_arrays(arrays)
    anchors2, anchor_ols = BR.generate_anchors(conf2, imdb2)
    assert anchors2.tobytes() == anchors.tobytes(), "tests/bbox_stats_ref.py: generate_anchors differs from the reference"
    conf2.anchors = anchors2
    means2, stds2 = BR.compute_bbox_stats(conf2, imdb2)
    assert means2.tobytes() == means.tobytes() and stds2.tobytes() == stds.tobytes(), "tests/bbox_stats_ref.py: compute_bbox_stats differs"
    gap = float(np.abs(anchor_ols - BR.ANCHOR_IOU).min())

    # per image: the reference's compute_targets, as compute_bbox_stats calls it
    per, tables, feat_sizes = [], [], []
    for im, im2 in zip(imdb, imdb2):
        sf = im.scale * conf.test_scale[0] / im.imH
        fs = ref_rpn.calc_output_size(np.array([im.imH, im.imW]) * sf, conf.feat_stride)
        feat_sizes.append([int(fs[0]), int(fs[1])])
        if len(im.gts) == 0:
            per.append(BR.image_sums(None))
            continue
        rois = ref_rpn.locate_anchors(conf.anchors, fs, conf.feat_stride)
        assert rois.dtype == np.float64
        igns, rmvs = ref_rpn.determine_ignores(im.gts, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h, np.inf, sf)
        gts_all = ref_rpn.bbXYWH2Coords(np.array([gt.bbox_full * sf for gt in im.gts]))
        keep, keep_i = (rmvs == False) & (igns == False), (rmvs == False) & (igns == True)      # noqa: E712
        gts_val, gts_ign = gts_all[keep, :], gts_all[keep_i, :]
        box_lbls = np.array([ref_rpn.clsName2Ind(conf.lbls, c) for c in np.array([gt.cls for gt in im.gts])[keep]])
        gts_3d = np.array([gt.bbox_3d for gt in im.gts])[keep, :]
        for gtind in range(gts_3d.shape[0]):
            gts_3d[gtind, 0:2] *= sf
        transforms, ols, _ = ref_rpn.compute_targets(gts_val, gts_ign, box_lbls, rois, conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo,
                                                     conf.bg_thresh_hi, conf.best_thresh, gts_3d=gts_3d, anchors=conf.anchors,
                                                     tracker=rois[:, 4])
        assert transforms.dtype == np.float32 and transforms.shape[1] == 12
        t2 = BR.image_transforms(conf2, im2)
        assert t2[0].tobytes() == transforms.tobytes(), "tests/bbox_stats_ref.py: compute_targets differs from the reference"
        tables.append((ols, ref_core.iou_ign(rois, gts_ign) if gts_ign.shape[0] else None))
        per.append(BR.image_sums(transforms))
    gap = min(gap, BR.nearest_threshold_gap(tables, conf))
    assert gap > 1e-9, "an overlap lies %.3e from a threshold" % gap
    n_fg = np.array([p[0] for p in per], dtype=np.int64)
    assert n_fg[EMPTY_IMAGE] == 0 and n_fg[IGNORED_IMAGE] == 0 and (np.delete(n_fg, [EMPTY_IMAGE, IGNORED_IMAGE]) > 0).all(), n_fg
    assert len({tuple(f) for f in feat_sizes}) >= 3

    out = dict(arrays, anchors=anchors, bbox_means=means, bbox_stds=stds, feat_sizes=np.array(feat_sizes, dtype=np.int64), n_fg=n_fg,
               sum_t=np.stack([p[1] for p in per]), sum_abs_t=np.stack([p[2] for p in per]), max_abs_t=np.stack([p[3] for p in per]),
               threshold_gap=np.array(gap))
    path = os.path.join(gen_golden.OUT, "bbox_stats.npz")
    np.savez_compressed(path, **out)
    print("feat sizes %s, n_fg %s, nearest threshold %.2e, %d bytes" % (feat_sizes, n_fg.tolist(), gap, os.path.getsize(path)))
    print("means", means.round(4).tolist())
    print("stds ", stds.round(4).tolist())


if __name__ == "__main__":
    main()
