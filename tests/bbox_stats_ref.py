"""Yardstick of the dataset-statistics tests: a numpy restatement of the reference's ``generate_anchors``
(lib/rpn_util.py:25-164, the ``cluster_anchors = 0`` / ``has_3d`` branch) and ``compute_bbox_stats`` (lib/rpn_util.py:732-889)
with ``compute_targets`` (lib/rpn_util.py:430-532) on FLOAT64 rois, as compute_bbox_stats calls it -- tests/rpn_loss_ref.py
restates the same assignment on the float32 rois of the loss.

Test infrastructure only -- the product never imports it.  It imports nothing of m3dssd_amd.host.dataset_stats: every step is
restated here, expression by expression where a rounding depends on it (the float32 ``transforms`` array, the float32 column
sums of pass 1, the longdouble accumulators), so that anchors, means and stds equal the reference's bit for bit
(tests/golden/bbox_stats.npz, tools/gen_golden_bbox_stats.py).
"""
import numpy as np

from m3dssd_amd.config import Conf

CLASS_NAMES = ["Car", "Pedestrian", "Cyclist", "Van", "Tram"]          # the fixture stores the class of a gt as an index into this
CONF_SCALARS = ("feat_stride", "min_gt_h", "max_gt_h", "min_gt_vis", "fg_thresh", "ign_thresh", "bg_thresh_lo", "bg_thresh_hi",
                "best_thresh")
ANCHOR_IOU = 0.2          # generate_anchors gives a gt to its best anchor above this overlap


# ---- the fixture's imdb as plain arrays ------------------------------------------------------------------------------------
def imdb_to_arrays(imdb):
    gts = [gt for im in imdb for gt in im.gts]
    return dict(im_hw=np.array([[im.imH, im.imW] for im in imdb], dtype=np.int64),
                im_scale=np.array([im.scale for im in imdb], dtype=np.float64),
                im_n_gts=np.array([len(im.gts) for im in imdb], dtype=np.int64),
                gt_bbox_full=np.array([gt.bbox_full for gt in gts], dtype=np.float64).reshape(-1, 4),
                gt_bbox_3d=np.array([gt.bbox_3d for gt in gts], dtype=np.float64).reshape(-1, 7),
                gt_cls=np.array([CLASS_NAMES.index(gt.cls) for gt in gts], dtype=np.int64),
                gt_ign=np.array([bool(gt.ign) for gt in gts], dtype=bool),
                gt_visibility=np.array([gt.visibility for gt in gts], dtype=np.float64))


def imdb_from_arrays(G):
    imdb, k = [], 0
    for i in range(len(G["im_n_gts"])):
        gts = []
        for _ in range(int(G["im_n_gts"][i])):
            gts.append(Conf(bbox_full=np.array(G["gt_bbox_full"][k]), bbox_3d=np.array(G["gt_bbox_3d"][k]), cls=CLASS_NAMES[int(G["gt_cls"][k])],
                            ign=bool(G["gt_ign"][k]), visibility=float(G["gt_visibility"][k])))
            k += 1
        imdb.append(Conf(imH=int(G["im_hw"][i, 0]), imW=int(G["im_hw"][i, 1]), scale=float(G["im_scale"][i]), gts=gts))
    return imdb


def conf_to_arrays(conf):
    out = {"conf_" + k: np.array(float(conf[k])) for k in CONF_SCALARS}
    out.update(conf_test_scale=np.array(conf.test_scale, dtype=np.int64), conf_anchor_scales=np.array(conf.anchor_scales, dtype=np.float64),
               conf_anchor_ratios=np.array(conf.anchor_ratios, dtype=np.float64), conf_lbls=np.array(list(conf.lbls)),
               conf_ilbls=np.array(list(conf.ilbls)))
    return out


def conf_from_arrays(G):
    """The fixture's settings; anchors, bbox_means and bbox_stds unset."""
    conf = Conf({k: float(G["conf_" + k]) for k in CONF_SCALARS})
    conf.feat_stride = int(conf.feat_stride)
    conf.test_scale = [int(v) for v in G["conf_test_scale"]]
    conf.anchor_scales, conf.anchor_ratios = np.array(G["conf_anchor_scales"]), np.array(G["conf_anchor_ratios"])
    conf.lbls, conf.ilbls = [str(v) for v in G["conf_lbls"]], [str(v) for v in G["conf_ilbls"]]
    conf.has_3d, conf.cluster_anchors = True, 0
    conf.anchors = conf.bbox_means = conf.bbox_stds = None
    return conf


# ---- pieces of lib/rpn_util.py and lib/core.py -----------------------------------------------------------------------------
def anchor_center(w, h, stride):
    anchor = np.zeros([4], dtype=np.float32)
    anchor[0] = -w / 2 + (stride - 1) / 2
    anchor[1] = -h / 2 + (stride - 1) / 2
    anchor[2] = w / 2 + (stride - 1) / 2
    anchor[3] = h / 2 + (stride - 1) / 2
    return anchor


def determine_ignores(gts, lbls, ilbls, min_gt_vis, min_gt_h, max_gt_h, scale_factor):
    igns = np.zeros([len(gts)], dtype=bool)
    rmvs = np.zeros([len(gts)], dtype=bool)
    for i, gt in enumerate(gts):
        ign = bool(gt.ign)
        ign |= gt.visibility < min_gt_vis
        ign |= gt.bbox_full[3] * scale_factor < min_gt_h
        ign |= gt.bbox_full[3] * scale_factor > max_gt_h
        ign |= gt.cls in ilbls
        igns[i], rmvs[i] = ign, gt.cls not in (lbls + ilbls)
    return igns, rmvs


def xywh_to_corners(box):
    if box.shape[0] == 0:
        return np.empty([0, 4], dtype=float)
    box[:, 2] += box[:, 0] - 1
    box[:, 3] += box[:, 1] - 1
    return box


def locate_anchors(anchors, feat_size, stride):
    """float64 [(A*H*W), 5]: x1 y1 x2 y2 anchor index; row = (a*H + h)*W + w (lib/rpn_util.py:1329-1398, numpy branch)."""
    sx = np.array(range(0, feat_size[1], 1)) * float(stride)
    sy = np.array(range(0, feat_size[0], 1)) * float(stride)
    sx, sy = np.meshgrid(sx, sy)
    A = anchors.shape[0]
    cols = [sx[None] + anchors[:, 0][:, None, None], sy[None] + anchors[:, 1][:, None, None],
            sx[None] + anchors[:, 2][:, None, None], sy[None] + anchors[:, 3][:, None, None],
            np.zeros((1,) + sx.shape) + np.arange(A, dtype=float)[:, None, None]]
    return np.concatenate([c.reshape(-1, 1) for c in cols], 1)


def iou(box_a, box_b, ign=False):
    """[M, N] float64 of lib/core.py: iou (341-380) or iou_ign (402-434), 'combinations' on numpy arrays."""
    mx = np.minimum(box_a[:, None, 2:4], box_b[None, :, 2:4])
    mn = np.maximum(box_a[:, None, 0:2], box_b[None, :, 0:2])
    d = np.clip(mx - mn, a_min=0, a_max=None)
    inter = d[:, :, 0] * d[:, :, 1]
    area_a = (box_a[:, 2] - box_a[:, 0]) * (box_a[:, 3] - box_a[:, 1])
    area_b = (box_b[:, 2] - box_b[:, 0]) * (box_b[:, 3] - box_b[:, 1])
    if ign:
        return inter / (area_a[:, None] + area_b[None, :] * 0 - inter * 0)
    return inter / (area_a[:, None] + area_b[None, :] - inter)


# ---- generate_anchors ------------------------------------------------------------------------------------------------------
def normalized_gts(conf, imdb):
    rows = []
    for im in imdb:
        if len(im.gts) == 0:
            continue
        scale = im.scale * conf.test_scale[0] / im.imH
        igns, rmvs = determine_ignores(im.gts, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h, np.inf, scale)
        keep = (rmvs == False) & (igns == False)      # noqa: E712
        val = xywh_to_corners(np.array([gt.bbox_full * scale for gt in im.gts]))[keep, :]
        g3 = np.array([gt.bbox_3d for gt in im.gts])[keep, :]
        for i in range(val.shape[0]):
            w = val[i, 2] - val[i, 0] + 1
            h = val[i, 3] - val[i, 1] + 1
            val[i, 0:4] = anchor_center(w, h, conf.feat_stride)
        if val.shape[0] > 0:
            rows += np.concatenate((val, g3), axis=1).tolist()
    return np.array(rows)


def generate_anchors(conf, imdb):
    """(anchors float64 [A, 9], overlap table [A, N] of the centred ground truths)."""
    anchors = np.zeros([len(conf.anchor_scales) * len(conf.anchor_ratios), 4], dtype=np.float32)
    a = 0
    for scale in conf.anchor_scales:
        for ratio in conf.anchor_ratios:
            anchors[a, 0:4] = anchor_center(scale * ratio, scale, conf.feat_stride)
            a += 1
    ngt = normalized_gts(conf, imdb)
    anchors = np.concatenate((anchors, np.zeros([anchors.shape[0], 5])), axis=1)
    per = [[[] for _ in range(5)] for _ in range(anchors.shape[0])]
    ols = iou(anchors[:, 0:4], ngt[:, 0:4])
    best_ols, best_anchor = np.amax(ols, axis=0), np.argmax(ols, axis=0)
    for g, gt in enumerate(ngt):
        if best_ols[g] > ANCHOR_IOU:
            for k in range(5):
                per[best_anchor[g]][k].append(gt[6 + k])
    for a in range(anchors.shape[0]):
        if len(per[a][0]) == 0:
            raise ValueError('Non-used anchor #{} found'.format(a))
        for k in range(5):
            anchors[a, 4 + k] = np.mean(np.array(per[a][k]))
    return anchors, ols


# ---- compute_targets on float64 rois, compute_bbox_stats -------------------------------------------------------------------
def image_inputs(conf, im):
    """What compute_bbox_stats hands compute_targets for one image with gts: (feat_size, gts_val, gts_ign, box_lbls, gts_3d)."""
    sf = im.scale * conf.test_scale[0] / im.imH
    feat_size = np.ceil(np.array(np.array([im.imH, im.imW]) * sf) / conf.feat_stride).astype(int)
    igns, rmvs = determine_ignores(im.gts, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h, np.inf, sf)
    gts_all = xywh_to_corners(np.array([gt.bbox_full * sf for gt in im.gts]))
    keep = (rmvs == False) & (igns == False)      # noqa: E712
    gts_val = gts_all[keep, :]
    gts_ign = gts_all[(rmvs == False) & (igns == True), :]      # noqa: E712
    box_lbls = np.array([conf.lbls.index(gt.cls) + 1 for gt, k in zip(im.gts, keep) if k], dtype=np.int64)
    gts_3d = np.array([gt.bbox_3d for gt in im.gts])[keep, :]
    for i in range(gts_3d.shape[0]):
        gts_3d[i, 0:2] *= sf
    return feat_size, gts_val, gts_ign, box_lbls, gts_3d


def compute_targets(gts_val, gts_ign, box_lbls, rois, conf, gts_3d, anchors):
    """(transforms float32 [R, 12]: dx dy dw dh label x y z w h l ry with label > 0 fg, -1 bg, 0 ignored; overlap table or None;
    ignore-overlap table or None)."""
    transforms = np.zeros([len(rois), 12], dtype=np.float32)
    ols = ols_ign = None
    if gts_val.shape[0] > 0 or gts_ign.shape[0] > 0:
        if gts_ign.shape[0] > 0:
            ols_ign = iou(rois, gts_ign, ign=True)
            ols_ign_max = np.amax(ols_ign, axis=1)
        else:
            ols_ign_max = np.zeros([rois.shape[0]], dtype=np.float32)
        if gts_val.shape[0] > 0:
            ols = iou(rois, gts_val)
            ols_max, targets = np.amax(ols, axis=1), np.argmax(ols, axis=1)
            gt_best_rois, gt_best_ols = np.argmax(ols, axis=0), np.amax(ols, axis=0)
            gt_best_rois = gt_best_rois[gt_best_ols >= conf.best_thresh]
            fg_inds = np.unique(np.concatenate((np.flatnonzero(ols_max >= conf.fg_thresh), gt_best_rois)))
            tg, src = gts_val[targets[fg_inds], :], rois[fg_inds, :]
            if len(fg_inds) > 0:
                ew, eh = src[:, 2] - src[:, 0] + 1.0, src[:, 3] - src[:, 1] + 1.0
                ecx, ecy = src[:, 0] + 0.5 * (ew - 1), src[:, 1] + 0.5 * (eh - 1)
                assert ew.dtype == rois.dtype
                gw, gh = tg[:, 2] - tg[:, 0] + 1.0, tg[:, 3] - tg[:, 1] + 1.0
                gcx, gcy = tg[:, 0] + 0.5 * (gw - 1.0), tg[:, 1] + 0.5 * (gh - 1.0)
                transforms[fg_inds, 0:4] = np.vstack(((gcx - ecx) / ew, (gcy - ecy) / eh, np.log(gw / ew), np.log(gh / eh))).transpose()
                a3 = anchors[rois[fg_inds, 4].astype(np.int64), 4:]
                t3 = gts_3d[targets[fg_inds]]
                transforms[fg_inds, 5:] = np.vstack(((t3[:, 0] - ecx) / ew, (t3[:, 1] - ecy) / eh, t3[:, 2] - a3[:, 0],
                                                     np.log(t3[:, 3] / a3[:, 1]), np.log(t3[:, 4] / a3[:, 2]), np.log(t3[:, 5] / a3[:, 3]),
                                                     t3[:, 6] - a3[:, 4])).transpose()
                transforms[fg_inds, 4] = [box_lbls[x] for x in targets[fg_inds]]
        else:
            ols_max = np.zeros(rois.shape[0], dtype=int)
            fg_inds = gt_best_rois = np.empty(shape=[0])
        ign_inds = np.flatnonzero(ols_ign_max >= conf.ign_thresh)
        bg_inds = np.flatnonzero((ols_max >= conf.bg_thresh_lo) & (ols_max < conf.bg_thresh_hi))
        bg_inds = np.setdiff1d(np.setdiff1d(np.setdiff1d(bg_inds, ign_inds), fg_inds), gt_best_rois)
        transforms[bg_inds.astype(np.int64), 4] = -1
    else:
        transforms[:, 4] = -1
    return transforms, ols, ols_ign


def image_transforms(conf, im, rois_dtype=np.float64):
    """compute_targets of one image of the imdb (needs conf.anchors); None for an image without gts.  rois_dtype=np.float32 gives
    what the loss path's arithmetic would (the test that the float64 bound tells the two apart)."""
    if len(im.gts) == 0:
        return None
    fs, val, ign, lbls, g3 = image_inputs(conf, im)
    rois = locate_anchors(conf.anchors, fs, conf.feat_stride).astype(rois_dtype)
    return compute_targets(val, ign, lbls, rois, conf, g3, conf.anchors)


def image_sums(transforms):
    """Per image over the fg rows, in longdouble cast to float64: (n_fg, sum t, sum |t|, max |t|) of the 11 columns."""
    z = np.zeros(11)
    if transforms is None:
        return 0, z, z.copy(), z.copy()
    fg = np.flatnonzero(transforms[:, 4] > 0)
    if len(fg) == 0:
        return 0, z, z.copy(), z.copy()
    t = transforms[fg][:, [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11]].astype(np.longdouble)
    return len(fg), t.sum(axis=0).astype(np.float64), np.abs(t).sum(axis=0).astype(np.float64), np.abs(t).max(axis=0).astype(np.float64)


def compute_bbox_stats(conf, imdb):
    """(means, stds) float64 [1, 11], accumulated like the reference: float32 column sums per image into longdouble (pass 1),
    longdouble squares of (float32 - longdouble mean) (pass 2)."""
    ld = np.longdouble
    sums, sq = np.zeros([1, 11], dtype=ld), np.zeros([1, 11], dtype=ld)
    count = np.zeros([1], dtype=ld) + 1e-10
    per = [image_transforms(conf, im) for im in imdb]
    for p in per:
        if p is None:
            continue
        transforms = p[0]
        gt_inds = np.flatnonzero(transforms[:, 4] > 0)
        if len(gt_inds) > 0:
            sums[:, 0:4] += np.sum(transforms[gt_inds, 0:4], axis=0)
            sums[:, 4:] += np.sum(transforms[gt_inds, 5:12], axis=0)
            count += len(gt_inds)
    means = sums / count
    for p in per:
        if p is None:
            continue
        transforms = p[0]
        gt_inds = np.flatnonzero(transforms[:, 4] > 0)
        if len(gt_inds) > 0:
            sq[:, 0:4] += np.sum(np.power(transforms[gt_inds, 0:4] - means[:, 0:4], 2), axis=0)
            sq[:, 4:] += np.sum(np.power(transforms[gt_inds, 5:12] - means[:, 4:], 2), axis=0)
    stds = np.sqrt((sq / count))
    return means.astype(float), stds.astype(float)


def nearest_threshold_gap(tables, conf):
    """Smallest |overlap - threshold| over the (overlap, ignore overlap) tables of compute_targets (None entries skipped)."""
    gap = np.inf
    for ols, ign_ov in tables:
        if ols is not None:
            for th in (conf.fg_thresh, conf.bg_thresh_hi, conf.best_thresh):
                gap = min(gap, float(np.abs(ols - th).min()))
        if ign_ov is not None:
            gap = min(gap, float(np.abs(ign_ov - conf.ign_thresh).min()))
    return gap
