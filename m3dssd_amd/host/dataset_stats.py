"""``generate_anchors`` (lib/rpn_util.py:25-164) and ``compute_bbox_stats`` (lib/rpn_util.py:732-889): what the training dataset
runs in its constructor when ``conf.anchors is None`` (lib/dataloader.py:885-887) -- the anchor priors and the means / stds of
the regression targets, from the imdb.

``generate_anchors`` is N_gt x A work and stays on the host in numpy, operation by operation like the reference, so that the
anchors equal the reference's bit for bit.  Implemented: ``cluster_anchors = 0`` (every shipped configuration); a truthy
``cluster_anchors`` raises NotImplementedError (the reference's k-means is not provided).

``compute_bbox_stats`` in the reference calls the numpy ``compute_targets`` twice per image.  Here the host part is the gt table
of each image (``pack_gts_scaled``: the boxes scaled to the test scale, ignores decided with ``max_gt_h = inf``); the images are
grouped by feature-map size, and m3d_rpn_target_stats (csrc/rpn_loss.hip) assigns the targets on float64 anchor boxes and
reduces them to 23 numbers per image.  Pass 1 (center 0) gives the means, pass 2 (center = means) the stds; the per-image rows
are added on the host in ``np.longdouble`` in imdb order.  The reference adds each image's float32 transforms in float32 first;
here every sum is float64 or wider, so means and stds agree with the reference's to float32 rounding of the largest target, not
bit for bit.  No ROCm device and no cache: NotImplementedError (no CPU fallback).  ``conf.has_3d`` false: NotImplementedError.

Caches (``anchors.pkl``, ``bbox_means.pkl``, ``bbox_stds.pkl`` in ``cache_folder``) are plain pickles with the reference's names:
they move both ways.  A cache hit touches no device.
"""
import os
import pickle

import numpy as np

from .. import rpn_util
from . import loss as hl

CHUNK = 64          # images per m3d_rpn_target_stats call
_get = hl._get


def _pickle_read(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _pickle_write(path, obj):
    with open(path, "wb") as f:
        pickle.dump(obj, f)


def _has_3d(conf):
    return bool(conf["has_3d"]) if "has_3d" in conf else False


def image_scale(conf, imobj):
    """scale_factor = imobj.scale * conf.test_scale[0] / imobj.imH"""
    return _get(imobj, "scale") * conf.test_scale[0] / _get(imobj, "imH")


def image_feat_size(conf, imobj):
    """(feat_h, feat_w) of one image at the test scale: calc_output_size([imH, imW] * scale_factor, stride)."""
    sf = image_scale(conf, imobj)
    fs = rpn_util.calc_output_size(np.array([_get(imobj, "imH"), _get(imobj, "imW")]) * sf, conf.feat_stride)
    return int(fs[0]), int(fs[1])


def _scaled_corners(gts, sf):
    box = np.array([np.asarray(_get(gt, "bbox_full"), dtype=np.float64) * sf for gt in gts])       # bbXYWH2Coords:
    box[:, 2] += box[:, 0] - 1
    box[:, 3] += box[:, 1] - 1
    return box


# ---- generate_anchors ------------------------------------------------------------------------------------------------------
def normalized_gts(conf, imdb):
    """[N, 11]: every valid ground truth of the imdb, its scaled 2-D box centred like an anchor (columns 0-3), then bbox_3d[0:7]."""
    rows = []
    for imobj in imdb:
        gts = _get(imobj, "gts")
        if len(gts) == 0:
            continue
        sf = image_scale(conf, imobj)
        igns, rmvs = hl.determine_ignores(gts, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h, np.inf, sf)
        keep = (rmvs == False) & (igns == False)      # noqa: E712
        val = _scaled_corners(gts, sf)[keep, :4]
        g3 = np.array([np.asarray(_get(gt, "bbox_3d"), dtype=np.float64) for gt in gts])[keep, :]
        for i in range(val.shape[0]):
            w = val[i, 2] - val[i, 0] + 1
            h = val[i, 3] - val[i, 1] + 1
            val[i, 0:4] = rpn_util.anchor_center(w, h, conf.feat_stride)
        if val.shape[0] > 0:
            rows += np.concatenate((val, g3), axis=1).tolist()
    return np.array(rows)


def _iou_anchor_gt(anchors, boxes):
    """[A, N] float64, lib/core.py:341-380 on numpy arrays."""
    mx = np.minimum(anchors[:, None, 2:4], boxes[None, :, 2:4])
    mn = np.maximum(anchors[:, None, 0:2], boxes[None, :, 0:2])
    d = np.clip(mx - mn, a_min=0, a_max=None)
    inter = d[:, :, 0] * d[:, :, 1]
    area_a = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    area_b = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    return inter / (area_a[:, None] + area_b[None, :] - inter)


def generate_anchors(conf, imdb, cache_folder):
    """Sets ``conf.anchors``: float32 [A, 4] without ``has_3d``, else float64 [A, 9] = the 2-D anchor of every scale x ratio
    (float32 values) and the mean z, w, h, l, ry of the ground truths it is the best anchor of (IoU > 0.2 after centring)."""
    path = os.path.join(cache_folder, "anchors.pkl") if cache_folder is not None else None
    if path is not None and os.path.exists(path):
        conf.anchors = _pickle_read(path)
        return
    anchors = rpn_util.generate_anchors_2d(conf.anchor_scales, conf.anchor_ratios, conf.feat_stride)
    if conf["cluster_anchors"] if "cluster_anchors" in conf else False:
        raise NotImplementedError("generate_anchors: cluster_anchors (the k-means of lib/rpn_util.py:186-427) is not provided; "
                                  "every shipped configuration sets cluster_anchors = 0")
    if _has_3d(conf):
        ngt = normalized_gts(conf, imdb)
        anchors = np.concatenate((anchors, np.zeros([anchors.shape[0], 5])), axis=1)
        if ngt.shape[0] == 0:
            raise ValueError('Non-used anchor #{} found'.format(0))
        ols = _iou_anchor_gt(anchors[:, 0:4], ngt[:, 0:4])
        best_ols = np.amax(ols, axis=0)
        best_anchor = np.argmax(ols, axis=0)
        for aind in range(anchors.shape[0]):
            mine = ngt[(best_anchor == aind) & (best_ols > 0.2)]          # in ground-truth order
            if mine.shape[0] == 0:
                raise ValueError('Non-used anchor #{} found'.format(aind))
            for k in range(5):
                anchors[aind, 4 + k] = np.mean(np.array(mine[:, 6 + k].tolist()))
    if path is not None:
        _pickle_write(path, anchors)
    conf.anchors = anchors


# ---- compute_bbox_stats ----------------------------------------------------------------------------------------------------
def pack_gts_scaled(conf, imobjs):
    """The gt table of m3d_rpn_target_stats, float64 [B, Gmax + 1, 12], laid out like ``loss.pack_gts``' but as
    compute_bbox_stats sees the ground truths: ``bbox_full * scale_factor`` before the corner conversion, ``bbox_3d[0:2] *
    scale_factor``, ignores decided on the scaled height with ``max_gt_h = inf``.  An image without ``gts`` gets an empty row."""
    per = []
    for imobj in imobjs:
        gts = _get(imobj, "gts")
        val, ign = [], []
        if len(gts) > 0:
            sf = image_scale(conf, imobj)
            igns, rmvs = hl.determine_ignores(gts, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h, np.inf, sf)
            box = _scaled_corners(gts, sf)
            for i, gt in enumerate(gts):
                if rmvs[i]:
                    continue
                if igns[i]:
                    ign.append([float(v) for v in box[i, :4]] + [0.0] * 8)
                    continue
                cls = _get(gt, "cls")
                if cls not in conf.lbls:
                    raise ValueError("unknown class")                     # clsName2Ind, lib/rpn_util.py:722-729
                b3 = np.array(_get(gt, "bbox_3d"), dtype=np.float64)[:7]
                b3[0:2] *= sf
                val.append([float(v) for v in box[i, :4]] + [float(list(conf.lbls).index(cls) + 1)] + [float(v) for v in b3])
        if len(val) + len(ign) > hl.MAX_GT:
            raise RuntimeError("compute_bbox_stats: %d ground truths (valid + ignore) in one image exceed the kernel's cap of %d"
                               % (len(val) + len(ign), hl.MAX_GT))
        per.append((val, ign))
    gmax = max([len(v) + len(i) for v, i in per] + [1])
    table = np.zeros((len(per), gmax + 1, hl.GT_COLS), dtype=np.float64)
    for b, (val, ign) in enumerate(per):
        table[b, 0, 0], table[b, 0, 1] = len(val), len(ign)
        if val:
            table[b, 1:1 + len(val)] = np.asarray(val)
        if ign:
            table[b, 1 + len(val):1 + len(val) + len(ign)] = np.asarray(ign)
    return table


def group_by_feat_size(conf, imdb, chunk=CHUNK):
    """[(feat_size, [imdb indices])]: the images grouped by feature-map size, each group cut into chunks of at most ``chunk``;
    every image appears once."""
    groups = {}
    for i, imobj in enumerate(imdb):
        groups.setdefault(image_feat_size(conf, imobj), []).append(i)
    out = []
    for fs in sorted(groups):
        idx = groups[fs]
        out += [(fs, idx[k:k + chunk]) for k in range(0, len(idx), chunk)]
    return out


def stats_conf_vec(conf):
    """The settings vector of m3d_rpn_target_stats: thresholds and stride; means 0, stds 1 and neutral loss settings (not read)."""
    return hl.pack_conf(np.zeros(11), np.ones(11), conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo, conf.bg_thresh_hi,
                        conf.best_thresh, float("inf"), None, 0, 1, 1, 1, 1, conf.feat_stride)


def _device_or_raise(conf, who):
    import torch
    name = conf["device"] if "device" in conf and conf["device"] else "cuda:0"
    dev = torch.device(name)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise NotImplementedError("%s: no cache and no ROCm device (device=%s): there is no CPU fallback" % (who, name))
    return dev


def image_target_stats(conf, imdb, center=None, plan=None, tables=None, device=None):
    """float64 [len(imdb), 23] on the host: m3d_rpn_target_stats' row of every image, in imdb order."""
    import torch
    dev = device if device is not None else _device_or_raise(conf, "compute_bbox_stats")
    plan = plan if plan is not None else group_by_feat_size(conf, imdb)
    anchors = torch.from_numpy(np.ascontiguousarray(np.asarray(conf.anchors, dtype=np.float64))).to(dev)
    vec = stats_conf_vec(conf)
    rows = np.zeros((len(imdb), hl.TARGET_STATS_COLS), dtype=np.float64)
    outs = []
    for k, (fs, idx) in enumerate(plan):
        table = tables[k] if tables is not None else pack_gts_scaled(conf, [imdb[i] for i in idx])
        outs.append(hl.rpn_target_stats(anchors, vec, table, fs, center))
    for (fs, idx), o in zip(plan, outs):          # downloads after the last launch
        rows[idx] = o.cpu().numpy()
    return rows


def compute_bbox_stats(conf, imdb, cache_folder=''):
    """Sets ``conf.bbox_means`` / ``conf.bbox_stds`` (float64 [1, 11]): mean and std of the raw regression targets over the fg
    anchors of every image of the imdb at the test scale."""
    pm = os.path.join(cache_folder, "bbox_means.pkl") if cache_folder is not None else None
    ps = os.path.join(cache_folder, "bbox_stds.pkl") if cache_folder is not None else None
    if pm is not None and os.path.exists(pm) and os.path.exists(ps):
        conf.bbox_means, conf.bbox_stds = _pickle_read(pm), _pickle_read(ps)
        return
    if not _has_3d(conf):
        raise NotImplementedError("compute_bbox_stats: has_3d = False (4 columns) is not provided; every shipped configuration is 3-D")
    dev = _device_or_raise(conf, "compute_bbox_stats")
    plan = group_by_feat_size(conf, imdb)
    tables = [pack_gts_scaled(conf, [imdb[i] for i in idx]) for _fs, idx in plan]
    ld = np.longdouble
    rows = image_target_stats(conf, imdb, None, plan, tables, dev)
    count = np.zeros([1], dtype=ld) + 1e-10
    sums = np.zeros([1, 11], dtype=ld)
    for r in rows:                                 # imdb order
        sums += r[1:12].astype(ld)
        count += r[0].astype(ld)
    means = sums / count
    rows = image_target_stats(conf, imdb, means.astype(np.float64), plan, tables, dev)
    sq = np.zeros([1, 11], dtype=ld)
    for r in rows:
        sq += r[12:23].astype(ld)
    stds = np.sqrt(sq / count)
    means, stds = means.astype(float), stds.astype(float)
    if pm is not None:
        _pickle_write(pm, means)
        _pickle_write(ps, stds)
    conf.bbox_means, conf.bbox_stds = means, stds
