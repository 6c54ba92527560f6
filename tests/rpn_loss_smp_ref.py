"""Yardstick of the RPN_3D_loss_smp tests: a restatement of the data loader's ``Kitti_Dataset_torch._targets``
(lib/dataloader.py:1014-1144) with the collate step, and of the reference's RPN_3D_loss_smp.forward (lib/loss/rpn_3d.py:705-1360)
with a dtype switch.  Built on the pieces of tests/rpn_loss_ref.py (``assign`` is its compute_targets restatement).

Test infrastructure only -- the product never imports it.

As in rpn_loss_ref, labels and samples follow the reference operation by operation in every dtype mode; ``dtype`` switches the
differentiable part: float32 is the reference's arithmetic, float64 the yardstick of the device tests.  Among equal scores the
lower row is taken first (the reference's torch.sort is unstable; the golden generator asserts the scores at the cut differ).

Two places where the restatement states what the product does, not what the reference does:
  * ``bbox_2d_lambda != 0``: the reference raises NameError (``bbox_x`` is commented out); the term is RPN_3D_loss' here;
  * an image with a valid gt but neither a fg nor an ignored anchor: the reference's branch (lib/loss/rpn_3d.py:961-987) rounds
    ``box_samples * (1 - fg_fraction)`` (0.16 -> 0) and therefore keeps EVERY anchor as bg; here such an image is sampled like
    any other, as RPN_3D_loss on the device and rpn_loss_ref do.  No golden case contains such an image.
"""
import numpy as np
import torch
import torch.nn.functional as F

from m3dssd_amd import rpn_util

import rpn_loss_ref as RR

IGN_FLAG = RR.IGN_FLAG
# the golden files: name -> (seed, variant, empty image, crop, B, ground truths per image)
GOLDEN_CASES = {"shipped": (11, "shipped", None, (128, 320), 2, 6), "allboxes": (11, "allboxes", None, (128, 320), 2, 6),
                "emptyimg": (12, "shipped", 1, (128, 320), 2, 6), "odd": (14, "shipped", 1, (40, 72), 3, 3)}


def golden_case(name):
    seed, variant, empty, crop, B, n_gt = GOLDEN_CASES[name]
    return RR.loss_conf(crop, 0, **RR.VARIANTS[variant]), RR.make_case(seed, crop, B, n_gt, empty_image=empty)


def image_targets(conf, imobj, rois32):
    """``_targets`` of one image: (labels_fg, labels_bg, labels_ign, labels int64 [R], bbox_2d float32 [R, 4], bbox_3d float32
    [R, 7], any_val, overlap tables or None)."""
    R = rois32.shape[0]
    val, ign, lab, g3 = RR.split_gts(imobj, conf)
    if len(val) == 0:
        z = np.zeros(R, dtype=np.int64)
        return z, np.ones(R, dtype=np.int64), z.copy(), z.copy(), np.zeros((R, 4), np.float32), np.zeros((R, 7), np.float32), 0, None
    labels, _gidx, t, ols = RR.assign(rois32, np.asarray(conf.anchors), val, ign, lab, g3, conf)
    fg, bg, ig = (labels > 0) & (labels != IGN_FLAG), labels == 0, labels == IGN_FLAG
    return fg.astype(np.int64), bg.astype(np.int64), ig.astype(np.int64), labels, t[:, :4].copy(), t[:, 4:].copy(), 1, ols


def make_target(conf, imobjs, feat_size):
    """The collated batch['target'] of the reference's loader (host tensors, int64 labels), plus the overlap tables of the
    generator's uniqueness check under the key '_overlaps' (not part of the loader's dict)."""
    rois32 = rpn_util.locate_anchors(np.asarray(conf.anchors), feat_size, conf.feat_stride, convert_tensor=True).float().numpy()
    per = [image_targets(conf, im, rois32) for im in imobjs]
    st = lambda i: torch.from_numpy(np.stack([p[i] for p in per]))      # noqa: E731
    B = len(imobjs)
    return {"labels_fg": st(0), "labels_bg": st(1), "labels_ign": st(2), "labels": st(3), "bbox_2d": st(4), "bbox_3d": st(5),
            "meta": {"rois": torch.from_numpy(np.stack([rois32] * B)), "any_val": torch.tensor([p[6] for p in per], dtype=torch.int64)},
            "_overlaps": [p[7] for p in per]}


def rpn_3d_loss_smp(conf, cls, prob, bbox_2d, bbox_3d, target, feat_size, dtype=torch.float64, grads=True):
    """Returns a dict like rpn_loss_ref.rpn_3d_loss: loss (python float), stats (the smp list with float values), labels [B, R]
    int64, targets [B, R, 11] float32, sampled [B, R] uint8 (1 fg, 2 bg), margins, fg_num, bg_num and g_cls / g_bbox_2d /
    g_bbox_3d (float64 numpy) when ``grads``."""
    if conf.bbox_3d_proj_lambda:
        raise NotImplementedError("bbox_3d_proj_lambda")
    B, R, C = cls.shape
    anchors = np.asarray(conf.anchors)
    rois32 = rpn_util.locate_anchors(anchors, feat_size, conf.feat_stride, convert_tensor=True).float().numpy()
    labels = target["labels"].cpu().numpy().astype(np.int64)
    targets = np.concatenate([target["bbox_2d"].cpu().numpy(), target["bbox_3d"].cpu().numpy()], axis=2)
    assert targets.dtype == np.float32
    any_val = target["meta"]["any_val"].cpu().numpy()
    prob_np = prob.detach().numpy()
    sampled = np.zeros((B, R), dtype=np.uint8)
    scores = np.zeros((B, R), dtype=np.float64)
    margins = []
    for b in range(B):
        if not any_val[b]:
            continue
        fi, bi = RR.sample(labels[b], prob_np[b], conf, R)
        margins += RR.cut_margins(labels[b], prob_np[b], conf, R)
        sampled[b, bi] = 2
        sampled[b, fi] = 1
        act = labels[b] != IGN_FLAG
        scores[b, act] = prob_np[b, act, labels[b, act]]

    t = lambda x: x.detach().clone().to(dtype).requires_grad_(grads)      # noqa: E731
    cls_d, b2_d, b3_d = t(cls), t(bbox_2d), t(bbox_3d)
    stats = []
    loss = torch.zeros((), dtype=dtype)
    fg_all, bg_all = (labels > 0) & (labels != IGN_FLAG), labels == 0
    pred = cls.argmax(dim=2).numpy()
    if conf.cls_2d_lambda and fg_all.any():
        stats.append({'name': 'fg', 'val': float(np.mean(pred[fg_all] == labels[fg_all])), 'format': '{:0.2f}', 'group': 'acc'})
    if conf.cls_2d_lambda:          # the reference tests the length of a 2-tuple: always present
        stats.append({'name': 'bg', 'val': float(np.mean(pred[bg_all] == labels[bg_all])) if bg_all.any() else float("nan"),
                      'format': '{:0.2f}', 'group': 'acc'})
    fg_s, bg_s = sampled == 1, sampled == 2
    fg_num, bg_num = int(fg_s.sum()), int(bg_s.sum())
    weight = np.zeros((B, R), dtype=np.float64)
    weight[fg_s | bg_s] = 1.0
    if conf.fg_fraction is not None and fg_num > 0:
        weight[fg_s] = (conf.fg_fraction / (1 - conf.fg_fraction)) * (bg_num / fg_num)
    if conf.focal_loss:
        weight[bg_s] *= (1 - scores[bg_s]) ** conf.focal_loss
        weight[fg_s] *= (1 - scores[fg_s]) ** conf.focal_loss
    w_t = torch.from_numpy(weight).to(dtype)
    lab_t = torch.from_numpy(labels)
    if conf.cls_2d_lambda:
        act = (w_t > 0)
        if bool(act.any()):
            ce = F.cross_entropy(cls_d[act], lab_t[act], reduction='none')
            l_cls = ((ce * w_t[act]).clamp(min=0, max=2000)).mean() * conf.cls_2d_lambda
            loss = loss + l_cls
            stats.append({'name': 'cls', 'val': float(l_cls.detach()), 'format': '{:0.4f}', 'group': 'loss'})
    if fg_num > 0:
        act = torch.from_numpy(fg_s)
        tar = torch.from_numpy(targets).to(dtype)
        if conf.bbox_2d_lambda:
            l2 = sum(F.smooth_l1_loss(b2_d[..., k][act], tar[..., k][act], reduction='none').mean() for k in range(4))
            loss = loss + l2 * conf.bbox_2d_lambda
        if conf.bbox_3d_lambda:
            c = [F.smooth_l1_loss(b3_d[..., k][act], tar[..., 4 + k][act], reduction='none').mean() for k in range(7)]
            l3 = ((c[0] + c[1] + c[2]) + (c[3] + c[4] + c[5] + c[6])) * conf.bbox_3d_lambda
            loss = loss + l3
            stats.append({'name': 'bbox3d', 'val': float(l3.detach()), 'format': '{:0.4f}', 'group': 'loss'})
        means = torch.from_numpy(np.asarray(conf.bbox_means, dtype=np.float64).reshape(-1)).to(dtype)
        stds = torch.from_numpy(np.asarray(conf.bbox_stds, dtype=np.float64).reshape(-1)).to(dtype)
        rois_t = torch.from_numpy(rois32).to(dtype)
        anc = torch.from_numpy(anchors[rois32[:, 4].astype(np.int64)].astype(np.float32)).to(dtype)
        ious, zs, rys = [], [], []
        for b in range(B):
            fi = torch.from_numpy(np.flatnonzero(fg_s[b]))
            if len(fi) == 0:
                continue
            ious.append(RR.iou_list(RR.decode_2d(rois_t[fi], b2_d[b, fi], means, stds), RR.decode_2d(rois_t[fi], tar[b, fi, 0:4], means, stds)))
            z_p = anc[fi, 4] + (b3_d[b, fi, 2] * stds[6] + means[6])
            z_t = anc[fi, 4] + (tar[b, fi, 6] * stds[6] + means[6])
            r_p = anc[fi, 8] + (b3_d[b, fi, 6] * stds[10] + means[10])
            r_t = anc[fi, 8] + (tar[b, fi, 10] * stds[10] + means[10])
            zs.append((z_t - z_p).abs())
            rys.append((r_t - r_p).abs())
        ious, zs, rys = torch.cat(ious), torch.cat(zs), torch.cat(rys)
        stats.append({'name': 'z', 'val': float(zs.mean().detach()), 'format': '{:0.2f}', 'group': 'misc'})
        stats.append({'name': 'ry', 'val': float(rys.mean().detach()), 'format': '{:0.2f}', 'group': 'misc'})
        stats.append({'name': 'iou', 'val': float(ious.mean().detach()), 'format': '{:0.2f}', 'group': 'acc'})
        if conf.iou_2d_lambda:
            l_iou = (-torch.log(ious)).mean() * conf.iou_2d_lambda
            loss = loss + l_iou
            stats.append({'name': 'iou', 'val': float(l_iou.detach()), 'format': '{:0.4f}', 'group': 'loss'})
        stats.append({'name': 'ttloss', 'val': float(loss.detach()), 'format': '{:0.4f}', 'group': 'loss'})
    out = dict(loss=float(loss.detach()), stats=stats, labels=labels, targets=targets, sampled=sampled, margins=margins, fg_num=fg_num,
               bg_num=bg_num)
    if grads and loss.requires_grad:
        loss.backward()
        z = lambda x: (x.grad if x.grad is not None else torch.zeros_like(x)).double().numpy()      # noqa: E731
        out.update(g_cls=z(cls_d), g_bbox_2d=z(b2_d), g_bbox_3d=z(b3_d))
    return out
