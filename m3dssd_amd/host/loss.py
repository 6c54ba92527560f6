"""RPN_3D_loss (lib/loss/rpn_3d.py:14-657) on the HIP library.

The reference copies ``prob`` to the host, assigns targets and samples in numpy one image at a time and uploads sixteen
``[B, R]`` arrays again.  Here the host part is what concerns a few dozen ground-truth boxes -- ``determine_ignores``, the class
lookup and the XYWH -> corner conversion (``pack_gts``) -- and one packed table is uploaded per call.  Target assignment
(``compute_targets``, lib/rpn_util.py:430-532), the hard-negative selection and the loss with its gradients run in
m3d_rpn_targets / m3d_rpn_loss (csrc/rpn_loss.hip); one small stat block is downloaded after the last launch for the ``stats``
list.  ``loss`` stays on the device and carries a ``grad_fn``: the gradients with respect to ``cls``, ``bbox_2d`` and ``bbox_3d``
were written by the same launch and are handed to autograd in ``backward`` (scaled when ``grad_output`` is not 1).

Not supported (NotImplementedError): ``bbox_3d_proj_lambda != 0`` (the reference's branch mixes host and device tensors),
random sampling (``hard_negatives=False`` with a finite ``box_samples``: it draws from numpy's global RNG stream) and
``RPN_3D_loss_smp`` (it consumes targets the data loader pre-computes).  Host tensors: NotImplementedError, no CPU fallback.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from . import ops

MAX_GT = 128          # M3D_RPN_MAX_GT
GT_COLS = 12          # M3D_RPN_GT_COLS
CONF_COUNT = 35       # M3D_RPN_CONF_COUNT
STAT_NAMES = ("loss", "cls", "bbox_2d", "bbox_3d", "iou_loss", "z", "ry", "iou_acc", "acc_fg", "acc_bg", "n_fg", "n_bg", "fg_num",
              "bg_num", "n_active", "fg_weight")          # M3D_RPN_STAT_*
IGN_FLAG = 3000


def _get(o, k):
    return o[k] if isinstance(o, dict) else getattr(o, k)


def determine_ignores(gts, lbls, ilbls, min_gt_vis=0.99, min_gt_h=0, max_gt_h=10e10, scale_factor=1):
    """lib/rpn_util.py:1280-1302: which ground truths are ignore regions, which are dropped."""
    igns = np.zeros([len(gts)], dtype=bool)
    rmvs = np.zeros([len(gts)], dtype=bool)
    for i, gt in enumerate(gts):
        h = _get(gt, "bbox_full")[3] * scale_factor
        cls = _get(gt, "cls")
        igns[i] = bool(_get(gt, "ign")) or _get(gt, "visibility") < min_gt_vis or h < min_gt_h or h > max_gt_h or cls in ilbls
        rmvs[i] = cls not in (list(lbls) + list(ilbls))
    return igns, rmvs


def pack_gts(imobjs, lbls, ilbls, min_gt_vis, min_gt_h):
    """The one upload of a loss call: float64 [B, Gmax + 1, 12].  Row 0 of an image = (n_valid, n_ignore); then the valid ground
    truths (x1 y1 x2 y2, class index 1.., bbox_3d[0:7]); then the ignore regions (x1 y1 x2 y2).  Corners are x + w - 1
    (bbXYWH2Coords).  The library refuses more than MAX_GT rows in one image (the kernels hold one image's table on chip)."""
    per = []
    for imobj in imobjs:
        gts = _get(imobj, "gts")
        igns, rmvs = determine_ignores(gts, lbls, ilbls, min_gt_vis, min_gt_h)
        val, ign = [], []
        for gt, ig, rm in zip(gts, igns, rmvs):
            if rm:
                continue
            x, y, w, h = (float(v) for v in np.asarray(_get(gt, "bbox_full"), dtype=np.float64)[:4])
            box = [x, y, w + (x - 1), h + (y - 1)]
            if ig:
                ign.append(box + [0.0] * 8)
            else:
                cls = _get(gt, "cls")
                if cls not in lbls:
                    raise ValueError("unknown class")                     # clsName2Ind, lib/rpn_util.py:722-729
                b3 = np.asarray(_get(gt, "bbox_3d"), dtype=np.float64)
                val.append(box + [float(list(lbls).index(cls) + 1)] + [float(v) for v in b3[:7]])
        per.append((val, ign))
    gmax = max([len(v) + len(i) for v, i in per] + [1])       # (more than MAX_GT: m3d_rpn_targets answers M3D_E_ARG)
    table = np.zeros((len(per), gmax + 1, GT_COLS), dtype=np.float64)
    for b, (val, ign) in enumerate(per):
        table[b, 0, 0], table[b, 0, 1] = len(val), len(ign)
        if val:
            table[b, 1:1 + len(val)] = np.asarray(val)
        if ign:
            table[b, 1 + len(val):1 + len(val) + len(ign)] = np.asarray(ign)
    return table


def pack_conf(bbox_means, bbox_stds, fg_thresh, ign_thresh, bg_thresh_lo, bg_thresh_hi, best_thresh, box_samples, fg_fraction,
              focal_loss, cls_2d_lambda, iou_2d_lambda, bbox_2d_lambda, bbox_3d_lambda, feat_stride):
    """The float64 [M3D_RPN_CONF_COUNT] settings vector of m3d_rpn_targets / m3d_rpn_loss."""
    means = np.asarray(bbox_means, dtype=np.float64).reshape(-1)
    stds = np.asarray(bbox_stds, dtype=np.float64).reshape(-1)
    if means.size != 11 or stds.size != 11:
        raise RuntimeError("rpn_loss: bbox_means / bbox_stds must hold 11 values (4 2-D + 7 3-D)")
    if fg_fraction is None and not math.isinf(float(box_samples)):
        raise ValueError("rpn_loss: fg_fraction=None needs box_samples=inf (the reference multiplies box_samples by it)")
    tail = [fg_thresh, ign_thresh, bg_thresh_lo, bg_thresh_hi, best_thresh, box_samples,
            float("nan") if fg_fraction is None else fg_fraction, focal_loss or 0.0, cls_2d_lambda or 0.0, iou_2d_lambda or 0.0,
            bbox_2d_lambda or 0.0, bbox_3d_lambda or 0.0, feat_stride]
    vec = np.concatenate([means, stds, np.asarray([float(v) for v in tail])])
    assert vec.size == CONF_COUNT
    return np.ascontiguousarray(vec)


def _check_inputs(who, cls, prob, bbox_2d, bbox_3d, n_anchors, feat_size):
    ops._require_cuda(*[t for t in (cls, prob, bbox_2d, bbox_3d) if t is not None])
    H, W = int(feat_size[0]), int(feat_size[1])
    R = n_anchors * H * W
    B = cls.shape[0]
    for name, t, last in (("cls", cls, None), ("prob", prob, None), ("bbox_2d", bbox_2d, 4), ("bbox_3d", bbox_3d, 7)):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s must be float32 (got %s)" % (who, name, t.dtype))
        if t.dim() != 3 or t.shape[0] != B or t.shape[1] != R or (last is not None and t.shape[2] != last) or \
                (last is None and t.shape[2] != cls.shape[2]):
            raise RuntimeError("%s: %s has shape %s; expected [%d, %d = %d anchors x %d x %d, %s]"
                               % (who, name, tuple(t.shape), B, R, n_anchors, H, W, last if last is not None else cls.shape[2]))
        if not t.is_contiguous():
            raise RuntimeError("%s: %s must be contiguous" % (who, name))
    return B, R, H, W, int(cls.shape[2])


class _Ctx:
    """Device-side state shared by rpn_targets and rpn_loss: anchors, settings, gt table, workspace."""

    def __init__(self, anchors, conf_vec, gt_table, feat_size, B, R, device):
        L = _hip.lib()
        self.anchors = anchors if torch.is_tensor(anchors) else \
            torch.from_numpy(np.ascontiguousarray(np.asarray(anchors, dtype=np.float64))).to(device)
        if self.anchors.dtype != torch.float64 or self.anchors.dim() != 2 or self.anchors.shape[1] != 9 or not self.anchors.is_cuda:
            raise RuntimeError("rpn_loss: anchors must be [A, 9] (x1 y1 x2 y2 z w h l ry)")
        self.conf = np.ascontiguousarray(conf_vec, dtype=np.float64)
        gt_table = np.ascontiguousarray(gt_table, dtype=np.float64)
        if gt_table.ndim != 3 or gt_table.shape[0] != B or gt_table.shape[2] != GT_COLS or gt_table.shape[1] < 1:
            raise RuntimeError("rpn_loss: gt table must be [B = %d, Gmax + 1, %d] (got %s)" % (B, GT_COLS, gt_table.shape))
        counts = gt_table[:, 0, 0] + gt_table[:, 0, 1]
        if (gt_table[:, 0, :2] < 0).any() or (counts > gt_table.shape[1] - 1).any():
            raise RuntimeError("rpn_loss: gt table counts exceed its rows")
        self.Gmax = gt_table.shape[1] - 1
        self.max_label = max([int(gt_table[b, 1:1 + int(gt_table[b, 0, 0]), 4].max()) for b in range(B) if gt_table[b, 0, 0] > 0] + [1])
        self.min_label = min([int(gt_table[b, 1:1 + int(gt_table[b, 0, 0]), 4].min()) for b in range(B) if gt_table[b, 0, 0] > 0] + [1])
        self.gt = torch.from_numpy(gt_table).to(device, non_blocking=False)            # the upload
        self.H, self.W = int(feat_size[0]), int(feat_size[1])
        self.A = int(self.anchors.shape[0])
        nbytes = L.m3d_rpn_loss_workspace_bytes(B, R)
        self.ws = torch.empty(nbytes + 256, device=device, dtype=torch.uint8)
        self.ws_base = (self.ws.data_ptr() + 255) // 256 * 256
        self.ws_bytes = nbytes

    def conf_ptr(self):
        return self.conf.ctypes.data


def _targets(ctx, cls, prob):
    L = _hip.lib()
    B, R, C = cls.shape
    dev = cls.device
    if ctx.min_label < 1 or ctx.max_label >= C:
        raise RuntimeError("rpn_loss: gt class labels must lie in 1 .. %d (got %d .. %d)" % (C - 1, ctx.min_label, ctx.max_label))
    labels = torch.empty(B, R, device=dev, dtype=torch.int16)
    gt_index = torch.empty(B, R, device=dev, dtype=torch.int16)
    targets = torch.empty(B, R, 11, device=dev, dtype=torch.float32)
    scores = torch.empty(B, R, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _hip.check(L.m3d_rpn_targets(ctx.anchors.data_ptr(), ctx.A, ctx.H, ctx.W, ctx.conf_ptr(), CONF_COUNT, ctx.gt.data_ptr(), B,
                                     ctx.Gmax, cls.data_ptr(), prob.data_ptr(), C, labels.data_ptr(), gt_index.data_ptr(),
                                     targets.data_ptr(), scores.data_ptr(), ctx.ws_base, ctx.ws_bytes, ops._stream()))
    return labels, gt_index, targets, scores


def _loss(ctx, cls, bbox_2d, bbox_3d, labels, targets, scores):
    L = _hip.lib()
    B, R, C = cls.shape
    dev = cls.device
    sampled = torch.empty(B, R, device=dev, dtype=torch.uint8)
    g_cls, g_2d, g_3d = torch.empty_like(cls), torch.empty_like(bbox_2d), torch.empty_like(bbox_3d)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    stats = torch.empty(len(STAT_NAMES), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _hip.check(L.m3d_rpn_loss(ctx.anchors.data_ptr(), ctx.A, ctx.H, ctx.W, ctx.conf_ptr(), CONF_COUNT, ctx.gt.data_ptr(), B, ctx.Gmax,
                                  cls.data_ptr(), bbox_2d.data_ptr(), bbox_3d.data_ptr(), C, labels.data_ptr(), targets.data_ptr(),
                                  scores.data_ptr(), sampled.data_ptr(), g_cls.data_ptr(), g_2d.data_ptr(), g_3d.data_ptr(),
                                  loss.data_ptr(), stats.data_ptr(), ctx.ws_base, ctx.ws_bytes, ops._stream()))
    return loss, stats, sampled, (g_cls, g_2d, g_3d)


def rpn_targets(cls, prob, anchors, conf_vec, gt_table, feat_size):
    """Target assignment alone: (labels int16 [B, R], gt_index int16 [B, R], targets float32 [B, R, 11], scores float32 [B, R])."""
    n_anchors = anchors.shape[0]
    B, R, H, W, C = _check_inputs("rpn_targets", cls, prob, None, None, n_anchors, feat_size)
    ctx = _Ctx(anchors, conf_vec, gt_table, feat_size, B, R, cls.device)
    return _targets(ctx, cls.detach(), prob.detach())


class _RpnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cls, bbox_2d, bbox_3d, prob, state):
        labels, gt_index, targets, scores = _targets(state, cls, prob)
        loss, stats, sampled, grads = _loss(state, cls, bbox_2d, bbox_3d, labels, targets, scores)
        ctx.save_for_backward(*grads)
        state.out = dict(labels=labels, gt_index=gt_index, targets=targets, scores=scores, sampled=sampled, stats=stats, grads=grads)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        out = []
        for g, need in zip(ctx.saved_tensors, ctx.needs_input_grad[:3]):
            out.append(g * grad_loss if need else None)
        return tuple(out) + (None, None)


def rpn_loss(cls, prob, bbox_2d, bbox_3d, anchors, conf_vec, gt_table, feat_size, return_details=False):
    """The loss layer below RPN_3D_loss: (loss 0-d float32 device tensor with grad_fn, stats float64 device tensor [16] in the
    order of STAT_NAMES); ``return_details`` adds a dict with labels, gt_index, targets, scores, sampled and the stored gradients."""
    n_anchors = anchors.shape[0]
    B, R, H, W, C = _check_inputs("rpn_loss", cls, prob, bbox_2d, bbox_3d, n_anchors, feat_size)
    state = _Ctx(anchors, conf_vec, gt_table, feat_size, B, R, cls.device)
    loss, stats = _RpnLoss.apply(cls, bbox_2d, bbox_3d, prob.detach(), state)
    return (loss, stats, state.out) if return_details else (loss, stats)


def stats_list(block, cls_2d_lambda, bbox_2d_lambda, bbox_3d_lambda, iou_2d_lambda):
    """The reference's stats list (entries, order, presence rules: lib/loss/rpn_3d.py:405-654) from a downloaded stat block."""
    s = dict(zip(STAT_NAMES, [float(v) for v in block]))
    out = []
    if cls_2d_lambda and s["n_fg"] > 0:
        out.append({'name': 'fg', 'val': s["acc_fg"], 'format': '{:0.2f}', 'group': 'acc'})
    if cls_2d_lambda and s["n_bg"] > 0:
        out.append({'name': 'bg', 'val': s["acc_bg"], 'format': '{:0.2f}', 'group': 'acc'})
    if cls_2d_lambda and s["n_active"] > 0:
        out.append({'name': 'cls', 'val': s["cls"], 'format': '{:0.4f}', 'group': 'loss'})
    if s["fg_num"] > 0:
        if bbox_2d_lambda:
            out.append({'name': 'bbox_2d', 'val': s["bbox_2d"], 'format': '{:0.4f}', 'group': 'loss'})
        if bbox_3d_lambda:
            out.append({'name': 'bbox_3d', 'val': s["bbox_3d"], 'format': '{:0.4f}', 'group': 'loss'})
        out.append({'name': 'z', 'val': s["z"], 'format': '{:0.2f}', 'group': 'misc'})
        out.append({'name': 'ry', 'val': s["ry"], 'format': '{:0.2f}', 'group': 'misc'})
        out.append({'name': 'iou', 'val': s["iou_acc"], 'format': '{:0.2f}', 'group': 'acc'})
        if iou_2d_lambda:
            out.append({'name': 'iou', 'val': s["iou_loss"], 'format': '{:0.4f}', 'group': 'loss'})
    return out


class RPN_3D_loss(nn.Module):
    """Drop-in for lib/loss/rpn_3d.py: RPN_3D_loss -- same constructor fields, same ``forward`` signature and return."""

    def __init__(self, conf):
        super(RPN_3D_loss, self).__init__()
        self.num_classes = len(conf.lbls) + 1
        self.num_anchors = conf.anchors.shape[0]
        self.anchors = conf.anchors
        self.bbox_means = conf.bbox_means
        self.bbox_stds = conf.bbox_stds
        self.feat_stride = conf.feat_stride
        self.fg_fraction = conf.fg_fraction
        self.box_samples = conf.box_samples
        self.ign_thresh = conf.ign_thresh
        self.nms_thres = conf.nms_thres
        self.fg_thresh = conf.fg_thresh
        self.bg_thresh_lo = conf.bg_thresh_lo
        self.bg_thresh_hi = conf.bg_thresh_hi
        self.best_thresh = conf.best_thresh
        self.hard_negatives = conf.hard_negatives
        self.focal_loss = conf.focal_loss
        self.crop_size = conf.crop_size
        self.cls_2d_lambda = conf.cls_2d_lambda
        self.iou_2d_lambda = conf.iou_2d_lambda
        self.bbox_2d_lambda = conf.bbox_2d_lambda
        self.bbox_3d_lambda = conf.bbox_3d_lambda
        self.bbox_3d_proj_lambda = conf.bbox_3d_proj_lambda
        self.lbls = conf.lbls
        self.ilbls = conf.ilbls
        self.min_gt_vis = conf.min_gt_vis
        self.min_gt_h = conf.min_gt_h
        self.max_gt_h = conf.max_gt_h
        self.device = conf.device
        self._anchors_dev = None
        self.last = None          # details of the last call (labels, sampled, ...): a dict of device tensors
        self._check_settings()

    def _check_settings(self):
        if self.bbox_3d_proj_lambda:
            raise NotImplementedError("RPN_3D_loss: bbox_3d_proj_lambda != 0 is not supported (the reference's own branch mixes host "
                                      "and device tensors)")
        if not self.hard_negatives and not math.isinf(float(self.box_samples)):
            raise NotImplementedError("RPN_3D_loss: random sampling (hard_negatives=False with a finite box_samples) is not supported: "
                                      "it draws from numpy's global RNG stream")

    def forward(self, cls, prob, bbox_2d, bbox_3d, imobjs, feat_size):
        self._check_settings()
        ops._require_cuda(cls, prob, bbox_2d, bbox_3d)
        if cls.shape[2] != self.num_classes:
            raise RuntimeError("RPN_3D_loss: cls has %d classes, conf.lbls gives %d" % (cls.shape[2], self.num_classes))
        if len(imobjs) != cls.shape[0]:
            raise RuntimeError("RPN_3D_loss: %d imobjs for a batch of %d" % (len(imobjs), cls.shape[0]))
        if self._anchors_dev is None or self._anchors_dev.device != cls.device:
            a = self.anchors.detach().cpu().numpy() if torch.is_tensor(self.anchors) else np.asarray(self.anchors)
            self._anchors_dev = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(cls.device)
        table = pack_gts(imobjs, self.lbls, self.ilbls, self.min_gt_vis, self.min_gt_h)
        vec = pack_conf(self.bbox_means, self.bbox_stds, self.fg_thresh, self.ign_thresh, self.bg_thresh_lo, self.bg_thresh_hi,
                        self.best_thresh, self.box_samples, self.fg_fraction, self.focal_loss, self.cls_2d_lambda, self.iou_2d_lambda,
                        self.bbox_2d_lambda, self.bbox_3d_lambda, self.feat_stride)
        loss, stats, self.last = rpn_loss(cls, prob, bbox_2d, bbox_3d, self._anchors_dev, vec, table, feat_size, return_details=True)
        block = stats.cpu().numpy()                                            # the one download
        return loss, stats_list(block, self.cls_2d_lambda, self.bbox_2d_lambda, self.bbox_3d_lambda, self.iou_2d_lambda)


class RPN_3D_loss_smp(nn.Module):
    def __init__(self, conf):
        super(RPN_3D_loss_smp, self).__init__()
        raise NotImplementedError("RPN_3D_loss_smp is not supported: it consumes the targets the reference's data loader pre-computes")
