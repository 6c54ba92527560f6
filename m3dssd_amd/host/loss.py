"""RPN_3D_loss (lib/loss/rpn_3d.py:14-657) and RPN_3D_loss_smp (lib/loss/rpn_3d.py:659-1360) on the HIP library.

The reference copies ``prob`` to the host, assigns targets and samples in numpy one image at a time and uploads sixteen
``[B, R]`` arrays again.  Here the host part is what concerns a few dozen ground-truth boxes -- ``determine_ignores``, the class
lookup and the XYWH -> corner conversion (``pack_gts``) -- and one packed table is uploaded per call.  Target assignment
(``compute_targets``, lib/rpn_util.py:430-532), the hard-negative selection and the loss with its gradients run in
m3d_rpn_targets / m3d_rpn_loss (csrc/rpn_loss.hip); one small stat block is downloaded after the last launch for the ``stats``
list.  ``loss`` stays on the device and carries a ``grad_fn``: the gradients with respect to ``cls``, ``bbox_2d`` and ``bbox_3d``
were written by the same launch and are handed to autograd in ``backward`` (scaled when ``grad_output`` is not 1).

RPN_3D_loss_smp is the criterion the training script binds when ``conf.pre_compute_target`` is set (all shipped
configurations): its fifth argument is the collated ``batch['target']`` dict the data loader assigned per image
(``Kitti_Dataset_torch._targets``, lib/dataloader.py:1014-1160), not a list of imobjs.  Here it reads ``labels`` (int64 or
int16), ``bbox_2d``, ``bbox_3d`` and ``meta['any_val']`` from that dict -- host tensors are uploaded through pinned staging --
and m3d_rpn_loss_smp validates the labels, gathers the sampling scores and counts on the device, then runs the select / loss /
finish launches of m3d_rpn_loss unchanged.  ``rpn_precompute_targets`` (m3d_rpn_precompute_targets) is the device form of
``_targets``: the same dict, made ahead of the forward from the packed gt table.  ``labels_fg`` / ``labels_bg`` /
``labels_ign`` and ``meta['rois']`` are functions of ``labels`` and ``conf.anchors`` and are not read.

Not supported (NotImplementedError): ``bbox_3d_proj_lambda != 0`` (the reference's branch mixes host and device tensors) and
random sampling (``hard_negatives=False`` with a finite ``box_samples``: it draws from a global RNG stream).  Host ``cls`` /
``prob`` / ``bbox_*``: NotImplementedError, no CPU fallback.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from . import ops

_C = _hip.CONSTANTS          # the header's #defines and enumerators
MAX_GT, GT_COLS, CONF_COUNT = _C["M3D_RPN_MAX_GT"], _C["M3D_RPN_GT_COLS"], _C["M3D_RPN_CONF_COUNT"]
# "loss", "cls", "bbox_2d", ...: the slots of the stat block, M3D_RPN_STAT_* in value order
STAT_NAMES = tuple(n[len("M3D_RPN_STAT_"):].lower() for n in sorted(_C, key=_C.get)
                   if n.startswith("M3D_RPN_STAT_") and n != "M3D_RPN_STAT_COUNT")
SMP_STAT_BAD_LABELS = _C["M3D_RPN_SMP_STAT_BAD_LABELS"]          # the stat block of m3d_rpn_loss_smp has one more slot
SMP_STAT_COUNT = _C["M3D_RPN_SMP_STAT_COUNT"]
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
    """Device-side state shared by rpn_targets and rpn_loss: anchors, settings, gt table (None: pre-computed targets), workspace."""

    def __init__(self, anchors, conf_vec, gt_table, feat_size, B, R, device):
        L = _hip.lib()
        self.anchors = anchors if torch.is_tensor(anchors) else \
            torch.from_numpy(np.ascontiguousarray(np.asarray(anchors, dtype=np.float64))).to(device)
        if self.anchors.dtype != torch.float64 or self.anchors.dim() != 2 or self.anchors.shape[1] != 9 or not self.anchors.is_cuda:
            raise RuntimeError("rpn_loss: anchors must be [A, 9] (x1 y1 x2 y2 z w h l ry)")
        self.conf = np.ascontiguousarray(conf_vec, dtype=np.float64)
        self.H, self.W = int(feat_size[0]), int(feat_size[1])
        self.A = int(self.anchors.shape[0])
        nbytes = L.m3d_rpn_loss_workspace_bytes(B, R)
        self.ws = torch.empty(nbytes + 256, device=device, dtype=torch.uint8)
        self.ws_base = (self.ws.data_ptr() + 255) // 256 * 256
        self.ws_bytes = nbytes
        if gt_table is None:
            self.gt, self.Gmax = None, 0
            return
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


def _conf_fields(self, conf):
    """The constructor fields both reference classes carry."""
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


class RPN_3D_loss(nn.Module):
    """Drop-in for lib/loss/rpn_3d.py: RPN_3D_loss -- same constructor fields, same ``forward`` signature and return."""

    def __init__(self, conf):
        super(RPN_3D_loss, self).__init__()
        _conf_fields(self, conf)
        self._anchors_dev = None
        self.last = None          # details of the last call (labels, sampled, ...): a dict of device tensors
        self._check_settings()

    def _check_settings(self):
        who = type(self).__name__
        if self.bbox_3d_proj_lambda:
            raise NotImplementedError(who + ": bbox_3d_proj_lambda != 0 is not supported (the reference's own branch mixes host "
                                      "and device tensors)")
        if not self.hard_negatives and not math.isinf(float(self.box_samples)):
            raise NotImplementedError(who + ": random sampling (hard_negatives=False with a finite box_samples) is not supported: "
                                      "it draws from a global RNG stream")

    def _upload_anchors(self, device):
        if self._anchors_dev is None or self._anchors_dev.device != device:
            a = self.anchors.detach().cpu().numpy() if torch.is_tensor(self.anchors) else np.asarray(self.anchors)
            self._anchors_dev = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)

    def _conf_vec(self):
        return pack_conf(self.bbox_means, self.bbox_stds, self.fg_thresh, self.ign_thresh, self.bg_thresh_lo, self.bg_thresh_hi,
                         self.best_thresh, self.box_samples, self.fg_fraction, self.focal_loss, self.cls_2d_lambda, self.iou_2d_lambda,
                         self.bbox_2d_lambda, self.bbox_3d_lambda, self.feat_stride)

    def forward(self, cls, prob, bbox_2d, bbox_3d, imobjs, feat_size):
        self._check_settings()
        ops._require_cuda(cls, prob, bbox_2d, bbox_3d)
        if cls.shape[2] != self.num_classes:
            raise RuntimeError("RPN_3D_loss: cls has %d classes, conf.lbls gives %d" % (cls.shape[2], self.num_classes))
        if len(imobjs) != cls.shape[0]:
            raise RuntimeError("RPN_3D_loss: %d imobjs for a batch of %d" % (len(imobjs), cls.shape[0]))
        self._upload_anchors(cls.device)
        table = pack_gts(imobjs, self.lbls, self.ilbls, self.min_gt_vis, self.min_gt_h)
        vec = self._conf_vec()
        loss, stats, self.last = rpn_loss(cls, prob, bbox_2d, bbox_3d, self._anchors_dev, vec, table, feat_size, return_details=True)
        block = stats.cpu().numpy()                                            # the one download
        return loss, stats_list(block, self.cls_2d_lambda, self.bbox_2d_lambda, self.bbox_3d_lambda, self.iou_2d_lambda)


# ---- pre-computed targets: rpn_precompute_targets, rpn_loss_smp, RPN_3D_loss_smp ---------------------------------------------
def rpn_precompute_targets(anchors, conf_vec, gt_table, feat_size, device):
    """``Kitti_Dataset_torch._targets`` for a whole batch on the device (m3d_rpn_precompute_targets: launches 1-3 without cls /
    prob).  Returns the target dict of rpn_loss_smp: labels, gt_index int16 [B, R]; bbox_2d float32 [B, R, 4]; bbox_3d float32
    [B, R, 7]; meta: {any_val int32 [B]}.  The bits are those of rpn_targets; rows that are not fg carry (0 - mean) / std."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise NotImplementedError("rpn_precompute_targets: device=%s: no CPU fallback" % (device,))
    L = _hip.lib()
    gt_table = np.asarray(gt_table)
    B = int(gt_table.shape[0])
    R = int(anchors.shape[0]) * int(feat_size[0]) * int(feat_size[1])
    ctx = _Ctx(anchors, conf_vec, gt_table, feat_size, B, R, dev)
    if ctx.min_label < 1:
        raise RuntimeError("rpn_precompute_targets: gt class labels must be >= 1 (got %d)" % ctx.min_label)
    labels = torch.empty(B, R, device=dev, dtype=torch.int16)
    gt_index = torch.empty(B, R, device=dev, dtype=torch.int16)
    b2t = torch.empty(B, R, 4, device=dev, dtype=torch.float32)
    b3t = torch.empty(B, R, 7, device=dev, dtype=torch.float32)
    any_val = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _hip.check(L.m3d_rpn_precompute_targets(ctx.anchors.data_ptr(), ctx.A, ctx.H, ctx.W, ctx.conf_ptr(), CONF_COUNT, ctx.gt.data_ptr(),
                                                B, ctx.Gmax, labels.data_ptr(), gt_index.data_ptr(), b2t.data_ptr(), b3t.data_ptr(),
                                                any_val.data_ptr(), ctx.ws_base, ctx.ws_bytes, ops._stream()))
    return dict(labels=labels, gt_index=gt_index, bbox_2d=b2t, bbox_3d=b3t, meta=dict(any_val=any_val))


TARGET_STATS_COLS = _C["M3D_RPN_TARGET_STATS_COLS"]          # n_fg, 11 sums, 11 sums of squares


def rpn_target_stats(anchors, conf_vec, gt_table, feat_size, center=None, device="cuda:0"):
    """What ``compute_bbox_stats`` (lib/rpn_util.py:732-889) needs of ``compute_targets``, per image, on the device
    (m3d_rpn_target_stats): float64 [B, 23] = n_fg, sum(t - center) and sum((t - center)^2) of the 11 raw float32 transforms over
    the fg rows.  The anchor boxes stay float64 (the reference's statistics do not cast them; its loss does).  ``center``:
    11 values, default zeros.  Of ``conf_vec`` only the thresholds and the stride are read."""
    dev = anchors.device if torch.is_tensor(anchors) else torch.device(device)
    if dev.type != "cuda":
        raise NotImplementedError("rpn_target_stats: device=%s: no CPU fallback" % (dev,))
    L = _hip.lib()
    anc = anchors if torch.is_tensor(anchors) else torch.from_numpy(np.ascontiguousarray(np.asarray(anchors, dtype=np.float64))).to(dev)
    if anc.dtype != torch.float64 or anc.dim() != 2 or anc.shape[1] != 9 or not anc.is_contiguous():
        raise RuntimeError("rpn_target_stats: anchors must be float64 [A, 9] (x1 y1 x2 y2 z w h l ry)")
    gt_table = np.ascontiguousarray(gt_table, dtype=np.float64)
    if gt_table.ndim != 3 or gt_table.shape[2] != GT_COLS or gt_table.shape[1] < 1 or gt_table.shape[0] < 1:
        raise RuntimeError("rpn_target_stats: gt table must be [B, Gmax + 1, %d] (got %s)" % (GT_COLS, gt_table.shape))
    if (gt_table[:, 0, :2] < 0).any() or (gt_table[:, 0, 0] + gt_table[:, 0, 1] > gt_table.shape[1] - 1).any():
        raise RuntimeError("rpn_target_stats: gt table counts exceed its rows")
    B, Gmax = int(gt_table.shape[0]), int(gt_table.shape[1]) - 1
    H, W = int(feat_size[0]), int(feat_size[1])
    A = int(anc.shape[0])
    vec = np.ascontiguousarray(conf_vec, dtype=np.float64)
    c = np.zeros(11, dtype=np.float64) if center is None else np.ascontiguousarray(np.asarray(center, dtype=np.float64).reshape(-1))
    if c.size != 11:
        raise RuntimeError("rpn_target_stats: center must hold 11 values (got %d)" % c.size)
    nbytes = L.m3d_rpn_target_stats_workspace_bytes(B, A * H * W)
    ws = torch.empty(max(nbytes, 0) + 256, device=dev, dtype=torch.uint8)
    ws_base = (ws.data_ptr() + 255) // 256 * 256
    gt = torch.from_numpy(gt_table).to(dev)
    cen = torch.from_numpy(c).to(dev)
    out = torch.empty(B, TARGET_STATS_COLS, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _hip.check(L.m3d_rpn_target_stats(anc.data_ptr(), A, H, W, vec.ctypes.data, int(vec.size), gt.data_ptr(), B, Gmax,
                                          cen.data_ptr(), out.data_ptr(), ws_base, nbytes, ops._stream()))
    return out


def _upload(t, device):
    """A device tensor as it is; a host tensor through pinned memory (staged where it is not pinned already)."""
    if t.is_cuda:
        if t.device != device:
            raise RuntimeError("rpn_loss_smp: a target tensor lives on %s, cls on %s" % (t.device, device))
        return t
    return (t if t.is_pinned() else t.pin_memory()).to(device, non_blocking=True)


def _target_tensors(target, B, R, device):
    """(labels int64 | int16 [B, R], bbox_2d [B, R, 4], bbox_3d [B, R, 7], any_val int32 [B]) on ``device`` from the target dict.
    Checked before anything is uploaded."""
    who = "rpn_loss_smp"
    if not isinstance(target, dict):
        raise RuntimeError("%s: the target must be the dict the data loader collates (labels, bbox_2d, bbox_3d, meta['any_val']), "
                           "got %s" % (who, type(target).__name__))
    for k in ("labels", "bbox_2d", "bbox_3d", "meta"):
        if k not in target:
            raise RuntimeError("%s: the target dict has no '%s'" % (who, k))
    if not isinstance(target["meta"], dict) or "any_val" not in target["meta"]:
        raise RuntimeError("%s: the target dict has no meta['any_val']" % who)
    want = {"labels": ((B, R), (torch.int64, torch.int16)), "bbox_2d": ((B, R, 4), (torch.float32,)), "bbox_3d": ((B, R, 7), (torch.float32,))}
    for k, (shape, dtypes) in want.items():
        t = target[k]
        if not torch.is_tensor(t):
            raise RuntimeError("%s: target['%s'] must be a tensor (got %s)" % (who, k, type(t).__name__))
        if tuple(t.shape) != shape:
            raise RuntimeError("%s: target['%s'] has shape %s; expected %s" % (who, k, tuple(t.shape), shape))
        if t.dtype not in dtypes:
            raise RuntimeError("%s: target['%s'] must be %s (got %s)" % (who, k, " or ".join(str(d) for d in dtypes), t.dtype))
        if not t.is_contiguous():
            raise RuntimeError("%s: target['%s'] must be contiguous" % (who, k))
    # functions of labels / conf.anchors: not read, but a wrong shape means the dict belongs to another batch
    for k in ("labels_fg", "labels_bg", "labels_ign"):
        if k in target and tuple(target[k].shape) != (B, R):
            raise RuntimeError("%s: target['%s'] has shape %s; expected %s" % (who, k, tuple(target[k].shape), (B, R)))
    rois = target["meta"].get("rois")
    if rois is not None and (rois.dim() != 3 or rois.shape[0] != B or rois.shape[1] != R):
        raise RuntimeError("%s: target['meta']['rois'] has shape %s; expected [%d, %d, 5]" % (who, tuple(rois.shape), B, R))
    any_val = target["meta"]["any_val"]
    any_val = any_val if torch.is_tensor(any_val) else torch.as_tensor(np.asarray(any_val))
    if tuple(any_val.shape) != (B,) or any_val.dtype.is_floating_point:
        raise RuntimeError("%s: target['meta']['any_val'] must hold %d integers (got %s %s)" % (who, B, any_val.dtype, tuple(any_val.shape)))
    any_val = _upload(any_val.contiguous(), device).to(torch.int32)
    return _upload(target["labels"], device), _upload(target["bbox_2d"], device), _upload(target["bbox_3d"], device), any_val


def _loss_smp(ctx, cls, prob, bbox_2d, bbox_3d, tgt):
    L = _hip.lib()
    B, R, C = cls.shape
    dev = cls.device
    labels_in, b2t, b3t, any_val = tgt
    labels = torch.empty(B, R, device=dev, dtype=torch.int16)
    targets = torch.empty(B, R, 11, device=dev, dtype=torch.float32)
    scores = torch.empty(B, R, device=dev, dtype=torch.float32)
    sampled = torch.empty(B, R, device=dev, dtype=torch.uint8)
    g_cls, g_2d, g_3d = torch.empty_like(cls), torch.empty_like(bbox_2d), torch.empty_like(bbox_3d)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    stats = torch.empty(SMP_STAT_COUNT, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _hip.check(L.m3d_rpn_loss_smp(ctx.anchors.data_ptr(), ctx.A, ctx.H, ctx.W, ctx.conf_ptr(), CONF_COUNT, B, labels_in.data_ptr(),
                                      labels_in.element_size(), b2t.data_ptr(), b3t.data_ptr(), any_val.data_ptr(), cls.data_ptr(),
                                      prob.data_ptr(), bbox_2d.data_ptr(), bbox_3d.data_ptr(), C, labels.data_ptr(), targets.data_ptr(),
                                      scores.data_ptr(), sampled.data_ptr(), g_cls.data_ptr(), g_2d.data_ptr(), g_3d.data_ptr(),
                                      loss.data_ptr(), stats.data_ptr(), ctx.ws_base, ctx.ws_bytes, ops._stream()))
    return loss, stats, dict(labels=labels, targets=targets, scores=scores, sampled=sampled, stats=stats, grads=(g_cls, g_2d, g_3d))


class _RpnLossSmp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cls, bbox_2d, bbox_3d, prob, state, tgt):
        loss, stats, state.out = _loss_smp(state, cls, prob, bbox_2d, bbox_3d, tgt)
        ctx.save_for_backward(*state.out["grads"])
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        out = []
        for g, need in zip(ctx.saved_tensors, ctx.needs_input_grad[:3]):
            out.append(g * grad_loss if need else None)
        return tuple(out) + (None, None, None)


def rpn_loss_smp(cls, prob, bbox_2d, bbox_3d, target, anchors, conf_vec, feat_size, return_details=False):
    """The loss layer below RPN_3D_loss_smp: (loss 0-d float32 device tensor with grad_fn, stats float64 device tensor [17]: the
    STAT_NAMES slots, then the count of labels outside {0, 1 .. C-1, 3000} -- such rows were treated as ignored; a caller that
    does not go through the module checks that slot).  ``return_details`` adds a dict with labels (int16), targets (packed
    [B, R, 11]), scores, sampled and the stored gradients."""
    n_anchors = anchors.shape[0]
    B, R, H, W, C = _check_inputs("rpn_loss_smp", cls, prob, bbox_2d, bbox_3d, n_anchors, feat_size)
    tgt = _target_tensors(target, B, R, cls.device)
    state = _Ctx(anchors, conf_vec, None, feat_size, B, R, cls.device)
    loss, stats = _RpnLossSmp.apply(cls, bbox_2d, bbox_3d, prob.detach(), state, tgt)
    return (loss, stats, state.out) if return_details else (loss, stats)


def stats_list_smp(block, cls_2d_lambda, bbox_3d_lambda, iou_2d_lambda):
    """The stats list of the reference's RPN_3D_loss_smp (entries, order, presence rules: lib/loss/rpn_3d.py:1099-1357) from a
    downloaded stat block: the 3-D term is named 'bbox3d', the 2-D term has no entry, 'ttloss' (the total) closes the fg branch.
    'bg' is present whenever the classification term is on (the reference tests the length of a 2-tuple, lib/loss/rpn_3d.py:1103),
    NaN -- its mean of nothing -- for a batch without a bg anchor."""
    s = dict(zip(STAT_NAMES, [float(v) for v in block]))
    out = []
    if cls_2d_lambda and s["n_fg"] > 0:
        out.append({'name': 'fg', 'val': s["acc_fg"], 'format': '{:0.2f}', 'group': 'acc'})
    if cls_2d_lambda:
        out.append({'name': 'bg', 'val': s["acc_bg"] if s["n_bg"] > 0 else float("nan"), 'format': '{:0.2f}', 'group': 'acc'})
    if cls_2d_lambda and s["n_active"] > 0:
        out.append({'name': 'cls', 'val': s["cls"], 'format': '{:0.4f}', 'group': 'loss'})
    if s["fg_num"] > 0:
        if bbox_3d_lambda:
            out.append({'name': 'bbox3d', 'val': s["bbox_3d"], 'format': '{:0.4f}', 'group': 'loss'})
        out.append({'name': 'z', 'val': s["z"], 'format': '{:0.2f}', 'group': 'misc'})
        out.append({'name': 'ry', 'val': s["ry"], 'format': '{:0.2f}', 'group': 'misc'})
        out.append({'name': 'iou', 'val': s["iou_acc"], 'format': '{:0.2f}', 'group': 'acc'})
        if iou_2d_lambda:
            out.append({'name': 'iou', 'val': s["iou_loss"], 'format': '{:0.4f}', 'group': 'loss'})
        out.append({'name': 'ttloss', 'val': s["loss"], 'format': '{:0.4f}', 'group': 'loss'})
    return out


class RPN_3D_loss_smp(RPN_3D_loss):
    """Drop-in for lib/loss/rpn_3d.py: RPN_3D_loss_smp -- same constructor fields, same ``forward`` signature and return; the
    fifth argument of ``forward`` is the target dict (the loader's collated batch['target'], host or device, or the dict of
    rpn_precompute_targets).  Nothing is uploaded before the first ``forward``.  Unlike the reference, the caller's ``bbox_2d``
    and the dict's ``bbox_2d`` are left as they are (the reference de-normalises both in place), and ``bbox_2d_lambda != 0``
    works (the reference raises NameError there) with the value RPN_3D_loss gives."""

    def __init__(self, conf):
        if torch.device(conf.device).type != "cuda":
            raise NotImplementedError("RPN_3D_loss_smp: conf.device=%s: no CPU fallback" % (conf.device,))
        super(RPN_3D_loss_smp, self).__init__(conf)

    def forward(self, cls, prob, bbox_2d, bbox_3d, imobjs, feat_size):
        self._check_settings()
        ops._require_cuda(cls, prob, bbox_2d, bbox_3d)
        if cls.shape[2] != self.num_classes:
            raise RuntimeError("RPN_3D_loss_smp: cls has %d classes, conf.lbls gives %d" % (cls.shape[2], self.num_classes))
        self._upload_anchors(cls.device)
        loss, stats, self.last = rpn_loss_smp(cls, prob, bbox_2d, bbox_3d, imobjs, self._anchors_dev, self._conf_vec(), feat_size,
                                              return_details=True)
        block = stats.cpu().numpy()                                            # the one download
        if block[SMP_STAT_BAD_LABELS]:
            raise RuntimeError("RPN_3D_loss_smp: %d labels are outside {0, 1 .. %d, %d}" % (int(block[SMP_STAT_BAD_LABELS]),
                                                                                            self.num_classes - 1, IGN_FLAG))
        return loss, stats_list_smp(block, self.cls_2d_lambda, self.bbox_3d_lambda, self.iou_2d_lambda)
