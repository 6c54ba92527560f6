"""Training input path on the device: the reference's ``lib.augmentations.Augmentation`` for a whole batch.

The reference's loader runs ``Augmentation(conf)`` per image in its worker processes (lib/dataloader.py:896,939-950): photometric
distortion, ``RandomMirror``, ``RandomTransform`` (a scale-and-shift ``cv2.warpAffine`` to ``crop_size``), ``Normalize``, the
ground-truth rewrite that goes with the mirror and the warp, then BGR->RGB and HWC->CHW.  Here the work is split by where it belongs:

``draw_params(conf, frame_sizes, rng)``      the random decisions, drawn in the reference's order with its comparisons (host)
``transform_labels(imobj, params)``          the ground-truth rewrite in float64 numpy, quirks included (host)
``augment_batch(frames, params, size, ..)``  the pixels: uint8 BGR frames -> float32 RGB planes, one launch (m3d_augment_u8)
``TrainAugmentation(conf)``                  the three together: ``x, imobjs_aug = aug(frames, imobjs)``

Two differences from a real ``cv2`` are documented in DESIGN.md section 7: the bilinear taps sit at the exact source coordinate
(``warpAffine`` rounds it to 1/32 pixel), and the float HSV formulas are OpenCV's as documented, not checked against a binary.
"""
import copy
import ctypes
import math

import numpy as np
import torch

from .. import _hip

MODE_NONE, MODE_CONTRAST_FIRST, MODE_CONTRAST_LAST = 0, 1, 2
PARAM_COLS = _hip.CONSTANTS["M3D_AUGMENT_PARAMS"]        # 14: h w mode delta alpha sat hue - Minv[6]
# PhotometricDistort's ranges (augmentations.py:243,266,308,380)
BRIGHTNESS_DELTA, CONTRAST_RANGE, SATURATION_RANGE, HUE_DELTA = 32, (0.5, 1.5), (0.5, 1.5), 18.0


def _has(o, k):
    return (k in o) if isinstance(o, dict) else hasattr(o, k)


def _get(o, k):
    return o[k] if isinstance(o, dict) else getattr(o, k)


def _set(o, k, v):
    if isinstance(o, dict):
        o[k] = v
    else:
        setattr(o, k, v)


def rotation_matrix(centre, scale):
    """``cv2.getRotationMatrix2D(centre, 0, scale)`` in float64: [[s, 0, (1 - s) cx], [0, s, (1 - s) cy]]."""
    cx, cy, s = float(centre[0]), float(centre[1]), float(scale)
    return np.array([[s, 0.0, (1.0 - s) * cx], [0.0, s, (1.0 - s) * cy]], dtype=np.float64)


def invert_affine(M):
    """Inverse of a 2x3 affine map in float64, in the order ``cv2.warpAffine`` inverts its argument."""
    M = np.asarray(M, dtype=np.float64)
    det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    d = 1.0 / det if det != 0 else 0.0
    a11, a22 = M[1, 1] * d, M[0, 0] * d
    a12, a21 = M[0, 1] * -d, M[1, 0] * -d
    b1 = -a11 * M[0, 2] - a12 * M[1, 2]
    b2 = -a21 * M[0, 2] - a22 * M[1, 2]
    return np.array([[a11, a12, b1], [a21, a22, b2]], dtype=np.float64)


def draw_params(conf, frame_sizes, rng=None):
    """One parameter dict per ``(h, w)`` of ``frame_sizes``, drawn from ``rng`` (``np.random.RandomState``; None: the global
    ``np.random``) in the order and with the comparisons of ``Augmentation(conf)`` called for one image after another
    (augmentations.py:164-234,393-469: ``<=`` for the photometric and mirror coins, ``<`` for the transform)."""
    rng = np.random if rng is None else rng
    distort_prob, mirror_prob, trans_prob = conf["distort_prob"], conf["mirror_prob"], conf["trans_prob"]
    shift, scale_trans = conf["shift"], conf["scale_trans"]
    out = []
    for h, w in frame_sizes:
        h, w = int(h), int(w)
        mode, delta, alpha, sat, hue = MODE_NONE, 0.0, 1.0, 1.0, 0.0
        if distort_prob > 0:
            first = rng.rand() <= 0.5
            mode = MODE_CONTRAST_FIRST if first else MODE_CONTRAST_LAST
            if rng.rand() <= distort_prob:
                delta = rng.uniform(-BRIGHTNESS_DELTA, BRIGHTNESS_DELTA)
            if first and rng.rand() <= distort_prob:
                alpha = rng.uniform(*CONTRAST_RANGE)
            if rng.rand() <= distort_prob:
                sat = rng.uniform(*SATURATION_RANGE)
            if rng.rand() <= distort_prob:
                hue = rng.uniform(-HUE_DELTA, HUE_DELTA)
            if not first and rng.rand() <= distort_prob:
                alpha = rng.uniform(*CONTRAST_RANGE)
        mirror = bool(rng.rand() <= mirror_prob)
        warped = bool(rng.rand() < trans_prob)
        if warped:
            scale = np.clip(rng.randn() * scale_trans, -scale_trans, scale_trans) + 1
            cx = w * (0.5 + np.clip(rng.randn() * shift, -2 * shift, 2 * shift))
            cy = h * (0.5 + np.clip(rng.randn() * shift, -2 * shift, 2 * shift))
        else:
            scale, cx, cy = 1.0, w * 0.5, h * 0.5
        out.append(make_params(h, w, mode=mode, delta=delta, alpha=alpha, sat=sat, hue=hue, mirror=mirror, warped=warped,
                               scale=scale, centre=(cx, cy)))
    return out


def make_params(h, w, mode=MODE_NONE, delta=0.0, alpha=1.0, sat=1.0, hue=0.0, mirror=False, warped=False, scale=1.0, centre=None):
    """The parameter dict of one image from explicit values (``draw_params`` draws them).  ``M`` is the forward matrix the labels
    go through; ``Minv`` is its float64 inverse with the mirror folded in (x_src = (w - 1) - u), the one matrix the kernel needs."""
    cx, cy = (w * 0.5, h * 0.5) if centre is None else centre
    M = rotation_matrix((cx, cy), scale)
    Minv = invert_affine(M)
    if mirror:
        Minv[0] = [-Minv[0, 0], -Minv[0, 1], (w - 1) - Minv[0, 2]]
    return dict(h=int(h), w=int(w), mode=int(mode), delta=float(delta), alpha=float(alpha), sat=float(sat), hue=float(hue),
                mirror=bool(mirror), warped=bool(warped), scale=scale, centre=(cx, cy), M=M, Minv=Minv)


def pack_params(params):
    """float64 [B, PARAM_COLS]: the rows m3d_augment_u8 reads."""
    rows = np.zeros((len(params), PARAM_COLS), dtype=np.float64)
    for i, p in enumerate(params):
        rows[i, :7] = [p["h"], p["w"], p["mode"], p["delta"], p["alpha"], p["sat"], p["hue"]]
        rows[i, 8:14] = np.asarray(p["Minv"], dtype=np.float64).reshape(6)
    return rows


def _wrap_pi(a):
    while a > math.pi:
        a -= math.pi * 2
    while a < (-math.pi):
        a += math.pi * 2
    return a


def _rot_to_alpha(ry3d, z3d, x3d):          # lib/util.py:527-535
    return _wrap_pi(ry3d - math.atan2(-z3d, x3d) - 0.5 * math.pi)


def _alpha_to_rot(alpha, z3d, x3d):         # lib/util.py:516-524
    return _wrap_pi(alpha + math.atan2(-z3d, x3d) + 0.5 * math.pi)


def _affine_point(pt, M):
    """lib/util.py:537-540: the point is cast to float32 before it meets the float64 matrix."""
    return np.dot(M, np.array([pt[0], pt[1], 1.], dtype=np.float32).T)[:2]


def transform_labels(imobj, params):
    """A deep copy of ``imobj`` with ``gts`` rewritten as RandomMirror and RandomTransform rewrite them (augmentations.py:199-232,
    343-369) and ``scale_factor`` set.  The reference's quirks are kept: the mirror uses the SOURCE width, recomputes ``rotY`` and
    ``alpha`` but leaves the 3-D centre ``bbox_3d[7:10]`` stale; the warp touches the labels only when its coin fired."""
    imobj = copy.deepcopy(imobj)
    gts = _get(imobj, "gts") if _has(imobj, "gts") else None
    if params["mirror"]:
        width = params["w"]
        p2_inv = _get(imobj, "p2_inv")
        for gt in gts:
            if _has(gt, "bbox_full"):
                b = _get(gt, "bbox_full")
                b[0] = width - b[0] - b[2]
            if _has(gt, "bbox_vis"):
                b = _get(gt, "bbox_vis")
                b[0] = width - b[0] - b[2]
            if _has(gt, "bbox_3d"):
                b3 = _get(gt, "bbox_3d")
                b3[0] = width - b3[0] - 1
                rot_y = b3[10]
                rot_y = _wrap_pi((-math.pi - rot_y) if rot_y < 0 else (math.pi - rot_y))
                cx, cy, cz = b3[0], b3[1], b3[2]
                c3 = p2_inv.dot(np.array([cx * cz, cy * cz, cz, 1]))
                b3[10] = rot_y
                b3[6] = _rot_to_alpha(rot_y, c3[2], c3[0])
    scale = params["scale"]
    _set(imobj, "scale_factor", scale)
    if gts is not None and params["warped"]:
        M = params["M"]
        p2_inv = _get(imobj, "p2_inv")
        for gt in gts:
            if _has(gt, "bbox_full"):
                b = _get(gt, "bbox_full")
                b[2:4] *= scale
                b[0:2] = _affine_point(b[0:2], M)
            if _has(gt, "bbox_vis"):
                b = _get(gt, "bbox_vis")
                b *= scale
            if _has(gt, "bbox_3d"):
                b3 = _get(gt, "bbox_3d")
                cx, cy = _affine_point(b3[0:2], M)
                cz = b3[2] / scale
                b3[0:3] = [cx, cy, cz]
                x3, y3, z3, _ = p2_inv.dot(np.array([cx * cz, cy * cz, 1 * cz, 1]))
                _set(gt, "center_3d", [x3, y3, z3])
                b3[7:10] = [x3, y3, z3]
                b3[10] = _alpha_to_rot(b3[6], z3, x3)
    return imobj


def _validate(rows, hmax, wmax):
    if not np.isfinite(rows).all():
        raise RuntimeError("augment_batch: a parameter is not finite")
    if (rows[:, 0] < 1).any() or (rows[:, 1] < 1).any() or (rows[:, 0] > hmax).any() or (rows[:, 1] > wmax).any():
        raise RuntimeError("augment_batch: a per-image size does not fit the %dx%d frame buffer" % (hmax, wmax))
    if (rows[:, 8] * rows[:, 12] - rows[:, 9] * rows[:, 11] == 0).any():
        raise RuntimeError("augment_batch: singular matrix")


def augment_batch(frames, params, size, mean, stds, device=None):
    """frames: uint8 [B, hmax, wmax, 3] BGR; image i occupies the top-left ``params[i]['h'] x params[i]['w']`` of its slot, so
    KITTI's mixed frame sizes share one buffer.  A ROCm tensor is used as it is; a host tensor goes through pinned staging to
    ``device`` (default: the current ROCm device).  Returns float32 [B, 3, size[0], size[1]] RGB planes on the device."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise RuntimeError("augment_batch: uint8 [B, hmax, wmax, 3] frames expected")
    B, hmax, wmax, _ = frames.shape
    if B < 1 or len(params) != B:
        raise RuntimeError("augment_batch: %d frames, %d parameter sets" % (B, len(params)))
    if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
        raise RuntimeError("augment_batch: size is (height, width)")
    rows = pack_params(params)
    _validate(rows, hmax, wmax)
    dev = frames.device if frames.is_cuda else torch.device("cuda" if device is None else device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise NotImplementedError("augment_batch: ROCm destination expected (no CPU path)")      # same stance as preprocess
    if not frames.is_cuda:
        frames = (frames if frames.is_pinned() else frames.contiguous().pin_memory()).to(dev, non_blocking=True)
    frames = frames.contiguous()
    H, W = int(size[0]), int(size[1])
    out = torch.empty(B, 3, H, W, device=frames.device, dtype=torch.float32)
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in stds])
    with torch.cuda.device(frames.device):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _hip.check(_hip.lib().m3d_augment_u8(frames.data_ptr(), B, hmax, wmax, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                             PARAM_COLS, m3, s3, out.data_ptr(), H, W, st))
    return out


class TrainAugmentation(object):
    """``Augmentation(conf)`` for a batch: ``x, imobjs_aug = aug(frames, imobjs, rng=None)``.  ``frames`` as ``augment_batch`` takes
    them; the per-image sizes come from ``imobjs[i].imH / imW`` where present, else every frame fills its slot.  ``imobjs_aug``
    goes straight into ``RPN_3D_loss.forward`` or ``pack_gts`` -> ``rpn_precompute_targets``."""

    def __init__(self, conf):
        self.conf = conf
        self.size = [int(v) for v in conf["crop_size"]]
        self.mean, self.stds = list(conf["image_means"]), list(conf["image_stds"])
        self.device = conf["device"] if "device" in conf else None

    def __call__(self, frames, imobjs, rng=None, frame_sizes=None):
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
            raise RuntimeError("TrainAugmentation: uint8 [B, hmax, wmax, 3] frames expected")
        if len(imobjs) != frames.shape[0]:
            raise RuntimeError("TrainAugmentation: %d frames, %d imobjs" % (frames.shape[0], len(imobjs)))
        if frame_sizes is None:
            frame_sizes = [(_get(o, "imH"), _get(o, "imW")) if _has(o, "imH") and _has(o, "imW") else frames.shape[1:3] for o in imobjs]
        params = draw_params(self.conf, frame_sizes, rng)
        x = augment_batch(frames, params, self.size, self.mean, self.stds, device=self.device)
        return x, [transform_labels(o, p) for o, p in zip(imobjs, params)]
