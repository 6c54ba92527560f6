"""numpy restatement of the image path of the reference's ``lib.augmentations.Augmentation`` (photometric distortion, mirror,
scale-and-shift warp, Normalize, BGR->RGB, HWC->CHW), parameterised by dtype: the float32 run mirrors the reference's own
precision, the float64 run is the truth the device kernel is measured against.  ``augment_image`` takes the parameter dict of
``m3dssd_amd.host.augment`` (the folded ``Minv``); this file does not import the package.

It also holds the numpy stand-ins for the three ``cv2`` calls on that path, which tools/gen_golden_augment.py installs as a stub
``cv2`` under the reference's own code (cv2 is not installed where the golden is generated):
``get_rotation_matrix_2d`` / ``warp_affine`` (bilinear at the EXACT source coordinate, constant border 0; a real warpAffine rounds
the coordinate to 1/32 pixel) / ``cvt_color`` (OpenCV's documented float BGR<->HSV forms, BGR->RGB).  Pixel agreement of these
formulas with a cv2 binary is NOT verified; this file is the contract for the pixels.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz")
FLT_EPSILON = float(np.finfo(np.float32).eps)
COLOR_BGR2RGB, COLOR_BGR2HSV, COLOR_HSV2BGR = 4, 40, 54
# (b, g, r) of each hue sector as indices into (v, v(1-s), v(1-s f), v(1-s(1-f)))
SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
MEAN, STDS = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


# ---------------------------------------------------------------------------------------------------------- colour
def bgr_to_hsv(img):
    """float BGR -> HSV, H in degrees: V = max, S = diff / (|V| + eps), H = (.) * (60 / (diff + eps)) (+120, +240; +360 if < 0)."""
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = diff / (np.abs(v) + FLT_EPSILON)
    k = 60.0 / (diff + FLT_EPSILON)
    h = np.where(v == r, (g - b) * k, np.where(v == g, (b - r) * k + 120.0, (r - g) * k + 240.0))
    h = np.where(h < 0, h + 360.0, h)
    return np.stack([h, s, v], axis=-1).astype(img.dtype)


def hsv_to_bgr(img):
    """float HSV -> BGR by sector, h / 60 wrapped into [0, 6); S == 0 gives grey."""
    h, s, v = img[..., 0], img[..., 1], img[..., 2]
    hh = h / 60.0
    hh = np.where(hh < 0, hh + 6.0, np.where(hh >= 6, hh - 6.0, hh))
    fs = np.floor(hh)
    hh = hh - fs
    bad = ~((fs >= 0) & (fs < 6))
    fs, hh = np.where(bad, 0, fs), np.where(bad, 0, hh).astype(img.dtype)
    sector = fs.astype(np.int64)
    tab = np.stack([v, v * (1.0 - s), v * (1.0 - s * hh), v * (1.0 - s * (1.0 - hh))], axis=-1)
    out = np.take_along_axis(tab, SECTORS[sector], axis=-1)
    out = np.where((s == 0)[..., None], v[..., None], out)
    return out.astype(img.dtype)


def cvt_color(img, code):
    if code == COLOR_BGR2RGB:
        return np.ascontiguousarray(img[:, :, ::-1])
    if code == COLOR_BGR2HSV:
        return bgr_to_hsv(img)
    if code == COLOR_HSV2BGR:
        return hsv_to_bgr(img)
    raise NotImplementedError(code)


def photometric(img, p):
    """PhotometricDistort on a float BGR image in the image's dtype, from the parameter dict (mode 1 / 2: contrast first / last)."""
    T = img.dtype.type
    img = img + T(p["delta"])
    if p["mode"] == 1:
        img = img * T(p["alpha"])
    hsv = bgr_to_hsv(img)
    hsv[..., 1] = hsv[..., 1] * T(p["sat"])
    h = hsv[..., 0] + T(p["hue"])
    h = np.where(h > 360.0, h - 360.0, h)
    hsv[..., 0] = np.where(h < 0.0, h + 360.0, h)
    img = hsv_to_bgr(hsv)
    if p["mode"] == 2:
        img = img * T(p["alpha"])
    return img


# ---------------------------------------------------------------------------------------------------------- geometry
def get_rotation_matrix_2d(centre, angle, scale):
    a = np.deg2rad(angle)
    al, be = np.cos(a) * scale, np.sin(a) * scale
    cx, cy = float(centre[0]), float(centre[1])
    return np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]], dtype=np.float64)


def invert_affine(M):
    M = np.array(M, dtype=np.float64)
    det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    d = 1.0 / det if det != 0 else 0.0
    a11, a22 = M[1, 1] * d, M[0, 0] * d
    a12, a21 = M[0, 1] * -d, M[1, 0] * -d
    return np.array([[a11, a12, -a11 * M[0, 2] - a12 * M[1, 2]], [a21, a22, -a21 * M[0, 2] - a22 * M[1, 2]]], dtype=np.float64)


def source_coords(Minv, H, W):
    """(u, v) = Minv . (x, y, 1) in float64 with separate multiplies and adds, and their floors."""
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    u = Minv[0, 0] * X + Minv[0, 1] * Y + Minv[0, 2]
    v = Minv[1, 0] * X + Minv[1, 1] * Y + Minv[1, 2]
    return u, v, np.floor(u), np.floor(v)


def border_mask(Minv, h, w, H, W):
    """[H, W] bool: no tap with a weight other than 0 lies inside the h x w source (the right / lower tap of an integer coordinate
    has weight 0)."""
    u, v, fu, fv = source_coords(Minv, H, W)
    in_x = ((fu >= 0) & (fu <= w - 1)) | ((fu >= -1) & (fu <= w - 2) & (u != fu))
    in_y = ((fv >= 0) & (fv <= h - 1)) | ((fv >= -1) & (fv <= h - 2) & (v != fv))
    return ~(in_x & in_y)


def sample_bilinear(img, Minv, H, W):
    """[h, w, C] float image -> [H, W, C]: four taps at the exact coordinate, a tap outside the image is 0, blend in img.dtype."""
    dt = img.dtype
    h, w = img.shape[:2]
    u, v, fu, fv = source_coords(Minv, H, W)
    fx, fy = (u - fu).astype(dt), (v - fv).astype(dt)
    gx, gy = 1 - fx, 1 - fy
    x0 = np.clip(np.nan_to_num(fu), -2, w + 1).astype(np.int64)
    y0 = np.clip(np.nan_to_num(fv), -2, h + 1).astype(np.int64)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(inside[..., None], img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0).astype(dt)

    out = (gx * gy)[..., None] * tap(y0, x0)
    out = out + (fx * gy)[..., None] * tap(y0, x0 + 1)
    out = out + (gx * fy)[..., None] * tap(y0 + 1, x0)
    out = out + (fx * fy)[..., None] * tap(y0 + 1, x0 + 1)
    return out.astype(dt)


def warp_affine(img, M, dsize):
    """cv2.warpAffine(img, M, (W, H)) with the default flags: dst(x, y) = src(M^-1 . (x, y, 1)), constant border 0."""
    return sample_bilinear(img, invert_affine(M), int(dsize[1]), int(dsize[0]))


# ---------------------------------------------------------------------------------------------------------- the image path
def normalise(img, mean, stds):
    dt = img.dtype
    out = img / 255.0
    out = out - np.asarray(mean, dtype=np.float32).astype(dt)
    return (out / np.asarray(stds, dtype=np.float32).astype(dt)).astype(dt)


def augment_image(frame, p, size, mean=MEAN, stds=STDS, dtype=np.float32):
    """uint8 BGR [hmax, wmax, 3] (the image is its top-left p['h'] x p['w']) -> [3, H, W] RGB planes in ``dtype``."""
    img = np.asarray(frame)[:p["h"], :p["w"]].astype(dtype)
    if p["mode"] != 0:
        img = photometric(img, p)
    out = sample_bilinear(img, np.asarray(p["Minv"], dtype=np.float64), int(size[0]), int(size[1]))
    out = normalise(out, mean, stds)
    return np.ascontiguousarray(out[:, :, ::-1].transpose(2, 0, 1))


def augment_frames(frames, params, size, mean=MEAN, stds=STDS, dtype=np.float32):
    return np.stack([augment_image(f, p, size, mean, stds, dtype) for f, p in zip(np.asarray(frames), params)])


# ---------------------------------------------------------------------------------------------------------- the golden file
class AttrDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    __setattr__ = dict.__setitem__


CONF_KEYS = ("distort_prob", "mirror_prob", "trans_prob", "shift", "scale_trans")
GT_FIELDS = ("bbox_full", "bbox_vis", "bbox_3d", "center_3d")


def make_imobj(fields, p2, classes=("Car", "Pedestrian", "Cyclist")):
    """imobj from {field: [n_gt, k] float64}: gts carry numpy bbox_full / bbox_vis and list bbox_3d / center_3d as the reference's
    loader builds them."""
    n = len(fields["bbox_full"])
    gts = [AttrDict(cls=classes[i % len(classes)], ign=False, visibility=1.0, bbox_full=np.array(fields["bbox_full"][i], dtype=np.float64),
                    bbox_vis=np.array(fields["bbox_vis"][i], dtype=np.float64), bbox_3d=[float(v) for v in fields["bbox_3d"][i]],
                    center_3d=[float(v) for v in fields["center_3d"][i]]) for i in range(n)]
    p2 = np.array(p2, dtype=np.float64)
    return AttrDict(gts=gts, p2=p2, p2_inv=np.linalg.inv(p2), scale_factor=1.0)


def label_fields(imobj):
    return {k: np.array([np.asarray(gt[k], dtype=np.float64) for gt in imobj["gts"]], dtype=np.float64) for k in GT_FIELDS}


def golden_cases(path=GOLDEN):
    """[(name, conf dict, seed, frames list of uint8 [h, w, 3], imobjs, size, expected images [n, 3, H, W], expected label fields
    per image, expected scale_factor per image)] from tests/golden/augment.npz."""
    G = np.load(path, allow_pickle=False)
    out = []
    for name in [str(s) for s in G["cases"]]:
        conf = AttrDict(zip(CONF_KEYS, [float(v) for v in G[name + "_conf"]]))
        conf.crop_size = [int(v) for v in G[name + "_size"]]
        conf.image_means, conf.image_stds = [float(v) for v in G["mean"]], [float(v) for v in G["stds"]]
        n = int(G[name + "_n"])
        frames = [G["%s_frame%d" % (name, i)] for i in range(n)]
        imobjs = [make_imobj({k: G["%s_in%d_%s" % (name, i, k)] for k in GT_FIELDS}, G["p2"]) for i in range(n)]
        want = [{k: G["%s_out%d_%s" % (name, i, k)] for k in GT_FIELDS} for i in range(n)]
        out.append((name, conf, int(G[name + "_seed"]), frames, imobjs, conf.crop_size, G[name + "_images"], want,
                    [float(v) for v in G[name + "_scale_factor"]]))
    return out


def pack_frames(frames):
    """Frames of mixed sizes into one zero-filled uint8 [B, hmax, wmax, 3] buffer."""
    hmax, wmax = max(f.shape[0] for f in frames), max(f.shape[1] for f in frames)
    buf = np.zeros((len(frames), hmax, wmax, 3), dtype=np.uint8)
    for i, f in enumerate(frames):
        buf[i, :f.shape[0], :f.shape[1]] = f
    return buf
