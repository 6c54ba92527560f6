#!/usr/bin/env python
"""Golden vectors for the training input path: the reference's own ``lib.augmentations.Augmentation(conf)`` followed by the
BGR->RGB swap and the HWC->CHW permute of ``lib/dataloader.py:943-950``, run here on seeded uint8 frames and seeded ground truths
with ``np.random`` seeded per case.

cv2 is not installed in the build container: the three cv2 calls on this path (``getRotationMatrix2D``, ``warpAffine``,
``cvtColor``) get the numpy stand-ins of tests/augment_ref.py; everything else -- the order of the random draws, the comparisons,
the clips, the label arithmetic with its quirks -- is the reference's code.  So the labels and the control flow of the golden are
the reference's; the pixels are pinned by the documented formulas (not checked against a cv2 binary: DESIGN.md section 7).
Writes tests/golden/augment.npz (inputs, seeds, conf values, output images, every rewritten label field; data only)."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.join(os.path.dirname(HERE), "tests"))
import gen_golden  # noqa: E402
import augment_ref as AR  # noqa: E402

SIZE = (16, 38)
SIZES = ((13, 37), (20, 36))
# KITTI-like projection scaled to the toy frames: focal length ~720, principal point inside the frame
P2 = np.array([[720.0, 0.0, 18.2, 4.5], [0.0, 720.0, 6.9, 0.2], [0.0, 0.0, 1.0, 0.003], [0.0, 0.0, 0.0, 1.0]])
SHIFT, SCALE_TRANS = 0.1, 0.4


def _first_is_contrast_first(seed):
    return np.random.RandomState(seed).rand() <= 0.5


# name -> (distort_prob, mirror_prob, trans_prob, full-range pixels, predicate(seed, scale factors of the two images))
CASES = [
    ("plain", -1, 0.0, 0.0, True, lambda s, sc: True),
    ("mirror", -1, 1.0, 0.0, True, lambda s, sc: True),
    ("warp_clip_lo_hi", -1, 0.0, 1.0, True, lambda s, sc: sc[0] == 1 - SCALE_TRANS and sc[1] == 1 + SCALE_TRANS),
    ("warp_mirror", -1, 1.0, 1.0, True, lambda s, sc: abs(sc[0] - 1) < SCALE_TRANS and sc[1] == 1 - SCALE_TRANS),
    ("shipped", -1, 0.5, 0.7, True, lambda s, sc: sc[0] != 1.0 and sc[1] == 1.0),
    ("photo_first", 1.0, 1.0, 1.0, False, lambda s, sc: _first_is_contrast_first(s)),
    ("photo_last", 1.0, 0.0, 1.0, False, lambda s, sc: not _first_is_contrast_first(s)),
    ("photo_half", 0.5, 0.5, 0.7, False, lambda s, sc: sc[0] != 1.0),
]


def make_inputs(rng, h, w, full_range):
    lo, hi = (0, 256) if full_range else (40, 216)
    im = rng.randint(lo, hi, size=(h, w, 3)).astype(np.uint8)
    if full_range:
        im[0, 0], im[-1, -1] = (0, 128, 255), (255, 0, 0)
    fields = {k: [] for k in AR.GT_FIELDS}
    for i, rot_y in enumerate((1.2, -0.8, -2.9)):                      # both rotY signs, one next to -pi
        bw, bh = rng.uniform(4, 12), rng.uniform(3, 8)
        x, y = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
        z = rng.uniform(8, 50)
        cx, cy = x + bw / 2 + rng.normal(0, 0.3), y + bh / 2 + rng.normal(0, 0.3)
        c3 = np.linalg.inv(P2).dot(np.array([cx * z, cy * z, z, 1.0]))
        alpha = rot_y - np.arctan2(-c3[2], c3[0]) - 0.5 * np.pi
        fields["bbox_full"].append([x, y, bw, bh])
        fields["bbox_vis"].append([x + 0.5, y + 0.25, bw - 1.0, bh - 0.5])
        fields["bbox_3d"].append([cx, cy, z, rng.normal(1.6, 0.1), rng.normal(1.5, 0.1), rng.normal(3.9, 0.3), alpha, c3[0], c3[1], c3[2], rot_y])
        fields["center_3d"].append([c3[0], c3[1], c3[2]])
    return im, {k: np.array(v, dtype=np.float64) for k, v in fields.items()}


def main():
    gen_golden._install_stubs()
    cv2 = sys.modules["cv2"]
    cv2.COLOR_BGR2RGB, cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR = AR.COLOR_BGR2RGB, AR.COLOR_BGR2HSV, AR.COLOR_HSV2BGR
    cv2.getRotationMatrix2D = AR.get_rotation_matrix_2d
    cv2.warpAffine = AR.warp_affine
    cv2.cvtColor = AR.cvt_color
    import torch
    from easydict import EasyDict
    from lib.augmentations import Augmentation

    def run(conf, seed, frames, imobjs):
        np.random.seed(seed)
        aug = Augmentation(conf)
        images, objs = [], []
        for im, imobj in zip(frames, imobjs):
            x, o = aug(im.copy(), copy.deepcopy(imobj))                    # dataloader.py:939
            x = cv2.cvtColor(x, cv2.COLOR_BGR2RGB)                         # dataloader.py:943
            x = torch.from_numpy(x).permute(2, 0, 1).contiguous().numpy()  # dataloader.py:950
            assert x.dtype == np.float32 and x.shape == (3,) + SIZE
            images.append(x)
            objs.append(o)
        return np.stack(images), objs

    out = {"cases": np.array([c[0] for c in CASES]), "p2": P2, "mean": np.asarray(AR.MEAN, np.float64), "stds": np.asarray(AR.STDS, np.float64)}
    rng = np.random.RandomState(11)
    for name, distort, mirror, trans, full_range, pred in CASES:
        conf = EasyDict(image_means=AR.MEAN, image_stds=AR.STDS, crop_size=list(SIZE), mirror_prob=mirror, distort_prob=distort,
                        trans_prob=trans, shift=SHIFT, scale_trans=SCALE_TRANS)
        frames, imobjs, fields = [], [], []
        for h, w in SIZES:
            im, f = make_inputs(rng, h, w, full_range)
            frames.append(im)
            fields.append(f)
            imobjs.append(EasyDict(AR.make_imobj(f, P2)))
            imobjs[-1].gts = [EasyDict(g) for g in imobjs[-1].gts]
        for seed in range(10000):
            images, objs = run(conf, seed, frames, imobjs)
            if pred(seed, [float(o.scale_factor) for o in objs]):
                break
        else:
            raise RuntimeError("no seed found for case " + name)
        out[name + "_conf"] = np.array([distort, mirror, trans, SHIFT, SCALE_TRANS], dtype=np.float64)
        out[name + "_seed"], out[name + "_n"], out[name + "_size"] = np.array(seed), np.array(len(frames)), np.array(SIZE)
        out[name + "_images"] = images
        out[name + "_scale_factor"] = np.array([float(o.scale_factor) for o in objs])
        for i, (im, f, o) in enumerate(zip(frames, fields, objs)):
            out["%s_frame%d" % (name, i)] = im
            for k in AR.GT_FIELDS:
                out["%s_in%d_%s" % (name, i, k)] = f[k]
                out["%s_out%d_%s" % (name, i, k)] = AR.label_fields(o)[k]
        print(name, "seed", seed, "scale factors", out[name + "_scale_factor"].tolist())
    path = os.path.join(gen_golden.OUT, "augment.npz")
    np.savez_compressed(path, **out)
    print(path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
