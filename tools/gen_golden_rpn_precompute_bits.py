#!/usr/bin/env python
"""Record what m3d_rpn_precompute_targets writes, bit for bit, on seeded cases of tests/rpn_loss_smp_ref.py:
tests/golden/rpn_precompute_bits.npz.

The fixture pins the float32-roi path of launches 1-3 of csrc/rpn_loss.hip across the change that made their roi arithmetic
generic over its scalar type (m3d_rpn_target_stats instantiates it in float64): it was written by the library built from the
commit BEFORE that change, on an MI355X, and tests/test_gpu_bbox_stats.py requires the same bits of the library in the tree.
Regenerate it only from a library whose float path is known to be the old one.

Stored per case: sha256 of labels, gt_index, bbox_2d, bbox_3d and any_val; for the small case `odd` the arrays themselves too,
so that a difference can be located.

Run (needs the device):  python tools/gen_golden_rpn_precompute_bits.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

CASES = ("odd", "shipped")
KEYS = ("labels", "gt_index", "bbox_2d", "bbox_3d", "any_val")


def precompute_bits(name, device="cuda:0"):
    """{key: numpy array} of rpn_precompute_targets on case `name` of rpn_loss_smp_ref.GOLDEN_CASES."""
    import rpn_loss_smp_ref as SR
    from m3dssd_amd.host import loss as hl
    from m3dssd_amd.host import ops
    conf, case = SR.golden_case(name)
    imobjs, fs = case[4], case[5]
    vec = hl.pack_conf(conf.bbox_means, conf.bbox_stds, conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo, conf.bg_thresh_hi,
                       conf.best_thresh, conf.box_samples, conf.fg_fraction, conf.focal_loss, conf.cls_2d_lambda, conf.iou_2d_lambda,
                       conf.bbox_2d_lambda, conf.bbox_3d_lambda, conf.feat_stride)
    table = hl.pack_gts(imobjs, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
    d = ops.rpn_precompute_targets(np.asarray(conf.anchors, dtype=np.float64), vec, table, fs, device)
    out = {k: d[k].cpu().numpy() for k in KEYS[:4]}
    out["any_val"] = d["meta"]["any_val"].cpu().numpy()
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "rpn_precompute_bits.npz"))
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    out = {}
    for name in CASES:
        bits = precompute_bits(name)
        for k in KEYS:
            out["%s_%s_sha256" % (name, k)] = np.array(digest(bits[k]))
            if name == "odd":
                out["%s_%s" % (name, k)] = bits[k]
        print(name, {k: digest(bits[k])[:12] for k in KEYS})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
