#!/usr/bin/env python
"""Generate tests/golden/rpn_loss_*.npz by running the REFERENCE's own RPN_3D_loss (lib/loss/rpn_3d.py) on the CPU.

Build-container only, like tools/gen_golden.py, whose import stubs it reuses (``conf.device = 'cpu'``).  The inputs are the
seeded cases of tests/rpn_loss_ref.py at 128x320, B = 2 (R = 23 040), ~6 ground truths per image mixing Car / Pedestrian /
Cyclist / Van (ignore class) / an unlisted class / a low-visibility one; one case has an image without a valid ground truth.
Settings: the shipped ones, box_samples = inf, focal_loss = 2, bbox_2d_lambda = 1.

Stored per file (data only): the case's seed, the gt table the reference's own determine_ignores / bbXYWH2Coords / clsName2Ind
give (in the packed layout of m3d_rpn_targets), per-anchor labels (int16), the sampled fg / bg masks (bit-packed), the
normalised targets of the fg rows, loss, every stat, and float64 checksums + strided samples of the three gradients.

The labels and targets are what the reference's compute_targets returned (recorded by a wrapper around it).  The sampled masks
are read off the reference's gradients: a row is sampled iff its cls gradient is non-zero, fg iff its bbox_3d gradient is.

The generator FAILS unless the reference's result is unique: no overlap within 1e-9 of a threshold, and the scores at ranks
k-1 and k of every selection differ (the reference's argsort is unstable).  With that, no anchor is excused from exact
comparison.

Run:  python tools/gen_golden_rpn_loss.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

CASES = {"shipped": (11, "shipped", None), "allboxes": (11, "allboxes", None), "focal2": (11, "focal2", None),
         "bbox2d": (11, "bbox2d", None), "emptyimg": (12, "shipped", 1)}


def main():
    gen_golden._install_stubs()
    import torch
    torch.set_num_threads(8)
    sys.path.append(os.path.join(gen_golden.REPO, "tests"))
    import rpn_loss_ref as RR
    import lib.rpn_util as ref_rpn
    import lib.core as ref_core
    import lib.loss.rpn_3d as ref_loss
    assert ref_loss.__file__.startswith(gen_golden.REF), ref_loss.__file__

    for name, (seed, variant, empty) in CASES.items():
        conf = RR.loss_conf((128, 320), 0, device="cpu", **RR.VARIANTS[variant])
        cls, prob, b2, b3, imobjs, fs = RR.make_case(seed, (128, 320), 2, 6, empty_image=empty)
        B, R, C = cls.shape
        seen = []
        orig = ref_rpn.compute_targets

        def recording(*a, **k):
            out = orig(*a, **k)
            seen.append(out)
            return out
        ref_loss.compute_targets = recording
        crit = ref_loss.RPN_3D_loss(conf)
        ins = [t.clone().requires_grad_(True) for t in (cls, b2, b3)]
        loss, stats = crit(ins[0], prob.clone(), ins[1], ins[2], imobjs, fs)
        loss.backward()
        ref_loss.compute_targets = orig
        g = [t.grad.double().numpy() for t in ins]

        # gt tables from the reference's own helpers
        rows, gap, it = [], np.inf, iter(seen)
        labels = np.zeros((B, R), dtype=np.int16)
        fg_rows, fg_targets = [], []
        rois = ref_rpn.locate_anchors(conf.anchors, fs, conf.feat_stride, convert_tensor=True).float().numpy()
        for b, imobj in enumerate(imobjs):
            gts = imobj.gts
            igns, rmvs = ref_rpn.determine_ignores(gts, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
            allb = ref_rpn.bbXYWH2Coords(np.array([gt.bbox_full for gt in gts]))
            g3 = np.array([gt.bbox_3d for gt in gts])
            keep_v, keep_i = (rmvs == False) & (igns == False), (rmvs == False) & (igns == True)     # noqa: E712
            lab = [ref_rpn.clsName2Ind(conf.lbls, gt.cls) for gt, k in zip(gts, keep_v) if k]
            val = np.concatenate([allb[keep_v], np.asarray(lab, dtype=np.float64).reshape(-1, 1), g3[keep_v][:, :7]], axis=1)
            rows.append((val, allb[keep_i]))
            if not keep_v.any():
                continue
            transforms, ols, _raw = next(it)
            lb = transforms[:, 4]
            labels[b] = np.where(lb > 0, lb, np.where(lb < 0, 0, RR.IGN_FLAG)).astype(np.int16)
            fi = np.flatnonzero(lb > 0)
            fg_rows.append(np.stack([np.full(len(fi), b), fi], axis=1))
            fg_targets.append(transforms[fi][:, [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11]])
            for th in (conf.fg_thresh, conf.bg_thresh_hi, conf.best_thresh):
                gap = min(gap, float(np.abs(ols - th).min()))
            if keep_i.any():
                gap = min(gap, float(np.abs(ref_core.iou_ign(rois, allb[keep_i]) - conf.ign_thresh).min()))
            for lo, hi in RR.cut_margins(labels[b].astype(np.int64), prob.numpy()[b], conf, R):
                assert lo != hi, "%s: the scores at the cut are equal (%r): the reference's choice is not unique" % (name, lo)
        assert gap > 1e-9, "%s: an overlap lies %.3e from a threshold" % (name, gap)
        gmax = max(len(v) + len(i) for v, i in rows)
        table = np.zeros((B, gmax + 1, 12))
        for b, (v, i) in enumerate(rows):
            table[b, 0, :2] = len(v), len(i)
            table[b, 1:1 + len(v)] = v
            table[b, 1 + len(v):1 + len(v) + len(i), :4] = i
        sampled = np.abs(g[0]).sum(axis=2) != 0
        fg_s = np.abs(g[2]).sum(axis=2) != 0
        assert not (fg_s & ~sampled).any() and not (fg_s & (labels <= 0)).any() and not (sampled & (labels == RR.IGN_FLAG)).any()
        out = dict(seed=np.array(seed), variant=np.array(variant), empty_image=np.array(-1 if empty is None else empty),
                   gt_table=table, labels=labels, sampled_fg=np.packbits(fg_s), sampled_bg=np.packbits(sampled & ~fg_s),
                   fg_rows=np.concatenate(fg_rows).astype(np.int32), fg_targets=np.concatenate(fg_targets).astype(np.float32),
                   loss=np.array(float(loss)), threshold_gap=np.array(gap),
                   stat_names=np.array([RR.stat_key(s) for s in stats]), stat_vals=np.array([float(s['val']) for s in stats]))
        for k, arr in zip(("g_cls", "g_bbox_2d", "g_bbox_3d"), g):
            out[k + "_sum"], out[k + "_sample"] = RR.grad_summary(arr)
        path = os.path.join(gen_golden.OUT, "rpn_loss_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("%s: loss %.6f, fg %d bg %d sampled, nearest threshold %.2e, %d bytes; stats %s"
              % (name, float(loss), int(fg_s.sum()), int((sampled & ~fg_s).sum()), gap, os.path.getsize(path),
                 ", ".join("%s=%.4f" % (RR.stat_key(s), float(s['val'])) for s in stats)))


if __name__ == "__main__":
    main()
