#!/usr/bin/env python
"""Generate tests/golden/rpn_loss_smp_*.npz by running the REFERENCE's own data-loader target assignment
(Kitti_Dataset_torch._targets, lib/dataloader.py:1014-1144) and its RPN_3D_loss_smp (lib/loss/rpn_3d.py:659-1360) on the CPU.

Build-container only, like tools/gen_golden_rpn_loss.py, whose import stubs (tools/gen_golden.py) it reuses.  ``_targets`` is
called per image with a types.SimpleNamespace as ``self`` (the fields it reads), the results are collated the way the default
collate function stacks them, and the loss gets non-leaf inputs (``cls * 1`` ...) because bbox_transform_inv_new de-normalises
``bbox_2d`` in place.

Cases (tests/rpn_loss_smp_ref.py: GOLDEN_CASES): the seeded 128x320, B = 2 cases `shipped`, `allboxes`, `emptyimg`, and `odd`:
a 40x72 crop (feat 5x9, R = 1 620: no multiple of 256 or of 1 024), B = 3, the middle image without a valid ground truth.

Stored per file (data only): the case's name, per-anchor labels (int16), any_val, the sampled fg / bg masks (bit-packed, read
off the gradients as in gen_golden_rpn_loss.py), the normalised targets of the fg rows, loss, every stat with its name, float64
checksums + strided samples of the three gradients.

The generator FAILS unless the reference's result is unique: no overlap within 1e-9 of a threshold, and the scores at ranks
k-1 and k of every selection differ (the reference's torch.sort is as unstable as its argsort).

Run:  python tools/gen_golden_rpn_loss_smp.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402


def main():
    gen_golden._install_stubs()
    import torch
    torch.set_num_threads(8)
    sys.path.append(os.path.join(gen_golden.REPO, "tests"))
    import rpn_loss_ref as RR
    import rpn_loss_smp_ref as SR
    import lib.rpn_util as ref_rpn
    import lib.core as ref_core
    import lib.dataloader as ref_data
    import lib.loss.rpn_3d as ref_loss
    assert ref_loss.__file__.startswith(gen_golden.REF) and ref_data.__file__.startswith(gen_golden.REF)

    for name in SR.GOLDEN_CASES:
        conf, (cls, prob, b2, b3, imobjs, fs) = SR.golden_case(name)
        conf.device = "cpu"
        B, R, C = cls.shape
        seen = []
        orig = ref_rpn.compute_targets

        def recording(*a, **k):
            out = orig(*a, **k)
            seen.append(out[1])
            return out
        ref_data.compute_targets = recording
        loader = types.SimpleNamespace(num_anchors=conf.anchors.shape[0], feat_size=fs, anchors=conf.anchors, feat_stride=conf.feat_stride,
                                       lbls=conf.lbls, ilbls=conf.ilbls, min_gt_vis=conf.min_gt_vis, min_gt_h=conf.min_gt_h,
                                       fg_thresh=conf.fg_thresh, ign_thresh=conf.ign_thresh, bg_thresh_lo=conf.bg_thresh_lo,
                                       bg_thresh_hi=conf.bg_thresh_hi, best_thresh=conf.best_thresh, bbox_means=conf.bbox_means,
                                       bbox_stds=conf.bbox_stds)
        per = [ref_data.Kitti_Dataset_torch._targets(loader, im) for im in imobjs]
        ref_data.compute_targets = orig
        st = lambda i: torch.from_numpy(np.stack([np.asarray(p[i]) for p in per]))      # noqa: E731
        any_val = torch.tensor([int(p[7]) for p in per])
        target = {"labels_fg": st(0), "labels_bg": st(1), "labels_ign": st(2), "labels": st(3).long(), "bbox_2d": st(4), "bbox_3d": st(5),
                  "meta": {"rois": st(6), "any_val": any_val, "p2": torch.stack([torch.eye(4)] * B)}}
        labels = target["labels"].numpy().copy()
        b2_tar, b3_tar = target["bbox_2d"].numpy().copy(), target["bbox_3d"].numpy().copy()      # (the loss de-normalises bbox_2d in place)

        # uniqueness: overlaps against the thresholds, scores at the cuts
        gap, it = np.inf, iter(seen)
        rois = ref_rpn.locate_anchors(conf.anchors, fs, conf.feat_stride).astype(np.float32)
        for b, imobj in enumerate(imobjs):
            if not int(any_val[b]):
                continue
            ols = next(it)
            for th in (conf.fg_thresh, conf.bg_thresh_hi, conf.best_thresh):
                gap = min(gap, float(np.abs(ols - th).min()))
            igns, rmvs = ref_rpn.determine_ignores(imobj.gts, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
            keep_i = (rmvs == False) & (igns == True)     # noqa: E712
            if keep_i.any():
                allb = ref_rpn.bbXYWH2Coords(np.array([gt.bbox_full for gt in imobj.gts]))
                gap = min(gap, float(np.abs(ref_core.iou_ign(rois, allb[keep_i]) - conf.ign_thresh).min()))
            assert ((labels[b] > 0) & (labels[b] != RR.IGN_FLAG)).any() or (labels[b] == RR.IGN_FLAG).any(), \
                "%s: image %d takes the reference's no-fg-no-ignore branch" % (name, b)
            for lo, hi in RR.cut_margins(labels[b], prob.numpy()[b], conf, R):
                assert lo != hi, "%s: the scores at the cut are equal (%r): the reference's choice is not unique" % (name, lo)
        assert gap > 1e-9, "%s: an overlap lies %.3e from a threshold" % (name, gap)

        crit = ref_loss.RPN_3D_loss_smp(conf)
        ins = [t.clone().requires_grad_(True) for t in (cls, b2, b3)]
        loss, stats = crit(ins[0] * 1, prob.clone(), ins[1] * 1, ins[2] * 1, target, fs)
        loss.backward()
        g = [t.grad.double().numpy() for t in ins]
        sampled = np.abs(g[0]).sum(axis=2) != 0
        fg_s = np.abs(g[2]).sum(axis=2) != 0
        assert not (fg_s & ~sampled).any() and not (fg_s & (labels <= 0)).any() and not (sampled & (labels == RR.IGN_FLAG)).any()
        fg_rows = np.argwhere((labels > 0) & (labels != RR.IGN_FLAG))
        fg_targets = np.concatenate([b2_tar, b3_tar], axis=2)[fg_rows[:, 0], fg_rows[:, 1]]
        out = dict(case=np.array(name), labels=labels.astype(np.int16), any_val=any_val.numpy().astype(np.int32),
                   sampled_fg=np.packbits(fg_s), sampled_bg=np.packbits(sampled & ~fg_s), fg_rows=fg_rows.astype(np.int32),
                   fg_targets=fg_targets.astype(np.float32), loss=np.array(float(loss.detach())), threshold_gap=np.array(gap),
                   stat_names=np.array([RR.stat_key(s) for s in stats]), stat_vals=np.array([float(s['val']) for s in stats]))
        for k, arr in zip(("g_cls", "g_bbox_2d", "g_bbox_3d"), g):
            out[k + "_sum"], out[k + "_sample"] = RR.grad_summary(arr)
        path = os.path.join(gen_golden.OUT, "rpn_loss_smp_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("%s: loss %r, fg %d bg %d sampled, nearest threshold %.2e, %d bytes; stats %s"
              % (name, float(loss.detach()), int(fg_s.sum()), int((sampled & ~fg_s).sum()), gap, os.path.getsize(path),
                 ", ".join("%s=%.4f" % (RR.stat_key(s), float(s['val'])) for s in stats)))


if __name__ == "__main__":
    main()
