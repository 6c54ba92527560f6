#!/usr/bin/env python
"""Times ``compute_bbox_stats`` (m3dssd_amd/host/dataset_stats.py, m3d_rpn_target_stats in csrc/rpn_loss.hip) on a synthetic imdb of
the KITTI training split's size: 3 712 images of the four KITTI frame sizes (about 375x1242), the shipped anchors (12 scales x
3 ratios, priors from ``generate_anchors`` on the same imdb), thresholds and test scale (384: feature maps 48-49 x 159,
R = 275 k - 280 k rows), six ground truths per image whose shapes cycle over the anchors'.

Figures (one JSON line, appended to --out):
  wall_s            compute_bbox_stats end to end, cold cache folder: grouping, gt packing, uploads, both passes, downloads
  pack_s            the host part alone: group_by_feat_size + pack_gts_scaled of every chunk (done once, used by both passes)
  kernel_ms         HIP events around the m3d_rpn_target_stats calls of ONE pass over the whole imdb (tables resident, one
                    workspace, nothing else between the events): median / min / iqr of --reps runs after --warmup
  anchors_s         generate_anchors (host numpy)
  numpy_subset_s    the numpy restatement of the reference (tests/bbox_stats_ref.py: compute_targets twice per image) on the
                    first --subset images, same process; numpy_full_s_extrapolated scales it to the imdb
  subset_max_err    device vs restatement on that subset: max |mean difference| / std and max relative std difference

usage: python tools/bbox_stats_bench.py [--images 3712] [--subset 64] [--reps 5] [--warmup 1] [--out profiles/bbox_stats_bench.jsonl]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from m3dssd_amd import _hip  # noqa: E402
from m3dssd_amd.config import Conf, Config  # noqa: E402
from m3dssd_amd.host import dataset_stats as ds  # noqa: E402
from m3dssd_amd.host import ops  # noqa: E402
import bbox_stats_ref as BR  # noqa: E402

KITTI_SIZES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]
N_GT = 6


def make_conf():
    conf = Config()
    conf.update(min_gt_vis=0.65, fg_thresh=0.5, ign_thresh=0.5, bg_thresh_lo=0, bg_thresh_hi=0.5, best_thresh=0.35, has_3d=True)
    return conf


def make_imdb(conf, n, seed=0):
    rng = np.random.RandomState(seed)
    n_anchor = len(conf.anchor_scales) * len(conf.anchor_ratios)
    imdb = []
    for i in range(n):
        h, w = KITTI_SIZES[[0, 0, 0, 1, 2, 3][i % 6]]
        gts = []
        for g in range(N_GT):
            a = (i * N_GT + g) % n_anchor
            sh = min(conf.anchor_scales[a // 3] * rng.uniform(0.9, 1.1) * h / conf.test_scale[0], h - 2.0)
            sw = sh * conf.anchor_ratios[a % 3] * rng.uniform(0.9, 1.1)
            x, y = rng.uniform(0, w - sw), rng.uniform(0, h - sh)
            cls = ["Car", "Pedestrian", "Cyclist", "Van", "Tram"][g % 3 if g < 4 else rng.randint(0, 5)]
            gts.append(Conf(bbox_full=np.array([x, y, sw, sh]), cls=cls, ign=False, visibility=0.3 if rng.rand() < 0.1 else 1.0,
                            bbox_3d=np.array([x + sw / 2 + rng.normal(0, 2), y + sh / 2 + rng.normal(0, 2), rng.uniform(5, 60),
                                              rng.normal(1.6, 0.1), rng.normal(1.5, 0.1), rng.normal(3.9, 0.3), rng.uniform(-3.1, 3.1)])))
        imdb.append(Conf(imH=h, imW=w, scale=1, gts=gts))
    return imdb


def stats(ts):
    ts = sorted(ts)
    n = len(ts)
    return {"median": round(ts[n // 2], 3), "min": round(ts[0], 3), "iqr": round(ts[(3 * n) // 4] - ts[n // 4], 3)}


def kernel_pass_ms(conf, plan, tables, dev, reps, warmup):
    """One pass of m3d_rpn_target_stats over every chunk, through the C ABI on resident buffers, between two events."""
    L = _hip.lib()
    anc = torch.from_numpy(np.ascontiguousarray(conf.anchors)).to(dev)
    A = int(anc.shape[0])
    vec = ds.stats_conf_vec(conf)
    cen = torch.zeros(11, device=dev, dtype=torch.float64)
    gts = [torch.from_numpy(t).to(dev) for t in tables]
    outs = [torch.empty(t.shape[0], 23, device=dev, dtype=torch.float64) for t in tables]
    need = max(L.m3d_rpn_target_stats_workspace_bytes(t.shape[0], A * fs[0] * fs[1]) for (fs, _), t in zip(plan, tables))
    ws = torch.empty(need + 256, device=dev, dtype=torch.uint8)
    base = (ws.data_ptr() + 255) // 256 * 256
    stream = ops._stream()

    def run():
        for (fs, _), t, g, o in zip(plan, tables, gts, outs):
            _hip.check(L.m3d_rpn_target_stats(anc.data_ptr(), A, fs[0], fs[1], vec.ctypes.data, int(vec.size), g.data_ptr(), t.shape[0],
                                              t.shape[1] - 1, cen.data_ptr(), o.data_ptr(), base, need, stream))
    ts = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            ts.append(e0.elapsed_time(e1))
    return stats(ts), int(sum(float(o[:, 0].sum()) for o in outs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3712)
    ap.add_argument("--subset", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bbox_stats_bench.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the device"
    dev = torch.device("cuda:0")
    conf = make_conf()
    imdb = make_imdb(conf, a.images)
    t0 = time.perf_counter()
    ds.generate_anchors(conf, imdb, None)
    anchors_s = time.perf_counter() - t0

    ds.compute_bbox_stats(conf.copy(), imdb[:8], None)            # untimed: library load, first launches
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as folder:
        t0 = time.perf_counter()
        ds.compute_bbox_stats(conf, imdb, folder)
        torch.cuda.synchronize()
        wall_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    plan = ds.group_by_feat_size(conf, imdb)
    tables = [ds.pack_gts_scaled(conf, [imdb[i] for i in idx]) for _fs, idx in plan]
    pack_s = time.perf_counter() - t0
    kernel_ms, n_fg = kernel_pass_ms(conf, plan, tables, dev, a.reps, a.warmup)

    sub = imdb[:a.subset]
    rconf = conf.copy()
    t0 = time.perf_counter()
    r_means, r_stds = BR.compute_bbox_stats(rconf, sub)
    numpy_s = time.perf_counter() - t0
    dconf = conf.copy()
    ds.compute_bbox_stats(dconf, sub, None)
    err = {"mean_over_std": float((np.abs(dconf.bbox_means - r_means) / r_stds).max()),
           "std_rel": float((np.abs(dconf.bbox_stds - r_stds) / r_stds).max())}

    res = {"op": "compute_bbox_stats", "images": a.images, "gts_per_image": N_GT, "anchors": int(conf.anchors.shape[0]),
           "feat_sizes": sorted({fs for fs, _ in plan}), "chunks": len(plan), "fg_rows": n_fg, "anchors_s": round(anchors_s, 3),
           "wall_s": round(wall_s, 3), "pack_s": round(pack_s, 3), "kernel_ms_per_pass": kernel_ms, "reps": a.reps,
           "numpy_subset": a.subset, "numpy_subset_s": round(numpy_s, 3),
           "numpy_full_s_extrapolated": round(numpy_s * a.images / a.subset, 1), "subset_max_err": err,
           "means": [round(float(v), 6) for v in conf.bbox_means[0]], "stds": [round(float(v), 6) for v in conf.bbox_stds[0]],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
