#!/usr/bin/env python
"""Times RPN_3D_loss on the device (csrc/rpn_loss.hip) at 384x1280, B = 4 and 8 (R = 276 480 anchors per image), shipped settings.

HIP events, `--warmup` untimed calls, then the median and minimum of `--reps` timed ones, for
  module    RPN_3D_loss.forward as a training script calls it: host gt packing, the one upload, six launches (loss AND the
            stored gradients), the one small download
  targets   m3d_rpn_targets alone (launches 1-3: gt max, gt row, assign)
  loss      m3d_rpn_loss alone (launches 4-6: select, loss + gradients, finish)
"Before": the float32 restatement of the reference class (tests/rpn_loss_ref.py, bit-identical to the reference's own numbers on
the golden cases) on this host's CPU at 16 threads, forward only and forward + backward, one run each.

Bytes each launch has to move (from the shapes, per anchor row; C classes, sampled fraction s from the run) are printed next to
the 6.3 TB/s the chip reaches on a float4 copy.  Launches 1, 2 and 4 re-read data that stays in the caches (the gt table; labels
and scores of one image, 1.7 MB), so their byte counts are cache traffic, not HBM traffic; they are bound by float64 arithmetic
and latency.  Per-launch TIMES come from a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/rpn_loss_bench.py --reps 20 --no-cpu
    python tools/rpn_loss_bench.py --merge BENCH.json --stats-csv DIR/.../t_kernel_stats.csv      (no GPU needed)

usage: python tools/rpn_loss_bench.py [--reps 50] [--warmup 5] [--batches 4 8] [--no-cpu]      (one JSON line per batch size)"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ROOF = 6.3e12
KERNELS = ("rpn_gt_max_kernel", "rpn_gt_row_kernel", "rpn_assign_kernel", "rpn_select_kernel", "rpn_loss_kernel", "rpn_finish_kernel")


def launch_bytes(B, R, C, n_gt, sampled_fg, sampled_bg):
    """Bytes per launch from the shapes: what the algorithm reads and writes, not what the caches absorb."""
    rows = B * R
    gt = B * (n_gt + 1) * 12 * 8
    return {
        "rpn_gt_max_kernel": gt,
        "rpn_gt_row_kernel": gt,
        "rpn_assign_kernel": rows * (4 * C + 4 + 2 + 2 + 44 + 4) + gt,
        "rpn_select_kernel": 2 * 4 * rows * 6,                                   # 2 selections x 4 digit passes over labels + scores
        "rpn_loss_kernel": rows * (2 + 4 + 1 + 4 * C + 16 + 28) + (sampled_fg + sampled_bg) * 4 * C + sampled_fg * (16 + 28 + 44),
        "rpn_finish_kernel": min((rows + 255) // 256, 2048) * 16 * 8,
    }


def timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4)}


def merge(bench_json, stats_csv):
    times = {}
    for row in csv.DictReader(open(stats_csv)):
        for k in KERNELS:
            if k in row["Name"]:
                times[k] = float(row["AverageUs"]) if "AverageUs" in row else float(row["AverageNs"]) / 1e3
    for line in open(bench_json):
        if not line.startswith("{"):
            continue
        res = json.loads(line)
        # the trace averages over both batch sizes; per-launch rates are only printed for a trace of ONE batch size
        res["launch_avg_us"] = {k: round(v, 1) for k, v in times.items()}
        res["launch_gbps"] = {k: round(res["launch_bytes"][k] / (times[k] * 1e-6) / 1e9, 1) for k in times}
        res["launch_share_of_hbm_roof"] = {k: round(res["launch_bytes"][k] / (times[k] * 1e-6) / HBM_ROOF, 3) for k in times}
        print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--gts", type=int, default=3, help="ground truths per image (3: the size the CPU figure of the issue used)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--merge")
    ap.add_argument("--stats-csv")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.stats_csv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rpn_loss_bench: no ROCm device")
    from m3dssd_amd.host import loss as hl
    import rpn_loss_ref as RR
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda:0")
    for B in a.batches:
        conf = RR.loss_conf((384, 1280), 0)
        cls, prob, b2, b3, imobjs, fs = RR.make_case(40 + B, (384, 1280), B, a.gts)
        crit = hl.RPN_3D_loss(conf)
        ins = [t.to(dev) for t in (cls, prob, b2, b3)]
        res = {"tool": "rpn_loss_bench", "B": B, "R": cls.shape[1], "gts_per_image": a.gts, "reps": a.reps,
               "threads_cpu": torch.get_num_threads()}
        res["module_ms"] = timed(lambda: crit(*ins, imobjs, fs), a.warmup, a.reps)
        vec = hl.pack_conf(conf.bbox_means, conf.bbox_stds, conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo, conf.bg_thresh_hi,
                           conf.best_thresh, conf.box_samples, conf.fg_fraction, conf.focal_loss, conf.cls_2d_lambda,
                           conf.iou_2d_lambda, conf.bbox_2d_lambda, conf.bbox_3d_lambda, conf.feat_stride)
        table = hl.pack_gts(imobjs, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
        anchors = torch.from_numpy(np.asarray(conf.anchors, dtype=np.float64)).to(dev)
        ctx = hl._Ctx(anchors, vec, table, fs, B, cls.shape[1], dev)
        res["targets_ms"] = timed(lambda: hl._targets(ctx, ins[0], ins[1]), a.warmup, a.reps)
        labels, gidx, targets, scores = hl._targets(ctx, ins[0], ins[1])
        res["loss_ms"] = timed(lambda: hl._loss(ctx, ins[0], ins[2], ins[3], labels, targets, scores), a.warmup, a.reps)
        st = dict(zip(hl.STAT_NAMES, crit.last["stats"].cpu().numpy().tolist()))
        res["sampled"] = {"fg": int(st["fg_num"]), "bg": int(st["bg_num"])}
        res["launch_bytes"] = launch_bytes(B, cls.shape[1], cls.shape[2], table.shape[1] - 1, int(st["fg_num"]), int(st["bg_num"]))
        total = sum(res["launch_bytes"][k] for k in ("rpn_assign_kernel", "rpn_loss_kernel", "rpn_finish_kernel"))
        res["hbm_bytes_streamed"] = total
        res["hbm_roof_ms"] = round(total / HBM_ROOF * 1e3, 4)
        if not a.no_cpu:
            t0 = time.perf_counter()
            RR.rpn_3d_loss(conf, cls, prob, b2, b3, imobjs, fs, dtype=torch.float32, grads=False)
            t1 = time.perf_counter()
            RR.rpn_3d_loss(conf, cls, prob, b2, b3, imobjs, fs, dtype=torch.float32, grads=True)
            t2 = time.perf_counter()
            res["cpu_restatement_f32_ms"] = {"forward": round((t1 - t0) * 1e3, 1), "forward_backward": round((t2 - t1) * 1e3, 1)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
