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

`--smp` times RPN_3D_loss_smp (m3d_rpn_loss_smp: ingest launch + launches 4-6) instead, against RPN_3D_loss on the same inputs
in the same process, median of `--reps` with the interquartile range:
  full_module      RPN_3D_loss.forward (as above)
  smp_resident     RPN_3D_loss_smp.forward on the device dict of rpn_precompute_targets (int16 labels): no upload
  smp_resident_i64 the same targets with int64 labels resident on the device (the loader's dtype)
  smp_host         RPN_3D_loss_smp.forward on the loader's host dict (int64 labels, pageable tensors): staged through pinned
                   memory and uploaded in every call
  smp_host_pinned  the same dict with the three tensors pinned once
  precompute       rpn_precompute_targets alone (gt packing excluded)

usage: python tools/rpn_loss_bench.py [--reps 50] [--warmup 5] [--batches 4 8] [--no-cpu] [--smp]   (one JSON line per batch size)"""
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
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "q1": round(ts[len(ts) // 4], 4),
            "q3": round(ts[(3 * len(ts)) // 4], 4)}


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


def smp(a):
    import numpy as np
    import torch
    from m3dssd_amd.host import loss as hl
    from m3dssd_amd.host import ops
    import rpn_loss_ref as RR
    dev = torch.device("cuda:0")
    for B in a.batches:
        conf = RR.loss_conf((384, 1280), 0, device="cuda:0")
        cls, prob, b2, b3, imobjs, fs = RR.make_case(40 + B, (384, 1280), B, a.gts)
        ins = [t.to(dev) for t in (cls, prob, b2, b3)]
        full, crit = hl.RPN_3D_loss(conf), hl.RPN_3D_loss_smp(conf)
        vec = full._conf_vec()
        table = hl.pack_gts(imobjs, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
        anchors = np.asarray(conf.anchors, dtype=np.float64)
        pre = ops.rpn_precompute_targets(anchors, vec, table, fs, dev)
        pre_i64 = dict(pre, labels=pre["labels"].long())
        host = dict(labels=pre_i64["labels"].cpu(), bbox_2d=pre["bbox_2d"].cpu(), bbox_3d=pre["bbox_3d"].cpu(),
                    meta=dict(any_val=pre["meta"]["any_val"].cpu().long()))
        pinned = dict(host, labels=host["labels"].pin_memory(), bbox_2d=host["bbox_2d"].pin_memory(), bbox_3d=host["bbox_3d"].pin_memory())
        res = {"tool": "rpn_loss_bench --smp", "B": B, "R": cls.shape[1], "gts_per_image": a.gts, "reps": a.reps, "warmup": a.warmup,
               "host_dict_mbytes": round(sum(host[k].numel() * host[k].element_size() for k in ("labels", "bbox_2d", "bbox_3d")) / 1e6, 1)}
        l_full, _ = full(*ins, imobjs, fs)
        for name, tgt in (("smp_resident", pre), ("smp_resident_i64", pre_i64), ("smp_host", host), ("smp_host_pinned", pinned)):
            l_smp, _ = crit(*ins, tgt, fs)
            assert l_smp.cpu().numpy().tobytes() == l_full.cpu().numpy().tobytes(), name          # the same loss, bit for bit
        res["full_module_ms"] = timed(lambda: full(*ins, imobjs, fs), a.warmup, a.reps)
        for name, tgt in (("smp_resident", pre), ("smp_resident_i64", pre_i64), ("smp_host", host), ("smp_host_pinned", pinned)):
            res[name + "_ms"] = timed(lambda: crit(*ins, tgt, fs), a.warmup, a.reps)
        res["precompute_ms"] = timed(lambda: ops.rpn_precompute_targets(anchors, vec, table, fs, dev), a.warmup, a.reps)
        res["full_module_again_ms"] = timed(lambda: full(*ins, imobjs, fs), a.warmup, a.reps)          # drift check: same as the first
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--gts", type=int, default=3, help="ground truths per image (3: the size the CPU figure of the issue used)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--smp", action="store_true", help="time RPN_3D_loss_smp against RPN_3D_loss")
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
    if a.smp:
        return smp(a)
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
