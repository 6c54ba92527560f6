#!/usr/bin/env python
"""Times the ANAB attention core of the training path -- ``ops.anab_attention`` (m3d_anab_attention_forward +
m3d_anab_attention_backward, csrc/anab_train.hip), forward + backward of all four gradients -- against the float32 torch
composition of the same operator (gated adaptive pooling, bmm, softmax, bmm under autograd) on the same inputs in the same
process, at B = 8 on the 48x160 map of a 384x1280 frame for (Ck, Cv) = (168, 128) (DLA-34) and (168, 256) (DLA-102).

HIP events around one forward + backward, `--warmup` untimed iterations, `--reps` timed ones (>= 50), median and minimum reported;
`torch.cuda.max_memory_allocated` of one iteration of each (above what the inputs hold) next to them.  With `--iteration` it also
times one full training iteration (anab_fullalign, DLA-34, B = 2 at 384x1280: forward, RPN_3D_loss, backward, SGD step) for the
record.

With `--dtype bf16` the operator leg is ``ops.anab_attention_bf16`` (the bf16 instantiation of the same csrc/anab_train.hip) against the parent path on the same bf16 tensors
(``ops.anab_attention`` under torch.autocast(bfloat16)), with the interquartile range of each leg, and `--iteration` runs under
autocast with ``ANAB.bf16_attention`` off and on.

usage: python tools/anab_train_bench.py [--reps 50] [--warmup 5] [--batch 8] [--dtype f32|bf16] [--iteration]
(one JSON line per measurement)"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3dssd_amd.host import ops  # noqa: E402

PSP = (1, 4, 8, 16)


def torch_core(q, k, v, g, B, H, W):
    def planes(t):
        return t.reshape(B, H, W, t.shape[-1]).permute(0, 3, 1, 2)

    kk, vv, gg = planes(k), planes(v), planes(g)
    kp = torch.cat([F.adaptive_avg_pool2d(kk * gg[:, i:i + 1], (z, z)).flatten(2) for i, z in enumerate(PSP)], -1)
    vp = torch.cat([F.adaptive_avg_pool2d(vv * gg[:, i:i + 1], (z, z)).flatten(2) for i, z in enumerate(PSP)], -1)
    att = torch.softmax(torch.bmm(q.reshape(B, H * W, -1), kp), dim=-1)
    return torch.bmm(att, vp.transpose(1, 2)).reshape(B * H * W, -1)


def timed(fn, warmup, reps):
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
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "iqr": round(ts[(3 * len(ts)) // 4] - ts[len(ts) // 4], 4)}


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def bench_operator(a, dev, ck, cv, H=48, W=160):
    B, n = a.batch, a.batch * H * W
    g = torch.Generator().manual_seed(1)
    # the module's layout: one row matrix, q | k | v | gates as column slices
    wide = torch.randn(n, 2 * ck + cv + 4, generator=g)
    wide[:, :ck] *= 0.3
    wide[:, 2 * ck + cv:] = torch.sigmoid(wide[:, 2 * ck + cv:])
    wide = wide.to(dev)
    go = torch.randn(n, cv, generator=g).to(dev)
    leaves = [wide[:, :ck], wide[:, ck:2 * ck], wide[:, 2 * ck:2 * ck + cv], wide[:, 2 * ck + cv:]]

    def step(fn):
        ts = [t.detach().requires_grad_(True) for t in leaves]
        fn(*ts, B, H, W).backward(go)

    res = {"op": "anab_attention forward+backward", "batch": B, "H": H, "W": W, "Ck": ck, "Cv": cv, "reps": a.reps}
    res["hip_ms"] = timed(lambda: step(ops.anab_attention), a.warmup, a.reps)
    res["torch_f32_ms"] = timed(lambda: step(torch_core), a.warmup, a.reps)
    res["hip_peak_mb"] = peak_mb(lambda: step(ops.anab_attention))
    res["torch_f32_peak_mb"] = peak_mb(lambda: step(torch_core))
    print(json.dumps(res), flush=True)


def bench_operator_bf16(a, dev, ck, cv, H=48, W=160):
    """``ops.anab_attention_bf16`` against the parent path on the same bf16 tensors in the same process: ``ops.anab_attention`` under
    torch.autocast(bfloat16), whose custom_fwd casts the four slices to float32 and hands a float32 activation back.  The rows are
    the module's: q | k | v | gates as column slices of one bf16 matrix padded to a row stride that is a multiple of 8."""
    B, n = a.batch, a.batch * H * W
    g = torch.Generator().manual_seed(1)
    width = (2 * ck + cv + 4 + 7) // 8 * 8
    wide = torch.randn(n, width, generator=g)
    wide[:, :ck] *= 0.3
    wide[:, 2 * ck + cv:] = torch.sigmoid(wide[:, 2 * ck + cv:])
    wide = wide.to(dev).bfloat16()
    go = torch.randn(n, cv, generator=g).to(dev)
    go16 = go.bfloat16()
    leaves = [wide[:, :ck], wide[:, ck:2 * ck], wide[:, 2 * ck:2 * ck + cv], wide[:, 2 * ck + cv:2 * ck + cv + 4]]

    def step16():
        ts = [t.detach().requires_grad_(True) for t in leaves]
        ops.anab_attention_bf16(*ts, B, H, W).backward(go16)

    def step_parent():
        ts = [t.detach().requires_grad_(True) for t in leaves]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = ops.anab_attention(*ts, B, H, W)
        out.backward(go)

    res = {"op": "anab_attention_bf16 forward+backward", "batch": B, "H": H, "W": W, "Ck": ck, "Cv": cv, "reps": a.reps}
    res["hip_bf16_ms"] = timed(step16, a.warmup, a.reps)
    res["parent_autocast_ms"] = timed(step_parent, a.warmup, a.reps)
    res["hip_bf16_peak_mb"] = peak_mb(step16)
    res["parent_autocast_peak_mb"] = peak_mb(step_parent)
    print(json.dumps(res), flush=True)


def iteration_case(dev):
    """(net in train mode, conf, frames, imobjs, criterion) of the timed training iteration: anab_fullalign, DLA-34, B = 2 at
    384x1280, eight ground truths per image (shared with tools/optim_bench.py)."""
    from m3dssd_amd import synth
    from m3dssd_amd.config import Conf
    from model.M3d_inference_align import build
    from lib.loss.rpn_3d import RPN_3D_loss
    import numpy as np
    crop, B = (384, 1280), 2
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0", **synth.config_flags("anab_fullalign"))
    conf.update(dict(min_gt_vis=0.65, box_samples=0.20, fg_fraction=0.20, bg_thresh_lo=0, bg_thresh_hi=0.5, fg_thresh=0.5,
                     ign_thresh=0.5, best_thresh=0.35, hard_negatives=True, focal_loss=0, cls_2d_lambda=1, iou_2d_lambda=1,
                     bbox_2d_lambda=0, bbox_3d_lambda=1, bbox_3d_proj_lambda=0.0))
    net = build(conf, "train")
    net.load_state_dict(synth.synth_state_dict(0))
    net = net.to(dev).train()
    x = synth.synth_frames(B, crop, 1234).to(dev)
    rng = np.random.default_rng(5)
    imobjs = []
    for _ in range(B):
        gts = []
        for i in range(8):
            h = float(rng.uniform(60, 250))
            w = float(h * rng.uniform(0.6, 1.5))
            bx, by = float(rng.uniform(0, crop[1] - w)), float(rng.uniform(0, crop[0] - h))
            b3 = [bx + w / 2, by + h / 2, float(rng.uniform(5, 60)), 1.6, 1.5, 3.9, float(rng.uniform(-3, 3)), 0.0, 1.0, 20.0]
            gts.append(Conf(cls=("Car", "Pedestrian", "Cyclist")[i % 3], ign=False, visibility=1.0, bbox_full=np.array([bx, by, w, h]),
                            bbox_3d=b3))
        imobjs.append(Conf(gts=gts, p2=np.eye(4), p2_inv=np.eye(4), scale_factor=1.0))
    return net, conf, x, imobjs, RPN_3D_loss(conf)


def bench_iteration(a, dev, autocast=False):
    net, conf, x, imobjs, crit = iteration_case(dev)
    crop, B = (384, 1280), 2
    opt = torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            cls, prob, b2, b3, fs = net(x)
        loss, _ = crit(cls.float(), prob.float(), b2.float(), b3.float(), imobjs, fs)
        opt.zero_grad()
        loss.backward()
        opt.step()

    from m3dssd_amd.host import train
    for flag in ((False, True) if autocast else (False,)):
        train.set_bf16_attention(net, flag)
        res = {"op": "training iteration anab_fullalign dla34", "batch": B, "crop": list(crop), "reps": min(a.reps, 10)}
        if autocast:
            res.update(autocast="bfloat16", bf16_attention=flag)
        res["iteration_ms"] = timed(step, 2, min(a.reps, 10))
        res["peak_mb"] = peak_mb(step)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iteration", action="store_true", help="also time one full training iteration (B = 2, 384x1280)")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32",
                    help="bf16: ops.anab_attention_bf16 against ops.anab_attention under autocast; --iteration then runs under autocast "
                         "with ANAB.bf16_attention off and on")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anab_train_bench: no ROCm device")
    dev = torch.device("cuda:0")
    for ck, cv in ((168, 128), (168, 256)):
        (bench_operator_bf16 if a.dtype == "bf16" else bench_operator)(a, dev, ck, cv)
    if a.iteration:
        bench_iteration(a, dev, autocast=a.dtype == "bf16")


if __name__ == "__main__":
    main()
