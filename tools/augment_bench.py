#!/usr/bin/env python
"""Times the training augmentation kernel -- ``augment_batch`` (m3d_augment_u8, csrc/augment.hip) -- at the training shape: B = 8
uint8 BGR frames of 375x1242 into float32 384x1280 RGB planes, with parameters drawn from the shipped configuration
(mirror_prob 0.5, trans_prob 0.7, shift 0.1, scale_trans 0.4, distort_prob -1), and a second leg with distort_prob = 1 (the
photometric step on every tap).

Yardsticks, measured in the same process on the same frames, alternating with the legs: ``preprocess()`` (m3d_preprocess_u8, the
existing test-time kernel that writes the same 47 MB: what "memory-bound" costs here), and the bytes-moved floor -- the uint8
frames read once plus the float planes written once (58 MB) over the HBM peak.

Two figures per leg, HIP events, `--warmup` untimed samples, `--reps` timed ones (>= 50), median / minimum / interquartile range:
`kernel_ms` -- `--burst` launches through the C ABI back to back into one output buffer between two events, divided by their
number (the device is never waiting for the host: this is the kernel), and `call_ms` -- one `augment_batch()` / `preprocess()`
call between two events, which at these kernel times mostly measures the host side of the call (parameter packing, checks,
allocation, ctypes), not the kernel.

usage: python tools/augment_bench.py [--reps 50] [--warmup 5] [--batch 8] [--burst 20] [--out profiles/augment_bench.jsonl]
(one JSON line per leg, appended to --out)"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3dssd_amd import _hip  # noqa: E402
from m3dssd_amd.config import Conf  # noqa: E402
from m3dssd_amd.host import augment as A  # noqa: E402
from m3dssd_amd.host.preprocess import preprocess  # noqa: E402

MEAN, STDS = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SRC, DST = (375, 1242), (384, 1280)
HBM_PEAK_GBS, HBM_COPY_GBS = 8000.0, 6290.0          # MI355X HBM3E: the specification, and what a float4 copy reaches


def one(fn, k=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def stats(ts):
    ts = sorted(ts)
    n = len(ts)
    return {"median": round(ts[n // 2], 4), "min": round(ts[0], 4), "iqr": round(ts[(3 * n) // 4] - ts[n // 4], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: needs the MI355X (no CPU timing is reported)")
    dev = torch.device("cuda:0")
    B = a.batch
    rng = np.random.RandomState(0)
    frames = torch.from_numpy(rng.randint(0, 256, size=(B,) + SRC + (3,)).astype(np.uint8)).to(dev)
    bytes_moved = B * (SRC[0] * SRC[1] * 3 + DST[0] * DST[1] * 3 * 4)
    floor_ms = bytes_moved / (HBM_PEAK_GBS * 1e9) * 1e3
    L = _hip.lib()
    out = torch.empty(B, 3, DST[0], DST[1], device=dev)
    m3, s3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STDS)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw_pre():
        _hip.check(L.m3d_preprocess_u8(frames.data_ptr(), B, SRC[0], SRC[1], m3, s3, out.data_ptr(), DST[0], DST[1], st))

    def raw_aug(rows):
        _hip.check(L.m3d_augment_u8(frames.data_ptr(), B, SRC[0], SRC[1], rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    A.PARAM_COLS, m3, s3, out.data_ptr(), DST[0], DST[1], st))

    legs = {}
    for name, distort in (("shipped", -1), ("photometric", 1.0)):
        conf = Conf(mirror_prob=0.5, trans_prob=0.7, shift=0.1, scale_trans=0.4, distort_prob=distort)
        params = A.draw_params(conf, [SRC] * B, np.random.RandomState(1))
        rows = A.pack_params(params)
        legs[name] = (params, lambda p=params: A.augment_batch(frames, p, DST, MEAN, STDS), lambda r=rows: raw_aug(r))
    pre = lambda: preprocess(frames, DST, MEAN, STDS)  # noqa: E731
    for _ in range(a.warmup):
        pre()
        one(raw_pre, a.burst)
        for _, fn, raw in legs.values():
            fn()
            one(raw, a.burst)
    torch.cuda.synchronize()
    t_pre, k_pre, t_leg, k_leg = [], [], {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(a.reps):                       # alternating: the legs and the yardstick see the same machine state
        t_pre.append(one(pre))
        k_pre.append(one(raw_pre, a.burst))
        for k, (_, fn, raw) in legs.items():
            t_leg[k].append(one(fn))
            k_leg[k].append(one(raw, a.burst))
    with open(a.out, "a") as f:
        for k, (params, _, _) in legs.items():
            s = stats(k_leg[k])
            line = {"op": "augment_batch", "leg": k, "batch": B, "src": list(SRC), "dst": list(DST), "reps": a.reps,
                    "mirrored": sum(p["mirror"] for p in params), "warped": sum(p["warped"] for p in params),
                    "burst": a.burst, "augment_kernel_ms": s, "preprocess_kernel_ms": stats(k_pre),
                    "augment_call_ms": stats(t_leg[k]), "preprocess_call_ms": stats(t_pre), "bytes_moved_mb": round(bytes_moved / 1e6, 1),
                    "floor_ms_at_hbm_peak": round(floor_ms, 4), "floor_ms_at_copy_rate": round(floor_ms * HBM_PEAK_GBS / HBM_COPY_GBS, 4), "gb_per_s": round(bytes_moved / s["median"] / 1e6, 1),
                    "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
