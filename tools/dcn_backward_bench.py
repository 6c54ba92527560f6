#!/usr/bin/env python
"""Times m3d_dcn_v2_backward (csrc/dcn_backward.hip) on the deformable layers of the M3DSSD DLA-34 plan at batch 8: the four
DeformConv shapes of the IDA up-sampling path plus shape_align (3x3, offsets of several pixels) and center_align (1x1).

HIP events around one call, `--warmup` untimed calls, `--reps` timed ones (>= 50), median and minimum reported.  Besides the full
call (all five gradients) it times the call with subsets of the gradient pointers set, which isolates the stages:
  weight_only   sampling kernel (writes col) + weight-gradient GEMM + slab reduce
  input_only    column-gradient GEMM + sampling kernel with the atomic scatter
  offmask_only  column-gradient GEMM + sampling kernel without atomics
Budget printed next to the measurement: the scatter adds N*Ho*Wo * kk * 4 corners * C * 4 bytes at the
chip-wide float-atomic rate of 1.3 TB/s, plus the two GEMMs of 2 * N*Ho*Wo * Co * kk*C FLOP each at the rate the forward's
wave-granular convolution reaches (94 TFLOP/s).

usage: python tools/dcn_backward_bench.py [--reps 50] [--warmup 5] [--batch 8]      (one JSON line per shape on stdout)"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from m3dssd_amd import _hip  # noqa: E402

ATOMIC_BYTES_PER_S = 1.3e12
GEMM_FLOPS = 94e12

# name, C, Co, H, W, k, pad, offset sigma
SHAPES = [
    ("ida_0.proj_1 512->256 12x40", 512, 256, 12, 40, 3, 1, 3.0),
    ("ida_0.node_1 256->256 24x80", 256, 256, 24, 80, 3, 1, 3.0),
    ("ida_1.proj_1 256->128 24x80", 256, 128, 24, 80, 3, 1, 3.0),
    ("ida_1.node_1 128->128 48x160", 128, 128, 48, 160, 3, 1, 3.0),
    ("shape_align 128->128 48x160", 128, 128, 48, 160, 3, 1, 6.0),
    ("center_align 128->128 48x160 1x1", 128, 128, 48, 160, 1, 0, 3.0),
]
MODES = {"all": (1, 1, 1, 1, 1), "weight_only": (0, 0, 0, 1, 0), "input_only": (1, 0, 0, 0, 0), "offmask_only": (0, 1, 1, 0, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dcn_backward_bench: no ROCm device")
    dev = torch.device("cuda:0")
    L = _hip.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, c, co, h, w, k, pad, sigma in SHAPES:
        n, kk = a.batch, k * k
        g = torch.Generator().manual_seed(1)
        x = torch.randn(n, c, h, w, generator=g).to(dev)
        off = (torch.randn(n, 2 * kk, h, w, generator=g) * sigma).to(dev)
        m = torch.sigmoid(torch.randn(n, kk, h, w, generator=g)).to(dev)
        wt = (torch.randn(co, c, k, k, generator=g) / (c * kk) ** 0.5).to(dev)
        go = torch.randn(n, co, h, w, generator=g).to(dev)
        outs = [torch.empty_like(x), torch.empty_like(off), torch.empty_like(m), torch.empty_like(wt), torch.empty(co, device=dev)]
        nbytes = L.m3d_dcn_v2_backward_workspace_bytes(n, c, h, w, co, k, k, 1, pad, 1, 1)
        ws = torch.empty(nbytes + 256, device=dev, dtype=torch.uint8)
        base = (ws.data_ptr() + 255) // 256 * 256

        def call(want):
            ptrs = [t.data_ptr() if wnt else None for t, wnt in zip(outs, want)]
            _hip.check(L.m3d_dcn_v2_backward(x.data_ptr(), wt.data_ptr(), off.data_ptr(), m.data_ptr(), go.data_ptr(), *ptrs, n, c, h, w,
                                             co, k, k, 1, 1, pad, pad, 1, 1, 1, base, nbytes, stream))

        res = {"shape": name, "batch": n, "reps": a.reps, "workspace_mb": round(nbytes / 2 ** 20, 1)}
        for mode, want in MODES.items():
            for _ in range(a.warmup):
                call(want)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(want)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            ts.sort()
            res[mode + "_ms"] = {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4)}
        P = n * h * w
        atomic_ms = P * kk * 4 * c * 4 / ATOMIC_BYTES_PER_S * 1e3
        gemm_ms = 2.0 * P * co * kk * c / GEMM_FLOPS * 1e3
        res["budget_ms"] = {"atomic_scatter": round(atomic_ms, 4), "each_gemm": round(gemm_ms, 4), "total": round(atomic_ms + 2 * gemm_ms, 4)}
        res["measured_over_budget"] = round(res["all_ms"]["median"] / (atomic_ms + 2 * gemm_ms), 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
