#!/usr/bin/env python
"""Times the DCNv2 operator of the training path -- m3d_dcn_v2_backward, m3d_dcn_v2_backward_bf16 and, with
--forward, m3d_dcn_v2_forward / m3d_dcn_v2_forward_bf16 (all four in csrc/dcn_op.hip) -- on the deformable layers of the M3DSSD
DLA-34 plan at batch 8: the four DeformConv shapes of the IDA up-sampling path plus shape_align (3x3, offsets of several pixels)
and center_align (1x1).

HIP events around one call, `--warmup` untimed calls, `--reps` timed ones (>= 50), median and minimum reported.  Besides the full
backward call (all five gradients) it times the call with subsets of the gradient pointers set, which isolates the stages:
  weight_only   sampling kernel (writes col) + weight-gradient GEMM + slab reduce
  input_only    column-gradient GEMM + sampling kernel with the atomic scatter
  offmask_only  column-gradient GEMM + sampling kernel without atomics
--dtype f32 | bf16 | both.  With `both` the two types alternate per shape and mode inside one process -- f32, bf16, f32 again --
and the line carries, per mode, the medians of the three legs, `spread_ms` = |median of the second f32 leg - median of the first|
(the run-to-run allowance) and `bf16_not_slower` = bf16 median <= first f32 median + spread.
Budget printed next to the backward measurement: the scatter adds N*Ho*Wo * kk * 4 corners * C * 4 bytes at
the chip-wide float-atomic rate of 1.3 TB/s (fp32 atomics in both types), plus the two GEMMs of 2 * N*Ho*Wo * Co * kk*C FLOP each
at the rate the forward's wave-granular convolution reaches (94 TFLOP/s).

--deterministic times m3d_dcn_v2_backward_det / _det_bf16 (grad_input as a 64-bit fixed-point sum: bitwise reproducible) next to the
float-atomic form: per shape and type, for the full call and for grad_input alone, the legs float, det, float again alternate inside
one process; the line carries their medians and interquartile ranges, `spread_ms` as above, `det_over_float` = det median / first
float median and, for grad_input alone, the rate of the 64-bit atomics if they were all the call did (`atomic_bytes` = N*Ho*Wo * kk *
4 corners * C * 8 bytes over the det median: a lower bound of the rate, the GEMM and the sampling are in the time).  The lines also
go to --out (default profiles/dcn_backward_det_bench.jsonl).

usage: python tools/dcn_backward_bench.py [--reps 50] [--warmup 5] [--batch 8] [--dtype f32|bf16|both] [--forward]
       python tools/dcn_backward_bench.py --deterministic [--reps 50] [--warmup 5] [--batch 8] [--out FILE]
(one JSON line per shape on stdout)"""
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


class Leg:
    """One compute type of one shape: its device tensors, workspaces and the two calls."""

    def __init__(self, dtype, data, geom, pad, dev, stream, det=False):
        self.bf16 = dtype == "bf16"
        L = self.L = _hip.lib()
        dt = torch.bfloat16 if self.bf16 else torch.float32
        x, off, m, wt, b, go = data
        self.x, self.wt, self.go = x.to(dt), wt.to(dt), go.to(dt)
        self.off, self.m, self.b = off, m, b                       # offsets / masks / bias stay float32 in both types
        n, c, h, w, co, k = geom
        self.out = torch.empty(n, co, h, w, device=dev, dtype=dt)
        self.grads = [torch.empty_like(self.x), torch.empty_like(off), torch.empty_like(m), torch.empty_like(self.wt),
                      torch.empty(co, device=dev)]
        q = (n, c, h, w, co, k, k, 1, pad, 1, 1)
        self.fbytes = (L.m3d_dcn_v2_workspace_bytes_bf16 if self.bf16 else L.m3d_dcn_v2_workspace_bytes_grouped)(*q)
        name = "m3d_dcn_v2_backward_det" if det else "m3d_dcn_v2_backward"
        self.bwd = getattr(L, name + ("_bf16" if self.bf16 else ""))
        self.bbytes = getattr(L, name + "_workspace_bytes" + ("_bf16" if self.bf16 else ""))(*q)
        self.ws = torch.empty(max(self.fbytes, self.bbytes) + 256, device=dev, dtype=torch.uint8)
        self.base = (self.ws.data_ptr() + 255) // 256 * 256
        self.tail = (n, c, h, w, co, k, k, 1, 1, pad, pad, 1, 1, 1, self.base)
        self.stream = stream

    def forward(self):
        L, p = self.L, lambda t: t.data_ptr()                      # noqa: E731
        if self.bf16:
            rc = L.m3d_dcn_v2_forward_bf16(p(self.x), p(self.wt), p(self.b), p(self.off), 0, p(self.m), 0, p(self.out), *self.tail,
                                           self.fbytes, self.stream)
        else:
            rc = L.m3d_dcn_v2_forward(p(self.x), p(self.wt), p(self.b), p(self.off), p(self.m), p(self.out), *self.tail, self.fbytes,
                                      self.stream)
        _hip.check(rc)

    def backward(self, want):
        L, p = self.L, lambda t: t.data_ptr()                      # noqa: E731
        ptrs = [t.data_ptr() if wnt else None for t, wnt in zip(self.grads, want)]
        if self.bf16:
            rc = self.bwd(p(self.x), p(self.wt), p(self.off), 0, p(self.m), 0, p(self.go), *ptrs, *self.tail, self.bbytes, self.stream)
        else:
            rc = self.bwd(p(self.x), p(self.wt), p(self.off), p(self.m), p(self.go), *ptrs, *self.tail, self.bbytes, self.stream)
        _hip.check(rc)


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


def make_data(n, c, co, h, w, k, sigma, dev):
    kk = k * k
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, c, h, w, generator=g).to(dev)
    off = (torch.randn(n, 2 * kk, h, w, generator=g) * sigma).to(dev)
    m = torch.sigmoid(torch.randn(n, kk, h, w, generator=g)).to(dev)
    wt = (torch.randn(co, c, k, k, generator=g) / (c * kk) ** 0.5).to(dev)
    go = torch.randn(n, co, h, w, generator=g).to(dev)
    return x, off, m, wt, torch.zeros(co, device=dev), go


def main_deterministic(a, dev, stream):
    out = open(a.out, "w") if a.out else None
    for name, c, co, h, w, k, pad, sigma in SHAPES:
        n, kk = a.batch, k * k
        data = make_data(n, c, co, h, w, k, sigma, dev)
        res = {"shape": name, "batch": n, "reps": a.reps, "op": "backward_det", "workspace_mb": {}}
        atomic_bytes = n * h * w * kk * 4 * c * 8
        for dtype in ("f32", "bf16"):
            legs = {"float": Leg(dtype, data, (n, c, h, w, co, k), pad, dev, stream),
                    "det": Leg(dtype, data, (n, c, h, w, co, k), pad, dev, stream, det=True)}
            res["workspace_mb"][dtype] = {form: round(lg.bbytes / 2 ** 20, 1) for form, lg in legs.items()}
            for mode in ("all", "input_only"):
                entry = {}
                for o in ("float", "det", "float_repeat"):
                    lg = legs[o.split("_")[0]]
                    entry[o] = timed(lambda: lg.backward(MODES[mode]), a.warmup, a.reps)
                entry["spread_ms"] = round(abs(entry["float_repeat"]["median"] - entry["float"]["median"]), 4)
                entry["det_over_float"] = round(entry["det"]["median"] / entry["float"]["median"], 3)
                if mode == "input_only":
                    entry["atomic_bytes"] = atomic_bytes
                    entry["atomic_tb_per_s_at_least"] = round(atomic_bytes / (entry["det"]["median"] * 1e-3) / 1e12, 3)
                res.setdefault(mode + "_ms", {})[dtype] = entry
            del legs
        line = json.dumps(res)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dtype", choices=("f32", "bf16", "both"), default="f32")
    ap.add_argument("--forward", action="store_true", help="time the operator's forward instead of the backward")
    ap.add_argument("--deterministic", action="store_true", help="time the bitwise-reproducible backward next to the float-atomic one")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "dcn_backward_det_bench.jsonl"), help="--deterministic: file the lines go to")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dcn_backward_bench: no ROCm device")
    dev = torch.device("cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if a.deterministic:
        return main_deterministic(a, dev, stream)
    order = {"f32": ("f32",), "bf16": ("bf16",), "both": ("f32", "bf16", "f32_repeat")}[a.dtype]
    for name, c, co, h, w, k, pad, sigma in SHAPES:
        n, kk = a.batch, k * k
        x, off, m, wt, b, go = make_data(n, c, co, h, w, k, sigma, dev)
        legs = {d: Leg(d, (x, off, m, wt, b, go), (n, c, h, w, co, k), pad, dev, stream) for d in set(o.split("_")[0] for o in order)}
        res = {"shape": name, "batch": n, "reps": a.reps, "op": "forward" if a.forward else "backward", "dtype": a.dtype,
               "workspace_mb": {d: round((lg.fbytes if a.forward else lg.bbytes) / 2 ** 20, 1) for d, lg in legs.items()}}
        modes = {"forward": None} if a.forward else MODES
        for mode, want in modes.items():
            entry = {}
            for o in order:
                lg = legs[o.split("_")[0]]
                entry[o] = timed(lg.forward if a.forward else (lambda: lg.backward(want)), a.warmup, a.reps)
            if a.dtype == "both":
                spread = abs(entry["f32_repeat"]["median"] - entry["f32"]["median"])
                entry["spread_ms"] = round(spread, 4)
                entry["bf16_not_slower"] = entry["bf16"]["median"] <= entry["f32"]["median"] + spread
            else:
                entry = entry[order[0]]
            res[mode + "_ms"] = entry
        if not a.forward:
            P = n * h * w
            atomic_ms = P * kk * 4 * c * 4 / ATOMIC_BYTES_PER_S * 1e3
            gemm_ms = 2.0 * P * co * kk * c / GEMM_FLOPS * 1e3
            res["budget_ms"] = {"atomic_scatter": round(atomic_ms, 4), "each_gemm": round(gemm_ms, 4),
                                "total": round(atomic_ms + 2 * gemm_ms, 4)}
            full = res["all_ms"]
            med = {o: full[o]["median"] for o in order} if a.dtype == "both" else {order[0]: full["median"]}
            res["measured_over_budget"] = {o: round(v / (atomic_ms + 2 * gemm_ms), 2) for o, v in med.items()}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
