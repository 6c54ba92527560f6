#!/usr/bin/env python
"""Times the deformable PS-ROI pooling operator -- m3d_dcn_v2_psroi_pooling_forward / _backward (csrc/psroi_pool.hip) -- next to
the float32 torch restatement of the same definition (tests/psroi_ref.py, run on the same device, backward through autograd) at
three shapes:
  example        model/DCNv2/test.py's example: data 2x32x64x64, 20 regions, P = 7, D = 32, G = 1
  ps_head        a position-sensitive head: C = 490, D = 10, G = 7, P = 7, 300 regions on 48x160
  roi_align      an RoI-align-like head: D = 256, G = 1, P = 7, 300 regions on 48x160
HIP events around one call, `--warmup` untimed calls, `--reps` timed ones (>= 50), median and minimum reported.

Bytes each form has to move (printed per shape, an accounting, not a measurement):
  kernels   forward: the pack of D*G*G channels (read + write), the four corner reads of every COUNTED sample
            (n*D*P*P * S*S * 4 floats times `samples_counted`, the share of the samples that fall on the map; served by the
            caches after the first touch of a row) and the two outputs;
            backward: the pack, the zero fill and the unpack of the staging buffer, the corner reads once more, as many atomic
            adds (`atomic_budget_ms`: those bytes at the float-atomic rate of DESIGN.md section 3, 1.3 TB/s of added bytes; a corner
            of weight 0 is skipped, which the count ignores) and grad_out.
  torch     per sample 4 indexed reads (8-byte index + 4-byte value in, 4 bytes out) and about 24 element-wise passes over
            [n, D, P, P] float32 tensors (3 floats moved per pass); autograd's backward about doubles it.

usage: python tools/psroi_pool_bench.py [--reps 50] [--warmup 5] [--no-torch]          (one JSON line per shape on stdout)"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from m3dssd_amd import _hip  # noqa: E402
import psroi_ref  # noqa: E402

ATOMIC_BYTES_PER_S = 1.3e12

# name, N, C, H, W, regions, D, G, P, S, region corner range, region size range (image pixels at scale 1/4)
SHAPES = [
    ("example 2x32x64x64 n20 P7 D32 G1", 2, 32, 64, 64, 20, 32, 1, 7, 4, 256, 64),
    ("ps_head 2x490x48x160 n300 P7 D10 G7", 2, 490, 48, 160, 300, 10, 7, 7, 4, 560, 160),
    ("roi_align 2x256x48x160 n300 P7 D256 G1", 2, 256, 48, 160, 300, 256, 1, 7, 4, 560, 160),
]


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
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch restatement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("psroi_pool_bench: no ROCm device")
    dev = torch.device("cuda:0")
    L = _hip.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, N, C, H, W, n, D, G, P, S, xy_max, wh_max in SHAPES:
        g = torch.Generator().manual_seed(1)
        data = torch.randn(N, C, H, W, generator=g).to(dev)
        rois = psroi_ref.make_rois(n, N, 2, xy_max=xy_max, wh_max=wh_max).to(dev)
        # the map covers 4 * W x 4 * H image pixels: keep the corners on it, as a detector's proposals are
        rois[:, 1].clamp_(max=4 * W - 1)
        rois[:, 3].clamp_(max=4 * W - 1)
        rois[:, 2].clamp_(max=4 * H - 1)
        rois[:, 4].clamp_(max=4 * H - 1)
        trans = torch.randn(n, 2, P, P, generator=g).to(dev)
        go = torch.randn(n, D, P, P, generator=g).to(dev)
        conf = (False, 0.25, D, G, P, P, S, 0.1)
        out, cnt = torch.empty(n, D, P, P, device=dev), torch.empty(n, D, P, P, device=dev)
        gd, gt = torch.empty_like(data), torch.empty_like(trans)
        q = (N, C, H, W, n, 1, D, G, P)
        fbytes, bbytes = L.m3d_dcn_v2_psroi_pooling_workspace_bytes(*q, 0), L.m3d_dcn_v2_psroi_pooling_workspace_bytes(*q, 1)
        ws = torch.empty(bbytes + 256, device=dev, dtype=torch.uint8)
        base = (ws.data_ptr() + 255) // 256 * 256
        tail = (N, C, H, W, n, n, 1, 0, 0.25, D, G, P, P, S, 0.1, base)
        p = lambda t: t.data_ptr()                                      # noqa: E731

        def fwd():
            _hip.check(L.m3d_dcn_v2_psroi_pooling_forward(p(data), p(rois), p(trans), p(out), p(cnt), *tail, fbytes, stream))

        def bwd(want=(1, 1)):
            _hip.check(L.m3d_dcn_v2_psroi_pooling_backward(p(go), p(data), p(rois), p(trans), p(gd) if want[0] else None,
                                                           p(gt) if want[1] else None, *tail, bbytes, stream))

        res = {"shape": name, "reps": a.reps, "workspace_mb": {"forward": round(fbytes / 2 ** 20, 2), "backward": round(bbytes / 2 ** 20, 2)}}
        res["forward_ms"] = timed(fwd, a.warmup, a.reps)
        res["backward_ms"] = timed(bwd, a.warmup, a.reps)
        res["backward_data_only_ms"] = timed(lambda: bwd((1, 0)), a.warmup, a.reps)
        res["backward_trans_only_ms"] = timed(lambda: bwd((0, 1)), a.warmup, a.reps)
        elems, plane = n * D * P * P, N * H * W * D * G * G * 4
        fwd()
        torch.cuda.synchronize()
        frac = float(cnt.sum().item()) / (elems * S * S)                # the share of the samples that count: only they are read or added
        gather = int(elems * S * S * 4 * 4 * frac)
        res["kernel_bytes_mb"] = {"forward": round((2 * plane + gather + 2 * elems * 4) / 1e6, 2),
                                  "backward": round((2 * plane + 3 * plane + N * C * H * W * 4 + 2 * gather + elems * 4) / 1e6, 2)}
        res["atomic_budget_ms"] = round(gather / ATOMIC_BYTES_PER_S * 1e3, 4)
        res["samples_counted"] = round(frac, 3)
        res["bins_with_samples"] = round(float((cnt > 0).float().mean().item()), 3)
        if not a.no_torch:
            d32, t32 = data.clone().requires_grad_(True), trans.clone().requires_grad_(True)

            def tfwd():
                with torch.no_grad():
                    psroi_ref.psroi_ref(data, rois, trans, conf)

            def tboth():
                d32.grad = t32.grad = None
                psroi_ref.psroi_ref(d32, rois, t32, conf)[0].backward(go)

            res["torch_forward_ms"] = timed(tfwd, 2, max(5, a.reps // 5))
            res["torch_forward_backward_ms"] = timed(tboth, 2, max(5, a.reps // 5))
            tf = S * S * elems * (4 * 16 + 24 * 12)
            res["torch_bytes_mb"] = {"forward": round(tf / 1e6, 2), "forward_backward": round(3 * tf / 1e6, 2)}
            ref = psroi_ref.psroi_ref(data, rois, trans, conf)[0]
            res["max_abs_diff_vs_torch"] = float((out - ref).abs().max().item())
            res["kernels_faster"] = {"forward": res["forward_ms"]["median"] < res["torch_forward_ms"]["median"],
                                     "forward_backward": res["forward_ms"]["median"] + res["backward_ms"]["median"]
                                     < res["torch_forward_backward_ms"]["median"]}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
