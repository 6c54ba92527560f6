#!/usr/bin/env python
"""Times the fused BatchNorm + residual + activation training operator -- ``ops.bn_act_train`` (m3d_bn_act_train_forward +
m3d_bn_act_train_backward, csrc/bn_train.hip), forward + backward of all gradients -- against the torch composition it replaces
(``nn.BatchNorm2d`` in training mode -> add -> in-place ``LeakyReLU``, autograd behind it) on the same tensors in the same process.

The shapes are the net's own: one training forward of anab_fullalign, DLA-34, B = 2 at 384x1280 with the flag on records (C, H, W,
residual, slope) of every BatchNorm site; equal shapes are grouped (`sites`: how many the net has).  Per group:
  * `hip_ms` / `torch_ms`: HIP events around ONE forward + backward with the device idle at its start, `--warmup` untimed iterations,
    `--reps` timed ones, median and interquartile range.  The two legs ALTERNATE rep by rep: at these sizes most of the figure is
    host time (Python, allocator, launches), and the host's speed drifts by a factor of two inside one process;
  * `hip_stream_ms` / `torch_stream_ms`: 30 forward + backward issued back to back between two events, per iteration: what a
    stream that is kept busy sees (the larger of host issue time and device time); `kernels_stream_ms`: the same for the four
    launches alone, through the C ABI on preallocated tensors;
  * `torch.cuda.max_memory_allocated` of one iteration of each (above what the inputs hold);
  * the bytes-moved floor -- three passes over the tensor forward and five backward, plus one each way with a residual -- at the HBM
    specification of `--hbm-tbs`.

With `--iteration` one full training iteration (the case of tools/anab_train_bench.py --iteration: forward, RPN_3D_loss, backward,
SGD step) is timed with the flag off, on, off and on again in the same process: median of 10 with the interquartile range, and the
peak memory of each.

usage: python tools/bn_train_bench.py [--reps 50] [--warmup 5] [--iteration] [--out profiles/bn_train_bench.jsonl]
(one JSON line per row, on stdout and appended to --out)"""
import argparse
import collections
import json
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3dssd_amd import _hip  # noqa: E402
from m3dssd_amd.host import ops, train  # noqa: E402
from tools.anab_train_bench import iteration_case, peak_mb, timed  # noqa: E402


def emit(a, row):
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def _stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "iqr": round(ts[(3 * len(ts)) // 4] - ts[len(ts) // 4], 4)}


def timed_pair(fn_a, fn_b, warmup, reps):
    """Per-iteration event times of two legs that alternate rep by rep -> (stats of a, stats of b)."""
    for _ in range(warmup):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fn_a, fn_b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return _stats(ts[0]), _stats(ts[1])


def streamed(fn, n=30):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) / n, 4)


def site_shapes(net, x):
    """(C, H, W, residual, slope) -> number of sites, from one flagged training forward."""
    seen = collections.Counter()
    real = ops.bn_act_train

    def record(xx, residual, weight, bias, rm, rv, momentum, eps, slope):
        seen[(xx.shape[1], xx.shape[2], xx.shape[3], residual is not None, round(float(slope), 6))] += 1
        return real(xx, residual, weight, bias, rm, rv, momentum, eps, slope)

    ops.bn_act_train = record
    try:
        n = train.set_fused_batchnorm(net, True)
        net(x)
    finally:
        ops.bn_act_train = real
        train.set_fused_batchnorm(net, False)
    assert sum(seen.values()) == n, "a BatchNorm site did not go through the operator"
    return seen


def bench_shape(a, dev, B, key, sites):
    C, H, W, has_res, slope = key
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    res = torch.randn(B, C, H, W, generator=g).to(dev) if has_res else None
    gy = torch.randn(B, C, H, W, generator=g).to(dev)
    bn = nn.BatchNorm2d(C, momentum=0.1).to(dev).train()
    act = nn.LeakyReLU(slope, inplace=True) if slope != 1.0 else None

    def leaves():
        return x.detach().requires_grad_(True), None if res is None else res.detach().requires_grad_(True)

    def step_hip():
        xx, rr = leaves()
        bn.zero_grad(set_to_none=True)
        ops.bn_act_train(xx, rr, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, slope).backward(gy)

    def step_torch():
        xx, rr = leaves()
        bn.zero_grad(set_to_none=True)
        out = bn(xx)
        if rr is not None:
            out = out + rr
        if act is not None:
            out = act(out)
        out.backward(gy)

    # the four launches alone, through the C ABI on preallocated tensors: what the device (or the bare launch path) takes
    L = _hip.lib()
    y, gx, gr = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x) if has_res else None
    vec = [torch.empty(C, device=dev) for _ in range(4)]                      # save_mean, save_invstd, grad_gamma, grad_beta
    ws_bytes = L.m3d_bn_act_train_workspace_bytes(B, C, H, W)
    ws, base = ops._workspace(ws_bytes, dev)
    stream = ops._stream()

    def step_kernels():
        _hip.check(L.m3d_bn_act_train_forward(x.data_ptr(), None if res is None else res.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(),
                                              bn.running_mean.data_ptr(), bn.running_var.data_ptr(), y.data_ptr(), vec[0].data_ptr(),
                                              vec[1].data_ptr(), B, C, H, W, bn.eps, bn.momentum, slope, base, ws_bytes, stream))
        _hip.check(L.m3d_bn_act_train_backward(gy.data_ptr(), x.data_ptr(), y.data_ptr(), bn.weight.data_ptr(), vec[0].data_ptr(),
                                               vec[1].data_ptr(), gx.data_ptr(), None if gr is None else gr.data_ptr(), vec[2].data_ptr(),
                                               vec[3].data_ptr(), B, C, H, W, slope, base, ws_bytes, stream))

    nbytes = 4 * B * C * H * W
    passes = 3 + 5 + (2 if has_res else 0)
    row = {"op": "bn_act_train forward+backward", "batch": B, "C": C, "H": H, "W": W, "residual": has_res, "slope": slope, "sites": sites,
           "reps": a.reps, "tensor_mb": round(nbytes / 2 ** 20, 2)}
    row["hip_ms"], row["torch_ms"] = timed_pair(step_hip, step_torch, a.warmup, a.reps)
    row["hip_stream_ms"] = min(streamed(step_hip), streamed(step_hip))
    row["torch_stream_ms"] = min(streamed(step_torch), streamed(step_torch))
    row["kernels_stream_ms"] = min(streamed(step_kernels), streamed(step_kernels))
    row["hip_peak_mb"] = peak_mb(step_hip)
    row["torch_peak_mb"] = peak_mb(step_torch)
    row["floor_ms_at_hbm_spec"] = round(passes * nbytes / (a.hbm_tbs * 1e12) * 1e3, 4)
    row["speedup"] = round(row["torch_ms"]["median"] / row["hip_ms"]["median"], 2)
    row["speedup_stream"] = round(row["torch_stream_ms"] / row["hip_stream_ms"], 2)
    emit(a, row)
    return row


def bench_iteration(a, dev, case):
    net, conf, x, imobjs, crit = case
    opt = torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9)

    def step():
        cls, prob, b2, b3, fs = net(x)
        loss, _ = crit(cls, prob, b2, b3, imobjs, fs)
        opt.zero_grad()
        loss.backward()
        opt.step()

    for flag in (False, True, False, True):
        train.set_fused_batchnorm(net, flag)
        row = {"op": "training iteration anab_fullalign dla34", "batch": x.shape[0], "crop": list(x.shape[2:]), "reps": 10,
               "fused_batchnorm": flag}
        row["iteration_ms"] = timed(step, 2, 10)
        row["peak_mb"] = peak_mb(step)
        emit(a, row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM specification in TB/s for the bytes-moved floor")
    ap.add_argument("--iteration", action="store_true", help="also time one full training iteration with the flag off / on / off / on")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bn_train_bench: no ROCm device")
    dev = torch.device("cuda:0")
    case = iteration_case(dev)
    net, x = case[0], case[2]
    shapes = site_shapes(net, x)
    net.zero_grad(set_to_none=True)
    torch.cuda.empty_cache()
    rows = [bench_shape(a, dev, x.shape[0], key, n) for key, n in sorted(shapes.items(), key=lambda kv: (-kv[0][0] * kv[0][1] * kv[0][2], kv[0]))]
    hip = sum(r["hip_ms"]["median"] * r["sites"] for r in rows)
    tor = sum(r["torch_ms"]["median"] * r["sites"] for r in rows)
    emit(a, {"op": "bn_act_train all sites of one iteration (sum of medians x sites)", "sites": sum(r["sites"] for r in rows),
             "shape_classes": len(rows), "hip_ms": round(hip, 3), "torch_ms": round(tor, 3),
             "hip_stream_ms": round(sum(r["hip_stream_ms"] * r["sites"] for r in rows), 3),
             "torch_stream_ms": round(sum(r["torch_stream_ms"] * r["sites"] for r in rows), 3),
             "floor_ms_at_hbm_spec": round(sum(r["floor_ms_at_hbm_spec"] * r["sites"] for r in rows), 3),
             "classes_where_torch_wins": [[r["C"], r["H"], r["W"], r["residual"], r["slope"]] for r in rows if r["speedup"] < 1.0]})
    if a.iteration:
        bench_iteration(a, dev, case)


if __name__ == "__main__":
    main()
