#!/usr/bin/env python
"""Step time of each model configuration (anab_fullalign, base, anab) at 1280x384 on one GPU, in the measurement mode of
bench.py's headline (pipelined hipGraph step: forward(batch k) beside detect(batch k-1), K batches + the final flush timed,
warm-up replays directly in front), for fp32 at bs 8 and bf16 at bs 64.  The configurations are measured in one process,
one after the other, and the whole set is repeated `--rounds` times, so that they are compared on the same clock state.

    python tools/config_step_time.py [--steps K] [--warmup W] [--rounds R] [--configs base,anab,...]

Prints one JSON line per (round, config, dtype): ms per step and images per second.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CROP = (384, 1280)
LEGS = (("f32", 8), ("bf16", 64))


def time_config(config, dtype, B, steps, warmup):
    import torch
    from m3dssd_amd import synth
    from m3dssd_amd.pipeline import PipelinedDetector
    from model.M3d_inference_align import build
    dev = torch.device("cuda:0")
    flags = synth.config_flags(config)
    conf = synth.synth_conf(CROP, 0, batch_size=B, device=str(dev), **flags)
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, **flags), strict=True)
    net = net.to(dev).set_compute_dtype(dtype)
    pipe = PipelinedDetector(net, conf, B, CROP[0], CROP[1])
    pipe.input.copy_(synth.synth_frames(B, CROP, 1234).to(dev))
    for _ in range(max(1, warmup)):
        pipe.step(as_block=True)
    pipe.flush(as_block=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        pipe.step(as_block=True)
    pipe.flush(as_block=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n_ops = len(net.engine().plan_for(B, *CROP).ops)
    del pipe, net
    torch.cuda.empty_cache()
    return dict(config=config, dtype=dtype, batch=B, steps=steps, ms_per_step=round(1e3 * dt / steps, 4),
                images_per_s=round(B * steps / dt, 1), launches=n_ops)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--configs", default="anab_fullalign,base,anab")
    args = ap.parse_args(argv)
    configs = args.configs.split(",")
    for r in range(args.rounds):
        for dtype, B in LEGS:
            for config in (configs if r % 2 == 0 else configs[::-1]):      # alternate the order between rounds
                res = time_config(config, dtype, B, args.steps, args.warmup)
                print(json.dumps(dict(round=r, **res)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
