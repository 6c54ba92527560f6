#!/usr/bin/env python
"""Step time of each model configuration (anab_fullalign, base, anab) at 1280x384 on one GPU, in the measurement mode of
bench.py's headline (pipelined hipGraph step: forward(batch k) beside detect(batch k-1), K batches + the final flush timed,
warm-up replays directly in front), for fp32 at bs 8 and bf16 at bs 64.  The configurations are measured in one process,
one after the other, and the whole set is repeated `--rounds` times, so that they are compared on the same clock state.

    python tools/config_step_time.py [--steps K] [--warmup W] [--rounds R] [--configs base,anab,...] [--back-bone dla34,dla102]
                                     [--legs f32,bf16]

``--back-bone`` lists the backbones to time (default dla34); DLA-102 runs its fp32 leg only (there is no bf16 DLA-102 plan).
``--legs`` keeps only the named dtype legs (default both), e.g. ``--legs f32`` for the fp32 comparison of the two backbones.

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


def time_config(config, dtype, B, steps, warmup, back_bone="dla34"):
    import torch
    from m3dssd_amd import synth
    from m3dssd_amd.pipeline import PipelinedDetector
    from model.M3d_inference_align import build
    dev = torch.device("cuda:0")
    flags = synth.config_flags(config)
    conf = synth.synth_conf(CROP, 0, batch_size=B, device=str(dev), back_bone=back_bone, **flags)
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, back_bone=back_bone, **flags), strict=True)
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
    return dict(config=config, back_bone=back_bone, dtype=dtype, batch=B, steps=steps, ms_per_step=round(1e3 * dt / steps, 4),
                images_per_s=round(B * steps / dt, 1), launches=n_ops)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--configs", default="anab_fullalign,base,anab")
    ap.add_argument("--back-bone", default="dla34", help="comma-separated backbones (dla34, dla102)")
    ap.add_argument("--legs", default=None, help="only these dtypes (f32, bf16)")
    args = ap.parse_args(argv)
    configs = args.configs.split(",")
    runs = [(bb, c) for bb in args.back_bone.split(",") for c in configs]
    for r in range(args.rounds):
        for dtype, B in LEGS:
            if args.legs and dtype not in args.legs.split(","):
                continue
            for bb, config in (runs if r % 2 == 0 else runs[::-1]):        # alternate the order between rounds
                if dtype == "bf16" and bb != "dla34":
                    continue
                res = time_config(config, dtype, B, args.steps, args.warmup, bb)
                print(json.dumps(dict(round=r, **res)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
