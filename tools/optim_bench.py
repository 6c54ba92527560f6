#!/usr/bin/env python
"""Times the fused optimizer step (m3dssd_amd/host/optim.py: m3d_optim_prepare + m3d_optim_step, csrc/optim.hip) against
``torch.optim`` on the same tensors in the same process.

The parameter set is the training module of anab_fullalign / DLA-34 (every parameter, as ``make_optimizer`` would take them) with
synthetic gradients.  Per solver (SGD with momentum and weight decay, Adam, Adamax) one JSON line with, in milliseconds of HIP
events (median of `--reps` >= 50, minimum, interquartile range, after `--warmup` untimed calls):

    fused              step()                               gradient pass + finish + update
    fused_zero_grads   step(zero_grads=True)                the same with the gradients zeroed in the update pass
    fused_loss         step(loss, skip_nonfinite=True, zero_grads=True)     what the training loop calls
    torch_default      torch.optim.X(...).step()            torch's choice of form for device tensors
    torch_foreach      torch.optim.X(..., foreach=True).step()
    torch_single       torch.optim.X(..., foreach=False).step()             the per-tensor loop
    torch_zero_grad    optimizer.zero_grad(set_to_none=False)               what zero_grads replaces (set_to_none=True costs no kernel,
                                                                            but the next backward then allocates every gradient)

and `floor_ms`: the bytes the fused step has to move (gradients once for the decision; parameters, gradients and state read,
parameters and state written by the update) at the HBM specification of `--hbm-tbs` (8 TB/s on the MI355X).

With `--iteration` it also times one full training iteration (anab_fullalign, DLA-34, B = 2 at 384x1280; the case of
tools/anab_train_bench.py --iteration) with torch.optim.SGD (zero_grad, backward, step) and with each fused solver
(backward, step(loss, skip_nonfinite=True, zero_grads=True)).

usage: python tools/optim_bench.py [--reps 50] [--warmup 5] [--iteration] [--out profiles/optim_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from anab_train_bench import iteration_case, timed  # noqa: E402
from m3dssd_amd.host import optim as O  # noqa: E402

SOLVERS = {
    "sgd": (O.SGD, torch.optim.SGD, dict(lr=1e-6, momentum=0.9, weight_decay=5e-4), 1),
    "adam": (O.Adam, torch.optim.Adam, dict(lr=1e-6, weight_decay=5e-4), 2),
    "adamax": (O.Adamax, torch.optim.Adamax, dict(lr=1e-6, weight_decay=5e-4), 2),
}


def emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def training_parameters(dev):
    from m3dssd_amd import synth
    from model.M3d_inference_align import build
    conf = synth.synth_conf((384, 1280), 0, batch_size=2, device="cuda:0", **synth.config_flags("anab_fullalign"))
    net = build(conf, "train")
    net.load_state_dict(synth.synth_state_dict(0))
    net = net.to(dev).train()
    params = [p for p in net.parameters() if p.requires_grad]
    g = torch.Generator(device=dev).manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-3
    return net, params


def bench_steps(a, dev):
    net, params = training_parameters(dev)
    numel = sum(p.numel() for p in params)
    loss = torch.ones((), device=dev)
    for name, (fused_cls, torch_cls, kw, n_state) in SOLVERS.items():
        res = {"tool": "optim_bench", "kind": "step", "solver": name, "tensors": len(params), "elements": numel, "reps": a.reps,
               "settings": kw}
        fused = fused_cls(params, **kw)
        res["fused"] = timed(lambda: fused.step(), a.warmup, a.reps)
        res["fused_zero_grads"] = timed(lambda: fused.step(zero_grads=True), a.warmup, a.reps)
        res["fused_loss"] = timed(lambda: fused.step(loss=loss, skip_nonfinite=True, zero_grads=True), a.warmup, a.reps)
        res["chunks"] = fused._n_chunks
        del fused
        for leg, extra in (("torch_default", {}), ("torch_foreach", dict(foreach=True)), ("torch_single", dict(foreach=False))):
            opt = torch_cls(params, **kw, **extra)
            res[leg] = timed(lambda: opt.step(), a.warmup, a.reps)
            if leg == "torch_default":
                res["torch_zero_grad"] = timed(lambda: opt.zero_grad(set_to_none=False), a.warmup, a.reps)
            del opt
        # gradients read twice (decision, update), parameters and state read and written
        nbytes = 4 * numel * (2 + 2 + 2 * n_state)
        res["bytes_moved"] = nbytes
        res["bytes_moved_zero_grads"] = nbytes + 4 * numel
        res["hbm_tbs"] = a.hbm_tbs
        res["floor_ms"] = round(nbytes / (a.hbm_tbs * 1e12) * 1e3, 4)
        emit(res, a.out)


def bench_iteration(a, dev):
    reps = min(a.reps, 10)
    for name in ("torch_sgd", "sgd", "adam", "adamax"):
        net, conf, x, imobjs, crit = iteration_case(dev)
        if name == "torch_sgd":
            opt = torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4)

            def step():
                cls, prob, b2, b3, fs = net(x)
                loss, _ = crit(cls, prob, b2, b3, imobjs, fs)
                opt.zero_grad()
                loss.backward()
                if float(loss) > 0:                                 # the reference's host decision (scripts/train_rpn_3d.py:208-218)
                    opt.step()
        else:
            fused_cls, _, kw, _ = SOLVERS[name]
            opt = fused_cls(net.parameters(), **dict(kw, lr=1e-4))

            def step():
                cls, prob, b2, b3, fs = net(x)
                loss, _ = crit(cls, prob, b2, b3, imobjs, fs)
                loss.backward()
                opt.step(loss=loss, skip_nonfinite=True, zero_grads=True)
        res = {"tool": "optim_bench", "kind": "iteration", "optimizer": name, "op": "training iteration anab_fullalign dla34", "batch": 2,
               "crop": [384, 1280], "reps": reps, "iteration_ms": timed(step, 2, reps)}
        emit(res, a.out)
        del opt, net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM specification in TB/s for the bytes-moved floor")
    ap.add_argument("--iteration", action="store_true", help="also time one full training iteration (B = 2, 384x1280) per optimizer")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.jsonl"), help="JSON lines are appended here ('' = stdout only)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: no ROCm device")
    dev = torch.device("cuda:0")
    if a.out and os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    bench_steps(a, dev)
    if a.iteration:
        bench_iteration(a, dev)


if __name__ == "__main__":
    main()
