#!/usr/bin/env python
"""Generate tests/golden/adjust_lr.npz by running the REFERENCE's own adjust_lr (lib/core.py:105-176) over a table of policies.

Build-container only, like tools/gen_golden_bbox_stats.py, whose import stubs (tools/gen_golden.py) it reuses.

The fixture holds numbers only.  One row per policy:
    solver       0 sgd, 1 adam, 2 adamax
    policy       0 step, 1 poly, 2 cos
    lr, lr_target, warmup, max_iter
    lr_steps     [n, 4], NaN padded (all NaN: conf.lr_steps = None)
    batch_skip   0: the key is absent from conf
    group_lrs    [n, 2]: the learning rates of the optimizer's two groups before the call
    iters        [n, 7]: 0, 1, the warm-up boundary - 1, + 0, + 1, mid-run, max_iter
    returned     [n, 7]: 0 where adjust_lr returned None (the batch_skip early return)
    lr_out       [n, 7]: the returned learning rate (float64; NaN where nothing was returned)
    group_out    [n, 7, 2]: the groups' learning rates after the call

Run:  python tools/gen_golden_adjust_lr.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

SOLVERS = ("sgd", "adam", "adamax")
POLICIES = ("step", "poly", "cos")
SHIPPED_ITERS = 70 * 928          # max_epoch 70 (kitti_3d_*.py:25) x ceil(3712 training images / batch 4) (train_rpn_3d.py:115,169)

# solver, policy, lr, lr_target, warmup, max_iter, lr_steps, batch_skip, group lrs
ROWS = [
    ("sgd", "cos", 0.002, 0.002 * 1e-5, 1.0 / 70, SHIPPED_ITERS, None, 0, (0.002, 0.002)),          # kitti_3d_anab(_fullalign).py
    ("sgd", "cos", 0.004, 0.004 * 1e-5, 1.0 / 70, SHIPPED_ITERS, None, 0, (0.004, 0.004)),          # kitti_3d_base.py
    ("sgd", "poly", 0.004, 4e-8, 0.05, 10000, None, 0, (0.004, 0.004)),
    ("sgd", "poly", 0.01, 1e-5, 0.34, 9000, [0.3, 0.6, 0.9], 0, (0.01, 0.01)),
    ("sgd", "step", 0.004, 4e-6, 0.1, 1000, None, 0, (0.004, 0.004)),
    ("sgd", "step", 0.004, 4e-6, 0.1, 1000, [0.5, 0.75], 0, (0.004, 0.004)),
    ("sgd", "cos", 0.002, 2e-8, 0.02, 5000, None, 2, (0.002, 0.001)),
    ("sgd", "cos", 0.002, 2e-8, 0.02, 5000, None, 3, (0.002, 0.001)),
    ("adam", "cos", 0.001, 1e-8, 0.02, 5000, None, 0, (0.001, 0.003)),
    ("adamax", "step", 0.002, 2e-8, 0.02, 5000, None, 0, (0.002, 0.0007)),
]


def iterations(max_iter, warmup):
    wb = int(max_iter * warmup)
    return [0, 1, wb - 1, wb, wb + 1, max_iter // 2 + 1, max_iter]


def make_conf(conf, row):
    """Fill a dict-like conf (attribute access, ``in``) from one row of the fixture's columns."""
    solver, policy, lr, lr_target, warmup, max_iter, lr_steps, batch_skip = row
    conf.solver_type, conf.lr_policy = solver, policy
    conf.lr, conf.lr_target, conf.warmup, conf.max_iter = float(lr), float(lr_target), float(warmup), int(max_iter)
    conf.lr_steps = None if lr_steps is None else [float(s) for s in lr_steps]
    if batch_skip:
        conf.batch_skip = int(batch_skip)
    return conf


def main():
    gen_golden._install_stubs()
    from easydict import EasyDict
    import lib.core as ref_core
    assert ref_core.__file__.startswith(gen_golden.REF)

    n, k = len(ROWS), 7
    out = dict(solver=np.zeros(n, np.int64), policy=np.zeros(n, np.int64), lr=np.zeros(n), lr_target=np.zeros(n), warmup=np.zeros(n),
               max_iter=np.zeros(n, np.int64), lr_steps=np.full((n, 4), np.nan), batch_skip=np.zeros(n, np.int64),
               group_lrs=np.zeros((n, 2)), iters=np.zeros((n, k), np.int64), returned=np.zeros((n, k), np.int64),
               lr_out=np.full((n, k), np.nan), group_out=np.zeros((n, k, 2)))
    for i, row in enumerate(ROWS):
        solver, policy, lr, lr_target, warmup, max_iter, lr_steps, batch_skip, group_lrs = row
        out["solver"][i], out["policy"][i] = SOLVERS.index(solver), POLICIES.index(policy)
        out["lr"][i], out["lr_target"][i], out["warmup"][i], out["max_iter"][i] = lr, lr_target, warmup, max_iter
        out["batch_skip"][i], out["group_lrs"][i] = batch_skip, group_lrs
        if lr_steps is not None:
            out["lr_steps"][i, :len(lr_steps)] = lr_steps
        its = iterations(max_iter, warmup)
        assert len(its) == k and min(its) >= 0
        out["iters"][i] = its
        for j, it in enumerate(its):
            conf = make_conf(EasyDict(), row[:8])
            opt = types.SimpleNamespace(param_groups=[{"lr": float(v)} for v in group_lrs])
            got = ref_core.adjust_lr(conf, opt, it)
            out["group_out"][i, j] = [g["lr"] for g in opt.param_groups]
            if got is not None:
                out["returned"][i, j], out["lr_out"][i, j] = 1, np.float64(got)
    assert out["returned"].sum() < n * k and out["returned"][:6].all(), "the batch_skip rows must hold both outcomes"
    path = os.path.join(gen_golden.OUT, "adjust_lr.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): %d policies x %d iterations" % (path, os.path.getsize(path), n, k))


if __name__ == "__main__":
    main()
