"""The cases and the references of the fused BatchNorm + residual + activation training operator (``ops.bn_act_train``,
m3d_bn_act_train_forward / _backward): ``make_case(i)`` builds CPU float32 inputs, ``ref_grads`` is the torch composition
``nn.BatchNorm2d`` (training) -> ``+ residual`` -> ``leaky_relu`` (nothing at slope 1) with autograd behind it -- in float64 on the
CPU the yardstick, in float32 on the device the measure of what a float32 evaluation costs.

A sign flip of one pre-activation z between two float32 evaluations changes an element of dz by (1 - slope) * grad_y: a
discontinuity of the function, not an error.  So ``make_case`` moves its inputs until min |z64| >= Z_MIN in every case with
slope < 1: the offending elements of ``residual`` are pushed away from zero, or, without a residual, ``beta`` of the offending
channels is shifted, and the check is repeated (``passes`` counts the repetitions)."""
import collections
import functools

import torch
from torch import nn

# (B, C, H, W, residual, slope)
CASES = [(2, 1, 1, 1, False, 0.01),        # 0: N = 2, the minimum; N / (N - 1) = 2
         (1, 3, 3, 5, True, 0.01),         # 1: H*W = 15: one element per lane only; odd C
         (2, 16, 8, 20, True, 0.01),       # 2: 16-byte path; the level0 channel count
         (3, 5, 7, 9, True, 0.0),          # 3: H*W = 63: slabs start off 16-byte boundaries; ReLU
         (2, 64, 4, 6, False, 0.0),        # 4: many channels, tiny map
         (2, 2, 96, 130, True, 0.01),      # 5: several chunks per channel, the last one ragged
         (2, 8, 6, 10, False, 1.0),        # 6: no activation (Tree.project)
         (2, 4, 16, 24, True, 0.01),       # 7: x = 8 + N(0, 1): mean >> 0, cancellation in sum(x^2) / N - mean^2
         (4, 512, 1, 2, True, 0.01)]       # 8: C = 512, N = 8
IDS = ["%dx%dx%dx%d_%s_slope%g" % (b, c, h, w, "res" if r else "nores", s) for b, c, h, w, r, s in CASES]
SEED0 = 300
EPS, MOMENTUM = 1e-5, 0.1
Z_MIN = 2.0 ** -10
MAX_PASSES = 64
NAMES = ("y", "grad_x", "grad_residual", "grad_gamma", "grad_beta", "save_mean", "save_invstd", "running_mean", "running_var")

Case = collections.namedtuple("Case", "shape has_res slope x residual gamma beta running_mean running_var grad_y passes")


def pre_activation(x, residual, gamma, beta, dtype=torch.float64):
    """z = batch_norm(x) * gamma + beta (+ residual) evaluated in ``dtype`` by the composition's own layers."""
    x = x.to(dtype)
    z = torch.nn.functional.batch_norm(x, None, None, gamma.to(dtype), beta.to(dtype), True, MOMENTUM, EPS)
    return z if residual is None else z + residual.to(dtype)


@functools.lru_cache(maxsize=None)
def make_case(i):
    B, C, H, W, has_res, slope = CASES[i]
    g = torch.Generator().manual_seed(SEED0 + i)
    x = torch.randn(B, C, H, W, generator=g)
    if i == 7:
        x = x + 8.0
    residual = torch.randn(B, C, H, W, generator=g) if has_res else None
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)      # both signs
    beta = 0.3 * torch.randn(C, generator=g)
    running_mean = 0.5 * torch.randn(C, generator=g)
    running_var = 0.5 + torch.rand(C, generator=g)
    grad_y = torch.randn(B, C, H, W, generator=g)
    passes = 0
    if slope < 1.0:
        while True:
            z = pre_activation(x, residual, gamma, beta)
            near = z.abs() < Z_MIN
            if not near.any():
                break
            passes += 1
            assert passes <= MAX_PASSES, "case %d: |z| stays below 2^-10 somewhere" % i
            if has_res:
                # 4 * Z_MIN away from where z stood: |z| >= 3 * Z_MIN afterwards, whatever float32 rounding of the sum does
                step = torch.where(z >= 0, 4 * Z_MIN, -4 * Z_MIN).float()
                residual = torch.where(near, residual + step, residual)
            else:
                beta = beta + near.any(0).any(-1).any(-1).float() * (2 * Z_MIN * passes)
    return Case((B, C, H, W), has_res, slope, x, residual, gamma, beta, running_mean, running_var, grad_y, passes)


def composition(x, residual, bn, slope):
    """The layers host/train.py runs at a site without the fused operator."""
    z = bn(x)
    if residual is not None:
        z = z + residual
    return z if slope == 1.0 else torch.nn.functional.leaky_relu(z, slope)


def ref_grads(case, dtype, device):
    """The nine tensors of NAMES from the torch composition in ``dtype`` on ``device`` (grad_residual None without a residual)."""
    B, C, H, W = case.shape
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).to(device=device, dtype=dtype).train()
    with torch.no_grad():
        bn.weight.copy_(case.gamma)
        bn.bias.copy_(case.beta)
        bn.running_mean.copy_(case.running_mean)
        bn.running_var.copy_(case.running_var)
    x = case.x.to(device=device, dtype=dtype).clone().requires_grad_(True)             # (clone: the cached case stays as it is)
    residual = None if case.residual is None else case.residual.to(device=device, dtype=dtype).clone().requires_grad_(True)
    y = composition(x, residual, bn, case.slope)
    wanted = [x, bn.weight, bn.bias] + ([residual] if residual is not None else [])
    grads = torch.autograd.grad(y, wanted, case.grad_y.to(device=device, dtype=dtype))
    xd = x.detach()
    save_mean = xd.mean((0, 2, 3))
    save_invstd = 1.0 / torch.sqrt(xd.var((0, 2, 3), unbiased=False) + EPS)
    out = dict(y=y.detach(), grad_x=grads[0], grad_residual=grads[3] if residual is not None else None, grad_gamma=grads[1],
               grad_beta=grads[2], save_mean=save_mean, save_invstd=save_invstd, running_mean=bn.running_mean.detach().clone(),
               running_var=bn.running_var.detach().clone())
    assert int(bn.num_batches_tracked) == 1
    return out
