"""Cases shared by tests/test_dcn_bf16_host.py (CPU) and tests/test_gpu_dcn_bf16.py: the exact-arithmetic backward cases of the bf16
DCNv2 operator and the float64 pieces both files recompute.

Operands come from exact_inputs.dcn_operands (inputs {+-1, +-2, +-3}, quarter-step offsets, masks {1/2, 1}, weights {+-1/2, +-1, +-2});
grad_output is drawn from {+-1, +-2}.  With Co <= 16, gcol[p][k][c] = sum_co go[p][co] * W[co][c][k] is a multiple of 1/2 of
magnitude at most 64: 8 significant bits, exact in bf16 and in fp32 alike, whichever storage the kernel picks; col = mask * val is
the forward's sample, a multiple of 1/32 of magnitude at most 3 (exact_inputs.py, bit budget of the deformable kernels).  Every
gradient is then a sum of exact products far below 2^24 quanta, so fp32 accumulation in any order returns the float64 number, and
the kernel has to return it rounded ONCE to the type it stores (tests/test_dcn_bf16_host.py asserts the premise per shape)."""
import torch

import dcn_grad_ref as R
import exact_inputs as X

# seed, n, c, h, w, co, k, pad, dg       (stride 1: dcn_operands; Co <= 16)
EXACT_BWD_CASES = [
    (11, 2, 32, 9, 11, 16, 3, 1, 1),       # the first forward shape
    (12, 2, 16, 7, 9, 16, 1, 0, 1),        # 1x1
    (13, 1, 24, 10, 12, 8, 3, 1, 3),       # three deformable groups of 8 channels, Co = 8
    (14, 1, 64, 8, 16, 16, 3, 1, 1),       # a full wave of channels, 128 pixels
    (15, 1, 72, 5, 7, 12, 3, 1, 1),        # C past one wave (padded to 128), 35 pixels, Co = 12
]

# n, c, h, w, co, k, pad, dg: the forward shapes
EXACT_FWD_CASES = [(2, 32, 9, 11, 16, 3, 1, 1), (1, 64, 8, 16, 128, 3, 1, 1), (2, 16, 7, 9, 16, 1, 0, 1), (1, 24, 10, 12, 8, 3, 1, 3)]


def exact_bwd_case(spec):
    """(ops dict of dcn_operands, grad_output float32 [n, co, ho, wo], ts, args) with ts / args in the form dcn_grad_ref takes."""
    seed, n, c, h, w, co, k, pad, dg = spec
    ops = X.dcn_operands(seed, n, c, h, w, co, k, pad, dg)
    g = torch.Generator().manual_seed(1000 + seed)
    ho, wo = ops["off"].shape[2:]
    go = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (n, co, ho, wo), generator=g)]
    ts = (ops["x"], ops["off"], ops["mask"], ops["weight"], ops["bias"])
    return ops, go, ts, (1, pad, 1, dg)


def col_gcol64(ops, go):
    """float64 col [P, KK, C] (the modulated samples) and gcol [P, KK, C] = sum_co go[p][co] * W[co][c][k]."""
    col = X.dcn_columns(ops, *X.dcn_corner_terms(ops))
    n, co = go.shape[:2]
    wt = ops["weight"].to(X.F64)
    kk = wt.shape[2] * wt.shape[3]
    gop = go.to(X.F64).permute(0, 2, 3, 1).reshape(-1, co)
    gcol = torch.einsum("po,ock->pkc", gop, wt.reshape(co, wt.shape[1], kk))
    return col, gcol


def ref_grads64(ts, go, args):
    return R.ref_grads(ts, go, args, dt=torch.float64)
