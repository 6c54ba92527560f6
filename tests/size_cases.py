"""The image sizes of tests/test_sizes_host.py (CPU) and tests/test_gpu_sizes.py (GPU): one table, chosen from the thresholds of
the routes of Engine._conv (Engine._route_wino44 / _route_wino / _route_wave, the library's igemm split-K) and of Engine._anab_ops /
Engine._anab_pool / EngineBF16._anab_bf16 so that every plan branch the two benched sizes (128x320, 384x1280) never take is taken
by one of them, and with frames chosen on the CPU so that the oracle has no (or few) near-ties.

A "near-tie pixel" of the free-running oracle: its top-1 minus top-2 foreground probability is below NEAR_TIE, or its top-1
probability lies within NEAR_TIE of the hard-mask threshold 0.5.  NEAR_TIE is twice the 1e-4 within which
gpu_common._check_decisions lets the engine take another decision, so an engine that passes _check_decisions can differ from the
oracle at such pixels only; where a case has none, engine and oracle must decide alike everywhere and every row is compared."""
import collections
import functools

import torch
import torch.nn.functional as F

NEAR_TIE = 2e-4
CLEAN_RADIUS = 4          # gpu_common._clean_rows: rows this many pixels around a differing decision are set aside

SizeCase = collections.namedtuple("SizeCase", "crop B seed near_ties steers")

SIZE_CASES = [
    # feature map 12x28 (HW = 336, no multiple of 32), level 5 is 3x7
    SizeCase((96, 224), 2, 4, 0, "unfused ANAB through igemm, generic pooling, odd level-4/5 maps"),
    # 12x32 (HW = 384), level 5 is 3x8
    SizeCase((96, 256), 2, 2, 0, "fused attend behind the generic pooling, odd height only"),
    # 20x52 (HW = 1040), level 5 is 5x13; the hard mask is on at 56 % of the pixels
    SizeCase((160, 416), 1, 9, 0, "unfused ANAB at B = 1 on a mid-sized map"),
    # 8x16 (HW = 128), level 5 is 2x4: the smallest map the bf16 engine accepts
    SizeCase((64, 128), 2, 2, 0, "fused attend with exactly one 128-row block"),
    # 4x8, level 5 is 1x2: the smallest legal input; 36 * 32 = 1152 anchors < nms_topN_pre
    SizeCase((32, 64), 2, 1, 0, "1x2 level-5 map, pooling size 16 on a 4-row map, fewer anchors than nms_topN_pre"),
    # 32x32, level 5 is 8x8
    SizeCase((256, 256), 1, 5, None, "nested pooling + fused attend away from the benched sizes, square"),
    # 20x24 (HW = 480): B * HW / 32 * 3 = 900 waves
    SizeCase((160, 192), 20, 1, None, "ANAB GEMMs on the wave kernel, a batch of 20"),
]
# near_ties: the number the oracle must show (0: every row is compared, no mask); None: a few occur, the rows CLEAN_RADIUS away
# from them must be at least CLEAN_MIN of all rows
CLEAN_MIN = 0.9


def case_id(c):
    return "%dx%d_b%d" % (c.crop[0], c.crop[1], c.B)


def by_crop(crop):
    return next(c for c in SIZE_CASES if c.crop == tuple(crop))


def near_tie_mask(fg):
    """fg: the oracle's fg_prob [B, A, fh, fw] -> bool [B, 1, fh, fw]."""
    top2 = fg.topk(2, dim=1)[0]
    return ((top2[:, 0:1] - top2[:, 1:2]) < NEAR_TIE) | ((top2[:, 0:1] - 0.5).abs() < NEAR_TIE)


def clean_fraction(mask, radius=CLEAN_RADIUS):
    """Share of the pixels (= of the rows: A rows per pixel) at least `radius` pixels away from every pixel of `mask`."""
    bad = mask.float()
    if bad.any():
        bad = F.max_pool2d(bad, 2 * radius + 1, stride=1, padding=radius)
    return (bad == 0).float().mean().item()


@functools.lru_cache(maxsize=None)
def oracle_fg(crop, B, seed):
    """fg_prob of the free-running CPU oracle on synth_frames(B, crop, seed) with the weights synth_state_dict(0)."""
    from m3dssd_amd import synth
    from oracle import model_cpu
    taps = {}
    with torch.no_grad():
        out = model_cpu.rpn_forward(synth.synth_state_dict(0), synth.synth_conf(crop, 0, batch_size=B, device="cpu"),
                                    synth.synth_frames(B, crop, seed), taps)
    assert all(torch.isfinite(t).all() for t in out)
    return taps["fg_prob"]
