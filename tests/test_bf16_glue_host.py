"""Host checks (no GPU) of tests/bf16_glue_ref.py: every float64 reference against the torch operator in float64, and the conditions
the case tables of tests/test_gpu_bf16_glue.py rely on (exactness of the exact-arithmetic operands, the tie patterns, the segment
lengths of the up-sampling table, the grid caps)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_glue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "m3dssd_amd", "csrc", "bf16_kernels.hip")


# ------------------------------------------------------------------------------------ references against torch, float64
@pytest.mark.parametrize("N,H,W,C", [(2, 8, 12, 8), (1, 7, 13, 16), (3, 9, 11, 8), (1, 2, 2, 8), (1, 3, 3, 8)])
def test_maxpool_ref_matches_torch(N, H, W, C):
    x = np.random.default_rng(H * W).standard_normal((N, H, W, C))
    want = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(R.maxpool_ref(x), want)
    neg = -np.abs(x) - 0.5
    assert np.array_equal(R.maxpool_ref(neg), F.max_pool2d(torch.from_numpy(neg).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("C,N,H,W", [(8, 2, 5, 7), (16, 1, 1, 1), (24, 3, 2, 9), (64, 1, 1, 33), (8, 2, 6, 1)])
def test_upsample_ref_matches_conv_transpose2d(C, N, H, W):
    g = torch.Generator().manual_seed(C + W)
    x = torch.randn(N, H, W, C, generator=g, dtype=R.F64)
    w = torch.rand(4, 4, C, generator=g, dtype=R.F64)
    skip = torch.randn(N, 2 * H, 2 * W, C, generator=g, dtype=R.F64)
    up = F.conv_transpose2d(x.permute(0, 3, 1, 2), w.permute(2, 0, 1).unsqueeze(1), None, stride=2, padding=1, groups=C).permute(0, 2, 3, 1)
    ref, S = R.upsample_ref(x, w, skip)
    assert float((ref - (up + skip)).abs().max()) <= 1e-12
    ref0, S0 = R.upsample_ref(x, w, None)
    assert float((ref0 - up).abs().max()) <= 1e-12
    assert bool((S >= ref.abs() - 1e-12).all()) and float((S - S0 - skip.abs()).abs().max()) <= 1e-12
    # S is the conv-transpose of the magnitudes
    up_abs = F.conv_transpose2d(x.abs().permute(0, 3, 1, 2), w.abs().permute(2, 0, 1).unsqueeze(1), None, stride=2, padding=1,
                                groups=C).permute(0, 2, 3, 1)
    assert float((S0 - up_abs).abs().max()) <= 1e-12


@pytest.mark.parametrize("rows,cs,valid", [(5, 384, 337), (3, 64, 1), (4, 512, 512), (1, 600, 500)])
def test_softmax_ref_matches_torch(rows, cs, valid):
    for scale in R.SOFTMAX_SCALES:
        x = R.softmax_logits(rows + cs, rows, cs, scale)
        want = torch.softmax(torch.from_numpy(x[:, :valid]).double(), -1).numpy()
        assert np.abs(R.softmax_ref(x, valid) - want).max() <= 1e-12


@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 7, 31), (1, 9, 33)])
def test_stem_ref_matches_conv2d(N, H, W):
    w, sc, sh = R.stem_params(H)
    img = np.random.default_rng(W).standard_normal((N, 3, H, W)).astype(np.float32)
    pre = F.conv2d(torch.from_numpy(img).double(), torch.from_numpy(w).double(), None, padding=3) * torch.from_numpy(sc).double().view(1, -1, 1, 1) \
        + torch.from_numpy(sh).double().view(1, -1, 1, 1)
    want = F.leaky_relu(pre, R.LEAKY_SLOPE).permute(0, 2, 3, 1).numpy()
    ref, T = R.stem_ref(img, w, sc, sh)
    assert np.abs(ref - want).max() <= 1e-12
    mag = F.conv2d(torch.from_numpy(np.abs(img)).double(), torch.from_numpy(np.abs(w)).double(), None, padding=3).permute(0, 2, 3, 1).numpy()
    assert np.abs(T - (np.abs(sc.astype(np.float64)) * mag + np.abs(sh.astype(np.float64)))).max() <= 1e-12
    assert (T >= np.abs(ref) - 1e-12).all()
    # the kernel's weight layout: row (i * 7 + j) * 3 + c, column = output channel
    p = R.stem_pack_weight(w)
    assert p.shape == (147, 16) and p[(2 * 7 + 5) * 3 + 1, 9] == w[9, 1, 2, 5]


def test_stem_normalise_u8_matches_the_float64_formula_and_the_layout():
    N, H, W, ih, iw = 2, 9, 11, 6, 7
    fr = R.stem_frames(3, N, ih, iw, "random")
    got = R.stem_normalise_u8(fr, H, W)
    assert got.dtype == np.float32 and got.shape == (N, 3, H, W)
    full = np.zeros((N, H, W, 3))
    full[:, :ih, :iw] = fr
    want = ((full / 255.0 - R.STEM_MEAN.astype(np.float64)) / R.STEM_STDS.astype(np.float64))[..., ::-1].transpose(0, 3, 1, 2)
    assert np.abs(got - want).max() <= 4 * R.E_F32 * np.abs(want).max()
    # plane 0 is BGR channel 2; the border holds (0 - mean) / std of that channel
    assert got[0, 0, H - 1, W - 1] == (np.float32(0) - R.STEM_MEAN[2]) / R.STEM_STDS[2]
    assert got[1, 2, 0, 0] == (np.float32(fr[1, 0, 0, 0]) / np.float32(255) - R.STEM_MEAN[0]) / R.STEM_STDS[0]
    for fill, byte in (("zeros", 0), ("full", 255)):
        assert (R.stem_frames(0, N, ih, iw, fill) == byte).all()


def test_stem_case_tables_reach_the_tile_edges_they_name():
    th, tw = R.STEM_TILE
    src = open(KERNELS).read()
    assert "#define STEM_TH %d\n" % th in src and "#define STEM_TW %d\n" % tw in src
    shapes = [(H, W) for _, H, W, _ in R.STEM_F32_CASES]
    assert any(H % th and W % tw for H, W in shapes) and any(H % th == 0 and W % tw == 0 for H, W in shapes)     # ragged and exact tiles
    assert any(H >= 3 * th and W >= 3 * tw for H, W in shapes)                                                   # an interior tile
    assert any(N > 2 for N, _, _, _ in R.STEM_F32_CASES) and any(cs > 16 for _, _, _, cs in R.STEM_F32_CASES)
    # the frame edge inside the patch (tile + 3-pixel halo) of the interior tile [th, 2 th) x [tw, 2 tw), in both directions: that
    # patch holds frame pixels and border pixels, and none of the image's zero padding
    assert any(H >= 3 * th and W >= 3 * tw and th - 3 < ih < 2 * th + 3 and tw - 3 < iw < 2 * tw + 3 for _, H, W, ih, iw in R.STEM_U8_CASES)
    assert any((H, W) == (ih, iw) for _, H, W, ih, iw in R.STEM_U8_CASES)                                        # frame equal to the crop
    assert all(ih <= H and iw <= W for _, H, W, ih, iw in R.STEM_U8_CASES)
    assert R.STEM_U8_CONSTANT_CASE in R.STEM_U8_CASES


# ------------------------------------------------------------------------------------ exact-arithmetic up-sampling operands
def test_upsample_exact_operands_are_exact_in_every_order():
    """For every case of the table: the fp32 sum of the five terms in all 120 orders equals the float64 sum, and that sum survives a
    round trip through bf16 -- so every form of the kernel has to return it bit for bit.  (With exact partial sums a fused
    multiply-add rounds nothing either.)"""
    for index, (C, N, H, W) in enumerate(R.UPS_SHAPES):
        x, w, skip = R.ups_operands("exact", index, C, N, H, W)
        assert bool((x != 0).all()) and bool((w != 0).all()) and bool((skip != 0).all())
        assert bool(((w / R.UPS_EXACT_QUANTUM) == (w / R.UPS_EXACT_QUANTUM).round()).all()) and float(w.abs().max()) <= 2.0
        assert torch.equal(x, x.round()) and torch.equal(skip, skip.round())
        for s in (skip, None):
            terms = R.upsample_terms(x.to(R.F64), w.to(R.F64), None if s is None else s.to(R.F64))
            ref = terms.sum(0)
            assert torch.equal(terms.to(torch.float32).to(R.F64), terms)                      # every product is an fp32 number
            sums = R.sum_in_every_order_f32(terms)
            assert bool((sums.to(R.F64) == ref.unsqueeze(0)).all()), (C, N, H, W)
            assert np.array_equal(R.round_bf16(ref.numpy()), ref.numpy()), (C, N, H, W)
            assert float(ref.abs().max()) <= 27.0


def test_upsample_big_case_operands_are_exact_too():
    """The operands of the two large grid-stride cases come from the same generator on the device: same lattice (checked here on a
    small shape drawn the same way).  C = 16 at 2 x 512 x 512 fills the capped grid exactly, C = 24 exceeds it."""
    groups, threads, _ = R.UPSAMPLE_CAP
    items = [R.upsample_items(*case) for case in R.UPSAMPLE_BIG]
    assert items[0] == groups * threads and items[1] > groups * threads        # the whole largest grid in one pass; beyond one pass
    for (C, N, H, W), n in zip(R.UPSAMPLE_BIG, items):
        assert n < 2 ** 31 - groups * threads                                  # the int instantiation (the long long one is left out)
        assert C not in R.UPS_SEG_CHANNELS
        x, w, skip = R.ups_exact_operands(5, C, 1, 3, 4)
        terms = R.upsample_terms(x.to(R.F64), w.to(R.F64), skip.to(R.F64))
        assert bool((R.sum_in_every_order_f32(terms).to(R.F64) == terms.sum(0).unsqueeze(0)).all())


def test_upsample_random_operands_are_bf16_numbers():
    x, w, skip = R.ups_operands("random", 3, 64, 1, 2, 33)
    assert np.array_equal(R.round_bf16(x.numpy()), x.numpy().astype(np.float64)) and np.array_equal(R.round_bf16(skip.numpy()), skip.numpy())
    assert w.dtype == torch.float32 and float(w.min()) >= 0 and float(w.max()) < 1


def test_upsample_table_reaches_every_segment_length():
    assert len(R.UPS_SHAPES) == 3 * 7 * 3 * 2 + 4 * 2
    for C in R.UPS_SEG_CHANNELS:
        nseg = R.ups_nseg(C)
        assert nseg == 256 // (C // 8) and R.ups_widths(C) == (1, 2, nseg - 1, nseg, nseg + 1, 2 * nseg + 1, 40)
        report = {W: (R.ups_seg_len(C, W), R.ups_ragged(C, W)) for (c, _, _, W) in R.UPS_SHAPES if c == C}
        print("C = %d, nseg = %d: W -> (P, ragged) %s" % (C, nseg, report))
        P = [p for p, _ in report.values()]
        assert 1 in P and 2 in P and max(P) >= 3, (C, report)
        assert any(r for _, r in report.values()), (C, report)
        for W, (p, ragged) in report.items():                                  # P and raggedness from first principles
            assert (p - 1) * nseg < W <= p * nseg
            used = -(-W // p)
            assert ragged == (W - (used - 1) * p < p)
        assert {(N, H) for (c, N, H, _) in R.UPS_SHAPES if c == C} == {(N, H) for N in (1, 3) for H in (1, 2, 5)}
    for C in R.UPS_OTHER_CHANNELS:
        assert C % 8 == 0 and C not in R.UPS_SEG_CHANNELS
        assert {(N, H, W) for (c, N, H, W) in R.UPS_SHAPES if c == C} == {(2, 5, 7), (1, 1, 1)}
    assert R.UPS_VARIANTS == [(s, p) for s in (True, False) for p in (False, True)]
    assert R.ups_strides(64, True) == (72, 80, 88) and R.ups_strides(64, False) == (64, 64, 64)


# ------------------------------------------------------------------------------------ conversion table
def test_conversion_tie_patterns_are_ties():
    ties = R.convert_tie_table()
    assert len(ties) == 2 * len(R.CONVERT_EXPONENTS) * len(R.CONVERT_UPPER_MANTISSAS)
    pats = set(int(v) for v in R.convert_patterns())
    parities = set()
    for bits, parity in ties:
        assert bits & 0xFFFF == 0x8000 and ((bits >> 16) & 1) == parity and bits in pats
        ex = (bits >> 23) & 0xFF
        assert 0 < ex < 255                                                   # a normal number
        parities.add(parity)
        # round to nearest even: an even upper half stays, an odd one moves up (possibly into the next binade, or to inf)
        want = (bits >> 16) + parity
        assert int(R.bf16_bits(np.array([bits], np.uint32).view(np.float32))[0]) == want
        for low in (0x7FFF, 0x8001, 0x0000):
            assert (bits & 0xFFFF0000) | low in pats
    assert parities == {0, 1}
    v = R.convert_patterns().view(np.float32)
    assert np.isfinite(v).all() and len(v) % 8 == 0
    assert not np.isfinite(R.widen(R.bf16_bits(v))).all()                     # some of them round up to inf


def test_conversion_special_values_are_what_they_are_named():
    s = R.CONVERT_SPECIALS.view(np.float32)
    assert len(s) % 8 == 0 and s[4] == np.finfo(np.float32).max and s[5] == -np.finfo(np.float32).max
    got = R.bf16_bits(s)
    assert list(got[:4]) == [0x0000, 0x8000, 0x7F80, 0xFF80]
    assert list(got[4:10]) == [0x7F80, 0xFF80, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80]
    sub = R.CONVERT_SUBNORMALS
    assert len(sub) % 8 == 0 and (((sub >> 23) & 0xFF) == 0).all() and ((sub & 0x7FFFFFFF) != 0).all()
    assert list(R.bf16_bits(sub.view(np.float32))[:8]) == [0x0000, 0x0000, 0x0000, 0x0001, 0x0001, 0x0002, 0x0040, 0x0080]
    nan = R.CONVERT_NANS
    assert len(nan) % 8 == 0 and np.isnan(nan.view(np.float32)).all() and len(set((nan & 0x007FFFFF).tolist())) >= 5
    assert np.isnan(R.widen(R.bf16_bits(nan.view(np.float32)))).all()


# ------------------------------------------------------------------------------------ softmax known values
def test_softmax_constant_row_value_does_not_depend_on_the_path_of_the_rounding():
    """bf16(1 / valid): the kernel forms 1.0f / s in fp32 and rounds that; rounding the float64 quotient once gives the same bits for
    every `valid` of the table (no fp32 quotient sits on a bf16 tie)."""
    for _, valid, _ in R.SOFTMAX_CASES:
        f32 = np.float32(1) / np.float32(valid)
        twice = int(R.bf16_bits(np.array([f32]))[0])                         # float64 -> fp32 -> bf16
        dist = {c: abs(float(R.widen(np.array([c], np.uint16))[0]) - 1.0 / valid) for c in (twice - 1, twice, twice + 1)}
        assert min(dist, key=dist.get) == twice and sorted(dist.values())[0] < sorted(dist.values())[1], (valid, dist)
    assert all(valid <= cs and valid <= out_cs <= 512 and out_cs % 2 == 0 for cs, valid, out_cs in R.SOFTMAX_CASES)
    assert R.SOFTMAX_BIG[0] in R.SOFTMAX_CASES


# ------------------------------------------------------------------------------------ grid caps
def test_grid_cap_cases_exceed_the_caps_named_in_the_source():
    lines = open(KERNELS).read().split("\n")
    for (groups, threads, line), kernel in ((R.MAXPOOL_BF16_CAP, "maxpool2x2_bf16_kernel"), (R.UPSAMPLE_CAP, "upsample2x_add_bf16_kernel<int>"),
                                            (R.F32_TO_BF16_CAP, "f32_to_bf16_kernel")):
        text = lines[line - 1]
        assert kernel in text and re.search(r"imin\(cdiv\([^)]*, %d\), %d\)" % (threads, groups), text), (kernel, line, text)
    assert R.maxpool_items(*R.MAXPOOL_BIG) > R.MAXPOOL_BF16_CAP[0] * R.MAXPOOL_BF16_CAP[1]
    assert R.F32_TO_BF16_BIG // 8 > R.F32_TO_BF16_CAP[0] * R.F32_TO_BF16_CAP[1] and R.F32_TO_BF16_BIG % 8 == 0
    assert R.F32_TO_BF16_BIG == 8192 * 256 * 8 + 8
    for N, H, W in R.MAXPOOL_DEGENERATE:
        assert R.maxpool_items(N, H, W, 8) == 0
    for C, in_cs, c_in0, out_cs, c_out0 in R.MAXPOOL_PARAMS:
        assert C % 8 == 0 and c_in0 + C <= in_cs and c_out0 + C <= out_cs and c_in0 % 8 == 0 and c_out0 % 8 == 0
