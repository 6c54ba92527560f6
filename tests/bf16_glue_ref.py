"""float64 references, case tables, bounds and input builders of the direct tests of the bf16 glue kernels
(csrc/bf16_kernels.hip: m3d_maxpool2x2_bf16, m3d_upsample2x_add_bf16, m3d_softmax_rows_bf16, m3d_f32_to_bf16, m3d_stem_conv7x7_bf16).
No GPU in here: tests/test_bf16_glue_host.py checks the references against torch in float64 and the conditions the tables rely on,
tests/test_gpu_bf16_glue.py runs the kernels.

The references are written from the definition of each operation (max over the 2 x 2 window; every input pixel scattered to a 4 x 4
patch of the output with stride 2 and padding 1; exp / sum; 147 products per output and channel), not through the torch operator the
host test compares them with.  bf16 values travel as uint16 bit patterns, so that a comparison is a comparison of bits.

Bounds (u = 2^-8: unit roundoff of bf16, round to nearest even; e = 2^-24: unit roundoff of fp32):
  upsample  |got - ref| <= u |ref| + 6 e S, S = sum |product| + |skip| at that element: at most five fp32 roundings of partial sums
            bounded by S (fused or not), 5 e S to first order and 6 e S with the second-order terms and the factor (1 + u) of the
            final rounding; then one rounding to bf16 of a number within 5 e S of ref.
  softmax   |got - ref| <= u ref + 1e-6: the fp32 row softmax is within 1e-6 (tests/test_gpu_rpn_glue.py: expf within 1 ulp on
            [0, 1], 8 additions per lane, a 6-level tree, one division, one product), then one rounding.
  stem      |got - ref| <= u |ref| + 151 e T, T = |scale| sum |x w| + |shift|: 147 fused multiply-adds, one multiply, one add, each
            one rounding of a partial result bounded by T; LeakyReLU is 1-Lipschitz (its own rounding on the negative branch is
            within the slack 151 - 149); then one rounding to bf16.
"""
import itertools

import numpy as np
import torch

U_BF16 = 2.0 ** -8
E_F32 = 2.0 ** -24
F64 = torch.float64


# ------------------------------------------------------------------------------------ bf16 as bits
def bf16_bits(a):
    """float array -> uint16 bit patterns of its bf16 rounding (round to nearest even, torch's CPU conversion)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def widen(bits):
    """uint16 bf16 bit patterns -> the float32 numbers they denote."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_bf16(a):
    """Round trip through bf16, back in float64."""
    return widen(bf16_bits(a)).astype(np.float64)


# ------------------------------------------------------------------------------------ 1. max-pool
# C, in_cs, first input channel, out_cs, first output channel
MAXPOOL_PARAMS = [(8, 8, 0, 8, 0), (32, 32, 0, 32, 0), (256, 256, 0, 256, 0), (16, 32, 8, 16, 0), (16, 16, 0, 24, 8), (64, 72, 8, 80, 0)]
MAXPOOL_MAPS = [(2, 8, 12), (1, 7, 12), (2, 8, 13), (3, 9, 11), (1, 2, 2), (1, 3, 3), (2, 24, 80)]
MAXPOOL_DEGENERATE = [(1, 1, 8), (1, 8, 1), (2, 1, 1)]           # H / 2 or W / 2 is 0: no output element
# grid caps: (workgroups, threads per workgroup, line of m3dssd_amd/csrc/bf16_kernels.hip that holds the workgroup count)
MAXPOOL_BF16_CAP = (16384, 256, 174)                             # hipLaunchKernelGGL(maxpool2x2_bf16_kernel, dim3(imin(cdiv(total, 256), 16384)), ...
MAXPOOL_BIG = (3, 512, 704, 128)                                 # N, H, W, C: one work item = 8 channels of one output pixel
UPSAMPLE_CAP = (16384, 256, 365)                                 # upsample2x_add_bf16_kernel<int>: dim3(imin(cdiv(total, 256), 16384))
# C, N, H, W; one work item = 8 channels of one OUTPUT pixel.  C = 16: 2 * 4 * 512 * 512 * 2 = 16384 * 256 items, EXACTLY the cap (every
# workgroup of the largest grid, one pass, no stride step); C = 24: 1.5 x the cap, the loop takes its stride step (and C / 8 = 3 is no
# power of two in the index divisions)
UPSAMPLE_BIG = [(16, 2, 512, 512), (24, 2, 512, 512)]
F32_TO_BF16_CAP = (8192, 256, 387)                               # f32_to_bf16_kernel: dim3(imin(cdiv(n / 8, 256), 8192)); 8 elements per thread
F32_TO_BF16_BIG = 8192 * 256 * 8 + 8


def maxpool_items(N, H, W, C):
    return N * (H // 2) * (W // 2) * (C // 8)


def upsample_items(C, N, H, W):
    return N * 2 * H * 2 * W * (C // 8)


def maxpool_ref(x):
    """x [N][H][W][C] (numpy) -> [N][H/2][W/2][C]: the maximum of each 2 x 2 window, odd H / W floored."""
    x = np.asarray(x, dtype=np.float64)
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    v = x[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C)
    return np.maximum(np.maximum(v[:, :, 0, :, 0], v[:, :, 0, :, 1]), np.maximum(v[:, :, 1, :, 0], v[:, :, 1, :, 1]))


def maxpool_input(seed, N, H, W, cs, negative):
    """bf16 bit patterns [N][H][W][cs] of randn (or of -|randn| - 0.5): no NaN and no zero of either sign (fmaxf leaves the sign
    of max(+0, -0) open)."""
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn(N, H, W, cs, generator=g)
    if negative:
        x = -x.abs() - 0.5
    bits = bf16_bits(x.numpy())
    assert ((bits & 0x7FFF) != 0).all()
    return bits


# ------------------------------------------------------------------------------------ 2. depthwise ConvTranspose2d(4, 2, 1) + skip
UPS_SEG_CHANNELS = (64, 128, 256)          # segment form by default, row form under M3D_UPSAMPLE_ROWS=2, grid-stride form under =0
UPS_OTHER_CHANNELS = (8, 16, 24, 512)      # grid-stride form whatever the knob says
UPS_KNOBS = ("0", "1", "2")


def ups_nseg(C):
    """Segments of an output row in the segment form: 256 threads / (C / 8) channel groups."""
    return 256 // (C // 8)


def ups_seg_len(C, W):
    """P = cdiv(W, nseg): input pixels per segment."""
    n = ups_nseg(C)
    return (W + n - 1) // n


def ups_ragged(C, W):
    """The last segment that has work is shorter than P."""
    return W % ups_seg_len(C, W) != 0


def ups_widths(C):
    n = ups_nseg(C)
    return (1, 2, n - 1, n, n + 1, 2 * n + 1, 40)


# C, N, H, W
UPS_SHAPES = [(C, N, H, W) for C in UPS_SEG_CHANNELS for W in ups_widths(C) for H in (1, 2, 5) for N in (1, 3)] + \
             [(C, N, H, W) for C in UPS_OTHER_CHANNELS for (N, H, W) in ((2, 5, 7), (1, 1, 1))]
UPS_KINDS = ("exact", "random")
# (has_skip, padded): padded = in_cs C + 8, skip_cs C + 16, out_cs C + 24 with sentinel pad channels, else all three = C
UPS_VARIANTS = [(True, False), (True, True), (False, False), (False, True)]
UPS_EXACT_QUANTUM = 0.125


def ups_strides(C, padded):
    """in_cs, skip_cs, out_cs"""
    return (C + 8, C + 16, C + 24) if padded else (C, C, C)


def ups_exact_operands(seed, C, N, H, W, device=None):
    """Exact-arithmetic operands (torch, float32): input and skip integers in {+-1, +-2, +-3}, weights k / 8 with 1 <= |k| <= 16.
    A product is a multiple of 1/8 of magnitude <= 6; any sum of up to four of them and the skip is a multiple of 1/8 of magnitude
    <= 27, i.e. at most 216 quanta: 8 significant bits, exact in fp32 AND in bf16, in any order, fused or not.  No zero anywhere: a
    zero would hide a dropped term."""
    g = torch.Generator(device="cpu" if device is None else device).manual_seed(int(seed))
    kw = dict(generator=g, device=device)

    def ints(shape, m):
        v = torch.randint(0, 2 * m, shape, **kw) - m            # -m .. m - 1
        return (v + (v >= 0).to(v.dtype)).to(torch.float32)     # -m .. -1, 1 .. m
    return ints((N, H, W, C), 3), ints((4, 4, C), 16) * UPS_EXACT_QUANTUM, ints((N, 2 * H, 2 * W, C), 3)


def ups_random_operands(seed, C, N, H, W):
    """randn input and skip (rounded to bf16), rand weights (fp32)."""
    g = torch.Generator().manual_seed(int(seed))
    r = lambda t: t.to(torch.bfloat16).to(torch.float32)        # noqa: E731
    return r(torch.randn(N, H, W, C, generator=g)), torch.rand(4, 4, C, generator=g), r(torch.randn(N, 2 * H, 2 * W, C, generator=g))


def ups_operands(kind, index, C, N, H, W):
    """The operands of case `index` of UPS_SHAPES (x [N][H][W][C], w [4][4][C], skip [N][2H][2W][C]; float32, x and skip bf16 numbers)."""
    return (ups_exact_operands if kind == "exact" else ups_random_operands)(1000 + 2 * index + (kind == "random"), C, N, H, W)


def upsample_terms(x, w, skip):
    """The (up to) five terms of every output element, [5][N][2H][2W][C] in the dtype of x: input pixel (iy, ix) times w[ky][kx] lands on
    output (2 iy - 1 + ky, 2 ix - 1 + kx); an output row y therefore takes rows iy = (y + 1 - ky) / 2 for the two ky of its parity,
    likewise for columns; term 2 * a + b is the product of the a-th such row and the b-th such column (0 where it lies outside the
    input), term 4 the skip (0 if None)."""
    N, H, W, C = x.shape
    dev = x.device
    out = torch.zeros((5, N, 2 * H, 2 * W, C), dtype=x.dtype, device=dev)
    y, xx = torch.arange(2 * H, device=dev), torch.arange(2 * W, device=dev)
    for a in range(2):
        ky = (y + 1) % 2 + 2 * a                                 # the two taps whose parity matches y + 1
        iy = (y + 1 - ky) // 2
        oky = (iy >= 0) & (iy < H)
        for b in range(2):
            kx = (xx + 1) % 2 + 2 * b
            ix = (xx + 1 - kx) // 2
            okx = (ix >= 0) & (ix < W)
            v = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
            wt = w[ky][:, kx].to(x.dtype)
            out[2 * a + b] = v * wt * (oky[:, None] & okx[None, :])[None, :, :, None].to(x.dtype)
    if skip is not None:
        out[4] = skip
    return out


def upsample_ref(x, w, skip):
    """float64 (ref, S): the sum of the terms and the sum of their magnitudes."""
    t = upsample_terms(x.to(F64), w.to(F64), None if skip is None else skip.to(F64))
    return t.sum(0), t.abs().sum(0)


def upsample_bound(ref, S):
    return U_BF16 * ref.abs() + 6 * E_F32 * S


PERMS5 = list(itertools.permutations(range(5)))


def sum_in_every_order_f32(terms):
    """terms [5][...] -> [120][...]: the fp32 sum of the five terms, one rounding per addition, in each of the 120 orders."""
    t = terms.to(torch.float32)
    return torch.stack([(((t[p[0]] + t[p[1]]) + t[p[2]]) + t[p[3]]) + t[p[4]] for p in PERMS5])


# ------------------------------------------------------------------------------------ 3. row softmax
# cs, valid, out_cs
SOFTMAX_CASES = [(384, 337, 384), (352, 337, 352), (1000, 337, 384), (64, 1, 8), (64, 63, 64), (64, 64, 64), (128, 65, 72), (512, 512, 512),
                 (512, 511, 512), (600, 500, 512)]
SOFTMAX_ROWS = (1, 3, 4, 5)
SOFTMAX_BIG = ((384, 337, 384), 7681)
SOFTMAX_SCALES = (1.0, 3.0, 10.0)


def softmax_ref(x, valid):
    """float64 softmax over the first `valid` columns of each row."""
    x = np.asarray(x, dtype=np.float64)[:, :valid]
    m = x.max(axis=1, keepdims=True)
    ex = np.exp(x - m)
    return ex / ex.sum(axis=1, keepdims=True)


def softmax_bound(ref):
    return U_BF16 * ref + 1e-6


def softmax_logits(seed, rows, cs, scale):
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randn(rows, cs, generator=g) * scale).numpy()


# ------------------------------------------------------------------------------------ 4. fp32 -> bf16
CONVERT_EXPONENTS = (1, 2, 63, 126, 127, 128, 129, 200, 253, 254)       # biased; 254 with an all-ones mantissa rounds up to inf
CONVERT_UPPER_MANTISSAS = (0x00, 0x01, 0x2A, 0x55, 0x7E, 0x7F)          # the 7 mantissa bits bf16 keeps: even and odd last bit, carries
CONVERT_LOW_HALVES = (0x8000, 0x7FFF, 0x8001, 0x0000)                   # tie, just below, just above, exact


def convert_tie_table():
    """[(fp32 bit pattern, parity of the upper half)] of every tie of the table: low half exactly 0x8000."""
    out = []
    for sign in (0, 1):
        for ex in CONVERT_EXPONENTS:
            for m in CONVERT_UPPER_MANTISSAS:
                upper = (sign << 15) | (ex << 7) | m
                out.append(((upper << 16) | 0x8000, upper & 1))
    return out


def convert_patterns():
    """uint32 bit patterns of normal numbers: ties (even and odd upper half), the neighbours of a tie, exact values; n % 8 == 0."""
    pats = []
    for sign in (0, 1):
        for ex in CONVERT_EXPONENTS:
            for m in CONVERT_UPPER_MANTISSAS:
                upper = (sign << 15) | (ex << 7) | m
                pats += [(upper << 16) | low for low in CONVERT_LOW_HALVES]
    assert len(pats) % 8 == 0
    return np.array(pats, dtype=np.uint32)


# +-0, +-inf, +-FLT_MAX (rounds to +-inf), the largest fp32 that stays finite (0x7F7F7FFF -> 0x7F7F) and its successor (a tie, odd: inf)
CONVERT_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0xFF7F7FFF,
                             0x7F7F8000, 0xFF7F8000, 0x7F7F0000, 0xFF7F0000, 0x3F800000, 0xBF800000, 0x00800000, 0x80800000], dtype=np.uint32)
# fp32 subnormals: smallest, just below / at / above the first tie (bf16 0x0000 | 0x0001), an odd tie, exact bf16 subnormals, the largest
# (rounds up to the smallest normal, 0x0080)
_SUB = [0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00010000, 0x00018000, 0x00400000, 0x007FFFFF]
CONVERT_SUBNORMALS = np.array(_SUB + [0x80000000 | v for v in _SUB], dtype=np.uint32)
# NaN: quiet, signalling with only low payload bits (a conversion that merely adds 0x7FFF + lsb turns 0x7F800001 into +inf), all ones, negative
CONVERT_NANS = np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0x7F808000, 0x7F80FFFF, 0xFF800001, 0x7FA00000], dtype=np.uint32)


# ------------------------------------------------------------------------------------ 5. stem
# N, H, W, out_cs (fp32 image)
STEM_F32_CASES = [(1, 1, 1, 16), (3, 7, 31, 16), (2, 8, 32, 24), (1, 9, 33, 40), (2, 17, 65, 16), (1, 24, 96, 16)]
# N, H, W, img_h, img_w (uint8 BGR frames)
STEM_U8_CASES = [(2, 16, 64, 16, 64), (2, 16, 64, 12, 50), (1, 24, 96, 9, 33), (3, 17, 65, 1, 1), (1, 24, 96, 23, 95)]
STEM_U8_FILLS = ("random", "zeros", "full")          # the two constant frames run at STEM_U8_CONSTANT_CASE
STEM_U8_CONSTANT_CASE = (2, 16, 64, 12, 50)
STEM_MEAN = np.array([0.406, 0.456, 0.485], dtype=np.float32)      # indexed by the BGR position, like the frame
STEM_STDS = np.array([0.225, 0.224, 0.229], dtype=np.float32)
STEM_TILE = (8, 32)                                                 # STEM_TH, STEM_TW of bf16_kernels.hip
LEAKY_SLOPE = 0.01


def stem_params(seed):
    """wgt [16][3][7][7], scale [16], shift [16] (float32 numpy)."""
    g = torch.Generator().manual_seed(int(seed))
    w = torch.randn(16, 3, 7, 7, generator=g) / 12
    return w.numpy(), (torch.rand(16, generator=g) + 0.5).numpy(), (torch.randn(16, generator=g) * 0.1).numpy()


def stem_pack_weight(w):
    """[16][3][7][7] -> the kernel's [7 * 7 * 3][16]."""
    return np.ascontiguousarray(np.transpose(w, (2, 3, 1, 0))).reshape(147, 16)


def stem_frames(seed, N, img_h, img_w, fill):
    if fill == "zeros":
        return np.zeros((N, img_h, img_w, 3), np.uint8)
    if fill == "full":
        return np.full((N, img_h, img_w, 3), 255, np.uint8)
    return np.random.default_rng(seed).integers(0, 256, size=(N, img_h, img_w, 3), dtype=np.uint8)


def stem_normalise_u8(frames, H, W, mean=STEM_MEAN, stds=STEM_STDS):
    """uint8 BGR frames [N][img_h][img_w][3] -> the fp32 image [N][3][H][W] the kernel convolves, in ITS order of operations and in
    float32 (each step one correctly rounded operation on both sides): x / 255, - mean, / std with mean / std indexed by the BGR
    position; (0 - mean) / std where the H x W crop extends past the frame; plane c = BGR channel 2 - c."""
    N, ih, iw, _ = frames.shape
    img = np.empty((N, H, W, 3), np.float32)
    img[:] = (np.float32(0) - mean) / stds
    x = frames.astype(np.float32) / np.float32(255.0)
    x = x - mean
    x = x / stds
    img[:, :ih, :iw] = x
    assert img.dtype == np.float32
    return np.ascontiguousarray(np.transpose(img[..., ::-1], (0, 3, 1, 2)))


def stem_ref(img, w, scale, shift):
    """float64 (ref, T) [N][H][W][16]: 7 x 7 convolution (pad 3) of the fp32 image [N][3][H][W], scale and shift per channel,
    LeakyReLU(0.01); T = |scale| sum |x w| + |shift|."""
    img, w = np.asarray(img, dtype=np.float64), np.asarray(w, dtype=np.float64)
    N, _, H, W = img.shape
    xp = np.zeros((N, 3, H + 6, W + 6))
    xp[:, :, 3:3 + H, 3:3 + W] = img
    acc, mag = np.zeros((N, H, W, 16)), np.zeros((N, H, W, 16))
    for i in range(7):
        for j in range(7):
            for c in range(3):
                p = xp[:, c, i:i + H, j:j + W, None] * w[None, None, None, :, c, i, j]
                acc += p
                mag += np.abs(p)
    sc, sh = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    pre = acc * sc + sh
    return np.where(pre >= 0, pre, pre * LEAKY_SLOPE), np.abs(sc) * mag + np.abs(sh)


def stem_bound(ref, T):
    return U_BF16 * np.abs(ref) + 151 * E_F32 * T
