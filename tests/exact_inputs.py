"""Exact-arithmetic operands for the bf16 kernels, and plain float64 references of the operations they compute.

The tolerance tests of the bf16 path (tests/test_gpu_bf16.py) compare a kernel that rounds an intermediate value (the modulated
bilinear sample, a hidden activation) with its reference inside a noise bound, and a noise bound cannot see a structural mistake
that is smaller than the noise: a dropped corner, a tap read one pixel off, a K chunk skipped.  The generators here draw every
operand from a small dyadic lattice chosen so that EVERY value a kernel ever holds -- corner weight, sample, hidden activation,
folded weight, partial sum -- is exactly representable in the narrowest type on its path.  Then no step rounds, the accumulation
order does not matter, and the kernel has to return the float64 result bit for bit (`compare_exact`, torch.equal, no tolerance).
`assert_exact_under` is the condition that makes this legitimate: the float64 reference evaluated once as it is and once with
every intermediate rounded to the kernel's narrow types must agree exactly; tests/test_exact_inputs_host.py checks it for every
generator and shape that tests/test_gpu_exact.py uses.  No zeros among inputs and weights: a zero would hide a dropped term.

The references are written from the definition of the operation (DCNv2: the corner rules of dcn_v2_im2col_cuda.cu:129-178 as
oracle/dcn.py:dcn_v2_forward_numpy states them, vectorised); they do not call the product library.
"""
import math

import torch

F64 = torch.float64
BF16 = torch.bfloat16
F16 = torch.float16


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _pick(g, values, shape):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)]


def _rt(t, dtype):
    """Round trip through `dtype` (round to nearest even), back in float64."""
    return t.to(torch.float32).to(dtype).to(F64)


class Rounding:
    """Where a kernel keeps a narrow value.  `narrow`: the sample / hidden activation (bf16: 8 significant bits, fp16: 11); `corner`:
    the bilinear corner weights with the mask folded in (fp32 in dcn_corners, fp16 in the v_pk_fma_f16 combine of bf16_dcn_patch.hip,
    whose partial sums are fp16 as well); `weight`: the GEMM weights (bf16, or the fp16 copy); the accumulator is fp32, summed in
    a scrambled order in chunks of 64 (any order must give the same bits)."""

    def __init__(self, narrow=None, corner=None, weight=None, acc32=False, seed=0):
        self.narrow_t, self.corner_t, self.weight_t, self.acc32, self.seed = narrow, corner, weight, acc32, seed

    def narrow(self, t):
        return t if self.narrow_t is None else _rt(t, self.narrow_t)

    def corner(self, t):
        return t if self.corner_t is None else _rt(t, self.corner_t)

    def partial(self, t):
        """A partial sum of the corner combine: fp16 in the patch kernel (fma chain on fp16 pairs), fp32 elsewhere."""
        return _rt(t, self.corner_t) if self.corner_t == F16 else (t if self.corner_t is None else _rt(t, torch.float32))

    def weight(self, t):
        return t if self.weight_t is None else _rt(t, self.weight_t)

    def matmul(self, a, b):
        """a [M, K] @ b [K, N]: float64, or fp32 accumulation over K in chunks of 64 taken in a seeded scrambled order."""
        if not self.acc32:
            return a @ b
        K = a.shape[1]
        perm = torch.randperm(K, generator=_gen(self.seed + K))
        a32, b32 = a[:, perm].to(torch.float32), b[perm].to(torch.float32)
        acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
        for k0 in range(0, K, 64):
            acc = acc + a32[:, k0:k0 + 64] @ b32[k0:k0 + 64]
        return acc.to(F64)


EXACT = Rounding()


def assert_exact_under(ref_fn, operands, narrow_dtype, corner_dtype=torch.float32, weight_dtype=None):
    """The float64 reference as it is == the reference with every intermediate the kernel keeps narrow rounded to that type (and
    the accumulation done in fp32 in a scrambled order).  Returns the float64 result."""
    ref = ref_fn(operands, EXACT)
    low = ref_fn(operands, Rounding(narrow_dtype, corner_dtype, narrow_dtype if weight_dtype is None else weight_dtype, True, 1))
    ndiff = int((ref != low).sum())
    assert torch.equal(ref, low), "operands are not exact under %s: %d of %d results differ, max |diff| %g" % (
        narrow_dtype, ndiff, ref.numel(), float((ref - low).abs().max()))
    assert torch.equal(ref, ref.to(torch.float32).to(F64)), "the float64 result is not an fp32 number"
    return ref


def round_out(ref64, out_dtype):
    """The float64 reference cast to the kernel's output type (round to nearest even), widened to fp32 for the comparison."""
    return ref64.to(torch.float32).to(out_dtype).to(torch.float32)


def compare_exact(got, ref64, out_dtype=torch.float32, quantum=None):
    """torch.equal of `got` (fp32 tensor holding the kernel's output, widened if it was bf16) against the float64 reference cast to
    the output type.  Returns (number of differing elements, message); the message names the first differing index, the count and
    the difference in quanta of the input lattice."""
    want = round_out(ref64, out_dtype)
    got = got.to(torch.float32)
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return 0, ""
    bad = (got != want) | torch.isnan(got)
    idx = tuple(int(v) for v in torch.nonzero(bad)[0])
    d = float(got[idx]) - float(want[idx])
    q = "" if quantum is None else " = %g quanta of %g" % (d / quantum, quantum)
    return int(bad.sum()), "first difference at %s: got %r, want %r (difference %g%s); %d of %d elements differ" % (
        idx, float(got[idx]), float(want[idx]), d, q, int(bad.sum()), bad.numel())


# ------------------------------------------------------------------------------------ DCNv2
# Bit budget of the deformable kernels (csrc/bf16_conv.hip load_tile / store_tile, csrc/bf16_dcn1x1.hip, csrc/bf16_dcn_patch.hip):
#   offsets   quarter steps, |offset| <= 3 (or the stated radius): lh, lw in {0, 1/4, 1/2, 3/4}
#   corners   uh * uw etc. are multiples of 1/16 in [0, 1]                                   -> 5 bits; fp32 (dcn_corners) and fp16 exact
#   mask      {1/2, 1} folded into the corner weights: multiples of 1/32 in [0, 1]          -> 6 bits; fp32 and fp16 exact
#   inputs    {+-1, +-2, +-3} (bf16, and the fp16 window copy of the patch kernel: exact)
#   sample    sum of 4 (corner weight x input): a multiple of 1/32 with |s| <= 3, i.e. at most 96 quanta -> 8 significant bits:
#             exact in bf16 (8 bits) and in fp16 (11 bits); every partial sum of the fp16 fma chain is such a number too
#   weights   {+-1/2, +-1, +-2} (bf16 and the fp16 copy exact); product with a sample: a multiple of 1/64, |p| <= 6
#   acc       at most 9 x 512 products: |sum| <= 27 648 = 1.8 M quanta of 1/64 < 2^24 -> every fp32 partial sum exact in any order
#   epilogue  bias {+-1/2, +-1}; scales powers of two in [1/2, 2], shifts and residuals multiples of 1/2: still multiples of 1/128
#             below 2^17 -> fp32 exact; a bf16 output is ONE rounding of that exact number
DCN_QUANTUM = 1.0 / 64.0


def dcn_operands(seed, n, c, h, w, co, k, pad, dg=1, max_off=3.0):
    """x [n,c,h,w], off [n,dg*2*k*k,h,w], mask [n,dg*k*k,h,w], weight [co,c,k,k], bias [co]: float32, stride 1."""
    g = _gen(seed)
    ho, wo = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    q = int(round(max_off * 4))
    ops = dict(
        x=_pick(g, [-3, -2, -1, 1, 2, 3], (n, c, h, w)),
        off=torch.randint(-q, q + 1, (n, dg * 2 * k * k, ho, wo), generator=g).to(F64) / 4.0,
        mask=_pick(g, [0.5, 1.0], (n, dg * k * k, ho, wo)),
        weight=_pick(g, [-2, -1, -0.5, 0.5, 1, 2], (co, c, k, k)),
        bias=_pick(g, [-1, -0.5, 0.5, 1], (co,)),
    )
    ops = {kk: v.to(torch.float32) for kk, v in ops.items()}
    ops.update(stride=1, pad=pad, dg=dg)
    return ops


def dcn_epilogue_operands(seed, ops, ref64, act):
    """Power-of-two scales, dyadic shifts and a residual for the shared epilogue: out = act(ref * scale + shift + res).  With
    `act` the shift lifts every pre-activation to >= 0 (LeakyReLU is then the identity: its negative branch multiplies by 0.01,
    which no lattice survives, and stays with the tolerance tests)."""
    g = _gen(seed + 77)
    co = ref64.shape[1]
    scale = _pick(g, [0.5, 1.0, 2.0], (co,))
    res = _pick(g, [-3, -2, -1, 1, 2, 3], tuple(ref64.shape))
    shift = _pick(g, [-1.5, -0.5, 0.5, 1.5], (co,))
    if act:
        low = float((ref64 * scale.view(1, -1, 1, 1) + res).min())
        shift = shift + float(2 ** math.ceil(math.log2(max(2.0, 2.0 - low))))
    return scale.to(torch.float32), shift.to(torch.float32), res.to(torch.float32)


def apply_epilogue(ref64, scale=None, shift=None, res=None, act=0):
    y = ref64
    if scale is not None:
        y = y * scale.to(F64).view(1, -1, 1, 1) + shift.to(F64).view(1, -1, 1, 1)
    if res is not None:
        y = y + res.to(F64)
    if act:
        y = torch.where(y >= 0, y, y * 0.01)
    return y


def _all_pixels(n, ho, wo):
    nb, yy, xx = torch.meshgrid(torch.arange(n), torch.arange(ho), torch.arange(wo), indexing="ij")
    return nb.reshape(-1), yy.reshape(-1), xx.reshape(-1)


def dcn_corner_terms(ops, pix=None, rnd=EXACT, dil=1):
    """The sampling of DCNv2 at the output pixels `pix` = (image, row, column index vectors; default: all, image-major): for
    every pixel P, tap t and deformable group the four corner weights (mask folded in) cw [P, dg, KK, 4] and the four corner
    values cv [P, KK, 4, C] (0 where the corner lies outside the image or the whole sample does).  Rules of
    dcn_v2_im2col_cuda.cu:129-178: the sample counts only if h_im > -1, w_im > -1, h_im < H, w_im < W (strict); a corner counts only
    if its row and column are inside the image; weights (1-lh)(1-lw), (1-lh) lw, lh (1-lw), lh lw.  `dil`: the dilation of the tap
    grid (tap (i, j) sits at (i * dil, j * dil) before its offset is added)."""
    x, off, mask = ops["x"].to(F64), ops["off"].to(F64), ops["mask"].to(F64)
    n, c, h, w = x.shape
    kh, kw = ops["weight"].shape[2:]
    KK, dg, pad, stride = kh * kw, ops["dg"], ops["pad"], ops["stride"]
    ho, wo = off.shape[2:]
    nb, yy, xx = _all_pixels(n, ho, wo) if pix is None else pix
    P = nb.numel()
    o = off[nb, :, yy, xx].view(P, dg, KK, 2)
    m = mask[nb, :, yy, xx].view(P, dg, KK)
    ti = (torch.arange(KK) // kw).view(1, 1, KK).to(F64)
    tj = (torch.arange(KK) % kw).view(1, 1, KK).to(F64)
    h_im = (yy * stride - pad).view(P, 1, 1).to(F64) + ti * dil + o[..., 0]
    w_im = (xx * stride - pad).view(P, 1, 1).to(F64) + tj * dil + o[..., 1]
    inside = (h_im > -1) & (w_im > -1) & (h_im < h) & (w_im < w)
    hl, wl = torch.floor(h_im), torch.floor(w_im)
    lh, lw = h_im - hl, w_im - wl
    uh, uw = 1 - lh, 1 - lw
    hl, wl = hl.long(), wl.long()
    cw = torch.stack([uh * uw, uh * lw, lh * uw, lh * lw], -1)                        # [P, dg, KK, 4]
    rows = torch.stack([hl, hl, hl + 1, hl + 1], -1)
    cols = torch.stack([wl, wl + 1, wl, wl + 1], -1)
    ok = inside.unsqueeze(-1) & (rows >= 0) & (rows <= h - 1) & (cols >= 0) & (cols <= w - 1)
    cw = rnd.corner(torch.where(ok, cw, torch.zeros_like(cw)) * m.unsqueeze(-1))
    rows, cols = rows.clamp(0, h - 1), cols.clamp(0, w - 1)
    xn = x.permute(0, 2, 3, 1)                                                          # [n, h, w, c]
    cg = c // dg
    cv = torch.zeros(P, KK, 4, c, dtype=F64)
    for gi in range(dg):
        v = xn[nb.view(P, 1, 1), rows[:, gi], cols[:, gi]]                             # [P, KK, 4, c]
        cv[..., gi * cg:(gi + 1) * cg] = v[..., gi * cg:(gi + 1) * cg]
    cv = cv * ok.view(P, dg, 1, KK, 4, 1).expand(P, dg, cg, KK, 4, 1).permute(0, 3, 4, 1, 2, 5).reshape(P, KK, 4, c)
    return cw, cv


def dcn_columns(ops, cw, cv, rnd=EXACT):
    """Modulated bilinear samples col [P, KK, C] = sum over the four corners of weight x value, corner by corner in the order of the
    kernels (partial sums kept in the combine's type), then ONE rounding to the type that holds the sample."""
    P, KK, _, c = cv.shape
    dg = cw.shape[1]
    cwc = cw.view(P, dg, 1, KK, 4).expand(P, dg, c // dg, KK, 4).reshape(P, c, KK, 4).permute(0, 2, 3, 1)    # [P, KK, 4, c]
    acc = rnd.partial(cwc[:, :, 0] * cv[:, :, 0])
    for q in range(1, 4):
        acc = rnd.partial(acc + cwc[:, :, q] * cv[:, :, q])
    return rnd.narrow(acc)


def dcn_gemm(ops, col, rnd=EXACT):
    """out [P, Co] = bias + col [P, KK*C] @ weight[Co, (tap, channel)]^T."""
    wt = rnd.weight(ops["weight"].to(F64))
    co, c, kh, kw = wt.shape
    wmat = wt.permute(2, 3, 1, 0).reshape(kh * kw * c, co)
    return rnd.matmul(col.reshape(col.shape[0], -1), wmat) + ops["bias"].to(F64).view(1, co)


def dcn_ref(ops, rnd=EXACT):
    """DCNv2 forward, float64: [n, co, ho, wo]."""
    n = ops["x"].shape[0]
    ho, wo = ops["off"].shape[2:]
    cw, cv = dcn_corner_terms(ops, None, rnd)
    out = dcn_gemm(ops, dcn_columns(ops, cw, cv, rnd), rnd)
    return out.view(n, ho, wo, -1).permute(0, 3, 1, 2).contiguous()


def pack_om(ops, cs):
    """[off | mask] as the kernels read them: NHWC fp32 with pixel stride cs (padding channels zero)."""
    om = torch.cat([ops["off"], ops["mask"]], 1).permute(0, 2, 3, 1)
    n, h, w, k = om.shape
    out = torch.zeros(n, h, w, cs)
    out[..., :k] = om
    return out.contiguous()


def border_grid_offsets(h, w):
    """tests/test_gpu_bf16.py:_border_grid_offsets on the quarter-step lattice: output pixel (i, j) of a 1x1 deformable conv
    samples at (hs[i % 8], ws[j % 8]) = exactly -1 (out: the gate is strict), -1 + 1/4 (just inside), between rows, 0, the last row,
    past the last row (one corner row dropped), H - 1/4 (just below H), exactly H (out).  -0.999 -> -1, H - 0.001 -> H would merge
    two entries, so the nearest quarter step INSIDE the gate is taken; H - 0.5 is on the lattice already."""
    hs = [-1.0, -0.75, -0.5, 0.0, h - 1.0, h - 0.5, h - 0.25, float(h)]
    ws = [-1.0, -0.75, -0.5, 0.0, w - 1.0, w - 0.5, w - 0.25, float(w)]
    off = torch.zeros(1, 2, h, w)
    for i in range(h):
        for j in range(w):
            off[0, 0, i, j] = hs[i % 8] - i
            off[0, 1, i, j] = ws[j % 8] - j
    return off


# ---- perturbations of the reference: what a structurally wrong kernel would compute ----------------------------------------------
PERTURBATIONS = ("corner_dropped", "low_corners_swapped", "chunk_dropped", "channels_swapped", "tap_shifted")


def perturbed_pixel(ops, kind, seed):
    """One seeded placement of the structural error `kind` in the float64 reference.  Returns (pix, wrong [P, Co], right [P, Co]):
    the outputs at the affected output pixels with and without the error.  Placements avoid the cases where the error is no
    error (a corner whose weight is 0 or that lies outside the image, two equal weights, a tap outside the image before and after
    the shift): those change nothing in ANY implementation."""
    g = _gen(seed)
    n, c, h, w = ops["x"].shape
    co, _, kh, kw = ops["weight"].shape
    KK = kh * kw
    ho, wo = ops["off"].shape[2:]
    for _ in range(1000):
        b, y, x_ = (int(torch.randint(0, m, (1,), generator=g)) for m in (n, ho, wo))
        t = int(torch.randint(0, KK, (1,), generator=g))
        pix = (torch.tensor([b]), torch.tensor([y]), torch.tensor([x_]))
        cw, cv = dcn_corner_terms(ops, pix)
        right = dcn_gemm(ops, dcn_columns(ops, cw, cv))
        if kind == "corner_dropped":
            q = int(torch.randint(0, 4, (1,), generator=g))
            if cw[0, 0, t, q] == 0:
                continue
            cw2 = cw.clone()
            cw2[0, :, t, q] = 0
            return pix, dcn_gemm(ops, dcn_columns(ops, cw2, cv)), right
        if kind == "low_corners_swapped":
            if cw[0, 0, t, 0] == cw[0, 0, t, 1] or torch.equal(cv[0, t, 0], cv[0, t, 1]):
                continue
            cv2 = cv.clone()
            cv2[0, t, 0], cv2[0, t, 1] = cv[0, t, 1], cv[0, t, 0]
            return pix, dcn_gemm(ops, dcn_columns(ops, cw, cv2)), right
        if kind == "chunk_dropped":
            col = dcn_columns(ops, cw, cv)
            c0 = 8 * int(torch.randint(0, c // 8, (1,), generator=g))
            if not col[0, t, c0:c0 + 8].abs().sum() > 0:
                continue
            col[0, t, c0:c0 + 8] = 0
            return pix, dcn_gemm(ops, col), right
        if kind == "tap_shifted":
            ops2 = dict(ops)
            ops2["off"] = ops["off"].clone()
            ops2["off"][b, 2 * t + 1, y, x_] += 1.0
            cw2, cv2 = dcn_corner_terms(ops2, pix)
            if cw[0, 0, t].abs().sum() == 0 and cw2[0, 0, t].abs().sum() == 0:
                continue
            return pix, dcn_gemm(ops2, dcn_columns(ops2, cw2, cv2)), right
        if kind == "channels_swapped":              # two input channels of one tap swapped in the weights of ONE output channel: all pixels
            o = int(torch.randint(0, co, (1,), generator=g))
            c1, c2 = (int(v) for v in torch.randperm(c, generator=g)[:2])
            i, j = t // kw, t % kw
            if ops["weight"][o, c1, i, j] == ops["weight"][o, c2, i, j]:
                continue
            if "_all" not in ops:                   # the unperturbed columns of every pixel, computed once per operand set
                pix = _all_pixels(n, ho, wo)
                col = dcn_columns(ops, *dcn_corner_terms(ops, pix))
                ops["_all"] = (pix, col, dcn_gemm(ops, col))
            pix, col, right = ops["_all"]
            ops2 = dict(ops)
            ops2["weight"] = ops["weight"].clone()
            ops2["weight"][o, c1, i, j], ops2["weight"][o, c2, i, j] = ops["weight"][o, c2, i, j], ops["weight"][o, c1, i, j]
            return pix, dcn_gemm(ops2, col), right
        raise ValueError(kind)
    raise AssertionError("no placement found for " + kind)


def tolerance_test_operands(shape):
    """The random operands of the first case of tests/test_gpu_bf16.py::test_dcn_bf16_matches_oracle (same generator calls), for
    the count of perturbations its bound lets through."""
    n, c, h, w, co, k, pad = shape
    g = _gen(sum(shape))
    r = lambda t: t.to(BF16).float()                          # noqa: E731
    x = r(torch.randn(n, c, h, w, generator=g))
    wt = r(torch.randn(co, c, k, k, generator=g) / (c * k * k) ** 0.5)
    b = torch.randn(co, generator=g) * 0.1
    off = torch.randn(n, 2 * k * k, h, w, generator=g) * 3.0
    off[0, 0, 0, 0] = -1.0 + pad
    m = torch.rand(n, k * k, h, w, generator=g)
    return dict(x=x, off=off, mask=m, weight=wt, bias=b, stride=1, pad=pad, dg=1)


# ------------------------------------------------------------------------------------ fused multi-layer chains
# Bit budget of the fused 1x1 chains (csrc/bf16_head_mlp.hip keeps a hidden map as bf16: 8 significant bits; bf16_head_mlp2.hip and
# the cls tail keep it as fp16 and fold the scales into fp16 / bf16 weights: 11 bits -- ONE generator, sized for 8):
#   input     +-1 (bf16)
#   layer 1   dense, weight x scale = +-1/16 with the scale 1 or 2 per channel (the weight is +-1/16 or +-1/32: the kernels that
#             fold the scale into bf16 / fp16 weights and the one that applies it to the accumulator hold the same numbers): the
#             pre-activation is a sum of Cin terms +-1/16, a multiple of 1/8 (Cin is even); |pre| is a few units
#   affine    integer shift that lifts the map to >= 0 (LeakyReLU = identity) -- hidden values are multiples of 1/8 below 32: at most
#             255 quanta -> 8 bits
#   layer 2+  NNZ = 16 entries per output row with weight x scale = +-1, eight of each sign (the integer shifts of the layer
#             below cancel), seeded
#             positions, every input column used: a sum of 16 hidden values stays a multiple of 1/8 a few units wide, where a dense
#             +-2^-k row over 256 inputs would need ~13 bits
#   last      dense +-1/4, power-of-two scales, shifts multiples of 1/2: the fp32 result is a multiple of 1/32 far below 2^24 quanta
# The bound on each hidden map (0 <= h < 32 in steps of 1/8) is a property of the seeded draw; `mlp_ref` asserts it and
# assert_exact_under decides.
MLP_QUANTUM = 1.0 / 32.0
MLP_NNZ = 16


def _sparse_rows(g, rows, cols, nnz=MLP_NNZ):
    """[rows, cols] with nnz entries +-1 per row, half of each sign, and every column used by at least one row."""
    wt = torch.zeros(rows, cols, dtype=F64)
    sign = torch.tensor([1.0, -1.0], dtype=F64).repeat(nnz // 2)
    cover = torch.randperm(cols, generator=g)
    for r in range(rows):
        first = cover[(r * nnz) % cols:(r * nnz) % cols + nnz] if r * nnz < cols else cover[:0]
        rest = torch.randperm(cols, generator=g)
        rest = rest[~torch.isin(rest, first)][:nnz - first.numel()]
        pos = torch.cat([first, rest])
        wt[r, pos] = sign[torch.randperm(nnz, generator=g)]
    assert rows * nnz < cols or bool((wt != 0).any(0).all())
    return wt


def mlp_operands(seed, m, chans, scales3=(0.5, 1.0, 2.0), x=None):
    """A chain of 1x1 layers chans[0] -> chans[1] -> ... on m pixels: x [m, chans[0]], layers [(w [co, ci], scale [co], shift
    [co])]; every layer but the last is followed by LeakyReLU(0.01)."""
    g = _gen(seed)
    x = _pick(g, [-1.0, 1.0], (m, chans[0])) if x is None else x.to(F64)
    layers, hcur = [], x
    for li in range(len(chans) - 1):
        ci, co = chans[li], chans[li + 1]
        last = li == len(chans) - 2
        if last:
            wt, sc = _pick(g, [-0.25, 0.25], (co, ci)), _pick(g, list(scales3), (co,))
            sh = _pick(g, [-1.5, -0.5, 0.5, 1.5], (co,))
        else:
            sc = _pick(g, [1.0, 2.0], (co,))                              # folded weight = weight * scale: +-1/16, or +-1 in the sparse rows
            wt = (_pick(g, [-1.0 / 16, 1.0 / 16], (co, ci)) if li == 0 else _sparse_rows(g, co, ci)) / sc.view(-1, 1)
            pre = hcur @ (wt * sc.view(-1, 1)).T
            sh = torch.full((co,), float(math.ceil(-float(pre.min()))), dtype=F64)
            hcur = pre + sh
        layers.append((wt.to(torch.float32), sc.to(torch.float32), sh.to(torch.float32)))
    return dict(x=x.to(torch.float32), layers=layers)


def mlp_ref(ops, rnd=EXACT):
    """float64 chain: h = LeakyReLU(h @ w^T * scale + shift) for every layer but the last; asserts the hidden maps are >= 0."""
    hcur = ops["x"].to(F64)
    for li, (wt, sc, sh) in enumerate(ops["layers"]):
        last = li == len(ops["layers"]) - 1
        wf = rnd.weight(wt.to(F64) * sc.to(F64).view(-1, 1))               # the scale folded into the weight, as the kernels hold it
        hcur = rnd.matmul(hcur, wf.T.contiguous()) + sh.to(F64).view(1, -1)
        if not last:
            assert float(hcur.min()) >= 0 and float(hcur.max()) < 32, (li, float(hcur.min()), float(hcur.max()))
            hcur = rnd.narrow(torch.where(hcur >= 0, hcur, hcur * 0.01))
    return hcur


# ------------------------------------------------------------------------------------ attention
# m3d_anab_attend_*: S = q . k over the key channels, P = softmax over the keys, out = act((P V + res) * scale + shift).  The
# exponential sits on the data path, so the probabilities are made exact instead: a ONE-HOT softmax.  Key j carries the 9-bit
# pattern of j as +-1 in ATT_BITS seeded channels (unique per key; 337 points with bf16-exact coordinates whose dot products peak
# at the target do not fit in two channels -- a convex arrangement of that many points needs more than 8 significant bits -- so the
# code is spread over nine), a query aimed at key j carries the same pattern times ATT_GAIN, zeros elsewhere; the other key
# channels hold +-1 (they meet the zeros of the query).  The target logit is 9 * ATT_GAIN; any other key differs in at least one
# bit: at most 7 * ATT_GAIN.  The kernels take exp(S - max) of the logits as computed (no 1/sqrt(d) factor; csrc/bf16_anab.hip,
# csrc/anab_attend.hip), and exp(x) in fp32 is exactly 0 below x = -104 (2^-150 = e^-103.97 rounds to 0; v_exp_f32 flushes
# earlier): the gap 2 * ATT_GAIN = 128 makes P exactly one-hot, the row sum exactly 1 and every rescale of the running-maximum
# form exactly 0 or 1.  The padding keys [keys, keys_pad) carry TWICE the pattern of key (index - keys) and the value 7: a kernel
# that let one in would hand its value to every query aimed at that key.
ATT_GAIN = 64.0
ATT_BITS = 9


def attend_operands(seed, B, HW, keys, ck=168, ckp=192, cv=128, kp=None):
    g = _gen(seed)
    kp = (keys + 63) // 64 * 64 if kp is None else kp
    pos = torch.randperm(ck, generator=g)[:ATT_BITS]
    bits = ((torch.arange(kp).view(-1, 1) >> torch.arange(ATT_BITS).view(1, -1)) & 1).to(F64) * 2 - 1     # [kp, 9]
    target = torch.stack([torch.cat([torch.randperm(keys, generator=g), torch.randint(0, keys, (max(0, HW - keys),), generator=g)])[
        torch.randperm(max(HW, keys), generator=g)][:HW] for _ in range(B)])
    q = torch.zeros(B * HW, ckp, dtype=F64)
    q[:, pos] = bits[target.view(-1)] * ATT_GAIN
    khat = torch.zeros(B, kp, ckp, dtype=F64)
    khat[:, :keys, :ck] = _pick(g, [-1.0, 1.0], (B, keys, ck))
    khat[:, :keys, pos] = bits[:keys]
    khat[:, keys:, pos] = 2.0 * bits[:kp - keys]
    vhat = torch.zeros(B, cv, kp, dtype=F64)
    vhat[:, :, :keys] = _pick(g, [-3, -2, -1, 1, 2, 3], (B, cv, keys))
    vhat[:, :, keys:] = 7.0                                     # rows past `keys` must be ignored
    res = _pick(g, [-3, -2, -1, 1, 2, 3], (B * HW, cv))
    scale = _pick(g, [0.5, 1.0, 2.0], (cv,))
    shift = _pick(g, [0.5, 1.5], (cv,)) + 16.0                  # |P V + res| <= 6, scale <= 2: every pre-activation >= 4.5 > 0
    f = lambda t: t.to(torch.float32)                           # noqa: E731
    return dict(q=f(q), khat=f(khat), vhat=f(vhat), res=f(res), scale=f(scale), shift=f(shift), target=target, keys=keys, B=B, HW=HW)


def attend_ref(ops, rnd=EXACT):
    """float64 softmax attention over the first `keys` keys as defined (the exponential taken in fp32: its underflow is the point);
    with the one-hot logits the result is (V[target] + res) * scale + shift exactly."""
    B, HW, keys = ops["B"], ops["HW"], ops["keys"]
    q, khat, vhat = ops["q"].to(F64), ops["khat"].to(F64), ops["vhat"].to(F64)
    S = torch.einsum("bpc,bkc->bpk", q.view(B, HW, -1), khat)[:, :, :keys]
    P = torch.exp((S - S.max(-1, keepdim=True)[0]).to(torch.float32)).to(F64)
    P = rnd.narrow(P)
    P = P / P.sum(-1, keepdim=True)
    o = torch.einsum("bpk,bck->bpc", P, vhat[:, :, :keys]).reshape(B * HW, -1)
    y = (o + ops["res"].to(F64)) * ops["scale"].to(F64) + ops["shift"].to(F64)
    assert float(y.min()) >= 0
    return y


# ------------------------------------------------------------------------------------ tree entry
# m3d_tree_entry_bf16_forward (csrc/bf16_tree_entry.hip): t = LeakyReLU(conv3x3 stride 2 (x) * s1 + t1), res = conv1x1(maxpool2x2(x)) * sp
# + tp, both stored as bf16.  Nothing narrow is kept between the input and the fp32 accumulator (the halo tile and the pooled
# pixels are fp16 copies of bf16 inputs: exact; the accumulators start at the shifts), so the layers may be dense:
#   inputs    {+-1, +-2, +-3} (bf16 -> fp16 exact; a maximum of four of them is one of them)
#   weights   {+-1/2, +-1, +-2} times a scale in {1/2, 1, 2}, folded on the host into fp16: {+-1/4 .. +-4}, exact
#   acc       at most 9 x 256 products of magnitude <= 12, multiples of 1/4: below 2^17 quanta -> fp32 exact in any order
#   shifts    multiples of 1/2; shift1 lifts every pre-activation of t to >= 0 (LeakyReLU = identity)
#   outputs   ONE rounding of the exact fp32 number to bf16 (round to nearest even)
TREE_QUANTUM = 0.25


def tree_entry_operands(seed, n, cin, H, W):
    g = _gen(seed)
    co = 2 * cin
    x = _pick(g, [-3, -2, -1, 1, 2, 3], (n, cin, H, W))
    w1 = _pick(g, [-2, -1, -0.5, 0.5, 1, 2], (co, cin, 3, 3))
    wp = _pick(g, [-2, -1, -0.5, 0.5, 1, 2], (co, cin, 1, 1))
    s1, sp = _pick(g, [0.5, 1.0, 2.0], (co,)), _pick(g, [0.5, 1.0, 2.0], (co,))
    tp = _pick(g, [-1.5, -0.5, 0.5, 1.5], (co,))
    pre = torch.nn.functional.conv2d(x, w1, None, stride=2, padding=1) * s1.view(1, -1, 1, 1)
    t1 = _pick(g, [0.0, 0.5], (co,)) + torch.ceil(-pre.amin(dim=(0, 2, 3)))            # per channel: the smallest lift to >= 0
    return {k: v.to(torch.float32) for k, v in dict(x=x, w1=w1, wp=wp, s1=s1, sp=sp, t1=t1, tp=tp).items()}


def tree_entry_ref(ops, rnd=EXACT):
    """float64 (t, res, bottom) stacked as one tensor [n, 2 co + cin, H/2, W/2] for assert_exact_under; see tree_entry_split."""
    Fn = torch.nn.functional
    x = ops["x"].to(F64)
    n, cin, H, W = x.shape
    co = 2 * cin
    w1 = rnd.weight(ops["w1"].to(F64) * ops["s1"].to(F64).view(-1, 1, 1, 1)).reshape(co, -1)
    wp = rnd.weight(ops["wp"].to(F64) * ops["sp"].to(F64).view(-1, 1, 1, 1)).reshape(co, -1)
    pooled = Fn.max_pool2d(x, 2, 2)
    col = Fn.unfold(x, 3, padding=1, stride=2).permute(0, 2, 1).reshape(-1, cin * 9)
    t = rnd.matmul(col, w1.T.contiguous()) + ops["t1"].to(F64).view(1, -1)
    assert float(t.min()) >= 0
    r = rnd.matmul(pooled.permute(0, 2, 3, 1).reshape(-1, cin), wp.T.contiguous()) + ops["tp"].to(F64).view(1, -1)
    to_map = lambda v: v.view(n, H // 2, W // 2, -1).permute(0, 3, 1, 2)               # noqa: E731
    return torch.cat([to_map(t), to_map(r), pooled], 1).contiguous()


# ------------------------------------------------------------------------------------ fused front end
# m3d_frontend2_bf16_forward (csrc/bf16_frontend2.hip): stem 7x7 (3 -> 16) -> level0 3x3 (16 -> 16) -> level1 3x3 stride 2 (16 -> 32),
# each + shift + LeakyReLU, scales folded into fp16 weights, the image tile and both intermediates fp16 (11 significant bits), zero
# outside the image; the result is stored as bf16.
#   image     float input: {+-1, +-2}.  uint8 input: bytes {0, 255} -- byte / 255.0f is the one inexact step of that path and is
#             exact for these two -- with integer means (-1) and power-of-two stds (1, 2, 1): {1, 2} and {1/2, 1}; the border between
#             the frame and H x W is (0 - mean) / std, non-zero as well
#   stem      dense +-1/8, scale 1: a multiple of 1/16 a few units wide; ONE integer shift for all channels lifts it to >= 0
#             (the shift travels as an fp16 weight against a constant 1 in the image tile) -> h0 < 32 in steps of 1/16: 9 bits
#   level0    8 PAIRS (+1, -1) per output channel, both members of a pair on the same tap: the common shift of h0 cancels in
#             every pair, also at the image border where a tap falls on the zero padding; every (tap, channel) column is used.
#             A sum of 8 differences of h0 values: a multiple of 1/16 below 128 after its integer shift -> 11 bits (dense +-2^-k
#             rows over 144 inputs would need ~15)
#   level1    dense +-1/4, scales {1/2, 1, 2}, per-channel shifts (multiples of 1/2) that lift it to >= 0: multiples of 1/128 below
#             2^13 -> fp32 exact; the bf16 output is ONE rounding
# As for the 1x1 chains the bounds on h0 / h1 are properties of the seeded draw: frontend_ref asserts them, assert_exact_under decides.
FRONT_QUANTUM = 1.0 / 128.0
FRONT_MEAN, FRONT_STDS = (-1.0, -1.0, -1.0), (1.0, 2.0, 1.0)


def _paired_rows(g, rows, chans, pairs=8):
    """[rows, chans, 3, 3]: `pairs` (+1, -1) pairs per row, a pair inside one tap; every (tap, channel) entry used by some row."""
    wt = torch.zeros(rows, 9, chans, dtype=F64)
    cover = [(t, int(c)) for t in range(9) for c in torch.randperm(chans, generator=g)]            # consecutive entries share a tap
    cover = [(cover[i], cover[i + 1]) for i in range(0, len(cover), 2)]
    assert len(cover) <= rows * pairs
    todo = [[cover[k] for k in range(r, len(cover), rows)] for r in range(rows)]          # the covering pairs, dealt round the rows
    for r in range(rows):
        while len(todo[r]) < pairs:                                       # filled up with random pairs on free entries
            t = int(torch.randint(0, 9, (1,), generator=g))
            c1, c2 = (int(v) for v in torch.randperm(chans, generator=g)[:2])
            used = {(tt, c) for pr in todo[r] for (tt, c) in pr}
            if (t, c1) not in used and (t, c2) not in used:
                todo[r].append(((t, c1), (t, c2)))
        for (t, c1), (_, c2) in todo[r]:
            if int(torch.randint(0, 2, (1,), generator=g)):
                c1, c2 = c2, c1
            wt[r, t, c1], wt[r, t, c2] = 1.0, -1.0
    assert bool((wt != 0).any(0).all()) and bool(((wt != 0).sum((1, 2)) == 2 * pairs).all()) and bool((wt.sum(2) == 0).all())
    return wt.permute(0, 2, 1).reshape(rows, chans, 3, 3).contiguous()


def frontend_image(ops):
    """The network input [n, 3, H, W] float64: the float image, or the uint8 BGR frames zero-padded to H x W, / 255, - mean, / std
    (indexed by the BGR position), BGR -> RGB planes."""
    if ops["frames"] is None:
        return ops["img"].to(F64)
    fr = ops["frames"]
    n, fh, fw, _ = fr.shape
    x = torch.zeros(n, ops["H"], ops["W"], 3, dtype=F64)
    x[:, :fh, :fw] = fr.to(F64)
    x = (x / 255.0 - torch.tensor(FRONT_MEAN, dtype=F64)) / torch.tensor(FRONT_STDS, dtype=F64)
    return x.flip(-1).permute(0, 3, 1, 2).contiguous()


def frontend_operands(seed, n, H, W, u8):
    g = _gen(seed)
    Fn = torch.nn.functional
    ops = dict(H=H, W=W, frames=None, img=None)
    if u8:
        ops["frames"] = (torch.randint(0, 2, (n, H - 5, W - 9, 3), generator=g) * 255).to(torch.uint8)
    else:
        ops["img"] = _pick(g, [-2, -1, 1, 2], (n, 3, H, W)).to(torch.float32)
    x = frontend_image(ops)
    ws = _pick(g, [-0.125, 0.125], (16, 3, 7, 7))
    pre = Fn.conv2d(x, ws, None, padding=3)
    t0 = torch.full((16,), float(math.ceil(-float(pre.min()))), dtype=F64)
    h0 = pre + t0.view(1, -1, 1, 1)
    w0 = _paired_rows(g, 16, 16)
    pre = Fn.conv2d(h0, w0, None, padding=1)
    t1 = torch.full((16,), float(math.ceil(-float(pre.min()))), dtype=F64)
    h1 = pre + t1.view(1, -1, 1, 1)
    w1 = _pick(g, [-0.25, 0.25], (32, 16, 3, 3))
    s2 = _pick(g, [0.5, 1.0, 2.0], (32,))
    pre = Fn.conv2d(h1, w1, None, stride=2, padding=1) * s2.view(1, -1, 1, 1)
    t2 = _pick(g, [0.0, 0.5], (32,)) + torch.ceil(-pre.amin(dim=(0, 2, 3)))
    one = torch.ones(16, dtype=F64)
    f = lambda t: t.to(torch.float32)                                     # noqa: E731
    ops["layers"] = [(f(ws), f(one), f(t0), 1, 3), (f(w0), f(one), f(t1), 1, 1), (f(w1), f(s2), f(t2), 2, 1)]
    return ops


def frontend_ref(ops, rnd=EXACT):
    """float64 chain of three convolutions (+ shift, LeakyReLU), zero padding between them: [n, 32, H/2, W/2]."""
    Fn = torch.nn.functional
    h = rnd.narrow(frontend_image(ops))
    for li, (wt, sc, sh, stride, pad) in enumerate(ops["layers"]):
        co, ci, k, _ = wt.shape
        wf = rnd.weight(wt.to(F64) * sc.to(F64).view(-1, 1, 1, 1)).reshape(co, -1)
        n, _, hh, ww = h.shape
        ho, wo = (hh + 2 * pad - k) // stride + 1, (ww + 2 * pad - k) // stride + 1
        col = Fn.unfold(h, k, padding=pad, stride=stride).permute(0, 2, 1).reshape(-1, ci * k * k)
        y = rnd.matmul(col, wf.T.contiguous()) + (rnd.weight(sh.to(F64)) if li == 0 else sh.to(F64)).view(1, -1)
        assert float(y.min()) >= 0, (li, float(y.min()))
        h = y.view(n, ho, wo, co).permute(0, 3, 1, 2).contiguous()
        if li < 2:
            assert float(h.max()) < (32 if li == 0 else 128), (li, float(h.max()))
            h = rnd.narrow(h)
    return h
