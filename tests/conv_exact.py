"""Exact-arithmetic operands for the fp32 convolution kernels, and the float64 reference of the contract they share.

Five fp32 kernel families take one descriptor (m3d_conv_desc, include/m3dssd_hip.h): the implicit GEMM, the wave-granular kernel,
Winograd F(2x2,3x3), Winograd F(4x4,3x3) and the level0 pair.  tests/exact_inputs.py holds the bf16 path to its contract with
operands on which no step of a kernel rounds; this module does the same for fp32.  `conv_contract_ref` computes a descriptor's
result in float64 from the definition (it imports nothing of the product but the weight packers, which only the Winograd
emulation and the device buffers use), tests/test_conv_exact_host.py proves on the CPU that every case is exact in fp32 in any
summation order and that a structural error moves the result, tests/test_gpu_conv_exact.py launches every case and compares with
torch.equal.  The case lists (CASES) are shared by the two.

Bit budgets (fp32: 24 significant bits; every partial sum must stay below 2^24 quanta of its lattice):
  direct sums (igemm, wave, level0 direct kernel)
    inputs    {+-1, +-2, +-3}, weights {+-1/2, +-1, +-2}: products are multiples of 1/2, |p| <= 6
    acc       at most 9 x 512 products: |sum| <= 27 648 = 55 296 quanta of 1/2 < 2^24 -> exact in any order
    DCNv2     offsets in quarter steps, mask {1/2, 1} as in exact_inputs.dcn_operands: a sample is a multiple of 1/32 with
              |s| <= 3, a product a multiple of 1/64; 9 x 512 of them: 1.8 M quanta < 2^24
  F(2x2,3x3)  the same lattice
    U = G g G^T is a multiple of 1/8 with |U| <= 4.5; V = B^T d B is an integer with |V| <= 12
    sum       over Cin = 512: at most 512 x 4.5 x 12 = 27 648 = 221 184 quanta of 1/8
    A^T . A   at most 9 of them: 2.0 M quanta < 2^24 -> exact in any order and grouping
  F(4x4,3x3)  G holds sixths and twenty-fourths: the weights are multiples of 9, 9 / 576 = 1 / 64 is dyadic
    lattice A inputs {+-1, +-2, +-3}, weights 9 x {+-1/2, +-1, +-2}: U is a multiple of 1/128; the order-independent bound
              max sum_c |U| |V| x 128 < 2^24 holds up to Cin = 64 (used where Cin <= 64)
    lattice B inputs {+-1}, weights {+-9}: U is a multiple of 1/64; the bound holds up to Cin = 512 (used above 64)
    the bound is asserted per case on the case's own operands (winograd_emulation); pack_wino44 computes U in float64 from a G
    whose sixths are not float64 numbers, so the host check transforms with the product's packer, not with a rational U
  epilogue    scales {1/2, 1, 2}, shifts {+-1/2, +-3/2}, residuals {+-1, +-2, +-3}: the pre-activation is a multiple of 1/256
              far below 2^24 quanta
  activation  the pre-activation is cast to fp32 (no rounding: it is an fp32 number) and LeakyReLU is where(y >= 0, y, y * 0.01f)
              with ONE fp32 multiply, which is what every epilogue computes (fmaxf(v, v * slope)): both branches are
              bit-comparable, the shift need not lift anything
  sigmoid     channels at or past sigmoid_from go through expf: compared at the project's bound for them, not exactly
No zeros among inputs and weights: a zero would hide a dropped term.
"""
import zlib

import torch

import exact_inputs as E

F64, F32 = torch.float64, torch.float32
SENT_IN = 4099.0          # pad lanes of the input and residual views: off every lattice, a kernel that reads one shows it
SENT_OUT = -777.0         # every output word before the launch
SLOPE32 = torch.tensor(0.01, dtype=F32)
X3, W3 = [-3, -2, -1, 1, 2, 3], [-2, -1, -0.5, 0.5, 1, 2]


def case(name, family, n=2, cin=32, h=9, w=11, cout=64, cout_pad=None, k=1, stride=1, pad=None, dil=1, deform=0, per_image=0,
         res_mode=None, scale=1, shift=1, act=1, sig=-1, in_x=4, out_x=4, res_x=8, planar=0, entry=None, forms=(), expect=None):
    """One descriptor.  h, w: the INPUT map; res_mode None: no residual; in_x / out_x / res_x: pad lanes of the three views
    (pixel stride = channels + pad); entry / forms: which launches the GPU test makes; expect: what the library's queries
    must answer for this descriptor (the PLAN pin)."""
    pad = dil * (k // 2) if pad is None else pad
    ho = (h + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    wo = (w + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    lattice = "direct"
    if family in ("w44", "l0"):
        lattice = "w44a" if cin <= 64 else "w44b"
    if cout_pad is None:
        unit = {"igemm": 32, "wave": 32 if cout <= 32 else (64 if cout <= 64 else 128), "w22": 32, "w44": 64, "l0": 16}[family]
        cout_pad = -(-cout // unit) * unit
    return dict(name=name, family=family, n=n, cin=cin, h=h, w=w, cout=cout, cout_pad=cout_pad, k=k, stride=stride, pad=pad,
                dil=dil, deform=deform, per_image=per_image, res_mode=res_mode, scale=scale, shift=shift, act=act, sig=sig,
                in_x=in_x, out_x=out_x, res_x=res_x, planar=planar, entry=entry, forms=tuple(forms), expect=expect, ho=ho, wo=wo,
                lattice=lattice, seed=zlib.crc32(name.encode()) & 0xFFFF)


def operands(c):
    """x [n, cin, h, w], weight [n or 1, cout, cin, k, k], off / mask (deformable), scale / shift [cout], res [n, cout, ho, wo]:
    float32 on the case's lattice; an operand the case does not use is None."""
    g = E._gen(c["seed"])
    n, ci, co, k, ho, wo = c["n"], c["cin"], c["cout"], c["k"], c["ho"], c["wo"]
    xs = [-1, 1] if c["lattice"] == "w44b" else X3
    ws = {"direct": W3, "w44a": [9 * v for v in W3], "w44b": [-9, 9]}[c["lattice"]]
    ops = dict(x=E._pick(g, xs, (n, ci, c["h"], c["w"])), weight=E._pick(g, ws, (n if c["per_image"] else 1, co, ci, k, k)),
               off=None, mask=None, scale=None, shift=None, res=None)
    if c["deform"]:
        ops["off"] = torch.randint(-12, 13, (n, 2 * k * k, ho, wo), generator=g).to(F64) / 4.0
        ops["mask"] = E._pick(g, [0.5, 1.0], (n, k * k, ho, wo))
    if c["scale"]:
        ops["scale"] = E._pick(g, [0.5, 1.0, 2.0], (co,))
    if c["shift"]:
        ops["shift"] = E._pick(g, [-1.5, -0.5, 0.5, 1.5], (co,))
    if c["res_mode"] is not None:
        ops["res"] = E._pick(g, X3, (n, co, ho, wo))
    return {kk: (None if v is None else v.to(F32)) for kk, v in ops.items()}


def pixels(c):
    """(image, row, column) of every output pixel, image-major: the row order of the NHWC output."""
    return E._all_pixels(c["n"], c["ho"], c["wo"])


def columns(c, ops, pix=None, rnd=E.EXACT, tap_dx=None, dil=None):
    """The A operand col [P, k*k, cin] (float64) at the output pixels `pix` (default: all): tap (i, j) of pixel (y, x) reads the
    input at (y * stride - pad + i * dil, x * stride - pad + j * dil), zero outside the map; deformable: the modulated bilinear
    sample of DCNv2 at that position plus the tap's offset.  tap_dx [P, k*k]: extra column shift per pixel and tap, and `dil`
    other than the case's: the structural errors of the sensitivity table."""
    nb, yy, xx = pixels(c) if pix is None else pix
    k, stride, pad = c["k"], c["stride"], c["pad"]
    dil = c["dil"] if dil is None else dil
    P, KK = nb.numel(), k * k
    if c["deform"]:
        off = ops["off"]
        if tap_dx is not None:
            off = off.clone()
            for t in range(KK):
                off[nb, 2 * t + 1, yy, xx] += tap_dx[:, t].to(off.dtype)
        dops = dict(x=ops["x"], off=off, mask=ops["mask"], weight=ops["weight"][0], stride=stride, pad=pad, dg=1)
        cw, cv = E.dcn_corner_terms(dops, (nb, yy, xx), rnd, dil=dil)
        return E.dcn_columns(dops, cw, cv, rnd)
    t = torch.arange(KK)
    iy = (yy * stride - pad).view(P, 1) + (t // k).view(1, KK) * dil
    ix = (xx * stride - pad).view(P, 1) + (t % k).view(1, KK) * dil
    if tap_dx is not None:
        ix = ix + tap_dx.long()
    ok = (iy >= 0) & (iy < c["h"]) & (ix >= 0) & (ix < c["w"])
    xn = ops["x"].to(F64).permute(0, 2, 3, 1)
    return xn[nb.view(P, 1), iy.clamp(0, c["h"] - 1), ix.clamp(0, c["w"] - 1)] * ok.unsqueeze(-1)


def gemm(c, col, nb, weight, rnd=E.EXACT):
    """acc [P, cout] = col [P, (tap, channel)] @ weight^T, with the weight set of each pixel's image where they are per image."""
    nw, co, ci, k, _ = weight.shape
    wm = weight.to(F64).permute(0, 3, 4, 2, 1).reshape(nw, k * k * ci, co)
    a = col.reshape(col.shape[0], -1)
    if nw == 1:
        return rnd.matmul(a, wm[0])
    out = torch.zeros(a.shape[0], co, dtype=F64)
    for i in range(nw):
        sel = nb == i
        if bool(sel.any()):
            out[sel] = rnd.matmul(a[sel], wm[i])
    return out


def res_rows(c, ops):
    return None if ops["res"] is None else ops["res"].to(F64).permute(0, 2, 3, 1).reshape(-1, c["cout"])


def epilogue(c, ops, acc, res, wrong=None):
    """The contract's epilogue on acc [P, cout] (float64): res_mode 0: acc * scale + shift + res, res_mode 1: (acc + res) * scale +
    shift, each of the three optional; cast to fp32; LeakyReLU with one fp32 multiply; sigmoid channels from the float64
    pre-activation.  Returns (pre float64, out float32).  wrong: one of the epilogue errors of the sensitivity table."""
    one, zero = torch.ones(c["cout"], dtype=F64), torch.zeros(c["cout"], dtype=F64)
    sc = one if ops["scale"] is None else ops["scale"].to(F64)
    sh = zero if ops["shift"] is None else ops["shift"].to(F64)
    r = torch.zeros_like(acc) if res is None else res
    mode = c["res_mode"] or 0
    if wrong == "res_mode_exchanged":
        mode = 1 - mode
    if wrong == "scale_after_residual":
        pre = (acc + sh + r) * sc
    elif mode == 1:
        pre = (acc + r) * sc + sh
    else:
        pre = acc * sc + sh + r
    y = pre.to(F32)
    if c["act"] == 1:
        y = torch.where(y >= 0, y, y * (SLOPE32 * 0 if wrong == "slope_zero" else SLOPE32))
    if c["sig"] >= 0:
        y = torch.cat([y[:, :c["sig"]], torch.sigmoid(pre[:, c["sig"]:]).to(F32)], 1)
    return pre, y


def conv_contract_ref(c, ops=None, rnd=E.EXACT):
    """The float64 result of the descriptor `c` from the definition.  Returns dict(ops, col, acc [M, cout] float64, pre [M, cout]
    float64 (before the activation), out [M, cout] float32 (what the kernel must store), pix); M = n * ho * wo, image-major."""
    ops = operands(c) if ops is None else ops
    pix = pixels(c)
    col = columns(c, ops, pix, rnd)
    acc = gemm(c, col, pix[0], ops["weight"], rnd)
    pre, out = epilogue(c, ops, acc, res_rows(c, ops))
    return dict(ops=ops, col=col, acc=acc, pre=pre, out=out, pix=pix)


def assert_exact_fp32(c, ref):
    """The premise of the torch.equal comparison for a direct-sum case: the reference evaluated with fp32 accumulation in a
    scrambled chunk order gives the same bits, and accumulator and pre-activation are fp32 numbers."""
    low = conv_contract_ref(c, ref["ops"], E.Rounding(corner=F32, acc32=True, seed=c["seed"]))
    assert torch.equal(ref["acc"], low["acc"]), "%s: not exact in fp32: %d of %d sums differ" % (
        c["name"], int((ref["acc"] != low["acc"]).sum()), ref["acc"].numel())
    for key in ("acc", "pre"):
        assert torch.equal(ref[key], ref[key].to(F32).to(F64)), "%s: %s is not an fp32 number" % (c["name"], key)
    assert torch.equal(ref["out"], low["out"])


# ---- structural errors: what a subtly wrong kernel would compute -----------------------------------------------------------------
ERRORS = ("tap_dropped", "tap_one_column_off_first", "tap_one_column_off_last", "k_stage_dropped", "channels_swapped",
          "res_mode_exchanged", "scale_after_residual", "slope_zero", "dilation_ignored")


def strip_edge_pixels(c, last):
    """Indices of the output pixels in the first column of the first tile (last = False) or the last column of the last tile (True)
    of every 16-tile strip; tiles of 4 x 4 pixels numbered along image rows, then rows, then images, as the F(4x4) kernels do."""
    nb, yy, xx = pixels(c)
    th, tw = -(-c["ho"] // 4), -(-c["wo"] // 4)
    tile = (nb * th + yy // 4) * tw + xx // 4
    if last:
        sel = ((tile % 16 == 15) | (tile == c["n"] * th * tw - 1)) & ((xx % 4 == 3) | (xx == c["wo"] - 1))
    else:
        sel = (tile % 16 == 0) & (xx % 4 == 0)
    return torch.nonzero(sel).view(-1)


def applies(c, ops, kind):
    """Whether the error is an error at all for this case (exchanging res_mode without a residual changes no implementation)."""
    if kind == "res_mode_exchanged":
        return ops["res"] is not None and ops["scale"] is not None
    if kind == "scale_after_residual":
        return ops["scale"] is not None and (ops["shift"] is not None or (ops["res"] is not None and (c["res_mode"] or 0) == 0))
    if kind == "slope_zero":
        return c["act"] == 1
    if kind == "dilation_ignored":
        return c["dil"] > 1
    return True


def with_error(c, ref, kind):
    """The output [M, cout] float32 of the reference with ONE structural error of `kind`, seeded by the case."""
    ops, col, acc, (nb, yy, xx) = ref["ops"], ref["col"], ref["acc"], ref["pix"]
    g = E._gen(c["seed"] + 13)
    KK = c["k"] * c["k"]
    t = int(torch.randint(0, KK, (1,), generator=g))
    res = res_rows(c, ops)
    if kind in ("res_mode_exchanged", "scale_after_residual", "slope_zero"):
        return epilogue(c, ops, acc, res, kind)[1]
    if kind == "tap_dropped":
        col2 = col.clone()
        col2[:, t] = 0
        return epilogue(c, ops, gemm(c, col2, nb, ops["weight"]), res)[1]
    if kind == "k_stage_dropped":
        c0 = 16 * int(torch.randint(0, c["cin"] // 16, (1,), generator=g))
        col2 = col.clone()
        col2[:, :, c0:c0 + 16] = 0
        return epilogue(c, ops, gemm(c, col2, nb, ops["weight"]), res)[1]
    if kind == "channels_swapped":
        wt = ops["weight"].clone()
        for _ in range(1000):
            o = int(torch.randint(0, c["sig"] if c["sig"] >= 0 else c["cout"], (1,), generator=g))     # an exactly compared channel
            c1, c2 = (int(v) for v in torch.randperm(c["cin"], generator=g)[:2])
            i, j = t // c["k"], t % c["k"]
            if not torch.equal(wt[:, o, c1, i, j], wt[:, o, c2, i, j]):
                break
        wt[:, o, c1, i, j], wt[:, o, c2, i, j] = ops["weight"][:, o, c2, i, j], ops["weight"][:, o, c1, i, j]
        return epilogue(c, ops, gemm(c, col, nb, wt), res)[1]
    if kind == "dilation_ignored":
        return epilogue(c, ops, gemm(c, columns(c, ops, ref["pix"], dil=1), nb, ops["weight"]), res)[1]
    if kind.startswith("tap_one_column_off"):
        idx = strip_edge_pixels(c, kind.endswith("last"))
        assert idx.numel() > 0
        sub = (nb[idx], yy[idx], xx[idx])
        for t in (int(v) for v in torch.randperm(KK, generator=g)):        # not a tap that lies outside the map before and after
            dx = torch.zeros(idx.numel(), KK)
            dx[:, t] = 1
            col2 = columns(c, ops, sub, tap_dx=dx)
            if not torch.equal(col2, col[idx]):
                break
        acc2 = acc.clone()
        acc2[idx] = gemm(c, col2, sub[0], ops["weight"])
        return epilogue(c, ops, acc2, res)[1]
    raise ValueError(kind)


# ---- Winograd: an fp32 emulation of the transform path ---------------------------------------------------------------------------
_BT = {2: [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
       4: [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]}


def unpack_u(c, weight):
    """U [xi, cout_pad, cin] (float32) as the PRODUCT's packer computes and rounds it, unpacked from its fragment order."""
    from m3dssd_amd.engine import pack_wino, pack_wino44, pack_wino44_c16
    ci, cop = c["cin"], c["cout_pad"]
    if c["family"] == "w22":
        return pack_wino(weight, cop, "cpu").view(16, cop // 32, ci // 8, 2, 32, 4).permute(0, 1, 4, 2, 3, 5).reshape(16, cop, ci)
    if c["family"] == "l0":
        return pack_wino44_c16(weight, "cpu").view(36, 4, 16, 4).permute(0, 2, 1, 3).reshape(36, 16, 16)
    return pack_wino44(weight, cop, "cpu").view(cop // 32, ci // 16, 36, 2, 4, 16, 4).permute(2, 0, 3, 5, 1, 4, 6).reshape(36, cop, ci)


def _at44(m):
    """w44_at of csrc/wino44_conv.hip on the leading axis of m [6, ...] (fp32, the kernel's grouping) -> [4, ...]."""
    s1, d1, s2, d2 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    return torch.stack([m[0] + s1 + s2, d2 * 2.0 + d1, s2 * 4.0 + s1, d2 * 8.0 + d1 + m[5]])


def _at22(m):
    """The s0 / s1 sums of the F(2x2) output transform (csrc/wino_conv.hip, wave kernel epilogue) on the leading axis of m [4, ...]."""
    return torch.stack([m[0] + m[1] + m[2], (m[1] - m[2]) - m[3]])


def winograd_emulation(c, ops, seed):
    """fp32 emulation of a Winograd kernel on the case: integer B^T d B, U from the product's packer, the channel sum in fp32 in
    chunks of 4 taken in a seeded scrambled order, A^T . A in the kernel's grouping.  Returns (acc [M, cout] as float64, the
    order-independent bound max sum_c |U| |V| in quanta of U's lattice)."""
    m = 2 if c["family"] == "w22" else 4
    a = m + 2
    n, ci, h, w, co = c["n"], c["cin"], c["h"], c["w"], c["cout"]
    assert h % m == 0 and w % m == 0 and c["k"] == 3 and c["stride"] == 1 and c["pad"] == 1 and c["dil"] == 1
    th, tw = h // m, w // m
    d = torch.nn.functional.unfold(ops["x"].to(F64), a, padding=1, stride=m)                     # [n, ci * a * a, th * tw]
    d = d.view(n, ci, a, a, th * tw).permute(0, 4, 1, 2, 3).reshape(n * th * tw, ci, a, a)
    bt = torch.tensor(_BT[m], dtype=F64)
    v64 = bt @ d @ bt.T
    v = (bt.to(F32) @ d.to(F32) @ bt.T.to(F32))
    assert torch.equal(v.to(F64), v64)
    v = v.permute(2, 3, 0, 1).reshape(a * a, -1, ci)                                             # [xi, tiles, ci]
    u = unpack_u(c, ops["weight"][0])[:, :co]                                                    # [xi, co, ci]
    quantum = {"w22": 1.0 / 8, "w44": None, "l0": None}[c["family"]] or (1.0 / 128 if c["lattice"] == "w44a" else 1.0 / 64)
    bound = float(torch.bmm(v.abs().to(F64), u.abs().to(F64).transpose(1, 2)).max()) / quantum
    perm = torch.randperm(ci, generator=E._gen(seed + ci))
    acc = torch.zeros(a * a, v.shape[1], co, dtype=F32)
    for k0 in range(0, ci, 4):
        p = perm[k0:k0 + 4]
        acc = acc + torch.bmm(v[:, :, p], u[:, :, p].transpose(1, 2))
    mm = acc.view(a, a, -1, co)
    if m == 4:
        y = torch.stack([_at44(z) for z in _at44(mm)])                                           # [yy, xx, tiles, co]
    else:
        y = torch.stack([_at22(z) for z in _at22(mm)])
    y = y.view(m, m, n, th, tw, co).permute(2, 3, 0, 4, 1, 5).reshape(n * h * w, co)
    return y.to(F64), bound


# ---- device buffers ----------------------------------------------------------------------------------------------------------------
def igemm_weight(c, weight):
    """The [Cout_pad][K] layout of m3d_conv2d_forward, K = (i * kw + j) * Cin + c, rows >= Cout zero; one set per image."""
    nw, co, ci, k, _ = weight.shape
    wp = torch.zeros(nw, c["cout_pad"], k * k * ci)
    wp[:, :co] = weight.permute(0, 1, 3, 4, 2).reshape(nw, co, k * k * ci)
    return wp


def packed_weight(c, weight, device):
    """(flat device tensor, floats between per-image sets) in the order the case's family reads."""
    from m3dssd_amd.engine import pack_frag, pack_wino, pack_wino44, pack_wino44_c16
    fam = c["family"]
    if fam == "igemm":
        wp = igemm_weight(c, weight)
        return wp.reshape(-1).contiguous().to(device), wp[0].numel()
    if fam == "wave":
        sets = [pack_frag(wp, c["cout_pad"], device) for wp in igemm_weight(c, weight)[:, :c["cout"]]]
        return torch.cat(sets).contiguous(), sets[0].numel()
    if fam == "w22":
        return pack_wino(weight[0], c["cout_pad"], device), 0
    if fam == "w44":
        return pack_wino44(weight[0], c["cout_pad"], device), 0
    return (pack_wino44_c16(weight[0], device), weight[0].permute(2, 3, 1, 0).contiguous().to(device)), 0


def nhwc_view(t, cs, fill):
    """[n, C, h, w] -> [n * h * w, cs] float32 with the pad lanes [C, cs) holding `fill`."""
    n, ch, h, w = t.shape
    out = torch.full((n * h * w, cs), fill, dtype=F32)
    out[:, :ch] = t.permute(0, 2, 3, 1).reshape(-1, ch)
    return out


def output_buffer(c):
    """The output pre-filled with the sentinel, and the offset (floats) at which the kernel's view starts.  NHWC: [M + 1 guard
    row][out_cs].  Planar: [n][3 slots][cout + 1 planes][ho * wo], the kernel writes slot 1."""
    hw = c["ho"] * c["wo"]
    if c["planar"]:
        return torch.full((c["n"], 3, c["cout"] + 1, hw), SENT_OUT, dtype=F32), (c["cout"] + 1) * hw
    return torch.full((c["n"] * hw + 1, c["cout"] + c["out_x"]), SENT_OUT, dtype=F32), 0


def split_output(c, buf):
    """(result [M, cout], True if every word outside it still holds the sentinel) of an output buffer after the launch."""
    co = c["cout"]
    if c["planar"]:
        guard = torch.cat([buf[:, 0].reshape(-1), buf[:, 2].reshape(-1), buf[:, 1, co:].reshape(-1)])
        return buf[:, 1, :co].permute(0, 2, 1).reshape(-1, co), bool((guard == SENT_OUT).all())
    guard = torch.cat([buf[:-1, co:].reshape(-1), buf[-1].reshape(-1)])
    return buf[:-1, :co], bool((guard == SENT_OUT).all())


# ---- the matrix -------------------------------------------------------------------------------------------------------------------
# expect = what the library's queries answer (tests/test_gpu_conv_exact.py asserts it before the launch):
#   igemm  (bm, bn, bk) of m3d_conv2d_tile, and for the split-K cases the slices of m3d_conv2d_splitk_plan
#   wave   (slices, waves per workgroup) of m3d_conv_wave_wgsplit_width
#   w22    slices of the wave kernel when it is given a workspace
#   w44    (m3d_wino44_kpair, slices of m3d_wino44_splitk_plan)
BIG64, BIG128 = dict(n=1, h=131, w=131), dict(n=1, h=113, w=113)       # 135 x 3 and 100 x 4 tiles of 128 rows: blocks128 >= 400
IGEMM = [
    # every NHWC tile once with res_mode 1 and LeakyReLU; the 2 x 9 x 11 map ends in a ragged row tile
    case("ig_128x32x16_res1", "igemm", cin=16, cout=40, cout_pad=64, res_mode=1, expect=(128, 32, 16)),
    case("ig_128x32x32_res1", "igemm", cout=27, res_mode=1, expect=(128, 32, 32)),
    case("ig_64x64_res1", "igemm", cout=64, res_mode=1, expect=(64, 64, 32)),
    case("ig_64x128_res1", "igemm", cout=128, res_mode=1, expect=(64, 128, 32)),
    case("ig_128x64_res1", "igemm", cout=192, res_mode=1, expect=(128, 64, 32), **BIG64),
    case("ig_128x128_res1", "igemm", cout=512, res_mode=1, expect=(128, 128, 32), **BIG128),
    case("ig_64x64_res0", "igemm", cout=64, res_mode=0, expect=(64, 64, 32)),
    case("ig_128x32x32_nores", "igemm", cout=27, expect=(128, 32, 32)),
    case("ig_64x128_scale_only", "igemm", cout=100, cout_pad=128, res_mode=0, shift=0, expect=(64, 128, 32)),
    case("ig_64x64_shift_only", "igemm", cout=64, res_mode=1, scale=0, expect=(64, 64, 32)),
    case("ig_128x32x32_sigmoid_tail", "igemm", cout=27, sig=18, out_x=1, expect=(128, 32, 32)),
    case("ig_64x64_3x3_stride2", "igemm", h=18, w=22, k=3, stride=2, cout=64, res_mode=1, expect=(64, 64, 32)),
    case("ig_64x64_3x3_dil2", "igemm", k=3, dil=2, cout=64, res_mode=0, expect=(64, 64, 32)),
]
IGEMM_DEFORM = [
    case("igd_64x64_stride2", "igemm", h=18, w=22, k=3, stride=2, deform=1, cout=64, res_mode=1, expect=(64, 64, 32)),
    case("igd_64x128_dil2", "igemm", k=3, dil=2, deform=1, cout=128, res_mode=0, expect=(64, 128, 32)),
    case("igd_128x64", "igemm", k=3, deform=1, cout=192, res_mode=1, expect=(128, 64, 32), **BIG64),
    case("igd_128x128", "igemm", k=3, deform=1, cout=512, expect=(128, 128, 32), **BIG128),
]
IGEMM_PLANAR = [
    case("igp_128x32", "igemm", cout=27, planar=1, expect=(128, 32, 32)),
    case("igp_64x64", "igemm", cout=64, planar=1, act=0, expect=(64, 64, 32)),
    case("igp_64x128_sigmoid_tail", "igemm", cout=100, cout_pad=128, planar=1, sig=90, expect=(64, 128, 32)),
    case("igp_128x64", "igemm", cout=192, planar=1, scale=0, expect=(128, 64, 32), **BIG64),
    case("igp_128x128", "igemm", cout=500, cout_pad=512, planar=1, shift=0, expect=(128, 128, 32), **BIG128),
]
IGEMM_SPLITK = [
    # (tile, slices): 3x3 x Cin 64 = 18 k-tiles -> 2 slices of 9; 1x1 x Cin 272 on the bk = 16 tile = 17 k-tiles -> 9 + 8
    case("igs_2slices_4byte_view", "igemm", cin=64, k=3, cout=40, cout_pad=64, res_mode=1, sig=30, out_x=1, expect=(64, 64, 32, 2)),
    case("igs_2slices_16byte_view", "igemm", cin=64, k=3, cout=40, cout_pad=64, res_mode=1, sig=30, out_x=4, expect=(64, 64, 32, 2)),
    case("igs_uneven_bk16", "igemm", cin=272, cout=40, cout_pad=64, res_mode=1, sig=30, out_x=1, expect=(128, 32, 16, 2)),
]
IGEMM_PER_IMAGE = [
    case("igw_howo128_bm128", "igemm", h=8, w=16, cout=27, per_image=1, res_mode=1, expect=(128, 32, 32)),
    case("igw_howo128_bm64", "igemm", h=8, w=16, cout=64, per_image=1, res_mode=0, expect=(64, 64, 32)),
    case("igw_howo64", "igemm", h=8, w=8, cout=64, per_image=1, res_mode=1, expect=(64, 64, 32)),
    # blocks128 = 101 x 4 >= 400 asks for 128 rows, Ho*Wo = 6464 = 50.5 x 128: the bm = 64 fall-back
    case("igw_fallback_to_bm64", "igemm", h=64, w=101, cout=512, per_image=1, expect=(64, 128, 32)),
]
IGEMM_PER_IMAGE_REFUSED = [
    case("igw_howo99_refused", "igemm", cout=64, per_image=1),
    # the 32-channel tiles exist with 128 rows only: a 128-row tile over two 64-pixel images would use the first image's weights
    case("igw_howo64_bn32_refused", "igemm", h=8, w=8, cout=27, per_image=1),
]
WAVE = [
    case("wv_dil2_plain", "wave", n=1, k=3, dil=2, cout=128, res_mode=0, in_x=0, entry="forward", expect=(2, 2)),
    case("wv_dil2_plain_wgsplit", "wave", n=1, k=3, dil=2, cout=128, res_mode=1, in_x=32, entry="wgsplit", expect=(2, 2)),
    case("wv_dil2_deform", "wave", n=1, k=3, dil=2, deform=1, cout=64, res_mode=1, in_x=0, entry="forward", expect=(2, 2)),
    case("wv_dil2_deform_wgsplit", "wave", n=1, k=3, dil=2, deform=1, cout=100, res_mode=0, in_x=32, entry="wgsplit", expect=(2, 2)),
    case("wv_per_image", "wave", h=8, w=12, cin=256, cout=64, per_image=1, res_mode=1, in_x=0, entry="forward", expect=(2, 2)),
    case("wv_per_image_workspace", "wave", h=8, w=12, cin=256, cout=100, per_image=1, res_mode=0, in_x=32, entry="workspace", expect=(2, 2)),
]
WAVE_REFUSED = [case("wv_per_image_howo99_refused", "wave", cin=256, cout=64, per_image=1, in_x=0)]
W22 = [
    # 30 tiles: a ragged last group for the 64-tile LDS kernel and the 32-tile wave kernel alike; Cin 128 -> 2 slices with a workspace
    case("w22_co27_sigmoid_tail", "w22", n=1, cin=128, h=10, w=12, k=3, cout=27, act=0, sig=18, forms=("lds", "wave_refused", "wave_ws"), expect=2),
    case("w22_co64_res1_wide_views", "w22", n=2, cin=128, h=6, w=10, k=3, cout=64, res_mode=1, forms=("lds", "wave", "wave_ws"), expect=2),
    case("w22_scale_only", "w22", n=1, cin=128, h=10, w=12, k=3, cout=40, res_mode=0, shift=0, forms=("lds", "wave", "wave_ws"), expect=2),
]
W44 = [
    # Cin <= 64: lattice A, plain workgroups (nb 1 = 64 channels, nb 2 = 128 channels)
    case("w44_one_tile_nores_noact", "w44", n=1, cin=16, h=4, w=4, k=3, cout=128, act=0, forms=("nb1", "nb2"), expect=(0, 1)),
    case("w44_ragged_co100_res1_wide_views", "w44", n=2, cin=32, h=8, w=12, k=3, cout=100, cout_pad=128, res_mode=1, forms=("nb1", "nb2", "touch"), expect=(0, 1)),
    case("w44_co40_res0", "w44", n=1, cin=48, h=20, w=36, k=3, cout=40, res_mode=0, forms=("nb1",), expect=(0, 1)),
    case("w44_co128_res0_scale_only", "w44", n=3, cin=64, h=12, w=20, k=3, cout=128, res_mode=0, shift=0, forms=("nb1", "nb2"), expect=(0, 1)),
    case("w44_co128_nores_shift_only", "w44", n=1, cin=64, h=8, w=8, k=3, cout=128, scale=0, forms=("nb1", "nb2"), expect=(0, 1)),
    # Cin >= 128: lattice B; nb 1 runs K-pair workgroups on these small maps
    case("w44_kpair_co100_res1_wide_views", "w44", n=2, cin=128, h=8, w=12, k=3, cout=100, cout_pad=128, res_mode=1, forms=("nb1", "nb2", "touch"), expect=(1, 1)),
    case("w44_kpair_co40_res0", "w44", n=1, cin=128, h=20, w=36, k=3, cout=40, res_mode=0, forms=("nb1",), expect=(1, 1)),
    case("w44_kpair_one_tile_nores_noact", "w44", n=1, cin=128, h=4, w=4, k=3, cout=128, act=0, forms=("nb1", "nb2"), expect=(1, 1)),
    case("w44_kpair_co128_nores", "w44", n=1, cin=256, h=8, w=8, k=3, cout=128, forms=("nb1", "nb2"), expect=(1, 1)),
    # split-K: 25 strips x 8 (4) blocks of 64 channels = 200 (100) workgroups -> 2 (4) slices
    case("w44_split2_nores_noact", "w44", n=1, cin=128, h=80, w=80, k=3, cout=512, act=0, forms=("split",), expect=(1, 2)),
    case("w44_split2_co500_res1_4byte_view", "w44", n=1, cin=128, h=80, w=80, k=3, cout=500, cout_pad=512, res_mode=1, out_x=1, forms=("split",), expect=(1, 2)),
    case("w44_split4_res0", "w44", n=1, cin=256, h=80, w=80, k=3, cout=256, res_mode=0, forms=("split",), expect=(1, 4)),
]
LEVEL0 = [case("l0_%dx%dx%d" % s, "l0", n=s[0], cin=16, h=s[1], w=s[2], k=3, cout=16) for s in ((1, 4, 4), (2, 8, 12), (3, 20, 36))]

DIRECT_CASES = IGEMM + IGEMM_DEFORM + IGEMM_PLANAR + IGEMM_SPLITK + IGEMM_PER_IMAGE + WAVE
WINOGRAD_CASES = W22 + W44 + LEVEL0
CASES = DIRECT_CASES + WINOGRAD_CASES
assert len({c["name"] for c in CASES}) == len(CASES)


def ids(cases):
    return [c["name"] for c in cases]
