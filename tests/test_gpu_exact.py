"""GPU tests with exact-arithmetic inputs (tests/exact_inputs.py): the bf16 deformable kernels, the fused multi-layer bf16 kernels
and the attention against a plain float64 reference, compared with torch.equal -- no element excluded, no tolerance.

The operands come from small dyadic lattices on which every value a kernel holds (corner weights, the modulated sample, hidden
activations, folded weights, fp32 partial sums) is exactly representable in the narrowest type on its path, so the kernel has to
return the float64 result bit for bit (fp32 output modes), or that result rounded once to bf16, round to nearest even (bf16 output
mode).  tests/test_exact_inputs_host.py proves the premise on the CPU for every generator and shape used here
(`assert_exact_under`) and shows that a dropped corner, swapped corners, a dropped 8-channel chunk, two swapped channels or a tap
read one column off always changes the result.  The tolerance tests of tests/test_gpu_bf16.py stay as they are: they cover
what rounds (random operands, the negative branch of LeakyReLU, sigmoid gates, a soft softmax).

Not covered here: the sigmoid gates of m3d_anab_qkvs_bf16_forward (an exponential on the data path).
"""
import ctypes
import time

import pytest
import torch

import exact_inputs as E
from gpu_common import _dev, _log, _nhwc16, _run_conv, _stream
from m3dssd_amd import _hip

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
OUT_DTYPE = {0: BF16, 1: torch.float32, 2: torch.float32}


def _expect(name, case, got, ref64, out_dtype, quantum, t0):
    ndiff, msg = E.compare_exact(got, ref64, out_dtype, quantum)
    _log("exact_" + name, dict(case=case, out=str(out_dtype).replace("torch.", ""), differing=ndiff, seconds=round(time.time() - t0, 3)))
    assert ndiff == 0, "%s %s (%s output): %s" % (name, case, str(out_dtype).replace("torch.", ""), msg)


def _dcn_bf16(ops, ref64, name, case, variant=None, patch=False, om_cs=None, epilogue=True, modes=(1, 0), res_is_input=False):
    """One set of exact DCNv2 operands through m3d_conv_bf16_forward: bias only, then BatchNorm-like affine + residual + LeakyReLU
    through the shared epilogue; fp32 and bf16 output."""
    k = ops["weight"].shape[2]
    om = E.pack_om(ops, om_cs if om_cs is not None else (32 if k == 3 else 4))
    x, wt, b, pad = ops["x"], ops["weight"], ops["bias"], ops["pad"]
    for om_mode in modes:
        t0 = time.time()
        var = variant(om_mode) if callable(variant) else variant
        res = x if res_is_input else None
        got = _run_conv(x, wt, b, None, 1, pad, 0, res, 0, -1, om_mode, om, variant=var, patch=patch)
        _expect(name, case + ["bias" + ("+input" if res_is_input else "")], got, E.apply_epilogue(ref64, res=res), OUT_DTYPE[om_mode],
                E.DCN_QUANTUM, t0)
        if not epilogue:
            continue
        t0 = time.time()
        scale, shift, res = E.dcn_epilogue_operands(sum(ops["x"].shape), ops, ref64, act=1)
        want = E.apply_epilogue(ref64, scale, shift, res, act=1)
        assert float(E.apply_epilogue(ref64, scale, shift, res, act=0).min()) >= 0        # LeakyReLU is the identity here
        # the bias goes through the affine: (acc + bias) * scale + shift = acc * scale + (bias * scale + shift), all dyadic
        ref_nb = ref64 - b.double().view(1, -1, 1, 1)
        assert torch.equal(E.apply_epilogue(ref_nb, scale, b * scale + shift, res, act=1), want)
        got = _run_conv(x, wt, None, None, 1, pad, 1, res, 0, -1, om_mode, om, variant=var, patch=patch, affine=(scale, b * scale + shift))
        _expect(name, case + ["affine+res+act"], got, want, OUT_DTYPE[om_mode], E.DCN_QUANTUM / 2, t0)


# ------------------------------------------------------------------------------------ DCNv2: implicit-GEMM bf16 tile
IGEMM_SHAPES = [(2, 128, 16, 40, 128, 3, 1), (1, 64, 9, 13, 64, 3, 1), (1, 512, 6, 10, 256, 3, 1), (2, 128, 16, 40, 128, 1, 0),
                (1, 24, 16, 24, 32, 1, 0)]


@pytest.mark.parametrize("shape", IGEMM_SHAPES)
def test_dcn_bf16_implicit_gemm_is_exact(shape):
    """csrc/bf16_conv.hip in deformable mode (uniform-K path, 1x1, and the general-K path with Cin 24): exact.  The 1x1 128 -> 128
    case with bf16 output is taken by csrc/bf16_dcn1x1.hip (variant 6); its fp32 output mode runs on the generic tile."""
    n, c, h, w, co, k, pad = shape
    ops = E.dcn_operands(sum(shape), n, c, h, w, co, k, pad)
    ref = E.dcn_ref(ops)
    is_1x1_kernel = (c, co, k) == (128, 128, 1)
    _dcn_bf16(ops, ref, "dcn_igemm", list(shape), variant=lambda mode: 6 if (is_1x1_kernel and mode == 0) else 0)


# ------------------------------------------------------------------------------------ DCNv2: LDS-patch kernel
PATCH_CASES = [
    # shape (n, c, h, w, co), variant, (image, channel of [off], row, column, value) of one offset placed at the window radius
    ((2, 128, 16, 32, 128), 4, None),
    ((1, 32, 16, 16, 100), 4, None),              # ragged Cout
    ((3, 64, 8, 16, 128), 3, None),               # one patch per image: every window crosses all four borders
    ((2, 256, 24, 80, 256), 3, None),
    ((2, 128, 16, 32, 128), 4, (1, 4, 9, 17, 8.75)),        # offsets that reach the window radius exactly: 9 rows of 16 x 16 tiles
    ((3, 64, 8, 16, 128), 3, (2, 13, 3, 8, -5.75)),         # radius 6 of the 8 x 16 tiles
]


def patch_operands(shape, at_radius):
    n, c, h, w, co = shape
    ops = E.dcn_operands(sum(shape) + 1, n, c, h, w, co, 3, 1)
    if at_radius is not None:
        b, ch, y, x, v = at_radius
        ops["off"][b, ch, y, x] = v
    return ops


@pytest.mark.parametrize("shape,variant,at_radius", PATCH_CASES)
def test_dcn_bf16_patch_kernel_is_exact(shape, variant, at_radius):
    """csrc/bf16_dcn_patch.hip (fp16 window in LDS, fp16 corner weights, v_pk_fma_f16 combine, fp16 weight copy): exact, bias
    only and through the shared epilogue, fp32 and bf16 output."""
    ops = patch_operands(shape, at_radius)
    ref = E.dcn_ref(ops)
    _dcn_bf16(ops, ref, "dcn_patch", list(shape) + [variant, at_radius is not None], variant=variant, patch=True,
              epilogue=at_radius is None)


def handover_operands():
    ops = E.dcn_operands(71, 2, 64, 16, 32, 128, 3, 1)
    ops["off"][1, 5, 7, 9] = 10.25                # dw of tap 2 at one pixel of image 1: beyond the radius 9 of its 16 x 16 tile
    return ops


def test_dcn_bf16_patch_kernel_hand_over_is_exact():
    """One pixel tile whose offset exceeds the radius: that tile is recomputed by the implicit-GEMM kernel, the others stay with the
    patch kernel -- and the WHOLE output equals the reference (tests/test_gpu_bf16.py can only say which kernel's bits a tile carries)."""
    ops = handover_operands()
    _dcn_bf16(ops, E.dcn_ref(ops), "dcn_patch_handover", [2, 64, 16, 32, 128], variant=4, patch=True, epilogue=False)


# ------------------------------------------------------------------------------------ DCNv2: 1x1 kernel
@pytest.mark.parametrize("n,h,w", [(2, 16, 40), (1, 9, 13), (3, 8, 16)])
@pytest.mark.parametrize("with_res", [False, True])
def test_dcn1x1_bf16_kernel_is_exact(n, h, w, with_res):
    """csrc/bf16_dcn1x1.hip (center_align: 1x1 DCNv2 128 -> 128 + bias (+ the input as residual)); several tiles, a ragged single
    tile (117 pixels).  Its output is bf16: the float64 result rounded once."""
    ops = E.dcn_operands(n * 100 + h, n, 128, h, w, 128, 1, 0)
    _dcn_bf16(ops, E.dcn_ref(ops), "dcn1x1", [n, h, w, with_res], variant=6, epilogue=False, modes=(0,), res_is_input=with_res)


# ------------------------------------------------------------------------------------ DCNv2: border grid
def border_operands(c, co, h, w, k):
    """k = 1: a 1x1 deformable conv sampling the quarter-step border grid; k = 3: the centre tap of a 3x3 does, the other taps have
    mask 0 and taps that would leave the patch radius are dropped (as tests/test_gpu_bf16.py does)."""
    ops = E.dcn_operands(5 + c, 1, c, h, w, co, k, k // 2)
    grid = E.border_grid_offsets(h, w)
    if k == 1:
        ops["off"], ops["mask"] = grid, torch.ones(1, 1, h, w)
    else:
        off, m = torch.zeros(1, 18, h, w), torch.zeros(1, 9, h, w)
        off[:, 8:10] = grid
        m[:, 4] = 1.0
        keep = (off.abs() <= 8.75).all(1, keepdim=True)
        ops["off"], ops["mask"] = off * keep, m * keep
    return ops


@pytest.mark.parametrize("c,co,k", [(64, 32, 1), (24, 32, 1), (32, 128, 3)])
def test_dcn_bf16_border_grid_is_exact(c, co, k):
    """Every in / out decision of the corner rules (exactly -1, just inside, between rows, the last row, past it, just below H,
    exactly H) on the bf16 tile (uniform-K Cin 64, general-K Cin 24) and on the patch kernel: exact equality with the reference."""
    h, w = (16, 24) if k == 1 else (16, 32)
    ops = border_operands(c, co, h, w, k)
    ref = E.dcn_ref(ops)
    assert (ref - ops["bias"].double().view(1, -1, 1, 1))[0, :, 0::8].abs().max() == 0       # sampled exactly at -1: only the bias
    _dcn_bf16(ops, ref, "dcn_border_grid", [c, co, k], variant=4 if k == 3 else 0, patch=k == 3, epilogue=False)


# ------------------------------------------------------------------------------------ DCNv2: the fp32 kernels as the control
CONTROL_SHAPES = [(2, 64, 12, 16, 32, 3, 1, 2), (1, 128, 16, 40, 128, 3, 1, 1), (2, 32, 9, 13, 128, 3, 1, 1), (2, 128, 16, 24, 256, 1, 0, 1),
                  (1, 20, 9, 7, 24, 3, 1, 1)]


@pytest.mark.parametrize("shape", CONTROL_SHAPES)
def test_dcn_fp32_kernels_are_exact_on_the_same_inputs(shape):
    """The control: the same exact operands through the fp32 deformable kernels -- the drop-in op m3d_dcn_v2_forward (also with
    deformable_groups = 2), the LDS-tiled deformable igemm and the wave-granular m3d_conv_wave_forward.  They are exact as well:
    it is the inputs, not a property of the bf16 kernels, that makes the comparison strict."""
    from m3dssd_amd.engine import pack_frag
    from m3dssd_amd.host import ops as hops
    from m3dssd_amd.host import standalone as S
    dev, L = _dev(), _hip.lib()
    n, c, h, w, co, k, pad, dg = shape
    ops = E.dcn_operands(sum(shape), n, c, h, w, co, k, pad, dg=dg)
    ref = E.dcn_ref(ops)
    x, off, m, wt, b = (ops[kk].to(dev) for kk in ("x", "off", "mask", "weight", "bias"))
    t0 = time.time()
    got = hops.dcn_v2_forward(x, off, m, wt, b, 1, pad, 1, dg).cpu()
    _expect("dcn_fp32_op", list(shape), got, ref, torch.float32, E.DCN_QUANTUM, t0)
    if dg != 1:
        return
    cin_pad = (c + 31) // 32 * 32
    cpt = 64 if co <= 64 else 128
    v, _ = S._to_nhwc(x, cin_pad)
    om, _ = S._to_nhwc(torch.cat([off, m], 1))
    t0 = time.time()
    out_blk, keep = S.conv_nhwc(v, wt, b, None, 1, pad, act=0, om=om, cout_pad_to=cpt)
    _expect("dcn_fp32_igemm", list(shape), S._to_nchw(out_blk, co).cpu(), ref, torch.float32, E.DCN_QUANTUM, t0)
    t0 = time.time()
    wp, co_, cop, kh, kw = S._pack(wt, cin_pad, cpt)
    frag = pack_frag(wp.view(cop, kh * kw * cin_pad), cop, dev)
    sc, sh = S._affine(co, b, None, dev)
    out = torch.zeros(n * h * w * co, device=dev)
    d = _hip.ConvDesc()
    d.inp, d.in_cs, d.N, d.H, d.W, d.Cin = v.ptr, v.cs, n, h, w, cin_pad
    d.wgt, d.Cout, d.Cout_pad = frag.data_ptr(), co, cop
    d.kh, d.kw, d.stride, d.pad, d.dil, d.Ho, d.Wo = k, k, 1, pad, 1, h, w
    d.out, d.out_cs, d.scale, d.shift = out.data_ptr(), co, sc.data_ptr(), sh.data_ptr()
    d.act, d.sigmoid_from = 0, -1
    d.dcn_offmask, d.dcn_om_cs = om.ptr, om.cs
    _hip.check(L.m3d_conv_wave_forward(ctypes.byref(d), S._stream()))
    torch.cuda.synchronize()
    _expect("dcn_fp32_wave", list(shape), out.view(n, h, w, co).permute(0, 3, 1, 2).cpu(), ref, torch.float32, E.DCN_QUANTUM, t0)


# ------------------------------------------------------------------------------------ fused heads
HEAD_SHAPES = [(1, 2, 8, 16, 36), (4, 1, 13, 21, 36), (2, 2, 16, 40, 5)]


def head_operands(G, n, h, w, cout):
    heads, x = [], None
    for gi in range(G):
        heads.append(E.mlp_operands(G * 100 + h + gi, n * h * w, [128, 256, 256, cout], x=x))
        x = heads[0]["x"]
    return heads


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("G,n,h,w,cout", HEAD_SHAPES)
def test_fused_head_mlp_bf16_is_exact(G, n, h, w, cout, form):
    """m3d_head_mlp_bf16_forward (hidden maps as bf16) and m3d_head_mlp2_bf16_forward (hidden maps as fp16, scales folded into the
    weights): three layers, the heads of one map in one launch, planar fp32 output -- exact."""
    from m3dssd_amd.engine_bf16 import pack_head2
    L, dev = _hip.lib(), _dev()
    heads = head_operands(G, n, h, w, cout)
    M, HW = n * h * w, h * w
    t0 = time.time()
    xin = _nhwc16(heads[0]["x"].view(n, h, w, 128).permute(0, 3, 1, 2), 136)
    out = torch.full((n, G * cout + 1, HW), 512.0, device=dev)
    lay = [[hd["layers"][li] for hd in heads] for li in range(3)]
    if form == 1:
        w3 = torch.zeros(G, 64, 256)
        w3[:, :cout] = torch.stack([l[0] for l in lay[2]])
        dv = [torch.stack([l[0] for l in lay[0]]).to(BF16), torch.stack([l[0] for l in lay[1]]).to(BF16), w3.to(BF16)]
        for li in range(3):
            dv += [torch.stack([l[1] for l in lay[li]]), torch.stack([l[2] for l in lay[li]])]
        dv = [t.to(dev).contiguous() for t in dv]
        d = _hip.HeadBf16Desc()
        d.inp, d.in_cs, d.M, d.Cin = xin.data_ptr(), 136, M, 128
        d.w1, d.w2, d.w3, d.s1, d.t1, d.s2, d.t2, d.s3, d.t3 = (t.data_ptr() for t in dv)
        d.Cout, d.Cout_pad, d.out = cout, 64, out.data_ptr()
        d.out_group_off, d.out_img_stride, d.HW, d.groups = cout * HW, (G * cout + 1) * HW, HW, G
        _hip.check(L.m3d_head_mlp_bf16_forward(ctypes.byref(d), _stream()))
    else:
        pk = pack_head2([tuple(v for li in range(3) for v in hd["layers"][li]) for hd in heads], dev)
        d = _hip.Head2Bf16Desc()
        d.inp, d.in_cs, d.M = xin.data_ptr(), 136, M
        d.w1f, d.w2f, d.w3, d.t1, d.t2, d.t3 = (t.data_ptr() for t in pk)
        d.Cout, d.out = cout, out.data_ptr()
        d.out_group_off, d.out_img_stride, d.HW, d.groups = cout * HW, (G * cout + 1) * HW, HW, G
        _hip.check(L.m3d_head_mlp2_bf16_forward(ctypes.byref(d), _stream()))
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[:, G * cout] == 512.0).all()
    ref = torch.cat([E.mlp_ref(hd).view(n, HW, cout).permute(0, 2, 1) for hd in heads], 1)
    _expect("head_mlp%d" % form, [G, n, h, w, cout], got[:, :G * cout], ref, torch.float32, E.MLP_QUANTUM, t0)


TAIL_SHAPES = [(2, 8, 16, 256), (1, 13, 21, 144), (2, 4, 16, 20)]


def tail_operands(n, h, w, cout):
    return E.mlp_operands(n * 100 + h + cout, n * h * w, [256, 256, cout])


@pytest.mark.parametrize("n,h,w,cout", TAIL_SHAPES)
def test_head_tail2_bf16_is_exact(n, h, w, cout):
    """m3d_head_tail2_bf16_forward (cls.3 + cls.6 in one launch, the hidden map as fp16): Cout 256 / 144 / 20, a ragged tile."""
    from m3dssd_amd.engine_bf16 import pack_tail2
    L, dev = _hip.lib(), _dev()
    ops = tail_operands(n, h, w, cout)
    M, HW = n * h * w, h * w
    t0 = time.time()
    xin = _nhwc16(ops["x"].view(n, h, w, 256).permute(0, 3, 1, 2), 264)
    (wa, sa, ta), (wb, sb, tb) = ops["layers"]
    out = torch.full((n, cout + 1, HW), 512.0, device=dev)
    pk = pack_tail2(wa, sa, ta, wb, sb, tb, dev)
    d = _hip.Tail2Bf16Desc()
    d.inp, d.in_cs, d.M = xin.data_ptr(), 264, M
    d.waf, d.wbf, d.t1, d.t2 = (t.data_ptr() for t in pk)
    d.Cout, d.out, d.out_img_stride, d.HW = cout, out.data_ptr(), (cout + 1) * HW, HW
    _hip.check(L.m3d_head_tail2_bf16_forward(ctypes.byref(d), _stream()))
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[:, cout] == 512.0).all()
    ref = E.mlp_ref(ops).view(n, HW, cout).permute(0, 2, 1)
    _expect("head_tail2", [n, h, w, cout], got[:, :cout], ref, torch.float32, E.MLP_QUANTUM, t0)


# ------------------------------------------------------------------------------------ ANAB projections
QKVS_SHAPES = [(2, 8, 16), (1, 13, 21)]


def qkvs_operands(n, h, w):
    """x +-1, weights +-1/16: q, k, v are multiples of 1/8 below 8 in magnitude -- exact in the bf16 they are stored in."""
    g = E._gen(h * 7 + w)
    x = E._pick(g, [-1.0, 1.0], (n * h * w, 128)).float()
    wq, wk, wv, ws = (E._pick(g, [-1.0 / 16, 1.0 / 16], (c, 128)).float() for c in (168, 168, 128, 4))
    return dict(x=x, layers=[(torch.cat([wq, wk, wv]), torch.ones(464), torch.zeros(464))], ws=ws)


@pytest.mark.parametrize("n,h,w", QKVS_SHAPES)
def test_anab_qkvs_bf16_q_and_kv_are_exact(n, h, w):
    """m3d_anab_qkvs_bf16_forward: q and k|v (bf16 outputs) exact, the padding rows of q exact zeros.  The sigmoid gates carry an
    exponential on the data path and stay with their tolerance test."""
    from m3dssd_amd.engine_bf16 import _head2_frag
    L, dev = _hip.lib(), _dev()
    ck, cv, ns, ckp = 168, 128, 4, 192
    ops = qkvs_operands(n, h, w)
    M = n * h * w
    t0 = time.time()
    wall = ops["layers"][0][0]
    stack = torch.zeros(512, 128)
    stack[:ck], stack[ckp:ckp + ck + cv], stack[ckp + ck + cv:ckp + ck + cv + ns] = wall[:ck], wall[ck:], ops["ws"]
    wf = torch.cat([_head2_frag(stack[256 * i:256 * (i + 1)], BF16) for i in range(2)], 0).contiguous().to(dev)
    xin = _nhwc16(ops["x"].view(n, h, w, 128).permute(0, 3, 1, 2), 136)
    q = torch.full((M, ckp + 8), 512.0, device=dev, dtype=BF16)
    kv = torch.full((M, ck + cv + 8), 512.0, device=dev, dtype=BF16)
    sg = torch.full((M, 8), 512.0, device=dev)
    d = _hip.QkvsBf16Desc()
    d.inp, d.in_cs, d.M, d.wf = xin.data_ptr(), 136, M, wf.data_ptr()
    d.q, d.q_cs, d.q_rows = q.data_ptr(), ckp + 8, ckp
    d.kv, d.kv_cs, d.kv_rows = kv.data_ptr(), ck + cv + 8, ck + cv
    d.s, d.s_cs, d.s_rows = sg.data_ptr(), 8, ns
    _hip.check(L.m3d_anab_qkvs_bf16_forward(ctypes.byref(d), _stream()))
    torch.cuda.synchronize()
    ref = E.mlp_ref(ops)
    _expect("anab_qkvs_q", [n, h, w], q[:, :ck].float().cpu(), ref[:, :ck], BF16, 0.125, t0)
    _expect("anab_qkvs_kv", [n, h, w], kv[:, :ck + cv].float().cpu(), ref[:, ck:], BF16, 0.125, t0)
    assert (q[:, ck:ckp].float() == 0).all() and (q[:, ckp:].float() == 512.0).all() and (kv[:, ck + cv:].float() == 512.0).all()


# ------------------------------------------------------------------------------------ attention with a one-hot softmax
ATTEND_SHAPES = [(2, 384, 337), (3, 128, 85)]      # H*W must be a multiple of 128 (the entry refuses anything else); 384 = three pixel tiles


@pytest.mark.parametrize("B,HW,keys", ATTEND_SHAPES)
@pytest.mark.parametrize("kernel", ["bf16", "f32"])
def test_anab_attend_one_hot_softmax_is_exact(B, HW, keys, kernel):
    """m3d_anab_attend_bf16, and m3d_anab_attend_f32 as its control, with logits whose softmax is exactly one-hot: the output is
    exactly the target key's value row plus the residual through the affine.  Every key index 0 .. keys - 1 is the target of at
    least one query of every image where H*W >= keys (384 >= 337, 128 >= 85); the padding keys would win if they were let in.
    Pins key and value indexing and the padding exactly, which the tolerance test can only bound."""
    L, dev = _hip.lib(), _dev()
    ops = E.attend_operands(B * 100 + keys, B, HW, keys, kp=None if kernel == "bf16" else (keys + 31) // 32 * 32)
    for b in range(B):
        assert ops["target"][b].unique().numel() == keys
    ref = E.attend_ref(ops)
    cv, ck, ckp = 128, 168, 192
    kp = ops["khat"].shape[1]
    t0 = time.time()
    dsc, dsh = ops["scale"].to(dev), ops["shift"].to(dev)
    if kernel == "bf16":
        dq, dk, dvv, dr = (ops[k].to(BF16).contiguous().to(dev) for k in ("q", "khat", "vhat", "res"))
        out = torch.full((B * HW, cv + 8), 512.0, device=dev, dtype=BF16)
        _hip.check(L.m3d_anab_attend_bf16(dq.data_ptr(), ckp, dk.data_ptr(), dvv.data_ptr(), B, HW, ckp, keys, kp, cv, dr.data_ptr(), cv,
                                          dsc.data_ptr(), dsh.data_ptr(), 1, out.data_ptr(), cv + 8, _stream()))
    else:
        dq, dk, dvv, dr = (ops[k].contiguous().to(dev) for k in ("q", "khat", "vhat", "res"))
        out = torch.full((B * HW, cv + 4), 512.0, device=dev)
        _hip.check(L.m3d_anab_attend_f32(dq.data_ptr(), ckp, dk.data_ptr(), ckp, dvv.data_ptr(), B, HW, ck, keys, kp, cv, dr.data_ptr(), cv,
                                         1, dsc.data_ptr(), dsh.data_ptr(), 1, out.data_ptr(), cv + 4, _stream()))
    torch.cuda.synchronize()
    assert (out[:, cv:].float() == 512.0).all()
    _expect("anab_attend_" + kernel, [B, HW, keys], out[:, :cv].float().cpu(), ref, BF16 if kernel == "bf16" else torch.float32, 0.5, t0)


# ------------------------------------------------------------------------------------ tree entry
TREE_SHAPES = [(cin, H, W) for cin in (32, 64, 128, 256) for (H, W) in ((24, 80), (20, 36))]


def tree_operands(cin, H, W):
    return E.tree_entry_operands(cin + H, 1, cin, H, W)


@pytest.mark.parametrize("cin,H,W", TREE_SHAPES)
def test_tree_entry_bf16_is_exact(cin, H, W):
    """m3d_tree_entry_bf16_forward (max-pool + 1x1 project + 3x3 stride-2 conv1 in one launch): every level's channel pair on
    partial tiles (24 x 80 -> 12 x 40, 20 x 36 -> 10 x 18).  t and res are the float64 results rounded once to bf16, bottom is exact."""
    from m3dssd_amd.engine_bf16 import pack_tree_entry
    L, dev = _hip.lib(), _dev()
    ops = tree_operands(cin, H, W)
    ref = E.tree_entry_ref(ops)
    n, co, Ho, Wo = 1, 2 * cin, H // 2, W // 2
    t0 = time.time()
    xin = _nhwc16(ops["x"], cin + 8)
    t = torch.full((n, Ho, Wo, co + 8), 512.0, device=dev, dtype=BF16)
    res = torch.full((n, Ho, Wo, co), 512.0, device=dev, dtype=BF16)
    bot = torch.full((n, Ho, Wo, cin + 16), 512.0, device=dev, dtype=BF16)
    wf = pack_tree_entry(ops["w1"], ops["s1"], ops["wp"], ops["sp"], dev)
    dv = [v.to(dev).contiguous() for v in (ops["t1"], ops["tp"])]
    d = _hip.TreeEntryBf16Desc()
    d.inp, d.in_cs, d.N, d.H, d.W, d.Cin, d.Cout = xin.data_ptr(), cin + 8, n, H, W, cin, co
    d.wfrag, d.shift1, d.shiftp = wf.data_ptr(), dv[0].data_ptr(), dv[1].data_ptr()
    d.t, d.t_cs, d.res, d.res_cs = t.data_ptr(), co + 8, res.data_ptr(), co
    d.bottom, d.bottom_cs = bot.data_ptr() + 2 * 8, cin + 16              # a channel slice [8, 8 + cin) of a wider buffer
    assert L.m3d_tree_entry_bf16_applicable(ctypes.byref(d)) == 1
    _hip.check(L.m3d_tree_entry_bf16_forward(ctypes.byref(d), _stream()))
    torch.cuda.synchronize()
    assert (t[..., co:].float() == 512.0).all() and (bot[..., :8].float() == 512.0).all() and (bot[..., 8 + cin:].float() == 512.0).all()
    for name, got, want in (("t", t[..., :co], ref[:, :co]), ("res", res, ref[:, co:2 * co]), ("bottom", bot[..., 8:8 + cin], ref[:, 2 * co:])):
        _expect("tree_entry_" + name, [cin, H, W], got.float().permute(0, 3, 1, 2).cpu(), want, BF16, E.TREE_QUANTUM, t0)


# ------------------------------------------------------------------------------------ fused front end
FRONT_SHAPES = [(1, 16, 32, False),         # one tile: every border at once
                (1, 48, 96, False),         # 3 x 3 tiles: the middle one takes the mask-free interior path
                (1, 32, 80, False),         # a width that is not a multiple of the tile
                (2, 32, 128, True),         # uint8 frames, smaller than the crop: the border between frame and crop is (0 - mean) / std
                (1, 48, 112, True)]         # uint8 with an interior tile


def front_operands(n, H, W, u8):
    return E.frontend_operands(H + W, n, H, W, u8)


@pytest.mark.parametrize("n,H,W,u8", FRONT_SHAPES)
def test_fused_frontend_bf16_is_exact(n, H, W, u8):
    """m3d_frontend2_bf16_forward (stem -> level0 -> level1 in one launch, the image tile and both intermediates fp16 in LDS): the
    float64 chain rounded once to bf16.  uint8 input with bytes {0, 255}, for which the division by 255 is exact."""
    from m3dssd_amd.engine_bf16 import pack_frontend_f16
    L, dev = _hip.lib(), _dev()
    ops = front_operands(n, H, W, u8)
    ref = E.frontend_ref(ops)
    t0 = time.time()
    src = (ops["frames"] if u8 else ops["img"]).contiguous().to(dev)
    (ws, s0, h0, _, _), (w0, s1, h1, _, _), (w1, s2, h2, _, _) = ops["layers"]
    out = torch.full((n, H // 2, W // 2, 40), 512.0, device=dev, dtype=BF16)
    mean3, stds3 = (ctypes.c_float * 3)(*E.FRONT_MEAN), (ctypes.c_float * 3)(*E.FRONT_STDS)
    f2 = pack_frontend_f16(ws, (s0, h0), w0, (s1, h1), w1, (s2, h2), dev)
    _hip.check(L.m3d_frontend2_bf16_forward(src.data_ptr(), 1 if u8 else 0, H - 5 if u8 else 0, W - 9 if u8 else 0, mean3, stds3,
                                            f2[0].data_ptr(), f2[1].data_ptr(), f2[2].data_ptr(), f2[3].data_ptr(), f2[4].data_ptr(),
                                            f2[5].data_ptr(), out.data_ptr(), 40, n, H, W, _stream()))
    torch.cuda.synchronize()
    assert (out[..., 32:].float() == 512.0).all()
    _expect("frontend2", [n, H, W, u8], out[..., :32].float().permute(0, 3, 1, 2).cpu(), ref, BF16, E.FRONT_QUANTUM, t0)
