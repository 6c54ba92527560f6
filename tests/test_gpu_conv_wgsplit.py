"""m3d_conv_wave_forward_wgsplit: the K split of the wave-granular convolution inside the workgroup (csrc/dcn_wave.hip,
conv_wave_kernel<.., S>): S = 2 / 4 / 8 waves own one 32-pixel tile, each runs one K slice of the plan, the partial sums are added
in slice order through LDS and the epilogue is applied in the same launch.  No workspace.

Shapes: M = 1 x 9 x 11 = 99 pixels (tiles of 32, 32, 32 and 3), so every case has a partial pixel tile and more than one
workgroup; the channel counts make the plan (4 tiles -> as many slices as leave 4 steps each, at most 8) yield every width and
every uneven last slice:
    3x3 x Cin  32:  9 steps -> 2 slices (5 + 4)          3x3 x Cin 64: 18 steps -> 4 slices (5 + 5 + 5 + 3)
    3x3 x Cin 128: 36 steps -> 8 slices (7 x 5 + 1)      1x1 x Cin 256: 8 steps -> 2 slices (4 + 4)
    1x1 x Cin 384: 12 steps -> 3 slices, run by a 4-wave workgroup whose last wave has no steps.
Cout 128 / 64 / 27 (-> 32) = four, two and one column tile per wave; Cout 100 and 27 end inside a 4-channel group.
Checks per case: the fp64 reference at the bound this kernel is held to in tests/test_gpu_dcn.py (_relerr < 2e-4); BIT equality
with the workspace form of m3d_conv_wave_forward on the same descriptor (same slices, same order, same epilogue function); two
runs bit-equal; nothing written past Cout."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from m3dssd_amd import _hip, synth
from gpu_common import _dev, _relerr

pytestmark = pytest.mark.gpu

H, W = 9, 11
# name: (Cin, Cout, k, stride, deform, res_mode (None: no residual), act, sigmoid_from, out_cs - Cout)
CASES = {
    "deform_c32_co128_s2": (32, 128, 3, 1, 1, 0, 1, -1, 0),
    "deform_c32_co64_s2_nores": (32, 64, 3, 1, 1, None, 1, -1, 0),
    "deform_c64_co128_s4_resmode1": (64, 128, 3, 1, 1, 1, 1, -1, 0),
    "deform_c64_co64_s4_sigmoid3": (64, 64, 3, 1, 1, 0, 1, 3, 0),
    "deform_c64_co100_s4_channel_tail": (64, 100, 3, 1, 1, 0, 1, -1, 0),
    "deform_c128_co128_s8_nores_noact": (128, 128, 3, 1, 1, None, 0, -1, 0),
    "deform_c128_co64_s8_4byte_view": (128, 64, 3, 1, 1, 0, 1, -1, 1),       # out_cs 65: no 16-byte access
    "plain_1x1_c256_co128_s2_resmode1": (256, 128, 1, 1, 0, 1, 1, -1, 0),
    "plain_3x3_stride2_c64_co128_s4": (64, 128, 3, 2, 0, 0, 1, -1, 0),
    "plain_1x1_c384_co64_3slices_on_4waves": (384, 64, 1, 1, 0, 0, 1, -1, 4),
    # the offset / mask conv of a DCNv2 layer: Cout 27 -> one 32-channel column tile per wave, sigmoid on the 9 mask channels
    "plain_3x3_c64_co27_s4_one_column_tile": (64, 27, 3, 1, 0, None, 0, 18, 1),
    "plain_3x3_c128_co27_s8_one_column_tile_4byte_view": (128, 27, 3, 1, 0, None, 0, 18, 0),
}


# what the plan makes of each case: (K slices, waves per workgroup), pinned through m3d_conv_wave_wgsplit_width so that a change of
# the plan's rule cannot quietly leave a width of the kernel untested
PLAN = {
    "deform_c32_co128_s2": (2, 2), "deform_c32_co64_s2_nores": (2, 2), "deform_c64_co128_s4_resmode1": (4, 4),
    "deform_c64_co64_s4_sigmoid3": (4, 4), "deform_c64_co100_s4_channel_tail": (4, 4), "deform_c128_co128_s8_nores_noact": (8, 8),
    "deform_c128_co64_s8_4byte_view": (8, 8), "plain_1x1_c256_co128_s2_resmode1": (2, 2), "plain_3x3_stride2_c64_co128_s4": (4, 4),
    "plain_1x1_c384_co64_3slices_on_4waves": (3, 4), "plain_3x3_c64_co27_s4_one_column_tile": (4, 4),
    "plain_3x3_c128_co27_s8_one_column_tile_4byte_view": (8, 8),
}


def _width(d):
    slices, width = ctypes.c_int(), ctypes.c_int()
    _hip.check(_hip.lib().m3d_conv_wave_wgsplit_width(ctypes.byref(d), ctypes.byref(slices), ctypes.byref(width)))
    return slices.value, width.value


def _case(name, case=None):
    """Descriptor + fp64 reference of one case (CASES[name], or the tuple given).  Returns (desc, out tensor, want [M, Cout]
    float64, Cout, out_cs, keep-alive)."""
    from m3dssd_amd.engine import pack_frag
    from m3dssd_amd.host import standalone as S
    from oracle import dcn as odcn
    ci, co, k, stride, deform, res_mode, act, sig, cs_extra = CASES[name] if case is None else case
    dev = _dev()
    pad = k // 2
    hi, wi = (H * stride, W * stride) if stride > 1 else (H, W)
    g = torch.Generator().manual_seed(1000 + sum(ord(c) for c in name))
    x = torch.randn(1, ci, hi, wi, generator=g)
    assert ((hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1) == (H, W)
    wt = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    scale = torch.rand(co, generator=g) + 0.5
    shift = torch.randn(co, generator=g)
    res = torch.randn(1, co, H, W, generator=g)
    if deform:
        off = torch.randn(1, 2 * k * k, H, W, generator=g) * 1.5
        msk = torch.sigmoid(torch.randn(1, k * k, H, W, generator=g))
        acc = odcn.dcn_v2_forward(x, off, msk, wt, torch.zeros(co), stride, pad, 1, 1).double()
    else:
        acc = F.conv2d(x.double(), wt.double(), stride=stride, padding=pad)
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    if res_mode is None:
        want = acc * sc + sh
    elif res_mode == 1:
        want = (acc + res.double()) * sc + sh
    else:
        want = acc * sc + sh + res.double()
    lk = torch.where(want > 0, want, want * 0.01) if act == 1 else want
    if sig >= 0:
        lk = torch.cat([lk[:, :sig], torch.sigmoid(want[:, sig:])], 1)
    want = lk.permute(0, 2, 3, 1).reshape(H * W, co)

    cpt = 32 if co <= 32 else (64 if co <= 64 else 128)
    v, _ = S._to_nhwc(x.to(dev), ci)
    wp, _co, cop, kh, kw = S._pack(wt.to(dev), ci, cpt)
    frag = pack_frag(wp.view(cop, kh * kw * ci), cop, dev)
    scd, shd = scale.to(dev), shift.to(dev)
    rv, _ = S._to_nhwc(res.to(dev))
    out_cs = co + cs_extra
    out = torch.empty(H * W * out_cs, device=dev)
    keep = [v, frag, scd, shd, rv, out]
    d = _hip.ConvDesc()
    d.inp, d.in_cs, d.N, d.H, d.W, d.Cin = v.ptr, v.cs, 1, hi, wi, ci
    d.wgt, d.Cout, d.Cout_pad = frag.data_ptr(), co, cop
    d.kh, d.kw, d.stride, d.pad, d.dil, d.Ho, d.Wo = k, k, stride, pad, 1, H, W
    d.out, d.out_cs, d.scale, d.shift = out.data_ptr(), out_cs, scd.data_ptr(), shd.data_ptr()
    if res_mode is not None:
        d.res, d.res_cs, d.res_mode = rv.ptr, rv.cs, res_mode
    d.act, d.sigmoid_from = act, sig
    if deform:
        om, _ = S._to_nhwc(torch.cat([off, msk], 1).to(dev))
        d.dcn_offmask, d.dcn_om_cs = om.ptr, om.cs
        keep.append(om)
    return d, out, want, co, out_cs, keep


def _run(fn, d, out):
    from m3dssd_amd.host import standalone as S
    out.fill_(-777.0)
    _hip.check(fn(ctypes.byref(d), S._stream()))
    torch.cuda.synchronize()
    return out.clone()


@pytest.mark.parametrize("name", sorted(CASES))
def test_wgsplit_matches_reference_and_workspace_form_bit_for_bit(name):
    L = _hip.lib()
    d, out, want, co, out_cs, keep = _case(name)
    assert not d.splitk_ws                                   # no workspace: the entry point needs none
    assert _width(d) == PLAN[name]
    a = _run(L.m3d_conv_wave_forward_wgsplit, d, out)
    b = _run(L.m3d_conv_wave_forward_wgsplit, d, out)
    assert torch.equal(a, b)
    got = a.view(H * W, out_cs)
    assert (got[:, co:] == -777.0).all()                     # nothing is written past Cout
    err = _relerr(got[:, :co].cpu().numpy(), want.numpy())
    print("%s: relerr vs fp64 = %.3e" % (name, err))
    assert err < 2e-4
    if d.Cout_pad % 64:
        # one column tile per wave: this entry point only (no unsplit-by-default and no workspace form to compare with)
        assert L.m3d_conv_wave_forward(ctypes.byref(d), None) != 0 and b"Cout_pad" in L.m3d_last_error()
        return
    unsplit = _run(L.m3d_conv_wave_forward, d, out)         # no workspace given: the plain, unsplit launch
    assert not torch.equal(a, unsplit), "the K split did not run (same bits as the unsplit sum order)"
    # the workspace form: global split + splitk_reduce_kernel, same slices, same order, same epilogue function
    ws = torch.empty(8 * H * W * d.Cout_pad, device=out.device)
    d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel() * 4
    ref = _run(L.m3d_conv_wave_forward, d, out)
    c = _run(L.m3d_conv_wave_forward_wgsplit, d, out)        # a workspace given is ignored
    d.splitk_ws, d.splitk_ws_bytes = None, 0
    ndiff = int((a.view(torch.int32) != ref.view(torch.int32)).sum())
    print("%s: words differing from the workspace form = %d, max |diff| = %.3e" % (name, ndiff, (a - ref).abs().max().item()))
    assert torch.equal(a.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(a, c)


def test_wgsplit_runs_an_unsplit_plan_unsplit():
    """1x1 x Cin 128 = 4 steps: the plan does not split (a slice has at least 4 steps); the entry point runs the layer as
    m3d_conv_wave_forward does without a workspace."""
    L = _hip.lib()
    d, out, want, co, out_cs, keep = _case("plain_1x1_c128_unsplit", (128, 128, 1, 1, 0, 0, 1, -1, 0))
    assert _width(d) == (1, 1)
    a = _run(L.m3d_conv_wave_forward_wgsplit, d, out)
    b = _run(L.m3d_conv_wave_forward, d, out)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert _relerr(a.view(H * W, out_cs)[:, :co].cpu().numpy(), want.numpy()) < 2e-4
    assert L.m3d_conv_wave_forward_wgsplit(None, None) != 0 and b"null" in L.m3d_last_error()


def test_unsplit_epilogue_channel_tail_on_a_16_byte_view():
    """Cout 102 on a view with out_cs 104: the 16-byte epilogue of the unsplit kernel ends inside a 4-channel group (channels
    100, 101 go out as 4-byte stores of single vector elements, 102 and 103 are not written); deformable and plain."""
    L = _hip.lib()
    for deform in (1, 0):
        d, out, want, co, out_cs, keep = _case("unsplit_co102_deform%d" % deform, (64, 102, 3, 1, deform, 0, 1, -1, 2))
        got = _run(L.m3d_conv_wave_forward, d, out).view(H * W, out_cs)
        assert (got[:, co:] == -777.0).all()
        assert _relerr(got[:, :co].cpu().numpy(), want.numpy()) < 2e-4


def test_plan_reports_the_split_of_the_benched_layers():
    """m3d_conv_wave_splitk_plan (fill threshold enforced) on the descriptors of the benched bs-8 plan, no launch: a 256 -> 128
    3x3 DCNv2 at 24x80 and its 27 -> 32 channel offset / mask conv both split 4 ways; the latter has no workspace form."""
    L = _hip.lib()
    for cout, cop, deform, want_bytes in ((128, 128, 1, 4 * 8 * 24 * 80 * 128 * 4), (27, 32, 0, 0)):
        d = _hip.ConvDesc()
        d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout, d.Cout_pad = 8, 24, 80, 256, 24, 80, cout, cop
        d.kh, d.kw, d.stride, d.pad, d.dil = 3, 3, 1, 1, 1
        if deform:
            d.dcn_offmask, d.dcn_om_cs = 16, 32              # (only "deformable or not" is read by the plan)
        splits, nbytes = ctypes.c_int(), ctypes.c_longlong()
        _hip.check(L.m3d_conv_wave_splitk_plan(ctypes.byref(d), ctypes.byref(splits), ctypes.byref(nbytes)))
        assert (splits.value, nbytes.value) == (4, want_bytes)
        assert _width(d) == (4, 4)


def test_bench_plan_has_no_global_split_on_the_wave_kernel():
    """bs 8, 1280x384 (the benched plan): the eight thin wave-kernel layers and the four 27-channel offset / mask convs of the
    24x80 maps carry the in-workgroup split, none a workspace split, and the split-K reduce launches left per forward are the
    three F(4x4) layers and the 12x40 offset / mask conv, which measured slower on the wave kernel and stays on the igemm
    (DESIGN.md section 3)."""
    from model.M3d_inference_align import build
    B, crop = 8, (384, 1280)
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0), strict=True)
    net = net.to(_dev())
    with torch.no_grad():
        net(synth.synth_frames(B, crop, 1234).to(_dev()))
    torch.cuda.synchronize()
    kinds = [op[1] for op in net.engine().plan_for(B, *crop).ops]
    wave = [k for k in kinds if k.startswith("conv_wave")]
    assert not [k for k in wave if "splitk" in k], wave
    wg = [k for k in wave if "wgsplit" in k]
    assert {"conv_wave<deform,wgsplit8>", "conv_wave<deform,wgsplit4>", "conv_wave<deform,wgsplit2>"} <= set(wg), wave
    names = [op[0] for op in net.engine().plan_for(B, *crop).ops if "wgsplit" in op[1]]
    assert len(wg) == 12 and sum(n.endswith(".offset_mask") for n in names) == 4, list(zip(names, wg))
    reduce_launches = [k for k in kinds if "splitk" in k]
    assert sorted(k.split("<")[0] for k in reduce_launches) == ["igemm", "wino44", "wino44", "wino44"], reduce_launches
