"""The fp32 convolution kernels bit for bit on exact-arithmetic inputs (tests/conv_exact.py: operands, float64 reference of the
contract of include/m3dssd_hip.h, the case matrix; tests/test_conv_exact_host.py: the proof that no step rounds on them).

Every case makes its launches through the C ABI and compares with torch.equal: the implicit GEMM in all NHWC, deformable and
planar tiles, its split-K and per-image-weight forms; what tests/test_gpu_conv_wgsplit.py lacks of the wave kernel (dilation,
per-image weights); the three forms of Winograd F(2x2,3x3); the plain, K-pair and split-K forms of F(4x4,3x3) at nb 1 / 2; the
level0 pair.  The views are wider than the channel counts: the pad lanes of input and residual hold a sentinel the kernel must
ignore, the output is pre-filled with a sentinel in every word, one guard row after the last pixel (planar: the neighbouring
planes and image slots) included, and every word outside [pixel < M][c < Cout] must still hold it afterwards.  No case assumes
a route: the form is asserted first through the library's own queries (`expect` of the case: the PLAN pins), so a moved
threshold fails here instead of leaving a form untested.  Sigmoid channels go through expf and keep the project's tolerance."""
import ctypes

import pytest
import torch

import conv_exact as X
import exact_inputs as E
from m3dssd_amd import _hip
from gpu_common import _dev, _log, _relerr, _stream

pytestmark = pytest.mark.gpu
WS_SENT = 4099.3          # every word of a split-K workspace before the launch: on no lattice, so a written word differs from it


def _ref(c):
    return X.conv_contract_ref(c)


def _build(c, ops, dev):
    """The descriptor of case `c` on device buffers.  -> (desc, output buffer, keep-alive list)."""
    n, ci, co, hw = c["n"], c["cin"], c["cout"], c["ho"] * c["wo"]
    xin = X.nhwc_view(ops["x"], ci + c["in_x"], X.SENT_IN).to(dev)
    wgt, img_stride = X.packed_weight(c, ops["weight"], dev)
    buf, out_off = X.output_buffer(c)
    buf = buf.to(dev)
    keep = [xin, wgt, buf]
    d = _hip.ConvDesc()
    d.inp, d.in_cs, d.N, d.H, d.W, d.Cin = xin.data_ptr(), ci + c["in_x"], n, c["h"], c["w"], ci
    d.wgt, d.Cout, d.Cout_pad = wgt.data_ptr(), co, c["cout_pad"]
    if c["per_image"]:
        d.wgt_img_stride = img_stride
    d.kh, d.kw, d.stride, d.pad, d.dil, d.Ho, d.Wo = c["k"], c["k"], c["stride"], c["pad"], c["dil"], c["ho"], c["wo"]
    d.out = buf.data_ptr() + 4 * out_off
    if c["planar"]:
        d.out_nchw, d.out_img_stride = 1, 3 * (co + 1) * hw
    else:
        d.out_cs = co + c["out_x"]
    for key in ("scale", "shift"):
        if ops[key] is not None:
            t = ops[key].to(dev)
            keep.append(t)
            setattr(d, key, t.data_ptr())
    if ops["res"] is not None:
        r = X.nhwc_view(ops["res"], co + c["res_x"], X.SENT_IN).to(dev)
        keep.append(r)
        d.res, d.res_cs, d.res_mode = r.data_ptr(), co + c["res_x"], c["res_mode"]
    d.act, d.sigmoid_from = c["act"], c["sig"]
    if c["deform"]:
        om = E.pack_om(dict(off=ops["off"], mask=ops["mask"]), 32).to(dev)
        keep.append(om)
        d.dcn_offmask, d.dcn_om_cs = om.data_ptr(), 32
    return d, buf, keep


def _launch(fn, d, buf, *args):
    buf.fill_(X.SENT_OUT)
    _hip.check(fn(ctypes.byref(d), *args, _stream()))
    torch.cuda.synchronize()
    return buf.cpu()


def _refused(fn, d, *args):
    rc = fn(ctypes.byref(d), *args, _stream())
    torch.cuda.synchronize()
    return (rc != 0), _hip.lib().m3d_last_error()


def _check(c, ref, out_cpu, what):
    """torch.equal on the exactly computed channels, the project's bound on the sigmoid channels, the sentinels."""
    got, guards_ok = X.split_output(c, out_cpu)
    ne = c["sig"] if c["sig"] >= 0 else c["cout"]
    nd, msg = E.compare_exact(got[:, :ne], ref["out"][:, :ne].to(X.F64), torch.float32, 1.0 / 256)
    sig_err = _relerr(got[:, ne:].numpy(), ref["out"][:, ne:].numpy()) if ne < c["cout"] else 0.0
    print("%s %s: %d of %d elements differ, sigmoid relerr %.2e, sentinels %s" % (c["name"], what, nd, got[:, :ne].numel(), sig_err,
                                                                                "intact" if guards_ok else "OVERWRITTEN"))
    _log("exact_conv_" + c["family"], dict(case=c["name"], form=what, differing=nd, sigmoid_relerr=sig_err, sentinels=guards_ok))
    assert nd == 0, "%s %s: %s" % (c["name"], what, msg)
    assert sig_err < 2e-4
    assert guards_ok, "%s %s: a word outside [pixel < M][c < Cout] was written" % (c["name"], what)
    return got


def _tile(d):
    t = [ctypes.c_int() for _ in range(4)]
    _hip.check(_hip.lib().m3d_conv2d_tile(ctypes.byref(d), *[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t[:3])


def _plan(fn, d):
    splits, nbytes = ctypes.c_int(), ctypes.c_longlong()
    _hip.check(fn(ctypes.byref(d), ctypes.byref(splits), ctypes.byref(nbytes)))
    return splits.value, nbytes.value


def _workspace(d, nbytes, dev, keep):
    ws = torch.full((max(nbytes // 4, 4),), WS_SENT, device=dev)
    keep.append(ws)
    d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel() * 4


# ------------------------------------------------------------------------------------ implicit GEMM
@pytest.mark.parametrize("c", X.IGEMM + X.IGEMM_DEFORM + X.IGEMM_PLANAR + X.IGEMM_PER_IMAGE,
                         ids=X.ids(X.IGEMM + X.IGEMM_DEFORM + X.IGEMM_PLANAR + X.IGEMM_PER_IMAGE))
def test_igemm_tile_is_exact(c):
    L = _hip.lib()
    ref = _ref(c)
    d, buf, keep = _build(c, ref["ops"], _dev())
    assert _tile(d) == c["expect"]
    _check(c, ref, _launch(L.m3d_conv2d_forward, d, buf), "tile%s" % (c["expect"],))


@pytest.mark.parametrize("c", X.IGEMM_SPLITK, ids=X.ids(X.IGEMM_SPLITK))
def test_igemm_splitk_is_exact_and_bit_equal_to_the_unsplit_launch(c):
    L = _hip.lib()
    ref = _ref(c)
    d, buf, keep = _build(c, ref["ops"], _dev())
    splits, nbytes = _plan(L.m3d_conv2d_splitk_plan, d)
    assert _tile(d) + (splits,) == c["expect"] and nbytes == splits * c["n"] * c["ho"] * c["wo"] * c["cout_pad"] * 4
    unsplit = _check(c, ref, _launch(L.m3d_conv2d_forward, d, buf), "unsplit")
    _workspace(d, nbytes, _dev(), keep)
    split = _check(c, ref, _launch(L.m3d_conv2d_forward, d, buf), "split%d" % splits)
    assert torch.equal(split.contiguous().view(torch.int32), unsplit.contiguous().view(torch.int32))


@pytest.mark.parametrize("c", X.IGEMM_PER_IMAGE_REFUSED, ids=X.ids(X.IGEMM_PER_IMAGE_REFUSED))
def test_igemm_per_image_weights_on_a_map_the_tiles_cannot_split_are_refused(c):
    L = _hip.lib()
    d, buf, keep = _build(c, X.operands(c), _dev())
    bad, msg = _refused(L.m3d_conv2d_forward, d)
    assert bad and b"per-image weights" in msg
    assert (buf.cpu() == X.SENT_OUT).all()
    t = [ctypes.c_int() for _ in range(4)]
    assert L.m3d_conv2d_tile(ctypes.byref(d), *[ctypes.byref(v) for v in t]) != 0 and b"per-image weights" in L.m3d_last_error()


def test_igemm_planar_output_with_a_residual_is_refused():
    L = _hip.lib()
    c = dict(X.IGEMM_PLANAR[1], res_mode=0)
    d, buf, keep = _build(c, X.operands(c), _dev())
    bad, msg = _refused(L.m3d_conv2d_forward, d)
    assert bad and b"residual" in msg
    assert (buf.cpu() == X.SENT_OUT).all()


# ------------------------------------------------------------------------------------ wave kernel
def _wave_width(d):
    slices, width = ctypes.c_int(), ctypes.c_int()
    _hip.check(_hip.lib().m3d_conv_wave_wgsplit_width(ctypes.byref(d), ctypes.byref(slices), ctypes.byref(width)))
    return slices.value, width.value


@pytest.mark.parametrize("c", X.WAVE, ids=X.ids(X.WAVE))
def test_wave_kernel_dilation_and_per_image_weights_are_exact(c):
    L = _hip.lib()
    ref = _ref(c)
    d, buf, keep = _build(c, ref["ops"], _dev())
    assert _wave_width(d) == c["expect"]
    plan = _plan(L.m3d_conv_wave_splitk_plan, d)
    _log("exact_conv_wave_plan", dict(case=c["name"], wgsplit_width=list(c["expect"]), splitk_plan=list(plan)))
    if c["entry"] == "wgsplit":
        _check(c, ref, _launch(L.m3d_conv_wave_forward_wgsplit, d, buf), "wgsplit%d" % c["expect"][0])
        return
    got = _check(c, ref, _launch(L.m3d_conv_wave_forward, d, buf), "unsplit")
    if c["entry"] == "workspace":
        slices = c["expect"][0]
        _workspace(d, slices * c["n"] * c["ho"] * c["wo"] * c["cout_pad"] * 4, _dev(), keep)
        split = _check(c, ref, _launch(L.m3d_conv_wave_forward, d, buf), "workspace%d" % slices)
        assert torch.equal(split, got)
        d.splitk_ws, d.splitk_ws_bytes = None, 0
        _check(c, ref, _launch(L.m3d_conv_wave_forward_wgsplit, d, buf), "wgsplit%d" % slices)


@pytest.mark.parametrize("c", X.WAVE_REFUSED, ids=X.ids(X.WAVE_REFUSED))
def test_wave_kernel_refuses_per_image_weights_on_a_map_of_99_pixels(c):
    L = _hip.lib()
    d, buf, keep = _build(c, X.operands(c), _dev())
    for fn in (L.m3d_conv_wave_forward, L.m3d_conv_wave_forward_wgsplit):
        bad, msg = _refused(fn, d)
        assert bad and b"per-image weights" in msg
    assert (buf.cpu() == X.SENT_OUT).all()


# ------------------------------------------------------------------------------------ Winograd F(2x2,3x3)
@pytest.mark.parametrize("c", X.W22, ids=X.ids(X.W22))
def test_winograd_f2x2_forms_are_exact(c):
    L = _hip.lib()
    dev = _dev()
    ref = _ref(c)
    d, buf, keep = _build(c, ref["ops"], dev)
    assert L.m3d_wino_conv3x3_variant(ctypes.byref(d)) == 0                   # thin layers: the LDS kernel is the automatic choice
    recommended = _plan(L.m3d_wino_conv3x3_splitk_plan, d)
    _log("exact_conv_w22_plan", dict(case=c["name"], recommended=list(recommended)))
    outs = {}
    for form in c["forms"]:
        if form == "wave_refused":
            bad, msg = _refused(L.m3d_wino_conv3x3_forward_ex, d, 1)
            assert bad and b"sigmoid" in msg
            continue
        if form == "wave_ws":
            # the plan query answers with the RECOMMENDED split (1 by default: the split form measured slower); a caller that forces
            # the wave kernel with a workspace gets the slices the plan computes, `expect` of them.  That the split form ran is
            # shown by the workspace: slice s writes [s][M][Cout_pad], so exactly expect * M * Cout_pad words lose their sentinel.
            words = c["n"] * c["h"] * c["w"] * c["cout_pad"]
            _workspace(d, 4 * words * 4, dev, keep)
            ws = keep[-1]
            outs[form] = _check(c, ref, _launch(L.m3d_wino_conv3x3_forward_ex, d, buf, 1), form)
            written = (ws.cpu() != WS_SENT).view(4, words)
            assert [bool(written[s].all()) for s in range(4)] == [s < c["expect"] for s in range(4)] and not written[c["expect"]:].any()
            d.splitk_ws, d.splitk_ws_bytes = None, 0
            continue
        outs[form] = _check(c, ref, _launch(L.m3d_wino_conv3x3_forward_ex, d, buf, {"lds": 0, "wave": 1}[form]), form)
    assert all(torch.equal(v, outs["lds"]) for v in outs.values()) or c["sig"] >= 0


# ------------------------------------------------------------------------------------ Winograd F(4x4,3x3)
@pytest.mark.parametrize("c", X.W44, ids=X.ids(X.W44))
def test_winograd_f4x4_forms_are_exact(c):
    L = _hip.lib()
    dev = _dev()
    ref = _ref(c)
    d, buf, keep = _build(c, ref["ops"], dev)
    assert L.m3d_wino44_applicable(ctypes.byref(d)) == 1
    splits, nbytes = _plan(L.m3d_wino44_splitk_plan, d)
    assert (L.m3d_wino44_kpair(ctypes.byref(d)), splits) == c["expect"]
    outs = []
    for form in c["forms"]:
        if form == "split":
            assert splits > 1 and nbytes == splits * c["n"] * c["h"] * c["w"] * c["cout_pad"] * 4
            _workspace(d, nbytes, dev, keep)
            outs.append(_check(c, ref, _launch(L.m3d_wino44_conv3x3_forward, d, buf), "split%d" % splits))
            assert (keep[-1].cpu() != WS_SENT).all()                        # every slice wrote its partial sums: the split form ran
            d.splitk_ws, d.splitk_ws_bytes = None, 0
            outs.append(_check(c, ref, _launch(L.m3d_wino44_conv3x3_forward_ex, d, buf, 1), "unsplit_nb1"))
        elif form == "touch":
            wgt = keep[1]
            outs.append(_check(c, ref, _launch(L.m3d_wino44_conv3x3_forward_touch, d, buf, 1, ctypes.c_void_p(wgt.data_ptr()),
                                               ctypes.c_longlong(wgt.numel() * 4)), "touch_nb1"))
        else:
            nb = int(form[2])
            what = "kpair" if nb == 1 and c["expect"][0] else form
            outs.append(_check(c, ref, _launch(L.m3d_wino44_conv3x3_forward_ex, d, buf, nb), what))
    assert all(torch.equal(v, outs[0]) for v in outs)


# ------------------------------------------------------------------------------------ level0 pair
@pytest.mark.parametrize("c", X.LEVEL0, ids=X.ids(X.LEVEL0))
def test_level0_pair_is_exact(c):
    L = _hip.lib()
    dev = _dev()
    ref = _ref(c)
    ops = ref["ops"]
    xin = X.nhwc_view(ops["x"], 20, X.SENT_IN).to(dev)
    (u44, wdir), _ = X.packed_weight(c, ops["weight"], dev)
    sc, sh = ops["scale"].to(dev), ops["shift"].to(dev)
    buf = X.output_buffer(c)[0].to(dev)
    for what, fn, wgt in (("c16_wino", L.m3d_conv3x3_c16_wino, u44), ("c16", L.m3d_conv3x3_c16, wdir)):
        buf.fill_(X.SENT_OUT)
        _hip.check(fn(xin.data_ptr(), 20, wgt.data_ptr(), sc.data_ptr(), sh.data_ptr(), buf.data_ptr(), 20, c["n"], c["h"], c["w"], _stream()))
        torch.cuda.synchronize()
        _check(c, ref, buf.cpu(), what)
