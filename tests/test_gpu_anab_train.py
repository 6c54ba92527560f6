"""The ANAB attention core for training on the device: m3d_anab_attention_forward / _backward against the float64 composition of
tests/anab_train_ref.py, reproducibility, NULL gradients, and the differentiable ANAB / shape_align / center_align modules.

Bound of the comparisons: per tensor err = max|got - ref64| / max|ref64|, and err_op <= 4 * err_torch32 + 2^-20, where
err_torch32 is the error of the float32 torch composition computed in the same test on the device: both are float32 evaluations
of the same sums in different orders (on the CPU two such orders differed by at most 1.9x on the operator cases, errors 0.4e-6 to
2.6e-6); a dropped bin or a wrong term shows at 1e-3 and above.

The operator cases also cover B > 1 together with several 512-pixel chunks of the key-major kernel, the nested pooling at Ck = 168,
Cv = 256 with several images, maps narrower than 16, rows whose logits pass ln(FLT_MAX), each image alone against the batch (bit
for bit), a canary behind the workspace, and the autograd layer with the grad_out layouts autograd produces (measured margins:
docs/LAB_NOTES.md section 15)."""
import functools

import pytest
import torch

from gpu_common import _dev, _log, _stream
from m3dssd_amd import _hip

import anab_train_ref as R
import poison

pytestmark = pytest.mark.gpu

# (B, H, W, Ck, Cv)
CASES = [(2, 8, 16, 168, 128),      # H < 16: two bins per pixel at scale 16
         (1, 16, 16, 64, 128),      # nested windows
         (1, 12, 32, 128, 128),     # uneven windows
         (1, 4, 32, 168, 128),      # H below two scales
         (1, 16, 40, 168, 128),     # the 128x320 map
         (1, 8, 16, 168, 256),      # value-channel split
         # batch x pixel chunks of the key-major kernel (512 pixels per chunk: partial row (img * nch + ch) * 352 + key) and narrow maps
         (2, 16, 72, 168, 128),     # 6: HW 1152 = 36 tiles, nch = 3 with a ragged last chunk of 4 tiles; windows overlap along x
         (2, 32, 48, 168, 128),     # 7: nested windows at Ck = 168 (the branch of the 48x160 training map), nch = 3, full chunks
         (2, 16, 40, 168, 256),     # 8: value-channel split with B = 2, nch = 2
         (3, 16, 40, 128, 128),     # 9: Ck = 128 with B = 3, nch = 2
         (1, 32, 4, 168, 128),      # 10: W < 8: 2 bins along x at scale 8, 4 at scale 16
         (1, 16, 8, 64, 128),       # 11: W = 8 < 16
         (1, 128, 1, 168, 128),     # 12: W = 1: a pixel lies in all 16 x-bins of scale 16
         (2, 64, 2, 168, 128)]      # 13: B = 2 on a narrow map
NEW0 = 6                            # the cases from here on are seeded 200 + (i - NEW0), the ones in front 100 + i
IDS = ["%dx%dx%d_ck%d_cv%d" % c for c in CASES]
PEAKED = [NEW0, NEW0 + 1, NEW0 + 2, NEW0 + 4]           # run again with every 37th row of q times 40 (logits past ln(FLT_MAX))
BATCHED = [NEW0, NEW0 + 1, NEW0 + 2]
LN_FLT_MAX = 88.73
GUARD = 7.25
CANARY = 4096                       # bytes behind the workspace size the library asks for, watched by every _run
NAMES = ("out", "grad_q", "grad_k", "grad_v", "grad_gates")


def _err(got, ref):
    return ((got.detach().double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max()).item()


def _bound(e32):
    return 4.0 * e32 + 2.0 ** -20


@functools.lru_cache(maxsize=None)
def _inputs(i, peaked=False):
    """The CPU inputs of case ``i`` (tests/anab_train_ref.py::make_core_case), ``peaked``: every 37th row of q times 40."""
    wide, views, gwide = R.make_core_case(*CASES[i], seed=100 + i if i < NEW0 else 200 + i - NEW0)
    if peaked:
        R.peak_rows_(wide, views, 37, 40.0)
    return wide, views, gwide


@functools.lru_cache(maxsize=None)
def _case(i, peaked=False):
    """Inputs on the device (slices of wider matrices), the float64 yardstick and the float32 torch composition's errors."""
    B, H, W, Ck, Cv = CASES[i]
    wide, views, gwide = _inputs(i, peaked)
    ts = [wide[:, o:o + c] for o, c in views]
    go = gwide[:, 4:4 + Cv]
    ref64 = R.core_grads(ts, go, B, H, W, torch.float64, "cpu")
    t32 = R.core_grads(ts, go, B, H, W, torch.float32, _dev())
    e32 = [_err(a, b) for a, b in zip(t32, ref64)]
    return wide.to(_dev()), views, gwide.to(_dev()), ref64, e32


@functools.lru_cache(maxsize=None)
def _canary():
    return (torch.arange(CANARY, device=_dev()) % 251).to(torch.uint8)


def _run(i, needs=(True, True, True, True), fill=None, forward=True, ws_fill=None, peaked=False, img=None):
    """The C ABI on strided views: outputs are slices (columns 4 .. 4 + C) of wider matrices pre-filled with GUARD (or poisoned with
    ``fill``), the workspace is poisoned with ``fill`` (or with ``ws_fill`` alone, which leaves the guard columns checkable).  Returns [out, grad_q, grad_k, grad_v, grad_gates] as the WIDE matrices.
    ``img``: that image of the batch alone (B = 1, every pointer moved to the image's rows).
    The workspace has exactly the size m3d_anab_attention_workspace_bytes gives; CANARY bytes behind it hold a pattern that must
    stand after the forward and after the backward."""
    B, H, W, Ck, Cv = CASES[i]
    wide, views, gwide, _, _ = _case(i, peaked)
    L, dev = _hip.lib(), _dev()
    row0 = 0
    if img is not None:
        assert 0 <= img < B
        row0, B = img * H * W, 1
    n = B * H * W
    cs = wide.stride(0)
    ptr = [wide.data_ptr() + 4 * (row0 * cs + o) for o, _ in views]
    go_ptr = gwide.data_ptr() + 4 * (row0 * gwide.stride(0) + 4)

    def fresh(c):
        t = torch.full((n, c + 8), GUARD, device=dev)
        if fill is not None:
            poison.poison_(t, fill)
        return t

    def workspace(backward):
        nbytes = L.m3d_anab_attention_workspace_bytes(B, H, W, Ck, Cv, backward)
        assert nbytes > 0
        ws = torch.zeros(nbytes + 256 + CANARY, device=dev, dtype=torch.uint8)
        if (fill or ws_fill) is not None:
            ws.fill_({"nan": 0xFF, "huge": 0x7F}[fill or ws_fill])        # (a byte tensor: the float pattern, not the small-integer one)
        base = (ws.data_ptr() + 255) // 256 * 256
        end = base - ws.data_ptr() + nbytes
        ws[end:end + CANARY] = _canary()
        return ws, base, nbytes, end

    def canary_stands(ws, end, what):
        assert torch.equal(ws[end:end + CANARY], _canary()), "%s wrote behind the workspace size it asks for" % what

    res = [None] * 5
    if forward:
        res[0] = fresh(Cv)
        ws, base, nbytes, end = workspace(0)
        _hip.check(L.m3d_anab_attention_forward(*ptr, res[0].data_ptr() + 16, B, H, W, Ck, Cv, cs, cs, cs, cs, res[0].stride(0), base,
                                                nbytes, _stream()))
        canary_stands(ws, end, "m3d_anab_attention_forward")
    for j, c in enumerate((Ck, Ck, Cv, 4)):
        if needs[j]:
            res[1 + j] = fresh(c)
    ws, base, nbytes, end = workspace(1)
    gp = [t.data_ptr() + 16 if t is not None else None for t in res[1:]]
    gcs = [t.stride(0) if t is not None else 0 for t in res[1:]]
    _hip.check(L.m3d_anab_attention_backward(*ptr, go_ptr, *gp, B, H, W, Ck, Cv, cs, cs, cs, cs, gwide.stride(0), *gcs,
                                             base, nbytes, _stream()))
    torch.cuda.synchronize()
    canary_stands(ws, end, "m3d_anab_attention_backward")
    return res


def _compare(tag, i, peaked):
    """Forward and backward of case ``i`` on a poisoned workspace against float64: guard columns, finite values, the bound."""
    _, _, _, ref64, e32 = _case(i, peaked)
    res = _run(i, ws_fill=("nan", "huge")[i % 2], peaked=peaked)
    errs = {}
    for name, wide_out, ref, e in zip(NAMES, res, ref64, e32):
        c = ref.shape[1]
        assert torch.equal(wide_out[:, :4], torch.full_like(wide_out[:, :4], GUARD)), name + ": guard columns in front were written"
        assert torch.equal(wide_out[:, 4 + c:], torch.full_like(wide_out[:, 4 + c:], GUARD)), name + ": guard columns behind were written"
        assert torch.isfinite(wide_out[:, 4:4 + c]).all(), name + " is not finite"
        errs[name] = (_err(wide_out[:, 4:4 + c], ref), e)
    print("anab_train " + tag, CASES[i], errs)
    _log("anab_train_" + tag, {"case": list(CASES[i]), "errs": {k: list(v) for k, v in errs.items()}})
    for name, (e_op, e) in errs.items():
        assert e_op <= _bound(e), "%s: err %.3e > 4 * %.3e + 2^-20" % (name, e_op, e)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_operator_matches_float64(i):
    _compare("operator", i, False)


@pytest.mark.parametrize("i", PEAKED, ids=[IDS[i] for i in PEAKED])
def test_operator_matches_float64_on_peaked_rows(i):
    """Every 37th row of q times 40: the largest logit of such a row passes ln(FLT_MAX), so the running maximum and the alpha rescale
    of the pixel-major kernel (and of m3d_anab_attend_f32 in the forward), and exp(s - m) recomputed by the key-major kernel from the
    stored statistics, carry the result.  Same bound as the mild cases: the float32 composition loses the same digits in dP - D."""
    B, H, W, Ck, Cv = CASES[i]
    wide, views, _ = _inputs(i, True)
    q, k, _, g = (wide[:, o:o + c].double() for o, c in views)
    top = R.anab_logits(q, k, g, B, H, W).amax(-1).flatten()
    nbig = int((top > LN_FLT_MAX).sum())
    print("anab_train peaked", CASES[i], "rows past ln(FLT_MAX):", nbig, "largest logit: %.1f" % top.max().item())
    assert nbig >= 4, "only %d rows have a logit above %.2f: the case tests nothing" % (nbig, LN_FLT_MAX)
    _compare("peaked", i, True)


@pytest.mark.parametrize("i", BATCHED, ids=[IDS[i] for i in BATCHED])
def test_batch_equals_its_images_bitwise(i):
    """Every sum's order depends only on the position inside the image, so an image run alone (B = 1, pointers at its rows) gives
    the bits the batch gives for it; a difference means a launch mixes images (a wrong image or chunk stride)."""
    B, H, W, Ck, Cv = CASES[i]
    hw = H * W
    full = _run(i, ws_fill="nan")
    for b in range(B):
        one = _run(i, ws_fill="huge", img=b)
        for name, wide_full, wide_one, c in zip(NAMES, full, one, (Cv, Ck, Ck, Cv, 4)):
            assert wide_one.shape == (hw, c + 8)
            assert torch.equal(wide_one[:, 4:4 + c], wide_full[b * hw:(b + 1) * hw, 4:4 + c]), "%s of image %d alone differs from the batch" % (name, b)


@pytest.mark.parametrize("i", [0, 4], ids=["8x16", "16x40"])
def test_backward_is_reproducible_on_poisoned_memory(i):
    first = None
    for rep in range(5):
        res = _run(i, fill=("nan", "huge")[rep % 2], forward=False)
        grads = [t[:, 4:4 + r.shape[1]].clone() for t, r in zip(res[1:], _case(i)[3][1:])]
        assert all(torch.isfinite(g).all() for g in grads)
        if first is None:
            first = grads
        else:
            for name, a, b in zip(NAMES[1:], first, grads):
                assert torch.equal(a, b), "%s differs between launch 0 and launch %d" % (name, rep)


def _single_gradient_calls(i):
    ref = _run(i, forward=False)
    for j in range(4):
        needs = tuple(k == j for k in range(4))
        res = _run(i, needs=needs, fill="nan", forward=False)
        c = _case(i)[3][1 + j].shape[1]
        assert torch.isfinite(ref[1 + j][:, 4:4 + c]).all(), NAMES[1 + j]
        assert torch.equal(res[1 + j][:, 4:4 + c], ref[1 + j][:, 4:4 + c]), NAMES[1 + j]


def test_single_gradient_calls_equal_the_full_call():
    _single_gradient_calls(0)


def test_single_gradient_calls_equal_the_full_call_on_the_split_value_path():
    _single_gradient_calls(NEW0 + 2)                 # Cv = 256: two value slices per key block, B = 2, nch = 2


# ------------------------------------------------------------------------------------ the autograd layer
AUTOGRAD_DIMS = (2, 16, 40, 168, 128)
# columns of the wide leaf: q at an odd float offset (not 16-byte aligned: ops copies it), k, v and gates at odd offsets too (taken
# as they are, with the leaf's row stride of 490 floats)
AUTOGRAD_VIEWS = ((3, 168), (177, 168), (351, 128), (483, 4))
AUTOGRAD_WIDTH = 490


@functools.lru_cache(maxsize=None)
def _autograd_leaf():
    B, H, W, Ck, Cv = AUTOGRAD_DIMS
    g = torch.Generator().manual_seed(300)
    n = B * H * W
    wide = torch.randn(n, AUTOGRAD_WIDTH, generator=g)                     # guard columns: ordinary numbers nobody may use
    for (o, c), scale in zip(AUTOGRAD_VIEWS, (0.3, 1.0, 1.0, 1.0)):
        wide[:, o:o + c] *= scale
    o, c = AUTOGRAD_VIEWS[3]
    wide[:, o:o + c] = torch.sigmoid(wide[:, o:o + c])
    return wide, torch.randn(n, Cv, generator=g), torch.randn(Cv, generator=g)


def _autograd_grads(fn, kind, dtype, device):
    """[out, grad of the wide leaf] of ``fn`` (ops.anab_attention or the composition) on column slices of one leaf, for one of the
    three forms of grad_out; also the strides of the grad_out that reached ``out``."""
    B, H, W, _, _ = AUTOGRAD_DIMS
    wide, go, vec = (t.to(device=device, dtype=dtype) for t in _autograd_leaf())
    wide.requires_grad_(True)
    out = fn(*(wide[:, o:o + c] for o, c in AUTOGRAD_VIEWS), B, H, W)
    seen = []
    out.register_hook(lambda t: seen.append(t.stride()))
    if kind == "contiguous":
        out.backward(go)
    elif kind == "sum0":
        out.sum(0).backward(vec)
    else:
        out.sum().backward()
    return [out.detach(), wide.grad], seen[0]


@pytest.mark.parametrize("kind,strides", [("contiguous", (128, 1)), ("sum0", (0, 1)), ("sum", (0, 0))], ids=["contiguous", "sum0", "sum"])
def test_autograd_layer_on_slices_of_one_leaf(kind, strides):
    """ops.anab_attention on column slices of one wide leaf (q unaligned and copied, k / v / gates as they are) with the three
    forms of grad_out autograd hands over: contiguous, (0, 1) behind .sum(0), (0, 0) behind .sum()."""
    from m3dssd_amd.host import ops
    got, seen = _autograd_grads(ops.anab_attention, kind, torch.float32, _dev())
    assert seen == strides, "grad_out arrived with strides %s" % (seen,)
    ref64, _ = _autograd_grads(R.anab_core, kind, torch.float64, "cpu")
    t32, _ = _autograd_grads(R.anab_core, kind, torch.float32, _dev())
    keep = torch.zeros(AUTOGRAD_WIDTH, dtype=torch.bool)
    for o, c in AUTOGRAD_VIEWS:
        keep[o:o + c] = True
    assert torch.equal(got[1][:, ~keep], torch.zeros_like(got[1][:, ~keep])), "the guard columns of the leaf got a gradient"
    pieces = lambda pair: [pair[0]] + [pair[1][:, o:o + c] for o, c in AUTOGRAD_VIEWS]
    errs = {}
    for name, a, r, t in zip(NAMES, pieces(got), pieces(ref64), pieces(t32)):
        assert torch.isfinite(a).all(), name
        errs[name] = (_err(a, r), _err(t, r))
    print("anab_train autograd", kind, errs)
    _log("anab_train_autograd", {"grad_out": kind, "errs": {k: list(v) for k, v in errs.items()}})
    for name, (e_op, e) in errs.items():
        assert e_op <= _bound(e), "%s: err %.3e > 4 * %.3e + 2^-20" % (name, e_op, e)


# ------------------------------------------------------------------------------------ the modules in training mode
def _grads_of(out, go, ts):
    return [out.detach()] + list(torch.autograd.grad(out, ts, go))


def _check(name, got, ref64, t32):
    errs = {}
    for n, g, r, t in zip(name, got, ref64, t32):
        errs[n] = (_err(g, r), _err(t, r))
    print("anab_train modules", errs)
    _log("anab_train_modules", {k: list(v) for k, v in errs.items()})
    for n, (e_op, e) in errs.items():
        assert e_op <= _bound(e), "%s: err %.3e > 4 * %.3e + 2^-20" % (n, e_op, e)


def test_anab_module_trains_and_eval_keeps_its_bits():
    from m3dssd_amd.host.attention import ANAB
    from m3dssd_amd.host.standalone import anab_forward
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    B, C, H, W = 2, 128, 8, 16
    mod = ANAB(C, 1)
    for p in mod.parameters():
        p.data = torch.randn(p.shape, generator=g) * 0.08
    mod = mod.to(dev).train()
    x = torch.randn(B, C, H, W, generator=g)
    go = torch.randn(B, C, H, W, generator=g)
    ws = [mod.query_conv.weight, mod.key_conv.weight, mod.value_conv.weight, mod.spatial_conv.weight]
    xd = x.to(dev).requires_grad_(True)
    out = mod(xd)
    assert out.shape == x.shape and out.is_contiguous() and out.grad_fn is not None
    got = _grads_of(out, go.to(dev), [xd] + ws)

    def compose(dtype, device):
        ts = [t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in [x] + ws]
        return _grads_of(R.anab_module(*ts), go.to(device=device, dtype=dtype), ts)

    _check(("out", "grad_x", "grad_wq", "grad_wk", "grad_wv", "grad_ws"), got, compose(torch.float64, "cpu"), compose(torch.float32, dev))
    # eval mode, and training mode without grad: the fused inference launches, the same bits
    want = anab_forward(mod, x.to(dev))
    assert torch.equal(mod.eval()(x.to(dev)), want)
    with torch.no_grad():
        assert torch.equal(mod.train()(x.to(dev)), want)
    assert (want - out.detach()).abs().max().item() <= 1e-4 * want.abs().max().item()


def _align_ref(kind, ind, x, prob, bx, by, w, b, mod, dtype, device):
    """The float composition of shape_align / center_align (feturealign_mgpu.py:48-99, 153-208, k = 1) with given top-1 indices."""
    cast = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype).requires_grad_(True)
    x, prob, bx, by, w, b = (cast(t) for t in (x, prob, bx, by, w, b))
    ind = ind.to(device)
    mask = torch.gather(prob, 1, ind)
    hard = (mask.detach().float() > mod.thresh).to(dtype)
    if kind == "shape":
        off = mod.offset_table.to(device=device, dtype=dtype)[ind[:, 0]].permute(0, 3, 1, 2) * hard
        kk, pad, ts = 9, 1, [x, w, b, prob]
    else:
        cv = lambda t: t.to(device=device, dtype=dtype)
        ox = torch.gather((bx * cv(mod.xy_std[0]) + cv(mod.xy_mean[0])) * cv(mod.anchors_w), 1, ind) * hard
        oy = torch.gather((by * cv(mod.xy_std[1]) + cv(mod.xy_mean[1])) * cv(mod.anchors_h), 1, ind) * hard
        off = torch.cat([oy, ox], 1)
        kk, pad, ts = 1, 0, [x, w, b, prob, bx, by]
    out = R.dcn_ref(x, off, mask.repeat(1, kk, 1, 1), w, b, 1, pad) + x
    return out, ts


@pytest.mark.parametrize("kind", ["shape", "center"])
def test_align_modules_train(kind):
    from m3dssd_amd import synth
    from m3dssd_amd.host import train
    from m3dssd_amd.host.align import center_align, shape_align
    dev = _dev()
    g = torch.Generator().manual_seed(21)
    B, C, H, W = 2, 32, 8, 16
    conf = synth.synth_conf((64, 128), 0, batch_size=B, device="cpu")
    anchors = torch.tensor(conf.anchors, dtype=torch.float)
    A = anchors.shape[0]
    if kind == "shape":
        mod = shape_align(C, anchors, feat_stride=8, feat_size=[H, W], kernel_size=3, k=1, thresh=0.5)
    else:
        mod = center_align(C, anchors, xy_mean=conf.bbox_means[0][0:2], xy_std=conf.bbox_stds[0][0:2], feat_stride=8,
                           feat_size=[H, W], kernel_size=1, k=1, thresh=0.5)
    mod.align.weight.data = torch.randn(mod.align.weight.shape, generator=g) / (C * mod.align.weight.shape[2] ** 2) ** 0.5
    mod.align.bias.data = torch.randn(C, generator=g) * 0.1
    mod = mod.to(dev).train()
    x = torch.randn(B, C, H, W, generator=g)
    prob = torch.rand(B, A, H, W, generator=g)                   # max over 36 anchors: above and below the 0.5 threshold both occur
    prob[:, :, :, : W // 2] *= 0.45
    bx, by = torch.randn(B, A, H, W, generator=g) * 0.5, torch.randn(B, A, H, W, generator=g) * 0.5
    go = torch.randn(B, C, H, W, generator=g)
    leaves = [t.to(dev).requires_grad_(True) for t in ((x, prob) if kind == "shape" else (x, prob, bx, by))]
    out = mod(leaves[0], leaves[1]) if kind == "shape" else mod(leaves[0], leaves[2], leaves[3], leaves[1])
    ts = [leaves[0], mod.align.weight, mod.align.bias] + leaves[1:]
    got = _grads_of(out, go.to(dev), ts)
    ind, mask = train._top1(leaves[1].detach())
    assert 0 < (mask > 0.5).sum().item() < mask.numel()
    refs = []
    for dtype, device in ((torch.float64, "cpu"), (torch.float32, dev)):
        o, rts = _align_ref(kind, ind, x, prob, bx, by, mod.align.weight, mod.align.bias, mod, dtype, device)
        refs.append(_grads_of(o, go.to(device=device, dtype=dtype), rts))
    names = ("out", "grad_x", "grad_weight", "grad_bias", "grad_prob") + (("grad_bbox_x", "grad_bbox_y") if kind == "center" else ())
    _check(names, got, refs[0], refs[1])


def test_public_operator_refusals_on_device_tensors():
    from m3dssd_amd.host import ops
    dev, n = _dev(), 128
    q, k, v, g = (torch.zeros(n, c, device=dev) for c in (168, 168, 128, 4))
    assert ops.anab_attention(q, k, v, g, 1, 8, 16).shape == (n, 128)
    with pytest.raises(RuntimeError, match="float32"):
        ops.anab_attention(q.double(), k.double(), v.double(), g.double(), 1, 8, 16)
    with pytest.raises(RuntimeError, match="float32"):
        ops.anab_attention(q, k, v.half(), g, 1, 8, 16)
    with pytest.raises(RuntimeError, match="HW % 128"):
        ops.anab_attention(q[:35], k[:35], v[:35], g[:35], 1, 5, 7)
    with pytest.raises(RuntimeError, match=r"\(Ck, Cv\)"):
        ops.anab_attention(q[:, :160], k[:, :160], v, g, 1, 8, 16)
    with pytest.raises(RuntimeError, match=r"\(Ck, Cv\)"):
        ops.anab_attention(q[:, :64], k[:, :64], torch.zeros(n, 256, device=dev), g, 1, 8, 16)
    with pytest.raises(RuntimeError):
        ops.anab_attention(q, k[:, :64], v, g, 1, 8, 16)
    with pytest.raises(NotImplementedError):
        ops.anab_attention(q.cpu(), k, v, g, 1, 8, 16)
    with torch.autocast("cuda", dtype=torch.bfloat16):           # autocast operands go back to float32
        out = ops.anab_attention(q.bfloat16(), k.bfloat16(), v.bfloat16(), g.bfloat16(), 1, 8, 16)
    assert out.dtype == torch.float32


def test_c_abi_refusals():
    """What the fp32 C ABI refuses, and with which code: a short workspace is M3D_E_WORKSPACE here (M3D_E_ARG in the bf16 entries,
    tests/test_gpu_anab_bf16.py), everything else M3D_E_ARG.  The workspace is 16 MiB: the fp32 operator asks for 7.4 / 8.3 MiB at this
    shape (the pooling scratch of a map whose windows do not nest), where the bf16 one stays below 2 MiB."""
    L, dev = _hip.lib(), _dev()
    E_ARG, E_WORKSPACE = -1, -3                                  # M3D_E_ARG, M3D_E_WORKSPACE
    t = torch.zeros(128, 512, device=dev)
    o = torch.zeros(128, 512, device=dev)
    size = 1 << 24
    ws = torch.zeros(2 * size, device=dev, dtype=torch.uint8)
    base = (ws.data_ptr() + 255) // 256 * 256
    p, po = t.data_ptr(), o.data_ptr()
    need = [L.m3d_anab_attention_workspace_bytes(1, 8, 16, 168, 128, b) for b in (0, 1)]
    assert 0 < need[0] < need[1] < size

    def fwd(Ck=168, Cv=128, H=8, W=16, nbytes=size, ws_ptr=base):
        return L.m3d_anab_attention_forward(p, p, p, p, po, 1, H, W, Ck, Cv, 512, 512, 512, 512, 512, ws_ptr, nbytes, _stream())

    def bwd(go=p, nbytes=size, go_cs=512):
        return L.m3d_anab_attention_backward(p, p, p, p, go, po, po, po, po, 1, 8, 16, 168, 128, 512, 512, 512, 512, go_cs, 512, 512, 512,
                                             512, base, nbytes, _stream())

    assert fwd() == 0 and bwd() == 0, L.m3d_last_error().decode()
    torch.cuda.synchronize()
    for code, word, call in ((E_ARG, "(Ck, Cv)", lambda: fwd(Ck=160)), (E_ARG, "(Ck, Cv)", lambda: fwd(Ck=64, Cv=256)),
                             (E_ARG, "HW % 128", lambda: fwd(H=5, W=7)),
                             (E_ARG, "256-byte aligned", lambda: fwd(ws_ptr=base + 16)),
                             (E_ARG, "16-byte aligned", lambda: bwd(go=p + 4)), (E_ARG, "16-byte aligned", lambda: bwd(go_cs=510)),
                             (E_WORKSPACE, "workspace", lambda: fwd(nbytes=need[0] - 1)),
                             (E_WORKSPACE, "workspace", lambda: bwd(nbytes=need[1] - 1))):
        assert call() == code, word
        assert word in L.m3d_last_error().decode(), (word, L.m3d_last_error().decode())
    assert L.m3d_anab_attention_workspace_bytes(1, 5, 7, 168, 128, 0) == -1
    torch.cuda.synchronize()
