"""The ANAB attention core for training on the device: m3d_anab_attention_forward / _backward against the float64 composition of
tests/anab_train_ref.py, reproducibility, NULL gradients, and the differentiable ANAB / shape_align / center_align modules.

Bound of the comparisons: per tensor err = max|got - ref64| / max|ref64|, and err_op <= 4 * err_torch32 + 2^-20, where
err_torch32 is the error of the float32 torch composition computed in the same test on the device: both are float32 evaluations
of the same sums in different orders (on the CPU two such orders differed by at most 1.9x on the operator cases, errors 0.4e-6 to
2.6e-6); a dropped bin or a wrong term shows at 1e-3 and above."""
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
         (1, 8, 16, 168, 256)]      # value-channel split
GUARD = 7.25
NAMES = ("out", "grad_q", "grad_k", "grad_v", "grad_gates")


def _err(got, ref):
    return ((got.detach().double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max()).item()


def _bound(e32):
    return 4.0 * e32 + 2.0 ** -20


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs on the device (slices of wider matrices), the float64 yardstick and the float32 torch composition's errors."""
    B, H, W, Ck, Cv = CASES[i]
    wide, views, gwide = R.make_core_case(B, H, W, Ck, Cv, seed=100 + i)
    ts = [wide[:, o:o + c] for o, c in views]
    go = gwide[:, 4:4 + Cv]
    ref64 = R.core_grads(ts, go, B, H, W, torch.float64, "cpu")
    t32 = R.core_grads(ts, go, B, H, W, torch.float32, _dev())
    e32 = [_err(a, b) for a, b in zip(t32, ref64)]
    return wide.to(_dev()), views, gwide.to(_dev()), ref64, e32


def _run(i, needs=(True, True, True, True), fill=None, forward=True, ws_fill=None):
    """The C ABI on strided views: outputs are slices (columns 4 .. 4 + C) of wider matrices pre-filled with GUARD (or poisoned with
    ``fill``), the workspace is poisoned with ``fill`` (or with ``ws_fill`` alone, which leaves the guard columns checkable).  Returns [out, grad_q, grad_k, grad_v, grad_gates] as the WIDE matrices."""
    B, H, W, Ck, Cv = CASES[i]
    wide, views, gwide, _, _ = _case(i)
    L, dev, n = _hip.lib(), _dev(), B * H * W
    ptr = [wide.data_ptr() + 4 * o for o, _ in views]
    cs = wide.stride(0)

    def fresh(c):
        t = torch.full((n, c + 8), GUARD, device=dev)
        if fill is not None:
            poison.poison_(t, fill)
        return t

    def workspace(backward):
        nbytes = L.m3d_anab_attention_workspace_bytes(B, H, W, Ck, Cv, backward)
        assert nbytes > 0
        ws = torch.zeros(nbytes + 256, device=dev, dtype=torch.uint8)
        if (fill or ws_fill) is not None:
            ws.fill_({"nan": 0xFF, "huge": 0x7F}[fill or ws_fill])        # (a byte tensor: the float pattern, not the small-integer one)
        return ws, (ws.data_ptr() + 255) // 256 * 256, nbytes

    res = [None] * 5
    if forward:
        res[0] = fresh(Cv)
        ws, base, nbytes = workspace(0)
        _hip.check(L.m3d_anab_attention_forward(*ptr, res[0].data_ptr() + 16, B, H, W, Ck, Cv, cs, cs, cs, cs, res[0].stride(0), base,
                                                nbytes, _stream()))
    for j, c in enumerate((Ck, Ck, Cv, 4)):
        if needs[j]:
            res[1 + j] = fresh(c)
    ws, base, nbytes = workspace(1)
    gp = [t.data_ptr() + 16 if t is not None else None for t in res[1:]]
    gcs = [t.stride(0) if t is not None else 0 for t in res[1:]]
    _hip.check(L.m3d_anab_attention_backward(*ptr, gwide.data_ptr() + 16, *gp, B, H, W, Ck, Cv, cs, cs, cs, cs, gwide.stride(0), *gcs,
                                             base, nbytes, _stream()))
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%dx%dx%d_ck%d_cv%d" % c for c in CASES])
def test_operator_matches_float64(i):
    _, _, _, ref64, e32 = _case(i)
    res = _run(i, ws_fill=("nan", "huge")[i % 2])          # forward and backward on a poisoned workspace
    errs = {}
    for name, wide_out, ref, e in zip(NAMES, res, ref64, e32):
        c = ref.shape[1]
        assert torch.equal(wide_out[:, :4], torch.full_like(wide_out[:, :4], GUARD)), name + ": guard columns in front were written"
        assert torch.equal(wide_out[:, 4 + c:], torch.full_like(wide_out[:, 4 + c:], GUARD)), name + ": guard columns behind were written"
        errs[name] = (_err(wide_out[:, 4:4 + c], ref), e)
    print("anab_train operator", CASES[i], errs)
    _log("anab_train_operator", {"case": list(CASES[i]), "errs": {k: list(v) for k, v in errs.items()}})
    for name, (e_op, e) in errs.items():
        assert e_op <= _bound(e), "%s: err %.3e > 4 * %.3e + 2^-20" % (name, e_op, e)


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


def test_single_gradient_calls_equal_the_full_call():
    ref = _run(0, forward=False)
    for j in range(4):
        needs = tuple(k == j for k in range(4))
        res = _run(0, needs=needs, fill="nan", forward=False)
        c = _case(0)[3][1 + j].shape[1]
        assert torch.equal(res[1 + j][:, 4:4 + c], ref[1 + j][:, 4:4 + c]), NAMES[1 + j]


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
