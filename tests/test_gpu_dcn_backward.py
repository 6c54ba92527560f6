"""GPU tests (-m gpu) of the DCNv2 backward: m3d_dcn_v2_backward through the C ABI, the autograd binding ops.dcn_v2 and the three
modules that wrap it (DCNv2, DCN, DeformConv).

Reference: tests/dcn_grad_ref.py, a float64 autograd restatement of the forward whose sampling coordinates are formed in float32
in the kernel's order (pinned on the CPU by tests/test_dcn_backward_host.py).  Bound for EVERY gradient element, the project's
op-level bar: |g_hip - g_ref64| <= 2e-4 * (1 + |g_ref64|); the closed-form tests compare with
torch.nn.functional.conv2d in float64 instead.  Every output of the C-ABI calls sits between sentinel-filled guard regions.
Measured maxima are logged through gpu_common._log (DESIGN.md section 4 quotes them)."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from m3dssd_amd import _hip
from gpu_common import *  # noqa: F401,F403
import dcn_bf16_cases as C
import dcn_grad_ref as R
import exact_inputs as X

pytestmark = pytest.mark.gpu

BOUND = 2e-4
NAMES = ("input", "offset", "mask", "weight", "bias")
SENT = -559038737          # 0xDEADBEEF as int32
GUARD = 64                 # 4-byte elements on each side (256 bytes)


class Guarded:
    """n floats on the device between two sentinel-filled guard regions; the payload starts as `fill` (default: the sentinel)."""

    def __init__(self, n, fill=None):
        self.n = int(n)
        self.raw = torch.full((GUARD + self.n + GUARD,), SENT, dtype=torch.int32, device=_dev())
        self.t = self.raw[GUARD:GUARD + self.n].view(torch.float32)
        if fill is not None:
            self.t.fill_(fill)
        self.ptr = self.t.data_ptr()

    def get(self):
        raw = self.raw.cpu().numpy()
        assert (raw[:GUARD] == SENT).all(), "write below the buffer"
        assert (raw[GUARD + self.n:] == SENT).all(), "write beyond the buffer"
        return raw[GUARD:GUARD + self.n].view(np.float32).copy()


class Problem:
    """Device copies of one case + a workspace; run() launches m3d_dcn_v2_backward and returns the wanted gradients as numpy."""

    def __init__(self, ts, go, args):
        dev = _dev()
        x, off, m, wt, b = ts
        self.stride, self.pad, self.dil, self.G = args
        self.n, self.c, self.h, self.w = x.shape
        self.co, _, self.kh, self.kw = wt.shape
        self.shapes = (tuple(x.shape), tuple(off.shape), tuple(m.shape), tuple(wt.shape), (self.co,))
        self.dev_in = [t.detach().to(dev).contiguous().float() for t in (x, wt, off, m, go)]
        self.L = _hip.lib()
        self.nbytes = self.L.m3d_dcn_v2_backward_workspace_bytes(self.n, self.c, self.h, self.w, self.co, self.kh, self.kw, self.stride,
                                                                 self.pad, self.dil, self.G)
        assert self.nbytes > 0
        self.ws = torch.empty(self.nbytes + 256, device=dev, dtype=torch.uint8)
        self.base = (self.ws.data_ptr() + 255) // 256 * 256

    def call(self, ptrs, nbytes=None):
        rc = self.L.m3d_dcn_v2_backward(*[t.data_ptr() for t in self.dev_in], *ptrs, self.n, self.c, self.h, self.w, self.co, self.kh,
                                        self.kw, self.stride, self.stride, self.pad, self.pad, self.dil, self.dil, self.G, self.base,
                                        self.nbytes if nbytes is None else nbytes, _stream())
        torch.cuda.synchronize()
        return rc

    def run(self, want=(1, 1, 1, 1, 1), fill=None):
        bufs = [Guarded(int(np.prod(s)), fill) if wnt else None for s, wnt in zip(self.shapes, want)]
        rc = self.call([b.ptr if b is not None else None for b in bufs])
        assert rc == 0, self.L.m3d_last_error().decode()
        return [b.get().reshape(s) if b is not None else None for b, s in zip(bufs, self.shapes)]


def _err(got, ref):
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, dtype=np.float64)
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.isfinite(got).all()
    return float(np.max(np.abs(got - ref) / (1.0 + np.abs(ref))))


def _check(tag, grads, refs, names=NAMES, bound=BOUND):
    errs = {n: _err(g, r) for n, g, r in zip(names, grads, refs) if g is not None}
    print(tag, " ".join("%s %.2e" % kv for kv in errs.items()))
    _log("dcn_backward", {"case": tag, **{"grad_" + k: v for k, v in errs.items()}})
    bad = {k: v for k, v in errs.items() if not v <= bound}
    assert not bad, (tag, bad)
    return errs


# ======================================================================================== 5. parity with the float64 reference
# n, c, co, h, w, k, stride, pad, dil, G, sigma, seed
PARITY_CASES = [
    (2, 8, 6, 9, 11, 3, 1, 1, 1, 1, 0.5, 10),          # 3x3 stride 1 pad 1; Ho*Wo = 99
    (2, 16, 16, 7, 9, 1, 1, 0, 1, 1, 3.0, 11),         # 1x1 pad 0: center_align's form
    (1, 8, 4, 10, 12, 3, 2, 1, 1, 2, 3.0, 12),         # stride 2, G = 2
    (1, 6, 5, 12, 10, 3, 1, 2, 2, 3, 3.0, 13),         # dilation 2 with pad 2, G = 3, C = 6, Co = 5
    (2, 20, 72, 11, 13, 3, 1, 1, 1, 1, 13.0, 14),      # C = 20, Co = 72, sigma 13 (the shape_align range): most samples outside
    (1, 64, 64, 16, 40, 3, 1, 1, 1, 1, 13.0, 15),      # sigma 13 on a map large enough to keep samples inside
    (2, 32, 128, 13, 17, 3, 1, 1, 1, 1, 0.5, 16),      # Co a multiple of 128 (the wide weight-gradient tile), odd pixel count
    (2, 256, 128, 24, 80, 3, 1, 1, 1, 1, 3.0, 17),     # M3DSSD: ida_up proj, 256 -> 128 at 24x80
    (2, 128, 128, 48, 160, 3, 1, 1, 1, 1, 3.0, 18),    # M3DSSD: the largest layer, 128 -> 128 at 48x160
]


@pytest.mark.parametrize("spec", PARITY_CASES)
def test_backward_matches_float64_reference(spec):
    ts, go, args = R.make_case(*spec)
    _, refs = R.ref_grads(ts, go, args)
    grads = Problem(ts, go, args).run()
    _check("parity %s" % (spec,), grads, refs)


@pytest.mark.parametrize("spec", C.EXACT_BWD_CASES)
def test_backward_is_exact_on_the_lattice(spec):
    """The five lattice cases of the bf16 operator (tests/dcn_bf16_cases.py) through the fp32 entry point: no step rounds there
    (tests/test_dcn_bf16_host.py asserts it on the CPU, grad_input's atomic sums included), so all five gradients equal the float64
    reference bit for bit.  The sampling kernel is one template for both types: this pins its fp32 instantiation."""
    _, go, ts, args = C.exact_bwd_case(spec)
    _, refs = C.ref_grads64(ts, go, args)
    grads = Problem(ts, go, args).run()
    for name, g, r in zip(NAMES, grads, refs):
        bad, msg = X.compare_exact(torch.from_numpy(g), r, torch.float32)
        assert bad == 0, "grad_%s: %s" % (name, msg)


# ======================================================================================== 6. closed forms
def test_zero_offsets_unit_mask_equal_a_plain_convolution():
    for (n, c, co, h, w, k, stride, pad, dil) in ((2, 16, 24, 10, 13, 3, 1, 1, 1), (1, 8, 8, 11, 9, 3, 2, 1, 1), (1, 8, 5, 9, 12, 3, 1, 2, 2),
                                                  (2, 32, 16, 6, 7, 1, 1, 0, 1)):
        g = torch.Generator().manual_seed(40 + k + stride + dil)
        ho, wo = R.out_size(h, w, k, k, stride, pad, dil)
        x = torch.randn(n, c, h, w, generator=g)
        wt = torch.randn(co, c, k, k, generator=g) / (c * k * k) ** 0.5
        b = torch.randn(co, generator=g)
        go = torch.randn(n, co, ho, wo, generator=g)
        off, m = torch.zeros(n, 2 * k * k, ho, wo), torch.ones(n, k * k, ho, wo)
        x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wt, b))
        F.conv2d(x64, w64, b64, stride, pad, dil).backward(go.double())
        gm = torch.zeros(n, k * k, ho, wo, dtype=torch.float64)
        for tap in range(k * k):
            wk = torch.zeros_like(wt, dtype=torch.float64)
            wk[:, :, tap // k, tap % k] = wt[:, :, tap // k, tap % k].double()
            gm[:, tap] = (go.double() * F.conv2d(x.double(), wk, None, stride, pad, dil)).sum(1)
        gi, _, gmask, gw, gb = Problem((x, off, m, wt, b), go, (stride, pad, dil, 1)).run()
        _check("conv2d closed form k%d s%d d%d" % (k, stride, dil), (gi, gmask, gw, gb), (x64.grad, gm, w64.grad, b64.grad),
               names=("input", "mask", "weight", "bias"))


def test_samples_far_outside_give_exact_zeros():
    ts, go, args = R.make_case(2, 16, 12, 9, 11, 3, 1, 1, 1, 1, 1.0, 50)
    x, off, m, wt, b = ts
    off = torch.full_like(off, 100.0)
    off[:, 1::4] = -100.0
    gi, goff, gm, gw, gb = Problem((x, off, m, wt, b), go, args).run()
    for name, t in (("input", gi), ("offset", goff), ("mask", gm), ("weight", gw)):
        assert not t.any(), name
    _check("far outside", (gb,), (go.double().sum((0, 2, 3)),), names=("bias",))


def _coords_to_offsets(th, tw, h, w, k, stride, pad, dil):
    """Offsets [n, 2kk, ho, wo] that put tap (i, j) of output pixel (y, x) at the target coordinates th / tw [n, kk, ho, wo]."""
    n, kk, ho, wo = th.shape
    off = torch.zeros(n, 2 * kk, ho, wo)
    ys = (torch.arange(ho) * stride - pad).view(1, ho, 1).float()
    xs = (torch.arange(wo) * stride - pad).view(1, 1, wo).float()
    for tap in range(kk):
        i, j = divmod(tap, k)
        off[:, 2 * tap] = th[:, tap] - (ys + i * dil)
        off[:, 2 * tap + 1] = tw[:, tap] - (xs + j * dil)
    return off


def test_border_grid_with_dropped_corners():
    """Coordinates in (-1, 0) and (H-1, H) on both axes: one or two of the four corners lie outside and are dropped."""
    n, c, co, h, w, k = 2, 16, 8, 9, 12, 3
    ts, go, args = R.make_case(n, c, co, h, w, k, 1, 1, 1, 1, 1.0, 60)
    x, _, m, wt, b = ts
    g = torch.Generator().manual_seed(61)
    frac = lambda: 0.05 + 0.9 * torch.rand(n, k * k, h, w, generator=g)
    pick = lambda: torch.rand(n, k * k, h, w, generator=g) < 0.5
    th = torch.where(pick(), frac() - 1.0, frac() + (h - 1))
    tw = torch.where(pick(), frac() - 1.0, frac() + (w - 1))
    off = _coords_to_offsets(th, tw, h, w, k, 1, 1, 1)
    _, refs = R.ref_grads((x, off, m, wt, b), go, args)
    assert refs[0].abs().max() > 0 and refs[1].abs().max() > 0
    _check("border grid", Problem((x, off, m, wt, b), go, args).run(), refs)


def test_integer_coordinates_take_the_one_sided_derivative():
    n, c, co, h, w, k = 2, 16, 8, 9, 12, 3
    ts, go, args = R.make_case(n, c, co, h, w, k, 1, 1, 1, 1, 1.0, 62)
    x, off, m, wt, b = ts
    off = torch.randint(-2, 3, off.shape, generator=torch.Generator().manual_seed(63)).float()
    _, refs = R.ref_grads((x, off, m, wt, b), go, args)
    _check("integer coordinates", Problem((x, off, m, wt, b), go, args).run(), refs)


# ======================================================================================== 7. non-finite offsets
def test_non_finite_coordinates_have_zero_gradients():
    ts, go, args = R.make_case(1, 32, 32, 8, 16, 3, 1, 1, 1, 1, 1.0, 70)
    x, off, m, wt, b = ts
    g = torch.Generator().manual_seed(71)
    hit = torch.rand(off.shape, generator=g) < 0.05
    vals = torch.tensor([float("nan"), float("inf"), -float("inf")])[torch.randint(0, 3, off.shape, generator=g)]
    bad = torch.where(hit, vals, off)
    # the reference sees the same samples far outside the map instead (a non-finite coordinate is "outside" in the forward)
    _, refs = R.ref_grads((x, torch.where(hit, torch.full_like(off, 1e4), off), m, wt, b), go, args)
    grads = Problem((x, bad, m, wt, b), go, args).run()
    for t in grads:
        assert np.isfinite(t).all()
    tap_hit = (hit[:, 0::2] | hit[:, 1::2]).numpy()                      # [n, kk, ho, wo]: either coordinate of the tap
    assert not grads[2][tap_hit].any()
    assert not grads[1][:, 0::2][tap_hit].any() and not grads[1][:, 1::2][tap_hit].any()
    _check("non-finite offsets", grads, refs)


# ======================================================================================== 8. NULL gradients, guards, workspace
def test_null_gradients_guards_and_workspace():
    ts, go, args = R.make_case(2, 20, 12, 9, 11, 3, 1, 1, 1, 2, 2.0, 80)
    _, refs = R.ref_grads(ts, go, args)
    pr = Problem(ts, go, args)
    full = pr.run()
    _check("null: all five", full, refs)
    for i in range(5):
        want = [0] * 5
        want[i] = 1
        alone = pr.run(want)
        assert [a is not None for a in alone] == [bool(v) for v in want]
        if i == 0:
            _check("null: grad_input alone", (alone[0],), (refs[0],), names=("input",))
        else:
            assert np.array_equal(alone[i].view(np.int32), full[i].view(np.int32)), NAMES[i]
    assert pr.call([None] * 5) == 0                                         # nothing wanted: nothing to do
    out = Guarded(int(np.prod(pr.shapes[3])))
    rc = pr.call([None, None, None, out.ptr, None], nbytes=pr.nbytes - 1)
    assert rc == -3                                                         # M3D_E_WORKSPACE
    msg = pr.L.m3d_last_error().decode()
    assert str(pr.nbytes) in msg and str(pr.nbytes - 1) in msg
    assert (out.get().view(np.int32) == SENT).all()
    pr.G = 3                                                                # 3 does not divide 20
    assert pr.call([None, None, None, out.ptr, None]) == -1                 # M3D_E_ARG
    assert "deformable_group" in pr.L.m3d_last_error().decode()


# ======================================================================================== 9. determinism, overwrite semantics
def test_twenty_launches_are_reproducible_and_outputs_are_overwritten():
    ts, go, args = R.make_case(2, 64, 64, 16, 40, 3, 1, 1, 1, 1, 3.0, 90)
    _, refs = R.ref_grads(ts, go, args)
    pr = Problem(ts, go, args)
    first = pr.run()
    worst = 0.0
    for it in range(1, 20):
        cur = pr.run(fill=float("nan") if it % 2 else 1e30)                # garbage in the outputs: they are overwritten
        for i in range(1, 5):
            assert np.array_equal(cur[i].view(np.int32), first[i].view(np.int32)), (it, NAMES[i])
        e = _err(cur[0], refs[0])
        worst = max(worst, e)
        assert e <= BOUND, (it, e)
    _check("determinism run 0", first, refs)
    _log("dcn_backward", {"case": "determinism: grad_input worst of 20", "grad_input": worst})


# ======================================================================================== 10. autograd, modules
def _leaves(ts, dev):
    return [t.detach().to(dev).requires_grad_(True) for t in ts]


def test_autograd_function_and_dcnv2_module():
    from m3dssd_amd.host import ops
    from model.DCNv2.dcn_v2 import DCNv2
    from model.DCNv2.dcn_v2_func import DCNv2Function
    dev = _dev()
    ts, go, args = R.make_case(2, 24, 20, 10, 14, 3, 1, 1, 1, 2, 2.0, 100)
    stride, pad, dil, G = args
    _, refs = R.ref_grads(ts, go, args)
    lv = _leaves(ts, dev)
    out = ops.dcn_v2(*lv, stride, pad, dil, G)
    with torch.no_grad():
        plain = ops.dcn_v2_forward(*[t.detach() for t in lv], stride, pad, dil, G)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    (out * go.to(dev)).sum().backward()
    _check("autograd ops.dcn_v2", [t.grad for t in lv], refs)
    # only the weights require grad: the result has a grad_fn and weight.grad is right
    lv = [t.detach().to(dev) for t in ts]
    lv[3].requires_grad_(True)
    out = DCNv2Function(stride, pad, dil, G)(*lv)
    assert out.grad_fn is not None
    (out * go.to(dev)).sum().backward()
    _check("autograd weights only", (lv[3].grad,), (refs[3],), names=("weight",))
    assert all(t.grad is None for i, t in enumerate(lv) if i != 3)
    # DCNv2 module: parameters and inputs
    mod = DCNv2(24, 20, 3, stride, pad, dil, G).to(dev)
    with torch.no_grad():
        mod.weight.copy_(ts[3])
        mod.bias.copy_(ts[4])
    x, off, m = _leaves(ts[:3], dev)
    out = mod(x, off, m)
    assert torch.equal(out.detach(), plain)
    (out * go.to(dev)).sum().backward()
    _check("autograd DCNv2 module", (x.grad, off.grad, m.grad, mod.weight.grad, mod.bias.grad), refs)


def _dcn_cpu64(mod64, x64):
    """DCN.forward (dcn_v2.py:64-70) as a float64 CPU composition around the reference restatement."""
    om = F.conv2d(x64, mod64.conv_offset_mask.weight, mod64.conv_offset_mask.bias, mod64.stride, mod64.padding)
    o1, o2, mask = torch.chunk(om, 3, dim=1)
    return R.dcn_ref(x64, torch.cat((o1, o2), 1), torch.sigmoid(mask), mod64.weight, mod64.bias, mod64.stride, mod64.padding,
                     mod64.dilation, mod64.deformable_groups)


def _make_dcn(cin, cout, G, seed):
    from model.DCNv2.dcn_v2 import DCN
    torch.manual_seed(seed)
    mod = DCN(cin, cout, (3, 3), 1, 1, deformable_groups=G)
    with torch.no_grad():
        mod.conv_offset_mask.weight.normal_(0, 0.05)
        mod.conv_offset_mask.bias.normal_(0, 0.5)
        mod.bias.normal_(0, 0.1)
    return mod


def test_dcn_module_gradients():
    dev = _dev()
    for G in (1, 2):
        mod = _make_dcn(16, 24, G, 110 + G)
        g = torch.Generator().manual_seed(112)
        x, go = torch.randn(2, 16, 11, 15, generator=g), torch.randn(2, 24, 11, 15, generator=g)
        ref_mod = copy.deepcopy(mod).double()
        x64 = x.double().requires_grad_(True)
        ref_out = _dcn_cpu64(ref_mod, x64)
        ref_out.backward(go.double())
        mod = mod.to(dev)
        xd = x.to(dev).requires_grad_(True)
        out = mod(xd)
        assert out.grad_fn is not None
        _check("DCN module G%d output" % G, (out,), (ref_out,), names=("output",))
        (out * go.to(dev)).sum().backward()
        _check("DCN module G%d" % G,
               (mod.conv_offset_mask.weight.grad, mod.conv_offset_mask.bias.grad, mod.weight.grad, mod.bias.grad, xd.grad),
               (ref_mod.conv_offset_mask.weight.grad, ref_mod.conv_offset_mask.bias.grad, ref_mod.weight.grad, ref_mod.bias.grad,
                x64.grad), names=("offmask_weight", "offmask_bias", "weight", "bias", "input"))


def test_deform_conv_training_mode():
    """DeformConv in training mode (pose_dla_dcn.py:482-485: DCN, BatchNorm with batch statistics, LeakyReLU): output and input
    gradient against the float64 CPU composition at the 5e-4 of test_standalone_modules_match_oracle."""
    from model.pose_dla_dcn import DeformConv
    dev = _dev()
    torch.manual_seed(120)
    dc = DeformConv(32, 48)
    with torch.no_grad():
        dc.conv.conv_offset_mask.weight.normal_(0, 0.05)
        dc.conv.conv_offset_mask.bias.normal_(0, 0.5)
        dc.actf[0].weight.uniform_(0.5, 1.5)
        dc.actf[0].bias.normal_(0, 0.2)
    g = torch.Generator().manual_seed(121)
    x, go = torch.randn(2, 32, 12, 18, generator=g), torch.randn(2, 48, 12, 18, generator=g)
    ref = copy.deepcopy(dc).double().train()
    x64 = x.double().requires_grad_(True)
    ref_out = F.leaky_relu(ref.actf[0](_dcn_cpu64(ref.conv, x64)), 0.01)
    ref_out.backward(go.double())
    dc = dc.to(dev).train()
    xd = x.to(dev).requires_grad_(True)
    out = dc(xd)
    (out * go.to(dev)).sum().backward()
    _check("DeformConv training", (out, xd.grad, dc.conv.weight.grad), (ref_out, x64.grad, ref.conv.weight.grad),
           names=("output", "input", "weight"), bound=5e-4)
    assert torch.allclose(dc.actf[0].running_mean.cpu().double(), ref.actf[0].running_mean, atol=1e-4)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        dc(x.to(dev))                                                       # training mode without grad: as before


# ======================================================================================== 11. five SGD steps
def test_five_sgd_steps_follow_the_float64_trajectory():
    from model.DCNv2.dcn_v2 import DCN
    dev = _dev()
    g = torch.Generator().manual_seed(0)
    c, co, h, w, k = 16, 16, 12, 20, 3
    x = torch.randn(2, c, h, w, generator=g)
    tgt = torch.roll(x, shifts=(1, -2), dims=(2, 3))[:, :co]
    mod = DCN(c, co, (k, k), 1, 1)
    with torch.no_grad():
        mod.conv_offset_mask.weight.copy_(torch.randn(27, c, k, k, generator=g) * 0.05)
        mod.conv_offset_mask.bias.zero_()
        mod.weight.copy_(torch.randn(co, c, k, k, generator=g) / (c * k * k) ** 0.5)
        mod.bias.zero_()
    ref = copy.deepcopy(mod).double()
    mod = mod.to(dev)
    names = ("conv_offset_mask.weight", "conv_offset_mask.bias", "weight", "bias")

    def steps(m, fwd, xin, target):
        ps = [m.conv_offset_mask.weight, m.conv_offset_mask.bias, m.weight, m.bias]
        losses = []
        for _ in range(5):
            loss = ((fwd(m, xin) - target) ** 2).mean()
            losses.append(float(loss))
            gs = torch.autograd.grad(loss, ps)
            with torch.no_grad():
                for p, gr in zip(ps, gs):
                    p -= 0.5 * gr
        return losses, [p.detach() for p in ps]

    l64, p64 = steps(ref, _dcn_cpu64, x.double(), tgt.double())
    lhip, phip = steps(mod, lambda m, xin: m(xin), x.to(dev), tgt.to(dev))
    print("losses hip %s\nlosses f64 %s" % (lhip, l64))
    assert lhip[-1] < lhip[0] and l64[-1] < l64[0]
    _check("sgd 5 steps", phip, p64, names=names)
    _log("dcn_backward", {"case": "sgd losses", "hip": lhip, "f64": l64})


# ======================================================================================== 12. the no_grad paths are the parent's
def test_no_grad_paths_are_unchanged():
    from m3dssd_amd.host import ops, standalone
    from model.DCNv2.dcn_v2 import DCNv2
    from model.pose_dla_dcn import DeformConv
    dev = _dev()
    ts, go, args = R.make_case(2, 32, 32, 10, 14, 3, 1, 1, 1, 1, 2.0, 130)
    x, off, m, wt, b = [t.to(dev) for t in ts]
    mod = DCNv2(32, 32, 3, 1, 1).to(dev)
    with torch.no_grad():
        out = mod(x, off, m)
        assert out.grad_fn is None and torch.equal(out, ops.dcn_v2_forward(x, off, m, mod.weight, mod.bias, 1, 1, 1, 1))
    dcn = _make_dcn(32, 32, 1, 131).to(dev)
    with torch.no_grad():
        out = dcn(x)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, standalone.dcn_layer_forward(dcn, x))
    for p in dcn.parameters():                                              # frozen parameters, grad mode on: the fused path
        p.requires_grad_(False)
    assert torch.equal(dcn(x), out)
    dc = DeformConv(32, 32).to(dev).eval()
    out = dc(x)                                                             # eval mode, grad mode on: the fused path
    assert out.grad_fn is None and torch.equal(out, standalone.deform_conv_forward(dc, x))
    with torch.no_grad():
        assert torch.equal(dc(x), out)
