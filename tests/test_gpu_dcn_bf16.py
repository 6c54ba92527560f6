"""GPU tests (-m gpu) of the bf16 DCNv2 operator: m3d_dcn_v2_forward_bf16 / m3d_dcn_v2_backward_bf16 through the C ABI (every output
between sentinel guard regions), and the autocast binding through ops.dcn_v2 and the DCNv2 / DCN / DeformConv modules.

Two kinds of comparison.  EXACT: operands from the dyadic lattice of tests/exact_inputs.py, on which no step of the kernels rounds
(tests/test_dcn_bf16_host.py asserts that premise on the CPU): forward and all five gradients must equal the float64 reference
rounded once to the type the kernel stores, bit for bit.  BOUNDED: random data, x / weight / grad_output rounded to bf16 first so
that the float64 reference (tests/dcn_grad_ref.py) sees the operands the kernel sees; the bounds are derived below from the
rounding points of the operator, not measured."""
import numpy as np
import pytest
import torch

from m3dssd_amd import _hip
from gpu_common import *  # noqa: F401,F403
import dcn_bf16_cases as C
import dcn_grad_ref as R
import exact_inputs as X
from test_gpu_dcn_backward import PARITY_CASES as F32_PARITY_CASES

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAMES = ("input", "offset", "mask", "weight", "bias")
KDT = (BF16, torch.float32, torch.float32, BF16, torch.float32)      # what m3d_dcn_v2_backward_bf16 writes
SENT_BYTE = 0xA5
GUARD = 256                # bytes on each side
U = 2.0 ** -8              # unit roundoff of bf16 as the bounds below use it (8 significant bits)


def _r16(t):
    return t.to(BF16).float()


class Guarded:
    """n elements of `dtype` on the device between two sentinel-filled guard regions; the payload starts as the sentinel bytes or
    as `fill`."""

    def __init__(self, n, dtype, fill=None):
        self.n, self.dtype = int(n), dtype
        self.nb = self.n * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((GUARD + self.nb + GUARD,), SENT_BYTE, dtype=torch.uint8, device=_dev())
        self.t = self.raw[GUARD:GUARD + self.nb].view(dtype)
        if fill is not None:
            self.t.fill_(fill)
        self.ptr = self.t.data_ptr()
        assert self.ptr % 2 == 0

    def get(self):
        raw = self.raw.cpu()
        assert (raw[:GUARD] == SENT_BYTE).all(), "write below the buffer"
        assert (raw[GUARD + self.nb:] == SENT_BYTE).all(), "write beyond the buffer"
        return raw[GUARD:GUARD + self.nb].clone().view(self.dtype)

    def untouched(self):
        return bool((self.raw.cpu() == SENT_BYTE).all())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


class Problem:
    """Device copies of one case (x / weight / grad_output as bf16, offset / mask as given: float32, or bf16 with om16) and the two
    workspaces; forward() and backward() go through the C ABI and return CPU tensors."""

    def __init__(self, ts, go, args, om16=False):
        dev = _dev()
        x, off, m, wt, b = ts
        self.stride, self.pad, self.dil, self.G = args
        self.n, self.c, self.h, self.w = x.shape
        self.co, _, self.kh, self.kw = wt.shape
        self.ho, self.wo = R.out_size(self.h, self.w, self.kh, self.kw, self.stride, self.pad, 1)
        self.shapes = (tuple(x.shape), tuple(off.shape), tuple(m.shape), tuple(wt.shape), (self.co,))
        d16 = lambda t: t.detach().to(dev).contiguous().to(BF16)            # noqa: E731
        d32 = lambda t: t.detach().to(dev).contiguous().float()             # noqa: E731
        self.x, self.wt = d16(x), d16(wt)
        self.go = None if go is None else d16(go)
        self.off, self.m = (d16(off), d16(m)) if om16 else (d32(off), d32(m))
        self.om16 = int(om16)
        self.b = d32(b)
        self.L = _hip.lib()
        self.geom = (self.n, self.c, self.h, self.w, self.co, self.kh, self.kw)
        self.fbytes = self.L.m3d_dcn_v2_workspace_bytes_bf16(*self.geom, self.stride, self.pad, 1, self.G)
        self.nbytes = self.L.m3d_dcn_v2_backward_workspace_bytes_bf16(*self.geom, self.stride, self.pad, 1, self.G)
        assert self.fbytes > 0 and self.nbytes > 0
        self.set_workspace(None)

    def set_workspace(self, byte):
        """Fresh workspaces, every byte = `byte` (None: whatever the allocator hands out)."""
        nb = max(self.fbytes, self.nbytes) + 256
        self.ws = torch.empty(nb, device=_dev(), dtype=torch.uint8) if byte is None else \
            torch.full((nb,), byte, device=_dev(), dtype=torch.uint8)
        self.base = (self.ws.data_ptr() + 255) // 256 * 256

    def _tail(self, dil, nbytes):
        return (*self.geom, self.stride, self.stride, self.pad, self.pad, dil, dil, self.G, self.base, nbytes, _stream())

    def forward_rc(self, out_ptr, dil=1, nbytes=None):
        rc = self.L.m3d_dcn_v2_forward_bf16(self.x.data_ptr(), self.wt.data_ptr(), self.b.data_ptr(), self.off.data_ptr(), self.om16,
                                            self.m.data_ptr(), self.om16, out_ptr, *self._tail(dil, self.fbytes if nbytes is None else nbytes))
        torch.cuda.synchronize()
        return rc

    def forward(self):
        out = Guarded(self.n * self.co * self.ho * self.wo, BF16)
        rc = self.forward_rc(out.ptr)
        assert rc == 0, self.L.m3d_last_error().decode()
        return out.get().view(self.n, self.co, self.ho, self.wo)

    def call(self, ptrs, dil=1, nbytes=None):
        rc = self.L.m3d_dcn_v2_backward_bf16(self.x.data_ptr(), self.wt.data_ptr(), self.off.data_ptr(), self.om16, self.m.data_ptr(),
                                             self.om16, self.go.data_ptr(), *ptrs, *self._tail(dil, self.nbytes if nbytes is None else nbytes))
        torch.cuda.synchronize()
        return rc

    def backward(self, want=(1, 1, 1, 1, 1), fill=None):
        bufs = [Guarded(int(np.prod(s)), dt, fill) if wnt else None for s, dt, wnt in zip(self.shapes, KDT, want)]
        rc = self.call([b.ptr if b is not None else None for b in bufs])
        assert rc == 0, self.L.m3d_last_error().decode()
        return [b.get().view(s) if b is not None else None for b, s in zip(bufs, self.shapes)]


# ======================================================================================== 1. exact forward
@pytest.mark.parametrize("shape", C.EXACT_FWD_CASES)
def test_forward_is_exact_on_the_lattice(shape):
    n, c, h, w, co, k, pad, dg = shape
    ops = X.dcn_operands(sum(shape), n, c, h, w, co, k, pad, dg)
    ref = X.dcn_ref(ops)
    pr = Problem((ops["x"], ops["off"], ops["mask"], ops["weight"], ops["bias"]), None, (1, pad, 1, dg))
    got = pr.forward()
    bad, msg = X.compare_exact(got, ref, BF16, X.DCN_QUANTUM)
    assert bad == 0, msg
    # teeth: what a structurally wrong kernel would compute differs from what came back
    for kind in X.PERTURBATIONS:
        (nb, yy, xx), wrong, right = X.perturbed_pixel(ops, kind, 5 + len(kind))
        g = got.float()[nb, :, yy, xx]
        assert torch.equal(g, X.round_out(right, BF16)), kind
        assert not torch.equal(g, X.round_out(wrong, BF16)), kind + ": the comparison cannot see this error"
    # bf16 offsets and masks (quarter steps, {1/2, 1}: exact in bf16) are widened exactly: the same bits
    got16 = Problem((ops["x"], ops["off"], ops["mask"], ops["weight"], ops["bias"]), None, (1, pad, 1, dg), om16=True).forward()
    assert torch.equal(_bits(got16), _bits(got))


# ======================================================================================== 2. exact backward
@pytest.mark.parametrize("spec", C.EXACT_BWD_CASES)
def test_backward_is_exact_on_the_lattice(spec):
    """All five gradients equal the float64 gradients rounded once to the stored type -- grad_input included, which a bf16
    accumulation (packed bf16 atomics) could not deliver: its partial sums need more than 8 bits."""
    ops, go, ts, args = C.exact_bwd_case(spec)
    _, refs = C.ref_grads64(ts, go, args)
    grads = Problem(ts, go, args).backward()
    for name, g, r, dt in zip(NAMES, grads, refs, KDT):
        bad, msg = X.compare_exact(g, r, dt)
        assert bad == 0, "grad_%s: %s" % (name, msg)
    grads16 = Problem(ts, go, args, om16=True).backward()
    for name, a, b in zip(NAMES, grads16, grads):
        assert torch.equal(_bits(a), _bits(b)), "bf16 offsets / masks: grad_" + name


# ======================================================================================== 3. parity on random data, derived bounds
# n, c, co, h, w, k, stride, pad, dil, G, sigma, seed: the non-dilated rows of the fp32 file up to (2, 32, 128, 13, 17, ...), a deep K,
# and sigma 13 on a map that keeps samples inside
PARITY_CASES = [s for s in F32_PARITY_CASES[:7] if s[8] == 1] + [
    (1, 256, 128, 6, 10, 3, 1, 1, 1, 1, 3.0, 21),
    (1, 64, 64, 16, 40, 3, 1, 1, 1, 1, 13.0, 22),
]


def _parity_refs(ts, go, args):
    """float64 reference (output, five gradients) on the operands the kernel sees, and the abs-pass quantities of the bounds."""
    x, off, m, wt, b = ts
    out, refs = R.ref_grads(ts, go, args)
    # S: the same quantities with x, weight and grad_output replaced by their absolute values (offsets and mask unchanged, bias 0).
    # The corner weights and the mask are non-negative, so S is the sum of the absolute values of the terms.
    s_out, s_grads = R.ref_grads((x.abs(), off, m, wt.abs(), torch.zeros_like(b)), go.abs(), args)
    stride, pad, dil, G = args
    n, c, h, w = x.shape
    co, _, kh, kw = wt.shape
    kk, cg = kh * kw, c // G
    # T[n, g*2kk + 2k (+1), y, x] = 2 max|x| * mask[p, g, k] * sum_c gcol_abs[p, g, k, c],  gcol_abs = sum_co |go| |W|
    gcol_abs = torch.einsum("nohw,ogk->ngkhw", go.abs().double(), wt.abs().double().reshape(co, G, cg, kk).sum(2))
    t_off = (2.0 * float(x.abs().max()) * m.double().view(n, G, kk, *m.shape[2:]) * gcol_abs)
    t_off = t_off.repeat_interleave(2, dim=2).reshape(off.shape)
    s_bias = go.abs().double().sum((0, 2, 3))
    return out, refs, s_out, s_grads, t_off, s_bias


def _bounded(tag, got, ref, spread):
    """|got - ref| <= 1.05 u (spread + |ref|) per element; returns max(err / bound)."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape and torch.isfinite(got).all(), tag
    bound = 1.05 * U * (spread.double() + ref.abs())
    err = (got - ref).abs()
    ratio = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                                   torch.zeros_like(err))).max())
    return ratio


def _check_parity(tag, pr, ts, go, args, check_out=True):
    out, refs, s_out, s_grads, t_off, s_bias = _parity_refs(ts, go, args)
    ratios = {}
    if check_out:
        # Output: sum over (tap, channel) of col * W.  col carries one rounding to bf16 (relative u per term: u * S in all), the
        # weights and inputs are bf16 already (the reference sees them), products are exact, the output is rounded once (u |ref|);
        # the bound allows two narrow operands per chain, 2 u S.  The 5 % covers the fp32 accumulation and second-order terms.
        ratios["output"] = _bounded(tag, pr.forward(), out, 2 * s_out)
    gi, goff, gm, gw, gb = pr.backward()
    # grad_input = sum gcol * mask * corner weight: gcol may be bf16 (u per term), the result is rounded once.
    ratios["grad_input"] = _bounded(tag, gi, refs[0], 2 * s_grads[0])
    # grad_offset = mask * sum_c gcol * d val / d(h, w); |d val / d coordinate| <= 2 max|x| (a difference of two corner values times
    # a weight <= 1, twice), so the terms sum to at most T = 2 max|x| * mask * sum_c gcol_abs; T stands where 2 S stands elsewhere.
    ratios["grad_offset"] = _bounded(tag, goff, refs[1], t_off)
    # grad_mask = sum_c gcol * val: one possibly narrow operand (gcol), val in fp32 from bf16 corner values.
    ratios["grad_mask"] = _bounded(tag, gm, refs[2], 2 * s_grads[2])
    # grad_weight = sum_p go * col: col rounded once per term, the result rounded once.
    ratios["grad_weight"] = _bounded(tag, gw, refs[3], 2 * s_grads[3])
    # grad_bias = sum_p go: bf16 values added in fp32; sum_p |go| stands where 2 S stands.
    ratios["grad_bias"] = _bounded(tag, gb, refs[4], s_bias)
    print(tag, " ".join("%s %.3f" % kv for kv in ratios.items()))
    _log("dcn_bf16", {"case": tag, **ratios})
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _bf16_case(spec):
    (x, off, m, wt, b), go, args = R.make_case(*spec)
    return (_r16(x), off, m, _r16(wt), b), _r16(go), args


@pytest.mark.parametrize("spec", PARITY_CASES)
def test_parity_with_the_float64_reference(spec):
    ts, go, args = _bf16_case(spec)
    _check_parity("bf16 parity %s" % (spec,), Problem(ts, go, args), ts, go, args)


# ======================================================================================== 4. the piecewise rule
def test_samples_far_outside_give_exact_zeros():
    ts, go, args = _bf16_case((2, 16, 12, 9, 11, 3, 1, 1, 1, 1, 1.0, 50))
    x, off, m, wt, b = ts
    off = torch.full_like(off, 100.0)
    off[:, 1::4] = -100.0
    gi, goff, gm, gw, gb = Problem((x, off, m, wt, b), go, args).backward()
    for name, t in (("input", gi), ("offset", goff), ("mask", gm), ("weight", gw)):
        assert not t.float().any(), name
    assert torch.allclose(gb.double(), go.double().sum((0, 2, 3)), rtol=1e-6, atol=1e-6)


def test_border_grid_and_integer_coordinates():
    """1x1, pad 0: the border grid of exact_inputs (coordinates exactly -1, just inside, between rows, the last row, past it with a
    corner row dropped, exactly H) with random bf16 data, and integer coordinates on a 3x3 (the one-sided derivative)."""
    h, w = 16, 16
    ts, go, args = _bf16_case((1, 16, 8, h, w, 1, 1, 0, 1, 1, 1.0, 60))
    x, _, m, wt, b = ts
    off = X.border_grid_offsets(h, w)
    _, refs = R.ref_grads((x, off, m, wt, b), go, args)
    assert refs[0].abs().max() > 0 and refs[1].abs().max() > 0
    _check_parity("bf16 border grid", Problem((x, off, m, wt, b), go, args), (x, off, m, wt, b), go, args)
    ts, go, args = _bf16_case((2, 16, 8, 9, 12, 3, 1, 1, 1, 1, 1.0, 62))
    x, off, m, wt, b = ts
    off = torch.randint(-2, 3, off.shape, generator=torch.Generator().manual_seed(63)).float()
    _check_parity("bf16 integer coordinates", Problem((x, off, m, wt, b), go, args), (x, off, m, wt, b), go, args)


def test_non_finite_coordinates_have_zero_gradients():
    ts, go, args = _bf16_case((1, 32, 32, 8, 16, 3, 1, 1, 1, 1, 1.0, 70))
    x, off, m, wt, b = ts
    g = torch.Generator().manual_seed(71)
    hit = torch.rand(off.shape, generator=g) < 0.05
    vals = torch.tensor([float("nan"), float("inf"), -float("inf")])[torch.randint(0, 3, off.shape, generator=g)]
    bad = torch.where(hit, vals, off)
    far = torch.where(hit, torch.full_like(off, 1e4), off)           # the reference sees the same samples far outside the map
    pr = Problem((x, bad, m, wt, b), go, args)
    grads = pr.backward()
    out = pr.forward()
    assert torch.isfinite(out.float()).all()
    for t in grads:
        assert torch.isfinite(t.float()).all()
    tap_hit = hit[:, 0::2] | hit[:, 1::2]
    assert not grads[2][tap_hit].any()
    assert not grads[1][:, 0::2][tap_hit].any() and not grads[1][:, 1::2][tap_hit].any()
    _check_parity("bf16 non-finite offsets", pr, (x, far, m, wt, b), go, args)


# ======================================================================================== 5. pointers and workspace
def test_null_gradients_workspace_and_dilation():
    ts, go, args = _bf16_case((2, 20, 12, 9, 11, 3, 1, 1, 1, 2, 2.0, 80))
    pr = Problem(ts, go, args)
    full = pr.backward()
    subsets = [tuple(int(i == j) for i in range(5)) for j in range(5)]
    for want in subsets:
        part = pr.backward(want)
        assert [a is not None for a in part] == [bool(v) for v in want]
        for i in range(1, 5):                                              # (grad_input: float atomics, covered by the bounds)
            if want[i]:
                assert torch.equal(_bits(part[i]), _bits(full[i])), (want, NAMES[i])
    assert pr.call([None] * 5) == 0
    # a workspace full of NaN bit patterns (all bytes 0xFF) gives the bits of a zeroed one
    from poison import poison_
    res = {}
    for fill in ("zero", "nan"):
        pr.set_workspace(0)
        poison_(pr.ws.view(torch.float32) if fill == "nan" else pr.ws, fill)
        res[fill] = (pr.forward(), pr.backward())
    assert torch.equal(_bits(res["zero"][0]), _bits(res["nan"][0]))
    for i in range(1, 5):
        assert torch.equal(_bits(res["zero"][1][i]), _bits(res["nan"][1][i])), NAMES[i]
    assert torch.isfinite(res["nan"][1][0].float()).all()
    # short workspaces
    out = Guarded(int(np.prod(pr.shapes[3])), BF16)
    assert pr.call([None, None, None, out.ptr, None], nbytes=pr.nbytes - 1) == -3          # M3D_E_WORKSPACE
    msg = pr.L.m3d_last_error().decode()
    assert str(pr.nbytes) in msg and str(pr.nbytes - 1) in msg
    fo = Guarded(pr.n * pr.co * pr.ho * pr.wo, BF16)
    assert pr.forward_rc(fo.ptr, nbytes=pr.fbytes - 1) == -3
    msg = pr.L.m3d_last_error().decode()
    assert str(pr.fbytes) in msg and str(pr.fbytes - 1) in msg
    # dilation 2 is refused, and says so
    assert pr.call([None, None, None, out.ptr, None], dil=2) == -1                           # M3D_E_ARG
    assert "dilation 1 only" in pr.L.m3d_last_error().decode()
    assert pr.forward_rc(fo.ptr, dil=2) == -1
    assert "dilation 1 only" in pr.L.m3d_last_error().decode()
    assert out.untouched() and fo.untouched()
    pr.G = 3                                                                                 # 3 does not divide 20
    assert pr.call([None, None, None, out.ptr, None]) == -1
    assert "deformable_group" in pr.L.m3d_last_error().decode()


# ======================================================================================== 6. reproducibility, overwrite semantics
def test_twenty_launches_are_reproducible_and_outputs_are_overwritten():
    ts, go, args = _bf16_case((2, 64, 64, 12, 20, 3, 1, 1, 1, 1, 3.0, 90))
    pr = Problem(ts, go, args)
    first = pr.backward()
    for it in range(1, 20):
        cur = pr.backward(fill=float("nan") if it % 2 else 1e30)
        for i in range(1, 5):
            assert torch.equal(_bits(cur[i]), _bits(first[i])), (it, NAMES[i])
        assert torch.isfinite(cur[0].float()).all()
    _check_parity("bf16 determinism run", pr, ts, go, args, check_out=False)


# ======================================================================================== 7. the autocast binding
def _record_calls(monkeypatch):
    from m3dssd_amd.host import ops
    calls, real = [], ops.dcn_v2

    def wrapper(*a, **kw):
        out = real(*a, **kw)
        calls.append((a, kw, out))
        return out
    monkeypatch.setattr(ops, "dcn_v2", wrapper)
    return calls, real


def _replay(real, call, go):
    """The explicit op on detached copies of the tensors the module handed over: (output, grads of the five tensors)."""
    a, kw, _ = call
    lv = [t.detach().clone().requires_grad_(True) for t in a[:5]]
    out = real(*lv, *a[5:], **kw)
    (out.float() * go).sum().backward()
    return out.detach(), [t.grad for t in lv]


def test_modules_under_autocast(monkeypatch):
    from m3dssd_amd.host import ops
    from model.DCNv2.dcn_v2 import DCN, DCNv2
    from model.pose_dla_dcn import DeformConv
    dev = _dev()
    calls, real = _record_calls(monkeypatch)
    g = torch.Generator().manual_seed(200)
    n, c, co, h, w = 2, 24, 20, 10, 14
    go = torch.randn(n, co, h, w, generator=g).to(dev)
    x16 = torch.randn(n, c, h, w, generator=g).to(dev).to(BF16)

    # DCNv2: offsets / mask given (float32 leaves), float32 parameters
    mod = DCNv2(c, co, 3, 1, 1, 1, 2).to(dev)
    with torch.no_grad():
        mod.bias.normal_(0, 0.1, generator=None)
    off = (torch.randn(n, 2 * 2 * 9, h, w, generator=g) * 2).to(dev).requires_grad_(True)
    m = torch.sigmoid(torch.randn(n, 2 * 9, h, w, generator=g)).to(dev).requires_grad_(True)
    x = x16.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16):
        out = mod(x, off, m)
    assert out.dtype == BF16 and out.grad_fn is not None
    (out.float() * go).sum().backward()
    assert x.grad.dtype == BF16 and off.grad.dtype == torch.float32 and m.grad.dtype == torch.float32
    assert mod.weight.grad.dtype == torch.float32 and mod.bias.grad.dtype == torch.float32
    r_out, r_g = _replay(real, calls[-1], go)
    assert torch.equal(_bits(out.detach()), _bits(r_out))
    for name, a, b in zip(NAMES[1:], (off.grad, m.grad, mod.weight.grad, mod.bias.grad), r_g[1:]):
        assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), name
        assert torch.isfinite(a).all() and a.abs().max() > 0, name
    assert torch.isfinite(x.grad.float()).all()
    # the weight gradient went through one bf16 rounding
    assert torch.equal(mod.weight.grad, mod.weight.grad.to(BF16).float())

    # DCN: its own offset / mask convolution runs under autocast and hands bf16 offsets over
    dcn = DCN(c, co, (3, 3), 1, 1).to(dev)
    with torch.no_grad():
        dcn.conv_offset_mask.weight.normal_(0, 0.05)
        dcn.conv_offset_mask.bias.normal_(0, 0.5)
    x = x16.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16):
        out = dcn(x)
    a, kw, _ = calls[-1]
    assert a[0].dtype == BF16 and a[1].dtype == BF16 and a[2].dtype == BF16 and a[3].dtype == torch.float32
    assert out.dtype == BF16
    (out.float() * go).sum().backward()
    r_out, r_g = _replay(real, calls[-1], go)
    assert torch.equal(_bits(out.detach()), _bits(r_out))
    for name, p, b in (("weight", dcn.weight, r_g[3]), ("bias", dcn.bias, r_g[4])):
        assert p.grad.dtype == torch.float32 and torch.equal(_bits(p.grad), _bits(b)), name
    for p in dcn.parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all()
    assert dcn.conv_offset_mask.weight.grad.abs().max() > 0

    # DeformConv in training mode
    dc = DeformConv(c, co).to(dev).train()
    with torch.no_grad():
        dc.conv.conv_offset_mask.weight.normal_(0, 0.05)
        dc.conv.conv_offset_mask.bias.normal_(0, 0.5)
    x = x16.clone().requires_grad_(True)
    ncalls = len(calls)
    with torch.autocast("cuda", dtype=BF16):
        out = dc(x)
    assert len(calls) == ncalls + 1 and calls[-1][2].dtype == BF16
    assert out.dtype == BF16
    (out.float() * go).sum().backward()
    for p in dc.parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all()
    assert x.grad.dtype == BF16 and torch.isfinite(x.grad.float()).all()


def test_float32_results_do_not_move_and_other_types_are_refused():
    from m3dssd_amd.host import ops
    dev = _dev()
    ts, go, args = R.make_case(2, 24, 20, 10, 14, 3, 1, 1, 1, 2, 2.0, 210)
    x, off, m, wt, b = [t.to(dev) for t in ts]
    go = go.to(dev)

    def f32():
        out = ops.dcn_v2_forward(x, off, m, wt, b, *args)
        return [out] + list(ops.dcn_v2_backward(x, off, m, wt, go, *args))
    before = f32()
    assert all(t.dtype == torch.float32 for t in before)
    o16 = ops.dcn_v2_forward(x.to(BF16), off, m, wt, b, *args)
    g16 = ops.dcn_v2_backward(x.to(BF16), off.to(BF16), m, wt, go.to(BF16), *args)
    assert o16.dtype == BF16
    assert [t.dtype for t in g16] == [BF16, BF16, torch.float32, torch.float32, torch.float32]
    after = f32()
    for i, (a_, b_) in enumerate(zip(before, after)):
        if i != 1:                                                         # (grad_input: float atomics)
            assert torch.equal(_bits(a_), _bits(b_)), i
    assert torch.allclose(before[1], after[1], rtol=1e-4, atol=1e-4)
    for dt in (torch.float16, torch.float64):
        with pytest.raises(RuntimeError, match="float32 and bfloat16"):
            ops.dcn_v2_forward(x.to(dt), off, m, wt, b, *args)
        with pytest.raises(RuntimeError, match="float32 and bfloat16"):
            ops.dcn_v2_backward(x.to(dt), off, m, wt, go, *args)
    with pytest.raises(RuntimeError, match="dilation 1 only"):
        ops.dcn_v2_forward(x.to(BF16), off, m, wt, b, 1, 2, 2, 2)
