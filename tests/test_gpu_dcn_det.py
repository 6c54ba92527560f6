"""GPU tests (-m gpu) of the deterministic DCNv2 backward: m3d_dcn_v2_backward_det / m3d_dcn_v2_backward_det_bf16 through the C ABI
(every output between sentinel guard regions, a guard behind the workspace) and the binding ops.dcn_v2 under
torch.use_deterministic_algorithms / ops.set_dcn_deterministic.

grad_input is a 64-bit fixed-point sum with one binary exponent per image (csrc/dcn_op.hip): the tests ask for the
accuracy of the float form (the project's op-level bar for fp32, the derived bf16 bound of tests/test_gpu_dcn_bf16.py), for exact
results where every contribution lies on the grid, for sums no float order survives, for the worst case of the overflow argument,
and for the same bits on every launch and in every batch.  The other four gradients must have the bits of the float entry."""
import numpy as np
import pytest
import torch

from m3dssd_amd import _hip
from gpu_common import *  # noqa: F401,F403
import dcn_bf16_cases as C
import dcn_grad_ref as R
import exact_inputs as X
from test_gpu_dcn_backward import BOUND, PARITY_CASES as F32_PARITY_CASES
from test_gpu_dcn_bf16 import PARITY_CASES as BF16_PARITY_CASES
from test_gpu_dcn_bf16 import Guarded, _bf16_case, _bits, _bounded, _parity_refs

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NAMES = ("input", "offset", "mask", "weight", "bias")
WS_GUARD = 256             # bytes behind the workspace
WS_SENT = 0xA5
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])


class Problem:
    """Device copies of one case (x / weight / grad_output in the compute type, offsets / masks / bias float32) and a workspace with
    a sentinel guard behind it; `det` picks the deterministic or the float entry of the type."""

    def __init__(self, ts, go, args, bf16, det=True):
        dev = _dev()
        x, off, m, wt, b = ts
        self.bf16, self.det = bf16, det
        self.dt = BF16 if bf16 else F32
        self.kdt = (self.dt, F32, F32, self.dt, F32)
        self.stride, self.pad, self.dil, self.G = args
        self.n, self.c, self.h, self.w = x.shape
        self.co, _, self.kh, self.kw = wt.shape
        self.shapes = (tuple(x.shape), tuple(off.shape), tuple(m.shape), tuple(wt.shape), (self.co,))
        d = lambda t, dt: t.detach().to(dev).contiguous().to(dt)              # noqa: E731
        self.x, self.wt, self.go = d(x, self.dt), d(wt, self.dt), d(go, self.dt)
        self.off, self.m = d(off, F32), d(m, F32)
        self.L = L = _hip.lib()
        name = "m3d_dcn_v2_backward" + ("_det" if det else "")
        self.fn = getattr(L, name + ("_bf16" if bf16 else ""))
        self.query = getattr(L, name + "_workspace_bytes" + ("_bf16" if bf16 else ""))
        self.nbytes = self.query(self.n, self.c, self.h, self.w, self.co, self.kh, self.kw, self.stride, self.pad, self.dil, self.G)
        assert self.nbytes > 0 and self.nbytes % 256 == 0
        self.raw = torch.full((256 + self.nbytes + WS_GUARD,), WS_SENT, dtype=torch.uint8, device=dev)
        self.lead = (-self.raw.data_ptr()) % 256
        self.base = self.raw.data_ptr() + self.lead

    def fill_workspace(self, value):
        self.raw[self.lead:self.lead + self.nbytes].view(F32).fill_(value)

    def workspace_guard_stands(self):
        return bool((self.raw[self.lead + self.nbytes:self.lead + self.nbytes + WS_GUARD] == WS_SENT).all())

    def call(self, ptrs, nbytes=None, dil=None, G=None):
        dil = self.dil if dil is None else dil
        tail = (self.n, self.c, self.h, self.w, self.co, self.kh, self.kw, self.stride, self.stride, self.pad, self.pad, dil, dil,
                self.G if G is None else G, self.base, self.nbytes if nbytes is None else nbytes, _stream())
        p = lambda t: t.data_ptr()                                           # noqa: E731
        if self.bf16:
            rc = self.fn(p(self.x), p(self.wt), p(self.off), 0, p(self.m), 0, p(self.go), *ptrs, *tail)
        else:
            rc = self.fn(p(self.x), p(self.wt), p(self.off), p(self.m), p(self.go), *ptrs, *tail)
        torch.cuda.synchronize()
        return rc

    def run(self, want=(1, 1, 1, 1, 1), fill=None):
        bufs = [Guarded(int(np.prod(s)), dt, fill) if wnt else None for s, dt, wnt in zip(self.shapes, self.kdt, want)]
        rc = self.call([b.ptr if b is not None else None for b in bufs])
        assert rc == 0, self.L.m3d_last_error().decode()
        assert self.workspace_guard_stands(), "write beyond the workspace"
        return [b.get().view(s) if b is not None else None for b, s in zip(bufs, self.shapes)]


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _relerr1(got, ref):
    """max |got - ref| / (1 + |ref|): the quantity of the project's op-level bar"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float(((got - ref).abs() / (1.0 + ref.abs())).max())


# ======================================================================================== 1. parity
# the first seven fp32 parity cases; the sigma-13 case on the 16x40 map that the issue names is the sixth of them
F32_CASES = list(dict.fromkeys(F32_PARITY_CASES[:7] + [(1, 64, 64, 16, 40, 3, 1, 1, 1, 1, 13.0, 15)]))


@pytest.mark.parametrize("spec", F32_CASES)
def test_fp32_parity_with_the_float64_reference(spec):
    ts, go, args = R.make_case(*spec)
    _, refs = R.ref_grads(ts, go, args)
    det = Problem(ts, go, args, False).run()
    flt = Problem(ts, go, args, False, det=False).run()
    e_det, e_flt = _relerr1(det[0], refs[0]), _relerr1(flt[0], refs[0])
    print("det parity %s: grad_input det %.3e float %.3e" % (spec, e_det, e_flt))
    _log("dcn_det", {"case": "fp32 parity %s" % (spec,), "grad_input_det": e_det, "grad_input_float": e_flt})
    assert e_det <= BOUND, (spec, e_det)
    for i in range(1, 5):
        assert _same_bits(det[i], flt[i]), NAMES[i]


@pytest.mark.parametrize("spec", BF16_PARITY_CASES)
def test_bf16_parity_with_the_float64_reference(spec):
    """grad_input under the derived bound of tests/test_gpu_dcn_bf16.py: |got - ref| <= 1.05 u (2 S + |ref|)."""
    ts, go, args = _bf16_case(spec)
    _, refs, _, s_grads, _, _ = _parity_refs(ts, go, args)
    det = Problem(ts, go, args, True).run()
    flt = Problem(ts, go, args, True, det=False).run()
    r_det = _bounded("det", det[0], refs[0], 2 * s_grads[0])
    r_flt = _bounded("float", flt[0], refs[0], 2 * s_grads[0])
    print("det parity bf16 %s: grad_input err / bound det %.3f float %.3f" % (spec, r_det, r_flt))
    _log("dcn_det", {"case": "bf16 parity %s" % (spec,), "grad_input_det": r_det, "grad_input_float": r_flt})
    assert r_det <= 1.0, (spec, r_det)
    for i in range(1, 5):
        assert _same_bits(det[i], flt[i]), NAMES[i]


# ======================================================================================== 2. exact on the lattice
@DTYPES
@pytest.mark.parametrize("spec", C.EXACT_BWD_CASES)
def test_backward_is_exact_on_the_lattice(spec, bf16):
    """Every contribution is a multiple of 1/64 of magnitude at most 64 (tests/dcn_bf16_cases.py); the bound of an image is
    2 * 32 * 1 = 64 at most, so 2^-s_n <= 2^(8 + 10 - 62): the contributions lie on the grid, the integer sum is exact, and the
    result is the float64 gradient rounded once to the stored type."""
    _, go, ts, args = C.exact_bwd_case(spec)
    _, refs = C.ref_grads64(ts, go, args)
    pr = Problem(ts, go, args, bf16)
    grads = pr.run()
    for name, g, r, dt in zip(NAMES, grads, refs, pr.kdt):
        bad, msg = X.compare_exact(g, r, dt)
        assert bad == 0, "grad_%s: %s" % (name, msg)


# ======================================================================================== 3. / 4. one element takes everything
H8, C8, K3 = 8, 8, 3
T8 = H8 * H8 * K3 * K3          # 576 contributions to one element
TARGET = (3, 4)


def _all_taps_to(ty, tx):
    """Integer offsets [1, 18, 8, 8] that send every tap of every output pixel of the 8x8 map (3x3, pad 1) to pixel (ty, tx)."""
    off = torch.zeros(1, 2 * K3 * K3, H8, H8)
    ys, xs = torch.arange(H8).view(H8, 1).float() - 1, torch.arange(H8).view(1, H8).float() - 1
    for tap in range(K3 * K3):
        i, j = divmod(tap, K3)
        off[0, 2 * tap] = ty - (ys + i)
        off[0, 2 * tap + 1] = tx - (xs + j)
    return off


@DTYPES
def test_cancellation_that_no_float_order_survives(bf16):
    """Co = 1, grad_out = 1 except one pixel of -1, weights 2^-c in channel c, masks 0 / 1 except 2^24 on one tap of two pixels:
    element (c, 3, 4) receives +2^24 2^-c, 320 times 2^-c and -2^24 2^-c (the corner weight of an integer coordinate is 1), and must
    be 320 * 2^-c.  A float accumulator that holds 2^24 drops every 1 that arrives before the -2^24.  320 = 5 * 2^6 has three
    significant bits: bf16 holds it."""
    ones = 320
    x = torch.zeros(1, C8, H8, H8)
    wt = (2.0 ** -torch.arange(C8).float()).view(1, C8, 1, 1).expand(1, C8, K3, K3).contiguous()
    go = torch.ones(1, 1, H8, H8)
    m = torch.zeros(H8 * H8, K3 * K3)
    p_pos, p_neg = 5, 50
    go.view(-1)[p_neg] = -1.0
    m[p_pos, 4] = 2.0 ** 24
    m[p_neg, 7] = 2.0 ** 24                                                  # the other taps of the negative pixel stay 0
    free = [(p, k) for p in range(H8 * H8) for k in range(K3 * K3) if p != p_neg and (p, k) != (p_pos, 4)]
    pick = torch.randperm(len(free), generator=torch.Generator().manual_seed(3))[:ones]
    for i in pick.tolist():
        m[free[i]] = 1.0
    m = m.t().reshape(1, K3 * K3, H8, H8).contiguous()
    ts = (x, _all_taps_to(*TARGET), m, wt, torch.zeros(1))
    gi = Problem(ts, go, (1, 1, 1, 1), bf16).run(want=(1, 0, 0, 0, 0))[0].float()
    want = torch.zeros(1, C8, H8, H8)
    want[0, :, TARGET[0], TARGET[1]] = ones * 2.0 ** -torch.arange(C8).float()
    assert torch.equal(gi, want), (gi[0, :, TARGET[0], TARGET[1]], gi.abs().sum())


@DTYPES
def test_the_worst_case_does_not_wrap(bf16):
    """Every one of the T = 576 contributions to one element is A W M itself, positive, with A W M = 2 - 2^-7 just below a power of
    two: the sum the overflow argument is about.  The result is T (2 - 2^-7) = 1147.5, rounded once for bf16."""
    v = 2.0 - 2.0 ** -7                                                      # eight significant bits: a bf16 value
    x = torch.zeros(1, C8, H8, H8)
    wt = torch.full((2, C8, K3, K3), 0.5)                                    # sum_co |W| = 1
    go = torch.full((1, 2, H8, H8), v)
    m = torch.ones(1, K3 * K3, H8, H8)
    ts = (x, _all_taps_to(*TARGET), m, wt, torch.zeros(2))
    gi = Problem(ts, go, (1, 1, 1, 1), bf16).run(want=(1, 0, 0, 0, 0))[0]
    want = torch.zeros(1, C8, H8, H8)
    want[0, :, TARGET[0], TARGET[1]] = T8 * v
    assert T8 * v == 1147.5
    assert torch.equal(gi.float(), want.to(gi.dtype).float()), gi[0, :, TARGET[0], TARGET[1]]


# ======================================================================================== 5. reproducible
@DTYPES
def test_twenty_launches_give_the_same_bits(bf16):
    make = _bf16_case if bf16 else (lambda spec: R.make_case(*spec))
    ts, go, args = make((2, 64, 64, 16, 40, 3, 1, 1, 1, 1, 3.0, 90))
    pr = Problem(ts, go, args, bf16)
    first = pr.run()
    assert torch.isfinite(first[0].float()).all() and first[0].float().abs().max() > 0
    for it in range(1, 20):
        fill = float("nan") if it % 2 else 1e30
        pr.fill_workspace(fill)
        cur = pr.run(fill=fill)                                              # garbage in outputs and workspace: both are overwritten
        for i in range(5):
            assert _same_bits(cur[i], first[i]), (it, NAMES[i])


# ======================================================================================== 6. batch invariance
@DTYPES
@pytest.mark.parametrize("spec", [(3, 20, 12, 9, 11, 3, 1, 1, 1, 2, 2.0, 140), (3, 64, 64, 16, 40, 3, 1, 1, 1, 1, 3.0, 141),
                                  (3, 16, 16, 7, 9, 1, 1, 0, 1, 1, 3.0, 142), (3, 8, 4, 10, 12, 3, 2, 1, 1, 2, 3.0, 143)])
def test_an_image_alone_and_in_a_batch_has_the_same_grad_input(spec, bf16):
    make = _bf16_case if bf16 else (lambda s: R.make_case(*s))
    ts, go, args = make(spec)
    x, off, m, wt, b = ts
    go = go.clone()
    go[1] *= 37.0                                                            # the images get different exponents
    go[2] *= 2.0 ** -9
    if bf16:
        go = go.to(BF16).float()
    whole = Problem((x, off, m, wt, b), go, args, bf16).run(want=(1, 0, 0, 0, 0))[0]
    for n in range(x.shape[0]):
        alone = Problem((x[n:n + 1], off[n:n + 1], m[n:n + 1], wt, b), go[n:n + 1], args, bf16).run(want=(1, 0, 0, 0, 0))[0]
        assert _same_bits(alone[0], whole[n]), n
    assert whole.float().abs().max() > 0


# ======================================================================================== 7. non-finite and zero data
@DTYPES
def test_non_finite_and_zero_grad_output(bf16):
    make = _bf16_case if bf16 else (lambda s: R.make_case(*s))
    ts, go, args = make((2, 20, 12, 9, 11, 3, 1, 1, 1, 2, 2.0, 150))
    clean = Problem(ts, go, args, bf16).run()
    bad = go.clone()
    bad[1, 5, 4, 6] = float("nan")
    got = Problem(ts, bad, args, bf16).run()
    assert torch.isnan(got[0][1].float()).all()
    assert _same_bits(got[0][0], clean[0][0])
    bad[1, 5, 4, 6] = float("inf")
    got = Problem(ts, bad, args, bf16).run(want=(1, 0, 0, 0, 0))
    assert torch.isnan(got[0][1].float()).all() and _same_bits(got[0][0], clean[0][0])
    zero = Problem(ts, torch.zeros_like(go), args, bf16).run(fill=float("nan"))
    for name, g in zip(NAMES, zero):
        assert not g.float().any(), name
    half = go.clone()
    half[0] = 0
    got = Problem(ts, half, args, bf16).run(want=(1, 0, 0, 0, 0), fill=float("nan"))[0]
    assert not got[0].float().any() and _same_bits(got[1], clean[0][1])


# ======================================================================================== 8. refusals
@DTYPES
def test_refusals_leave_the_outputs_untouched(bf16):
    make = _bf16_case if bf16 else (lambda s: R.make_case(*s))
    ts, go, args = make((2, 20, 12, 9, 11, 3, 1, 1, 1, 2, 2.0, 80))
    pr = Problem(ts, go, args, bf16)
    flt = Problem(ts, go, args, bf16, det=False)
    assert pr.nbytes >= flt.nbytes
    outs = [Guarded(int(np.prod(s)), dt) for s, dt in zip(pr.shapes, pr.kdt)]
    ptrs = [o.ptr for o in outs]
    assert pr.call(ptrs, nbytes=pr.nbytes - 1) == -3                         # M3D_E_WORKSPACE
    msg = pr.L.m3d_last_error().decode()
    assert str(pr.nbytes) in msg and str(pr.nbytes - 1) in msg and "det_workspace_bytes" in msg
    assert pr.nbytes > flt.nbytes and pr.call(ptrs, nbytes=flt.nbytes) == -3      # the float form's size is too small: the staging doubles
    assert pr.call(ptrs, G=3) == -1                                          # M3D_E_ARG: 3 does not divide 20
    assert "deformable_group" in pr.L.m3d_last_error().decode()
    if bf16:
        assert pr.call(ptrs, dil=2) == -1
        assert "dilation 1 only" in pr.L.m3d_last_error().decode()
    assert all(o.untouched() for o in outs)
    assert pr.workspace_guard_stands()
    assert pr.call([None] * 5) == 0                                          # nothing wanted: nothing to do


# ======================================================================================== 9. the binding
@DTYPES
def test_the_binding_follows_the_flag_and_the_switch(bf16):
    from m3dssd_amd.host import ops
    dev = _dev()
    make = _bf16_case if bf16 else (lambda s: R.make_case(*s))
    ts, go, args = make((2, 24, 20, 10, 14, 3, 1, 1, 1, 2, 2.0, 100))
    direct = Problem(ts, go, args, bf16).run()
    dt = BF16 if bf16 else F32

    def through_autograd():
        x, off, m, wt, b = ts
        lv = [x.to(dev).to(dt).requires_grad_(True), off.to(dev).requires_grad_(True), m.to(dev).requires_grad_(True),
              wt.to(dev).to(dt).requires_grad_(True), b.to(dev).requires_grad_(True)]
        out = ops.dcn_v2(*lv, *args)
        out.backward(go.to(dev).to(dt))
        return [t.grad.cpu() for t in lv]

    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    assert ops.set_dcn_deterministic(None) is None
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert ops.dcn_deterministic()
        flagged = through_autograd()
        torch.use_deterministic_algorithms(False)
        assert not ops.dcn_deterministic()
        ops.set_dcn_deterministic(True)
        switched = through_autograd()
    finally:
        ops.set_dcn_deterministic(None)
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])
    for got in (flagged, switched):
        for name, a, b in zip(NAMES, got, direct):
            assert a.dtype == b.dtype and _same_bits(a, b), name
    x, off, m, wt, b = ts
    explicit = ops.dcn_v2_backward(x.to(dev).to(dt), off.to(dev), m.to(dev), wt.to(dev).to(dt), go.to(dev).to(dt), *args, deterministic=True)
    assert _same_bits(explicit[0].cpu(), direct[0])


# ======================================================================================== 10. one training step, twice
def test_two_training_steps_from_one_seed_have_the_same_gradients():
    """anab_fullalign, DLA-34, 64x128, B = 2: forward + RPN_3D_loss + backward under torch.use_deterministic_algorithms, built twice
    from the same seed.  Every parameter gradient has passed through grad_input of a deformable layer or sits behind one."""
    from lib.loss.rpn_3d import RPN_3D_loss
    from m3dssd_amd import synth
    from m3dssd_amd.host import ops
    from model.M3d_inference_align import build
    import rpn_loss_ref as RR
    crop, B = (64, 128), 2
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
              torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    assert ops.set_dcn_deterministic(None) is None

    def step():
        conf = RR.loss_conf(crop, 0, device="cuda:0")
        flags = synth.config_flags("anab_fullalign")
        conf.update(flags)
        conf.batch_size = B
        net = build(conf, "train")
        net.load_state_dict(synth.synth_state_dict(0, back_bone="dla34", **flags), strict=True)
        net = net.to(_dev()).train()
        x = synth.synth_frames(B, crop, 1234).to(_dev())
        imobjs = RR.make_case(31, crop, B, 6)[4]
        cls, prob, b2, b3, fs = net(x)
        loss, _ = RPN_3D_loss(conf)(cls, prob, b2, b3, imobjs, fs)
        assert torch.isfinite(loss)
        loss.backward()
        return float(loss.detach()), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}

    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        assert ops.dcn_deterministic()
        loss_a, a = step()
        loss_b, b = step()
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before[2], before[3]
    assert loss_a == loss_b and a.keys() == b.keys() and len(a) > 100
    differ = [n for n in a if not _same_bits(a[n], b[n])]
    assert not differ, (len(differ), len(a), differ[:8])
    assert sum(bool(g.abs().max() > 0) for g in a.values()) > len(a) // 2
