"""The fused BatchNorm + residual + activation training operator on the device: m3d_bn_act_train_forward / _backward against the
float64 composition of tests/bn_train_ref.py, reproducibility and isolation, argument errors, the autograd layer
(``ops.bn_act_train``), the wiring behind ``train.set_fused_batchnorm``, whole-network gradients and one iteration followed by eval.

Bound of the operator comparisons (the rule of tests/test_gpu_anab_train.py): per tensor err = max|got - ref64| / max|ref64|, and
err_op <= 4 * err_torch32 + 2^-20, where err_torch32 is the error of the float32 torch composition computed in the same test on
the device: both are float32 evaluations of the same sums in different orders; a dropped chunk or a wrong term shows at 1e-3 and
above.  Measured margins: docs/LAB_NOTES.md section 19."""
import functools
import itertools

import pytest
import torch
from torch import nn

from gpu_common import _dev, _log, _stream
from m3dssd_amd import _hip, synth
from m3dssd_amd.host import ops, train
from m3dssd_amd.host.dla import BasicBlock, DeformConv, Tree

import bn_train_ref as R
import poison
import rpn_loss_ref as RR

pytestmark = pytest.mark.gpu

GUARD = 7.25
PAD = 4                             # floats of GUARD in front of and behind every output (16 bytes: the alignment is kept)
CANARY = 4096                       # bytes behind the workspace size the library asks for, watched by every _run
E_ARG = _hip.CONSTANTS["M3D_E_ARG"]


def _err(got, ref):
    return ((got.detach().double().cpu().reshape(-1) - ref.double().cpu().reshape(-1)).abs().max() / ref.double().abs().max()).item()


def _bound(e32):
    return 4.0 * e32 + 2.0 ** -20


@functools.lru_cache(maxsize=None)
def _case(i):
    """The case, the float64 yardstick and the errors of the float32 torch composition on the device."""
    c = R.make_case(i)
    ref64 = R.ref_grads(c, torch.float64, "cpu")
    t32 = R.ref_grads(c, torch.float32, _dev())
    e32 = {n: _err(t32[n], ref64[n]) for n in R.NAMES if ref64[n] is not None}
    return c, ref64, e32


@functools.lru_cache(maxsize=None)
def _canary():
    return (torch.arange(CANARY, device=_dev()) % 251).to(torch.uint8)


class _Guarded:
    """``numel`` floats with PAD floats of GUARD on either side; ``shift`` more floats in front move the payload off 16 bytes."""

    def __init__(self, numel, shift=0, init=None):
        self.lo, self.numel = PAD + shift, numel
        self.buf = torch.full((self.lo + numel + PAD,), GUARD, device=_dev())
        if init is not None:
            self.view().copy_(init.reshape(-1))

    def view(self):
        return self.buf[self.lo:self.lo + self.numel]

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def untouched_outside(self):
        return bool((self.buf[:self.lo] == GUARD).all()) and bool((self.buf[self.lo + self.numel:] == GUARD).all())

    def untouched(self):
        return bool((self.buf == GUARD).all())


def _workspace(nbytes, fill):
    """Exactly ``nbytes`` at a 256-byte boundary, poisoned with a tests/poison.py pattern (float64 words: NaN / 1.4e306), and CANARY
    bytes behind it."""
    ws = torch.zeros((nbytes + 256 + CANARY + 7) // 8, device=_dev(), dtype=torch.float64)
    if fill is not None:
        poison.poison_(ws, fill)
    u8 = ws.view(torch.uint8)
    base = (ws.data_ptr() + 255) // 256 * 256
    end = base - ws.data_ptr() + nbytes
    u8[end:end + CANARY] = _canary()
    return u8, base, end


def _run(i, needs=(True, True, True, True), ws_fill=None, shift=0, grad_y=None, forward_only=False, slope=None, ws_short=0, shape=None):
    """Forward and backward of case ``i`` through the C ABI.  Every tensor the kernels write lies in a GUARD-filled buffer; the
    workspace has exactly the size the library asks for.  ``shift``: floats by which x, residual, grad_y and the outputs are moved off
    their 16-byte boundary.  Returns ({name: flat tensor or None}, status of the forward, status of the backward); an argument
    error (``slope`` / ``ws_short`` / ``shape`` overrides) leaves the outputs to be checked by the caller in ``res['_bufs']``."""
    c, _, _ = _case(i)
    B, C, H, W = shape or c.shape
    n = B * C * H * W
    L, dev = _hip.lib(), _dev()
    slope = c.slope if slope is None else slope
    src = {k: getattr(c, k).to(dev) for k in ("x", "gamma", "beta", "grad_y")}
    if grad_y is not None:
        src["grad_y"] = grad_y.to(dev)
    x, gy = (_Guarded(n, shift, src[k].reshape(-1)[:n]) for k in ("x", "grad_y"))
    res_in = _Guarded(n, shift, c.residual.to(dev).reshape(-1)[:n]) if c.residual is not None else None
    rm, rv = _Guarded(C, 0, c.running_mean[:C].to(dev)), _Guarded(C, 0, c.running_var[:C].to(dev))
    y, sm, si = _Guarded(n, shift), _Guarded(C), _Guarded(C)
    nbytes = L.m3d_bn_act_train_workspace_bytes(B, C, H, W)
    if nbytes < 0:                  # an unsupported shape: the calls must refuse it whatever the workspace is
        nbytes = 4096
    ws, base, end = _workspace(nbytes, ws_fill)
    rc_f = L.m3d_bn_act_train_forward(x.ptr(), None if res_in is None else res_in.ptr(), src["gamma"].data_ptr(), src["beta"].data_ptr(),
                                      rm.ptr(), rv.ptr(), y.ptr(), sm.ptr(), si.ptr(), B, C, H, W, R.EPS, R.MOMENTUM, slope, base,
                                      nbytes - ws_short, _stream())
    torch.cuda.synchronize()
    assert torch.equal(ws[end:end + CANARY], _canary()), "m3d_bn_act_train_forward wrote behind the workspace size it asks for"
    bufs = dict(y=y, save_mean=sm, save_invstd=si, running_mean=rm, running_var=rv)
    out = {k: v.view() for k, v in bufs.items()}
    rc_b = None
    if not forward_only:
        g = [_Guarded(n, shift) if needs[0] else None, _Guarded(n, shift) if needs[1] else None,
             _Guarded(C) if needs[2] else None, _Guarded(C) if needs[3] else None]
        ws, base, end = _workspace(nbytes, ws_fill)
        rc_b = L.m3d_bn_act_train_backward(gy.ptr(), x.ptr(), y.ptr(), src["gamma"].data_ptr(), sm.ptr(), si.ptr(),
                                           *(None if t is None else t.ptr() for t in g), B, C, H, W, slope, base, nbytes - ws_short,
                                           _stream())
        torch.cuda.synchronize()
        assert torch.equal(ws[end:end + CANARY], _canary()), "m3d_bn_act_train_backward wrote behind the workspace size it asks for"
        for k, t in zip(("grad_x", "grad_residual", "grad_gamma", "grad_beta"), g):
            out[k] = None if t is None else t.view()
            if t is not None:
                bufs[k] = t
    for k, t in bufs.items():
        assert t.untouched_outside(), k + ": bytes outside the tensor were written"
    out["_bufs"] = bufs
    return out, rc_f, rc_b


def _compare(tag, i, shift):
    c, ref64, e32 = _case(i)
    out, rc_f, rc_b = _run(i, ws_fill=("nan", "huge")[i % 2], shift=shift)
    assert rc_f == 0 and rc_b == 0, _hip.lib().m3d_last_error().decode()
    if c.slope < 1.0:
        # precondition of the comparison: both evaluations stand on the same side of every kink
        n_diff = int(((out["y"].cpu() > 0) != (ref64["y"].reshape(-1) > 0)).sum())
        assert n_diff == 0, "the sign of %d pre-activations differs from float64: choose another seed" % n_diff
    errs = {}
    for name in R.NAMES:
        if ref64[name] is None:
            continue
        assert torch.isfinite(out[name]).all(), name + " is not finite"
        errs[name] = (_err(out[name], ref64[name]), e32[name])
    print("bn_train " + tag, R.CASES[i], errs)
    _log("bn_train_" + tag, {"case": list(R.CASES[i]), "errs": {k: list(v) for k, v in errs.items()}})
    for name, (e_op, e) in errs.items():
        assert e_op <= _bound(e), "%s: err %.3e > 4 * %.3e + 2^-20" % (name, e_op, e)


# ------------------------------------------------------------------------------------ 1. operator against float64
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.IDS)
def test_operator_matches_float64(i):
    B, C, H, W = R.make_case(i).shape
    L = _hip.lib()
    chunks = L.m3d_bn_act_train_chunks(B, C, H, W)
    assert chunks >= 1 and L.m3d_bn_act_train_workspace_bytes(B, C, H, W) == 16 * C * chunks
    if i == 5:
        # several chunks per channel and a ragged last one; the chunk size is asked of the library: the largest N with one chunk
        size = next(n for n in range(2, 1 << 20) if L.m3d_bn_act_train_chunks(1, 1, 1, n + 1) == 2)
        assert chunks == -(-B * H * W // size) and chunks > 1 and (B * H * W) % size != 0, (chunks, size)
    _compare("operator", i, 0)


@pytest.mark.parametrize("i", [2, 5, 7], ids=[R.IDS[i] for i in (2, 5, 7)])
def test_operator_matches_float64_off_16_byte_boundaries(i):
    """H*W % 4 == 0 but every big tensor starts 4 bytes past a 16-byte boundary: the one-element-per-lane kernels run."""
    assert (R.CASES[i][2] * R.CASES[i][3]) % 4 == 0
    _compare("unaligned", i, 1)


# ------------------------------------------------------------------------------------ 2. reproducibility and isolation
def _same_bits(a, b, what):
    for name in R.NAMES:
        if a.get(name) is None or b.get(name) is None:
            continue
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), "%s: %s differs in bits" % (what, name)


@pytest.mark.parametrize("i", [1, 2, 5, 8], ids=[R.IDS[i] for i in (1, 2, 5, 8)])
def test_bits_do_not_depend_on_the_launch_or_the_workspace(i):
    first, rc_f, rc_b = _run(i)
    assert rc_f == 0 and rc_b == 0
    _same_bits(first, _run(i)[0], "a second run")
    for fill in ("nan", "huge", "zero"):
        _same_bits(first, _run(i, ws_fill=fill)[0], "a workspace poisoned with %r" % fill)


@pytest.mark.parametrize("i", [2, 3, 5], ids=[R.IDS[i] for i in (2, 3, 5)])
def test_each_subset_of_gradients_gives_the_same_bits(i):
    full, _, _ = _run(i, ws_fill="nan")
    for needs in itertools.product((False, True), repeat=4):
        part, rc_f, rc_b = _run(i, needs=needs, ws_fill="huge")
        assert rc_f == 0 and rc_b == 0, needs
        for name, need in zip(("grad_x", "grad_residual", "grad_gamma", "grad_beta"), needs):
            assert (part[name] is not None) == need
        _same_bits(full, part, "gradients %s alone" % (needs,))


# ------------------------------------------------------------------------------------ 3. argument errors
@pytest.mark.parametrize("what,kw", [("N = 1", dict(shape=(1, 4, 1, 1))), ("slope -0.1", dict(slope=-0.1)), ("slope 1.5", dict(slope=1.5)),
                                     ("short workspace", dict(ws_short=1))], ids=["n1", "slope_neg", "slope_big", "short_ws"])
def test_argument_errors_launch_nothing(what, kw):
    out, rc_f, rc_b = _run(2, ws_fill="nan", **kw)
    msg = _hip.lib().m3d_last_error().decode()
    print(what, "->", rc_f, rc_b, msg)
    assert rc_f == E_ARG and rc_b == E_ARG and msg
    for name in ("y", "save_mean", "save_invstd", "grad_x", "grad_residual", "grad_gamma", "grad_beta"):
        assert out["_bufs"][name].untouched(), "%s was written by a refused call (%s)" % (name, what)
    c = R.make_case(2)
    C = kw.get("shape", c.shape)[1]
    assert torch.equal(out["running_mean"].cpu(), c.running_mean[:C]) and torch.equal(out["running_var"].cpu(), c.running_var[:C])
    if "shape" in kw:
        assert _hip.lib().m3d_bn_act_train_workspace_bytes(*kw["shape"]) == -1 and _hip.lib().m3d_bn_act_train_chunks(*kw["shape"]) == -1


def test_null_pointers_are_refused():
    c, _, _ = _case(2)
    B, C, H, W = c.shape
    L, dev = _hip.lib(), _dev()
    t = {k: getattr(c, k).to(dev) for k in ("x", "gamma", "beta", "grad_y")}
    y, sm, si = torch.full(c.shape, GUARD, device=dev), torch.full((C,), GUARD, device=dev), torch.full((C,), GUARD, device=dev)
    nbytes = L.m3d_bn_act_train_workspace_bytes(B, C, H, W)
    ws = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    fwd = [t["x"].data_ptr(), None, t["gamma"].data_ptr(), t["beta"].data_ptr(), None, None, y.data_ptr(), sm.data_ptr(), si.data_ptr()]
    for k in (0, 2, 3, 6, 7, 8):
        a = list(fwd)
        a[k] = None
        assert L.m3d_bn_act_train_forward(*a, B, C, H, W, R.EPS, R.MOMENTUM, c.slope, ws.data_ptr(), nbytes, _stream()) == E_ARG, k
    assert L.m3d_bn_act_train_forward(*fwd, B, C, H, W, R.EPS, R.MOMENTUM, c.slope, None, nbytes, _stream()) == E_ARG
    bwd = [t["grad_y"].data_ptr(), t["x"].data_ptr(), y.data_ptr(), t["gamma"].data_ptr(), sm.data_ptr(), si.data_ptr()]
    gx = torch.full(c.shape, GUARD, device=dev)
    for k in range(6):
        a = list(bwd)
        a[k] = None
        assert L.m3d_bn_act_train_backward(*a, gx.data_ptr(), None, None, None, B, C, H, W, c.slope, ws.data_ptr(), nbytes, _stream()) == E_ARG, k
    torch.cuda.synchronize()
    assert all(bool((v == GUARD).all()) for v in (y, sm, si, gx))
    # without running statistics and without a residual the call is valid
    _hip.check(L.m3d_bn_act_train_forward(*fwd, B, C, H, W, R.EPS, R.MOMENTUM, c.slope, ws.data_ptr(), nbytes, _stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and not bool((y == GUARD).all())


# ------------------------------------------------------------------------------------ 4. autograd layer
def _through_ops(i, x_layout, expanded, frozen=False):
    c, _, _ = _case(i)
    dev = _dev()
    if x_layout == "strided":                   # every other column of a wider tensor
        wide = torch.zeros(*c.shape[:3], 2 * c.shape[3], device=dev)
        wide[..., ::2] = c.x.to(dev)
        x = wide[..., ::2]
    else:                                       # channels-last memory behind an NCHW view
        x = c.x.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not x.is_contiguous() and torch.equal(x, c.x.to(dev))
    x.requires_grad_(True)
    residual = c.residual.to(dev).requires_grad_(True) if c.residual is not None else None
    w, b = c.gamma.to(dev).requires_grad_(not frozen), c.beta.to(dev).requires_grad_(not frozen)
    rm, rv = c.running_mean.to(dev), c.running_var.to(dev)
    y = ops.bn_act_train(x, residual, w, b, rm, rv, R.MOMENTUM, R.EPS, c.slope)
    if expanded:
        (y.sum() * 0.37).backward()             # grad_out is an expanded scalar: every stride is 0
    else:
        y.backward(c.grad_y.to(dev))
    return dict(y=y.detach().reshape(-1), grad_x=x.grad.reshape(-1), grad_residual=None if residual is None else residual.grad.reshape(-1),
                grad_gamma=w.grad, grad_beta=b.grad, running_mean=rm, running_var=rv)


@pytest.mark.parametrize("i,x_layout,expanded", [(2, "strided", False), (2, "channels_last", True), (3, "strided", True), (4, "channels_last", False)])
def test_autograd_layer_equals_the_c_abi(i, x_layout, expanded):
    c, _, _ = _case(i)
    want, _, _ = _run(i, grad_y=torch.full(c.shape, 0.37) if expanded else None)
    got = _through_ops(i, x_layout, expanded)
    _same_bits(want, got, "ops.bn_act_train")
    frozen = _through_ops(i, x_layout, expanded, frozen=True)
    assert frozen["grad_gamma"] is None and frozen["grad_beta"] is None
    _same_bits(want, frozen, "ops.bn_act_train with frozen weight and bias")


def test_autograd_layer_refuses_other_dtypes():
    c, _, _ = _case(2)
    dev = _dev()
    args = [c.x.to(dev), c.residual.to(dev), c.gamma.to(dev), c.beta.to(dev), c.running_mean.to(dev), c.running_var.to(dev)]
    for k, dtype in ((0, torch.float16), (1, torch.bfloat16), (2, torch.float64)):
        a = list(args)
        a[k] = a[k].to(dtype)
        with pytest.raises(RuntimeError, match=str(dtype).replace("torch.", "")):
            ops.bn_act_train(*a, R.MOMENTUM, R.EPS, c.slope)
    assert torch.equal(args[4].cpu(), c.running_mean)


# ------------------------------------------------------------------------------------ 5. wiring
def _build(crop, B, phase="train", conf=None):
    from model.M3d_inference_align import build
    flags = synth.config_flags("anab_fullalign")
    if conf is None:
        conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0", back_bone="dla34", **flags)
    net = build(conf, phase)
    net.load_state_dict(synth.synth_state_dict(0, back_bone="dla34", **flags), strict=True)
    return net.to(_dev()), conf


def _weighted_sum(out, seed):
    g = torch.Generator().manual_seed(seed)
    return sum((t * torch.randn(t.shape, generator=g).to(t.device)).sum() for t in out[:4])


class _Calls:
    """Counts the calls of F.batch_norm (by the module handed over: the BatchNorm2d whose weight it is) and of ops.bn_act_train."""

    def __init__(self, monkeypatch, net):
        self.torch_bn, self.fused = [], []
        names = {id(m.weight): n for n, m in net.named_modules() if isinstance(m, nn.BatchNorm2d)}
        real_bn, real_op = torch.nn.functional.batch_norm, ops.bn_act_train

        def batch_norm(inp, running_mean, running_var, weight=None, *args, **kwargs):
            self.torch_bn.append(names.get(id(kwargs.get("weight", weight)), "?"))
            return real_bn(inp, running_mean, running_var, weight, *args, **kwargs)

        def bn_act_train(x, residual, weight, *args, **kwargs):
            self.fused.append(names.get(id(weight), "?"))
            return real_op(x, residual, weight, *args, **kwargs)

        monkeypatch.setattr(torch.nn.functional, "batch_norm", batch_norm)
        monkeypatch.setattr(ops, "bn_act_train", bn_act_train)

    def reset(self):
        self.torch_bn, self.fused = [], []


def test_wiring(monkeypatch):
    crop, B = (64, 128), 2
    net, conf = _build(crop, B)
    x = synth.synth_frames(B, crop, 77).to(_dev())
    bns = {n: m for n, m in net.named_modules() if isinstance(m, nn.BatchNorm2d)}
    calls = _Calls(monkeypatch, net)
    # flag off: every site is torch's
    _weighted_sum(net(x), 5).backward()
    off = sorted(calls.torch_bn)
    had_grad = {n for n, p in net.named_parameters() if p.grad is not None}
    assert calls.fused == [] and len(off) == len(set(off)) and "?" not in off
    assert set(off) == set(bns), "a BatchNorm2d of the net is not reached by the training forward"
    # flag on: none is
    for m in bns.values():
        m.reset_running_stats()
    assert train.set_fused_batchnorm(net) == len(off)
    net.zero_grad(set_to_none=True)
    calls.reset()
    _weighted_sum(net(x), 5).backward()
    assert calls.torch_bn == [], calls.torch_bn
    assert sorted(calls.fused) == off
    assert all(int(m.num_batches_tracked) == 1 for m in bns.values())
    grads = {n: p.grad for n, p in net.named_parameters()}
    assert {n for n, g in grads.items() if g is not None} == had_grad
    assert all(torch.isfinite(grads[n]).all() for n in had_grad)
    dropped = {"%s.project.%s" % (name, k) for name, m in net.named_modules() if isinstance(m, Tree) and m.levels > 1 and m.project is not None
               for k, _ in m.project.named_parameters()}
    assert len(dropped) > 1 and all(grads[n] is None for n in dropped)
    # a frozen layer (eval mode) goes back to torch, and only that one
    frozen = "base.base.level3.tree1.tree2.bn1"
    bns[frozen].eval()
    calls.reset()
    net(x)
    assert calls.torch_bn == [frozen] and sorted(calls.fused + [frozen]) == off
    bns[frozen].train()
    # the other conditions that keep the torch layers: no momentum, no running statistics
    bns[frozen].momentum = None
    calls.reset()
    net(x)
    assert calls.torch_bn == [frozen]
    bns[frozen].momentum = 0.1
    # under bfloat16 autocast the flag changes nothing
    calls.reset()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        net(x)
    assert calls.fused == [] and sorted(calls.torch_bn) == off
    train.set_fused_batchnorm(net, False)
    calls.reset()
    net(x)
    assert calls.fused == [] and sorted(calls.torch_bn) == off


# ------------------------------------------------------------------------------------ 6. whole-network gradients
@pytest.fixture
def deterministic_torch():
    """The recipe of tests/test_gpu_train_mode.py: with it two passes of the same code are bit-identical."""
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
              torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.use_deterministic_algorithms(before[0], warn_only=before[1])
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before[2], before[3]


def _bn_functional(x, w, b, eps):
    return torch.nn.functional.batch_norm(x, None, None, w, b, True, 0.0, eps)


def _bn_by_hand(x, w, b, eps):
    mean = x.mean((0, 2, 3), keepdim=True)
    var = x.var((0, 2, 3), unbiased=False, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def _value_of_hip_gradient_of(bn_core):
    """``ops.bn_act_train`` with the VALUE of the HIP forward and the GRADIENT of the torch composition around ``bn_core``, the
    activation written as z * where(y_hip > 0, 1, slope): the same piecewise-linear function at the same point."""
    def swapped(x, residual, weight, bias, running_mean, running_var, momentum, eps, slope):
        class Swapped(torch.autograd.Function):
            @staticmethod
            def forward(ctx, *ts):
                y = ops.bn_act_train_forward(ts[0], ts[3] if len(ts) > 3 else None, ts[1], ts[2], running_mean, running_var, momentum,
                                             eps, slope)
                ctx.save_for_backward(y, *ts)
                return y

            @staticmethod
            def backward(ctx, go):
                y, *ts = ctx.saved_tensors
                ts = [t.detach().requires_grad_(True) for t in ts]
                with torch.enable_grad():
                    z = bn_core(ts[0], ts[1], ts[2], eps)
                    if len(ts) > 3:
                        z = z + ts[3]
                    out = z * torch.where(y > 0, 1.0, slope).to(z.dtype)
                return torch.autograd.grad(out, ts, go)

        return Swapped.apply(x, weight, bias, *(() if residual is None else (residual,)))

    return swapped


def _biases_in_front_of_batchnorm(net):
    """Their gradient is exactly zero (the mean subtraction removes a constant), and so is that of center_align2d's bias, whose
    output feeds 1x1 convolutions in front of a BatchNorm only (tests/test_gpu_train_mode.py)."""
    names = {"center_align2d.align.bias"}
    for name, m in net.named_modules():
        if isinstance(m, BasicBlock):
            names |= {name + ".conv1.bias", name + ".conv2.bias"}
        elif isinstance(m, DeformConv):
            names.add(name + ".conv.bias")
        elif isinstance(m, nn.Sequential) and len(m) == 7 and isinstance(m[1], nn.BatchNorm2d):
            names |= {name + ".0.bias", name + ".3.bias"}
    return names


def test_whole_network_gradients(monkeypatch, deterministic_torch):
    """A: the operator.  B: its value with autograd's gradient through F.batch_norm.  C: as B with batch-norm written out by hand.
    worst(A vs B) <= 4 * worst(B vs C) + 2^-20: the yardstick is the distance between two float32 torch evaluations of the same
    gradients, independent of the code under test; 4 is the project's margin for another order of the same float32 sums."""
    crop, B = (64, 128), 2
    net, conf = _build(crop, B)
    x = synth.synth_frames(B, crop, 77).to(_dev())
    assert train.set_fused_batchnorm(net) > 0
    start = {k: v.clone() for k, v in net.state_dict().items()}

    def run():
        net.load_state_dict(start)                  # the running statistics of the previous run
        net.train()
        net.zero_grad(set_to_none=True)
        out = net(x)
        _weighted_sum(out, 9).backward()
        return {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, [t.detach() for t in out[:4]]

    ga, out_a = run()
    monkeypatch.setattr(ops, "bn_act_train", _value_of_hip_gradient_of(_bn_functional))
    gb, out_b = run()
    monkeypatch.setattr(ops, "bn_act_train", _value_of_hip_gradient_of(_bn_by_hand))
    gc, out_c = run()
    monkeypatch.undo()
    for other in (out_b, out_c):
        assert all(torch.equal(a, b) for a, b in zip(out_a, other)), "the forwards are not the same function value"
    assert ga.keys() == gb.keys() == gc.keys()
    zero = _biases_in_front_of_batchnorm(net)
    assert all(n in ga for n in zero)

    def figures(got, ref):
        def scale(n):
            return ref[n[:-len("bias")] + "weight" if n in zero else n].abs().max().clamp_min(1e-30)
        errs = {n: ((got[n] - ref[n]).abs().max() / scale(n)).item() for n in got}
        return sorted(errs.items(), key=lambda kv: -kv[1])

    ab, bc, ac = figures(ga, gb), figures(gb, gc), figures(ga, gc)
    fig = dict(a_vs_b=ab[:4], b_vs_c=bc[:4], a_vs_c=ac[:4], median_a_vs_b=ab[len(ab) // 2][1], median_b_vs_c=bc[len(bc) // 2][1],
               tensors=len(ab))
    print("bn_train whole-network gradients:", fig)
    _log("bn_train_whole_network_gradients", fig)
    assert all(torch.isfinite(g).all() for g in ga.values())
    assert ab[0][1] <= 1e-2, "a wiring error, whatever the yardstick says: %s" % (ab[:4],)
    assert ab[0][1] <= 4 * bc[0][1] + 2.0 ** -20, (ab[:4], bc[:4])


# ------------------------------------------------------------------------------------ 7. one iteration, then eval
def test_one_training_iteration_then_eval():
    from lib.loss.rpn_3d import RPN_3D_loss
    crop, B = (128, 320), 2
    conf = RR.loss_conf(crop, 0, device="cuda:0")
    conf.update(synth.config_flags("anab_fullalign"))
    conf.batch_size = B
    net, _ = _build(crop, B, conf=conf)
    x = synth.synth_frames(B, crop, 1234).to(_dev())
    imobjs = RR.make_case(31, crop, B, 6)[4]
    net.eval()
    with torch.no_grad():
        before = [t.clone() for t in net(x)]
    stats_before = {n: b.clone() for n, b in net.named_buffers() if n.endswith("running_mean") or n.endswith("running_var")}
    net.train()
    assert train.set_fused_batchnorm(net) == len(stats_before) // 2
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9)
    crit = RPN_3D_loss(conf)
    cls, prob, b2, b3, fs = net(x)
    loss, stats = crit(cls, prob, b2, b3, imobjs, fs)
    assert torch.isfinite(loss)
    opt.zero_grad()
    loss.backward()
    opt.step()
    net.eval()
    moved = [n for n, b in net.named_buffers() if n in stats_before and not torch.equal(b, stats_before[n])]
    assert len(moved) == len(stats_before), "running statistics the operator did not write: %s" % sorted(set(stats_before) - set(moved))[:4]
    with torch.no_grad():
        after = [t.clone() for t in net(x)]
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[3], before[3])
    fresh, _ = _build(crop, B, phase="test", conf=conf)
    fresh.load_state_dict(net.state_dict(), strict=True)
    fresh = fresh.to(_dev()).eval()
    with torch.no_grad():
        want = fresh(x)
    for a, b in zip(after, want):
        assert torch.equal(a, b)
