"""GPU tests (-m gpu) of the deformable PS-ROI pooling: m3d_dcn_v2_psroi_pooling_forward / _backward through the C ABI, the
autograd binding ops.psroi_pooling and the modules DCNv2PoolingFunction, DCNv2Pooling and DCNPooling.

Reference: tests/psroi_ref.py, a float64 autograd restatement of the definition whose coordinates are formed in float32 in the
documented order (pinned on the CPU by tests/test_psroi_host.py).  Bounds, from the roundings on the path (psroi_ref.py):
  forward, per output:   32 * 2^-24 * max|data|   (at most 24 roundings: three per corner weight, the products, the 4-term and the
                         16-term sums, one division);
  gradients, per element: (T + 16) * 2^-24 * A with T terms of absolute sum A (psroi_ref.grad_terms).
The lattice case has no rounding at all and is compared bit for bit.  Every output of a C-ABI call sits between sentinel-filled
guard regions."""
import functools

import numpy as np
import pytest
import torch

from m3dssd_amd import _hip
from gpu_common import _dev, _stream
import poison
import psroi_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = -559038737          # 0xDEADBEEF as int32
GUARD = 64                 # 4-byte elements on each side (256 bytes)
E_ARG, E_WORKSPACE = -1, -3


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
        return torch.from_numpy(raw[GUARD:GUARD + self.n].view(np.float32).copy())


class Problem:
    """Device copies of one case + a workspace; forward() / backward() launch the C-ABI calls and return CPU tensors."""

    def __init__(self, data, rois, trans, conf, ws_fill=None):
        dev = _dev()
        self.conf = conf
        self.no_trans, self.scale, self.D, self.G, self.P, self.part, self.S, self.std = conf
        self.N, self.C, self.H, self.W = data.shape
        self.n = rois.shape[0]
        self.data, self.rois = data.float().contiguous().to(dev), rois.float().contiguous().to(dev)
        self.trans = None if trans is None else trans.float().contiguous().to(dev)
        self.rows, self.K = (0, 1) if trans is None else (trans.shape[0], trans.shape[1] // 2)
        self.L = _hip.lib()
        q = (self.N, self.C, self.H, self.W, self.n, self.K, self.D, self.G, self.P)
        self.fbytes = self.L.m3d_dcn_v2_psroi_pooling_workspace_bytes(*q, 0)
        self.bbytes = self.L.m3d_dcn_v2_psroi_pooling_workspace_bytes(*q, 1)
        assert 0 <= self.fbytes <= self.bbytes
        self.ws = torch.zeros(self.bbytes + 256, device=dev, dtype=torch.uint8)
        if ws_fill is not None:
            poison.poison_(self.ws.view(torch.float32), ws_fill)
        self.base = (self.ws.data_ptr() + 255) // 256 * 256
        self.oshape = (self.n, self.D, self.P, self.P)

    def _tail(self, nbytes):
        return (self.N, self.C, self.H, self.W, self.n, self.rows, self.K, int(self.no_trans), self.scale, self.D, self.G, self.P,
                self.part, self.S, self.std, self.base, nbytes, _stream())

    def _p(self, t):
        return None if t is None else t.data_ptr()

    def forward_rc(self, out, cnt, nbytes=None):
        rc = self.L.m3d_dcn_v2_psroi_pooling_forward(self._p(self.data), self._p(self.rois), self._p(self.trans), out, cnt,
                                                     *self._tail(self.fbytes if nbytes is None else nbytes))
        torch.cuda.synchronize()
        return rc

    def forward(self, want_count=True):
        ne = int(np.prod(self.oshape))
        out, cnt = Guarded(ne), Guarded(ne) if want_count else None
        rc = self.forward_rc(out.ptr, cnt.ptr if cnt else None)
        assert rc == 0, self.L.m3d_last_error().decode()
        return out.get().view(self.oshape), cnt.get().view(self.oshape) if cnt else None

    def backward_rc(self, go, gd, gt, nbytes=None):
        rc = self.L.m3d_dcn_v2_psroi_pooling_backward(self._p(go), self._p(self.data), self._p(self.rois), self._p(self.trans), gd, gt,
                                                      *self._tail(self.bbytes if nbytes is None else nbytes))
        torch.cuda.synchronize()
        return rc

    def backward(self, go, want=(1, 1), fill=None):
        go = go.float().contiguous().to(_dev())
        gd = Guarded(self.data.numel(), fill) if want[0] else None
        gt = Guarded(self.trans.numel(), fill) if want[1] and self.trans is not None else None
        rc = self.backward_rc(go, gd.ptr if gd else None, gt.ptr if gt else None)
        assert rc == 0, self.L.m3d_last_error().decode()
        return (gd.get().view(self.data.shape) if gd else None), (gt.get().view(self.trans.shape) if gt else None)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ======================================================================================== the lattice case: bit for bit
@functools.lru_cache(maxsize=None)
def _lattice():
    data, rois, trans, go, conf = R.lattice_case()
    out, cnt, gd, gt = R.ref_grads(data, rois, trans, go, conf)
    return (data, rois, trans, go, conf), (out.float(), cnt.float(), gd.float(), gt.float())


def test_lattice_case_through_the_c_abi_is_exact():
    (data, rois, trans, go, conf), (out_r, cnt_r, gd_r, gt_r) = _lattice()
    pb = Problem(data, rois, trans, conf)
    out, cnt = pb.forward()
    assert torch.equal(out, out_r) and torch.equal(cnt, cnt_r)
    gd, gt = pb.backward(go)
    assert torch.equal(gd, gd_r), (gd - gd_r).abs().max()
    assert torch.equal(gt, gt_r), (gt - gt_r).abs().max()


def test_lattice_case_through_the_modules_is_exact():
    from model.DCNv2.dcn_v2 import DCNv2Pooling
    from m3dssd_amd.host import ops
    (data, rois, trans, go, conf), (out_r, cnt_r, gd_r, gt_r) = _lattice()
    dev = _dev()
    d, t = data.to(dev).requires_grad_(True), trans.to(dev).requires_grad_(True)
    m = DCNv2Pooling(conf[1], conf[4], conf[2], False, group_size=conf[3], part_size=conf[5], sample_per_part=conf[6], trans_std=conf[7])
    out = m(d, rois.to(dev), t)
    out.backward(go.to(dev))
    assert torch.equal(out.detach().cpu(), out_r) and torch.equal(d.grad.cpu(), gd_r) and torch.equal(t.grad.cpu(), gt_r)
    o2, c2 = ops.psroi_pooling_forward(data.to(dev), rois.to(dev), trans.to(dev), *conf)
    assert torch.equal(o2.cpu(), out_r) and torch.equal(c2.cpu(), cnt_r)
    with pytest.raises(RuntimeError):
        ops.psroi_pooling_forward(data.to(dev).bfloat16(), rois.to(dev), trans.to(dev), *conf)
    with pytest.raises(RuntimeError):
        ops.psroi_pooling_forward(data.to(dev), rois.to(dev), trans.to(dev), *conf[:7], 1.5)


# ======================================================================================== test.py's zero-offset case
def test_zero_offset_case_through_the_modules():
    from model.DCNv2.dcn_v2 import DCNv2Pooling, DCNPooling
    data, rois, c0, c1, trans = R.zero_offset_case()
    dev = _dev()
    ref, _ = R.psroi_ref(data.double(), rois, None, c0)
    pooling = DCNv2Pooling(spatial_scale=1.0 / 4, pooled_size=7, output_dim=16, no_trans=True, group_size=1, trans_std=0.1).to(dev)
    dpooling = DCNv2Pooling(spatial_scale=1.0 / 4, pooled_size=7, output_dim=16, no_trans=False, group_size=1, trans_std=0.1).to(dev)
    out = pooling(data.to(dev), rois.to(dev), data.new_empty(0).to(dev))
    dout = dpooling(data.to(dev), rois.to(dev), trans.to(dev))
    bound = 32 * U * 2.0
    print("zero offset: max err %.3e (bound %.3e), means %s" % ((out.cpu().double() - ref).abs().max(), bound,
                                                                 [out[i].mean().item() for i in range(2)]))
    assert (out.cpu().double() - ref).abs().max() <= bound
    for i, mean in enumerate(R.ZERO_OFFSET_MEANS):
        assert abs(out[i].double().mean().item() - mean) <= bound + 5e-8
    assert _bits_equal(out, dout)
    torch.manual_seed(0)
    md = DCNPooling(spatial_scale=1.0 / 4, pooled_size=7, output_dim=16, no_trans=False, group_size=1, trans_std=0.1, deform_fc_dim=32).to(dev)
    with torch.no_grad():
        got = md(data.to(dev), rois.to(dev))
    assert torch.equal(got, out * 0.5)


# ======================================================================================== random parity with the float64 restatement
def _case(which):
    g = torch.Generator().manual_seed(100 + which)
    if which == 1:          # test.py's gradient shape
        data = torch.randn(2, 3, 5, 5, generator=g) * 0.01
        b = torch.randint(2, (4, 1), generator=g).float()
        x, y = torch.rand(4, 1, generator=g) * 15, torch.rand(4, 1, generator=g) * 15
        w, h = torch.rand(4, 1, generator=g) * 10, torch.rand(4, 1, generator=g) * 10
        rois = torch.cat((b, x, y, x + w, y + h), 1)
        return data, rois, torch.randn(4, 2, 3, 3, generator=g), (False, 0.25, 3, 1, 3, 3, 4, 0.1)
    if which == 2:          # more than one wave of channels, not a multiple of 64; regions partly or wholly outside the map
        data = torch.randn(2, 70, 64, 64, generator=g)
        return data, R.make_rois(20, 2, 102), torch.randn(20, 2, 7, 7, generator=g), (False, 0.25, 70, 1, 7, 7, 4, 0.1)
    if which == 3:          # group cells, two classes, part cells of 2 x 2 bins, spare channels and a spare trans row
        data = torch.randn(2, 38, 24, 28, generator=g)
        rois = R.make_rois(6, 2, 103, xy_max=90, wh_max=60, integer=False)
        return data, rois, torch.randn(7, 4, 3, 3, generator=g), (False, 0.25, 4, 3, 6, 3, 2, 0.3)
    if which == 5:          # P = part = 23: the float32 part index differs from (ph * part) // P at ph = 7 and 14
        data = torch.randn(1, 2, 20, 24, generator=g)
        rois = torch.tensor([[0, 6, 4, 85, 70], [0, 20, 10, 60, 75]]).float()
        return data, rois, torch.randn(2, 2, 23, 23, generator=g), (False, 0.25, 2, 1, 23, 23, 2, 0.3)
    data = torch.randn(2, 4, 16, 16, generator=g)      # x2 < x1 (the 0.1 floor of the region size) and a single pixel
    rois = torch.tensor([[0, 40, 30, 20, 50], [1, 12, 12, 12, 12]]).float()
    return data, rois, torch.randn(2, 2, 3, 3, generator=g), (False, 0.25, 4, 1, 3, 3, 2, 0.2)


@functools.lru_cache(maxsize=None)
def _case_ref(which):
    """A case, its grad_out, the float64 reference (out, count, grad_data, grad_trans) and the term counts: computed once."""
    data, rois, trans, conf = _case(which)
    g = torch.Generator().manual_seed(200 + which)
    go = torch.randn(rois.shape[0], conf[2], conf[4], conf[4], generator=g)
    return (data, rois, trans, conf), go, R.ref_grads(data, rois, trans, go, conf), R.grad_terms(data, rois, trans, go, conf)


def _within(a, b, T, A, factor=1):
    """|a - b| <= factor * (T + 16) * 2^-24 * A in every element"""
    return ((a.double() - b.double()).abs() - factor * (T + 16) * U * A).max().item() <= 0


@pytest.mark.parametrize("which", [1, 2, 3, 4, 5])
def test_random_parity_with_the_float64_restatement(which):
    (data, rois, trans, conf), go, (out_r, cnt_r, gd_r, gt_r), (Td, Ad, Tt, At) = _case_ref(which)
    pb = Problem(data, rois, trans, conf)
    out, cnt = pb.forward()
    gd, gt = pb.backward(go)
    assert torch.equal(cnt.double(), cnt_r)
    assert (cnt_r > 0).any()
    if which == 2:
        assert (cnt_r == 0).any() and ((cnt_r > 0) & (cnt_r < 16)).any()
    if which == 5:          # the bins whose float32 part index is not (ph * part) // P are in use, and their offsets differ
        pidx = R.part_index(23, 23)
        odd = [q for q in range(23) if pidx[q] != q]
        assert odd == [7, 14] and (cnt_r[:, :, odd] > 0).any() and (cnt_r[:, :, :, odd] > 0).any()
        assert (trans[:, :, pidx[odd]] != trans[:, :, odd]).all()
    fb = 32 * U * data.abs().max().item()
    ferr = (out.double() - out_r).abs().max().item()
    derr = ((gd.double() - gd_r).abs() - (Td + 16) * U * Ad).max().item()
    terr = ((gt.double() - gt_r).abs() - (Tt + 16) * U * At).max().item()
    print("case %d: forward err %.3e (bound %.3e); grad_data excess %.3e, max err %.3e; grad_trans excess %.3e, max err %.3e"
          % (which, ferr, fb, derr, (gd.double() - gd_r).abs().max(), terr, (gt.double() - gt_r).abs().max()))
    assert torch.isfinite(out).all() and torch.isfinite(gd).all() and torch.isfinite(gt).all()
    assert ferr <= fb
    assert derr <= 0 and terr <= 0
    assert gd_r.any() and gt_r.any()
    # no_trans on the same regions: the forward and grad_data
    conf0 = (True,) + conf[1:]
    o0_r, c0_r, gd0_r, _ = R.ref_grads(data, rois, None, go, conf0)
    Td0, Ad0, _, _ = R.grad_terms(data, rois, None, go, conf0)
    p0 = Problem(data, rois, None, conf0)
    o0, c0 = p0.forward()
    gd0, gt0 = p0.backward(go)
    assert gt0 is None and torch.equal(c0.double(), c0_r) and (o0.double() - o0_r).abs().max().item() <= fb
    assert ((gd0.double() - gd0_r).abs() - (Td0 + 16) * U * Ad0).max().item() <= 0


# ======================================================================================== unusable regions
def test_unusable_regions_give_zeros_and_touch_nothing():
    g = torch.Generator().manual_seed(300)
    N, C, H, W, D, P = 2, 8, 20, 24, 8, 3
    data = torch.randn(N, C, H, W, generator=g)
    nan, inf = float("nan"), float("inf")
    rois = torch.tensor([[0, 10, 12, 50, 60], [-1, 10, 12, 50, 60], [1, 20, 8, 70, 40], [N, 10, 12, 50, 60], [0.5, 10, 12, 50, 60],
                         [0, nan, 12, 50, 60], [1, 10, 12, inf, 60], [nan, 10, 12, 50, 60], [1, 30, 30, 80, 75], [1e9, 0, 0, 9, 9],
                         [0, 10, -inf, 50, 60]]).float()
    valid = [0, 2, 8]
    bad = [i for i in range(rois.shape[0]) if i not in valid]
    trans = torch.randn(rois.shape[0], 2, P, P, generator=g)
    go = torch.randn(rois.shape[0], D, P, P, generator=g)
    conf = (False, 0.25, D, 1, P, P, 4, 0.1)
    pb = Problem(data, rois, trans, conf)
    out, cnt = pb.forward()
    gd, gt = pb.backward(go)
    assert not out[bad].any() and not cnt[bad].any() and not gt[bad].any()
    assert torch.isfinite(out).all() and torch.isfinite(gd).all() and torch.isfinite(gt).all()
    pv = Problem(data, rois[valid], trans[valid], conf)
    out_v, cnt_v = pv.forward()
    gd_v, gt_v = pv.backward(go[valid])
    assert _bits_equal(out[valid], out_v) and _bits_equal(cnt[valid], cnt_v) and _bits_equal(gt[valid], gt_v)
    assert (cnt_v > 0).any()
    Td, Ad, _, _ = R.grad_terms(data, rois[valid], trans[valid], go[valid], conf)
    assert not gd[Td == 0].any() and (Td == 0).any()                     # nothing outside the valid regions' reach
    _, _, gd_r, gt_r = R.ref_grads(data, rois, trans, go, conf)         # the restatement treats the regions the same way
    assert ((gd.double() - gd_r).abs() - (Td + 16) * U * Ad).max().item() <= 0
    assert not gt_r[bad].any()


# ======================================================================================== argument errors
def test_argument_errors():
    g = torch.Generator().manual_seed(400)
    data = torch.randn(2, 8, 10, 12, generator=g)
    rois = torch.tensor([[0, 4, 4, 30, 30], [1, 8, 2, 40, 36]]).float()
    ne = 2 * 8 * 3 * 3

    def both(pb, code, text, nbytes=None):
        out, gd = Guarded(ne, 7.0), Guarded(data.numel(), 7.0)
        go = torch.zeros(pb.oshape, device=_dev())
        for rc in (pb.forward_rc(out.ptr, None, nbytes), pb.backward_rc(go, gd.ptr, None, nbytes)):
            assert rc == code, (rc, pb.L.m3d_last_error().decode())
            assert text in pb.L.m3d_last_error().decode(), pb.L.m3d_last_error().decode()
        assert (out.get() == 7.0).all() and (gd.get() == 7.0).all()         # a refused call writes nothing

    trans = torch.zeros(2, 2, 3, 3)
    # C < D * G^2
    pb = Problem(data, rois, trans, (False, 0.25, 8, 1, 3, 3, 2, 0.1))
    pb.G = 2
    both(pb, E_ARG, "channels")
    assert pb.L.m3d_dcn_v2_psroi_pooling_workspace_bytes(2, 8, 10, 12, 2, 1, 8, 2, 3, 0) == -1
    # D % K != 0
    pb = Problem(data, rois, torch.zeros(2, 6, 3, 3), (False, 0.25, 6, 1, 3, 3, 2, 0.1))
    pb.D, pb.oshape = 8, (2, 8, 3, 3)
    both(pb, E_ARG, "multiple of the class count")
    assert pb.L.m3d_dcn_v2_psroi_pooling_workspace_bytes(2, 8, 10, 12, 2, 3, 8, 1, 3, 0) == -1
    # trans with fewer rows than regions
    pb = Problem(data, rois, trans[:1], (False, 0.25, 8, 1, 3, 3, 2, 0.1))
    both(pb, E_ARG, "trans has 1 rows for 2 regions")
    # sizes below 1, trans_std outside [0, 1]
    for field, value, text in (("P", 0, "at least 1"), ("S", 0, "at least 1"), ("G", 0, "at least 1"), ("part", 0, "at least 1"),
                               ("std", 1.5, "trans_std"), ("std", -0.1, "trans_std"), ("std", float("nan"), "trans_std"),
                               ("rows", 2 ** 27, "2^31")):
        pb = Problem(data, rois, trans, (False, 0.25, 8, 1, 3, 3, 2, 0.1))
        setattr(pb, field, value)
        both(pb, E_ARG, text)
    # a short workspace: both sizes in the message
    pb = Problem(data, rois, trans, (False, 0.25, 8, 1, 3, 3, 2, 0.1))
    assert pb.fbytes > 256
    out = Guarded(ne, 7.0)
    assert pb.forward_rc(out.ptr, None, pb.fbytes - 1) == E_WORKSPACE
    msg = pb.L.m3d_last_error().decode()
    assert str(pb.fbytes - 1) in msg and str(pb.fbytes) in msg
    gd = Guarded(data.numel(), 7.0)
    assert pb.backward_rc(torch.zeros(pb.oshape, device=_dev()), gd.ptr, None, pb.bbytes - 1) == E_WORKSPACE
    msg = pb.L.m3d_last_error().decode()
    assert str(pb.bbytes - 1) in msg and str(pb.bbytes) in msg
    assert (out.get() == 7.0).all() and (gd.get() == 7.0).all()
    # no region: M3D_OK, nothing launched; the gradients asked for are zero
    pb = Problem(data, rois[:0], trans, (False, 0.25, 8, 1, 3, 3, 2, 0.1))
    assert pb.forward_rc(None, None, 0) == 0
    gd, gt = Guarded(data.numel(), 7.0), Guarded(trans.numel(), 7.0)
    assert pb.backward_rc(None, gd.ptr, gt.ptr, 0) == 0
    assert not gd.get().any() and not gt.get().any()


# ======================================================================================== determinism, NULL, overwrite, workspace
def test_determinism_null_pointers_overwrite_and_workspace_independence():
    (data, rois, trans, conf), go, _, (Td, Ad, _, _) = _case_ref(2)
    pb = Problem(data, rois, trans, conf)
    out, cnt = pb.forward()
    gd, gt = pb.backward(go)
    for _ in range(4):                                                     # 5 launches in all
        gd_i, gt_i = pb.backward(go)
        assert _bits_equal(gt_i, gt)
    # NULL = not wanted; the other gradient does not change (grad_data: float atomics, to roundoff)
    gd_n, none = pb.backward(go, want=(1, 0))
    none2, gt_n = pb.backward(go, want=(0, 1))
    assert none is None and none2 is None and _bits_equal(gt_n, gt)
    assert _within(gd_n, gd, Td, Ad, 2)                                     # two atomic sums of the same terms
    assert pb.backward_rc(go.to(_dev()), None, None) == 0
    out_n, cnt_none = pb.forward(want_count=False)
    assert cnt_none is None and _bits_equal(out_n, out)
    # overwrite: pre-filled buffers are replaced, not added to
    gd_f, gt_f = pb.backward(go, fill=1000.0)
    assert _bits_equal(gt_f, gt) and _within(gd_f, gd, Td, Ad, 2) and (gd_f == 0).any()
    # nothing depends on what the workspace held
    for fill in ("nan", "huge"):
        pp = Problem(data, rois, trans, conf, ws_fill=fill)
        out_p, cnt_p = pp.forward()
        gd_p, gt_p = pp.backward(go)
        assert _bits_equal(out_p, out) and _bits_equal(cnt_p, cnt) and _bits_equal(gt_p, gt)
        assert torch.isfinite(gd_p).all()
        assert _within(gd_p, gd, Td, Ad, 2)


# ======================================================================================== the reference's flows
def _example_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(2, 32, 64, 64, generator=g)
    return data, R.make_rois(20, 2, seed + 1), torch.randn(20, 2, 7, 7, generator=g)


def test_example_dpooling_flow_on_a_side_stream():
    from model.DCNv2.dcn_v2 import DCNv2Pooling
    dev = _dev()
    data, rois, offset = _example_inputs(600)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        inp, rois, offset = data.to(dev).requires_grad_(True), rois.to(dev), offset.to(dev).requires_grad_(True)
        pooling = DCNv2Pooling(spatial_scale=1.0 / 4, pooled_size=7, output_dim=32, no_trans=True, group_size=1, trans_std=0.1).to(dev)
        dpooling = DCNv2Pooling(spatial_scale=1.0 / 4, pooled_size=7, output_dim=32, no_trans=False, group_size=1, trans_std=0.1).to(dev)
        out = pooling(inp, rois, offset)
        dout = dpooling(inp, rois, offset)
        assert tuple(out.shape) == (20, 32, 7, 7) and tuple(dout.shape) == (20, 32, 7, 7)
        g = torch.Generator().manual_seed(601)
        t_out = (torch.rand(out.shape, generator=g) * 0.02 - 0.01).to(dev)
        t_dout = (torch.rand(out.shape, generator=g) * 0.02 - 0.01).to(dev)
        (t_out - out).mean().backward()
        g1 = inp.grad.clone()
        assert offset.grad is None or not offset.grad.any()              # the plain pooling does not use the offsets
        (t_dout - dout).mean().backward()
        g2 = inp.grad.clone()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.isfinite(g2).all() and torch.isfinite(offset.grad).all() and offset.grad.any() and g1.any()
    # input.grad accumulated: the second call added its own gradient onto the first
    go = torch.full(out.shape, -1.0 / out.numel())
    conf = (False, 0.25, 32, 1, 7, 7, 4, 0.1)
    _, _, gd_r, gt_r = R.ref_grads(data, rois, offset, go, conf)
    Td, Ad, Tt, At = R.grad_terms(data, rois, offset, go, conf)
    own = g2.cpu().double() - g1.cpu().double()
    assert ((own - gd_r).abs() - (Td + 16) * U * Ad - U * g2.cpu().double().abs()).max().item() <= 0     # (+ the rounding of the addition)
    assert ((offset.grad.cpu().double() - gt_r).abs() - (Tt + 16) * U * At).max().item() <= 0


def test_example_mdpooling_flow_on_a_side_stream():
    from model.DCNv2.dcn_v2 import DCNPooling
    dev = _dev()
    data, rois, _ = _example_inputs(610)
    torch.manual_seed(611)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        inp = data.to(dev).requires_grad_(True)
        dpooling = DCNPooling(spatial_scale=1.0 / 4, pooled_size=7, output_dim=32, no_trans=False, group_size=1, trans_std=0.1,
                              deform_fc_dim=64).to(dev)
        with torch.no_grad():                                              # leave the zero initialisation: real offsets and masks
            dpooling.offset_fc[4].weight.normal_(0, 0.05)
            dpooling.mask_fc[2].weight.normal_(0, 0.05)
        dout = dpooling(inp, rois.to(dev))
        assert tuple(dout.shape) == (20, 32, 7, 7)
        target = (torch.rand(dout.shape) * 0.2 - 0.1).to(dev)
        (target - dout).mean().backward()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.isfinite(dout).all() and torch.isfinite(inp.grad).all() and inp.grad.any()
    for name, p in dpooling.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert dpooling.offset_fc[0].weight.grad.any() and dpooling.mask_fc[0].weight.grad.any()
