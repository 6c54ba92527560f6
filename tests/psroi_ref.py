"""The yardstick of the deformable PS-ROI pooling tests: a differentiable pure-torch restatement of the operator in the gather
form, written from the definition in include/m3dssd_hip.h and run in float64 under torch.autograd (the reference's CUDA cannot
run here, so there is no golden file; tests/test_psroi_host.py pins this file by closed forms and gradcheck).

Per sample (ih, iw) of every (region, class, bin): the coordinates, the counted predicate (-0.5 <= w <= W - 0.5, the same for h,
region usable), the clamp to the map, floor and ceil, four indexed reads whose bilinear weights are (1 - dx) / dx and (1 - dy) /
dy with dx = w - floor(w); the counted samples are summed and divided by their number.  floor, ceil and the predicate have
derivative zero and the clamp has derivative zero outside the map, so the autograd gradients are the ones the backward has to
produce: the slope between the floor and the ceil column, 0 where they coincide.

A counted / not counted decision and a floor are discontinuous in the coordinate.  With ``coord32`` (the default) the
coordinates are therefore formed in float32, every operation rounded once in the documented order, and only then cast to the
working precision (the cast is differentiable); everything downstream is float64.  ``coord32=False`` keeps them in the working
precision: needed by torch.autograd.gradcheck.  The part and group indices are always the documented float32 expressions.

``conf`` = (no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part, trans_std), the argument
order of ops.psroi_pooling_forward.  spatial_scale and trans_std are used at their float32 values: what the C ABI receives.

``grad_terms`` returns, per gradient element, the number of terms T its sum has and the sum A of their absolute values; the GPU
tests bound the error of an element by (T + 16) * 2^-24 * A:
  grad_data:  one term per (counted sample, corner of non-zero weight) that lands on the element, |grad_out / count| * weight;
  grad_trans: one term per (channel of the class, bin of the part cell, counted sample with distinct floor / ceil),
              |trans_std * roi size * grad_out / count * slope|, the slope being the signed bilinear slope of the sample.
A sum of T terms in any order has at most T - 1 roundings of partial sums bounded by A; a term carries at most 16 further
roundings (the division by the count, three per corner weight or slope, the products with trans_std and the roi size)."""
import torch


def round_half_away(x):
    """roundf: to the nearest integer, halves away from zero (torch.round goes to even).  Exact: x - trunc(x) is exact."""
    r = torch.trunc(x)
    return r + torch.sign(x) * ((x - r).abs() >= 0.5).to(x.dtype)


def part_index(P, part):
    """floorf((float)q / P * part_size) for q = 0 .. P-1, in float32 (clamped into the tensor as the kernel does)."""
    q = torch.arange(P, dtype=torch.float32)
    v = torch.floor(q / torch.tensor(float(P), dtype=torch.float32) * torch.tensor(float(part), dtype=torch.float32))
    return v.long().clamp(0, part - 1)


def group_index(P, G):
    """clamp(floorf((float)q * G / P), 0, G - 1) for q = 0 .. P-1, in float32."""
    q = torch.arange(P, dtype=torch.float32)
    v = torch.floor(q * torch.tensor(float(G), dtype=torch.float32) / torch.tensor(float(P), dtype=torch.float32))
    return v.long().clamp(0, G - 1)


class _Walk:
    """The geometry of one call and an iterator over its S * S samples."""

    def __init__(self, data, rois, trans, conf, coord32):
        no_trans, scale, D, G, P, part, S, trans_std = conf
        self.N, self.C, self.H, self.W = data.shape
        self.n, self.D, self.G, self.P, self.part, self.S = rois.shape[0], D, G, P, part, S
        dev, dt = data.device, data.dtype
        cdt = torch.float32 if coord32 else dt
        n, H, W = self.n, self.H, self.W
        self.K = K = 1 if no_trans else trans.shape[1] // 2
        assert D % K == 0 and self.C >= D * G * G
        self.cec = cec = D // K
        r32 = rois.detach().float()
        bf = r32[:, 0].double()
        self.ok = ok = torch.isfinite(r32).all(1) & (bf >= 0) & (bf < self.N) & (bf == torch.floor(bf))
        # an unusable region takes part as a dummy region whose samples are never counted: no NaN enters the graph
        r = torch.where(ok[:, None], r32, torch.zeros_like(r32)).to(cdt)
        self.b = r[:, 0].long()
        sc = torch.tensor(float(scale), dtype=torch.float32, device=dev).to(cdt)
        self.ts = ts = torch.tensor(float(trans_std), dtype=torch.float32, device=dev).to(cdt)
        Pf, Sf = torch.tensor(float(P), dtype=cdt, device=dev), torch.tensor(float(S), dtype=cdt, device=dev)
        rs_w, rs_h = round_half_away(r[:, 1]) * sc - 0.5, round_half_away(r[:, 2]) * sc - 0.5
        re_w, re_h = (round_half_away(r[:, 3]) + 1.0) * sc - 0.5, (round_half_away(r[:, 4]) + 1.0) * sc - 0.5
        self.roi_w, self.roi_h = roi_w, roi_h = (re_w - rs_w).clamp(min=0.1), (re_h - rs_h).clamp(min=0.1)
        bin_w, bin_h = roi_w / Pf, roi_h / Pf
        sub_w, sub_h = bin_w / Sf, bin_h / Sf
        self.pidx = pidx = part_index(P, part).to(dev)
        gidx = group_index(P, G).to(dev)
        v4 = lambda t: t.view(n, 1, 1, 1)                                      # noqa: E731
        if no_trans:
            tx = ty = torch.zeros(n, 1, P, P, dtype=cdt, device=dev)
        else:
            t = (trans[:n].to(cdt) * ts)[:, :, pidx][:, :, :, pidx]              # [n, 2K, P (ph), P (pw)]
            tx, ty = t[:, 0::2], t[:, 1::2]
        pq = torch.arange(P, device=dev).to(cdt)
        wstart = (pq.view(1, 1, 1, P) * v4(bin_w) + v4(rs_w)) + tx * v4(roi_w)
        hstart = (pq.view(1, 1, P, 1) * v4(bin_h) + v4(rs_h)) + ty * v4(roi_h)
        sq = torch.arange(S, device=dev).to(cdt)
        self.w = (wstart.unsqueeze(-1) + sq * sub_w.view(n, 1, 1, 1, 1)).to(dt)    # [n, K, P, P, S (iw)]
        self.h = (hstart.unsqueeze(-1) + sq * sub_h.view(n, 1, 1, 1, 1)).to(dt)    # [n, K, P, P, S (ih)]
        c = torch.arange(D, device=dev).view(K, cec, 1, 1)
        ch = (c * G + gidx.view(1, 1, P, 1)) * G + gidx.view(1, 1, 1, P)           # input channel [K, cec, P, P]
        self.base = (self.b.view(n, 1, 1, 1, 1) * self.C + ch.unsqueeze(0)) * (H * W)
        okv = ok.view(n, 1, 1, 1, 1)
        self.cw = (self.w >= -0.5) & (self.w <= W - 0.5) & okv
        self.chh = (self.h >= -0.5) & (self.h <= H - 0.5) & okv
        self.count = (self.chh.unsqueeze(-1) & self.cw.unsqueeze(-2)).sum((-1, -2))   # [n, K, P, P]

    def samples(self):
        """Per sample: counted [n, K, 1, P, P], the flat indices of the corners (y1 x1, y2 x1, y1 x2, y2 x2) [n, K, cec, P, P],
        dx, dy [n, K, 1, P, P] and whether floor and ceil differ in x / in y."""
        H, W = self.H, self.W
        for ih in range(self.S):
            for iw in range(self.S):
                m = self.cw[..., iw] & self.chh[..., ih]
                ws, hs = self.w[..., iw], self.h[..., ih]
                zero = torch.zeros_like(ws)
                wc = torch.where(m, ws.clamp(0, W - 1), zero)
                hc = torch.where(m, hs.clamp(0, H - 1), zero)
                x1, x2 = torch.floor(wc).detach(), torch.ceil(wc).detach()
                y1, y2 = torch.floor(hc).detach(), torch.ceil(hc).detach()
                dx, dy = (wc - x1).unsqueeze(2), (hc - y1).unsqueeze(2)
                pix = lambda y, x: self.base + (y * W + x).long().unsqueeze(2)    # noqa: E731
                yield m.unsqueeze(2), (pix(y1, x1), pix(y2, x1), pix(y1, x2), pix(y2, x2)), dx, dy, (x2 != x1).unsqueeze(2), \
                    (y2 != y1).unsqueeze(2)


def psroi_ref(data, rois, trans, conf, coord32=True):
    """(out, count), both [n, D, P, P] in the dtype of ``data``; differentiable in ``data`` and ``trans``."""
    wk = _Walk(data, rois, trans, conf, coord32)
    flat = data.reshape(-1)
    total = 0
    for m, (i11, i12, i21, i22), dx, dy, _, _ in wk.samples():
        ux, uy = 1 - dx, 1 - dy
        val = ux * uy * flat[i11] + ux * dy * flat[i12] + dx * uy * flat[i21] + dx * dy * flat[i22]
        total = total + torch.where(m, val, torch.zeros_like(val))
    cnt = wk.count.unsqueeze(2).to(data.dtype)
    out = torch.where(cnt > 0, total / cnt.clamp(min=1), torch.zeros_like(total))
    shape = (wk.n, wk.D, wk.P, wk.P)
    return out.reshape(shape), cnt.expand(wk.n, wk.K, wk.cec, wk.P, wk.P).reshape(shape)


def sample_coords(data_shape, rois, trans, conf, coord32=True, dt=torch.float64):
    """(w [n, K, P, P, S], h [n, K, P, P, S], count [n, K, P, P]) of a call: what the lattice test inspects."""
    wk = _Walk(torch.zeros(data_shape, dtype=dt), rois, None if trans is None else trans.to(dt), conf, coord32)
    return wk.w, wk.h, wk.count


def ref_grads(data, rois, trans, go, conf, dt=torch.float64, coord32=True):
    """Forward output, count and the gradients (data, trans) of sum(out * go), in ``dt`` on the CPU; trans may be None (no_trans)."""
    d = data.detach().cpu().to(dt).requires_grad_(True)
    t = None if trans is None else trans.detach().cpu().to(dt).requires_grad_(True)
    out, cnt = psroi_ref(d, rois.detach().cpu(), t, conf, coord32=coord32)
    out.backward(go.detach().cpu().to(dt))
    gt = None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t))
    return out.detach(), cnt.detach(), d.grad, gt


def grad_terms(data, rois, trans, go, conf, dt=torch.float64, coord32=True):
    """(T_data, A_data, T_trans, A_trans): per gradient element the number of terms and the sum of their absolute values (module
    docstring); the trans pair is None when no_trans."""
    no_trans = conf[0]
    data = data.detach().cpu().to(dt)
    trans = None if no_trans else trans.detach().cpu().to(dt)
    wk = _Walk(data, rois.detach().cpu(), trans, conf, coord32)
    flat = data.reshape(-1)
    n, K, cec, P, part = wk.n, wk.K, wk.cec, wk.P, wk.part
    cnt = wk.count.unsqueeze(2).to(dt)
    g = go.detach().cpu().to(dt).reshape(n, K, cec, P, P).abs() / cnt.clamp(min=1)
    Td, Ad = torch.zeros_like(flat), torch.zeros_like(flat)
    Tt = At = None
    if not no_trans:
        Tt, At = torch.zeros(trans.numel(), dtype=dt), torch.zeros(trans.numel(), dtype=dt)
        cell = wk.pidx.view(P, 1) * part + wk.pidx.view(1, P)                                  # [P, P]
        tix = ((torch.arange(n).view(n, 1, 1, 1) * 2 * K + 2 * torch.arange(K).view(1, K, 1, 1)) * part * part + cell).unsqueeze(2)
        tix = tix.expand(n, K, cec, P, P)
        fw = (wk.ts.to(dt) * wk.roi_w.to(dt)).view(n, 1, 1, 1, 1)
        fh = (wk.ts.to(dt) * wk.roi_h.to(dt)).view(n, 1, 1, 1, 1)
    for m, idx, dx, dy, xdiff, ydiff in wk.samples():
        ux, uy = 1 - dx, 1 - dy
        me = m.expand(n, K, cec, P, P)
        for ix, wgt in zip(idx, (ux * uy, ux * dy, dx * uy, dx * dy)):
            on = (me & (wgt > 0)).to(dt)
            Td.index_add_(0, ix.reshape(-1), on.reshape(-1))
            Ad.index_add_(0, ix.reshape(-1), (on * g * wgt).reshape(-1))
        if not no_trans:
            v11, v12, v21, v22 = (flat[ix] for ix in idx)
            for xy, f, diff, slope in ((0, fw, xdiff, uy * (v21 - v11) + dy * (v22 - v12)), (1, fh, ydiff, ux * (v12 - v11) + dx * (v22 - v21))):
                on = (me & diff).to(dt)
                ti = (tix + xy * part * part).reshape(-1)
                Tt.index_add_(0, ti, on.reshape(-1))
                At.index_add_(0, ti, (on * f * g * slope.abs()).reshape(-1))
    if no_trans:
        return Td.view_as(data), Ad.view_as(data), None, None
    return Td.view_as(data), Ad.view_as(data), Tt.view_as(trans), At.view_as(trans)


def make_rois(n, N, seed, xy_max=256, wh_max=64, integer=True):
    """Regions drawn as model/DCNv2/test.py's example_dpooling does: corners anywhere in a xy_max square, sizes below wh_max."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(N, (n, 1), generator=g).float()
    if integer:
        x, y = (torch.randint(xy_max, (n, 1), generator=g).float() for _ in range(2))
        w, h = (torch.randint(wh_max, (n, 1), generator=g).float() for _ in range(2))
    else:
        x, y = (torch.rand(n, 1, generator=g) * xy_max for _ in range(2))
        w, h = (torch.rand(n, 1, generator=g) * wh_max for _ in range(2))
    return torch.cat((b, x, y, x + w, y + h), dim=1)


# ---------------------------------------------------------------------------------------------------- the shared cases
def zero_offset_case():
    """model/DCNv2/test.py: check_pooling_zero_offset.  (data, rois, conf for no_trans, conf with trans, trans)."""
    data = torch.zeros(2, 16, 64, 64)
    data[0, :, 16:26, 16:26] = 1.
    data[1, :, 10:20, 20:30] = 2.
    rois = torch.tensor([[0, 65, 65, 103, 103], [1, 81, 41, 119, 79]]).float()
    return data, rois, (True, 0.25, 16, 1, 7, 7, 4, 0.1), (False, 0.25, 16, 1, 7, 7, 4, 0.1), torch.zeros(20, 2, 7, 7)


ZERO_OFFSET_MEANS = (0.9715069, 1.9430137)


def lattice_case(seed=0):
    """The exact-arithmetic case: every count is 16, every sample coordinate is an odd multiple of 1/4 inside the map (never an
    integer, never clamped), data in {+-1, +-2, +-3}, trans multiples of 1/8 in [-1/4, 1/4], grad_out multiples of 1/4 in [-2, 2]:
    no step of a correct kernel rounds.  (data, rois, trans, grad_out, conf)."""
    g = torch.Generator().manual_seed(seed)
    N, H, W, D, G, P, part, S, K = 2, 32, 32, 4, 2, 4, 2, 4, 2
    data = (torch.randint(1, 4, (N, D * G * G, H, W), generator=g) * (torch.randint(0, 2, (N, D * G * G, H, W), generator=g) * 2 - 1)).float()
    rois = torch.tensor([[0, 17, 21, 48, 52], [1, 33, 13, 96, 44], [1, 45, 41, 76, 104], [0, 9, 9, 40, 40]]).float()
    trans = (torch.randint(-2, 3, (rois.shape[0], 2 * K, part, part), generator=g)).float() / 8
    go = (torch.randint(-8, 9, (rois.shape[0], D, P, P), generator=g)).float() / 4
    return data, rois, trans, go, (False, 0.25, D, G, P, part, S, 0.5)
