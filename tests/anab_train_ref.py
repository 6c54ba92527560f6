"""Yardsticks of the train-mode tests.

``anab_core``: the ANAB attention core as a differentiable torch composition -- the reference's PAPAModule (gated
AdaptiveAvgPool2d pyramids of the keys and the values, model/module/attention.py:136-147) + bmm + softmax + bmm (:207-211) -- on
row matrices [B*H*W, C] in whatever dtype and on whatever device they come (float64 on the CPU: the yardstick; float32 on the
device: the error a float32 evaluation in another summation order makes).  ``anab_module`` wraps it with the projections and the
residual of ANAB.forward; ``anab_logits`` gives the logits in front of its softmax and ``peak_rows_`` scales rows of q so that they
pass ln(FLT_MAX).  tests/test_anab_train_host.py pins both against oracle.model_cpu.anab and with gradcheck.

``dcn_ref``: the gather-form DCNv2 of tests/dcn_grad_ref.py, device-aware (the index vectors are made on the input's device), so
that a whole network can run with it in place of the HIP operator."""
import torch
import torch.nn.functional as F

PSP = (1, 4, 8, 16)


def _planes(t, B, H, W):
    return t.reshape(B, H, W, t.shape[-1]).permute(0, 3, 1, 2)


def _pooled(t, g, B, H, W):
    """The gated pyramid of a row matrix: [B, C, 337], bins scale-major (1 + 16 + 64 + 256)."""
    tt, gg = _planes(t, B, H, W), _planes(g, B, H, W)
    return torch.cat([F.adaptive_avg_pool2d(tt * gg[:, i:i + 1], (z, z)).flatten(2) for i, z in enumerate(PSP)], -1)


def anab_logits(q, k, g, B, H, W):
    """The logits [B, H*W, 337] that ``anab_core`` hands to its softmax."""
    return torch.bmm(q.reshape(B, H * W, -1), _pooled(k, g, B, H, W))


def anab_core(q, k, v, g, B, H, W):
    hw = H * W
    vp = _pooled(v, g, B, H, W)                                                                                       # [B, Cv, 337]
    att = torch.softmax(anab_logits(q, k, g, B, H, W), dim=-1)
    return torch.bmm(att, vp.transpose(1, 2)).reshape(B * hw, -1)


def anab_module(x, wq, wk, wv, ws):
    """ANAB.forward on NCHW ``x`` with the four 1x1 weights [Cout, C, 1, 1]: x + attention."""
    B, C, H, W = x.shape
    rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
    q, k, v = rows @ wq.reshape(wq.shape[0], C).t(), rows @ wk.reshape(wk.shape[0], C).t(), rows @ wv.reshape(wv.shape[0], C).t()
    g = torch.sigmoid(rows @ ws.reshape(ws.shape[0], C).t())
    out = anab_core(q, k, v, g, B, H, W) + rows
    return out.reshape(B, H, W, C).permute(0, 3, 1, 2)


def core_grads(ts, go, B, H, W, dtype, device):
    """Output and the four gradients of sum(out * go) of ``anab_core`` in ``dtype`` on ``device``."""
    ts = [t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in ts]
    out = anab_core(*ts, B, H, W)
    out.backward(go.detach().to(device=device, dtype=dtype))
    return [out.detach()] + [t.grad for t in ts]


def dcn_ref(inp, offset, mask, weight, bias, stride, pad, dil=1, G=1):
    """tests/dcn_grad_ref.py::dcn_ref with float32 coordinates in the kernel's order, on the device of ``inp``."""
    n, c, h, w = inp.shape
    co, _, kh, kw = weight.shape
    kk = kh * kw
    ho = (h + 2 * pad - (dil * (kh - 1) + 1)) // stride + 1
    wo = (w + 2 * pad - (dil * (kw - 1) + 1)) // stride + 1
    dt, dev = inp.dtype, inp.device
    ys = (torch.arange(ho, device=dev) * stride - pad).view(1, ho, 1)
    xs = (torch.arange(wo, device=dev) * stride - pad).view(1, 1, wo)
    cg = c // G
    flat = inp.reshape(n, c, h * w)
    out = bias.view(1, co, 1, 1).expand(n, co, ho, wo).clone()
    for g in range(G):
        xg = flat[:, g * cg:(g + 1) * cg]
        for i in range(kh):
            for j in range(kw):
                k = i * kw + j
                hy = ((ys + i * dil).float() + offset[:, g * 2 * kk + 2 * k].float()).to(dt)
                wx = ((xs + j * dil).float() + offset[:, g * 2 * kk + 2 * k + 1].float()).to(dt)
                m = mask[:, g * kk + k]
                inside = (hy > -1) & (wx > -1) & (hy < h) & (wx < w)
                hl, wl = torch.floor(hy), torch.floor(wx)
                lh, lw = hy - hl, wx - wl
                val = 0
                for (dy, dx, wt) in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
                    yy, xx = (hl.detach() + dy), (wl.detach() + dx)
                    ok = inside & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)
                    idx = (yy.clamp(0, h - 1).long() * w + xx.clamp(0, w - 1).long()).view(n, 1, ho * wo).expand(n, cg, ho * wo)
                    v = torch.gather(xg, 2, idx).view(n, cg, ho, wo)
                    val = val + v * torch.where(ok, wt, torch.zeros_like(wt)).unsqueeze(1)
                col = val * m.unsqueeze(1)
                out = out + torch.einsum("oc,nchw->nohw", weight[:, g * cg:(g + 1) * cg, i, j], col)
    return out


def make_core_case(B, H, W, Ck, Cv, seed):
    """float32 CPU inputs (q, k, v, gates) as column slices of ONE wider row matrix (so every row stride differs from its channel
    count and the neighbour columns are guard values: 4 columns of 1e30 between and around the slices), and grad_out likewise."""
    g = torch.Generator().manual_seed(seed)
    n = B * H * W
    wide = torch.full((n, 4 + Ck + 4 + Ck + 4 + Cv + 4 + 4 + 4), 1e30)
    o = 4
    views = []
    for c, scale in ((Ck, 0.3), (Ck, 1.0), (Cv, 1.0), (4, 1.0)):
        wide[:, o:o + c] = torch.randn(n, c, generator=g) * scale
        views.append((o, c))
        o += c + 4
    go, gc = views[3]
    wide[:, go:go + gc] = torch.sigmoid(wide[:, go:go + gc])
    gwide = torch.full((n, Cv + 8), 1e30)
    gwide[:, 4:4 + Cv] = torch.randn(n, Cv, generator=g)
    return wide, views, gwide


def peak_rows_(wide, views, every=37, factor=40.0):
    """Every ``every``-th row of q (rows 0, every, 2 every, ...) times ``factor``, in place: with q ~ 0.3 N(0, 1) and factor 40 the
    largest logit of such a row passes ln(FLT_MAX) = 88.72, so exp(s) overflows float32 where exp(s - max) does not."""
    o, c = views[0]
    wide[::every, o:o + c] *= factor
    return wide
