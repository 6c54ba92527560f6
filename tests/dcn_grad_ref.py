"""The yardstick of the DCNv2 gradient tests: a differentiable pure-torch restatement of the forward in the gather form, run in
float64 under torch.autograd (oracle/ has a forward only).

Per deformable group and tap: sampling coordinates, the inside predicate (h > -1, w > -1, h < H, w < W), floor, four clamped
torch.gather's whose bilinear weights are multiplied by the validity of their corner, times the mask; then the contraction with
the weights.  This is m3d_dcn_v2_forward as include/m3dssd_hip.h defines it, piecewise rule included, so its autograd gradients
are the analytic derivatives the backward has to produce (floor has derivative zero: at an integer coordinate the result is
the one-sided derivative towards +).

d val / d offset is discontinuous where a sampling coordinate crosses an integer, and a coordinate summed in float64 can fall on
the other side of an integer than the kernel's float32 sum.  With ``coord32`` (the default) the coordinates are therefore
formed in float32 in the kernel's order, (float)(y * stride - pad + i * dil) + offset, and only then cast to the working
precision (the cast is differentiable: grad_offset still flows); everything downstream is float64.  ``coord32=False`` keeps
them in the working precision: needed by torch.autograd.gradcheck, whose 1e-6 perturbations a float32 rounding would swallow.

tests/test_dcn_backward_host.py pins this file: its float32 forward against oracle.dcn.dcn_v2_forward, and gradcheck."""
import torch


def out_size(h, w, kh, kw, stride, pad, dil):
    return (h + 2 * pad - (dil * (kh - 1) + 1)) // stride + 1, (w + 2 * pad - (dil * (kw - 1) + 1)) // stride + 1


def dcn_ref(inp, offset, mask, weight, bias, stride, pad, dil, G, coord32=True):
    n, c, h, w = inp.shape
    co, _, kh, kw = weight.shape
    kk = kh * kw
    ho, wo = out_size(h, w, kh, kw, stride, pad, dil)
    dt = inp.dtype
    cdt = torch.float32 if coord32 else dt
    ys = (torch.arange(ho) * stride - pad).view(1, ho, 1)
    xs = (torch.arange(wo) * stride - pad).view(1, 1, wo)
    cg = c // G
    flat = inp.reshape(n, c, h * w)
    out = bias.view(1, co, 1, 1).expand(n, co, ho, wo).clone()
    for g in range(G):
        xg = flat[:, g * cg:(g + 1) * cg]
        for i in range(kh):
            for j in range(kw):
                k = i * kw + j
                hy = ((ys + i * dil).to(cdt) + offset[:, g * 2 * kk + 2 * k].to(cdt)).to(dt)
                wx = ((xs + j * dil).to(cdt) + offset[:, g * 2 * kk + 2 * k + 1].to(cdt)).to(dt)
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
                    # where(), not a product: a dropped corner contributes nothing even when its weight is not finite
                    val = val + v * torch.where(ok, wt, torch.zeros_like(wt)).unsqueeze(1)
                col = val * m.unsqueeze(1)
                out = out + torch.einsum("oc,nchw->nohw", weight[:, g * cg:(g + 1) * cg, i, j], col)
    return out


def make_case(n, c, co, h, w, k, stride, pad, dil, G, sigma, seed):
    """(input, offset, mask, weight, bias) float32 on the CPU, grad_output, (stride, pad, dil, G): offsets N(0, sigma), masks from a
    sigmoid, grad_output N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    ho, wo = out_size(h, w, k, k, stride, pad, dil)
    x = torch.randn(n, c, h, w, generator=g)
    off = torch.randn(n, G * 2 * k * k, ho, wo, generator=g) * sigma
    m = torch.sigmoid(torch.randn(n, G * k * k, ho, wo, generator=g))
    wt = torch.randn(co, c, k, k, generator=g) / (c * k * k) ** 0.5
    b = torch.randn(co, generator=g)
    go = torch.randn(n, co, ho, wo, generator=g)
    return (x, off, m, wt, b), go, (stride, pad, dil, G)


def ref_grads(ts, go, args, dt=torch.float64, coord32=True):
    """Forward output and the five gradients (input, offset, mask, weight, bias) of sum(out * go), in ``dt`` on the CPU."""
    ts = [t.detach().cpu().to(dt).requires_grad_(True) for t in ts]
    out = dcn_ref(*ts, *args, coord32=coord32)
    out.backward(go.detach().cpu().to(dt))
    return out.detach(), [t.grad for t in ts]


# the five shapes the yardstick is pinned on (tests/test_dcn_backward_host.py): k = 1 / 3, stride 2, dilation 2 with pad 2, G = 1 / 2 / 3
PIN_CASES = [(2, 8, 6, 9, 11, 3, 1, 1, 1, 1, 2.0, 0), (1, 8, 4, 10, 12, 3, 2, 1, 1, 2, 3.0, 1), (2, 4, 4, 7, 9, 1, 1, 0, 1, 1, 2.0, 2),
             (1, 6, 5, 12, 10, 3, 1, 2, 2, 3, 4.0, 3), (2, 32, 32, 24, 40, 3, 1, 1, 1, 1, 3.0, 4)]
