"""The differentiable forwards: what the modules run in training mode with grad enabled on a device tensor (the rule DCNv2 /
DeformConv follow).  Custom blocks go through the HIP operators with a backward (``ops.dcn_v2``, ``ops.anab_attention``); everything
else is the layers PyTorch-ROCm has, so their gradients are autograd's -- except that ``set_fused_batchnorm`` (opt-in) sends every
BatchNorm2d + residual add + LeakyReLU site through one HIP operator too (``ops.bn_act_train``).  Eval mode and no-grad calls
never come here: they keep the fused inference launches (host/standalone.py, engine.py)."""
import torch
from torch import nn

from .. import _hip, rpn_util
from . import ops


def wants_grad(mod, *ts):
    """Training mode, grad enabled, device tensors."""
    return mod.training and torch.is_grad_enabled() and all(t.is_cuda for t in ts)


# ---- ANAB (model/module/attention.py:183-216) --------------------------------------------------------------------------------------
def anab_forward(mod, x):
    B, C, H, W = x.shape
    ck = mod.key_ch
    rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
    # one matmul with the stacked query | key | value | spatial weights: the projection gradients are autograd's
    ws = [mod.query_conv.weight, mod.key_conv.weight, mod.value_conv.weight, mod.spatial_conv.weight]
    # opt-in (set_bf16_attention) and only under bfloat16 autocast on the device: the bf16 operator on the bf16 rows of the matmul
    bf16 = mod.bf16_attention and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16
    if bf16:
        # zero rows behind the stacked weights: the row stride of qkvs becomes a multiple of 8 elements, so q is taken as it is
        ws.append(ws[0].new_zeros((-(2 * ck + C + 4)) % 8, C, 1, 1))
    wall = torch.cat(ws, 0)
    qkvs = rows @ wall.reshape(wall.shape[0], C).t()
    q, k, v = qkvs[:, :ck], qkvs[:, ck:2 * ck], qkvs[:, 2 * ck:2 * ck + C]
    gates = torch.sigmoid(qkvs[:, 2 * ck + C:2 * ck + C + 4])
    if bf16 and qkvs.dtype == torch.bfloat16:
        out = (ops.anab_attention_bf16(q, k, v, gates, B, H, W) + rows).to(torch.bfloat16)
    else:
        out = ops.anab_attention(q, k, v, gates, B, H, W) + rows
    return out.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def set_bf16_attention(net, flag=True):
    """Turns the bf16 attention operator (``ops.anab_attention_bf16``) on or off for every ANAB below ``net``; it is taken only under
    ``torch.autocast("cuda", dtype=torch.bfloat16)``.  Returns the number of blocks set."""
    from .attention import ANAB
    n = 0
    for m in net.modules():
        if isinstance(m, ANAB):
            m.bf16_attention = bool(flag)
            n += 1
    return n


# ---- shape_align / center_align (model/module/feturealign_mgpu.py:48-99, 153-208 with k = 1) ------------------------------------------
def _top1(prob):
    """Top-1 anchor per pixel by m3d_fg_top1 (lowest index among equal maxima: the engine's rule) -> ind [B, 1, H, W] int64, and
    the mask = the probability there, gathered with torch so that a gradient reaches a ``prob`` that is not detached (softmax over
    the single top value is 1: no term)."""
    B, A, H, W = prob.shape
    p = prob.detach().contiguous().float()
    idx = torch.empty(B * H * W, device=prob.device, dtype=torch.int32)
    val = torch.empty(B * H * W, device=prob.device, dtype=torch.float32)
    with torch.cuda.device(prob.device):
        _hip.check(_hip.lib().m3d_fg_top1(p.data_ptr(), B, A, H * W, idx.data_ptr(), val.data_ptr(), ops._stream()))
    ind = idx.view(B, 1, H, W).long()
    return ind, torch.gather(prob, 1, ind)


def shape_align_forward(mod, x, prob):
    kk = mod.kernel_size[0] * mod.kernel_size[1]
    ind, mask = _top1(prob)
    hard = (mask > mod.thresh).to(x.dtype)
    tab = mod.offset_table.to(x.device)
    offset = tab[ind[:, 0]].permute(0, 3, 1, 2) * hard            # [B, 2 kk, H, W]
    return mod.align(x.contiguous(), offset.contiguous(), mask.repeat(1, kk, 1, 1)) + x


def center_align_forward(mod, x, bbox_x, bbox_y, prob):
    kk = mod.kernel_size[0] * mod.kernel_size[1]
    ind, mask = _top1(prob)
    hard = (mask > mod.thresh).to(x.dtype)
    dev = x.device
    offset_x = (bbox_x * mod.xy_std[0].to(dev) + mod.xy_mean[0].to(dev)) * mod.anchors_w.to(dev)
    offset_y = (bbox_y * mod.xy_std[1].to(dev) + mod.xy_mean[1].to(dev)) * mod.anchors_h.to(dev)
    offset_x = torch.gather(offset_x, 1, ind) * hard
    offset_y = torch.gather(offset_y, 1, ind) * hard
    offset = torch.cat([offset_y, offset_x], 1).repeat(1, kk, 1, 1)
    return mod.align(x.contiguous(), offset.contiguous(), mask.repeat(1, kk, 1, 1)) + x


# ---- BatchNorm (batch statistics) + residual + activation as one operator (opt-in) ------------------------------------------------
def set_fused_batchnorm(net, flag=True):
    """Turns the fused training operator (``ops.bn_act_train``: BatchNorm2d with batch statistics + residual add + LeakyReLU in two
    launches forward, two backward) on or off for every BatchNorm2d below ``net``; the default is off.  Returns the number of
    BatchNorm sites set -- in an RPN every one of them is reached by the training forward.  A site keeps its torch layers while its
    BatchNorm is in eval mode (a frozen layer), has ``momentum=None``, no affine parameters or no running statistics, while its
    input is not float32, and inside a ``torch.autocast`` region (where a float32 input is the exception)."""
    n = 0
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.fused_train = bool(flag)
            n += 1
    return n


def _act_slope(act):
    """The slope of ``ops.bn_act_train`` that stands for the activation module (None: no activation), or None when it has none."""
    if act is None:
        return 1.0
    if type(act) is nn.LeakyReLU:
        return float(act.negative_slope) if 0.0 <= act.negative_slope <= 1.0 else None
    if type(act) is nn.ReLU:
        return 0.0
    return None


def _fused(bn, x):
    return (getattr(bn, "fused_train", False) and bn.training and bn.momentum is not None and bn.affine and bn.track_running_stats
            and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled("cuda"))


def bn_act(bn, x, act=None, residual=None):
    """``act(bn(x) + residual)`` (``act`` / ``residual`` may be None): the torch layers, or ``ops.bn_act_train`` where
    ``set_fused_batchnorm`` asked for it and the site qualifies."""
    if _fused(bn, x) and (residual is None or residual.dtype == torch.float32):
        slope = _act_slope(act)
        if slope is not None:
            bn.num_batches_tracked.add_(1)                        # as nn.BatchNorm2d.forward in training mode
            return ops.bn_act_train(x, residual, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, slope)
    out = bn(x)
    if residual is not None:
        out = out + residual
    return out if act is None else act(out)


def seq_forward(seq, x):
    """``seq(x)`` for an nn.Sequential; with the fused operator on, each BatchNorm2d is taken together with the activation module
    that follows it (base_layer, level0 / level1, Tree.project, DeformConv.actf, the RPN heads, bbox_z3d_gl).  The walk then calls
    the members itself: forward hooks of the Sequential and of a fused BatchNorm2d / activation do not run; the other members' do."""
    mods = list(seq)
    if not any(isinstance(m, nn.BatchNorm2d) and getattr(m, "fused_train", False) for m in mods):
        return seq(x)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.BatchNorm2d):
            act = mods[i + 1] if i + 1 < len(mods) and _act_slope(mods[i + 1]) is not None else None
            x = bn_act(m, x, act)
            i += 1 if act is None else 2
        else:
            x = m(x)
            i += 1
    return x


# ---- DLA (model/pose_dla_dcn.py; the line ranges are in host/dla.py) ---------------------------------------------------------------
def basic_block_forward(mod, x, residual=None):
    if residual is None:
        residual = x
    out = bn_act(mod.bn1, mod.conv1(x), mod.relu)
    return bn_act(mod.bn2, mod.conv2(out), mod.relu, residual)


def bottleneck_forward(mod, x, residual=None):
    if residual is None:
        residual = x
    out = bn_act(mod.bn1, mod.conv1(x), mod.relu)
    out = bn_act(mod.bn2, mod.conv2(out), mod.relu)
    return bn_act(mod.bn3, mod.conv3(out), mod.relu, residual)


def root_forward(mod, *xs):
    return bn_act(mod.bn, mod.conv(torch.cat(xs, 1)), mod.relu, xs[0] if mod.residual else None)


def tree_forward(mod, x, residual=None, children=None):
    children = [] if children is None else children
    bottom = mod.downsample(x) if mod.downsample is not None else x
    # (a Tree of more than one level hands this to tree1, itself a Tree, which computes its own: the value is dropped, as in the
    # reference -- the BatchNorm of the projection still sees the batch)
    residual = seq_forward(mod.project, bottom) if mod.project is not None else bottom
    if mod.level_root:
        children.append(bottom)
    x1 = mod.tree1(x, residual)
    if mod.levels == 1:
        return mod.root(mod.tree2(x1), x1, *children)
    children.append(x1)
    return mod.tree2(x1, children=children)


def dla_forward(mod, x):
    y = []
    x = seq_forward(mod.base_layer, x)
    for i in range(6):
        level = getattr(mod, "level%d" % i)
        x = seq_forward(level, x) if i < 2 else level(x)
        y.append(x)
    return y


def ida_up_forward(mod, layers, startp, endp):
    for i in range(startp + 1, endp):
        j = i - startp
        layers[i] = getattr(mod, "up_%d" % j)(getattr(mod, "proj_%d" % j)(layers[i]))
        layers[i] = getattr(mod, "node_%d" % j)(layers[i] + layers[i - 1])


def dla_up_forward(mod, layers):
    out = [layers[-1]]
    for i in range(len(layers) - mod.startp - 1):
        getattr(mod, "ida_%d" % i)(layers, len(layers) - i - 2, len(layers))
        out.insert(0, layers[-1])
    return out


def dlaseg_forward(mod, x):
    layers = mod.dla_up(mod.base(x))
    y = [layers[i].clone() for i in range(mod.last_level - mod.first_level)]
    mod.ida_up(y, 0, len(y))
    return y[-1]


# ---- RPN (model/M3d_inference_align.py:215-304) ---------------------------------------------------------------------------------------
def rpn_forward(mod, x):
    if x.dim() != 4 or not x.dtype.is_floating_point:
        raise RuntimeError("RPN (training mode): the input is a normalised float image batch [B, 3, H, W]")
    B = x.shape[0]
    x = mod.base(x.float())
    assert x.shape[2] == mod.feat_size[0], "x.shape is {}".format(x.shape)
    cls = seq_forward(mod.cls, x)
    fh, fw, A = cls.shape[2], cls.shape[3], mod.num_anchors
    cls = cls.view(B, mod.num_classes, fh * A, fw)
    prob = mod.softmax(cls)
    fg_prob = (1 - prob.detach()[:, 0, :, :]).view(B, A, fh, fw)
    feats = mod.shape_align(x, fg_prob) if mod.shape_align is not None else x
    bbox_x, bbox_y = seq_forward(mod.bbox_x, feats), seq_forward(mod.bbox_y, feats)
    if mod.center_align2d is not None:
        feats_align2d = mod.center_align2d(feats, bbox_x.detach(), bbox_y.detach(), fg_prob)
    else:
        feats_align2d = feats
    bbox_w, bbox_h = seq_forward(mod.bbox_w, feats_align2d), seq_forward(mod.bbox_h, feats_align2d)
    bbox_x3d, bbox_y3d = seq_forward(mod.bbox_x3d, feats), seq_forward(mod.bbox_y3d, feats)
    if mod.center_align3d is not None:
        feats_align3d = mod.center_align3d(feats, bbox_x3d.detach(), bbox_y3d.detach(), fg_prob)
    else:
        feats_align3d = feats
    bbox_w3d, bbox_h3d = seq_forward(mod.bbox_w3d, feats_align3d), seq_forward(mod.bbox_h3d, feats_align3d)
    bbox_l3d, bbox_rY3d = seq_forward(mod.bbox_l3d, feats_align3d), seq_forward(mod.bbox_rY3d, feats_align3d)
    feats_gl = seq_forward(mod.bbox_z3d_gl, feats_align3d) if getattr(mod, "bbox_z3d_gl", None) is not None else feats_align3d
    bbox_z3d = seq_forward(mod.bbox_z3d, feats_gl)

    def flat(t):
        return rpn_util.flatten_tensor(t.view(B, 1, fh * A, fw))

    bbox_2d = torch.cat([flat(t) for t in (bbox_x, bbox_y, bbox_w, bbox_h)], dim=2)
    bbox_3d = torch.cat([flat(t) for t in (bbox_x3d, bbox_y3d, bbox_z3d, bbox_w3d, bbox_h3d, bbox_l3d, bbox_rY3d)], dim=2)
    feat_size = torch.tensor([fh, fw], dtype=torch.float, device=x.device)
    return rpn_util.flatten_tensor(cls), rpn_util.flatten_tensor(prob), bbox_2d, bbox_3d, feat_size
