"""Synthetic weights, configuration and frames.

The reference ships no trained weights, no KITTI data and no pickled ``conf``
(its .gitignore:6 drops data/), so benchmarks, smoke runs, golden fixtures and
parity tests all use a deterministic synthetic recipe (numpy PCG64, one stream per
tensor keyed by crc32 of its state_dict name, so values do not depend on order):

* ``param_spec`` lists every state_dict entry of ``RPN(dla34)`` -- 542 tensors (fullalign;
  526 for base, 535 for anab; ``back_bone="dla102"``: 944 / 928 / 937), the
  contract in SURVEY.md 8b; tools/gen_golden.py asserts it equals the reference
  model's own ``state_dict()`` keys and shapes.
* conv_offset_mask is re-randomised (the reference zero-inits it,
  model/DCNv2/dcn_v2.py:60-62, which would make every DCN degenerate), BN running
  stats are randomised, and the background logit bias is raised so that both
  branches of the ``fg > 0.5`` hard mask (feturealign_mgpu.py:62,164) occur; the ANAB query / key projections are scaled
  so that the 337-key softmax is not saturated (see ANAB_QK_GAIN below).
"""
import math
import zlib
from collections import OrderedDict

import numpy as np
import torch

from .config import CONFIG_FLAGS, Config
from . import rpn_util

HEADS = ["cls", "bbox_x", "bbox_y", "bbox_w", "bbox_h", "bbox_x3d", "bbox_y3d"]
HEADS_TAIL = ["bbox_z3d"]
HEADS_TAIL2 = ["bbox_w3d", "bbox_h3d", "bbox_l3d", "bbox_rY3d"]
BG_BIAS = 4.2
BOX_OUT_GAIN = 0.15
ANAB_QK_GAIN = 0.1


def _bn(spec, p, c):
    spec[p + ".weight"] = (c,)
    spec[p + ".bias"] = (c,)
    spec[p + ".running_mean"] = (c,)
    spec[p + ".running_var"] = (c,)
    spec[p + ".num_batches_tracked"] = ()


def _conv(spec, p, co, ci, k, bias):
    spec[p + ".weight"] = (co, ci, k, k)
    if bias:
        spec[p + ".bias"] = (co,)


def _block(spec, p, ci, co):
    _conv(spec, p + ".conv1", co, ci, 3, True)
    _bn(spec, p + ".bn1", co)
    _conv(spec, p + ".conv2", co, co, 3, True)
    _bn(spec, p + ".bn2", co)


def _bottleneck(spec, p, ci, co):
    """Bottleneck (pose_dla_dcn.py:162-200, expansion 2): 1x1 ci -> co/2, 3x3, 1x1 co/2 -> co, no biases."""
    cb = co // 2
    _conv(spec, p + ".conv1", cb, ci, 1, False)
    _bn(spec, p + ".bn1", cb)
    _conv(spec, p + ".conv2", cb, cb, 3, False)
    _bn(spec, p + ".bn2", cb)
    _conv(spec, p + ".conv3", co, cb, 1, False)
    _bn(spec, p + ".bn3", co)


def _tree(spec, p, levels, ci, co, level_root, root_dim=0, block=_block):
    if root_dim == 0:
        root_dim = 2 * co
    if level_root:
        root_dim += ci
    if levels == 1:
        block(spec, p + ".tree1", ci, co)
        block(spec, p + ".tree2", co, co)
        _conv(spec, p + ".root.conv", co, root_dim, 1, False)
        _bn(spec, p + ".root.bn", co)
    else:
        _tree(spec, p + ".tree1", levels - 1, ci, co, False, 0, block)
        _tree(spec, p + ".tree2", levels - 1, co, co, False, root_dim + co, block)
    if ci != co:
        _conv(spec, p + ".project.0", co, ci, 1, False)
        _bn(spec, p + ".project.1", co)


def _deform(spec, p, ci, co):
    _bn(spec, p + ".actf.0", co)
    spec[p + ".conv.weight"] = (co, ci, 3, 3)
    spec[p + ".conv.bias"] = (co,)
    spec[p + ".conv.conv_offset_mask.weight"] = (27, ci, 3, 3)
    spec[p + ".conv.conv_offset_mask.bias"] = (27,)


def _ida(spec, p, o, chans):
    for i in range(1, len(chans)):
        _deform(spec, "%s.proj_%d" % (p, i), chans[i], o)
        spec["%s.up_%d.weight" % (p, i)] = (o, 1, 4, 4)
        _deform(spec, "%s.node_%d" % (p, i), o, o)


def _head(spec, p, ci, co, k0):
    _conv(spec, p + ".0", 256, ci, k0, True)
    _bn(spec, p + ".1", 256)
    _conv(spec, p + ".3", 256, 256, 1, True)
    _bn(spec, p + ".4", 256)
    _conv(spec, p + ".6", co, 256, 1, True)


# per backbone (pose_dla_dcn.py:419-440): level depths, channels, block, residual root
BACKBONES = {
    "dla34": dict(levels=(1, 1, 1, 2, 2, 1), channels=(16, 32, 64, 128, 256, 512), block="basic", residual_root=False),
    "dla102": dict(levels=(1, 1, 1, 3, 4, 1), channels=(16, 32, 128, 256, 512, 1024), block="bottleneck", residual_root=True),
}


def backbone(name):
    if name not in BACKBONES:
        raise NotImplementedError("back_bone %r: this build runs %s" % (name, " / ".join(BACKBONES)))
    return BACKBONES[name]


def param_spec(num_anchors=36, num_classes=4, shape_align=True, center_align=True, attention="ANAB", back_bone="dla34"):
    """OrderedDict name -> shape, in the reference's registration order.  The flags drop the sub-modules the reference does not
    create (M3d_inference_align.py:138-168): the align modules when their flag is off, bbox_z3d_gl unless attention == "ANAB";
    the defaults give the fullalign model.  ``back_bone="dla102"``: Bottleneck trees of depth [1, 1, 1, 3, 4, 1] and channels
    [16, 32, 128, 256, 512, 1024], so every map from DLAUp on (heads, alignment, ANAB) is 256 channels wide instead of 128."""
    s = OrderedDict()
    bb = backbone(back_bone)
    ch, lv = list(bb["channels"]), bb["levels"]
    blk = _bottleneck if bb["block"] == "bottleneck" else _block
    b = "base.base"
    _conv(s, b + ".base_layer.0", ch[0], 3, 7, False)
    _bn(s, b + ".base_layer.1", ch[0])
    _conv(s, b + ".level0.0", ch[0], ch[0], 3, False)
    _bn(s, b + ".level0.1", ch[0])
    _conv(s, b + ".level1.0", ch[1], ch[0], 3, False)
    _bn(s, b + ".level1.1", ch[1])
    for i in range(2, 6):
        _tree(s, "%s.level%d" % (b, i), lv[i], ch[i - 1], ch[i], i > 2, block=blk)
    c3, c4, c5 = ch[3], ch[4], ch[5]
    _ida(s, "base.dla_up.ida_0", c4, [c4, c5])
    _ida(s, "base.dla_up.ida_1", c3, [c3, c4, c4])
    _ida(s, "base.ida_up", c3, [c3, c4])
    c = c3                                                     # base_channels: the width of feats0 and every map after it
    _head(s, "cls", c, num_anchors * num_classes, 3)
    for h in HEADS[1:]:
        _head(s, h, c, num_anchors, 1)
    if center_align:
        for p in ("center_align2d", "center_align3d"):
            s[p + ".align.weight"] = (c, c, 1, 1)
            s[p + ".align.bias"] = (c,)
    if shape_align:
        s["shape_align.align.weight"] = (c, c, 3, 3)
        s["shape_align.align.bias"] = (c,)
        s["shape_align.proj.weight"] = (c, 2 * c, 1, 1)
    _head(s, "bbox_z3d", c, num_anchors, 1)
    if attention == "ANAB":
        s["bbox_z3d_gl.0.value_conv.weight"] = (c, c, 1, 1)
        s["bbox_z3d_gl.0.spatial_conv.weight"] = (4, c, 1, 1)
        s["bbox_z3d_gl.0.key_conv.weight"] = (168, c, 1, 1)
        s["bbox_z3d_gl.0.query_conv.weight"] = (168, c, 1, 1)
        _bn(s, "bbox_z3d_gl.1", c)
    for h in HEADS_TAIL2:
        _head(s, h, c, num_anchors, 1)
    return s


def _rng(seed, name):
    return np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))


def _bilinear_up(shape):
    c, _, k, _ = shape
    f = math.ceil(k / 2)
    cc = (2 * f - 1 - f % 2) / (2.0 * f)
    w = np.zeros(shape, dtype=np.float32)
    for i in range(k):
        for j in range(k):
            w[:, 0, i, j] = (1 - math.fabs(i / f - cc)) * (1 - math.fabs(j / f - cc))
    return w


# DLA-102 only: the residual roots add every tree's x2 once more and the Bottleneck's last 1x1 sums over half the channels, so
# with the DLA-34 recipe the backbone maps grow level by level.  These gains on the backbone's root convs and the Bottleneck
# output convs keep max |level5| and max |feats0| at the DLA-34 network's magnitude (tests/test_dla102_host.py checks it).
DLA102_ROOT_GAIN = 0.2
DLA102_CONV3_GAIN = 0.2


def _dla102_gain(name):
    if ".root.conv." in name:
        return DLA102_ROOT_GAIN
    if name.endswith(".conv3.weight"):
        return DLA102_CONV3_GAIN
    return 1.0


def config_flags(name):
    """The flag keywords of param_spec / synth_state_dict / synth_conf for a shipped configuration
    ("base", "anab", "anab_fullalign")."""
    return dict(CONFIG_FLAGS[name])


def synth_state_dict(seed=0, num_anchors=36, num_classes=4, shape_align=True, center_align=True, attention="ANAB",
                     back_bone="dla34"):
    """Every tensor is drawn from its own stream keyed by its name: a configuration without some sub-modules gets the same
    values for the keys it shares with the fullalign dict."""
    spec = param_spec(num_anchors, num_classes, shape_align, center_align, attention, back_bone)
    deep = back_bone == "dla102"
    sd = OrderedDict()
    for name, shape in spec.items():
        g = _rng(seed, name)
        prefix, leaf = name.rsplit(".", 1)
        is_bn = (prefix + ".running_var") in spec
        is_dcn_main = name.endswith(".conv.weight") and (prefix + ".conv_offset_mask.weight") in spec
        if leaf == "num_batches_tracked":
            v = np.zeros((), dtype=np.int64)
        elif leaf == "running_mean":
            v = g.normal(0.0, 0.1, shape)
        elif leaf == "running_var":
            v = g.uniform(0.8, 1.2, shape)
        elif is_bn and leaf == "weight":
            v = g.uniform(0.8, 1.2, shape)
        elif is_bn and leaf == "bias":
            v = g.normal(0.0, 0.1, shape)
        elif leaf == "bias":
            v = g.normal(0.0, 0.05, shape)
            if "conv_offset_mask" in name:
                v = g.normal(0.0, 0.5, shape)
            if name == "cls.6.bias":                          # class-major: channel = cls*A + a
                v = g.normal(0.0, 0.5, shape)
                v[:num_anchors] += BG_BIAS
        elif ".up_" in name:
            v = _bilinear_up(shape) * g.uniform(0.9, 1.1, (shape[0], 1, 1, 1))
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            if "conv_offset_mask" in name:
                v = g.normal(0.0, 0.7 / math.sqrt(fan_in), shape)
            elif is_dcn_main or name.endswith(".align.weight"):
                stdv = 3.74 / math.sqrt(fan_in)               # uniform like DCNv2.reset_parameters, gain tuned so features keep O(1) spatial variance
                v = g.uniform(-stdv, stdv, shape)
            elif name.startswith("bbox_z3d_gl.0"):
                v = g.normal(0.0, 1.0 / math.sqrt(fan_in), shape)
                if name.endswith(("query_conv.weight", "key_conv.weight")):
                    # unit-gain random query / key projections of O(10) features give attention logits of +-2800 over the 337
                    # keys: a saturated (one-hot) softmax whose output flips on fp32 roundoff -- the float64 run of the
                    # oracle graph then differs from its own float32 run by 6e-4 in z3d (tools/truth_probe.py), and the
                    # P.V product is hardly exercised.  0.1 on each side puts the logits at std ~2, max ~25 (mean top weight
                    # 0.3 at 1280x384): a working attention block, conditioned like a trained one.
                    v = v * ANAB_QK_GAIN
            else:
                v = g.normal(0.0, 0.8 * math.sqrt(2.0 / fan_in), shape)
                if name.startswith("bbox_") and name.endswith(".6.weight"):
                    v = v * BOX_OUT_GAIN                      # regression deltas ~N(0, 0.3): realistic align offsets
                if deep and name.startswith("base.base.level"):
                    v = v * _dla102_gain(name)
        dt = torch.int64 if leaf == "num_batches_tracked" else torch.float32
        sd[name] = torch.from_numpy(np.asarray(v)).to(dt).reshape(shape)
    return sd


def synth_conf(crop_size=(384, 1280), seed=0, batch_size=1, device="cuda:0", shape_align=True, center_align=True,
               attention="ANAB", back_bone="dla34"):
    """Stand-in for the pickled training conf: 2-D anchors from the reference recipe
    (lib/rpn_util.py:39-52,167-183), seeded 3-D anchor columns and bbox_means/stds."""
    rng = np.random.Generator(np.random.PCG64([seed, 0xC0F]))
    conf = Config(back_bone=back_bone)
    conf.attention, conf.center_align, conf.shape_align = attention, center_align, shape_align
    conf.crop_size = list(crop_size)
    conf.batch_size = batch_size
    conf.device = device
    a2d = rpn_util.generate_anchors_2d(conf.anchor_scales, conf.anchor_ratios, conf.feat_stride)
    n = a2d.shape[0]
    a3d = np.zeros((n, 5), dtype=np.float32)
    a3d[:, 0] = rng.uniform(5.0, 60.0, n)
    a3d[:, 1] = rng.normal(1.6, 0.1, n)
    a3d[:, 2] = rng.normal(1.5, 0.1, n)
    a3d[:, 3] = rng.normal(3.9, 0.3, n)
    a3d[:, 4] = rng.uniform(-1.0, 1.0, n)
    conf.anchors = np.concatenate([a2d, a3d], axis=1).astype(np.float32)
    conf.bbox_means = rng.normal(0.0, 0.05, (1, 11)).astype(np.float32)
    conf.bbox_stds = rng.uniform(0.1, 0.6, (1, 11)).astype(np.float32)
    return conf


def synth_frames(batch, crop_size=(384, 1280), seed=1234, pad_right_third=False):
    """randn frames (~ normalised-image statistics); optionally the right
    third zeroed, mimicking the test-time Padding (lib/augmentations.py:135-160)."""
    g = np.random.Generator(np.random.PCG64([seed, batch, crop_size[0], crop_size[1]]))
    x = g.standard_normal((batch, 3, crop_size[0], crop_size[1]), dtype=np.float32)
    if pad_right_third:
        x[:, :, :, (2 * crop_size[1]) // 3:] = 0.0
    return torch.from_numpy(x)


def synth_boxes(n, seed=0):
    """SURVEY.md 8d NMS micro-bench: centres U([0,1280]x[0,384]), w,h U(5,200)xU(5,150),
    distinct scores = permutation / n."""
    g = np.random.Generator(np.random.PCG64([seed, n, 0xB0]))
    c = g.uniform([0, 0], [1280, 384], (n, 2))
    wh = g.uniform([5, 5], [200, 150], (n, 2))
    s = (g.permutation(n).astype(np.float64) + 1.0) / n
    return np.concatenate([c - wh / 2, c + wh / 2, s[:, None]], axis=1).astype(np.float32)
