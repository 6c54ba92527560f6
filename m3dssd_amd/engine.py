"""Inference engine: the whole RPN.forward of M3DSSD as a fixed sequence of HIP kernel launches.

Design (MI355X-first):
  * activations live in HBM as NHWC fp32; channel concatenations (DLA ``Root`` inputs) are never
    materialised -- producers write straight into channel slices of one buffer (``View.slice``);
  * every conv / DCN is one ``m3d_conv2d_forward`` launch with BatchNorm(eval) + bias folded into a
    per-channel affine, residual add and LeakyReLU in the epilogue;
  * parameters are folded / packed once (``Engine.__init__``), buffers and launch descriptors are
    built once per input shape (``_Plan``) and replayed; PyTorch only owns device memory + streams;
  * the backbone of a plan is one walk, ``Engine._dla_levels`` (the Trees of level2 .. level5, driven by ``BACKBONE_TREES``) and
    ``Engine._dla_up`` (DLAUp / IDAUp), for DLA-34 and DLA-102 and for this engine and the bf16 one (``engine_bf16.EngineBF16``):
    an engine supplies the primitives the walk calls -- ``_front`` (everything up to level1), ``_act``, ``_layer``, ``_offmask``,
    ``_maxpool``, ``_upsample_add``, ``_tree_entry`` -- and its own RPN stage (``_rpn_ops``, on the shared ``_rpn_*`` steps).

Reference graph being executed: model/M3d_inference_align.py:215-313 (RPN.forward),
model/pose_dla_dcn.py:391-397,314-327,546-578,687-696 (DLA-34, Tree, IDAUp, DLAUp, DLASeg), :162-200,261-269,435-441
(DLA-102: Bottleneck, residual Root),
model/DCNv2/dcn_v2.py:64-70 (DCN), model/module/feturealign_mgpu.py:48-99,153-208,
model/module/attention.py:183-216.
"""
import collections
import ctypes
import math
import os

import numpy as np
import torch

from . import _hip
from ._hip import ConvDesc, MlpDesc
from .config import model_flags

BN_EPS = 1e-5
SELECT_KEYS = os.environ.get("M3D_SELECT_KEYS", "1") != "0"     # anchor_select also writes the detection stage's sort keys
# Detection-only tail (plan.tail: box heads at the needed pixels only).  A detector asked with sparse_heads=None takes it when at
# most this fraction of an image's pixels can hold one of the nms_topN_pre rows (min(k, HW) / HW); DESIGN.md section 3, "needed
# pixels", has the measured cost of the selection pass that the constant stands for.
SPARSE_HEADS_MAX_FRACTION = 0.5
PSP_SIZES = (1, 4, 8, 16)
# channels of the stem, level0 .. level5 (pose_dla_dcn.py:419-440); channels[3] is the width of feats0 and every map after it
BACKBONE_CHANNELS = {"dla34": (16, 32, 64, 128, 256, 512), "dla102": (16, 32, 128, 256, 512, 1024)}
# what the one walk of level2 .. level5 (Engine._dla_levels) and the one packer of their Trees need to know of a backbone: the depths
# of the four Trees, the convs of a block (2: BasicBlock, 3: Bottleneck), and whether a Root adds children[0] to its output
BACKBONE_TREES = {"dla34": ((1, 2, 2, 1), 2, False), "dla102": ((1, 3, 4, 1), 3, True)}
# the box heads in the order of their rows in the planar box staging [B][11][A][HW]
BOX_HEADS = ("bbox_x", "bbox_y", "bbox_w", "bbox_h", "bbox_x3d", "bbox_y3d", "bbox_z3d", "bbox_w3d", "bbox_h3d", "bbox_l3d", "bbox_rY3d")


def _rup(a, b):
    return (a + b - 1) // b * b


class View:
    """NHWC view (possibly a channel slice) of a device buffer."""
    __slots__ = ("t", "ptr", "n", "h", "w", "c", "cs", "keep")

    def __init__(self, t, n, h, w, c, cs=None, ptr=None):
        self.t, self.n, self.h, self.w, self.c = t, n, h, w, c
        self.cs = c if cs is None else cs
        self.ptr = t.data_ptr() if ptr is None else ptr

    def slice(self, c0, c):
        assert c0 % 4 == 0 and c0 + c <= self.cs
        return View(self.t, self.n, self.h, self.w, c, self.cs, self.ptr + 4 * c0)

    def torch_nchw(self):
        """Debug helper: materialise as an NCHW torch tensor (copies)."""
        full = self.t.view(self.n, self.h, self.w, self.cs)
        off = (self.ptr - self.t.data_ptr()) // 4
        return full[..., off:off + self.c].permute(0, 3, 1, 2).contiguous()


class _Stream:
    @staticmethod
    def current(device=None):
        return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def fold_affine(device, cout, bias=None, bn=None):
    """Per-channel fp32 (scale, shift) that stand for a conv's bias and the BatchNorm(eval) behind it, bn = (weight, bias,
    running_mean, running_var): y = conv(x) * scale + shift."""
    scale = torch.ones(cout, device=device, dtype=torch.float32)
    shift = torch.zeros(cout, device=device, dtype=torch.float32)
    if bias is not None:
        shift = bias.detach().to(device, torch.float32).clone()
    if bn is not None:
        g, b, m, v = (t.detach().to(device, torch.float32) for t in bn)
        scale = g / torch.sqrt(v + BN_EPS)
        shift = (shift - m) * scale + b
    return scale.contiguous(), shift.contiguous()


class PackedConv:
    """Packed weights + folded affine of one conv (or DCN main conv)."""

    def __init__(self, eng, weight, bias=None, bn=None, cout_pad_to=32, cin_pad=None):
        w = weight.detach().to(eng.device, torch.float32).contiguous()
        self.cout, self.cin, self.kh, self.kw = w.shape
        self.cin_pad = self.cin if cin_pad is None else cin_pad
        self.cout_pad = _rup(self.cout, cout_pad_to)
        self.wp = torch.empty(self.cout_pad * self.kh * self.kw * self.cin_pad, device=eng.device, dtype=torch.float32)
        _hip.check(eng.L.m3d_pack_conv_weight(w.data_ptr(), self.wp.data_ptr(), self.cout, self.cout_pad, self.cin,
                                              self.cin_pad, self.kh, self.kw, _Stream.current()))
        self.scale, self.shift = fold_affine(eng.device, self.cout, bias, bn)
        self.has_affine = (bias is not None) or (bn is not None)
        self._eng_device = eng.device
        self._frag = None
        self.wino = None
        self._w_cpu = None
        if USE_WINO and self.kh == 3 and self.kw == 3 and self.cin_pad == self.cin and self.cin % 16 == 0 and self.cin >= 32:
            self.wino = pack_wino(w, self.cout_pad, eng.device)
            if USE_WINO44 and self.cout_pad % 64 == 0:
                self._w_cpu = w.detach().cpu()            # F(4x4,3x3) weights are packed on first use (wino44())
        self._wino44 = None

    def wino44(self):
        """U = G g G^T of Winograd F(4x4,3x3) in the fragment order of m3d_wino44_conv3x3_forward, or None."""
        if self._wino44 is None and self._w_cpu is not None:
            self._wino44 = pack_wino44(self._w_cpu, self.cout_pad, self._eng_device)
        return self._wino44


    def frag(self):
        """The packed [Cout_pad, kh*kw*Cin_pad] matrix in MFMA-fragment order (m3d_conv_wave_forward), built on demand."""
        if self._frag is None:
            k = self.kh * self.kw * self.cin_pad
            self._frag = pack_frag(self.wp.view(self.cout_pad, k), self.cout_pad, self._eng_device)
        return self._frag


def pack_frag(weight2d, rows_pad, device):
    """[R, K] -> MFMA-fragment order for m3d_head_mlp_forward: [R/32][K/8][h=2][r=32][t=4] (rows zero-padded)."""
    w = weight2d.detach().to(device, torch.float32)
    r, k = w.shape
    assert k % 8 == 0 and rows_pad % 32 == 0 and rows_pad >= r
    if rows_pad != r:
        w = torch.cat([w, w.new_zeros(rows_pad - r, k)], 0)
    return w.view(rows_pad // 32, 32, k // 8, 2, 4).permute(0, 2, 3, 1, 4).contiguous().view(-1)


_WINO_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)


def pack_wino(weight, cout_pad, device):
    """[Cout, Cin, 3, 3] -> Winograd F(2x2,3x3) weights U = G g G^T (computed in fp64, rounded once to fp32) in
    MFMA-fragment order [16 xi][Cout_pad/32][Cin/8][h=2][r=32][t=4] for m3d_wino_conv3x3_forward."""
    g = weight.detach().to("cpu", torch.float64)
    co, ci = g.shape[0], g.shape[1]
    assert g.shape[2:] == (3, 3) and ci % 8 == 0 and cout_pad % 32 == 0 and cout_pad >= co
    u = torch.einsum("ai,ocij,bj->aboc", _WINO_G, g, _WINO_G).reshape(16, co, ci)
    if cout_pad != co:
        u = torch.cat([u, u.new_zeros(16, cout_pad - co, ci)], 1)
    u = u.view(16, cout_pad // 32, 32, ci // 8, 2, 4).permute(0, 1, 3, 4, 2, 5).contiguous()
    return u.to(torch.float32).reshape(-1).to(device)


_WINO44_G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                          [0, 0, 1]], dtype=torch.float64)


def pack_wino44(weight, cout_pad, device):
    """[Cout, Cin, 3, 3] -> Winograd F(4x4,3x3) weights U = G g G^T (6 x 6 per filter, computed in fp64, rounded once to fp32) in
    the B-fragment order of v_mfma_f32_16x16x4_f32 for m3d_wino44_conv3x3_forward: [Cout_pad/32][Cin/16][36 xi][j 2][lane 64][e 4]
    with value U[xi][cin = 16 s + 4 (lane >> 4) + e][cout = 32 cb + 16 j + (lane & 15)]."""
    g = weight.detach().to("cpu", torch.float64)
    co, ci = g.shape[0], g.shape[1]
    assert g.shape[2:] == (3, 3) and ci % 16 == 0 and cout_pad % 32 == 0 and cout_pad >= co
    u = torch.einsum("ai,ocij,bj->aboc", _WINO44_G, g, _WINO44_G).reshape(36, co, ci)
    if cout_pad != co:
        u = torch.cat([u, u.new_zeros(36, cout_pad - co, ci)], 1)
    # [xi][cb][j][n16][s][q][e] -> [cb][s][xi][j][q][n16][e]   (lane = q * 16 + n16)
    u = u.view(36, cout_pad // 32, 2, 16, ci // 16, 4, 4).permute(1, 4, 0, 2, 5, 3, 6).contiguous()
    return u.to(torch.float32).reshape(-1).to(device)


def pack_wino44_c16(weight, device):
    """[16, 16, 3, 3] -> U = G g G^T for m3d_conv3x3_c16_wino (DLA level0): [36 xi][64 lanes = 16 (cin / 4) + cout][cin % 4], fp64 -> fp32."""
    g = weight.detach().to("cpu", torch.float64)
    assert tuple(g.shape) == (16, 16, 3, 3)
    u = torch.einsum("ai,ocij,bj->abco", _WINO44_G, g, _WINO44_G).reshape(36, 4, 4, 16)      # xi, cin / 4, cin % 4, cout
    return u.permute(0, 1, 3, 2).contiguous().to(torch.float32).reshape(-1).to(device)


WINO_MIN_BLOCKS = int(os.environ.get("M3D_WINO_MIN_BLOCKS", "128"))
FUSED_ANAB = os.environ.get("M3D_FUSED_ANAB", "1") != "0"       # logits + softmax + P.V of ANAB in one launch (csrc/anab_attend.hip)
# detection-only tail: the one-launch attention at the listed pixels only (m3d_anab_attend_f32_rows); 0: the dense launch there too.
# On by default: it met the step-time criterion ("The ANAB attention at the needed pixels").
ANAB_ROWS = os.environ.get("M3D_ANAB_ROWS", "1") != "0"
USE_ANAB_WAVE = os.environ.get("M3D_ANAB_WAVE", "1") != "0"
USE_ANAB_NESTED = os.environ.get("M3D_ANAB_NESTED", "1") != "0"
USE_DCN_WAVE = os.environ.get("M3D_DCN_WAVE", "1") != "0"
USE_CONV_WAVE = os.environ.get("M3D_CONV_WAVE", "1") != "0"
# thin wave-kernel layers: the K slices are the waves of one workgroup (m3d_conv_wave_forward_wgsplit, no workspace);
# M3D_CONV_WAVE_WGSPLIT=0 restores the global split (workspace + reduce launch) for A/B runs
USE_CONV_WAVE_WGSPLIT = os.environ.get("M3D_CONV_WAVE_WGSPLIT", "1") != "0"
# the 27 -> 32 channel offset / mask convs of the 24x80 maps (plans of up to 4 slices) on the one-column-tile form of the same
# kernel (0: split-K igemm).  The 12x40 one (8 slices) stays on the igemm: 29.7 us there against ~27 us for igemm + reduce.
USE_OFFMASK_WAVE = os.environ.get("M3D_OFFMASK_WAVE", "1") != "0"
USE_WINO = os.environ.get("M3D_WINO", "1") != "0"
USE_WINO44 = os.environ.get("M3D_WINO44", "1") != "0"
# F(4x4,3x3) workgroups (16 tiles x 128 or 64 channels, one per CU, 256 CUs): 128-channel workgroups need >= 200 of them; the
# 64-channel form (half the MFMAs per transformed input) pays from ~2 rounds on: in the network, bs 8, level2 (64 -> 64 @ 96x320,
# 960 workgroups) gains 10 %, level4 (256 -> 256 @ 24x80, 240 workgroups) loses 5 % against the F(2x2,3x3) wave kernel
WINO44_TOUCH = os.environ.get("M3D_WINO44_TOUCH", "1") != "0"
WINO44_TOUCH_SPAN = int(os.environ.get("M3D_WINO44_TOUCH_SPAN", "2"))   # launches between two F(4x4) layers that a folded touch bridges
USE_WINO44_SPLITK = os.environ.get("M3D_WINO44_SPLITK", "1") != "0"
W44_SPLIT_NB = 2 if os.environ.get("M3D_W44_SPLIT_NB", "1") == "2" else 1    # form of the split-K launches (csrc/wino44_conv.hip)
W44_SPLIT_KPAIR = os.environ.get("M3D_W44_SPLIT_NB", "1") == "3"             # ... K-pair workgroups inside every slice
# Round 4: the 64-channel form runs TWO workgroups per CU (wino44_kernel<1, 2>) and beats the 128-channel form on every layer
# (128 -> 128 @ 48x160: 0.056 vs 0.065 ms, 128 -> 256: 0.114 vs 0.130); the 128-channel form is kept for experiments
# (M3D_WINO44_MIN_WGS=200 restores the round-3 choice).
WINO44_MIN_WGS = int(os.environ.get("M3D_WINO44_MIN_WGS", "1000000"))
WINO44_MIN_WGS_NB1 = int(os.environ.get("M3D_WINO44_MIN_WGS_NB1", "200"))


class OpCost:
    """Algorithmic HBM bytes of a helper launch (the `desc` slot of a plan op that has no conv / head descriptor)."""

    def __init__(self, hbm_bytes):
        self.hbm_bytes = int(hbm_bytes)


def lo_hi_contains(start, end, n, br):
    """Is the side branch (b0, b1, join) wholly inside ops[start:end]?  (A partial range runs its ops in line.)"""
    lo, hi = start, (n if end is None else end)
    return lo <= br[0] and br[2] <= hi


class _Plan:
    """Buffers + launch list for one input shape."""

    def __init__(self):
        self.ops = []          # (name, callable)
        self.keep = []         # tensors kept alive
        self.named = {}        # name -> View / tensor (taps for tests)
        self.w44_prev = None   # (index into ops, touch record) of the latest F(4x4) launch: it warms the cache for the next one
        self.branches = []     # (b0, b1, join): ops [b0, b1) on a side stream beside ops [b1, join) (Engine._run_plan)
        # detection-only tail: ops that stand in for ops[tail_start:-1] (everything behind anchor_select but bundle_outputs) when
        # only the top-k decode reads the box staging (Engine.run_plan(tail=True)); None: the plan has none
        self.tail = None
        self.tail_start = None
        # index into ops -> factory(rpn stage record) of the launch that stands in for that op in the tail (its row-list / gated
        # form), registered where the dense op is appended; the tail takes it for ops behind anchor_select (Engine._rpn_tail)
        self.sparse = {}
        # The tail in two parts (Engine._rpn_post3d): tail_pre = the tail without the launches whose outputs feed columns 8..12 of
        # a decoded row and nothing else, post3d = those launches on the list of the pixels that survive the NMS
        # (plan.post_rows / plan.post_n_rows, written by m3d_post_rows).  None: the engine does not offer the split.
        self.tail_pre = None
        self.post3d = None
        self.post_rows = self.post_n_rows = None
        self.post3d_reads = []     # (tensor, index of the first op that writes it) of every map a post3d launch reads
        # index into ops -> (pre, post, reads), registered where the dense op is appended: pre = the op's form in tail_pre (None:
        # it has none there), post = its form in post3d, each (factory(rpn stage record), name, flops, desc) with None = the
        # dense op's; reads = the tensors the post form reads
        self.deferred = {}
        self.post3d_declined = None    # why the builder of an op rules the split out, if it does
        self.first_write = {}      # data_ptr of a buffer -> index of the first op that writes it (the buffers `wrote` was told of)

    def sparse_form(self, factory):
        """Register the detection-only form of the op appended last."""
        self.sparse[len(self.ops) - 1] = factory

    def deferred_form(self, pre, post, reads):
        """Register the two forms of the op appended last in the split tail (see `deferred`)."""
        self.deferred[len(self.ops) - 1] = (pre, post, list(reads))

    def wrote(self, *tensors):
        """The op appended last writes these buffers."""
        for t in tensors:
            self.first_write.setdefault(t.data_ptr(), len(self.ops) - 1)


class _RpnStage:
    """State of the RPN stage of one plan, shared by the steps both plan builders make it from (Engine._rpn_*): sizes, the planar
    fp32 staging of the head outputs, and what anchor_select, the output bundling and the tail's selection pass add to it."""

    def __init__(self, B, A, NC, fh, fw):
        self.B, self.A, self.NC, self.fh, self.fw = B, A, NC, fh, fw
        self.HW = fh * fw
        self.R = A * self.HW

    def box_planar(self, k):
        return (self.box_pl, 11 * self.A * self.HW, k * self.A)

    def box_ptr(self, k):
        return self.box_pl.data_ptr() + 4 * k * self.A * self.HW          # image 0; per-image stride handled via [B][11][A][HW]


def conv_desc(name, pc, x, out, stride, pad, act=0, res=None, res_mode=0, sigmoid_from=-1, om=None, affine=True, wgt_ptr=None,
              wgt_img_stride=0, cout=None, cout_pad=None, scale=None, shift=None, kh=None, kw=None):
    """The m3d_conv_desc of one layer: weights and sizes from the packed conv `pc`, or, with pc = None, from wgt_ptr (+
    wgt_img_stride) / cout / cout_pad / kh / kw; input x, NHWC output view `out`; epilogue = scale / shift (given, or pc's folded
    affine unless affine = False), residual, act / sigmoid_from; om = the offset / mask map of a deformable layer."""
    assert (pc is None) != (wgt_ptr is None), name
    d = ConvDesc()
    d.inp, d.in_cs, d.N, d.H, d.W, d.Cin = x.ptr, x.cs, x.n, x.h, x.w, x.c
    d.wgt, d.wgt_img_stride = (pc.wp.data_ptr() if pc is not None else wgt_ptr), wgt_img_stride
    d.Cout = pc.cout if cout is None else cout
    d.Cout_pad = pc.cout_pad if cout_pad is None else cout_pad
    d.kh, d.kw, d.stride, d.pad, d.dil = (pc.kh if kh is None else kh), (pc.kw if kw is None else kw), stride, pad, 1
    d.Ho = (x.h + 2 * pad - d.kh) // stride + 1
    d.Wo = (x.w + 2 * pad - d.kw) // stride + 1
    assert out.h == d.Ho and out.w == d.Wo and out.c >= d.Cout, (name, out.h, out.w, d.Ho, d.Wo)
    d.out, d.out_cs = out.ptr, out.cs
    if scale is not None:
        d.scale, d.shift = scale.data_ptr(), shift.data_ptr()
    elif affine and pc is not None and pc.has_affine:
        d.scale, d.shift = pc.scale.data_ptr(), pc.shift.data_ptr()
    if res is not None:
        d.res, d.res_cs, d.res_mode = res.ptr, res.cs, res_mode
    d.act, d.sigmoid_from = act, sigmoid_from
    if om is not None:
        d.dcn_offmask, d.dcn_om_cs = om.ptr, om.cs
    return d


def desc_with(d, **fields):
    """A copy of descriptor d with `fields` set: a route of Engine._conv never changes the descriptor it was asked about."""
    c = type(d).from_buffer_copy(d)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def conv_kind(family, tile=(), deform=False, splitk=1, wgsplit=1, kpair=False, per_image=False):
    """The kind of a conv op: "family<tile,options>", the options in this order (bench.py and profiles/ key on the strings)."""
    parts = [str(t) for t in tile] + ["deform"] * deform + ["splitk%d" % splitk] * (splitk > 1) \
        + ["wgsplit%d" % wgsplit] * (wgsplit > 1) + ["kpair"] * kpair + ["per_image"] * per_image
    return family + ("<%s>" % ",".join(parts) if parts else "")


# what a route of Engine._conv answers when it takes a layer: kind (family, tile, conv_kind's options), launch closure, the
# descriptor it launches (slot 4 of the op) and the tensors the plan has to keep alive for it
_Route = collections.namedtuple("_Route", "family tile options launch desc keep")


class Engine:
    def __init__(self, state_dict, conf, device=None, backbone_only=False):
        self.L = _hip.lib()
        self.backbone_only = backbone_only
        self.device = torch.device(device if device is not None else conf.device)
        if self.device.type != "cuda":
            raise NotImplementedError("the M3DSSD HIP engine runs on a ROCm device only (got %s)" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.conf = conf
        self.back_bone = str(conf.back_bone) if "back_bone" in conf else "dla34"
        if self.back_bone not in BACKBONE_CHANNELS:
            raise NotImplementedError("back_bone %r: the engine runs %s" % (self.back_bone, " / ".join(BACKBONE_CHANNELS)))
        if getattr(self, "compute_dtype", "f32") == "bf16" and self.back_bone != "dla34":
            raise NotImplementedError("the bf16 engine runs the dla34 backbone only; run back_bone %r in fp32" % self.back_bone)
        sd = {k[7:] if k.startswith("module.") else k: v for k, v in state_dict.items()}
        self.sd = sd
        self.A = int(np.asarray(conf.anchors).shape[0]) if not backbone_only else 0
        self.NC = len(conf.lbls) + 1 if not backbone_only else 0
        self.stride = int(conf.feat_stride)
        # (shape_align, center_align, anab): which stages the plan runs (M3d_inference_align.py:241-277)
        self.flags = model_flags(conf) if not backbone_only else (False, False, False)
        with torch.cuda.device(self.device):
            self._pack(sd)
        self.plans = {}
        self.profile = None    # set to a list to collect (name, kind, flops, ms) per op (HIP events on the launch stream)
        self.profile_kinds = None   # optional set: only ops of these kinds are bracketed with events
        self._pending = []

    # ------------------------------------------------------------------ parameters
    def _bn(self, p):
        sd = self.sd
        return (sd[p + ".weight"], sd[p + ".bias"], sd[p + ".running_mean"], sd[p + ".running_var"])

    def _pc(self, conv, bn=None, **kw):
        sd = self.sd
        return PackedConv(self, sd[conv + ".weight"], sd.get(conv + ".bias"), self._bn(bn) if bn else None, **kw)

    DCN_PACK = dict(cout_pad_to=64)     # how _pc packs the main conv of a DCN (the bf16 engine pads none)

    def _pack_front(self, sd, P):
        """Front-end extras of this engine: level0 also as a direct VALU conv, weights [(i*3+j)*16 + cin][cout], and as F(4x4,3x3)."""
        w0 = sd["base.base.level0.0.weight"].detach().to(self.device, torch.float32)
        c16 = tuple(w0.shape) == (16, 16, 3, 3)
        P["level0.direct"] = w0.permute(2, 3, 1, 0).contiguous() if c16 else None
        P["level0.wino44"] = pack_wino44_c16(w0, self.device) if (USE_WINO44 and c16) else None

    def _pack(self, sd):
        dev = self.device
        P = {}
        b = "base.base"
        # stem 7x7: [16,3,7,7] -> [(i*7+j)*3+c][16]
        w = sd[b + ".base_layer.0.weight"].detach().to(dev, torch.float32)
        P["stem.w"] = w.permute(2, 3, 1, 0).contiguous()
        P["stem.scale"], P["stem.shift"] = fold_affine(dev, w.shape[0], None, self._bn(b + ".base_layer.1"))
        P["level0"] = self._pc(b + ".level0.0", b + ".level0.1")
        P["level1"] = self._pc(b + ".level1.0", b + ".level1.1")
        self._pack_front(sd, P)

        depths, block_convs, _ = BACKBONE_TREES[self.back_bone]

        def tree(p, levels):
            """Any Tree: leaves carry the two blocks, the root and the project.  The project of a Tree of depth > 1 is computed by
            the reference and then ignored (its tree1 computes its own): not packed."""
            if levels > 1:
                tree(p + ".tree1", levels - 1)
                tree(p + ".tree2", levels - 1)
                return
            for blk in (p + ".tree1", p + ".tree2"):
                for i in range(1, block_convs + 1):
                    P["%s.conv%d" % (blk, i)] = self._pc("%s.conv%d" % (blk, i), "%s.bn%d" % (blk, i))
            P[p + ".root"] = self._pc(p + ".root.conv", p + ".root.bn")
            if (p + ".project.0.weight") in sd:
                P[p + ".project"] = self._pc(p + ".project.0", p + ".project.1")

        for lv, levels in zip((2, 3, 4, 5), depths):
            tree("%s.level%d" % (b, lv), levels)

        def deform(p):
            P[p + ".om"] = self._pc(p + ".conv.conv_offset_mask")
            P[p + ".dcn"] = self._pc(p + ".conv", p + ".actf.0", **self.DCN_PACK)

        def ida(p, n):
            for i in range(1, n):
                deform("%s.proj_%d" % (p, i))
                deform("%s.node_%d" % (p, i))
                up = sd["%s.up_%d.weight" % (p, i)].detach().to(dev, torch.float32)     # [C,1,4,4]
                P["%s.up_%d" % (p, i)] = up[:, 0].permute(1, 2, 0).contiguous()          # [4][4][C]

        ida("base.dla_up.ida_0", 2)
        ida("base.dla_up.ida_1", 3)
        ida("base.ida_up", 2)

        self.P = P
        if not self.backbone_only:
            self._pack_heads(sd, P)
        torch.cuda.synchronize(self.device)

    def _pack_anab(self, P, wq, wk, wv, ws):
        """One fused 1x1 conv producing [Q (168 -> 192 pad) | K 168 | V 128 | S 4], sigmoid on S."""
        self.ck, self.cv, self.ns = wq.shape[0], wv.shape[0], ws.shape[0]
        self.ck_pad = _rup(self.ck, 32)
        cin = wq.shape[1]
        zpad = torch.zeros(self.ck_pad - self.ck, cin, 1, 1)
        wall = torch.cat([wq.detach().cpu().float(), zpad, wk.detach().cpu().float(), wv.detach().cpu().float(),
                          ws.detach().cpu().float()], 0)
        P["anab.qkvs"] = PackedConv(self, wall, None, None)
        self.anab_off = dict(q=0, k=self.ck_pad, v=self.ck_pad + self.ck, s=self.ck_pad + self.ck + self.cv)
        self.anab_ctot = wall.shape[0]

    def _pack_head(self, sd, P, p):
        """The three layers of head p, and the 1x1 ones also in the fragment order of the fused-MLP kernel."""
        P[p + ".0"] = self._pc(p + ".0", p + ".1")
        P[p + ".3"] = self._pc(p + ".3", p + ".4")
        P[p + ".6"] = self._pc(p + ".6", cout_pad_to=256 if p == "cls" else 64)   # fused-MLP output tile
        for li, rows in ((".0", 256), (".3", 256), (".6", P[p + ".6"].cout_pad)):
            wt = sd[p + li + ".weight"]
            if wt.shape[2] == 1:                                                    # 1x1 layers only
                P[p + li + ".frag"] = pack_frag(wt.reshape(wt.shape[0], wt.shape[1]), rows, self.device)

    def _pack_heads(self, sd, P):
        """Heads, align stages and ANAB; an engine packs the layers its own kernels read in _pack_head / _pack_anab."""
        dev = self.device
        self.box_heads = list(BOX_HEADS)
        for h in ["cls"] + self.box_heads:
            self._pack_head(sd, P, h)
        with_shape, with_center, with_anab = self.flags
        for p in ("shape_align",) * with_shape + ("center_align2d", "center_align3d") * with_center:
            P[p] = self._pc(p + ".align", **self.DCN_PACK)
        if with_anab:
            a = "bbox_z3d_gl.0"
            self._pack_anab(P, sd[a + ".query_conv.weight"], sd[a + ".key_conv.weight"], sd[a + ".value_conv.weight"],
                            sd[a + ".spatial_conv.weight"])
            bn = self._bn("bbox_z3d_gl.1")
            P["anab.bn.scale"], P["anab.bn.shift"] = fold_affine(dev, bn[0].shape[0], None, bn)

        # constants of the align stages
        anchors = torch.as_tensor(np.asarray(self.conf.anchors), dtype=torch.float32)
        aw = (anchors[:, 2] - anchors[:, 0])
        ah = (anchors[:, 3] - anchors[:, 1])
        tab = torch.zeros(self.A, 18, dtype=torch.float32)
        h_step, w_step = ah / self.stride / 3, aw / self.stride / 3        # feturealign_mgpu.py:119-136
        for i in range(3):
            for j in range(3):
                k = i * 3 + j
                tab[:, 2 * k] = (h_step - 1) * (i - 3 / 2 + 0.5)
                tab[:, 2 * k + 1] = (w_step - 1) * (j - 3 / 2 + 0.5)
        P["shape.table"] = tab.to(dev).contiguous()
        P["anchor_wh"] = torch.stack([aw / self.stride, ah / self.stride], 1).to(dev).contiguous()
        P["anchors"] = anchors.to(dev).contiguous()
        P["means"] = torch.as_tensor(np.asarray(self.conf.bbox_means), dtype=torch.float32).reshape(-1).to(dev)
        P["stds"] = torch.as_tensor(np.asarray(self.conf.bbox_stds), dtype=torch.float32).reshape(-1).to(dev)

    # ------------------------------------------------------------------ launch helpers
    def _buf(self, plan, n, h, w, c, cs=None, name=None, zero=False):
        cs = c if cs is None else cs
        t = (torch.zeros if zero else torch.empty)(n * h * w * cs, device=self.device, dtype=torch.float32)
        plan.keep.append(t)
        v = View(t, n, h, w, c, cs)
        if name:
            plan.named[name] = v
        return v

    def _conv(self, plan, name, pc, x, out, stride=1, pad=0, cin_true=None, wgt_frag=False, per_image=False, **layer):
        """Append one convolution: its descriptor (conv_desc takes `layer`), launched by the first kernel family that takes it: F(4x4)
        Winograd, F(2x2) Winograd, wave kernel on the caller's fragment-ordered weights (wgt_frag), wave kernel, implicit GEMM.
        cin_true: the input channels the FLOPs count (default: pc's, or x's); per_image only marks the kind (image_gemm)."""
        d = conv_desc(name, pc, x, out, stride, pad, **layer)
        plan.keep += [layer[k] for k in ("scale", "shift") if layer.get(k) is not None]
        route = (self._route_wino44(plan, name, d, pc) or self._route_wino(d, pc) or self._route_frag(name, d, wgt_frag)
                 or self._route_wave(d, pc) or self._route_igemm(d))
        plan.keep += route.keep
        # algorithmic FLOPs of the layer: 2 * pixels * Cout * taps * Cin (true channel counts, no padding)
        cin_true = cin_true if cin_true is not None else pc.cin if pc is not None else x.c
        flops = 2.0 * d.N * d.Ho * d.Wo * d.Cout * d.kh * d.kw * cin_true
        kind = conv_kind(route.family, route.tile, deform=d.dcn_offmask is not None, per_image=per_image, **route.options)
        plan.ops.append((name, kind, flops, route.launch, route.desc))
        plan.wrote(out.t)

    def _launch(self, fn, d, *args):
        """The launch closure of a descriptor entry point: fn(d, *args, stream)."""
        ref = ctypes.byref(d)
        return lambda st: _hip.check(fn(ref, *args, st))

    def _splitk(self, plan_fn, d, workspace=lambda splits: True):
        """Split-K of d as the library's `plan_fn` plans it -> (splits, the descriptor to launch, tensors to keep): a copy of d with
        a fresh workspace where the plan splits and names scratch bytes (and `workspace(splits)` holds), else d itself."""
        splits, nbytes = ctypes.c_int(), ctypes.c_longlong()
        _hip.check(plan_fn(ctypes.byref(d), ctypes.byref(splits), ctypes.byref(nbytes)))
        if splits.value > 1 and nbytes.value > 0 and workspace(splits.value):
            ws = torch.empty(nbytes.value // 4, device=self.device, dtype=torch.float32)
            return splits.value, desc_with(d, splitk_ws=ws.data_ptr(), splitk_ws_bytes=nbytes.value), [ws]
        return splits.value, d, []

    def _route_wino44(self, plan, name, d, pc):
        """Winograd F(4x4,3x3): 4x fewer MFMA FLOPs than the direct convolution (F(2x2,3x3): 2.25x) where the layer fills the chip
        with 16-tile workgroups (csrc/wino44_conv.hip).  The only route that touches the plan: it owns the touch bookkeeping."""
        L = self.L
        if (pc is None or pc._w_cpu is None or d.dcn_offmask is not None or d.sigmoid_from >= 0
                or L.m3d_wino44_applicable(ctypes.byref(d)) != 1):
            return None
        strips = -(-(d.N * d.H * d.W) // 256)
        nb = 2 if (d.Cout_pad % 128 == 0 and strips * (d.Cout_pad // 128) >= WINO44_MIN_WGS) else \
            (1 if strips * (d.Cout_pad // 64) >= WINO44_MIN_WGS_NB1 else 0)
        splits, keep = 1, []
        if not nb and USE_WINO44_SPLITK:
            # small maps (256 -> 256 @ 24x80, 512 -> 512 @ 12x40 at bs 8): K slices as gridDim.z fill the chip, a second launch
            # adds the partial outputs in slice order
            splits, d, keep = self._splitk(L.m3d_wino44_splitk_plan, d)
            nb = W44_SPLIT_NB if splits > 1 else 0
        if not nb:
            return None
        u44 = pc.wino44()
        d = desc_with(d, wgt=u44.data_ptr())
        # U (2.4-38 MB) is cold in HBM when the layer starts and the kernel's B fragments run only ~1400 cycles ahead of the
        # MFMAs: the PREVIOUS F(4x4) launch touches this layer's U (every thread a few lines, under its own first loads); a
        # layer with no F(4x4) launch shortly before it gets a touch launch of its own
        nxt = {"ptr": None, "bytes": 0}
        if WINO44_TOUCH:
            nbytes = u44.numel() * 4
            if plan.w44_prev is not None and len(plan.ops) - plan.w44_prev[0] <= WINO44_TOUCH_SPAN:
                plan.w44_prev[1]["ptr"], plan.w44_prev[1]["bytes"] = u44.data_ptr(), nbytes
            else:
                plan.ops.append((name + ".touch", "touch", 0.0,
                                 lambda st: _hip.check(L.m3d_cache_touch(u44.data_ptr(), nbytes, st)), OpCost(nbytes)))
        plan.w44_prev = (len(plan.ops), nxt)        # (_conv appends this layer's op next)
        kpair = nb == 1 and (L.m3d_wino44_kpair(ctypes.byref(d)) == 1 if splits == 1 else W44_SPLIT_KPAIR)
        ref = ctypes.byref(d)
        return _Route("wino44", (16, 16 * nb), dict(splitk=splits, kpair=kpair),
                      lambda st: _hip.check(L.m3d_wino44_conv3x3_forward_touch(ref, nb, nxt["ptr"], nxt["bytes"], st)),
                      d, keep + [u44])

    def _route_wino(self, d, pc):
        """Winograd F(2x2,3x3): 2.25x fewer MFMA FLOPs for the plain 3x3 stride-1 layers on even maps.  The kernel works on
        256-pixel x 32-channel tiles: a narrow layer (the 27-channel DCN offset / mask convs) on a small map yields fewer than
        WINO_MIN_BLOCKS workgroups and is left to the routes behind this one."""
        L = self.L
        blocks = -(-(d.N * d.H * d.W) // 256) * (d.Cout_pad // 32)
        if (pc is None or pc.wino is None or (d.kh, d.kw, d.stride, d.pad) != (3, 3, 1, 1) or d.dcn_offmask is not None
                or d.H % 2 or d.W % 2 or blocks < WINO_MIN_BLOCKS):
            return None
        # (thin layers: the wave form split along K across waves, where the library recommends it)
        splits, d, keep = self._splitk(L.m3d_wino_conv3x3_splitk_plan, desc_with(d, wgt=pc.wino.data_ptr()))
        launch = self._launch(L.m3d_wino_conv3x3_forward, d)
        if L.m3d_wino_conv3x3_variant(ctypes.byref(d)) == 1:
            return _Route("wino_wave", (32, 32), dict(splitk=splits), launch, d, keep)
        return _Route("wino_lds", (64, 32, 16), {}, launch, d, keep)

    def _route_frag(self, name, d, wgt_frag):
        """Explicit fragment-ordered (per-image) weights: the caller has already decided for the wave-granular kernel."""
        if not wgt_frag:
            return None
        assert d.in_cs % 32 == 0 and d.inp % 128 == 0, name
        if self.L.m3d_conv_wave_applicable(ctypes.byref(d)) <= 0:
            raise RuntimeError("%s: fragment-ordered weights but the wave kernel does not apply" % name)
        return _Route("conv_wave", (), {}, self._launch(self.L.m3d_conv_wave_forward, d), d, [])

    def _route_wave(self, d, pc):
        """Wave-granular kernel (csrc/dcn_wave.hip), plain or deformable.  Thin layers are split along K: across the waves of a
        workgroup (no workspace), or across workgroups through a workspace."""
        L = self.L
        if (pc is None or not (USE_DCN_WAVE if d.dcn_offmask is not None else USE_CONV_WAVE) or d.in_cs % 32 or d.inp % 128
                or pc.cin_pad != d.Cin):
            return None

        def wgsplit(splits):        # (a plan that splits has already passed the fill threshold WITH its split)
            return splits > 1 and USE_CONV_WAVE_WGSPLIT and (d.Cout_pad % 64 == 0 or (USE_OFFMASK_WAVE and splits <= 4))

        splits, dw, keep = self._splitk(L.m3d_conv_wave_splitk_plan, d, workspace=lambda s: not wgsplit(s))
        if wgsplit(splits):
            fn, options = L.m3d_conv_wave_forward_wgsplit, dict(wgsplit=splits)
        elif L.m3d_conv_wave_applicable(ctypes.byref(dw)) > 0:
            fn, options = L.m3d_conv_wave_forward, dict(splitk=splits)
        else:
            return None
        dw = desc_with(dw, wgt=pc.frag().data_ptr())
        return _Route("conv_wave", (), options, self._launch(fn, dw), dw, keep)

    def _route_igemm(self, d):
        """Implicit GEMM (m3d_conv2d_forward): takes every descriptor; layers with too few output tiles are split along K."""
        L = self.L
        bm, bn, bk, grid = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _hip.check(L.m3d_conv2d_tile(ctypes.byref(d), ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(bk), ctypes.byref(grid)))
        splits, d, keep = self._splitk(L.m3d_conv2d_splitk_plan, d)
        return _Route("igemm", (bm.value, bn.value, bk.value), dict(splitk=splits), self._launch(L.m3d_conv2d_forward, d), d, keep)

    def _op(self, plan, name, kind, fn, flops=0.0, nbytes=None):
        """A launch outside the conv / head descriptors: `flops` = arithmetic it executes, `nbytes` = the HBM bytes it has to
        move once (inputs + outputs), so that bench.py can hold it against its own roof (HBM for the element-wise helpers)."""
        plan.ops.append((name, kind, float(flops), fn, OpCost(nbytes) if nbytes is not None else None))

    # ------------------------------------------------------------------ plan construction
    def _build_plan(self, B, H, W):
        """The plan of both engines: the backbone is one walk (_dla_levels, _dla_up) over the primitives an engine implements
        (_front, _act, _layer, _offmask, _maxpool, _upsample_add, _tree_entry); the RPN stage is the engine's own (_rpn_ops)."""
        plan = _Plan()
        l1 = self._front(plan, B, H, W)
        feats0 = self._dla_up(plan, *self._dla_levels(plan, l1))
        if not self.backbone_only:
            self._rpn_ops(plan, feats0)
        return plan

    def _plan_input(self, plan):
        """The plan's input slots and the constants of the uint8 path: (in_ptr, in_u8, mean3, stds3).  in_ptr = [pointer] is set
        by forward() (the caller's NCHW tensor is read in place), in_u8 = [pointer, h, w] of uint8 BGR frames by forward_u8()."""
        in_ptr, in_u8 = [0], [0, 0, 0]
        plan.named["input_ptr"], plan.named["input_u8"] = in_ptr, in_u8
        mean3 = (ctypes.c_float * 3)(*[float(v) for v in self.conf.image_means])
        stds3 = (ctypes.c_float * 3)(*[float(v) for v in self.conf.image_stds])
        return in_ptr, in_u8, mean3, stds3

    # ---- what the backbone walk is made of in this engine: fp32 NHWC maps, one m3d_conv2d_forward-family launch per layer
    _act = _buf                 # an activation map
    _layer = _conv              # one conv layer from a packed conv

    def _front(self, plan, B, H, W):
        """Stem, level0 (in one of its three forms) and level1; returns level1."""
        L, P = self.L, self.P
        in_ptr, in_u8, mean3, stds3 = self._plan_input(plan)
        s0 = self._buf(plan, B, H, W, 16)

        def stem(st):
            if in_u8[0]:                  # test-time input path fused into the stem's loads
                _hip.check(L.m3d_stem_conv7x7_u8(in_u8[0], in_u8[1], in_u8[2], mean3, stds3, P["stem.w"].data_ptr(),
                                                 P["stem.scale"].data_ptr(), P["stem.shift"].data_ptr(), s0.ptr, s0.cs, B, H,
                                                 W, st))
            else:
                _hip.check(L.m3d_stem_conv7x7(in_ptr[0], P["stem.w"].data_ptr(), P["stem.scale"].data_ptr(),
                                              P["stem.shift"].data_ptr(), s0.ptr, s0.cs, B, H, W, st))
        # (bytes: the fp32 NCHW image; with uint8 frames the input is 4x smaller)
        self._op(plan, "stem", "stem", stem, flops=2.0 * B * H * W * 16 * 147, nbytes=B * H * W * (3 + 16) * 4)
        l0 = self._buf(plan, B, H, W, 16, name="level0")
        if P.get("level0.wino44") is not None and H % 4 == 0 and W % 4 == 0 and os.environ.get("M3D_LEVEL0_WINO44", "1") != "0":
            pc0 = P["level0"]       # F(4x4,3x3) on 16x16x4 MFMAs: 144 MFMAs per 256 pixels instead of 576 (csrc/wino44_conv.hip)
            self._op(plan, "level0", "wino44_c16", lambda st: _hip.check(L.m3d_conv3x3_c16_wino(
                s0.ptr, s0.cs, P["level0.wino44"].data_ptr(), pc0.scale.data_ptr(), pc0.shift.data_ptr(), l0.ptr, l0.cs,
                B, H, W, st)), flops=2.0 * B * H * W * 16 * 144, nbytes=B * H * W * 32 * 4)
        elif P["level0.direct"] is not None and os.environ.get("M3D_LEVEL0_IGEMM", "0") != "1":
            pc0 = P["level0"]
            self._op(plan, "level0", "conv3x3_c16", lambda st: _hip.check(L.m3d_conv3x3_c16(
                s0.ptr, s0.cs, P["level0.direct"].data_ptr(), pc0.scale.data_ptr(), pc0.shift.data_ptr(), l0.ptr, l0.cs,
                B, H, W, st)), flops=2.0 * B * H * W * 16 * 144, nbytes=B * H * W * 32 * 4)
        else:
            self._conv(plan, "level0", P["level0"], s0, l0, 1, 1, act=1)
        l1 = self._buf(plan, B, H // 2, W // 2, 32, name="level1")
        self._conv(plan, "level1", P["level1"], l0, l1, 2, 1, act=1)
        return l1

    def _offmask(self, plan, p, x):
        """The 27 offset / mask channels of DCN p over x (18 offsets, 9 sigmoid masks), from its own 3x3 conv."""
        om = self._buf(plan, x.n, x.h, x.w, 27, 28)
        self._conv(plan, p + ".offset_mask", self.P[p + ".om"], x, om, 1, 1, act=0, sigmoid_from=18)
        return om

    def _maxpool(self, plan, name, x, out):
        self._op(plan, name, "maxpool", lambda st: _hip.check(self.L.m3d_maxpool2x2(
            x.ptr, x.cs, out.ptr, out.cs, x.n, x.h, x.w, x.c, st)), nbytes=x.n * x.h * x.w * x.c * 5)

    def _upsample_add(self, plan, name, x, upw, skip, out):
        """out = the depthwise 4x4 stride-2 transposed conv (weights upw) of x + skip."""
        self._op(plan, name, "upsample", lambda st: _hip.check(self.L.m3d_upsample2x_add(
            x.ptr, x.cs, upw.data_ptr(), skip.ptr, skip.cs, out.ptr, out.cs, x.n, x.h, x.w, x.c, st)),
            flops=2.0 * x.n * 4 * x.h * x.w * x.c * 4, nbytes=x.n * x.h * x.w * x.c * 4 * (1 + 4 + 4))

    def _tree_entry(self, plan, p, x, co, bottom, res):
        """Max-pool (-> bottom, or nowhere if None) + project (-> res) + the stride-2 tree1.conv1 of leaf Tree p as one launch:
        returns conv1's output map, or None where the engine has no such launch (this one has none)."""
        return None

    # ---- the backbone walk, shared by the fp32 and the bf16 plan and by DLA-34 and DLA-102
    def _dla_levels(self, plan, l1):
        """level2 .. level5 (pose_dla_dcn.py:162-200,261-327): four Trees of BasicBlocks (DLA-34: depths 1, 2, 2, 1) or Bottlenecks
        (DLA-102: 1, 3, 4, 1, residual roots); returns (level3, level4, level5).  The walk follows Tree.forward for any depth: a
        Tree of depth > 1 hands its `children` (the downsampled input when it is a level root, then the output of every tree1 on the
        way down) to its tree2, and the leaf at the end of the tree2 chain concatenates (x2, x1, *children) for its root.  That
        concatenation is one buffer, allocated by the outermost Tree of the chain; every child is written straight into its slice
        of it, so DLA-34's level3 root reads [x2 | x1 | bottom | X1] and its level5 root [x2 | x1 | bottom]."""
        P, B = self.P, l1.n
        chs = BACKBONE_CHANNELS[self.back_bone]
        depths, block_convs, root_residual = BACKBONE_TREES[self.back_bone]

        def conv(name, x, out, stride, pad, act=1, res=None):        # (a layer's name in the plan is its key in P)
            self._layer(plan, name, P[name], x, out, stride, pad, act=act, res=res)

        def basic(p, x, res, out, stride):
            """3x3 (stride) -> 3x3 + residual, each with BN + LeakyReLU."""
            t = self._act(plan, B, out.h, out.w, P[p + ".conv1"].cout)
            conv(p + ".conv1", x, t, stride, 1)
            conv(p + ".conv2", t, out, 1, 1, res=res)

        def bottleneck(p, x, res, out, stride):
            """1x1 (at the input resolution) -> 3x3 (stride) -> 1x1 + residual, each with BN + LeakyReLU."""
            cb = P[p + ".conv1"].cout
            t1 = self._act(plan, B, x.h, x.w, cb)
            conv(p + ".conv1", x, t1, 1, 0)
            t2 = self._act(plan, B, out.h, out.w, cb)
            conv(p + ".conv2", t1, t2, stride, 1)
            conv(p + ".conv3", t2, out, 1, 0, res=res)

        block = basic if block_convs == 2 else bottleneck

        def tree(p, levels, x, co, stride, out, level_root=False, root_dim=0, cat=None, pos=None, bottom=None, pool=None):
            """Tree.forward writing its result into `out`.  cat / pos: the root concatenation this Tree ends in and the list
            holding its next free channel (None: this Tree starts a chain and allocates it).  pool / bottom: the name of the
            max-pool of a stride-2 Tree and the slice it goes to when a root reads it, both decided by the outermost Tree of a
            tree1 chain (every tree1 pools the same input as its parent); the leaf of the chain launches it."""
            ci = x.c
            root_dim = (root_dim or 2 * co) + (ci if level_root else 0)
            h, w = x.h // stride, x.w // stride
            if cat is None:
                # width of the leaf root at the end of the tree2 chain: each level down adds one child of width co
                cat = self._act(plan, B, h, w, root_dim + co * (levels - 1))
                pos = [2 * co]
            if stride > 1 and pool is None:
                pool = p + ".downsample"
                if level_root:                                       # children.append(bottom): pooled into its slice
                    bottom = cat.slice(pos[0], ci)
                    pos[0] += ci
            if levels > 1:
                # (the project of a Tree of depth > 1 is computed by the reference and then ignored: its tree1 computes its own)
                x1 = cat.slice(pos[0], co)                            # children.append(x1) after tree1
                pos[0] += co
                tree(p + ".tree1", levels - 1, x, co, stride, x1, bottom=bottom, pool=pool)
                tree(p + ".tree2", levels - 1, x1, co, 1, out, root_dim=root_dim + co, cat=cat, pos=pos)
                return
            assert cat.c == root_dim, (p, cat.c, root_dim)
            x2v, x1v = cat.slice(0, co), cat.slice(co, co)
            project = P.get(p + ".project")
            res = self._act(plan, B, h, w, co) if project is not None else None
            t = None
            if stride > 1 and project is not None and block is basic:
                t = self._tree_entry(plan, p, x, co, bottom, res)
            if t is not None:
                conv(p + ".tree1.conv2", t, x1v, 1, 1, res=res)
            else:
                if stride == 1:
                    bottom = x
                else:
                    if bottom is None:
                        bottom = self._act(plan, B, h, w, ci)
                    self._maxpool(plan, pool, x, bottom)
                if project is not None:
                    conv(p + ".project", bottom, res, 1, 0, act=0)
                else:
                    res = bottom
                block(p + ".tree1", x, res, x1v, stride)
            block(p + ".tree2", x1v, x1v, x2v, 1)
            # Root: LeakyReLU(BN(conv(cat)) [+ children[0] = x2])
            conv(p + ".root", cat, out, 1, 0, res=x2v if root_residual else None)

        outs = [l1]
        for lv, levels in zip((2, 3, 4, 5), depths):
            x = outs[-1]
            out = self._act(plan, B, x.h // 2, x.w // 2, chs[lv], name="level%d" % lv)
            tree("base.base.level%d" % lv, levels, x, chs[lv], 2, out, level_root=lv > 2)
            outs.append(out)
        return outs[2:]

    def _dla_up(self, plan, l3, l4, l5):
        """DLAUp / IDAUp (pose_dla_dcn.py:546-578,687-696): every step is DCN -> up-sample + add -> DCN; returns feats0."""
        P, B = self.P, l3.n

        def deform(p, x, out):
            om = self._offmask(plan, p, x)
            self._layer(plan, p + ".dcn", P[p + ".dcn"], x, out, 1, 1, act=1, om=om)
            plan.named[p + ".out"] = out

        def ida_step(p, i, x, skip, co):
            proj = self._act(plan, B, x.h, x.w, co)
            deform("%s.proj_%d" % (p, i), x, proj)
            summed = self._act(plan, B, 2 * x.h, 2 * x.w, co)
            self._upsample_add(plan, "%s.up_%d" % (p, i), proj, P["%s.up_%d" % (p, i)], skip, summed)
            node = self._act(plan, B, 2 * x.h, 2 * x.w, co)
            deform("%s.node_%d" % (p, i), summed, node)
            return node

        c3, c4 = BACKBONE_CHANNELS[self.back_bone][3:5]                # DLA-34: 128 / 256, DLA-102: 256 / 512
        L5a = ida_step("base.dla_up.ida_0", 1, l5, l4, c4)             # c4 @ H/16
        L4b = ida_step("base.dla_up.ida_1", 1, l4, l3, c3)             # c3 @ H/8
        L5b = ida_step("base.dla_up.ida_1", 2, L5a, L4b, c3)           # c3 @ H/8
        feats0 = plan.named["feats0"] = ida_step("base.ida_up", 1, L5a, L5b, c3)     # c3 @ H/8
        plan.feat = (feats0.h, feats0.w)
        return feats0

    def _rpn_ops(self, plan, feats0):
        """Everything behind feats0 (M3d_inference_align.py:241-313): heads, align stages, ANAB, outputs, the detection-only tail."""
        L, P = self.L, self.P
        B, c3 = feats0.n, feats0.c
        r = self._rpn_stage(plan, B, feats0.h, feats0.w)
        fh, fw, HW, A, NC = r.fh, r.fw, r.HW, r.A, r.NC
        with_shape, with_center, with_anab = self.flags
        # detection-only tail: bbox_x3d / bbox_y3d feed feats_align3d, which ANAB pools over the whole map: dense in every launch
        dense_heads = {"bbox_x3d", "bbox_y3d"} if with_center else set()
        # box planes 6..10 (z3d, w3d, h3d, l3d, rY3d) feed columns 8..12 of a decoded row, which nobody reads before the row has
        # survived the NMS and the post-NMS cut ("After the NMS"): the heads of the split tail's second part
        deferred_heads = set(self.box_heads[6:])

        def head_desc(p, x, planar, first):
            t, img_stride, ch_off = planar
            d = MlpDesc()
            d.inp, d.in_cs, d.M, d.Cin = x.ptr, x.cs, B * HW, x.c
            if first is not None:
                d.w1, d.s1, d.t1 = P[p + ".0.frag"].data_ptr(), first.scale.data_ptr(), first.shift.data_ptr()
            mid, last = P[p + ".3"], P[p + ".6"]
            d.w2, d.s2, d.t2 = P[p + ".3.frag"].data_ptr(), mid.scale.data_ptr(), mid.shift.data_ptr()
            d.w3, d.s3, d.t3 = P[p + ".6.frag"].data_ptr(), last.scale.data_ptr(), last.shift.data_ptr()
            d.Cout, d.Cout_pad = last.cout, last.cout_pad
            d.out, d.out_img_stride, d.HW = t.data_ptr() + 4 * ch_off * HW, img_stride, HW
            flops = 2.0 * B * HW * ((x.c * 256 if first is not None else 0) + 256 * 256 + 256 * last.cout)
            return d, flops

        def mlp_array(items):
            """(descriptor array, flops, op name) of the heads items = [(p, x, planar)] as one fused-MLP launch."""
            arr = (MlpDesc * len(items))()
            flops = 0.0
            for i, (p, x, planar) in enumerate(items):
                arr[i], f = head_desc(p, x, planar, P[p + ".0"])
                flops += f
            return arr, flops, "+".join(p for p, _, _ in items) + ".mlp"

        def rows_form(items, arr, rows_of):
            """The row-list launch of `arr` on the list rows_of(stage record) = (rows, n_rows); the dense heads stay dense."""
            n = len(items)
            mask = sum(1 << i for i, (p, _, _) in enumerate(items) if p not in dense_heads)

            def factory(r):
                rows, n_rows = rows_of(r)
                return lambda st: _hip.check(L.m3d_head_mlp_forward_rows(arr, n, rows.data_ptr(), n_rows.data_ptr(), mask, st))
            return factory

        def heads(items):
            """1x1 heads with no mutual dependency as ONE fused-MLP launch (grid.y = head): items = [(p, x, planar)].  The 64-wide
            launches have a row-list form for the tail: bit i of its mask = head i runs at the listed pixels only."""
            arr, flops, name = mlp_array(items)
            n = len(items)
            plan.ops.append((name, "head_mlp<3,%d>" % arr[0].Cout_pad, flops,
                             lambda st: _hip.check(L.m3d_head_mlp_forward_batched(arr, n, st)), arr))
            if arr[0].Cout_pad == 64:
                plan.sparse_form(rows_form(items, arr, lambda r: (r.rows, r.n_rows)))
                late = [it for it in items if it[0] in deferred_heads]
                if late:
                    # the split tail: the heads in front of the NMS on the needed pixels, the deferred ones on the survivors' pixels
                    early = [it for it in items if it[0] not in deferred_heads]
                    forms = []
                    for part, rows_of in ((early, lambda r: (r.rows, r.n_rows)), (late, lambda r: (r.post_rows, r.post_n_rows))):
                        if part:
                            parr, pflops, pname = mlp_array(part)
                            forms.append((rows_form(part, parr, rows_of), pname, pflops, parr))
                        else:
                            forms.append(None)
                    plan.deferred_form(forms[0], forms[1], [x.t for _, x, _ in late])

        def head(p, x, planar, k0=1):
            """3-layer head.  A 1x1 head runs as one fused-MLP launch; the cls head runs its 3x3 conv through the
            Winograd kernel and the remaining two 1x1 layers fused."""
            if k0 == 1:
                return heads([(p, x, planar)])
            h1 = self._buf(plan, B, fh, fw, 256)
            self._conv(plan, p + ".0", P[p + ".0"], x, h1, 1, k0 // 2, act=1)
            d, flops = head_desc(p, h1, planar, None)
            ref = ctypes.byref(d)
            plan.ops.append((p + ".mlp", "head_mlp<2,%d>" % d.Cout_pad, flops,
                             lambda st: _hip.check(L.m3d_head_mlp_forward(ref, st)), d))

        head("cls", feats0, (r.cls_pl, NC * A * HW, 0), 3)
        self._rpn_select(plan, r)

        # the stages the configuration has (M3d_inference_align.py:241-277): without shape_align the heads read feats0, without
        # center_align the size heads read `feats`, without ANAB the z3d head reads feats_align3d; an absent stage's map is
        # published under its reference name as an alias of the map that stands in for it
        if with_shape:
            om_sa = self._buf(plan, B, fh, fw, 27, 28)
            self._rpn_shape_offsets(plan, r, om_sa, cost=True)
            feats = self._buf(plan, B, fh, fw, c3, name="feats")
            self._conv(plan, "shape_align.dcn", P["shape_align"], feats0, feats, 1, 1, act=0, res=feats0, om=om_sa)
        else:
            feats = plan.named["feats"] = feats0

        def center_align(p, x, kx, ky, mi, out):
            om = self._buf(plan, B, fh, fw, 3, 4)
            self._rpn_center_offsets(plan, r, p, om, kx, ky, mi, cost=True)
            self._conv(plan, p + ".dcn", P[p], x, out, 1, 0, act=0, res=x, om=om)

        # heads are grouped by the feature map they read (M3d_inference_align.py:139-176): the four centre heads first,
        # then both centre alignments, then the six size / orientation heads (+ z3d without ANAB).  Without the centre
        # alignments every box head but an ANAB-fed z3d reads `feats`: one launch.
        z3d_now = [] if with_anab else ["bbox_z3d"]
        if with_center:
            heads([("bbox_x", feats, r.box_planar(0)), ("bbox_y", feats, r.box_planar(1)),
                   ("bbox_x3d", feats, r.box_planar(4)), ("bbox_y3d", feats, r.box_planar(5))])
            f2d = self._buf(plan, B, fh, fw, c3, name="feats_align2d")
            center_align("center_align2d", feats, 0, 1, 0, f2d)
            f3d = self._buf(plan, B, fh, fw, c3, name="feats_align3d")
            center_align("center_align3d", feats, 4, 5, 4, f3d)
            heads([("bbox_w", f2d, r.box_planar(2)), ("bbox_h", f2d, r.box_planar(3))] +
                  [(h, f3d, r.box_planar(self.box_heads.index(h))) for h in z3d_now + ["bbox_w3d", "bbox_h3d", "bbox_l3d", "bbox_rY3d"]])
        else:
            f2d = f3d = plan.named["feats_align2d"] = plan.named["feats_align3d"] = feats
            heads([(h, feats, r.box_planar(k)) for k, h in enumerate(self.box_heads) if h != "bbox_z3d" or not with_anab])

        # ---- ANAB ---------------------------------------------------------------------
        if with_anab:
            # zeroed: the tail's row-list attention writes it at the listed pixels only, and it is published in plan.named
            gl = self._buf(plan, B, fh, fw, c3, name="feats_gl", zero=True)
            self._anab_ops(plan, f3d, gl, P["anab.bn.scale"], P["anab.bn.shift"], act=1, res_mode=1)
            head("bbox_z3d", gl, r.box_planar(6))
        else:
            plan.named["feats_gl"] = f3d

        self._rpn_outputs(plan, r)
        self._rpn_tail(plan, r)

    # ------------------------------------------------------------------ RPN-stage steps shared by the fp32 and the bf16 plan
    # (what they launch reads and writes fp32 / integer data in both: the planar staging, the selection, the align offsets)
    def _rpn_stage(self, plan, B, fh, fw):
        """The stage's record with the planar fp32 staging of the head outputs: cls [B][NC][A][HW], box [B][11][A][HW]."""
        r = _RpnStage(B, self.A, self.NC, fh, fw)
        r.cls_pl = torch.empty(B * r.NC * r.R, device=self.device, dtype=torch.float32)
        r.box_pl = torch.empty(B * 11 * r.R, device=self.device, dtype=torch.float32)
        plan.keep += [r.cls_pl, r.box_pl]
        plan.named["cls_planar"], plan.named["box_planar"] = r.cls_pl, r.box_pl
        # every op from here on may write the planar staging: a detection stage that reads it for the PREVIOUS batch
        # (m3dssd_amd.pipeline.PipelinedDetector, planar form) has to be done before op `planar_first_op` of this one starts
        plan.named["planar_first_op"] = len(plan.ops)
        r.means = np.asarray(self.conf.bbox_means, dtype=np.float32).reshape(-1)
        r.stds = np.asarray(self.conf.bbox_stds, dtype=np.float32).reshape(-1)
        return r

    def _rpn_select(self, plan, r):
        """anchor_select behind the class head: per pixel the best anchor and its foreground probability."""
        L, B, A, NC, HW = self.L, r.B, r.A, r.NC, r.HW
        cls_pl = r.cls_pl
        sel_idx = r.sel_idx = torch.empty(B * HW, device=self.device, dtype=torch.int32)
        sel_prob = r.sel_prob = torch.empty(B * HW, device=self.device, dtype=torch.float32)
        plan.keep += [sel_idx, sel_prob]
        plan.named["sel_idx"], plan.named["sel_prob"] = sel_idx, sel_prob
        if NC == 4 and A >= 4 and SELECT_KEYS:
            # + the detection stage's sort keys (plan.named["score_bits"], created by _rpn_outputs) while the logits are in registers
            plan.named["keys_by_select"] = True
            plan.named["score_bits_first_write_op"] = len(plan.ops)     # a detect(k-1) beside forward(k) must be done before it
            self._op(plan, "anchor_select", "select", lambda st: _hip.check(L.m3d_anchor_select_keys(
                cls_pl.data_ptr(), B, A, HW, sel_idx.data_ptr(), sel_prob.data_ptr(), plan.named["score_bits"].data_ptr(), st)),
                nbytes=B * HW * (A * NC + 2 + A) * 4)
        else:
            self._op(plan, "anchor_select", "select", lambda st: _hip.check(L.m3d_anchor_select(
                cls_pl.data_ptr(), B, A, NC, HW, sel_idx.data_ptr(), sel_prob.data_ptr(), None, st)),
                nbytes=B * HW * (A * NC + 2) * 4)

    def _rpn_shape_offsets(self, plan, r, om, cost):
        """shape_align's DCN offsets (27 per pixel into `om`) from the selected anchor's shape; the DCN itself is the caller's.
        cost: state the launch's HBM bytes (the fp32 plan does, the bf16 plan never did)."""
        L, P, B, A, HW = self.L, self.P, r.B, r.A, r.HW
        self._op(plan, "shape_align.offsets", "align", lambda st: _hip.check(L.m3d_align_offsets(
            0, r.sel_idx.data_ptr(), r.sel_prob.data_ptr(), 0.5, P["shape.table"].data_ptr(), None, None, None, 0.0, 1.0, 0.0,
            1.0, om.ptr, om.cs, B, A, HW, 9, 0, st)), nbytes=B * HW * (2 + 28) * 4 if cost else None)

    def _rpn_center_offsets(self, plan, r, p, om, kx, ky, mi, cost):
        """The DCN offsets of centre alignment p (3 per pixel into `om`) from box rows kx, ky of the staging, de-normalised with
        means / stds [mi], [mi + 1]; the DCN itself is the caller's.  center_align2d has a gated form for the tail: the 1x1
        alignment is a per-pixel function, so behind sparse bbox_x / bbox_y it reads them at the needed pixels only."""
        L, P, B, A, HW = self.L, self.P, r.B, r.A, r.HW
        ms = (float(r.means[mi]), float(r.stds[mi]), float(r.means[mi + 1]), float(r.stds[mi + 1]))
        self._op(plan, p + ".offsets", "align", lambda st: _hip.check(L.m3d_align_offsets(
            1, r.sel_idx.data_ptr(), r.sel_prob.data_ptr(), 0.5, None, r.box_ptr(kx), r.box_ptr(ky), P["anchor_wh"].data_ptr(),
            *ms, om.ptr, om.cs, B, A, HW, 1, 11 * A * HW, st)), nbytes=B * HW * (2 + 2 + 4) * 4 if cost else None)
        if p == "center_align2d":
            plan.sparse_form(lambda r: lambda st: _hip.check(L.m3d_align_offsets_gated(
                r.sel_idx.data_ptr(), r.sel_prob.data_ptr(), 0.5, r.box_ptr(kx), r.box_ptr(ky), P["anchor_wh"].data_ptr(), *ms,
                r.need.data_ptr(), om.ptr, om.cs, B, A, HW, 11 * A * HW, st)))

    def _rpn_outputs(self, plan, r):
        """The bundled outputs [B, R, .] and the op that writes them from the planar staging."""
        L, B, A, NC, HW, R = self.L, r.B, r.A, r.NC, r.HW, r.R
        cls_pl, box_pl = r.cls_pl, r.box_pl
        cls = torch.empty(B, R, NC, device=self.device, dtype=torch.float32)
        prob = torch.empty(B, R, NC, device=self.device, dtype=torch.float32)
        b2 = torch.empty(B, R, 4, device=self.device, dtype=torch.float32)
        b3 = torch.empty(B, R, 7, device=self.device, dtype=torch.float32)
        key = r.key = torch.empty(B, R, device=self.device, dtype=torch.int32)   # monotone score bits (u32)
        plan.named.update(cls=cls, prob=prob, bbox_2d=b2, bbox_3d=b3, score_bits=key)
        assert NC == 4, "bundle kernel is written for 4 classes (bg + 3)"
        # destination of the four bundled outputs: the plan's own buffers, or -- for one forward -- fresh tensors handed in by
        # Engine.forward(fresh=True) (RPN.forward returns fresh tensors like the reference: written in place, no copies)
        dst = plan.named["out_dst"] = [cls, prob, b2, b3]
        self._op(plan, "bundle_outputs", "bundle", lambda st: _hip.check(L.m3d_bundle_outputs(
            cls_pl.data_ptr(), box_pl.data_ptr(), dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(), dst[3].data_ptr(),
            key.data_ptr(), B, A, HW, st)), nbytes=B * R * (NC + 11 + 2 * NC + 4 + 7 + 1) * 4)

    def _rpn_tail(self, plan, r):
        """The detection-only tail (plan.tail) of a plan whose anchor_select writes the keys.
        m3d_topk_decode_planar reads the box staging at the nms_topN_pre best rows of an image and nowhere else, the score is a
        function of the class head alone (anchor_select has written the keys), and row a * HW + pix belongs to pixel pix: a box
        head whose planar output feeds nothing but the decode is needed at the pixels that hold one of those rows.  The centre
        alignments are 1x1 (feats_align2d[p] depends on bbox_x[p], bbox_y[p] and the dense `feats`), so with them bbox_x / bbox_y
        stay sparse behind gated offsets; bbox_x3d / bbox_y3d feed feats_align3d, which ANAB pools over the whole map: dense.
        feats_gl feeds bbox_z3d and nothing else, and that head runs at the listed pixels: so does the attention behind the dense
        projection and pooling (its queries, softmax, P.V and epilogue are per-pixel functions).
        What the selection reads and writes is fp32 / integer in the bf16 plan too, so m3d_need_rows and m3d_align_offsets_gated
        serve both.  An op has a sparse form where the code that appended it registered one (plan.sparse); every other op of
        ops[tail_start:-1] is taken as it is.  A registration in front of anchor_select (ANAB + z3d of the bf16 ANAB-only
        configuration, which run beside the class head) is not looked at: those ops run before the selection exists and stay dense.
        Issued on one stream (run_plan(tail=True)): a side branch of the plan is time-neutral here."""
        if not plan.named.get("keys_by_select"):
            return
        L, B, A, HW, R = self.L, r.B, r.A, r.HW, r.R
        t0 = plan.named["score_bits_first_write_op"] + 1
        # zeroed: the dense forward (plan.ops) never writes them, and the list is written up to n_rows only -- they are
        # published in plan.named and must not show what the allocation held (uninitialised memory)
        need = r.need = torch.zeros(B * HW, device=self.device, dtype=torch.uint8)
        rows = r.rows = torch.zeros(B * HW, device=self.device, dtype=torch.int32)
        n_rows = r.n_rows = torch.zeros(1, device=self.device, dtype=torch.int32)
        thresh = torch.zeros(B, device=self.device, dtype=torch.int32)
        nb = L.m3d_need_rows_workspace_bytes(B, HW)
        ws = torch.empty(nb, device=self.device, dtype=torch.uint8)
        plan.keep += [need, rows, n_rows, thresh, ws]
        plan.named.update(need=need, need_rows=rows, n_rows=n_rows, need_thresh=thresh)
        k_pre = plan.named["sparse_k"] = [min(int(self.conf.nms_topN_pre), R)]      # set by the caller at launch time
        key = r.key
        tail = [("need_rows", "select", 0.0, lambda st: _hip.check(L.m3d_need_rows(
            key.data_ptr(), B, A, HW, int(k_pre[0]), thresh.data_ptr(), need.data_ptr(), rows.data_ptr(), n_rows.data_ptr(),
            ws.data_ptr(), nb, st)), OpCost(B * R * 4 * 4))]
        for i in range(t0, len(plan.ops) - 1):
            op, sparse = plan.ops[i], plan.sparse.get(i)
            tail.append(op if sparse is None else op[:3] + (sparse(r), op[4]))
        plan.tail, plan.tail_start = tail, t0
        self._rpn_post3d(plan, r, t0)

    # entries of the sort inside m3d_post_rows (B * nms_topN_post)
    POST_ROWS_MAX = 4096

    def _rpn_post3d(self, plan, r, t0):
        """The tail in two parts (plan.tail_pre, plan.post3d) where the plan's builders registered deferred forms.
        Columns 8..12 of a decoded row come from box planes 6..10, and m3d_nms_sorted_dev and the post-NMS cut read columns 0..4:
        the launches that feed those planes and nothing else are needed at the pixels of the at most nms_topN_post rows per image
        that m3d_select_post copies.  A detector that runs detect(k-1) beside forward(k) issues post3d on that side branch, so
        every map a post3d launch reads must still hold batch k-1 there: its first writer has to stand at or behind
        `planar_first_op`, where the branch has joined.  That is decided from the buffers (plan.first_write); a map whose writer
        was never recorded counts as written in front.  Declined (both lists stay None): nothing registered, a builder ruled it
        out (the attention is not the one-launch row-list route), a map fails the rule, or B * nms_topN_post exceeds the sort."""
        forms = {i: f for i, f in plan.deferred.items() if i >= t0}
        if not forms or plan.post3d_declined is not None:
            return
        if r.B * int(self.conf.nms_topN_post) > self.POST_ROWS_MAX:
            return
        join = int(plan.named["planar_first_op"])
        reads = {}
        for _, _, rd in forms.values():
            for t in rd:
                reads[t.data_ptr()] = (t, plan.first_write.get(t.data_ptr(), -1))
        if any(w < join for _, w in reads.values()):
            return
        # the survivors' pixels: zeroed for the same reason as the needed-pixel list above
        r.post_rows = torch.zeros(r.B * r.HW, device=self.device, dtype=torch.int32)
        r.post_n_rows = torch.zeros(1, device=self.device, dtype=torch.int32)
        plan.keep += [r.post_rows, r.post_n_rows]
        plan.post_rows, plan.post_n_rows = r.post_rows, r.post_n_rows      # (not in plan.named: its keys are pinned by the manifest)

        def form(op, f):
            factory, name, flops, desc = f
            return (op[0] if name is None else name, op[1], op[2] if flops is None else flops, factory(r),
                    op[4] if desc is None else desc)

        pre = [plan.tail[0]]
        for i in range(t0, len(plan.ops) - 1):
            if i not in forms:
                pre.append(plan.tail[1 + i - t0])
            elif forms[i][0] is not None:
                pre.append(form(plan.ops[i], forms[i][0]))
        plan.tail_pre = pre
        plan.post3d = [form(plan.ops[i], forms[i][1]) for i in sorted(forms)]
        plan.post3d_reads = list(reads.values())

    def _anab_ops(self, plan, x, out, scale, shift, act, res_mode):
        """Append the ANAB launches: fused QKVS 1x1 conv -> weighted pyramid pooling -> logits GEMM (per-image
        pooled keys as weights) -> row softmax -> P.V GEMM with the residual (+ optional BN/LeakyReLU) epilogue."""
        L, P = self.L, self.P
        B, fh, fw = x.n, x.h, x.w
        HW = fh * fw
        ctot, off = self.anab_ctot, self.anab_off
        qkvs = self._buf(plan, B, fh, fw, ctot, _rup(ctot, 32))          # 128-byte pixel rows: the wave kernel's gather map
        self._conv(plan, "anab.qkvs", P["anab.qkvs"], x, qkvs, 1, 0, act=0, sigmoid_from=off["s"], affine=False)
        n_bins = sum(s * s for s in PSP_SIZES)
        # the two per-image GEMMs go to the wave-granular kernel when they yield enough waves; their weights (pooled keys /
        # values) are then written in MFMA-fragment order by the pooling finish and the key count is padded to 128
        fused = FUSED_ANAB and ((self.cv == 128 and self.ck in (64, 128, 168)) or (self.cv == 256 and self.ck == 168)) \
            and HW % 128 == 0
        wave_ok = (not fused) and USE_ANAB_WAVE and USE_CONV_WAVE and HW % 32 == 0 and self.ck_pad % 32 == 0 and self.cv % 128 == 0
        nw = B * HW // 32
        wave_logits = wave_ok and nw * (_rup(n_bins, 128) // 128) >= 900
        keys_pad = _rup(n_bins, 128) if wave_logits else _rup(n_bins, 32)
        wave_pv = wave_ok and keys_pad % 32 == 0 and nw * (self.cv // 128) >= 900
        frag = (1 if wave_logits else 0) | (2 if wave_pv else 0)
        ckv = self.ck + self.cv
        khat = torch.zeros(B * keys_pad * self.ck_pad, device=self.device, dtype=torch.float32)
        vhatT = torch.zeros(B * self.cv * keys_pad, device=self.device, dtype=torch.float32)
        plan.keep += [khat, vhatT]
        plan.named["anab.khat"], plan.named["anab.vhatT"] = khat, vhatT
        kvv, sv = qkvs.slice(off["k"], ckv), qkvs.slice(off["s"], self.ns)
        self._anab_pool(plan, kvv.ptr, kvv.cs, sv.ptr, sv.cs, B, fh, fw, khat, vhatT, keys_pad, frag, nested=USE_ANAB_NESTED,
                        nested_nbytes=B * HW * (ckv + self.ns) * 4)
        qv = qkvs.slice(off["q"], self.ck_pad)
        if fused:
            # logits + softmax + P.V in one launch: the fp32 logits (7680 x 352 per image) never reach HBM
            rp, rcs = (x.ptr, x.cs) if x is not None else (None, 0)
            sp = scale.data_ptr() if scale is not None else None
            hp = shift.data_ptr() if shift is not None else None

            def attend(fn, *row_list):      # the launch through the dense entry point, or through the row-list one with its list
                return lambda st: _hip.check(fn(
                    qv.ptr, qv.cs, khat.data_ptr(), self.ck_pad, vhatT.data_ptr(), B, HW, self.ck, n_bins, keys_pad, self.cv, rp,
                    rcs, res_mode, sp, hp, 1 if act else 0, out.ptr, out.cs, *row_list, st))

            self._op(plan, "anab.attend", "anab_attend", attend(L.m3d_anab_attend_f32),
                     flops=2.0 * B * HW * n_bins * (self.ck + self.cv),
                nbytes=B * HW * (self.ck + 3 * self.cv) * 4 + B * keys_pad * (self.ck + self.cv) * 4)
            plan.wrote(out.t)
            if ANAB_ROWS:
                plan.sparse_form(lambda r: attend(L.m3d_anab_attend_f32_rows, r.rows.data_ptr(), r.n_rows.data_ptr()))
                # split tail: `out` feeds bbox_z3d and nothing else, so the attention waits for the survivors' pixels
                plan.deferred_form(None, (lambda r: attend(L.m3d_anab_attend_f32_rows, r.post_rows.data_ptr(),
                                                           r.post_n_rows.data_ptr()), None, None, None),
                                   [qkvs.t, khat, vhatT] + ([x.t] if x is not None else []))
            else:
                plan.post3d_declined = "the attention runs dense in the tail"
            return
        plan.post3d_declined = "the attention is not the one-launch route"

        def image(v, i):
            return View(v.t, 1, v.h, v.w, v.c, v.cs, v.ptr + 4 * i * v.h * v.w * v.cs)

        def image_gemm(name, inp, outv, wgt, stride, frag, res=None, **kw):
            """1x1 convolution whose weights differ per image (`stride` floats apart in wgt).  The wave kernel and the igemm take
            them in one launch, the igemm picking a tile's weights by the image of the tile's first row: no tile may straddle two
            images, which holds for H*W % 64 == 0.  Any other map gets one igemm launch per image, with that image's weights as
            shared weights, as ONE plan op."""
            if frag or HW % 64 == 0:
                self._conv(plan, name, None, inp, outv, 1, 0, res=res, wgt_ptr=wgt.data_ptr(), wgt_img_stride=stride, kh=1, kw=1,
                           wgt_frag=frag, **kw)
                return
            sub = _Plan()
            for i in range(B):
                self._conv(sub, name, None, image(inp, i), image(outv, i), 1, 0, res=None if res is None else image(res, i),
                           wgt_ptr=wgt.data_ptr() + 4 * i * stride, kh=1, kw=1, per_image=True, **kw)
            assert len(sub.ops) == B and len({op[1] for op in sub.ops}) == 1, [op[:2] for op in sub.ops]
            plan.keep += sub.keep
            fns = [op[3] for op in sub.ops]
            plan.ops.append((name, sub.ops[0][1], sum(op[2] for op in sub.ops), lambda st: [fn(st) for fn in fns], sub.ops[0][4]))

        logits = self._buf(plan, B, fh, fw, keys_pad)
        image_gemm("anab.logits", qv, logits, khat, keys_pad * self.ck_pad, wave_logits, act=0, affine=False, cout=n_bins,
                   cout_pad=keys_pad, cin_true=self.ck)
        self._op(plan, "anab.softmax", "softmax", lambda st: _hip.check(L.m3d_softmax_rows(
            logits.ptr, B * HW, n_bins, keys_pad, st)), nbytes=B * HW * n_bins * 8)
        image_gemm("anab.pv", logits, out, vhatT, self.cv * keys_pad, wave_pv, res=x, act=act, res_mode=res_mode, cout=self.cv,
                   cout_pad=_rup(self.cv, 32), scale=scale, shift=shift, cin_true=n_bins)

    def _anab_pool(self, plan, kv_ptr, kv_cs, s_ptr, s_cs, B, fh, fw, khat, vhatT, keys_pad, frag, nested=True, nested_nbytes=None):
        """The gated pyramid pooling of ANAB in both plans: fp32 K|V (kv_ptr, pixel stride kv_cs) weighted by the gates (s_ptr, s_cs)
        -> the pooled keys khat [B][keys_pad][ck_pad] and values vhatT [B][cv][keys_pad]; frag: bit 0 / bit 1 = khat / vhatT in
        MFMA-fragment order.  One pass where the windows of the four scales nest and `nested` allows it (nested_nbytes: the cost slot
        of that op), else partial sums per work item and a finish launch."""
        L, ck, cv = self.L, self.ck, self.cv
        if nested and fh % 16 == 0 and fw % 16 == 0 and PSP_SIZES == (1, 4, 8, 16):
            # the windows of the four scales nest: one pass over the features (csrc/rpn_kernels.hip)
            scratch = torch.empty(L.m3d_anab_pool_nested_scratch_bytes(B, ck + cv) // 4, device=self.device, dtype=torch.float32)
            plan.keep.append(scratch)
            self._op(plan, "anab.pool_nested", "anab_pool", lambda st: _hip.check(L.m3d_anab_pool_nested(
                kv_ptr, kv_cs, s_ptr, s_cs, B, fh, fw, ck, cv, scratch.data_ptr(), khat.data_ptr(), keys_pad, self.ck_pad,
                vhatT.data_ptr(), frag, st)), nbytes=nested_nbytes)
            plan.wrote(khat, vhatT)
            return
        items, bin_scale, bin_slots, bin_inv = self._anab_items(fh, fw)
        n_bins, max_slots = len(bin_scale), int(bin_slots.max())
        d_items, d_bscale = torch.from_numpy(items).to(self.device), torch.from_numpy(bin_scale).to(self.device)
        d_bslots, d_binv = torch.from_numpy(bin_slots).to(self.device), torch.from_numpy(bin_inv).to(self.device)
        partial = torch.empty(B * n_bins * max_slots * (ck + cv), device=self.device, dtype=torch.float32)
        plan.keep += [d_items, d_bscale, d_bslots, d_binv, partial]
        self._op(plan, "anab.pool_partial", "anab_pool", lambda st: _hip.check(L.m3d_anab_pool_partial(
            kv_ptr, kv_cs, s_ptr, s_cs, d_items.data_ptr(), items.shape[0], d_bscale.data_ptr(), n_bins, partial.data_ptr(),
            max_slots, B, fh, fw, ck + cv, st)))
        self._op(plan, "anab.pool_finish", "anab_pool", lambda st: _hip.check(L.m3d_anab_pool_finish(
            partial.data_ptr(), d_bslots.data_ptr(), d_binv.data_ptr(), n_bins, max_slots, ck, cv, khat.data_ptr(), keys_pad,
            self.ck_pad, vhatT.data_ptr(), B, frag, st)))
        plan.wrote(khat, vhatT)

    @classmethod
    def anab_standalone(cls, mod, x):
        """ANAB.forward for a stand-alone module: x is an NHWC View; returns the output View."""
        eng = cls.__new__(cls)
        eng.L, eng.device, eng.profile, eng.P = _hip.lib(), x.t.device, None, {}
        eng._pack_anab(eng.P, mod.query_conv.weight, mod.key_conv.weight, mod.value_conv.weight,
                       mod.spatial_conv.weight)
        plan = _Plan()
        out = eng._buf(plan, x.n, x.h, x.w, x.c)
        eng._anab_ops(plan, x, out, None, None, act=0, res_mode=0)
        eng.run_plan(plan)
        out.keep = plan          # keep the intermediate buffers alive until the caller has copied out
        return out

    @staticmethod
    def _anab_items(H, W):
        """Work items of the pyramid pooling: AdaptiveAvgPool2d windows (start = floor(i*H/s),
        end = ceil((i+1)*H/s)) split into chunks of ceil(H/16) rows x ceil(W/4) columns, so that the
        whole-map "size 1" bin is spread over 64 workgroups instead of serialising on one."""
        rchunk, cchunk = max(1, math.ceil(H / 16)), max(1, math.ceil(W / 4))
        items, bin_scale, bin_slots, bin_inv = [], [], [], []
        b = 0
        for si, s in enumerate(PSP_SIZES):
            for i in range(s):
                h0, h1 = (i * H) // s, -((-(i + 1) * H) // s)
                for j in range(s):
                    w0, w1 = (j * W) // s, -((-(j + 1) * W) // s)
                    slot = 0
                    for r0 in range(h0, h1, rchunk):
                        for c0 in range(w0, w1, cchunk):
                            items.append((b, r0, min(r0 + rchunk, h1), c0, min(c0 + cchunk, w1), slot))
                            slot += 1
                    bin_scale.append(si)
                    bin_slots.append(slot)
                    bin_inv.append(1.0 / ((h1 - h0) * (w1 - w0)))
                    b += 1
        return (np.asarray(items, dtype=np.int32), np.asarray(bin_scale, dtype=np.int32),
                np.asarray(bin_slots, dtype=np.int32), np.asarray(bin_inv, dtype=np.float32))

    # ------------------------------------------------------------------ execution
    def plan_for(self, B, H, W):
        key = (B, H, W)
        if key not in self.plans:
            if H % 32 or W % 32:
                raise RuntimeError("input H and W must be multiples of 32 (got %dx%d)" % (H, W))
            with torch.cuda.device(self.device):
                self.plans[key] = self._build_plan(B, H, W)
        return self.plans[key]

    def _run_to(self, plan, fresh):
        """Run the plan; fresh=True: the four bundled outputs are written into newly allocated tensors (returned), the plan's own
        output buffers are left as they are; else into the plan-owned buffers (returned as views)."""
        n = plan.named
        owned = (n["cls"], n["prob"], n["bbox_2d"], n["bbox_3d"])
        if not fresh:
            self.run_plan(plan)
            return owned
        dst = n["out_dst"]
        outs = [torch.empty_like(t) for t in owned]
        dst[:] = outs
        try:
            self.run_plan(plan)
        finally:
            dst[:] = owned
        return tuple(outs)

    def forward(self, x, fresh=False):
        """x: float32 [B,3,H,W] on the engine's device -> (cls, prob, bbox_2d, bbox_3d) device tensors: views of plan-owned
        buffers, overwritten by the next call with the same shape, or (fresh=True) newly allocated tensors."""
        if not x.is_cuda:
            raise NotImplementedError("M3DSSD HIP engine: input must be a ROCm device tensor")
        if x.device != self.device:
            raise RuntimeError("M3DSSD HIP engine on %s got an input on %s" % (self.device, x.device))
        B, _, H, W = x.shape
        plan = self.plan_for(B, H, W)
        x = x.contiguous()
        plan.named["input_ptr"][0] = x.data_ptr()
        plan.named["input_u8"][0] = 0
        return self._run_to(plan, fresh)

    def forward_u8(self, frames, size=None, fresh=False):
        """frames: uint8 [B, h, w, 3] BGR device tensor (what cv2.imread returns, batched) -> the same outputs as
        forward(Preprocess(frames)): padding to `size` (default conf.crop_size), /255, -mean, /stds, BGR->RGB
        (lib/augmentations.py:472-501, lib/dataloader.py:943-950) happen inside the stem kernel's loads."""
        if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise NotImplementedError("forward_u8: uint8 [B, h, w, 3] ROCm device tensor expected")
        H, W = (int(v) for v in (size if size is not None else self.conf.crop_size))
        B, h, w, _ = frames.shape
        if frames.device != self.device:
            raise RuntimeError("M3DSSD HIP engine on %s got frames on %s" % (self.device, frames.device))
        if h > H or w > W:
            raise RuntimeError("forward_u8: frame %dx%d does not fit the padded size %dx%d" % (h, w, H, W))
        plan = self.plan_for(B, H, W)
        frames = frames.contiguous()
        plan.named["input_u8"][:] = [frames.data_ptr(), h, w]
        try:
            return self._run_to(plan, fresh)
        finally:
            plan.named["input_u8"][0] = 0

    def forward_backbone(self, x):
        """Backbone + DCN up-sampling only (DLASeg.forward): returns the NHWC View of the 128-channel (DLA-102: 256) map."""
        B, _, H, W = x.shape
        plan = self.plan_for(B, H, W)
        x = x.contiguous()
        plan.named["input_ptr"][0] = x.data_ptr()
        self.run_plan(plan)
        return plan.named["feats0"]

    def run_plan(self, plan, start=0, end=None, tail=False):
        """Issue plan.ops[start:end] on the ENGINE device's current stream (the whole forward by default); the engine's
        device is made current for the launches, whatever the caller's current device is.
        tail=True: the detection-only form -- plan.ops[start:plan.tail_start], then plan.tail in place of everything behind it up
        to bundle_outputs (`end` must be the index of bundle_outputs), all on the current stream: side branches are not forked in
        this form.  The box staging is then written at the needed pixels only:
        what follows may be the planar top-k decode, not bundle_outputs.  plan.named["sparse_k"][0] is the k of that decode.
        tail="pre": plan.tail_pre in place of plan.tail -- box planes 6..10 are then not written at all; what follows is
        m3d_topk_decode_planar_2d, the NMS, m3d_post_rows and run_post3d."""
        with torch.cuda.device(self.device):
            if not tail:
                return self._run_plan(plan, start, end)
            if getattr(plan, "tail", None) is None:
                raise RuntimeError("run_plan(tail=True): this plan has no detection-only tail")
            tail_ops = plan.tail
            if tail == "pre":
                if getattr(plan, "tail_pre", None) is None:
                    raise RuntimeError("run_plan(tail='pre'): this plan does not offer the split tail")
                tail_ops = plan.tail_pre
            # (a plan with side branches -- the bf16 one, ANAB beside the size heads -- is issued in line here, on one stream)
            if end != len(plan.ops) - 1 or not 0 <= start <= plan.tail_start:
                raise RuntimeError("run_plan(tail=True): ops [%r, %r) do not end in front of bundle_outputs (op %d) behind a start "
                                   "in [0, %d]" % (start, end, len(plan.ops) - 1, plan.tail_start))
            self._run_plan(plan, start, end, plan.ops[start:plan.tail_start] + tail_ops)

    def run_post3d(self, plan):
        """Issue plan.post3d on the engine device's current stream: the deferred heads and the attention at the pixels that
        m3d_post_rows listed (plan.post_rows / plan.post_n_rows), writing box planes 6..10 there."""
        if getattr(plan, "post3d", None) is None:
            raise RuntimeError("run_post3d: this plan does not offer the split tail")
        with torch.cuda.device(self.device):
            self._run_plan(plan, 0, 0, plan.post3d)

    def sparse_heads_default(self, plan, k):
        """The plan-time rule of a detector's sparse_heads=None for a decode of the k best rows per image."""
        if getattr(plan, "tail", None) is None:
            return False
        hw = plan.feat[0] * plan.feat[1]
        return min(int(k), hw) <= SPARSE_HEADS_MAX_FRACTION * hw

    def _run_plan(self, plan, start, end, ops=None):
        st = _Stream.current(self.device)
        tail = ops is not None
        if not tail:
            ops = plan.ops[start:end]
        if self.profile is None:
            brs = [] if tail else [br for br in getattr(plan, "branches", ()) if lo_hi_contains(start, end, len(plan.ops), br)]
            if brs:
                # side branches: ops [b0, b1) run on a second stream beside ops [b1, join) (no data dependence between the two
                # groups: the plan builder vouches for that); fork / join by stream waits, so the pattern is captured by a hipGraph
                lo, hi = start, (len(plan.ops) if end is None else end)
                main = torch.cuda.current_stream(self.device)
                if getattr(self, "_side", None) is None:
                    self._side = torch.cuda.Stream(self.device)
                side = self._side
                sst = ctypes.c_void_p(side.cuda_stream)
                forks = {br[0] for br in brs}
                joins = {br[2] for br in brs}
                on_side = set()
                for b0, b1, _ in brs:
                    on_side.update(range(b0, b1))
                for i in range(lo, hi):
                    if i in joins:
                        main.wait_stream(side)
                    if i in forks:
                        side.wait_stream(main)
                    plan.ops[i][3](sst if i in on_side else st)
                if hi in joins:
                    main.wait_stream(side)
                return
            for op in ops:
                op[3](st)
            return
        L = self.L
        evs = []
        for op in ops:
            if self.profile_kinds is not None and op[1] not in self.profile_kinds:
                op[3](st)
                continue
            e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
            _hip.check(L.m3d_event_create(ctypes.byref(e0)))
            _hip.check(L.m3d_event_create(ctypes.byref(e1)))
            _hip.check(L.m3d_event_record(e0, st))
            op[3](st)
            _hip.check(L.m3d_event_record(e1, st))
            evs.append((op, e0, e1))
        self._pending += evs

    def flush_profile(self):
        """Resolve the recorded HIP events (synchronises) into self.profile rows (name, kind, flops, ms)."""
        L = self.L
        for op, e0, e1 in self._pending:
            ms = ctypes.c_float()
            _hip.check(L.m3d_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
            self.profile.append((op[0], op[1], op[2], ms.value))
            L.m3d_event_destroy(e0)
            L.m3d_event_destroy(e1)
        self._pending = []
