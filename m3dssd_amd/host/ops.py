"""Tensor-level wrappers over the C ABI for NCHW torch tensors (the op-level drop-in boundary).

These are what the standalone modules (DCNv2, DCN, ...) call.  The whole-network path
(``RPN.forward``) does not go through here -- it runs the NHWC engine (m3dssd_amd/engine.py).
"""
import collections
import ctypes

import torch

from .. import _hip


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            # the reference raises NotImplementedError for non-CUDA input (model/DCNv2/dcn_v2_func.py:23-24)
            raise NotImplementedError("M3DSSD HIP ops need ROCm device tensors; there is no CPU fallback")


_DCN_DTYPES = (torch.float32, torch.bfloat16)


def _dcn_prepare(name, inp, offset, mask, weight, stride, padding, dilation, deformable_groups):
    """The checks and casts the forward and the backward share.  The compute type is the dtype of ``inp``: float32 or bfloat16.
    ``weight`` is cast to it (autocast's cast of a float32 parameter); offsets and masks are used as float32 -- a bfloat16 tensor is
    handed over as it is and widened by the kernel (exact), anything else is cast to float32.  Returns (offset, mask, weight,
    (n, c, h, w, co, kh, kw, ho, wo), offset_is_bf16, mask_is_bf16)."""
    if not inp.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")          # dcn_v2_cuda.c:21
    if not weight.is_contiguous():
        raise RuntimeError("weight tensor has to be contiguous")         # dcn_v2_cuda.c:22
    if inp.dtype not in _DCN_DTYPES:
        raise RuntimeError("%s: the input is %s; float32 and bfloat16 are supported" % (name, inp.dtype))
    if not weight.dtype.is_floating_point:
        raise RuntimeError("%s: the weight is %s; a floating-point tensor is needed" % (name, weight.dtype))
    bf16 = inp.dtype == torch.bfloat16
    n, c, h, w = inp.shape
    co, ck, kh, kw = weight.shape
    if ck != c:
        raise RuntimeError("Input shape and kernel channels wont match: (%d vs %d)." % (c, ck))   # dcn_v2_cuda.c:37-39
    if deformable_groups < 1 or c % deformable_groups:
        raise RuntimeError("%s: deformable_groups (%d) must divide the input channels (%d)" % (name, deformable_groups, c))
    if bf16 and dilation != 1:
        raise RuntimeError("%s: the bf16 path supports dilation 1 only (got %d); use float32 tensors for a dilated layer"
                           % (name, dilation))
    ho = (h + 2 * padding - (dilation * (kh - 1) + 1)) // stride + 1
    wo = (w + 2 * padding - (dilation * (kw - 1) + 1)) // stride + 1
    if tuple(offset.shape) != (n, deformable_groups * 2 * kh * kw, ho, wo) or \
            tuple(mask.shape) != (n, deformable_groups * kh * kw, ho, wo):
        raise RuntimeError("%s: offset/mask shape does not match the output size" % name)
    weight = weight.to(inp.dtype)                                        # (a no-op for a weight of the compute type)
    off16 = bf16 and offset.dtype == torch.bfloat16
    mask16 = bf16 and mask.dtype == torch.bfloat16
    offset = offset.contiguous() if off16 else offset.contiguous().float()
    mask = mask.contiguous() if mask16 else mask.contiguous().float()
    return offset, mask, weight, (n, c, h, w, co, kh, kw, ho, wo), int(off16), int(mask16)


def _workspace(nbytes, device):
    ws = torch.empty(nbytes + 256, device=device, dtype=torch.uint8)
    return ws, (ws.data_ptr() + 255) // 256 * 256


def dcn_v2_forward(inp, offset, mask, weight, bias, stride, padding, dilation=1, deformable_groups=1):
    """DCNv2Function.forward (model/DCNv2/dcn_v2_func.py:22-38) on the HIP library.  float32 input: m3d_dcn_v2_forward; bfloat16
    input (what torch.autocast hands over): m3d_dcn_v2_forward_bf16, bfloat16 output.  Other types raise RuntimeError."""
    _require_cuda(inp, offset, mask, weight, bias)
    offset, mask, weight, dims, off16, mask16 = _dcn_prepare("dcn_v2_forward", inp, offset, mask, weight, stride, padding, dilation,
                                                             deformable_groups)
    n, c, h, w, co, kh, kw, ho, wo = dims
    L = _hip.lib()
    bias = bias.contiguous().float()
    out = torch.empty(n, co, ho, wo, device=inp.device, dtype=inp.dtype)
    geom = (n, c, h, w, co, kh, kw, stride, stride, padding, padding, dilation, dilation, deformable_groups)
    if inp.dtype == torch.bfloat16:
        nbytes = L.m3d_dcn_v2_workspace_bytes_bf16(n, c, h, w, co, kh, kw, stride, padding, dilation, deformable_groups)
        if nbytes < 0:
            raise RuntimeError("dcn_v2_forward: bad shape")
        ws, base = _workspace(nbytes, inp.device)
        with torch.cuda.device(inp.device):
            _hip.check(L.m3d_dcn_v2_forward_bf16(inp.data_ptr(), weight.data_ptr(), bias.data_ptr(), offset.data_ptr(), off16,
                                                 mask.data_ptr(), mask16, out.data_ptr(), *geom, base, nbytes, _stream()))
        return out
    nbytes = L.m3d_dcn_v2_workspace_bytes_grouped(n, c, h, w, co, kh, kw, stride, padding, dilation, deformable_groups)
    ws, base = _workspace(nbytes, inp.device)
    with torch.cuda.device(inp.device):
        _hip.check(L.m3d_dcn_v2_forward(inp.data_ptr(), weight.data_ptr(), bias.data_ptr(), offset.data_ptr(),
                                        mask.data_ptr(), out.data_ptr(), *geom, base, nbytes, _stream()))
    return out


_dcn_det_mode = None       # None: follow torch.are_deterministic_algorithms_enabled(); True / False: override it


def set_dcn_deterministic(mode):
    """Selects the form of grad_input in the DCNv2 backward and returns the previous mode.  ``True``: the bitwise-reproducible form
    (m3d_dcn_v2_backward_det / _det_bf16: 64-bit fixed-point sums); ``False``: float atomics (last bits depend on arrival order);
    ``None`` (the default): the reproducible form iff ``torch.are_deterministic_algorithms_enabled()``, warn-only or not --
    PyTorch's rule for an operator that has a deterministic alternative."""
    global _dcn_det_mode
    if mode is not None and not isinstance(mode, bool):
        raise TypeError("set_dcn_deterministic: mode must be None, True or False")
    prev, _dcn_det_mode = _dcn_det_mode, mode
    return prev


def dcn_deterministic():
    """The form a DCNv2 backward that runs now would take (see ``set_dcn_deterministic``)."""
    return torch.are_deterministic_algorithms_enabled() if _dcn_det_mode is None else _dcn_det_mode


def dcn_v2_backward(inp, offset, mask, weight, grad_output, stride, padding, dilation=1, deformable_groups=1,
                    needs=(True, True, True, True, True), deterministic=None):
    """DCNv2Function.backward (model/DCNv2/dcn_v2_func.py:40-62) on the HIP library: returns (grad_input, grad_offset, grad_mask,
    grad_weight, grad_bias); an entry of ``needs`` that is False gives None and skips the work only that gradient needs.
    Every returned gradient is freshly written (nothing is accumulated into).  The compute type is the dtype of ``inp`` (float32
    or bfloat16); each gradient comes back in the dtype of the tensor it belongs to (grad_bias: float32), so a float32 weight
    under a bfloat16 input gets a float32 gradient that went through one bfloat16 rounding.
    ``deterministic``: True = grad_input from m3d_dcn_v2_backward_det (a function of the inputs alone: the same bits on every launch
    and in any batch; all NaN for an image whose grad_output, masks or the weights hold a NaN or infinity), False = float atomics,
    None = ``dcn_deterministic()``.  The other four gradients are reproducible, with the same bits, either way."""
    _require_cuda(inp, offset, mask, weight, grad_output)
    det = dcn_deterministic() if deterministic is None else bool(deterministic)
    owner_dtypes = (inp.dtype, offset.dtype, mask.dtype, weight.dtype, torch.float32)
    offset, mask, weight, dims, off16, mask16 = _dcn_prepare("dcn_v2_backward", inp, offset, mask, weight, stride, padding, dilation,
                                                             deformable_groups)
    n, c, h, w, co, kh, kw, ho, wo = dims
    if tuple(grad_output.shape) != (n, co, ho, wo):
        raise RuntimeError("dcn_v2_backward: grad_output shape does not match the output size")
    L = _hip.lib()
    bf16 = inp.dtype == torch.bfloat16
    grad_output = grad_output.contiguous().to(inp.dtype)
    shapes = (inp.shape, offset.shape, mask.shape, weight.shape, (co,))
    # what the kernels write: the compute type for grad_input / grad_weight, float32 for grad_offset / grad_mask / grad_bias
    kdt = (inp.dtype, torch.float32, torch.float32, inp.dtype, torch.float32)
    grads = [torch.empty(tuple(s), device=inp.device, dtype=dt) if need else None for s, dt, need in zip(shapes, kdt, needs)]
    query, call = {(False, False): (L.m3d_dcn_v2_backward_workspace_bytes, L.m3d_dcn_v2_backward),
                   (False, True): (L.m3d_dcn_v2_backward_det_workspace_bytes, L.m3d_dcn_v2_backward_det),
                   (True, False): (L.m3d_dcn_v2_backward_workspace_bytes_bf16, L.m3d_dcn_v2_backward_bf16),
                   (True, True): (L.m3d_dcn_v2_backward_det_workspace_bytes_bf16, L.m3d_dcn_v2_backward_det_bf16)}[(bf16, det)]
    nbytes = query(n, c, h, w, co, kh, kw, stride, padding, dilation, deformable_groups)
    if nbytes < 0:
        raise RuntimeError("dcn_v2_backward: bad shape")
    ws, base = _workspace(nbytes, inp.device)
    ptrs = [g.data_ptr() if g is not None else None for g in grads]
    geom = (n, c, h, w, co, kh, kw, stride, stride, padding, padding, dilation, dilation, deformable_groups)
    with torch.cuda.device(inp.device):
        if bf16:
            _hip.check(call(inp.data_ptr(), weight.data_ptr(), offset.data_ptr(), off16, mask.data_ptr(), mask16,
                            grad_output.data_ptr(), *ptrs, *geom, base, nbytes, _stream()))
        else:
            _hip.check(call(inp.data_ptr(), weight.data_ptr(), offset.data_ptr(), mask.data_ptr(),
                            grad_output.data_ptr(), *ptrs, *geom, base, nbytes, _stream()))
    return tuple(g if g is None else g.to(dt) for g, dt in zip(grads, owner_dtypes))


class _DCNv2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
        ctx.conf = (stride, padding, dilation, deformable_groups)
        ctx.save_for_backward(inp, offset, mask, weight)
        return dcn_v2_forward(inp, offset, mask, weight, bias, stride, padding, dilation, deformable_groups)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        inp, offset, mask, weight = ctx.saved_tensors
        grads = dcn_v2_backward(inp, offset, mask, weight, grad_output, *ctx.conf, needs=tuple(ctx.needs_input_grad[:5]))
        return grads + (None, None, None, None)


def dcn_v2(inp, offset, mask, weight, bias, stride, padding, dilation=1, deformable_groups=1):
    """The DCNv2 operator, differentiable in its five tensor arguments: m3d_dcn_v2_forward (the bits of ``dcn_v2_forward``) with
    m3d_dcn_v2_backward behind it -- or m3d_dcn_v2_backward_det, whose grad_input is bitwise reproducible, when ``dcn_deterministic()``
    holds at the time the backward runs (``torch.use_deterministic_algorithms(True)`` or ``set_dcn_deterministic(True)``)."""
    _require_cuda(inp, offset, mask, weight, bias)
    return _DCNv2.apply(inp, offset, mask, weight, bias, stride, padding, dilation, deformable_groups)


def _psroi_prepare(name, data, rois, offset, no_trans, output_dim, group_size, pooled_size, part_size, sample_per_part, trans_std):
    """The checks the pooling forward and backward share.  Returns (rois, offset or None, (N, C, H, W, n, rows, K))."""
    _require_cuda(data, rois)
    if not no_trans:
        _require_cuda(offset)
    for t, what in ((data, "data"), (rois, "rois")) + (() if no_trans else ((offset, "offset"),)):
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s is %s; only float32 is supported" % (name, what, t.dtype))
    if not (0.0 <= trans_std <= 1.0):
        raise RuntimeError("%s: trans_std must lie in [0, 1]" % name)            # the reference's assert (dcn_v2_func.py:97)
    if data.dim() != 4 or rois.dim() != 2 or rois.shape[1] != 5:
        raise RuntimeError("%s: data must be [N, C, H, W] and rois [n, 5]" % name)
    if not data.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")
    N, C, H, W = data.shape
    n = rois.shape[0]
    rows, K = 0, 1
    if not no_trans:
        if offset.dim() != 4 or offset.shape[1] % 2 or offset.shape[1] < 2 or tuple(offset.shape[2:]) != (part_size, part_size):
            raise RuntimeError("%s: offset must be [>= n, 2 * classes, part_size, part_size]" % name)
        rows, K = offset.shape[0], offset.shape[1] // 2
        offset = offset.contiguous()
    return rois.contiguous(), (None if no_trans else offset), (N, C, H, W, n, rows, K)


def _psroi_workspace(L, name, dims, output_dim, group_size, pooled_size, backward, device):
    N, C, H, W, n, rows, K = dims
    nbytes = L.m3d_dcn_v2_psroi_pooling_workspace_bytes(N, C, H, W, n, K, output_dim, group_size, pooled_size, int(backward))
    if nbytes < 0:
        raise RuntimeError("%s: bad shape (data channels %d, output_dim %d, group_size %d, classes %d)" % (name, C, output_dim, group_size, K))
    return _workspace(nbytes, device) + (nbytes,)


def psroi_pooling_forward(data, rois, offset, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                          sample_per_part, trans_std):
    """DCNv2PoolingFunction.forward (model/DCNv2/dcn_v2_func.py:99-115) on the HIP library: m3d_dcn_v2_psroi_pooling_forward.
    float32 only.  Returns (output, output_count), both [n, output_dim, pooled_size, pooled_size]; ``offset`` is ignored when
    ``no_trans``."""
    name = "psroi_pooling_forward"
    rois, offset, dims = _psroi_prepare(name, data, rois, offset, no_trans, output_dim, group_size, pooled_size, part_size,
                                        sample_per_part, trans_std)
    N, C, H, W, n, rows, K = dims
    L = _hip.lib()
    out = torch.empty(n, output_dim, pooled_size, pooled_size, device=data.device, dtype=torch.float32)
    count = torch.empty_like(out)
    ws, base, nbytes = _psroi_workspace(L, name, dims, output_dim, group_size, pooled_size, False, data.device)
    with torch.cuda.device(data.device):
        _hip.check(L.m3d_dcn_v2_psroi_pooling_forward(data.data_ptr(), rois.data_ptr(), None if offset is None else offset.data_ptr(),
                                                      out.data_ptr(), count.data_ptr(), N, C, H, W, n, rows, K, int(bool(no_trans)),
                                                      float(spatial_scale), output_dim, group_size, pooled_size, part_size,
                                                      sample_per_part, float(trans_std), base, nbytes, _stream()))
    return out, count


def psroi_pooling_backward(grad_output, data, rois, offset, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                           sample_per_part, trans_std, needs=(True, True)):
    """DCNv2PoolingFunction.backward (model/DCNv2/dcn_v2_func.py:117-140) on the HIP library: returns (grad_data, grad_offset),
    freshly written; an entry of ``needs`` that is False (or grad_offset under ``no_trans``) gives None and skips its work.  The
    sample counts are recomputed by the kernel."""
    name = "psroi_pooling_backward"
    _require_cuda(grad_output)
    rois, offset, dims = _psroi_prepare(name, data, rois, offset, no_trans, output_dim, group_size, pooled_size, part_size,
                                        sample_per_part, trans_std)
    N, C, H, W, n, rows, K = dims
    if tuple(grad_output.shape) != (n, output_dim, pooled_size, pooled_size):
        raise RuntimeError("%s: grad_output shape does not match the output size" % name)
    if grad_output.dtype != torch.float32:
        raise RuntimeError("%s: grad_output is %s; only float32 is supported" % (name, grad_output.dtype))
    L = _hip.lib()
    grad_output = grad_output.contiguous()
    gdata = torch.empty_like(data) if needs[0] else None
    goff = torch.empty_like(offset) if needs[1] and offset is not None else None
    ws, base, nbytes = _psroi_workspace(L, name, dims, output_dim, group_size, pooled_size, True, data.device)
    with torch.cuda.device(data.device):
        _hip.check(L.m3d_dcn_v2_psroi_pooling_backward(grad_output.data_ptr(), data.data_ptr(), rois.data_ptr(),
                                                       None if offset is None else offset.data_ptr(),
                                                       None if gdata is None else gdata.data_ptr(),
                                                       None if goff is None else goff.data_ptr(), N, C, H, W, n, rows, K,
                                                       int(bool(no_trans)), float(spatial_scale), output_dim, group_size, pooled_size,
                                                       part_size, sample_per_part, float(trans_std), base, nbytes, _stream()))
    return gdata, goff


class _PSROIPooling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, rois, offset, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part,
                trans_std):
        ctx.conf = (no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part, trans_std)
        ctx.save_for_backward(data, rois, offset)
        out, count = psroi_pooling_forward(data, rois, offset, *ctx.conf)
        ctx.mark_non_differentiable(count)
        return out, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output, _grad_count):
        data, rois, offset = ctx.saved_tensors
        gdata, goff = psroi_pooling_backward(grad_output, data, rois, offset, *ctx.conf,
                                             needs=(ctx.needs_input_grad[0], ctx.needs_input_grad[2]))
        if ctx.needs_input_grad[2] and goff is None:            # no_trans: the offsets are not used
            goff = torch.zeros_like(offset)
        return (gdata, None, goff) + (None,) * 8


def psroi_pooling(data, rois, offset, no_trans, spatial_scale, output_dim, group_size=1, pooled_size=7, part_size=None,
                  sample_per_part=4, trans_std=0.0, return_count=False):
    """Deformable PS-ROI pooling, differentiable in ``data`` and ``offset`` (``rois`` get None): m3d_dcn_v2_psroi_pooling_forward
    with m3d_dcn_v2_psroi_pooling_backward behind it.  ``offset`` may be an empty tensor when ``no_trans``."""
    _require_cuda(data, rois)
    part_size = pooled_size if part_size is None else part_size
    out, count = _PSROIPooling.apply(data, rois, offset, bool(no_trans), spatial_scale, output_dim, group_size, pooled_size, part_size,
                                     sample_per_part, trans_std)
    return (out, count) if return_count else out


_ANAB_PAIRS = ((64, 128), (128, 128), (168, 128), (168, 256))

# What differs between the two compute types of the ANAB training operator.  ``q_align`` / ``kvg_align``: (bytes, row-stride multiple
# in elements) that a view must meet to be handed over as it is, else it is copied once.  ``kvg_align`` None: k / v / gates are
# handed over untouched with whatever row stride they have, and a non-unit inner stride of any operand raises.
_AnabType = collections.namedtuple("_AnabType", "dtype dtype_name query forward backward q_align kvg_align")
_ANAB_F32 = _AnabType(torch.float32, "float32", "m3d_anab_attention_workspace_bytes", "m3d_anab_attention_forward",
                      "m3d_anab_attention_backward", (16, 4), None)
_ANAB_BF16 = _AnabType(torch.bfloat16, "bfloat16", "m3d_anab_attention_workspace_bytes_bf16", "m3d_anab_attention_forward_bf16",
                       "m3d_anab_attention_backward_bf16", (16, 8), (4, 2))


def _anab_aligned(t, align=_ANAB_F32.q_align):
    """q / grad_out go through 16-byte loads (bf16 k / v / gates through 4-byte loads): an unaligned view or an odd row stride is
    copied once, and so is a view whose rows overlap (row stride below the channel count: the expanded grad_out that autograd hands
    over behind ``.sum(0)``)."""
    nbytes, stride_of = align
    if t.data_ptr() % nbytes == 0 and t.stride(0) % stride_of == 0 and t.stride(0) >= t.shape[1] and t.stride(1) == 1:
        return t
    return t.contiguous()


def _anab_prepare(name, q, k, v, gates, B, H, W, ty=_ANAB_F32):
    """The shape and type rules of both calls, then the alignment contract of the kernels -> (Ck, Cv, q, k, v, gates).  The operands
    are row matrices [rows, C] that may be column slices of a wider one."""
    _require_cuda(q, k, v, gates)
    rows = B * H * W
    for t, what in ((q, "q"), (k, "k"), (v, "v"), (gates, "gates")):
        if t.dtype != ty.dtype:
            raise RuntimeError("%s: %s is %s; only %s is supported" % (name, what, t.dtype, ty.dtype_name))
        if t.dim() != 2 or t.shape[0] != rows:
            raise RuntimeError("%s: %s must be a row matrix [B*H*W = %d, C] (got %s)" % (name, what, rows, tuple(t.shape)))
        if ty.kvg_align is None and (t.stride(1) != 1 or t.stride(0) < t.shape[1]):
            raise RuntimeError("%s: %s must have unit stride inside a row (a column slice of a row-major matrix)" % (name, what))
    ck, cv = q.shape[1], v.shape[1]
    if k.shape[1] != ck or gates.shape[1] != 4:
        raise RuntimeError("%s: q and k need the same channel count and gates 4 channels (got %d, %d, %d)"
                           % (name, ck, k.shape[1], gates.shape[1]))
    if (H * W) % 128:
        raise RuntimeError("%s: H*W must be a multiple of 128 (HW %% 128 == 0; got %dx%d)" % (name, H, W))
    if (ck, cv) not in _ANAB_PAIRS:
        raise RuntimeError("%s: (Ck, Cv) must be one of %s (got (%d, %d))" % (name, _ANAB_PAIRS, ck, cv))
    if ty.kvg_align is not None:
        k, v, gates = (_anab_aligned(t, ty.kvg_align) for t in (k, v, gates))
    return ck, cv, _anab_aligned(q, ty.q_align), k, v, gates


def _anab_forward(ty, q, k, v, gates, B, H, W):
    name = ty.forward[4:]
    ck, cv, q, k, v, gates = _anab_prepare(name, q, k, v, gates, B, H, W, ty)
    L = _hip.lib()
    nbytes = getattr(L, ty.query)(B, H, W, ck, cv, 0)
    if nbytes < 0:
        raise RuntimeError("%s: unsupported shape" % name)
    out = torch.empty(B * H * W, cv, device=q.device, dtype=ty.dtype)
    ws, base = _workspace(nbytes, q.device)
    with torch.cuda.device(q.device):
        _hip.check(getattr(L, ty.forward)(q.data_ptr(), k.data_ptr(), v.data_ptr(), gates.data_ptr(), out.data_ptr(), B, H, W, ck, cv,
                                          q.stride(0), k.stride(0), v.stride(0), gates.stride(0), cv, base, nbytes, _stream()))
    return out


def _anab_backward(ty, q, k, v, gates, grad_out, B, H, W, needs):
    name = ty.backward[4:]
    _require_cuda(grad_out)
    ck, cv, q, k, v, gates = _anab_prepare(name, q, k, v, gates, B, H, W, ty)
    if grad_out.dtype != ty.dtype or tuple(grad_out.shape) != (B * H * W, cv):
        raise RuntimeError("%s: grad_out must be %s [B*H*W, Cv]" % (name, ty.dtype_name))
    L = _hip.lib()
    grad_out = _anab_aligned(grad_out, ty.q_align)
    nbytes = getattr(L, ty.query)(B, H, W, ck, cv, 1)
    if nbytes < 0:
        raise RuntimeError("%s: unsupported shape" % name)
    grads = [torch.empty(B * H * W, c, device=q.device, dtype=ty.dtype) if need else None for c, need in zip((ck, ck, cv, 4), needs)]
    ptrs = [g.data_ptr() if g is not None else None for g in grads]
    ws, base = _workspace(nbytes, q.device)
    with torch.cuda.device(q.device):
        _hip.check(getattr(L, ty.backward)(q.data_ptr(), k.data_ptr(), v.data_ptr(), gates.data_ptr(), grad_out.data_ptr(), *ptrs, B, H,
                                           W, ck, cv, q.stride(0), k.stride(0), v.stride(0), gates.stride(0), grad_out.stride(0), ck,
                                           ck, cv, 4, base, nbytes, _stream()))
    return tuple(grads)


def anab_attention_forward(q, k, v, gates, B, H, W):
    """m3d_anab_attention_forward: out [B*H*W, Cv] = softmax_keys(q . khat^T) . vhat with the gated pyramid pooling of ANAB."""
    return _anab_forward(_ANAB_F32, q, k, v, gates, B, H, W)


def anab_attention_backward(q, k, v, gates, grad_out, B, H, W, needs=(True, True, True, True)):
    """m3d_anab_attention_backward: (grad_q, grad_k, grad_v, grad_gates), freshly written and contiguous; an entry of ``needs`` that
    is False gives None and skips the work only that gradient needs."""
    return _anab_backward(_ANAB_F32, q, k, v, gates, grad_out, B, H, W, needs)


def anab_attention_forward_bf16(q, k, v, gates, B, H, W):
    """m3d_anab_attention_forward_bf16: anab_attention_forward on bfloat16 rows, bfloat16 out [B*H*W, Cv]."""
    return _anab_forward(_ANAB_BF16, q, k, v, gates, B, H, W)


def anab_attention_backward_bf16(q, k, v, gates, grad_out, B, H, W, needs=(True, True, True, True)):
    """m3d_anab_attention_backward_bf16: (grad_q, grad_k, grad_v, grad_gates) in bfloat16, freshly written and contiguous; an entry
    of ``needs`` that is False gives None and skips the work only that gradient needs."""
    return _anab_backward(_ANAB_BF16, q, k, v, gates, grad_out, B, H, W, needs)


def _anab_fn_forward(ctx, ty, q, k, v, gates, B, H, W):
    ctx.dims = (B, H, W)
    ctx.save_for_backward(q, k, v, gates)
    return _anab_forward(ty, q, k, v, gates, B, H, W)


def _anab_fn_backward(ctx, ty, grad_out):
    return _anab_backward(ty, *ctx.saved_tensors, grad_out, *ctx.dims, needs=tuple(ctx.needs_input_grad[:4])) + (None, None, None)


class _ANABAttention(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, q, k, v, gates, B, H, W):
        return _anab_fn_forward(ctx, _ANAB_F32, q, k, v, gates, B, H, W)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return _anab_fn_backward(ctx, _ANAB_F32, grad_out)


class _ANABAttentionBf16(torch.autograd.Function):
    # (no custom_fwd cast: the operands are bfloat16 already, inside an autocast region or outside one)
    @staticmethod
    def forward(ctx, q, k, v, gates, B, H, W):
        return _anab_fn_forward(ctx, _ANAB_BF16, q, k, v, gates, B, H, W)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return _anab_fn_backward(ctx, _ANAB_BF16, grad_out)


def anab_attention(q, k, v, gates, B, H, W):
    """The ANAB attention core (gated pyramid pooling of k / v into 337 keys, softmax(q . khat^T) . vhat), differentiable in its four
    tensor arguments: m3d_anab_attention_forward with m3d_anab_attention_backward behind it.  Row matrices [B*H*W, C], float32;
    column slices of one wider matrix are taken as they are (their row stride is handed to the kernels).  ``gates`` are the four
    spatial gates behind their sigmoid.  No torch fallback: an unsupported shape raises RuntimeError."""
    _require_cuda(q, k, v, gates)
    # (the shape and type rules are checked by anab_attention_forward, behind the float32 cast of custom_fwd under autocast)
    return _ANABAttention.apply(q, k, v, gates, B, H, W)


def anab_attention_bf16(q, k, v, gates, B, H, W):
    """``anab_attention`` in bfloat16: bfloat16 row matrices in (column slices are taken as they are where they meet the alignment
    of the kernels, else copied once), bfloat16 out, bfloat16 gradients; m3d_anab_attention_forward_bf16 with
    m3d_anab_attention_backward_bf16 behind it, inside or outside an autocast region, never through float32.  Any operand that is not
    bfloat16 raises RuntimeError; no torch fallback."""
    _require_cuda(q, k, v, gates)
    for t, what in ((q, "q"), (k, "k"), (v, "v"), (gates, "gates")):
        if t.dtype != torch.bfloat16:
            raise RuntimeError("anab_attention_bf16: %s is %s; only bfloat16 is supported" % (what, t.dtype))
    return _ANABAttentionBf16.apply(q, k, v, gates, B, H, W)


def _bn_check(name, named):
    """The type rules of both calls: device tensors (NotImplementedError: no CPU fallback), float32 (RuntimeError naming the dtype)."""
    _require_cuda(*(t for _, t in named))
    for what, t in named:
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s is %s; only float32 is supported" % (name, what, t.dtype))


def _bn_forward(x, residual, weight, bias, running_mean, running_var, momentum, eps, slope):
    """m3d_bn_act_train_forward -> (y, save_mean, save_invstd, x and weight as handed over).  The running statistics are updated in
    place."""
    name = "bn_act_train_forward"
    named = [("x", x), ("weight", weight), ("bias", bias)] + [(w, t) for w, t in (("residual", residual), (
        "running_mean", running_mean), ("running_var", running_var)) if t is not None]
    _bn_check(name, named)
    if x.dim() != 4:
        raise RuntimeError("%s: x must be [B, C, H, W] (got %s)" % (name, tuple(x.shape)))
    B, C, H, W = x.shape
    if residual is not None and residual.shape != x.shape:
        raise RuntimeError("%s: residual %s does not match x %s" % (name, tuple(residual.shape), tuple(x.shape)))
    for what, t in named[1:3] + [n for n in named[3:] if n[0] != "residual"]:
        if tuple(t.shape) != (C,):
            raise RuntimeError("%s: %s must be [C = %d] (got %s)" % (name, what, C, tuple(t.shape)))
    for what, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None and not t.is_contiguous():
            raise RuntimeError("%s: %s is written in place and has to be contiguous" % (name, what))
    L = _hip.lib()
    nbytes = L.m3d_bn_act_train_workspace_bytes(B, C, H, W)
    if nbytes < 0:
        # (torch: "Expected more than 1 value per channel when training")
        raise RuntimeError("%s: unsupported shape %s (more than 1 value per channel is needed)" % (name, tuple(x.shape)))
    x = x.detach().contiguous()
    residual = None if residual is None else residual.detach().contiguous()
    weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
    y = torch.empty_like(x)
    save_mean = torch.empty(C, device=x.device, dtype=torch.float32)
    save_invstd = torch.empty_like(save_mean)
    ws, base = _workspace(nbytes, x.device)
    with torch.cuda.device(x.device):
        _hip.check(L.m3d_bn_act_train_forward(x.data_ptr(), None if residual is None else residual.data_ptr(), weight.data_ptr(),
                                              bias.data_ptr(), None if running_mean is None else running_mean.data_ptr(),
                                              None if running_var is None else running_var.data_ptr(), y.data_ptr(),
                                              save_mean.data_ptr(), save_invstd.data_ptr(), B, C, H, W, float(eps), float(momentum),
                                              float(slope), base, nbytes, _stream()))
    return y, save_mean, save_invstd, x, weight


def bn_act_train_forward(x, residual, weight, bias, running_mean, running_var, momentum, eps, slope):
    """m3d_bn_act_train_forward, value only: y = act(batch_norm(x; batch statistics) (+ residual)) with act(z) = z > 0 ? z : slope * z,
    and the running statistics (either may be None) updated in place as nn.BatchNorm2d does with a float ``momentum``."""
    return _bn_forward(x, residual, weight, bias, running_mean, running_var, momentum, eps, slope)[0]


def _bn_backward(grad_y, x, y, weight, save_mean, save_invstd, slope, needs):
    """m3d_bn_act_train_backward on operands the forward has checked and made contiguous; ``grad_y`` is autograd's."""
    name = "bn_act_train_backward"
    if not grad_y.is_cuda:
        raise NotImplementedError("M3DSSD HIP ops need ROCm device tensors; there is no CPU fallback")
    if grad_y.dtype != torch.float32 or grad_y.shape != x.shape:
        raise RuntimeError("%s: grad_y is %s %s; float32 %s is needed" % (name, grad_y.dtype, tuple(grad_y.shape), tuple(x.shape)))
    B, C, H, W = x.shape
    L = _hip.lib()
    nbytes = L.m3d_bn_act_train_workspace_bytes(B, C, H, W)
    grad_y = grad_y.contiguous()                                 # (an expanded grad_y is copied)
    grads = [torch.empty_like(x) if needs[0] else None, torch.empty_like(x) if needs[1] else None,
             torch.empty_like(save_mean) if needs[2] else None, torch.empty_like(save_mean) if needs[3] else None]
    ws, base = _workspace(nbytes, x.device)
    with torch.cuda.device(x.device):
        _hip.check(L.m3d_bn_act_train_backward(grad_y.data_ptr(), x.data_ptr(), y.data_ptr(), weight.data_ptr(), save_mean.data_ptr(),
                                               save_invstd.data_ptr(), *(None if g is None else g.data_ptr() for g in grads), B, C, H, W,
                                               float(slope), base, nbytes, _stream()))
    return tuple(grads)


def bn_act_train_backward(grad_y, x, y, weight, save_mean, save_invstd, slope, needs=(True, True, True, True)):
    """m3d_bn_act_train_backward: (grad_x, grad_residual, grad_weight, grad_bias), freshly written and contiguous; an entry of
    ``needs`` that is False gives None and skips the work only that gradient needs."""
    name = "bn_act_train_backward"
    _bn_check(name, (("grad_y", grad_y), ("x", x), ("y", y), ("weight", weight), ("save_mean", save_mean), ("save_invstd", save_invstd)))
    if x.dim() != 4 or y.shape != x.shape or _hip.lib().m3d_bn_act_train_workspace_bytes(*x.shape) < 0:
        raise RuntimeError("%s: x and y must be [B, C, H, W] of one supported shape (got %s, %s)" % (name, tuple(x.shape), tuple(y.shape)))
    for what, t in (("weight", weight), ("save_mean", save_mean), ("save_invstd", save_invstd)):
        if tuple(t.shape) != (x.shape[1],):
            raise RuntimeError("%s: %s must be [C = %d] (got %s)" % (name, what, x.shape[1], tuple(t.shape)))
    return _bn_backward(grad_y, x.contiguous(), y.contiguous(), weight.detach().contiguous(), save_mean.contiguous(),
                        save_invstd.contiguous(), slope, needs)


class _BNActTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, momentum, eps, slope):
        y, save_mean, save_invstd, xc, wc = _bn_forward(x, residual, weight, bias, running_mean, running_var, momentum, eps, slope)
        ctx.slope = slope
        ctx.save_for_backward(xc, y, wc, save_mean, save_invstd)              # two activation tensors: the input and the OUTPUT
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, y, weight, save_mean, save_invstd = ctx.saved_tensors
        grads = _bn_backward(grad_y, x, y, weight, save_mean, save_invstd, ctx.slope, ctx.needs_input_grad[:4])
        return grads + (None,) * 5


def bn_act_train(x, residual, weight, bias, running_mean, running_var, momentum, eps, slope):
    """BatchNorm2d with batch statistics (+ ``residual``, which may be None) + activation (``slope``: 0 ReLU, a LeakyReLU's
    negative_slope, 1 none) as one operator, differentiable in x, residual, weight and bias: m3d_bn_act_train_forward with
    m3d_bn_act_train_backward behind it.  float32 NCHW device tensors (made contiguous); ``running_mean`` / ``running_var`` are
    updated in place.  A host tensor raises NotImplementedError, another dtype RuntimeError (the checks of ``bn_act_train_forward``);
    no torch fallback."""
    return _BNActTrain.apply(x, residual, weight, bias, running_mean, running_var, momentum, eps, slope)


def rpn_targets(cls, prob, anchors, conf_vec, gt_table, feat_size):
    """compute_targets (lib/rpn_util.py:430-532) for a whole batch on the device: m3d_rpn_targets.  ``anchors`` float64 device
    [A, 9], ``conf_vec`` from ``host.loss.pack_conf``, ``gt_table`` from ``host.loss.pack_gts``; see host/loss.py."""
    from . import loss
    return loss.rpn_targets(cls, prob, anchors, conf_vec, gt_table, feat_size)


def rpn_loss(cls, prob, bbox_2d, bbox_3d, anchors, conf_vec, gt_table, feat_size, return_details=False):
    """The RPN_3D_loss computation below the module: m3d_rpn_targets + m3d_rpn_loss, differentiable in cls, bbox_2d, bbox_3d."""
    from . import loss
    return loss.rpn_loss(cls, prob, bbox_2d, bbox_3d, anchors, conf_vec, gt_table, feat_size, return_details)


def rpn_precompute_targets(anchors, conf_vec, gt_table, feat_size, device):
    """Kitti_Dataset_torch._targets (lib/dataloader.py:1014-1144) for a whole batch on the device, ahead of the forward:
    m3d_rpn_precompute_targets.  Returns the dict RPN_3D_loss_smp / rpn_loss_smp take: labels, gt_index (int16 [B, R]), bbox_2d
    (float32 [B, R, 4]), bbox_3d (float32 [B, R, 7]), meta: {any_val (int32 [B])}, all on ``device``."""
    from . import loss
    return loss.rpn_precompute_targets(anchors, conf_vec, gt_table, feat_size, device)


def rpn_loss_smp(cls, prob, bbox_2d, bbox_3d, target, anchors, conf_vec, feat_size, return_details=False):
    """The RPN_3D_loss_smp computation below the module: m3d_rpn_loss_smp over the pre-computed ``target`` dict (the reference's
    collated batch['target'], host or device, or the dict of rpn_precompute_targets), differentiable in cls, bbox_2d, bbox_3d."""
    from . import loss
    return loss.rpn_loss_smp(cls, prob, bbox_2d, bbox_3d, target, anchors, conf_vec, feat_size, return_details)


def rpn_target_stats(anchors, conf_vec, gt_table, feat_size, center=None, device="cuda:0"):
    """The per-image sums compute_bbox_stats (lib/rpn_util.py:732-889) takes over compute_targets, on the device with float64 anchor
    boxes: m3d_rpn_target_stats.  Returns float64 [B, 23] on the device: n_fg, sum(t - center) and sum((t - center)^2) of the 11
    raw float32 transforms over each image's fg rows.  ``gt_table`` from ``host.dataset_stats.pack_gts_scaled``."""
    from . import loss
    return loss.rpn_target_stats(anchors, conf_vec, gt_table, feat_size, center, device)


def nms_sorted(boxes_sorted, thresh):
    """Device NMS on score-sorted boxes [B, n, >=4] (or [n, >=4]) -> (keep [B, n] int32, num [B] int32)."""
    _require_cuda(boxes_sorted)
    L = _hip.lib()
    b3 = boxes_sorted if boxes_sorted.dim() == 3 else boxes_sorted[None]
    b3 = b3.contiguous().float()
    B, n, s = b3.shape
    keep = torch.empty(B, max(n, 1), device=b3.device, dtype=torch.int32)
    num = torch.zeros(B, device=b3.device, dtype=torch.int32)
    ws = torch.empty(max(1, L.m3d_nms_workspace_bytes(B, n)), device=b3.device, dtype=torch.uint8)
    with torch.cuda.device(b3.device):
        _hip.check(L.m3d_nms_sorted_dev(b3.data_ptr(), B, n, s, float(thresh), ws.data_ptr(), keep.data_ptr(),
                                        num.data_ptr(), _stream()))
    return keep, num
