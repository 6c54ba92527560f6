"""Tensor-level wrappers over the C ABI for NCHW torch tensors (the op-level drop-in boundary).

These are what the standalone modules (DCNv2, DCN, ...) call.  The whole-network path
(``RPN.forward``) does not go through here -- it runs the NHWC engine (m3dssd_amd/engine.py).
"""
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


def dcn_v2_backward(inp, offset, mask, weight, grad_output, stride, padding, dilation=1, deformable_groups=1,
                    needs=(True, True, True, True, True)):
    """DCNv2Function.backward (model/DCNv2/dcn_v2_func.py:40-62) on the HIP library: returns (grad_input, grad_offset, grad_mask,
    grad_weight, grad_bias); an entry of ``needs`` that is False gives None and skips the work only that gradient needs.
    Every returned gradient is freshly written (nothing is accumulated into).  The compute type is the dtype of ``inp`` (float32
    or bfloat16); each gradient comes back in the dtype of the tensor it belongs to (grad_bias: float32), so a float32 weight
    under a bfloat16 input gets a float32 gradient that went through one bfloat16 rounding."""
    _require_cuda(inp, offset, mask, weight, grad_output)
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
    query = L.m3d_dcn_v2_backward_workspace_bytes_bf16 if bf16 else L.m3d_dcn_v2_backward_workspace_bytes
    nbytes = query(n, c, h, w, co, kh, kw, stride, padding, dilation, deformable_groups)
    if nbytes < 0:
        raise RuntimeError("dcn_v2_backward: bad shape")
    ws, base = _workspace(nbytes, inp.device)
    ptrs = [g.data_ptr() if g is not None else None for g in grads]
    geom = (n, c, h, w, co, kh, kw, stride, stride, padding, padding, dilation, dilation, deformable_groups)
    with torch.cuda.device(inp.device):
        if bf16:
            _hip.check(L.m3d_dcn_v2_backward_bf16(inp.data_ptr(), weight.data_ptr(), offset.data_ptr(), off16, mask.data_ptr(), mask16,
                                                  grad_output.data_ptr(), *ptrs, *geom, base, nbytes, _stream()))
        else:
            _hip.check(L.m3d_dcn_v2_backward(inp.data_ptr(), weight.data_ptr(), offset.data_ptr(), mask.data_ptr(),
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
    m3d_dcn_v2_backward behind it."""
    _require_cuda(inp, offset, mask, weight, bias)
    return _DCNv2.apply(inp, offset, mask, weight, bias, stride, padding, dilation, deformable_groups)


def rpn_targets(cls, prob, anchors, conf_vec, gt_table, feat_size):
    """compute_targets (lib/rpn_util.py:430-532) for a whole batch on the device: m3d_rpn_targets.  ``anchors`` float64 device
    [A, 9], ``conf_vec`` from ``host.loss.pack_conf``, ``gt_table`` from ``host.loss.pack_gts``; see host/loss.py."""
    from . import loss
    return loss.rpn_targets(cls, prob, anchors, conf_vec, gt_table, feat_size)


def rpn_loss(cls, prob, bbox_2d, bbox_3d, anchors, conf_vec, gt_table, feat_size, return_details=False):
    """The RPN_3D_loss computation below the module: m3d_rpn_targets + m3d_rpn_loss, differentiable in cls, bbox_2d, bbox_3d."""
    from . import loss
    return loss.rpn_loss(cls, prob, bbox_2d, bbox_3d, anchors, conf_vec, gt_table, feat_size, return_details)


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
