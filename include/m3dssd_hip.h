/*
 * m3dssd_hip.h -- C ABI of libm3dssd_hip.so: the MI355X (gfx950) native hot path of M3DSSD.
 *
 * Plain pointers and sizes only (no torch types).  All device pointers are BORROWED (the
 * caller -- torch, or any other allocator -- owns them); nothing here allocates device
 * memory except the legacy host-pointer `_nms` twin, which mirrors the reference's own
 * behaviour.  Every entry point is stream-ordered on the `hipStream_t` it is given,
 * re-entrant per stream, and returns an int status: 0 = ok, <0 = M3D_E_* (the host layer
 * maps these to Python RuntimeError, like THError/THArgCheck did in the reference).
 *
 * Reference interfaces replaced (paths relative to mumianyuxin/M3DSSD):
 *   m3d_dcn_v2_forward ......... void dcn_v2_cuda_forward(THCudaTensor *input, *weight, *bias, *ones,
 *                                 *offset, *mask, *output, *columns, kernel_h, kernel_w, stride_h,
 *                                 stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group)
 *                                 model/DCNv2/src/dcn_v2_cuda.h:9-17, dcn_v2_cuda.c:10-102,
 *                                 kernel model/DCNv2/src/cuda/dcn_v2_im2col_cuda.cu:118-180
 *   m3d_dcn_v2_backward ........ void dcn_v2_cuda_backward(THCudaTensor *input, *weight, *bias, *ones, *offset, *mask,
 *                                 *columns, *grad_input, *grad_weight, *grad_bias, *grad_offset, *grad_mask,
 *                                 *grad_output, kernel_h, ..., deformable_group)
 *                                 model/DCNv2/src/dcn_v2_cuda.h:18-29, dcn_v2_cuda.c:104-241, kernels
 *                                 model/DCNv2/src/cuda/dcn_v2_im2col_cuda.cu:49-116,182-312
 *   m3d_dcn_v2_backward_workspace_bytes .. the `ones` / `columns` scratch tensors of that call (dcn_v2_func.py:41-48)
 *   m3d_rpn_targets / m3d_rpn_loss .. RPN_3D_loss.forward, lib/loss/rpn_3d.py:54-657, with compute_targets,
 *                                 lib/rpn_util.py:430-532 (host numpy in the reference) and the backward autograd derives
 *   m3d_rpn_loss_smp ........... RPN_3D_loss_smp.forward, lib/loss/rpn_3d.py:705-1360 (targets pre-computed by the loader)
 *   m3d_rpn_precompute_targets . Kitti_Dataset_torch._targets, lib/dataloader.py:1014-1144, for a whole batch
 *   m3d_rpn_target_stats ....... the per-image sums of compute_bbox_stats, lib/rpn_util.py:732-889 (it calls the numpy
 *                                 compute_targets twice per image of the imdb; float64 rois, unlike the loss)
 *   m3d_optim_prepare / _step .. torch.optim.SGD / Adam / Adamax .step() as lib/core.py:76-99 constructs them, and the
 *                                 `if total_loss > 0` of scripts/train_rpn_3d.py:208-218 as a device decision
 *   _nms / m3d_nms_sorted_dev .. void _nms(int* keep_out, int* num_out, const float* boxes_host,
 *                                 int boxes_num, int boxes_dim, float nms_overlap_thresh, int device_id)
 *                                 lib/nms/gpu_nms.hpp:1-2, lib/nms/nms_kernel.cu:91-144 (kernel :34-78)
 *   m3d_conv2d_forward ......... the cuDNN/ATen nn.Conv2d + BatchNorm2d(eval) + LeakyReLU + residual
 *                                 chains of model/pose_dla_dcn.py:107-121,261-269,379-389 and the RPN
 *                                 heads model/M3d_inference_align.py:66-210, plus (deformable mode)
 *                                 the fused im2col+GEMM of dcn_v2_cuda.c:80-96 without `columns`
 *   m3d_wino_conv3x3_forward ... the same Conv2d 3x3 stride-1 layers through Winograd F(2x2,3x3)
 *   m3d_head_mlp_forward ....... the 3-layer 1x1 heads, model/M3d_inference_align.py:77-210 (one launch per head)
 *   m3d_stem_conv7x7 ........... DLA.base_layer, model/pose_dla_dcn.py:336-340
 *   m3d_conv3x3_c16 ............ DLA.level0 (3x3 16->16 at full resolution), model/pose_dla_dcn.py:341-342
 *   m3d_maxpool2x2 ............. Tree.downsample nn.MaxPool2d(2,2), pose_dla_dcn.py:306,316
 *   m3d_upsample2x_add ......... IDAUp: depthwise ConvTranspose2d(4, s2, p1) + skip add,
 *                                 pose_dla_dcn.py:536-538,550-552
 *   m3d_anchor_select .......... softmax over classes + fg_prob + topk(k=1)/max/hard mask,
 *                                 M3d_inference_align.py:229-234, feturealign_mgpu.py:58-62,160-164
 *   m3d_align_offsets .......... offset/mask synthesis of shape_align (feturealign_mgpu.py:119-136,
 *                                 166-183) and center_align (:67-89)
 *   m3d_anab_pool* ............. PAPAModule weighted adaptive average pooling, attention.py:136-147
 *   m3d_softmax_rows ........... nn.Softmax(dim=-1) on the 337-key logits, attention.py:208
 *   m3d_bundle_outputs ......... flatten_tensor x13 + torch.cat + softmax, M3d_inference_align.py:280-301,
 *                                 lib/rpn_util.py:892-901 (+ the score key used by top-k)
 *   m3d_decode_rows ............ lib/rpn_util.py:1442-1521 (im_detect_3d decode) and
 *                                 bbox_transform_inv :1137-1186, for the top-N-pre rows
 */
#ifndef M3DSSD_HIP_H
#define M3DSSD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *m3d_stream_t; /* hipStream_t */

enum {
    M3D_OK = 0,
    M3D_E_ARG = -1,      /* bad argument / unsupported shape (message via m3d_last_error) */
    M3D_E_HIP = -2,      /* a HIP runtime call or kernel launch failed */
    M3D_E_WORKSPACE = -3 /* workspace too small */
};

/* Thread-local text of the last error returned on this thread. */
const char *m3d_last_error(void);
/* Library/ABI version.  Policy: the number moves whenever a caller built against the previous header could misbehave --
 * a signature or struct layout changes, the CONTRACT of an argument changes (a workspace size rule, a row limit, a
 * precondition), or existing entry points are removed or replaced.  Purely additive entry points do NOT move it: an old
 * binding never calls them, and a new binding on a library that lacks them fails at load, because the Python binding resolves
 * every declared name when it opens the library (m3dssd_amd/_hip.py: lib()).  A binding checks the number once after dlopen
 * and refuses a library of another version.
 *   4 -> 5 (round 6): m3d_conv_bf16_desc.dcn_ws sized by m3d_conv_bf16_dcn_ws_bytes(N, Ho, Wo) (was ">= 1024 bytes"),
 *                     m3d_nms_sorted_dev / m3d_topk_decode accept up to 16 384 rows per image (was 4 096), 15 entry
 *                     points added in round 5 (anab_attend_*, head_mlp2 / tail2 / qkvs bf16, tree_entry, frontend2, ...),
 *                     the round-4 experimental forms (bf16_wino2, bf16_frontend, bf16_head_mlp) left the product library.
 *   added under 5: m3d_dcn_v2_backward, m3d_dcn_v2_backward_workspace_bytes (additive; nothing existing changed);
 *                  m3d_rpn_targets, m3d_rpn_loss, m3d_rpn_loss_workspace_bytes (additive);
 *                  m3d_topk_decode_planar_mw, m3d_topk_decode_mw_workspace_bytes (additive);
 *                  m3d_conv_wave_forward_wgsplit, m3d_conv_wave_wgsplit_width (additive);
 *                  m3d_need_rows, m3d_need_rows_workspace_bytes, m3d_head_mlp_forward_rows, m3d_align_offsets_gated (additive);
 *                  m3d_dcn_v2_forward_bf16, m3d_dcn_v2_workspace_bytes_bf16, m3d_dcn_v2_backward_bf16,
 *                  m3d_dcn_v2_backward_workspace_bytes_bf16 (additive);
 *                  m3d_anab_attend_f32_rows (additive);
 *                  m3d_head_mlp2_bf16_forward_rows, m3d_anab_attend_bf16_rows (additive);
 *                  m3d_dcn_v2_psroi_pooling_forward, m3d_dcn_v2_psroi_pooling_backward,
 *                  m3d_dcn_v2_psroi_pooling_workspace_bytes (additive);
 *                  m3d_anab_attention_forward, m3d_anab_attention_backward, m3d_anab_attention_workspace_bytes (additive);
 *                  m3d_anab_attention_forward_bf16, m3d_anab_attention_backward_bf16,
 *                  m3d_anab_attention_workspace_bytes_bf16 (additive);
 *                  m3d_rpn_loss_smp, m3d_rpn_precompute_targets (additive);
 *                  m3d_refine_3d_host (additive);
 *                  m3d_rpn_target_stats, m3d_rpn_target_stats_workspace_bytes (additive);
 *                  m3d_dcn_v2_backward_det, m3d_dcn_v2_backward_det_bf16, m3d_dcn_v2_backward_det_workspace_bytes,
 *                  m3d_dcn_v2_backward_det_workspace_bytes_bf16 (additive);
 *                  m3d_optim_prepare, m3d_optim_step, m3d_optim_state_bytes (additive);
 *                  m3d_bn_act_train_forward, m3d_bn_act_train_backward, m3d_bn_act_train_workspace_bytes,
 *                  m3d_bn_act_train_chunks (additive);
 *                  m3d_topk_decode_planar_2d, m3d_post_rows, m3d_fill_post_3d (additive). */
#define M3D_ABI_VERSION 5
int m3d_abi_version(void);
/* "file:sha256[:16];file:sha256[:16];..." of the sources (csrc .hip / .h files and this header) the loaded library was built from. */
const char *m3d_source_hashes(void);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32), NHWC activations.
 *   GEMM view: M = N*Ho*Wo pixels, N = Cout, K = kh*kw*Cin (tap-major, channel-minor).
 *   out = act( conv(in, wgt) * scale[c] + shift[c] + res )   (res_mode 0; scale/shift/res optional)
 *   out = act( (conv(in, wgt) + res) * scale[c] + shift[c] )  (res_mode 1)
 * Deformable mode (dcn_offmask != NULL): the A operand is the modulated bilinear gather of
 * DCNv2 (dcn_v2_im2col_cuda.cu:18-47,129-178) computed on the fly -- no `columns` buffer.
 * ------------------------------------------------------------------------------------------ */
typedef struct m3d_conv_desc {
    const float *in;          /* NHWC view: in[(n*H + h)*W + w][c], pixel stride in_cs floats   */
    int in_cs;
    int N, H, W, Cin;         /* Cin % 16 == 0                                                  */
    const float *wgt;         /* packed [Cout_pad][K], K = (i*kw + j)*Cin + c; rows >= Cout = 0 */
    long long wgt_img_stride; /* 0, or floats between per-image weight sets (needs Ho*Wo % BM == 0) */
    int Cout, Cout_pad;       /* Cout_pad % 32 == 0                                             */
    int kh, kw, stride, pad, dil;
    int Ho, Wo;
    float *out;
    int out_cs;               /* NHWC pixel stride (out_nchw == 0)                              */
    int out_nchw;             /* 1: planar out[n*out_img_stride + c*Ho*Wo + p]                  */
    long long out_img_stride;
    const float *scale;       /* [Cout] or NULL (=1)                                            */
    const float *shift;       /* [Cout] or NULL (=0)                                            */
    const float *res;         /* NHWC residual view or NULL                                     */
    int res_cs;
    int res_mode;             /* 0: acc*scale+shift+res   1: (acc+res)*scale+shift (BN after the add) */
    int act;                  /* 0 none, 1 LeakyReLU(0.01)                                      */
    int sigmoid_from;         /* channels >= this get sigmoid instead of act; <0: none          */
    const float *dcn_offmask; /* NHWC [.., 3*kh*kw]: 2k=dh, 2k+1=dw, 2*kh*kw+k=mask; NULL=plain */
    int dcn_om_cs;
    float *splitk_ws;         /* optional scratch for split-K (small-M layers); NULL = never split   */
    long long splitk_ws_bytes;
} m3d_conv_desc;

int m3d_conv2d_forward(const m3d_conv_desc *d, m3d_stream_t stream);
/* Split-K plan of m3d_conv2d_forward for this descriptor: *splits (1 = no split) and the scratch bytes
 * (splits * N*Ho*Wo * Cout_pad * 4) the caller should provide through splitk_ws to enable it.  A layer whose
 * output tiles cannot give each of the 256 CUs a workgroup is split along K; partial sums are added in split
 * order by a second launch (deterministic), which also applies the epilogue. */
int m3d_conv2d_splitk_plan(const m3d_conv_desc *d, int *splits, long long *ws_bytes);

/* Wave-granular convolution / deformable convolution (csrc/dcn_wave.hip): same descriptor as m3d_conv2d_forward
 * (dcn_offmask optional), except that `wgt` is the packed [Cout_pad, kh*kw*Cin] matrix in MFMA-fragment order
 * [Cout_pad/32][kh*kw*Cin/8][h=2][r=32][t=4].  Each wave owns 32 pixels x 128 channels (64 when Cout_pad is an odd multiple of 64) and works alone (no workgroup
 * barrier).  m3d_conv_wave_applicable returns the number of waves the layer yields, or 0 when it does not apply
 * (needs Cin % 32 == 0, in_cs % 32 == 0, 128-byte aligned input, Cout_pad % 64 == 0, NHWC output; per-image weights
 * -- wgt_img_stride in floats between fragment-packed sets -- need Ho*Wo % 32 == 0) or when there are too few waves to fill the chip; the caller then stays on m3d_conv2d_forward. */
int m3d_conv_wave_applicable(const m3d_conv_desc *d);
/* Thin layers (too few 32 x 128 tiles) can still take this path split along K across waves: *splits and the scratch bytes to
 * pass through splitk_ws / splitk_ws_bytes (partials are reduced in split order by a second launch, which applies the
 * epilogue).  Without a workspace the layer is simply not split. */
int m3d_conv_wave_splitk_plan(const m3d_conv_desc *d, int *splits, long long *ws_bytes);
int m3d_conv_wave_forward(const m3d_conv_desc *d, m3d_stream_t stream);
/* The same layer with the K split of m3d_conv_wave_splitk_plan INSIDE the workgroups: the S = 2 / 4 / 8 waves of a workgroup
 * own one tile, each runs one K slice (the slices of the plan), the partial sums are added in slice order through LDS and the
 * epilogue is applied in the same launch -- the same bits as the workspace form, no workspace, no second launch.  splitk_ws /
 * splitk_ws_bytes are ignored (the plan is computed as if a workspace were given); a layer the plan does not split runs
 * unsplit.  This entry point alone also takes plain convolutions (no dcn_offmask, shared weights) with Cout_pad % 64 == 32:
 * one 32-channel column tile per wave (the 27 -> 32 channel offset / mask convs); m3d_conv_wave_splitk_plan reports their
 * split with *ws_bytes = 0 (there is no workspace form of them). */
int m3d_conv_wave_forward_wgsplit(const m3d_conv_desc *d, m3d_stream_t stream);
/* What that call launches: *slices = K slices (1 = unsplit; the fill threshold is advisory here as in the forward calls, so a
 * small layer is split too), *width = waves per workgroup (1 / 2 / 4 / 8, the next width that holds the slices). */
int m3d_conv_wave_wgsplit_width(const m3d_conv_desc *d, int *slices, int *width);

/* Winograd F(2x2,3x3) variant for 3x3 / stride 1 / pad 1 / even H,W plain convolutions (same descriptor; `wgt`
 * must point to the Winograd-transformed weights U = G g G^T packed in fragment order
 * [16 xi][Cout_pad/32][Cin/8][64][4], see m3dssd_amd/engine.py:pack_wino).  2.25x fewer MFMA FLOPs, fp32. */
int m3d_wino_conv3x3_forward(const m3d_conv_desc *d, m3d_stream_t stream);
/* Which kernel m3d_wino_conv3x3_forward runs for this descriptor: 1 = register-resident one-wave kernel (32 tiles x 32
 * channels x 16 transform positions in 512 registers, no LDS), 0 = LDS kernel (64 tiles x 32 channels per 512-thread
 * workgroup) -- chosen when the layer yields too few waves for the 1024 SIMDs or needs the sigmoid epilogue. */
int m3d_wino_conv3x3_variant(const m3d_conv_desc *d);
/* Thin layers can still use the wave kernel split along K across waves (and only the split form has the sigmoid epilogue):
 * *splits and the scratch bytes to pass through splitk_ws / splitk_ws_bytes; partials are reduced in split order by a second
 * launch.  m3d_wino_conv3x3_variant answers for the descriptor as given (with or without a workspace). */
int m3d_wino_conv3x3_splitk_plan(const m3d_conv_desc *d, int *splits, long long *ws_bytes);
/* Same with the kernel chosen by the caller: variant -1 = automatic, 0 = LDS kernel, 1 = wave kernel (tests, tuning). */
int m3d_wino_conv3x3_forward_ex(const m3d_conv_desc *d, int variant, m3d_stream_t stream);
/* Winograd F(4x4,3x3) on v_mfma_f32_16x16x4_f32 (csrc/wino44_conv.hip): 4x fewer MFMA FLOPs than the direct 3x3 convolution
 * (F(2x2,3x3): 2.25x).  Same descriptor and epilogue (scale / shift, residual, LeakyReLU) as m3d_wino_conv3x3_forward; `wgt`
 * points to U = G g G^T (6x6 per filter, fp64 -> fp32) packed [Cout_pad/32][Cin/16][36 xi][2][64][4], see
 * m3dssd_amd/engine.py:pack_wino44.  Needs H % 4 == W % 4 == 0, Cin % 16 == 0, Cout_pad % 64 == 0, no sigmoid channels, NHWC
 * output (m3d_wino44_applicable = 1).  fp32 rounding error ~7x that of direct summation (rms 1.5e-6 of the output scale at
 * Cin = 128). */
int m3d_wino44_applicable(const m3d_conv_desc *d);
int m3d_wino44_conv3x3_forward(const m3d_conv_desc *d, m3d_stream_t stream);
/* nb = 16-channel blocks per wave: 1 or 0 = 64-channel workgroups, two per CU (round 4: the faster form on every layer); 2 =
 * 128-channel workgroups, one per CU with the whole register file (needs Cout_pad % 128 == 0; round 3's form, kept for A/B runs).
 * Layers whose 64-channel workgroups would fill less than ~60 % of the 512 CU slots run "K-pair" workgroups (512 threads: the two
 * halves of the input channels side by side, accumulators traded through LDS at the end): m3d_wino44_kpair() says whether. */
int m3d_wino44_conv3x3_forward_ex(const m3d_conv_desc *d, int nb, m3d_stream_t stream);
int m3d_wino44_kpair(const m3d_conv_desc *d);
/* Split-K for maps whose 16-tile strips x 64-channel blocks do not fill the chip (512 -> 512 @ 12x40 at bs 8):
 * *splits slices of >= 64 input channels run as gridDim.z, raw partial outputs go to splitk_ws ([splits][N*H*W][Cout_pad]
 * fp32, *ws_bytes), a second launch adds them in slice order and applies the epilogue.  *splits = 1 / *ws_bytes = 0: no split.
 * m3d_wino44_conv3x3_forward and _ex with nb == 0 or nb == the split form (1 = 64-channel workgroups by default) split when the
 * descriptor carries a workspace of at least *ws_bytes; _ex with the other nb runs unsplit.  The split form and the fill
 * threshold are process-wide and read ONCE from the environment (M3D_W44_SPLIT_NB = 1 | 2, M3D_W44_SPLIT_FILL = workgroups a
 * layer must reach to run unsplit): size the workspace with m3d_wino44_splitk_plan in the process that launches, not from a
 * table computed under another setting. */
int m3d_wino44_splitk_plan(const m3d_conv_desc *d, int *splits, long long *ws_bytes);
/* Same as _ex, and every thread of the launch first touches a few 128-byte lines of [touch, touch + touch_bytes): the engine
 * passes the U tensor of the NEXT F(4x4) layer, which is then in the memory-side cache instead of HBM when that layer's B
 * fragments (four transform positions of lookahead) ask for it -- 256 -> 256 @ 24x80: 0.087 -> 0.063 ms in the network.
 * touch = NULL: none. */
int m3d_wino44_conv3x3_forward_touch(const m3d_conv_desc *d, int nb, const void *touch, long long touch_bytes, m3d_stream_t stream);

/* Touches one dword of every 128-byte line of [p, p + bytes): warms the memory-side cache with a weight tensor ahead of a
 * kernel whose operand lookahead does not cover an HBM round trip (the engine issues it before the F(4x4,3x3) layers). */
int m3d_cache_touch(const void *p, long long bytes, m3d_stream_t stream);
/* Fed-input upload as a kernel (replaces the per-frame im.cuda() of lib/rpn_util.py:1427-1429 for the pipelined detector):
 * copies `bytes` from the 16-byte-aligned pinned-host buffer whose address the 8-byte word *src_slot holds -- src_slot itself
 * lives in pinned host memory and is read when the kernel RUNS, so one captured graph serves a different frame set every replay
 * -- to dst (device, 16-byte aligned).  *src_slot == NULL: no copy. */
int m3d_upload_indirect(const void *const *src_slot, void *dst, long long bytes, m3d_stream_t stream);

/* Average launch geometry chosen for a descriptor (for roofline bookkeeping / tests). */
int m3d_conv2d_tile(const m3d_conv_desc *d, int *bm, int *bn, int *bk, int *grid);

/* ------------------------------------------------------------------------------------------
 * bf16 path (BASELINE.json configs[2]: bs = 64, bf16 storage, MFMA v_mfma_f32_32x32x16_bf16, fp32 accumulation).
 * Same operator as m3d_conv2d_forward -- conv (+ optional DCNv2 gather) + folded BatchNorm / bias + residual +
 * LeakyReLU / sigmoid in ONE launch -- on bf16 NHWC activations and bf16 weights packed [Cout_pad][Kpad],
 * K index = (i*kw + j)*Cin + c, zero padded to Kpad % 64 == 0 and Cout_pad % 32 == 0.  scale / shift / offsets / masks
 * stay fp32.  A kernel larger than 1x1 needs a power-of-two Cin; Cin % 8 == 0, in_cs % 8 == 0.
 * `groups` > 1 runs that many independent problems of identical geometry in one launch (the RPN heads that read the same
 * map): group g reads in + g*in_group_off, wgt + g*wgt_group_off, scale/shift + g*ss_group_off and writes
 * out + g*out_group_off (element units of the respective type).
 * ------------------------------------------------------------------------------------------ */
typedef struct m3d_conv_bf16_desc {
    const void *in;           /* bf16 NHWC view, pixel stride in_cs elements                                 */
    int in_cs;
    int N, H, W, Cin;
    const void *wgt;          /* bf16 [Cout_pad][Kpad]                                                       */
    long long wgt_img_stride; /* 0, or bf16 elements between per-image weight sets (needs Ho*Wo % 128 == 0)  */
    int Cout, Cout_pad, Kpad;
    int kh, kw, stride, pad;
    int Ho, Wo;
    void *out;
    int out_cs;               /* NHWC pixel stride in output elements (modes 0, 1)                           */
    int out_mode;             /* 0: bf16 NHWC   1: fp32 NHWC   2: fp32 planar out[n*out_img_stride + c*Ho*Wo + p] */
    long long out_img_stride;
    const float *scale;       /* [groups][Cout] or NULL (=1)                                                 */
    const float *shift;       /* [groups][Cout] or NULL (=0)                                                 */
    const void *res;          /* bf16 NHWC residual view or NULL                                             */
    int res_cs;
    int res_mode;             /* 0: acc*scale+shift+res   1: (acc+res)*scale+shift                           */
    int act;                  /* 0 none, 1 LeakyReLU(0.01)                                                   */
    int sigmoid_from;         /* channels >= this get sigmoid instead of act; <0: none                       */
    const float *dcn_offmask; /* fp32 NHWC [.., 3*kh*kw] (2k = dh, 2k+1 = dw, 2*kh*kw + k = mask); NULL = plain conv */
    int dcn_om_cs;
    int groups;
    long long in_group_off, wgt_group_off, out_group_off;
    int ss_group_off;
    /* Deformable 3x3 / stride 1 / pad 1 only, all three optional (NULL / 0 = implicit-GEMM kernel as before): an fp16 copy of
     * `wgt` (same [Cout_pad][Kpad] layout; bf16 -> fp16 is exact for |w| in [6.1e-5, 65504]) and m3d_conv_bf16_dcn_ws_bytes(N, Ho,
     * Wo) bytes of device scratch enable the LDS-patch kernel (csrc/bf16_dcn_patch.hip): every 16 x 16 (H % 16 == 0) or 8 x 16
     * (H % 8 == 0) pixel tile samples from an LDS-resident fp16 window sized to its own largest |offset| when that is <= 9 (<= 6)
     * and raises its word in dcn_ws otherwise; the implicit-GEMM kernel launched behind it recomputes the tiles that did
     * (W % 16 == 0, Cin % 32 == 0, Cout_pad % 128 == 0) -- decided on the device per tile, no host synchronisation.
     * Mixed rounding: a recomputing workgroup rewrites its whole 128-pixel tile, so which of the two kernels' roundings (fp16
     * window vs bf16 gather; both inside the bf16 tolerance) a pixel carries depends on the OFFSET DATA of its neighbourhood;
     * for given inputs the output is deterministic.  `res` must not alias `out` on this path (checked: M3D_E_ARG). */
    const void *wgt_f16;
    void *dcn_ws;
    long long dcn_ws_bytes;
    /* Plain 3x3 / stride 1 / pad 1, optional (NULL = halo-tile / implicit-GEMM kernels as before): the same weights in the
     * fragment order of csrc/bf16_conv_wide.hip -- [Cout_pad/128][Cin/32][9 taps][2 K-steps of 16][4 blocks of 32 channels]
     * [64 lanes][8] with lane = 32 * (k / 8) + (channel % 32) (m3dssd_amd/engine_bf16.py:PackedBf16.wave3x3) -- enable the
     * 128 x 128 wave-tile kernel on maps with H % 8 == 0, W % 16 == 0, Cin % 32 == 0, Cout_pad % 128 == 0, bf16 NHWC output. */
    const void *wgt_wave;
} m3d_conv_bf16_desc;
int m3d_conv_bf16_forward(const m3d_conv_bf16_desc *d, m3d_stream_t stream);
/* Bytes of dcn_ws the LDS-patch DCNv2 kernel needs for N x Ho x Wo output pixels (one flag word per pixel tile; 0 = the map does not tile). */
long long m3d_conv_bf16_dcn_ws_bytes(int N, int Ho, int Wo);
/* The kernel m3d_conv_bf16_forward launches for `d`, as m3d_conv_bf16_variant names it (profiling labels; no launch; -1 for a null
 * descriptor).  Tests and tools pin the numbers; 7 belonged to a retired kernel and stays unused. */
enum {
    M3D_BF16_CONV_IGEMM = 0,       /* implicit-GEMM tile (bf16_conv_kernel)                                                     */
    M3D_BF16_CONV_HALO16 = 1,      /* 3x3 halo tile of 8 x 16 pixels (bf16_conv3x3_halo_kernel)                                 */
    M3D_BF16_CONV_HALO32 = 2,      /* 3x3 halo tile of 8 x 32 pixels (bf16_conv3x3_halo_kernel)                                 */
    M3D_BF16_CONV_DCN_PATCH8 = 3,  /* deformable 3x3 with the sampling window in LDS, patches of 8 x 16 pixels ...               */
    M3D_BF16_CONV_DCN_PATCH16 = 4, /* ... of 16 x 16 pixels (bf16_dcn_patch_kernel); behind either, the implicit-GEMM kernel is  */
                                   /* launched and recomputes, on the device, the tiles whose offsets do not fit                */
    M3D_BF16_CONV_WIDE = 5,        /* 3x3 with 128 x 128 wave tiles (bf16_conv3x3_wide_kernel; needs wgt_wave)                  */
    M3D_BF16_CONV_DCN1X1 = 6,      /* deformable 1x1, 128 -> 128 channels, bf16 NHWC output (bf16_dcn1x1_kernel: center_align,  */
                                   /* feturealign_mgpu.py:48-99)                                                                */
    M3D_BF16_CONV_C64 = 8          /* 3x3 64 -> 64 channels on maps that tile 8 x 32 pixels, persistent workgroups with the     */
                                   /* weights resident in LDS (bf16_conv3x3_c64_kernel: DLA level2)                             */
};
int m3d_conv_bf16_variant(const m3d_conv_bf16_desc *d);

/* Entry of a DLA tree of the bf16 path in one launch (model/pose_dla_dcn.py:314-327, :107-121): bottom = MaxPool2d(2, 2)(x) (written
 * when `bottom` is not NULL), res = affine(Conv1x1(bottom)) (Tree.project), t = LeakyReLU(affine(Conv3x3 stride 2 pad 1 (x)))
 * (tree1.conv1) -- x is read once.  Cin % 32 == 0, Cout % 64 == 0, even H / W.  wfrag fp16 [Cout/32][Cin/32][10][2][64 lanes][8]:
 * slice ws, chunk c, tap t (0..8 = 3x3 taps row-major, 9 = the 1x1), block b, lane l (row r = l % 16, k-group l / 16), element e =
 * scale[ch] * W[ch][32 c + 8 (l / 16) + e][tap] with ch = 32 ws + 8 (r / 4) + 4 b + r % 4 (m3dssd_amd/engine_bf16.py:
 * pack_tree_entry); shift1 / shiftp fp32 [Cout]; all views bf16 NHWC with pixel strides in elements (% 8 == 0). */
typedef struct m3d_tree_entry_bf16_desc {
    const void *in;
    int in_cs, N, H, W, Cin, Cout;
    const void *wfrag;
    const float *shift1, *shiftp;
    void *t; int t_cs;
    void *res; int res_cs;
    void *bottom; int bottom_cs;
} m3d_tree_entry_bf16_desc;
int m3d_tree_entry_bf16_applicable(const m3d_tree_entry_bf16_desc *d);
int m3d_tree_entry_bf16_forward(const m3d_tree_entry_bf16_desc *d, m3d_stream_t stream);

/* Fused 3-layer RPN head of the bf16 path (model/M3d_inference_align.py:77-210): [1x1 128 -> 256, affine, LeakyReLU] ->
 * [1x1 256 -> 256, affine, LeakyReLU] -> [1x1 256 -> Cout, affine] per 128-pixel tile in ONE launch, hidden activations in LDS.
 * `groups` heads that read the same map share the launch: weights bf16 row-major [groups][256][128], [groups][256][256],
 * [groups][Cout_pad = 64][256]; scale / shift fp32 [groups][256], [groups][256], [groups][Cout]; output planar fp32
 * out[g*out_group_off + img*out_img_stride + c*HW + p]. */
typedef struct m3d_head_bf16_desc {
    const void *in;           /* bf16 [M][in_cs], first 128 channels used */
    int in_cs;
    long long M;
    int Cin;                  /* 128 */
    const void *w1, *w2, *w3;
    const float *s1, *t1, *s2, *t2, *s3, *t3;
    int Cout, Cout_pad;       /* Cout <= 64, Cout_pad == 64 */
    float *out;
    long long out_group_off, out_img_stride;
    int HW;
    int groups;
} m3d_head_bf16_desc;
int m3d_head_mlp_bf16_forward(const m3d_head_bf16_desc *d, m3d_stream_t stream);
/* Round-5 form of the fused head (csrc/bf16_head_mlp2.hip): the weights of layers 1 / 2 live in registers for the whole launch (wave w
 * of the 8-wave workgroup owns output channels [32w, 32w + 32)), hidden activations fp16 in LDS, layers 2 / 3 on fp16 MFMA.  The
 * caller folds the BatchNorm scales into the weights and packs them (m3dssd_amd/engine_bf16.py: pack_head2):
 *   w1f bf16 [groups][8 waves][8 K-steps][64 lanes][8], w2f fp16 [groups][8][16][64][8]: lane l of wave w, K-step s, element e =
 *       scale[ch] * W[ch][16 s + 8 (l / 32) + e] with ch = 32 w + 16 ((r % 8) / 4) + 4 (r / 8) + r % 4, r = l % 32;
 *   w3 fp16 [groups][64][256] row-major, scale folded, rows >= Cout zero; t1 / t2 [groups][256], t3 [groups][64] fp32 shifts.
 * Same input / output conventions as m3d_head_mlp_bf16_forward (128 input channels, Cout <= 64, planar fp32 output). */
typedef struct m3d_head2_bf16_desc {
    const void *in;           /* bf16 [M][in_cs], first 128 channels used */
    int in_cs;
    long long M;
    const void *w1f, *w2f, *w3;
    const float *t1, *t2, *t3;
    int Cout;
    float *out;
    long long out_group_off, out_img_stride;
    int HW;
    int groups;
} m3d_head2_bf16_desc;
int m3d_head_mlp2_bf16_forward(const m3d_head2_bf16_desc *d, m3d_stream_t stream);
/* Row-list form: the same heads -- all d->groups of the launch -- evaluated only at the *n_rows (device) pixels rows[j] =
 * img * HW + pix (ascending: what m3d_need_rows writes).  Tile t of the launch takes list entries [128 t, 128 t + 128), gathers
 * their input rows and scatters its planar stores per entry, so a tile may straddle images.  At the listed pixels the outputs are
 * bit-equal to m3d_head_mlp2_bf16_forward on the same descriptor; every other element of the output planes is left as it was.
 * Nothing is read back on the host (the grid is the dense launch's), and entries at or past *n_rows are never read.  A NULL row
 * list (rows or n_rows) is refused. */
int m3d_head_mlp2_bf16_forward_rows(const m3d_head2_bf16_desc *d, const int *rows, const int *n_rows, m3d_stream_t stream);
/* The two 1x1 layers behind the 3x3 convolution of the class head (M3d_inference_align.py:66-76: 256 -> 256 + affine + LeakyReLU,
 * 256 -> Cout <= 256 + affine) in one launch, same scheme: waf bf16 / wbf fp16 fragments [8 waves][16 K-steps][64 lanes][8] in the
 * layout of w2f above (scales folded, rows >= Cout of wbf zero), t1 / t2 fp32 [256] shifts (t2 past Cout ignored); input bf16
 * [M][in_cs >= 256]; output planar fp32 out[img * out_img_stride + c * HW + p]. */
typedef struct m3d_tail2_bf16_desc {
    const void *in;
    int in_cs;
    long long M;
    const void *waf, *wbf;
    const float *t1, *t2;
    int Cout;
    float *out;
    long long out_img_stride;
    int HW;
} m3d_tail2_bf16_desc;
int m3d_head_tail2_bf16_forward(const m3d_tail2_bf16_desc *d, m3d_stream_t stream);
/* The bias-free 1x1 projections of ANAB (model/module/attention.py:169-173, 183-200) over one 128-channel input in one launch:
 * wf bf16 fragments [16 row blocks][8 K-steps][64 lanes][8] (the layout of w1f above with the row blocks in the place of the waves)
 * of the stacked matrix [query rows padded with zeros to q_rows | key | value (kv_rows in all) | gates (s_rows) | zeros up to 512];
 * q bf16 [M][q_cs] gets all q_rows (the padding rows as zeros), kv bf16 [M][kv_cs], s fp32 [M][s_cs] = sigmoid(gates). */
typedef struct m3d_qkvs_bf16_desc {
    const void *in;
    int in_cs;
    long long M;
    const void *wf;
    void *q; int q_cs, q_rows;
    void *kv; int kv_cs, kv_rows;
    float *s; int s_cs, s_rows;
} m3d_qkvs_bf16_desc;
int m3d_anab_qkvs_bf16_forward(const m3d_qkvs_bf16_desc *d, m3d_stream_t stream);

/* HBM-bound helpers of the bf16 path: NHWC bf16 views (pixel strides in bf16 elements, multiples of 8), fp32 arithmetic.
 * m3d_stem_conv7x7_bf16: DLA.base_layer from the fp32 [N][3][H][W] image (is_u8 = 0; img_h/img_w/mean3/stds3 ignored) or
 * from uint8 BGR frames [N][img_h][img_w][3] with the reference's test-time Preprocess fused into the loads (is_u8 = 1,
 * mean3 / stds3 host pointers as in m3d_stem_conv7x7_u8); wgt [7*7*3][16] fp32. */
int m3d_stem_conv7x7_bf16(const void *img, int is_u8, int img_h, int img_w, const float *mean3, const float *stds3,
                          const float *wgt, const float *scale, const float *shift, void *out, int out_cs, int N, int H, int W,
                          m3d_stream_t stream);
/* Fused front end of the bf16 path (csrc/bf16_frontend2.hip): base_layer 7x7 3->16 -> level0 3x3 16->16 -> level1 3x3/2 16->32,
 * each + folded BN + LeakyReLU (pose_dla_dcn.py:336-345,391-397) in ONE launch: the image is read once, only the level1 map
 * [N][H/2][W/2][out_cs >= 32] bf16 is written.  img / is_u8 / img_h / img_w / mean3 / stds3 as in m3d_stem_conv7x7_bf16.  fp16 inside the kernel (the tiles never leave LDS), the
 * BatchNorm scales folded into fp16 weights by the caller, the shifts added as the C operand of the MFMA chains; stem on
 * v_mfma_f32_32x32x16_f16 with two adjacent output pixels per column.  Operands (m3dssd_amd/engine_bf16.py: pack_frontend_f16):
 *   w_stem_frag fp16 [7 tap rows][2 K-steps][64 lanes][8]: lane l, element e = weight * scale of channel 4 * ((l % 32) / 8) +
 *               (l % 4) [(l % 32) % 8 < 4: pixel shift 0, else 1], colour e % 4 (3 = zero), tap column 4 * kstep + 2 * (l / 32)
 *               + e / 4 - shift (outside [0, 7): zero); colour slot 3 of tap (0, 0) = the channel's BatchNorm shift (the kernel
 *               writes 1.0 into that slot of every image pixel; t_stem itself is not read);
 *   w_l0 / w_l1 fp16 [16 | 32][160], k = tap * 16 + c (k >= 144 zero), scale folded; t_* fp32 shifts [16], [16], [32].
 */
int m3d_frontend2_bf16_forward(const void *img, int is_u8, int img_h, int img_w, const float *mean3, const float *stds3,
                               const void *w_stem_frag, const float *t_stem, const void *w_l0, const float *t_l0,
                               const void *w_l1, const float *t_l1, void *out, int out_cs, int N, int H, int W,
                               m3d_stream_t stream);
/* ANAB attention of the bf16 path in one launch (model/module/attention.py:207-211 + the BatchNorm / LeakyReLU after the block):
 * out[p] = act((softmax_k(q[p] . khat[k]) @ vhat + res[p]) * scale + shift) per image, replacing the logits GEMM / row softmax /
 * P.V GEMM sequence (m3d_conv_bf16_forward with per-image weights, m3d_softmax_rows_bf16).  q bf16 [B*HW][q_cs] (channels
 * [Ck, Ck_pad) zero), khat bf16 [B][keys_pad][Ck_pad], vhatT bf16 [B][Cv][keys_pad] (rows >= keys ignored), res bf16 [B*HW][res_cs]
 * or NULL, scale / shift fp32 [Cv] or NULL, out bf16 [B*HW][out_cs].  Built for Ck_pad = 192, Cv = 128; HW % 128 == 0.
 * The padding -- khat rows [keys, keys_pad) and vhatT columns [keys, keys_pad) -- is ignored whatever it holds (NaN included): the
 * padded keys get probability 0 and their value columns are replaced by zeros when the last key tile is staged.  (The three-launch
 * form still multiplies the padding: m3d_anab_pool_nested* leave what the caller allocated, the engine allocates with zeros.)
 * The columns [Ck, Ck_pad) of the valid khat rows are operand (there is no Ck argument): finite, normally zero. */
int m3d_anab_attend_bf16(const void *q, int q_cs, const void *khat, const void *vhatT, int B, int HW, int Ck_pad, int keys,
                         int keys_pad, int Cv, const void *res, int res_cs, const float *scale, const float *shift, int act,
                         void *out, int out_cs, m3d_stream_t stream);
/* Row-list form, the contract of m3d_anab_attend_f32_rows: the same attention at the *n_rows (device) pixels rows[j] =
 * b * HW + pix only (ascending: what m3d_need_rows writes).  q, res and out are read / written at the listed pixels and nowhere
 * else, khat / vhatT are the whole images' as above, and the output is bit-equal to the dense call's there.  An image may list no
 * pixel, and entries at or past *n_rows are never read.  Built for the one-pass kernel: refused under M3D_ANAB_ONLINE=0. */
int m3d_anab_attend_bf16_rows(const void *q, int q_cs, const void *khat, const void *vhatT, int B, int HW, int Ck_pad, int keys,
                              int keys_pad, int Cv, const void *res, int res_cs, const float *scale, const float *shift, int act,
                              void *out, int out_cs, const int *rows, const int *n_rows, m3d_stream_t stream);
/* 2 x 2 max-pool, stride 2, odd H / W floored; H or W of 1 has no output element: M3D_OK, nothing launched (m3d_maxpool2x2 likewise). */
int m3d_maxpool2x2_bf16(const void *in, int in_cs, void *out, int out_cs, int N, int H, int W, int C, m3d_stream_t stream);
int m3d_upsample2x_add_bf16(const void *in, int in_cs, const float *wgt /*[4][4][C] fp32*/, const void *skip, int skip_cs,
                            void *out, int out_cs, int N, int H, int W, int C, m3d_stream_t stream);
int m3d_f32_to_bf16(const float *src, void *dst, long long n /* % 8 == 0 */, m3d_stream_t stream);
/* softmax over the first `valid` fp32 columns of each row (pixel stride cs) -> bf16 probabilities (row stride out_cs <= 512,
 * columns [valid, out_cs) zeroed): the P operand of the bf16 P.V GEMM of ANAB (attention.py:208-209). */
int m3d_softmax_rows_bf16(const float *x, int rows, int valid, int cs, void *out, int out_cs, m3d_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused RPN head (model/M3d_inference_align.py:77-210): per-pixel MLP
 *   [1x1 Cin->256 + affine + LeakyReLU] -> 1x1 256->256 + affine + LeakyReLU -> 1x1 256->Cout + affine
 * in ONE launch; hidden activations stay in LDS.  Cin = 128 or 256 with w1 given (3 layers; 256: the DLA-102 heads) or
 * Cin = 256 with w1 = NULL (2 layers: `in` is already the first hidden activation, e.g. after the 3x3 cls conv).
 * Weights are packed in MFMA-fragment order: element W[J*32 + r][G*8 + h*4 + t] (row-tile J, k-group G,
 * r < 32, h < 2, t < 4) at float index ((J*(K/8) + G)*64 + h*32 + r)*4 + t; rows zero-padded to 256 for
 * w1/w2 and to Cout_pad in {64, 256} for w3.  Output is planar: out[n*out_img_stride + c*HW + p].
 * ------------------------------------------------------------------------------------------ */
typedef struct m3d_mlp_desc {
    const float *in;          /* NHWC view [M][in_cs], first Cin channels used                     */
    int in_cs;
    long long M;              /* pixels = N*H*W                                                    */
    int Cin;
    const float *w1, *s1, *t1;
    const float *w2, *s2, *t2;
    const float *w3, *s3, *t3;
    int Cout, Cout_pad;
    float *out;
    long long out_img_stride;
    int HW;
} m3d_mlp_desc;
int m3d_head_mlp_forward(const m3d_mlp_desc *d, m3d_stream_t stream);
/* n (<= 16) independent heads of the same depth, M, Cin and Cout_pad in ONE launch (grid.y = head): the regression heads
 * that read the same aligned feature map (M3d_inference_align.py:139-176) have no mutual dependency. */
int m3d_head_mlp_forward_batched(const m3d_mlp_desc *d, int n, m3d_stream_t stream);
/* Row-list form of the batched launch (three-layer heads with Cout_pad = 64): head i with bit i of sparse_head_mask set is
 * evaluated only at the *n_rows (device) pixels rows[j] = n * HW + pix (what m3d_need_rows writes) -- tile t of the launch takes
 * rows [64t, 64t + 64) of the list -- and leaves every other element of its output planes as it is; at the listed pixels the
 * values are bit-equal to the dense launch.  Heads with a clear bit run as in m3d_head_mlp_forward_batched.  Nothing is read
 * back: the grid is sized for the dense M and the tiles past the list return at once. */
int m3d_head_mlp_forward_rows(const m3d_mlp_desc *d, int n, const int *rows, const int *n_rows, unsigned int sparse_head_mask,
                              m3d_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Drop-in for dcn_v2_cuda_forward: NCHW contiguous fp32 device tensors, exactly the reference
 * argument meaning.  `workspace` replaces the reference's `ones`/`columns` scratch tensors
 * (dcn_v2_func.py:28): the caller allocates m3d_dcn_v2_workspace_bytes() bytes.
 * deformable_group = G > 1 (model/DCNv2/test.py:169-179; the M3DSSD path itself uses 1): G must divide `channels`;
 * offset is [N, G*2*kh*kw, Ho, Wo], mask [N, G*kh*kw, Ho, Wo] (dcn_v2_im2col_cuda.cu:139-156); the workspace then comes
 * from m3d_dcn_v2_workspace_bytes_grouped (returns -1 for an invalid G).
 * ------------------------------------------------------------------------------------------ */
long long m3d_dcn_v2_workspace_bytes(int batch, int channels, int height, int width, int channels_out,
                                     int kernel_h, int kernel_w, int stride, int pad, int dilation);
long long m3d_dcn_v2_workspace_bytes_grouped(int batch, int channels, int height, int width, int channels_out,
                                             int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                             int deformable_group);
int m3d_dcn_v2_forward(const float *input, const float *weight, const float *bias, const float *offset,
                       const float *mask, float *output, int batch, int channels, int height, int width,
                       int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h,
                       int pad_w, int dilation_h, int dilation_w, int deformable_group, void *workspace,
                       long long workspace_bytes, m3d_stream_t stream);

/* Drop-in for dcn_v2_cuda_backward (csrc/dcn_op.hip): NCHW contiguous fp32 device tensors, the reference's argument
 * meaning with `ones` / `columns` replaced by the caller's workspace of m3d_dcn_v2_backward_workspace_bytes() bytes (-1 for an
 * invalid group count; the size does not depend on which gradients are asked for).  Given grad_output [N, Co, Ho, Wo] it
 * produces grad_input [N, C, H, W], grad_offset [N, G*2*kh*kw, Ho, Wo], grad_mask [N, G*kh*kw, Ho, Wo], grad_weight
 * [Co, C, kh, kw] and grad_bias [Co]: the analytic derivative of m3d_dcn_v2_forward as it is defined (a sample contributes iff
 * h_im > -1, w_im > -1, h_im < H, w_im < W, a corner iff it lies inside the image, hl = floor(h_im); a NaN / inf coordinate is
 * outside and has zero gradients).  Two differences from the reference:
 *   - every non-NULL gradient is OVERWRITTEN (the reference accumulates into grad_weight / grad_bias and adds into a
 *     grad_input its caller has zeroed, dcn_v2_func.py:44-48);
 *   - any of the five gradient pointers may be NULL = not wanted (autograd's needs_input_grad); the work only it needs is skipped.
 * grad_offset, grad_mask, grad_weight and grad_bias are bitwise reproducible from run to run; grad_input is accumulated with
 * float atomics, as in the reference (dcn_v2_im2col_cuda.cu:234), and may differ in its last bits between runs.
 * Same restrictions and errors as the forward (stride_h == stride_w etc.; M3D_E_ARG / M3D_E_WORKSPACE with both sizes). */
long long m3d_dcn_v2_backward_workspace_bytes(int batch, int channels, int height, int width, int channels_out,
                                              int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                              int deformable_group);
int m3d_dcn_v2_backward(const float *input, const float *weight, const float *offset, const float *mask,
                        const float *grad_output,
                        float *grad_input, float *grad_offset, float *grad_mask, float *grad_weight, float *grad_bias,
                        int batch, int channels, int height, int width, int channels_out, int kernel_h, int kernel_w,
                        int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w,
                        int deformable_group, void *workspace, long long workspace_bytes, m3d_stream_t stream);

/* The same operator on bf16 tensors (csrc/dcn_op.hip): what a training loop under torch.autocast(dtype=bfloat16) hands over.
 * input [N, C, H, W], weight [Co, C, kh, kw], grad_output / output [N, Co, Ho, Wo] and grad_input are bf16 NCHW contiguous, bias
 * and grad_bias fp32; offset and mask are fp32 (`*_is_bf16` = 0) or bf16 (1), widened exactly and used as fp32; grad_offset and
 * grad_mask are written as fp32, grad_weight as bf16 (the type of the weight it belongs to).  Coordinates, the inside rule, floor
 * and the corner weights are those of the fp32 calls (fp32 arithmetic, the same piecewise rule).  Rounding points: the modulated
 * sample mask * val -> bf16 once (the MFMA operand), products exact, fp32 accumulation, bias added in fp32, output -> bf16 once;
 * backward: gcol fp32, col = mask * val bf16, grad_input accumulated in fp32 with float atomics and rounded to bf16 once,
 * grad_weight rounded once after the split-order sum.  Semantics of the backward as m3d_dcn_v2_backward: every non-NULL gradient
 * is overwritten, NULL = not wanted, grad_offset / grad_mask / grad_weight / grad_bias bitwise reproducible.
 * Any C / Co (padded inside, nothing written past the tensors), deformable_group >= 1 dividing C, stride 1 or 2, kernels up to 3x3.
 * dilation must be 1: the bf16 convolution has none -- M3D_E_ARG "the bf16 path supports dilation 1 only", and the size queries
 * return -1 for it as for an invalid group count.  The workspace size does not depend on which gradients are asked for;
 * M3D_E_WORKSPACE carries both sizes. */
long long m3d_dcn_v2_workspace_bytes_bf16(int batch, int channels, int height, int width, int channels_out,
                                          int kernel_h, int kernel_w, int stride, int pad, int dilation, int deformable_group);
int m3d_dcn_v2_forward_bf16(const void *input, const void *weight, const float *bias, const void *offset, int offset_is_bf16,
                            const void *mask, int mask_is_bf16, void *output, int batch, int channels, int height, int width,
                            int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                            int dilation_h, int dilation_w, int deformable_group, void *workspace, long long workspace_bytes,
                            m3d_stream_t stream);
long long m3d_dcn_v2_backward_workspace_bytes_bf16(int batch, int channels, int height, int width, int channels_out,
                                                   int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                                   int deformable_group);
int m3d_dcn_v2_backward_bf16(const void *input, const void *weight, const void *offset, int offset_is_bf16, const void *mask,
                             int mask_is_bf16, const void *grad_output,
                             void *grad_input, float *grad_offset, float *grad_mask, void *grad_weight, float *grad_bias,
                             int batch, int channels, int height, int width, int channels_out, int kernel_h, int kernel_w,
                             int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w,
                             int deformable_group, void *workspace, long long workspace_bytes, m3d_stream_t stream);

/* The two backward calls with a bitwise-reproducible grad_input (csrc/dcn_op.hip): the argument lists, restrictions, error codes
 * and messages of m3d_dcn_v2_backward / m3d_dcn_v2_backward_bf16, a workspace of m3d_dcn_v2_backward_det_workspace_bytes[_bf16]()
 * bytes (never smaller than the float form's: the staging buffer of grad_input doubles; -1 where the float queries return -1).
 * grad_offset, grad_mask, grad_weight and grad_bias take the same path and have the bits of the float form.  grad_input is a
 * function of the inputs alone: the same bits on every launch, and for an image alone or inside any batch.
 *   - Every contribution gcol * mask * w_q is the fp32 value the float form adds.  It is scaled by 2^s_n (exact), rounded to the
 *     nearest integer and added into a 64-bit integer sum (integer atomics: addition is associative); the finished sum is
 *     converted to fp32 (round to nearest), scaled by 2^-s_n (exact) and, for bf16, rounded once more to bf16.
 *   - s_n is chosen per image n and deformable group from order-independent maxima: A_n = max |grad_output[n]|, W_g = max over
 *     (channel of the group, tap) of sum_co |weight[co][c][tap]|, M_n = max |mask[n, group]|.  With 2^E > 2 A_n W_g M_n (one spare
 *     bit for the rounding of the GEMM) and T = Ho*Wo*kh*kw contributions at most per element, s_n = 62 - E - ceil(log2 T): no
 *     input can overflow the sum (DESIGN.md has the argument).  Resolution: 2^-s_n = 2^(E + ceil(log2 T) - 62), 45 bits below 2^E
 *     on a 48x160 map with a 3x3 kernel.
 *   - Differences from the float form: if A_n, W_g or M_n is not finite (a NaN or infinity in grad_output[n], the weights or the
 *     masks of image n), or their product reaches 2^126, grad_input of image n (that group's channels) is all NaN; if the product
 *     is zero that grad_input is zero.  Non-finite offsets are treated as in the float form (outside, zero gradients). */
long long m3d_dcn_v2_backward_det_workspace_bytes(int batch, int channels, int height, int width, int channels_out,
                                                  int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                                  int deformable_group);
int m3d_dcn_v2_backward_det(const float *input, const float *weight, const float *offset, const float *mask,
                            const float *grad_output,
                            float *grad_input, float *grad_offset, float *grad_mask, float *grad_weight, float *grad_bias,
                            int batch, int channels, int height, int width, int channels_out, int kernel_h, int kernel_w,
                            int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w,
                            int deformable_group, void *workspace, long long workspace_bytes, m3d_stream_t stream);
long long m3d_dcn_v2_backward_det_workspace_bytes_bf16(int batch, int channels, int height, int width, int channels_out,
                                                       int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                                       int deformable_group);
int m3d_dcn_v2_backward_det_bf16(const void *input, const void *weight, const void *offset, int offset_is_bf16, const void *mask,
                                 int mask_is_bf16, const void *grad_output,
                                 void *grad_input, float *grad_offset, float *grad_mask, void *grad_weight, float *grad_bias,
                                 int batch, int channels, int height, int width, int channels_out, int kernel_h, int kernel_w,
                                 int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w,
                                 int deformable_group, void *workspace, long long workspace_bytes, m3d_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Deformable position-sensitive RoI pooling (csrc/psroi_pool.hip): the drop-ins for dcn_v2_psroi_pooling_cuda_forward /
 * _backward, the operator behind DCNv2PoolingFunction (model/DCNv2/dcn_v2_func.py:76-146).  fp32 contiguous device tensors:
 *   data  [batch, channels, height, width];  rois [num_rois, 5] = (batch index, x1, y1, x2, y2) in image pixels;
 *   trans [trans_rows >= num_rois, 2 * num_classes, part_size, part_size], ignored (may be NULL) when no_trans;
 *   out, top_count [num_rois, output_dim, pooled_size, pooled_size]; top_count may be NULL.
 * With P = pooled_size, S = sample_per_part, G = group_size, D = output_dim: K = 1 when no_trans, else num_classes;
 * channels_each_class = D / K.  For output (i, c, ph, pw) every value below is fp32 and every operation is rounded once, in
 * this order, with no fused multiply-add:
 *   rs_w = roundf(x1) * spatial_scale - 0.5 (roundf: halves away from zero), re_w = (roundf(x2) + 1) * spatial_scale - 0.5,
 *   rs_h / re_h likewise from y1 / y2;  roi_w = max(re_w - rs_w, 0.1), roi_h likewise;
 *   bin_w = roi_w / P, sub_w = bin_w / S (IEEE divisions), the same for h;
 *   part_w = floorf((float)pw / P * part_size), part_h = floorf((float)ph / P * part_size)   (float32, not (pw * part) / P);
 *   gw = clamp(floorf((float)pw * G / P), 0, G - 1), gh likewise;  class = c / channels_each_class;
 *   tx = trans[i, 2 * class, part_h, part_w] * trans_std, ty = trans[i, 2 * class + 1, part_h, part_w] * trans_std (0 if no_trans);
 *   wstart = (pw * bin_w + rs_w) + tx * roi_w, hstart = (ph * bin_h + rs_h) + ty * roi_h;
 *   sample (ih, iw), 0 <= ih, iw < S: w = wstart + iw * sub_w, h = hstart + ih * sub_h;  input channel (c * G + gh) * G + gw.
 * A sample counts iff both coordinates are finite, -0.5 <= w <= width - 0.5 and -0.5 <= h <= height - 0.5.  A counted sample is
 * clamped to [0, width - 1] x [0, height - 1] and read bilinearly between floor and ceil of each coordinate with weight
 * w - floor(w) on the ceil side (at an integer coordinate both corners coincide).  top_count = the number of counted samples;
 * out = their sum divided by top_count (one fp32 division), 0 when top_count is 0.
 * Backward, given grad_out: grad_data receives, per counted sample, grad_out / count times the four corner weights at the four
 * corners; grad_trans[i, 2 * class (+1), part_h, part_w] receives, per counted sample, trans_std * roi_w * grad_out / count *
 * d val / d w (the y element: roi_h and d / d h), the bilinear slope between the floor and ceil columns, 0 at an integer or clamped
 * coordinate.  The count is recomputed, not taken from the caller.  rois get no gradient; rows of trans past num_rois get zeros.
 * Where this library is stricter than the reference (which dereferences without looking):
 *   - a region whose batch index is not an integer in [0, batch), or with a non-finite corner, gives zeros, count 0 and no
 *     gradient; nothing is read or written for it beyond its own output rows;
 *   - channels < D * G * G, D not divisible by K, trans_rows < num_rois, P / S / G / part_size < 1 and trans_std outside [0, 1]
 *     are M3D_E_ARG; no input can make a kernel address memory outside its tensors;
 *   - every non-NULL gradient is OVERWRITTEN (the reference adds into tensors its caller has zeroed); a NULL gradient pointer =
 *     not wanted, and the work only it needs is skipped; with no_trans grad_trans is ignored;
 *   - grad_trans is bitwise reproducible from run to run (butterfly over the lanes, then a fixed order over the bins of a part
 *     cell; no atomics); grad_data is summed with float atomics, as in the reference, and may differ in its last bits.
 * The workspace (256-byte aligned) holds a pixel-major copy of the first D * G * G channels of data and, for the backward
 * (`backward` != 0 in the query), the fp32 staging buffer of grad_data and the per-wave partials of grad_trans; no result
 * depends on what it held.  The query returns -1 for invalid sizes; num_classes = 1 for no_trans.  M3D_E_WORKSPACE carries both
 * sizes.  num_rois = 0 returns M3D_OK without a kernel launch (the backward then zero-fills the gradients asked for).
 * ------------------------------------------------------------------------------------------ */
long long m3d_dcn_v2_psroi_pooling_workspace_bytes(int batch, int channels, int height, int width, int num_rois,
                                                   int num_classes, int output_dim, int group_size, int pooled_size,
                                                   int backward);
int m3d_dcn_v2_psroi_pooling_forward(const float *data, const float *rois, const float *trans, float *out, float *top_count,
                                     int batch, int channels, int height, int width, int num_rois, int trans_rows,
                                     int num_classes, int no_trans, float spatial_scale, int output_dim, int group_size,
                                     int pooled_size, int part_size, int sample_per_part, float trans_std, void *workspace,
                                     long long workspace_bytes, m3d_stream_t stream);
int m3d_dcn_v2_psroi_pooling_backward(const float *grad_out, const float *data, const float *rois, const float *trans,
                                      float *grad_data, float *grad_trans, int batch, int channels, int height, int width,
                                      int num_rois, int trans_rows, int num_classes, int no_trans, float spatial_scale,
                                      int output_dim, int group_size, int pooled_size, int part_size, int sample_per_part,
                                      float trans_std, void *workspace, long long workspace_bytes, m3d_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * RPN_3D_loss on the device (csrc/rpn_loss.hip): target assignment, hard-negative sampling, fused loss + gradients.
 * Row r of an image is anchor (a, h, w), r = (a*H + h)*W + w, R = A*H*W rows (locate_anchors' order); cls / prob are
 * [B, R, C], bbox_2d [B, R, 4], bbox_3d [B, R, 7], contiguous float32 device tensors.
 *   anchors   device, float64 [A, 9]: x1 y1 x2 y2 z w h l ry (conf.anchors widened).
 *   conf      HOST, float64 [M3D_RPN_CONF_COUNT], indices below.  box_samples may be +inf; fg_fraction NaN = None (only with
 *             box_samples = inf, as in the reference).
 *   gt_table  device, float64 [B, Gmax + 1, M3D_RPN_GT_COLS] -- the one upload of a call.  Row 0 of an image: n_valid, n_ignore.
 *             Rows 1 .. n_valid: x1 y1 x2 y2 (corners), class label (1 .. C-1), then bbox_3d[0:7] = cx cy z w h l ry.  The next
 *             n_ignore rows: x1 y1 x2 y2 of the ignore regions.  n_valid + n_ignore <= Gmax <= M3D_RPN_MAX_GT; a larger Gmax is
 *             M3D_E_ARG (nothing is truncated).  An image with n_valid = 0 contributes nothing (label 0 everywhere).
 * m3d_rpn_targets writes, per row: labels (int16: class for fg, 0 for bg, 3000 for ignored), gt_index (int16: the valid gt a fg
 * row regresses to, -1 otherwise), targets (float32 [B, R, 11]: the normalised 2-D (4) and 3-D (7) transforms; (0 - mean) / std
 * where the row is not fg), scores (float32: prob[label], the key of the sampling), and leaves the per-image counts in the
 * workspace.  m3d_rpn_loss must get the SAME workspace, untouched, and the same labels / targets / scores; it writes sampled
 * (uint8: 0 no, 1 fg, 2 bg), the gradients of `loss` with respect to cls, bbox_2d and bbox_3d (zero for unsampled rows), the
 * float32 loss and the float64 stat block (indices below).  Among equal scores the lower row is sampled first.  A sampled fg
 * whose decoded box misses its target gives loss = +inf like the reference and a ZERO IoU-term gradient for that row (the
 * reference's is NaN).  Everything is bitwise reproducible from run to run; nothing is copied to the host.
 * ------------------------------------------------------------------------------------------ */
#define M3D_RPN_MAX_GT 128
#define M3D_RPN_GT_COLS 12
enum {
    M3D_RPN_CONF_MEANS = 0,        /* 11 */
    M3D_RPN_CONF_STDS = 11,        /* 11 */
    M3D_RPN_CONF_FG_THRESH = 22,
    M3D_RPN_CONF_IGN_THRESH = 23,
    M3D_RPN_CONF_BG_LO = 24,
    M3D_RPN_CONF_BG_HI = 25,
    M3D_RPN_CONF_BEST_THRESH = 26,
    M3D_RPN_CONF_BOX_SAMPLES = 27,
    M3D_RPN_CONF_FG_FRACTION = 28,
    M3D_RPN_CONF_FOCAL = 29,
    M3D_RPN_CONF_LAMBDA_CLS = 30,
    M3D_RPN_CONF_LAMBDA_IOU = 31,
    M3D_RPN_CONF_LAMBDA_2D = 32,
    M3D_RPN_CONF_LAMBDA_3D = 33,
    M3D_RPN_CONF_STRIDE = 34,
    M3D_RPN_CONF_COUNT = 35
};
enum {
    M3D_RPN_STAT_LOSS = 0,
    M3D_RPN_STAT_CLS = 1,
    M3D_RPN_STAT_BBOX_2D = 2,
    M3D_RPN_STAT_BBOX_3D = 3,
    M3D_RPN_STAT_IOU_LOSS = 4,
    M3D_RPN_STAT_Z = 5,
    M3D_RPN_STAT_RY = 6,
    M3D_RPN_STAT_IOU_ACC = 7,
    M3D_RPN_STAT_ACC_FG = 8,
    M3D_RPN_STAT_ACC_BG = 9,
    M3D_RPN_STAT_N_FG = 10,       /* fg / bg rows of the batch (all, not only the sampled) */
    M3D_RPN_STAT_N_BG = 11,
    M3D_RPN_STAT_FG_NUM = 12,     /* sampled fg / bg rows of the batch */
    M3D_RPN_STAT_BG_NUM = 13,
    M3D_RPN_STAT_N_ACTIVE = 14,   /* rows in the mean of the classification loss */
    M3D_RPN_STAT_FG_WEIGHT = 15,
    M3D_RPN_STAT_COUNT = 16
};
long long m3d_rpn_loss_workspace_bytes(int B, long long R);
int m3d_rpn_targets(const double *anchors, int A, int H, int W, const double *conf, int n_conf, const double *gt_table, int B,
                    int Gmax, const float *cls, const float *prob, int C, short *labels, short *gt_index, float *targets,
                    float *scores, void *workspace, long long workspace_bytes, m3d_stream_t stream);
int m3d_rpn_loss(const double *anchors, int A, int H, int W, const double *conf, int n_conf, const double *gt_table, int B,
                 int Gmax, const float *cls, const float *bbox_2d, const float *bbox_3d, int C, const short *labels,
                 const float *targets, const float *scores, unsigned char *sampled, float *grad_cls, float *grad_bbox_2d,
                 float *grad_bbox_3d, float *loss, double *stats, void *workspace, long long workspace_bytes,
                 m3d_stream_t stream);

/* RPN_3D_loss_smp on the device (lib/loss/rpn_3d.py:659-1360): the same loss over targets that were assigned ahead of the
 * forward, by the data loader (Kitti_Dataset_torch._targets, lib/dataloader.py:1014-1160) or by m3d_rpn_precompute_targets.
 *
 * m3d_rpn_precompute_targets is m3d_rpn_targets without cls / prob (launches 1-3, no scores, no accuracy counts): labels and
 * gt_index as there, the targets in the loader's layout -- bbox_2d_tar float32 [B, R, 4] and bbox_3d_tar float32 [B, R, 7], the
 * same bits as columns 0-3 and 4-10 of m3d_rpn_targets' `targets` ((0 - mean) / std where a row is not fg, 0 in an image
 * without a valid gt) -- and any_val int32 [B]: 1 where the image has a valid gt.
 *
 * m3d_rpn_loss_smp has no gt table.  labels_in is device [B, R], int64 (label_bytes = 8: what the loader collates) or int16
 * (label_bytes = 2: what m3d_rpn_targets / m3d_rpn_precompute_targets write), each 0 (bg), 1 .. C-1 (fg) or 3000 (ignored);
 * any other value is counted in stats[M3D_RPN_SMP_STAT_BAD_LABELS] and the row treated as ignored.  bbox_2d_tar / bbox_3d_tar /
 * any_val as above, on the device.  One ingest launch writes labels (int16), targets (float32 [B, R, 11], packed) and scores
 * (prob[label]; 0 for an ignored row and in an image with any_val = 0) -- caller buffers like those of m3d_rpn_targets -- and
 * leaves the per-image counts in the workspace; launches 4-6 of m3d_rpn_loss follow unchanged.  An image with any_val = 0
 * selects nothing; its labels still enter the fg / bg accuracy.  Outputs as m3d_rpn_loss; `stats` holds
 * M3D_RPN_SMP_STAT_COUNT doubles.  Fed the labels and targets m3d_rpn_targets wrote, every output equals m3d_rpn_loss' bit for
 * bit.  Workspace: m3d_rpn_loss_workspace_bytes(B, R), contents irrelevant on entry. */
enum {
    M3D_RPN_SMP_STAT_BAD_LABELS = 16,   /* after the M3D_RPN_STAT_* slots */
    M3D_RPN_SMP_STAT_COUNT = 17
};
int m3d_rpn_precompute_targets(const double *anchors, int A, int H, int W, const double *conf, int n_conf,
                               const double *gt_table, int B, int Gmax, short *labels, short *gt_index, float *bbox_2d_tar,
                               float *bbox_3d_tar, int *any_val, void *workspace, long long workspace_bytes,
                               m3d_stream_t stream);
int m3d_rpn_loss_smp(const double *anchors, int A, int H, int W, const double *conf, int n_conf, int B, const void *labels_in,
                     int label_bytes, const float *bbox_2d_tar, const float *bbox_3d_tar, const int *any_val, const float *cls,
                     const float *prob, const float *bbox_2d, const float *bbox_3d, int C, short *labels, float *targets,
                     float *scores, unsigned char *sampled, float *grad_cls, float *grad_bbox_2d, float *grad_bbox_3d,
                     float *loss, double *stats, void *workspace, long long workspace_bytes, m3d_stream_t stream);

/* The reduction compute_bbox_stats (lib/rpn_util.py:732-889) makes of compute_targets, per image on the device: launches 1-3 of
 * m3d_rpn_targets with the reducing form of launch 3, then one finish launch.  anchors, gt_table, Gmax and the thresholds and
 * stride of `conf` as for m3d_rpn_precompute_targets; the means, stds and loss settings of `conf` are NOT read (nor checked).
 * Unlike the loss path, the anchor boxes stay FLOAT64 here through the overlaps and the transforms, as the reference's
 * compute_bbox_stats has them (it does not cast locate_anchors' result; the loss does).
 *   center  device, float64 [11]: subtracted from every transform (zeros for the pass that finds the means, the means for the
 *           pass that finds the stds).
 *   out     device, float64 [B, M3D_RPN_TARGET_STATS_COLS]; per image over its fg rows: n_fg, then sum(t32 - center) for the 11
 *           columns (2-D dx dy dw dh, 3-D x y z w h l ry), then sum((t32 - center)^2) for the 11 columns.  t32 is the raw
 *           transform (mean 0, std 1) rounded to float32 like the reference's array; differences, squares and sums are float64.
 *           An image with n_valid = 0 gives a zero row.
 * No float atomics, fixed summation order: an image's row holds the same bits whatever batch, batch slot or workspace contents
 * it is computed with.  Workspace: m3d_rpn_target_stats_workspace_bytes(B, R), contents irrelevant on entry. */
#define M3D_RPN_TARGET_STATS_COLS 23
long long m3d_rpn_target_stats_workspace_bytes(int B, long long R);
int m3d_rpn_target_stats(const double *anchors, int A, int H, int W, const double *conf, int n_conf, const double *gt_table, int B,
                         int Gmax, const double *center, double *out, void *workspace, long long workspace_bytes,
                         m3d_stream_t stream);

/* The optimizer step on the device (csrc/optim.hip): torch.optim.SGD(lr, momentum, weight_decay), Adam(lr, weight_decay) and
 * Adamax(lr, weight_decay) as lib/core.py:76-99 builds them, over a whole float32 parameter set, and the decision of
 * scripts/train_rpn_3d.py:208-218 (`if total_loss > 0`) without the host.  kind: 0 SGD, 1 Adam, 2 Adamax.
 *   table    device, n_entries records of M3D_OPTIM_ENTRY_BYTES: { float *p, *g, *s0, *s1; long long numel; int group, pad; }.
 *            s0 = momentum_buffer (null: the group's momentum is 0) / exp_avg, s1 = exp_avg_sq / exp_inf (null for SGD); all float32,
 *            contiguous, `numel` elements, 4-byte aligned (16-byte aligned tensors are accessed 16 bytes at a time); group <
 *            n_groups.  The CONTENTS of the table are the caller's responsibility: the library cannot read them on the host.
 *   chunks   device, n_chunks records { int entry, index; }: elements [index * M3D_OPTIM_CHUNK, min(numel, (index + 1) *
 *            M3D_OPTIM_CHUNK)) of table[entry].  Every element of every tensor in exactly one chunk; one workgroup per chunk.
 *   hyper    HOST, float64 [n_groups][M3D_OPTIM_HYPER_COLS]: lr, momentum, weight_decay, beta1, beta2, eps.  They travel as kernel
 *            arguments (no upload); each float32 scalar of the update is the float64 expression rounded once (e.g. 1 - beta1).
 *   state    device, m3d_optim_state_bytes(n_chunks) bytes, 16-byte aligned: a head of M3D_OPTIM_STATE_HEAD_BYTES (fields at the
 *            M3D_OPTIM_STATE_* byte offsets) followed by the per-chunk partials.  The caller zeroes it once and sets the 2 x 8
 *            running products to 1.0; afterwards it belongs to these calls (t, products) and may be read at any time.
 * m3d_optim_prepare: grad_sq_sum = sum g*g over the table (float64; fixed order: per chunk in thread order and a fixed tree, then
 * the chunk partials in chunk order, 256 consecutive runs combined by the same tree; no atomics: the same bits on every launch),
 * grad_nonfinite = the number of inf / NaN gradient elements, do_step = (loss == null || *loss > 0) && (!skip_nonfinite ||
 * grad_nonfinite == 0) -- `loss` is a device float32 scalar; NaN gives no step.  When do_step: t += 1, prod1[g] *= beta1,
 * prod2[g] *= beta2 (float64), bc1 = 1 - prod1, bc2_sqrt = sqrt(1 - prod2), step_size = lr / bc1, rounded to float32 once (Adam,
 * Adamax).  Otherwise t, the products and the derived scalars keep their bits.
 * m3d_optim_step: nothing is written when do_step is clear.  Otherwise p and the state tensors are updated in place by the
 * arithmetic stated at the top of csrc/optim.hip (one correctly rounded float32 operation at a time, no FMA; tests/optim_ref.py is
 * the same in numpy), and with zero_grads != 0 every g is overwritten with zeros in the same pass.  Must follow a prepare on the
 * same stream with the same table, kind and hyper.
 * Errors (M3D_E_ARG, nothing launched): a null table / chunks / hyper / state, negative sizes, kind outside 0 .. 2, n_groups
 * outside 1 .. M3D_OPTIM_MAX_GROUPS, a non-finite or negative setting, betas outside [0, 1), a state block below
 * m3d_optim_state_bytes (the message carries both sizes).  m3d_optim_state_bytes returns -1 for n_chunks < 0. */
#define M3D_OPTIM_CHUNK 4096
#define M3D_OPTIM_MAX_GROUPS 8
#define M3D_OPTIM_ENTRY_BYTES 48
#define M3D_OPTIM_HYPER_COLS 6
enum {
    M3D_OPTIM_STATE_GRAD_SQ_SUM = 0, /* double */
    M3D_OPTIM_STATE_NONFINITE = 8,   /* long long */
    M3D_OPTIM_STATE_DO_STEP = 16,    /* int */
    M3D_OPTIM_STATE_T = 24,          /* long long: taken steps */
    M3D_OPTIM_STATE_PROD1 = 32,      /* double [M3D_OPTIM_MAX_GROUPS]: beta1^t */
    M3D_OPTIM_STATE_PROD2 = 96,      /* double [M3D_OPTIM_MAX_GROUPS]: beta2^t */
    M3D_OPTIM_STATE_BC1 = 160,       /* float [M3D_OPTIM_MAX_GROUPS] */
    M3D_OPTIM_STATE_BC2_SQRT = 192,  /* float [M3D_OPTIM_MAX_GROUPS] */
    M3D_OPTIM_STATE_STEP_SIZE = 224, /* float [M3D_OPTIM_MAX_GROUPS]: lr / bc1 */
    M3D_OPTIM_STATE_HEAD_BYTES = 256
};
long long m3d_optim_state_bytes(int n_chunks);
int m3d_optim_prepare(const void *table, int n_entries, const void *chunks, int n_chunks, int kind, const double *hyper,
                      int n_groups, const float *loss, int skip_nonfinite, void *state, long long state_bytes,
                      m3d_stream_t stream);
int m3d_optim_step(const void *table, int n_entries, const void *chunks, int n_chunks, int kind, const double *hyper, int n_groups,
                   int zero_grads, void *state, long long state_bytes, m3d_stream_t stream);

/* BatchNorm2d with BATCH statistics + optional residual add + activation, for TRAINING (csrc/bn_train.hip): the chain behind every
 * convolution of the training forward (model/pose_dla_dcn.py:107-121,261-269,379-389,482-485, M3d_inference_align.py:66-210) as one
 * operator.  fp32, NCHW, contiguous: x, residual, y and the gradients [B, C, H, W]; gamma, beta, the running statistics, save_mean,
 * save_invstd, grad_gamma, grad_beta [C]; N = B*H*W values per channel.  slope in [0, 1]: 0 = ReLU, a LeakyReLU's negative_slope,
 * 1 = no activation.
 *   forward   mean = sum(x) / N,   var = max(sum(x^2) / N - mean^2, 0)  (biased),   invstd = 1 / sqrt(var + eps)
 *             z = (x - mean) * invstd * gamma + beta (+ residual),   y = z > 0 ? z : slope * z
 *             running_mean = (1 - momentum) * running_mean + momentum * mean
 *             running_var  = (1 - momentum) * running_var  + momentum * var * N / (N - 1)          (either may be NULL: not kept)
 *             save_mean = mean, save_invstd = invstd, rounded once to float32: what the backward takes
 *   backward  dz = grad_y * (y > 0 ? 1 : slope)   (the mask is taken from the saved OUTPUT y),   grad_residual = dz,
 *             grad_beta = sum(dz),   grad_gamma = sum(dz * xhat) with xhat = (x - save_mean) * save_invstd,
 *             grad_x = gamma * save_invstd * (dz - grad_beta / N - xhat * grad_gamma / N)
 * Structure: a channel's N positions n = b * H*W + p are cut into m3d_bn_act_train_chunks(B, C, H, W) chunks of 4096 (the last one
 * shorter), one workgroup per (channel, chunk).  Each direction is two launches: the first writes the two sums of every (channel,
 * chunk) into the workspace, every workgroup of the second adds the partials of its channel in a fixed order and applies.  The four
 * sums (x, x^2; dz, dz * xhat) are accumulated in float64 from the float32 values; the running statistics are evaluated in float64
 * and rounded once.
 * Semantics: no atomics and a fixed summation order -- the same bits on every launch; every word of the workspace that is read
 * was written by the same call, so nothing depends on what it held; every non-NULL gradient is OVERWRITTEN, a NULL gradient is "not
 * wanted" and skips the work only it needs, and a gradient has the same bits whichever others were asked for (all four NULL: nothing
 * is launched).  16-byte accesses when H*W % 4 == 0 and x / residual / y / grad_y / grad_x / grad_residual are 16-byte aligned, one
 * element per lane otherwise; all tensors 4-byte aligned.  y may not alias x or residual.
 * Workspace: 16-byte aligned, m3d_bn_act_train_workspace_bytes(B, C, H, W) bytes (16 per channel and chunk; the same for both
 * directions); -1 (and -1 chunks) for a shape that is not supported: a size < 1, N < 2, N beyond 2^31 - 8193.
 * Errors (M3D_E_ARG with m3d_last_error, nothing launched): such a shape (N < 2: batch statistics of one value, torch raises there
 * too), slope outside [0, 1] (NaN included), eps negative or not finite, a NULL required pointer (everything not marked NULL-able
 * above, the workspace included), a workspace below the size asked for (the message carries both sizes) or not 16-byte aligned. */
long long m3d_bn_act_train_workspace_bytes(int B, int C, int H, int W);
int m3d_bn_act_train_chunks(int B, int C, int H, int W);
int m3d_bn_act_train_forward(const float *x, const float *residual, const float *gamma, const float *beta, float *running_mean,
                             float *running_var, float *y, float *save_mean, float *save_invstd, int B, int C, int H, int W, double eps,
                             double momentum, float slope, void *workspace, long long workspace_bytes, m3d_stream_t stream);
int m3d_bn_act_train_backward(const float *grad_y, const float *x, const float *y, const float *gamma, const float *save_mean,
                              const float *save_invstd, float *grad_x, float *grad_residual, float *grad_gamma, float *grad_beta, int B,
                              int C, int H, int W, float slope, void *workspace, long long workspace_bytes, m3d_stream_t stream);

/* Weight packing: [Cout, Cin, kh, kw] (torch layout) -> [Cout_pad, kh*kw*Cin_pad] (tap-major, zero pad). */
int m3d_pack_conv_weight(const float *w, float *packed, int Cout, int Cout_pad, int Cin, int Cin_pad, int kh,
                         int kw, m3d_stream_t stream);
/* Layout changes at the op boundary. */
int m3d_nchw_to_nhwc(const float *in, float *out, int N, int C, int H, int W, int out_cs, m3d_stream_t stream);
int m3d_nhwc_to_nchw(const float *in, int in_cs, float *out, int N, int C, int H, int W, m3d_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backbone helpers (NHWC, channel-sliced views allowed through *_cs).
 * ------------------------------------------------------------------------------------------ */
/* 7x7, 3->16, stride 1, pad 3 on an NCHW image; fused affine (folded BN) + LeakyReLU; NHWC out. */
int m3d_stem_conv7x7(const float *img_nchw, const float *wgt /*[7*7*3][16]*/, const float *scale,
                     const float *shift, float *out, int out_cs, int N, int H, int W, m3d_stream_t stream);
/* Test-time input path of the reference: uint8 BGR frames [N][img_h][img_w][3] (what cv2.imread returns),
 * zero border at the bottom / right up to H x W, /255, -mean, /stds in float32 (mean / stds: HOST pointers to 3 floats, indexed
 * by BGR channel position exactly as lib/augmentations.py:44-57 applies them), BGR -> RGB, HWC -> CHW
 * (augmentations.py:472-501, dataloader.py:943-950).  Bit-identical to the numpy arithmetic.  m3d_preprocess_u8 writes the
 * [N][3][H][W] float tensor; m3d_stem_conv7x7_u8 feeds the stem directly (no float image in HBM: 1.5 MB instead of 5.9 MB
 * per 384x1280 frame cross the boundary). */
int m3d_preprocess_u8(const unsigned char *frames_bgr, int N, int img_h, int img_w, const float *mean3, const float *stds3,
                      float *out_nchw, int H, int W, m3d_stream_t stream);
int m3d_stem_conv7x7_u8(const unsigned char *frames_bgr, int img_h, int img_w, const float *mean3, const float *stds3,
                        const float *wgt, const float *scale, const float *shift, float *out, int out_cs, int N, int H, int W,
                        m3d_stream_t stream);
/* Training input path of the reference (lib/augmentations.py:164-234,236-469: photometric distortion, mirror, scale-and-shift warp
 * to H x W, Normalize; then BGR -> RGB, HWC -> CHW) for N uint8 BGR frames that share one [N][hmax][wmax][3] buffer, in one launch
 * per 16 images.  The random decisions are the host's: `params` is a HOST pointer to N rows of `param_stride` doubles
 * (>= M3D_AUGMENT_PARAMS), which travel to the kernel as launch arguments (no upload, no device allocation):
 *   [0] h  [1] w           the image's own size, <= hmax x wmax
 *   [2] mode               0 no photometric step, 1 contrast first, 2 contrast last
 *   [3] delta [4] alpha [5] sat [6] hue     brightness, contrast, saturation, hue shift in degrees (|hue| <= 360); [7] reserved
 *   [8..13] Minv           row-major 2x3: (x_src, y_src) = Minv . (x, y, 1), evaluated in float64; a mirror is folded in by the host
 * Bilinear taps at the exact source coordinate; a tap outside h x w is 0 AFTER the photometric step, so the border normalises to
 * (0 - mean) / std.  mean / stds: HOST pointers to 3 floats, indexed by BGR position.  Everything is validated before the first
 * launch (M3D_E_ARG: null pointer, N < 1, a size above the buffer's, a non-finite parameter, a singular Minv).  Deterministic. */
#define M3D_AUGMENT_PARAMS 14
int m3d_augment_u8(const unsigned char *frames_bgr, int N, int hmax, int wmax, const double *params, int param_stride,
                   const float *mean3, const float *stds3, float *out_nchw, int H, int W, m3d_stream_t stream);
/* 3x3, 16 -> 16, stride 1, pad 1 (DLA level0, pose_dla_dcn.py:341-342) as a direct VALU convolution: NHWC in/out,
 * wgt [(i*3+j)*16 + cin][16 cout], fused affine (folded BN) + LeakyReLU. */
int m3d_conv3x3_c16(const float *in, int in_cs, const float *wgt, const float *scale, const float *shift, float *out,
                    int out_cs, int N, int H, int W, m3d_stream_t stream);
/* The same layer as Winograd F(4x4,3x3) on v_mfma_f32_16x16x4_f32 (csrc/wino44_conv.hip: 4x fewer MFMA FLOPs; fp32 rounding ~7x
 * that of direct summation, as for m3d_wino44_conv3x3_forward): `U` = G g G^T of the 16 x 16 filters packed [36 xi][64 lanes =
 * 16 * (cin / 4) + cout][cin % 4] (m3dssd_amd/engine.py:pack_wino44_c16); H % 4 == W % 4 == 0. */
int m3d_conv3x3_c16_wino(const float *in, int in_cs, const float *U, const float *scale, const float *shift, float *out,
                         int out_cs, int N, int H, int W, m3d_stream_t stream);
int m3d_maxpool2x2(const float *in, int in_cs, float *out, int out_cs, int N, int H, int W, int C,
                   m3d_stream_t stream);
/* out = ConvTranspose2d_depthwise(in, wgt[4][4][C], stride 2, pad 1) + skip ;  in is [N,H,W,C], out/skip [N,2H,2W,C] */
int m3d_upsample2x_add(const float *in, int in_cs, const float *wgt, const float *skip, int skip_cs,
                       float *out, int out_cs, int N, int H, int W, int C, m3d_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Alignment stages.
 * ------------------------------------------------------------------------------------------ */
/* cls_planar [B][num_classes*A][HW] (class-major).  Writes per pixel: top-1 fg anchor (lowest
 * index among equals), its fg probability, and fg_all [B][A][HW] (may be NULL). */
int m3d_anchor_select(const float *cls_planar, int B, int A, int num_classes, int HW, int *sel_idx,
                      float *sel_prob, float *fg_all, m3d_stream_t stream);
/* The same selection for 4 classes that also writes the detection stage's sort keys score_bits [B][A*HW] (the bits
 * m3d_score_keys_planar / m3d_bundle_outputs produce) while the logits are in registers. */
int m3d_anchor_select_keys(const float *cls_planar, int B, int A, int HW, int *sel_idx, float *sel_prob,
                           unsigned int *score_bits, m3d_stream_t stream);
/* Top-1 over anchors of a given fg-probability map [B][A][HW] (lowest index among equals). */
int m3d_fg_top1(const float *prob, int B, int A, int HW, int *idx, float *val, m3d_stream_t stream);
/* mode 0 = shape_align (table [A][2*kk] -> offmask [B*HW][3*kk], kk=9), mode 1 = center_align
 * (bbox_x/bbox_y planar: value of image b, anchor a, pixel p at b*box_img_stride + a*HW + p;
 *  anchor_wh [A][2] = (w/stride, h/stride), mean/std xy). */
int m3d_align_offsets(int mode, const int *sel_idx, const float *sel_prob, float thresh, const float *table,
                      const float *bbox_x, const float *bbox_y, const float *anchor_wh, float mean_x,
                      float std_x, float mean_y, float std_y, float *offmask, int om_cs, int B, int A, int HW,
                      int kk, long long box_img_stride, m3d_stream_t stream);
/* mode 1 where bbox_x / bbox_y hold values only at the pixels with need[b*HW + p] != 0 (m3d_need_rows): the same offsets there,
 * offset 0 at the other pixels, whose bbox_x / bbox_y are not read (they may hold anything); the mask channel everywhere. */
int m3d_align_offsets_gated(const int *sel_idx, const float *sel_prob, float thresh, const float *bbox_x, const float *bbox_y,
                            const float *anchor_wh, float mean_x, float std_x, float mean_y, float std_y,
                            const unsigned char *need, float *offmask, int om_cs, int B, int A, int HW,
                            long long box_img_stride, m3d_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ANAB (asymmetric non-local block).
 * ------------------------------------------------------------------------------------------ */
/* items: int32 [n_items][6] = (bin, h0, h1, w0, w1, slot); grid = n_items x B.
 * kv: NHWC view of the K|V channels (C = Ck + Cv), s: NHWC view of the sigmoid gates, bin_scale[bin]
 * = which gate weights that bin; partial [B][n_bins][max_slots][C]. */
int m3d_anab_pool_partial(const float *kv, int kv_cs, const float *s, int s_cs, const int *items, int n_items,
                          const int *bin_scale, int n_bins, float *partial, int max_slots, int B, int H, int W,
                          int C, m3d_stream_t stream);
/* Reduce slots, divide by bin area, scatter into GEMM operand layouts:
 *   khat [B][keys_pad][ck_pad]  (row = key j, col = channel)   -- "weights" of the logits GEMM
 *   vhatT[B][Cv][keys_pad]      (row = channel, col = key j)   -- "weights" of the P.V GEMM   */
int m3d_anab_pool_finish(const float *partial, const int *bin_slots, const float *bin_inv_area, int n_bins,
                         int max_slots, int Ck, int Cv, float *khat, int keys_pad, int ck_pad, float *vhatT,
                         int B, int frag, m3d_stream_t stream);
/* (frag bit 0 / bit 1 in either finish: khat / vhatT is written in MFMA-fragment order [R/32][K/8][2][32][4], the `wgt` layout of
 * m3d_conv_wave_forward, instead of row-major.)
 * Both steps in one call for psp sizes (1, 4, 8, 16) on maps with H % 16 == 0 and W % 16 == 0, where the adaptive windows of
 * the four scales nest: the features are read once instead of once per scale.  `scratch` holds
 * m3d_anab_pool_nested_scratch_bytes(B, Ck + Cv) bytes; `s` = the 4 gate channels (scale order), bins in scale-major order
 * (1 + 16 + 64 + 256 = 337 keys).  Same outputs as m3d_anab_pool_partial + m3d_anab_pool_finish up to fp32 summation order. */
long long m3d_anab_pool_nested_scratch_bytes(int B, int C);
int m3d_anab_pool_nested(const float *kv, int kv_cs, const float *s, int s_cs, int B, int H, int W, int Ck, int Cv,
                         float *scratch, float *khat, int keys_pad, int ck_pad, float *vhatT, int frag, m3d_stream_t stream);
/* The same with the K|V map stored as bf16 (bf16 engine: the K|V conv writes bf16 NHWC, the 4 gate channels come from a separate
 * fp32 conv); fp32 sums, same outputs up to the rounding of the features. */
int m3d_anab_pool_nested_bf16(const void *kv, int kv_cs, const float *s, int s_cs, int B, int H, int W, int Ck, int Cv,
                              float *scratch, float *khat, int keys_pad, int ck_pad, float *vhatT, int frag, m3d_stream_t stream);
/* ... that also writes bf16 twins of khat / vhatT (same element order; either may be NULL): the operands of m3d_anab_attend_bf16,
 * without the two m3d_f32_to_bf16 launches. */
int m3d_anab_pool_nested_bf16_ex(const void *kv, int kv_cs, const float *s, int s_cs, int B, int H, int W, int Ck, int Cv,
                                 float *scratch, float *khat, int keys_pad, int ck_pad, float *vhatT, int frag,
                                 void *khat16, void *vhat16, m3d_stream_t stream);
/* The attention of ANAB in ONE launch on fp32 MFMA (csrc/anab_attend.hip; attention.py:207-211 + the BatchNorm / activation behind the
 * block): out[p] = act(softmax_k(q[p] . khat[k]) @ vhat (+ res[p], scale, shift)) per image, replacing the logits GEMM, the row softmax
 * and the P.V GEMM (the logits never reach memory; one pass over the keys with a running maximum).  q [B*HW][q_cs] (first Ck
 * channels), khat [B][keys_pad][k_cs] and vhatT [B][Cv][keys_pad] row-major as m3d_anab_pool_nested / _finish write them with
 * frag = 0; Ck in {64, 128, 168} with Cv = 128, or Ck = 168 with Cv = 256 (DLA-102: two workgroups per pixel tile, one per
 * half of the value channels), HW % 128 == 0, keys_pad % 32 == 0; res_mode as in m3d_conv_desc (0: + res behind the
 * affine, 1: before it); scale / shift / res may be NULL.
 * khat rows [keys, keys_pad), khat columns [Ck, k_cs) and vhatT columns [keys, keys_pad) are ignored whatever they hold, as for
 * m3d_anab_attend_bf16. */
int m3d_anab_attend_f32(const float *q, int q_cs, const float *khat, int k_cs, const float *vhatT, int B, int HW, int Ck,
                        int keys, int keys_pad, int Cv, const float *res, int res_cs, int res_mode, const float *scale,
                        const float *shift, int act, float *out, int out_cs, m3d_stream_t stream);
/* Row-list form: the same attention at the *n_rows (device) pixels rows[j] = b * HW + pix only (ascending: what m3d_need_rows
 * writes).  q, res and out are read / written at listed pixels and nowhere else, and there the output is bit-equal to the dense
 * call's; khat / vhatT are the whole images' as above.  An image may list no pixel, and entries at or past *n_rows are never read.
 * Nothing is read back: the grid is the dense one, and the workgroups past an image's part of the list return at once. */
int m3d_anab_attend_f32_rows(const float *q, int q_cs, const float *khat, int k_cs, const float *vhatT, int B, int HW, int Ck,
                             int keys, int keys_pad, int Cv, const float *res, int res_cs, int res_mode, const float *scale,
                             const float *shift, int act, float *out, int out_cs, const int *rows, const int *n_rows,
                             m3d_stream_t stream);
/* The ANAB attention core for TRAINING (csrc/anab_train.hip; attention.py:136-147 + 207-211, no residual / affine / activation: those
 * stay with the caller).  Per image, fp32, row views with a channel stride each: q [B*HW][q_cs] (first Ck channels), k (Ck), v (Cv),
 * g (the 4 gates behind their sigmoid, scale order), bins b = the AdaptiveAvgPool2d windows of sizes (1, 4, 8, 16) in scale-major
 * order (337 keys; start = floor(i*H/s), end = ceil((i+1)*H/s)):
 *     khat[b][c] = (1 / area_b) * sum_{p in win_b} g[p][scale(b)] * k[p][c],   vhat likewise from v,
 *     S = q . khat^T,   P = softmax_keys(S),   out = P . vhat               (out [B*HW][out_cs], first Cv channels).
 * Forward: the pooling launches of the engine (m3d_anab_pool_nested where H % 16 == 0 and W % 16 == 0, m3d_anab_pool_partial +
 * _finish otherwise; K and V pooled one after the other) and m3d_anab_attend_f32 without its epilogue, so it has that kernel's
 * support set: (Ck, Cv) in {(64, 128), (128, 128), (168, 128), (168, 256)}, H * W % 128 == 0, any H, W >= 1 otherwise; anything else is
 * M3D_E_ARG and m3d_anab_attention_workspace_bytes returns -1.  khat [B][352][round_up(Ck, 32)] and vhat^T [B][Cv][352] are the
 * first two blocks of the workspace.
 * Backward, with dO = grad_out and O = P . vhat:
 *     dvhat = P^T dO,  dP = dO vhat^T,  D = rowsum(dO * O),  dS = P * (dP - D),  dq = dS khat,  dkhat = dS^T q,
 *     and with w_b(p) = [p in win_b] / area_b:   dk[p][c] = sum_b w_b(p) g[p][scale(b)] dkhat[b][c],   dv the same with dvhat,
 *     dg[p][s] = sum_{b: scale(b) = s} w_b(p) (sum_c k[p][c] dkhat[b][c] + sum_c v[p][c] dvhat[b][c]).
 * A pixel is taken with EVERY bin that contains it (one per scale where the windows nest, up to two per dimension where H or W is
 * not a multiple of the scale, more where H < scale).  The backward pools again into its own workspace (it needs nothing of the
 * forward's); S, P, dP and dS live in registers only; the products run on fp32 MFMA.
 * Semantics: every non-NULL gradient is OVERWRITTEN (channels past Ck / Cv / 4 inside its stride are neither read nor written); a
 * NULL gradient is "not wanted" and skips the work only it needs; a result is the same bits whichever other gradients were asked
 * for and from run to run (no atomics; the sums over the pixels of an image are taken in a fixed order); nothing depends on what
 * the workspace held.  q and grad_out: 16-byte aligned views, row strides multiples of 4 floats; workspace 256-byte aligned,
 * m3d_anab_attention_workspace_bytes(B, H, W, Ck, Cv, backward) bytes. */
long long m3d_anab_attention_workspace_bytes(int B, int H, int W, int Ck, int Cv, int backward);
int m3d_anab_attention_forward(const float *q, const float *k, const float *v, const float *g, float *out, int B, int H, int W, int Ck,
                               int Cv, int q_cs, int k_cs, int v_cs, int g_cs, int out_cs, void *workspace, long long workspace_bytes,
                               m3d_stream_t stream);
int m3d_anab_attention_backward(const float *q, const float *k, const float *v, const float *g, const float *grad_out, float *grad_q,
                                float *grad_k, float *grad_v, float *grad_g, int B, int H, int W, int Ck, int Cv, int q_cs, int k_cs,
                                int v_cs, int g_cs, int go_cs, int gq_cs, int gk_cs, int gv_cs, int gg_cs, void *workspace,
                                long long workspace_bytes, m3d_stream_t stream);
/* The same operator with bf16 tensors (csrc/anab_train.hip on its bf16 element traits; the compute type of torch.autocast(bfloat16)): the mathematics, the
 * bin rule, the support set, the semantics of NULL gradients, overwriting, reproducibility (no atomics, fixed summation order, the
 * same bits whichever gradients were asked for) and independence of the workspace's contents are those of the fp32 functions above.
 * All nine tensors are bf16 (grad_g too), strides in elements; the products run on v_mfma_f32_32x32x16_bf16 with Ck = 168 padded
 * with zeros to 176.  Rounding points, part of the contract:
 *   - pooling sums (a fixed order that depends only on the window), softmax statistics (m, l, D) and all accumulators are fp32;
 *   - khat / vhat are rounded once to bf16, as MFMA operands; S and dP are never rounded;
 *   - P is rounded once as an MFMA operand: the unnormalised exp(S - m) in the forward's P . vhat, with 1 / l applied to the fp32
 *     accumulator, and the normalised exp(S - m) / l in the backward's P^T . dO;
 *   - dS = P * (dP - D) (P in fp32) is rounded once, as the operand of dq and dkhat;
 *   - dkhat / dvhat, their sums over the pixel chunks and the gather stay fp32; every output is rounded once to bf16.
 * 1 / l is an IEEE division (correctly rounded: exactly 1/2 for l = 2); exp is expf.
 * Alignment: q and grad_out are 16-byte aligned views with row strides that are multiples of 8 elements; k, v and g are 4-byte
 * aligned with even row strides; outputs have no alignment rule.  Anything else is M3D_E_ARG, a workspace below
 * m3d_anab_attention_workspace_bytes_bf16(B, H, W, Ck, Cv, backward) bytes included (-1 for an unsupported shape); the workspace is
 * 256-byte aligned.  The forward is one pooling launch (bf16 khat, khat^T, vhat, vhat^T into the zeroed workspace) and one
 * attention launch; the backward pools again and needs nothing of the forward's. */
long long m3d_anab_attention_workspace_bytes_bf16(int B, int H, int W, int Ck, int Cv, int backward);
int m3d_anab_attention_forward_bf16(const void *q, const void *k, const void *v, const void *g, void *out, int B, int H, int W, int Ck,
                                    int Cv, int q_cs, int k_cs, int v_cs, int g_cs, int out_cs, void *workspace,
                                    long long workspace_bytes, m3d_stream_t stream);
int m3d_anab_attention_backward_bf16(const void *q, const void *k, const void *v, const void *g, const void *grad_out, void *grad_q,
                                     void *grad_k, void *grad_v, void *grad_g, int B, int H, int W, int Ck, int Cv, int q_cs, int k_cs,
                                     int v_cs, int g_cs, int go_cs, int gq_cs, int gk_cs, int gv_cs, int gg_cs, void *workspace,
                                     long long workspace_bytes, m3d_stream_t stream);
/* In-place softmax over the first `valid` columns of each row; columns [valid, cs) are zeroed. */
int m3d_softmax_rows(float *x, int rows, int valid, int cs, m3d_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Outputs, decode, NMS.
 * ------------------------------------------------------------------------------------------ */
/* planar staging (cls [B][4A][HW], box [B][11][A][HW] in the order x,y,w,h,x3d,y3d,z3d,w3d,h3d,l3d,rY3d)
 * -> cls/prob [B][A*HW][4], bbox_2d [B][A*HW][4], bbox_3d [B][A*HW][7], and (optional) score_bits [B][A*HW]: the
 * max fg class probability of the row as monotone unsigned bits (a > b as floats <=> bits(a) > bits(b)), the sort
 * key of m3d_topk_decode. */
int m3d_bundle_outputs(const float *cls_planar, const float *box_planar, float *cls, float *prob, float *bbox_2d,
                       float *bbox_3d, unsigned int *score_bits, int B, int A, int HW, m3d_stream_t stream);
/* The sort keys alone (score_bits [B][A*HW]) from the planar class logits, with the softmax arithmetic of m3d_bundle_outputs (the
 * same bits): for callers that only run the detection stage (m3d_topk_decode_planar) and never read cls / prob / bbox_2d /
 * bbox_3d in full -- 5.5 MB per image instead of the 38 MB the bundling moves.  HW % 4 == 0, 16-byte aligned buffers. */
int m3d_score_keys_planar(const float *cls_planar, unsigned int *score_bits, int B, int A, int HW, m3d_stream_t stream);
/* The reference's `argsort()[::-1][:nms_topN_pre]` + decode (lib/rpn_util.py:1442-1544) in one launch, one workgroup
 * per image: radix select of the k rows with the largest (score, -row) -- descending score, ascending row among equal
 * scores: a total order, unlike the reference's unstable argsort -- bitonic sort of those k, decode of exactly those rows
 * -> aboxes [B][k][14] (x1,y1,x2,y2,score,cls,x3d,y3d,z3d,w3d,h3d,l3d,ry3d,anchor), score-descending; rows_out [B][k]
 * (optional) gets the selected row ids.  1 <= k <= min(R, 16384), R < 2^22; workspace: m3d_topk_decode_workspace_bytes. */
long long m3d_topk_decode_workspace_bytes(int B, int R);
int m3d_topk_decode(const unsigned int *score_bits, const float *prob, const float *bbox_2d, const float *bbox_3d,
                    const float *rois /*[R][5]*/, const float *anchors /*[A][9]*/, const float *means /*[11]*/,
                    const float *stds /*[11]*/, float *aboxes, int *rows_out, void *workspace, long long workspace_bytes,
                    int B, int R, int k, m3d_stream_t stream);
/* Same with the test-time scale factor of every image (scale [B] device floats, or NULL = 1): the 2-D corners and the projected
 * 3-D centre are divided by it right after the decode -- BEFORE the NMS that follows, as im_detect_3d does
 * (lib/rpn_util.py:1504-1506; the +1 area convention of the NMS is not scale invariant). */
int m3d_topk_decode_scaled(const unsigned int *score_bits, const float *prob, const float *bbox_2d, const float *bbox_3d,
                           const float *rois, const float *anchors, const float *means, const float *stds, const float *scale,
                           float *aboxes, int *rows_out, void *workspace, long long workspace_bytes, int B, int R, int k,
                           m3d_stream_t stream);
/* m3d_topk_decode_scaled reading the planar staging of the heads instead of the bundled tensors (cls_planar [B][4A][HW],
 * box_planar [B][11][A*HW]; score_bits from m3d_score_keys_planar or m3d_bundle_outputs): row = a*HW + p like
 * lib/rpn_util.py:892-901 flattens it; class probabilities of the k decoded rows are recomputed from their logits.  Output
 * identical (bit for bit) to m3d_bundle_outputs + m3d_topk_decode_scaled. */
int m3d_topk_decode_planar(const unsigned int *score_bits, const float *cls_planar, const float *box_planar, const float *rois,
                           const float *anchors, const float *means, const float *stds, const float *scale, float *aboxes,
                           int *rows_out, void *workspace, long long workspace_bytes, int B, int A, int HW, int k,
                           m3d_stream_t stream);
/* m3d_topk_decode_planar for few images on a large chip: the pass over all R keys is spread over `wgs_per_image` workgroups
 * per image (histogram of the top 11 score bits into a global histogram, then every workgroup appends its slice's keys above /
 * inside the threshold bin to global lists), and one finishing workgroup per image walks the lower digits, sorts and decodes.
 * Four launches whatever the data (graph-capturable), integer atomics only, nothing carried over between calls.  Same contract
 * and limits, output identical bit for bit.  wgs_per_image: 0 = the library's choice, else 1 .. 256 (M3D_E_ARG outside);
 * slices are whole 16-byte groups of keys, so trailing workgroups may be idle.  workspace:
 * m3d_topk_decode_mw_workspace_bytes(B, R = A * HW, k)  (-1 for a non-positive argument). */
long long m3d_topk_decode_mw_workspace_bytes(int B, int R, int k);
int m3d_topk_decode_planar_mw(const unsigned int *score_bits, const float *cls_planar, const float *box_planar, const float *rois,
                              const float *anchors, const float *means, const float *stds, const float *scale, float *aboxes,
                              int *rows_out, void *workspace, long long workspace_bytes, int B, int A, int HW, int k,
                              int wgs_per_image, m3d_stream_t stream);
/* The pixels whose box-head outputs the top-k decode can read.  score_bits [B][A*HW]: the monotone keys (row = a*HW + pix).
 *   thresh [B]    the exact k-th largest key of each image (k >= A*HW: the smallest key)
 *   need [B*HW]   1 where any of the pixel's A keys is >= thresh[b], else 0 (keys equal to the threshold only enlarge the set)
 *   rows [B*HW]   the needed pixels as b*HW + pix, ascending; entries past *n_rows are not written
 *   n_rows        their number, on the device
 * Six launches whatever the data (graph-capturable), integer atomics only, nothing read back, nothing carried over between
 * calls.  workspace: m3d_need_rows_workspace_bytes(B, HW)  (-1 for a non-positive argument). */
long long m3d_need_rows_workspace_bytes(int B, int HW);
int m3d_need_rows(const unsigned int *score_bits, int B, int A, int HW, int k, unsigned int *thresh, unsigned char *need,
                  int *rows, int *n_rows, void *workspace, long long workspace_bytes, m3d_stream_t stream);
/* Decode `n_rows` selected rows per image -> aboxes [B][n_rows][14]
 * (x1,y1,x2,y2,score,cls,x3d,y3d,z3d,w3d,h3d,l3d,ry3d,anchor). */
int m3d_decode_rows(const long long *rows /*[B][n_rows] row ids*/, const float *prob, const float *bbox_2d,
                    const float *bbox_3d, const float *rois /*[R][5]*/, const float *anchors /*[A][9]*/,
                    const float *means /*[11]*/, const float *stds /*[11]*/, float *aboxes, int B, int R,
                    int n_rows, m3d_stream_t stream);

/* Greedy NMS on device.  boxes_dev [B][n][box_stride>=4] sorted by descending score; mask_ws needs
 * B*n*ceil(n/64) uint64.  keep_dev [B][n] int32 (kept positions, ascending), num_keep_dev [B].
 * n <= 16384 (the reference's _nms is unbounded -- the host-pointer twin `_nms` below is too; the path calls this with
 * nms_topN_pre = 3000 rows): up to 4096 rows one wave holds the whole "removed" bit set of an image in registers (64 lanes x 64
 * bits), up to 16384 it lives in LDS; larger n returns M3D_E_ARG. */
long long m3d_nms_workspace_bytes(int B, int n);
int m3d_nms_sorted_dev(const float *boxes_dev, int B, int n, int box_stride, float thresh, void *mask_ws,
                       int *keep_dev, int *num_keep_dev, m3d_stream_t stream);
/* Kept rows of the NMS -> fixed-size blocks (lib/rpn_util.py:1547-1555 `aboxes[keep][:nms_topN_post]`): block
 * [B][post + 1][14], rows [0, min(num_keep, post)) = aboxes[keep[j]], the rest zero, row `post` = (count, 0, ...) -- the
 * message of the multi-GPU all-gather; counts [B] (optional) gets min(num_keep, post). */
int m3d_select_post(const float *aboxes /*[B][n][14]*/, const int *keep /*[B][n]*/, const int *num_keep /*[B]*/, int B, int n,
                    int post, float *block, int *counts, m3d_stream_t stream);
/* The 3-D size, depth and angle of a row (columns 8..12: z3d, w3d, h3d, l3d, ry3d) are read by nobody before the row is among
 * the `post` rows per image that m3d_select_post copies (the NMS reads columns 0..4).  Three entry points let the heads behind
 * those columns run at the pixels of the selected rows only:
 *   m3d_topk_decode_planar_2d: m3d_topk_decode_planar (same arguments, workspace and limits) that does not read box planes 6..10
 *     and writes +0 to columns 8..12; rows_out is required.  Every other column and rows_out are bit-equal to the full decode.
 *   m3d_post_rows: rows_out [B][n] of that decode, keep [B][n] / num_keep [B] of the NMS -> rows: the distinct pixels
 *     b*HW + rows_out[b][keep[b][j]] % HW of the first min(num_keep[b], post) kept rows of every image, ascending (the list
 *     m3d_need_rows writes, for m3d_head_mlp_forward_rows / m3d_anab_attend_f32_rows), n_rows their number on the device.
 *     rows holds min(B*post, B*HW) entries; entries at or past *n_rows are not written.  One launch whatever the data
 *     (graph-capturable), nothing read back, nothing carried over between calls.  B*post <= 4096, else M3D_E_ARG.
 *   m3d_fill_post_3d: columns 8..12 of rows [0, min(counts[b], post)) of block [B][post + 1][14] (as m3d_select_post wrote it
 *     from the 2-D decode; counts: its counts) from box planes 6..10 at the staging row rows_out[b][keep[b][j]], with the
 *     arithmetic of the full decode (the same bits).  Nothing else of the block is written. */
int m3d_topk_decode_planar_2d(const unsigned int *score_bits, const float *cls_planar, const float *box_planar, const float *rois,
                              const float *anchors, const float *means, const float *stds, const float *scale, float *aboxes,
                              int *rows_out, void *workspace, long long workspace_bytes, int B, int A, int HW, int k,
                              m3d_stream_t stream);
int m3d_post_rows(const int *rows_out, const int *keep, const int *num_keep, int B, int n, int post, int HW, int *rows,
                  int *n_rows, m3d_stream_t stream);
int m3d_fill_post_3d(const float *box_planar, const float *rois, const float *anchors, const float *means, const float *stds,
                     const int *rows_out, const int *keep, const int *counts, int B, int A, int HW, int n, int post, float *block,
                     m3d_stream_t stream);
/* Exact twin of the reference's _nms (lib/nms/gpu_nms.hpp): host pointers, synchronous. */
void _nms(int *keep_out, int *num_out, const float *boxes_host, int boxes_num, int boxes_dim,
          float nms_overlap_thresh, int device_id);

/* ------------------------------------------------------------------------------------------
 * Post-NMS 3-D refinement (lib/rpn_util.py:1801-1847 per-box loop of test_kitti_3d): convertAlpha2Rot,
 * hill_climb on the yaw (step_r_init, halving down to r_lim; the depth step is 0 as in the reference call) scored by
 * test_projection, convertRot2Alpha, camera-space centre.  One thread per row, float64.
 *   aboxes [B][K][14] fp32 rows (x1 y1 x2 y2 score cls x3d y3d z3d w3d h3d l3d alpha anchor), counts [B],
 *   p2 / p2_inv [B][16] row-major 4x4 doubles (device), out [B][K][16] doubles:
 *   valid, cls, alpha, x1, y1, x2, y2, h3d, w3d, l3d, x3d, y3d (bottom centre), z3d, ry3d, score, 0
 *   (valid = 0 and zeros for rows past counts[b] or with score < score_thresh) -- the fields of the KITTI result line
 *   '{cls} -1 -1 {alpha} {x1} {y1} {x2} {y2} {h} {w} {l} {x} {y} {z} {ry} {score}' (lib/rpn_util.py:1848-1849).
 * ------------------------------------------------------------------------------------------ */
int m3d_refine_3d(const float *aboxes, const int *counts, int B, int K, const double *p2, const double *p2_inv,
                  double score_thresh, int hill_climbing, double step_r_init, double r_lim, double *out, m3d_stream_t stream);
/* The same with the two per-image steps im_detect_3d / test_kitti_3d apply between NMS and the loop folded in, so that the call can
 * sit in a captured graph right behind m3d_select_post: scale [B] fp32 (device, or NULL) -- x1 y1 x2 y2 x3d y3d are divided by
 * scale[b] in float32 first (`coords_2d[:, 0:4] /= scale_factor`, lib/rpn_util.py:1506-1507 -- the reference does it BEFORE the NMS: pass the factors to m3d_topk_decode_scaled and NULL here to reproduce that); clip_wh [B][2] fp32 = (imW, imH)
 * (device, or NULL; an entry <= 0 disables it) -- the 2-D box is then clipped to [0, imW - 1] x [0, imH - 1] (:1533-1538).  The
 * rows themselves are not modified.  K may include the count row of a m3d_select_post block (it lies past counts[b]). */
int m3d_refine_3d_ex(const float *aboxes, const int *counts, int B, int K, const double *p2, const double *p2_inv,
                     const float *scale, const float *clip_wh, double score_thresh, int hill_climbing, double step_r_init,
                     double r_lim, double *out, m3d_stream_t stream);
/* Host twin of m3d_refine_3d_ex: the same arguments without the stream, every pointer a HOST pointer; synchronous, no device work.
 * A plain loop over the B*K rows through the row function the kernel calls (like the m3d_eval_* host natives below).
 * Angles: the reference's `while a > pi: a -= 2 pi` wrap does not terminate for a non-finite angle or |a| above ~1e17; here (kernel
 * and twin) an angle beyond 64 turns, inf or NaN is reduced once with remainder(a, 2 pi) (inf / NaN -> NaN); within 64 turns the
 * reference's loops run unchanged. */
int m3d_refine_3d_host(const float *aboxes, const int *counts, int B, int K, const double *p2, const double *p2_inv,
                       const float *scale, const float *clip_wh, double score_thresh, int hill_climbing, double step_r_init,
                       double r_lim, double *out);

/* ------------------------------------------------------------------------------------------
 * KITTI AP evaluator natives (lib/eval/eval.py, lib/eval/rotate_iou.py of the reference, which compiles them
 * with numba / numba.cuda).
 * m3d_rotate_iou_eval: rotate_iou_gpu_eval (rotate_iou.py:264-326).  boxes [N][5], qboxes [K][5] = (cx, cy, dx, dy, angle)
 *   float32 DEVICE pointers; iou [N][K] float32 device: entry [n][k] = devRotateIoUEval(qboxes[k], boxes[n], criterion) with
 *   criterion -1 IoU, 0 / qbox area, 1 / box area, 2 the intersection area itself.
 * The remaining entry points are HOST functions on float64 / int64 numpy-style arrays (synchronous, no device work):
 * m3d_eval_image_box_overlap: image_box_overlap (eval.py:84-113), boxes [N][4], q [K][4] -> out [N][K].
 * m3d_eval_d3_overlap: d3_box_overlap_kernel (eval.py:116-141) on boxes [N][7] / qboxes [K][7] = (x, y, z, l, h, w, ry);
 *   rinc [N][K] holds the BEV intersection areas on entry, the 3-D overlaps on return.
 * m3d_eval_statistics: compute_statistics_jit (eval.py:152-272) for one image.  overlaps [det][ov_stride] (detection j vs
 *   ground truth i at [j*ov_stride + i]), gt_datas [gt][5] = bbox, alpha; dt_datas [det][6] = bbox, alpha, score;
 *   ignored_* int64 (0 evaluate, 1 ignore, -1 other class); stats[4] = tp, fp, fn, similarity; thresholds_out (optional,
 *   room for gt_size values) gets the scores of the true positives, *n_thresholds their number.
 * m3d_eval_fused_statistics: fused_compute_statistics (eval.py:287-333) over a part of n_images images whose overlaps form
 *   one [sum det][sum gt] matrix; pr [n_thresholds][4] is accumulated into (tp, fp, fn, similarity).
 * ------------------------------------------------------------------------------------------ */
int m3d_rotate_iou_eval(const float *boxes_dev, int N, const float *qboxes_dev, int K, int criterion, float *iou_dev,
                        m3d_stream_t stream);
int m3d_eval_image_box_overlap(const double *boxes, int N, const double *q, int K, int criterion, double *out);
int m3d_eval_d3_overlap(const double *boxes, int N, const double *qboxes, int K, double *rinc, int criterion);
int m3d_eval_statistics(const double *overlaps, long long ov_stride, const double *gt_datas, int gt_size, const double *dt_datas,
                        int det_size, const long long *ignored_gt, const long long *ignored_det, const double *dc_bboxes, int n_dc,
                        int metric, double min_overlap, double thresh, int compute_fp, int compute_aos, double *stats,
                        double *thresholds_out, int *n_thresholds);
int m3d_eval_fused_statistics(const double *overlaps, long long ov_stride, double *pr, const long long *gt_nums,
                              const long long *dt_nums, const long long *dc_nums, int n_images, const double *gt_datas,
                              const double *dt_datas, const double *dontcares, const long long *ignored_gts,
                              const long long *ignored_dets, int metric, double min_overlap, const double *thresholds,
                              int n_thresholds, int compute_aos);

/* ------------------------------------------------------------------------------------------
 * Instrumentation: HIP-event timing of a launch sequence on a stream (used by bench.py).
 * ------------------------------------------------------------------------------------------ */
/* One wave samples the shader-cycle counter and the 100 MHz wall clock at both ends of a `seconds`-long window (<= 1 s):
 * out4_dev = {cycles0, realtime0, cycles1, realtime1}; (cycles1 - cycles0) / (realtime1 - realtime0) x 100 MHz = the shader clock the
 * chip held while whatever ran next to it on other streams (bench.py: sclk_under_step_ghz). */
int m3d_clock_probe(long long *out4_dev, double seconds, m3d_stream_t stream);
int m3d_event_create(void **ev);
int m3d_event_record(void *ev, m3d_stream_t stream);
int m3d_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on stop */
int m3d_event_destroy(void *ev);

#ifdef __cplusplus
}
#endif
#endif /* M3DSSD_HIP_H */
