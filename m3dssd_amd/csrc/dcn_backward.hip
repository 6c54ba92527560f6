// Backward pass of DCNv2: the drop-in for dcn_v2_cuda_backward (model/DCNv2/src/dcn_v2_cuda.c:104-241, kernels
// model/DCNv2/src/cuda/dcn_v2_im2col_cuda.cu:49-116,182-312) on NCHW fp32 tensors.  The mathematics is the analytic derivative
// of the forward as THIS library defines it, piecewise rule included: a sample at (h_im, w_im) contributes iff h_im > -1,
// w_im > -1, h_im < H, w_im < W, each of its four corners iff it lies inside the image, hl = floor(h_im), lh = h_im - hl; the
// sampling state comes from dcn_corners (common.h) -- the same code the forward kernels run, no lane masks in SGPRs.
//
// Per deformable group (channel slice g of the input, offset / mask slice g, weights not grouped), everything NHWC inside:
//   1. gcol[p][k*C + c] = sum_co grad_out[p][co] * W[co][c][k]: a 1x1 convolution Co -> kk*C of grad_out on m3d_conv2d_forward
//      with a pack of the transposed weight matrix (no new GEMM);
//   2. dcn_bwd_sample_kernel: one wave per output pixel, lane = channel.  Per tap it recomputes the corner state, reads gcol and
//      the four corner rows, and produces grad_mask[p][k] = sum_c gcol * val, grad_offset[p][2k], [2k+1] = mask * sum_c gcol *
//      d val / d(h, w) (butterfly reduction over the lanes: fixed order), col[p][k*C + c] = mask * val (the forward's A operand,
//      kept for step 3) and adds gcol * mask * w_q into the four corner rows of grad_input with float atomics: each atomic
//      wave-instruction is 64 lanes x one channel = 256 contiguous bytes of one NHWC pixel row;
//   3. dcn_bwd_wgrad_kernel: grad_weight[co][k*C + c] = sum_p grad_out[p][co] * col[p][k*C + c] on v_mfma_f32_32x32x2_f32.  The
//      reduction runs over pixels and the output is tiny, so the pixel range is split over workgroups; every split writes a raw
//      partial slab (grad_bias = pixel sums of grad_out rides in the same launch), dcn_bwd_reduce_kernel adds the slabs in split
//      order and scatters to the [Co][C][kh][kw] layout.
// `col` is written once by the sampling kernel and read back by the weight-gradient GEMM (not gathered again in the operand
// load): the sampling kernel has every value in registers anyway (grad_mask needs val), and the GEMM stays a plain two-operand
// stream without sampling code in its loop.
//
// Determinism: grad_offset, grad_mask, grad_weight, grad_bias are bitwise reproducible (fixed reduction orders).  grad_input is
// accumulated with float atomics, as the reference does (dcn_v2_im2col_cuda.cu:234): its last bits depend on arrival order.
// Every non-NULL gradient is OVERWRITTEN (the reference accumulates into grad_weight / grad_bias and adds into a zeroed
// grad_input); a NULL gradient pointer = not wanted, and the work only it needs is skipped.
#include <string.h>

#include "common.h"

static inline long long rupll(long long a, long long b) { return (a + b - 1) / b * b; }

// ------------------------------------------------------------------------------------------------------------------------
// [Co, Ctot, kh, kw] (channel slice [c0, c0 + C)) -> the packed weights of the 1x1 convolution that yields gcol:
// p[(k*Cp + c)][co] with row length cs (rows of padded channels and columns >= Co are zero)
__global__ void dcn_bwd_pack_wt_kernel(const float *__restrict__ w, float *__restrict__ p, int Co, int cs, int C, int Cp, int KK,
                                       int Ctot, int c0)
{
    const long long total = (long long)KK * Cp * cs;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int co = (int)(i % cs);
        const int c = (int)((i / cs) % Cp);
        const int k = (int)(i / ((long long)cs * Cp));
        p[i] = (co < Co && c < C) ? w[((long long)co * Ctot + c0 + c) * KK + k] : 0.f;
    }
}

// NHWC [N*HW][in_cs] -> channel slice [c0, c0 + C) of an NCHW tensor with Ctot channels, through a 32x32 LDS tile
__global__ void dcn_bwd_nhwc_to_nchw_slice_kernel(const float *__restrict__ in, int in_cs, float *__restrict__ out, int C, int HW,
                                                  int Ctot, int c0s)
{
    __shared__ float t[32][33];
    const int n = blockIdx.z, c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + r, c = c0 + tx;
        t[r][tx] = (c < C && p < HW) ? in[((size_t)n * HW + p) * in_cs + c] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, p = p0 + tx;
        if (c < C && p < HW) out[((size_t)n * Ctot + c0s + c) * HW + p] = t[tx][r];
    }
}

// ------------------------------------------------------------------------------------------------------------------------
struct DcnBwdSampleArgs {
    const float *in;     // [N*H*W][cp], channels >= C zero
    const float *om;     // [P][om_cs]: 2k = dh, 2k+1 = dw, 2kk + k = mask
    const float *gcol;   // [P][kk*cp] or NULL (then only col is produced)
    float *col;          // [P][kk*cp] or NULL
    float *gin;          // [N*H*W][cp], zeroed, or NULL
    float *goff, *gmask; // NCHW, already moved to this group's first channel, or NULL
    long long goff_img, gmask_img;   // floats between images of goff / gmask
    int P, H, W, Ho, Wo, cp, kh, kw, stride, pad, dil, om_cs;
};

__device__ __forceinline__ float and_not(float v, int drop) { return __uint_as_float(__float_as_uint(v) & ~(unsigned)drop); }

__device__ __forceinline__ float wave_sum(float v)    // butterfly over the 64 lanes: the same order in every run
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One wave per output pixel, lane = channel (cp % 64 == 0: no partial wave, so no lane mask anywhere in the sampling code).
// The corner state of a tap is the same in every lane; whether a corner row gets its atomic add is decided on the scalar unit
// (readfirstlane + scalar branch), not through a lane mask.
__global__ __launch_bounds__(256) void dcn_bwd_sample_kernel(DcnBwdSampleArgs a)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.P) return;
    const int HoWo = a.Ho * a.Wo;
    const int n = p / HoWo, pix = p - n * HoWo;
    const int y = pix / a.Wo, x = pix - y * a.Wo;
    const int kk = a.kh * a.kw;
    const size_t K = (size_t)kk * a.cp;
    const float *omp = a.om + (size_t)p * a.om_cs;
    const size_t img = (size_t)n * a.H * a.W * a.cp;
    const float *inb = a.in + img;
    for (int k = 0; k < kk; ++k) {
        const int i = k / a.kw, j = k - i * a.kw;
        const float dh = omp[2 * k], dw = omp[2 * k + 1], mk = omp[2 * kk + k];
        const float h_im = (float)(y * a.stride - a.pad + i * a.dil) + dh, w_im = (float)(x * a.stride - a.pad + j * a.dil) + dw;
        float w[4];
        int o[4], drop[4];
        dcn_corners(h_im, w_im, a.H, a.W, 0, w, o, drop);
        // d w_q / d h_im and d w_q / d w_im of the kept corners (w = {uh*uw, uh*lw, lh*uw, lh*lw}); a dropped corner has none
        const float lh = h_im - floorf(h_im), lw = w_im - floorf(w_im), uh = 1.f - lh, uw = 1.f - lw;
        const float dwh[4] = {and_not(-uw, drop[0]), and_not(-lw, drop[1]), and_not(uw, drop[2]), and_not(lw, drop[3])};
        const float dww[4] = {and_not(-uh, drop[0]), and_not(uh, drop[1]), and_not(-lh, drop[2]), and_not(lh, drop[3])};
        size_t row[4];
        int keep[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            row[q] = (size_t)(unsigned)(o[q] & ~drop[q]) * a.cp;          // a dropped corner reads pixel 0 with weight 0
            keep[q] = __builtin_amdgcn_readfirstlane(drop[q]) == 0;
        }
        float sm = 0.f, sh = 0.f, sw = 0.f;
        for (int c = lane; c < a.cp; c += 64) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = and_not(inb[row[q] + c], drop[q]);
            const float val = w[0] * v[0] + w[1] * v[1] + w[2] * v[2] + w[3] * v[3];
            const size_t ci = (size_t)p * K + (size_t)k * a.cp + c;
            if (a.col) a.col[ci] = mk * val;
            if (a.gcol) {
                const float g = a.gcol[ci];
                sm += g * val;
                sh += g * (dwh[0] * v[0] + dwh[1] * v[1] + dwh[2] * v[2] + dwh[3] * v[3]);
                sw += g * (dww[0] * v[0] + dww[1] * v[1] + dww[2] * v[2] + dww[3] * v[3]);
                if (a.gin) {
                    const float gm = g * mk;
                    float *gb = a.gin + img + c;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (keep[q]) atomicAdd(gb + row[q], gm * w[q]);
                }
            }
        }
        if (a.gcol && (a.goff || a.gmask)) {
            sm = wave_sum(sm);
            sh = wave_sum(sh);
            sw = wave_sum(sw);
            if (lane == 0) {
                if (a.gmask) a.gmask[(size_t)n * a.gmask_img + (size_t)k * HoWo + pix] = sm;
                if (a.goff) {
                    float *gp = a.goff + (size_t)n * a.goff_img + (size_t)(2 * k) * HoWo + pix;
                    gp[0] = mk * sh;
                    gp[HoWo] = mk * sw;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// grad_weight partials: D[co][kc] = sum over the pixels of one split of go[p][co] * col[p][kc].  One wave per workgroup owns a
// (32 * TA) x 64 tile of D; one v_mfma_f32_32x32x2_f32 consumes two pixels (A = go^T: row co = lane % 32, k = lane / 32;
// B = col: k = lane / 32, column kc = lane % 32), both operands are 128-byte row segments of their NHWC buffers.  The pixel sums
// of go (grad_bias) ride along in the workgroups of the first column block.  DW == false: bias sums only.
template <int TA, bool DW>
__global__ __launch_bounds__(64) void dcn_bwd_wgrad_kernel(const float *__restrict__ go, int go_cs, const float *__restrict__ col, int K,
                                                           float *__restrict__ slab, float *__restrict__ bslab, int co_pad, int P,
                                                           int chunk)
{
    constexpr int U = 4;                                 // pixel pairs in flight: all loads of a step issue before its MFMAs
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    const int kc0 = blockIdx.x * 64, co0 = blockIdx.y * 32 * TA, s = blockIdx.z;
    const int p_beg = s * chunk, p_end = min(P, p_beg + chunk);
    f32x16 acc[TA][2];
    float bsum[TA];
#pragma unroll
    for (int t = 0; t < TA; ++t) {
        bsum[t] = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
    }
    for (int pp = p_beg; pp < p_end; pp += 2 * U) {
        float av[U][TA], bv[U][2];
#pragma unroll
        for (int e = 0; e < U; ++e) {
            const int p = pp + 2 * e + half;
            const bool ok = p < p_end;                   // past the end of the split: the operand is zero (row p_beg is read)
            const size_t pc = (size_t)(ok ? p : p_beg);
#pragma unroll
            for (int t = 0; t < TA; ++t) {
                const float g = go[pc * go_cs + co0 + 32 * t + l31];
                av[e][t] = ok ? g : 0.f;
            }
            if constexpr (DW) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float cv = col[pc * K + kc0 + 32 * u + l31];
                    bv[e][u] = ok ? cv : 0.f;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < U; ++e) {
#pragma unroll
            for (int t = 0; t < TA; ++t) {
                bsum[t] += av[e][t];
                if constexpr (DW) {
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e][t], bv[e][u], acc[t][u], 0, 0, 0);
                }
            }
        }
    }
    if constexpr (DW) {
        // D layout of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int t = 0; t < TA; ++t)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
                    slab[((size_t)s * co_pad + co) * K + kc0 + 32 * u + l31] = acc[t][u][r];
                }
    }
    if (blockIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < TA; ++t) {
            const float b = bsum[t] + __shfl_xor(bsum[t], 32);
            if (half == 0) bslab[(size_t)s * co_pad + co0 + 32 * t + l31] = b;
        }
    }
}

// slabs added in split order; grad_weight element (co, c0 + c, k) <- column k*cp + c, grad_bias[co] <- the bias slabs
__global__ void dcn_bwd_reduce_kernel(const float *__restrict__ slab, const float *__restrict__ bslab, float *__restrict__ gw,
                                      float *__restrict__ gb, int splits, int Co, int co_pad, int C, int cp, int KK, int Ctot, int c0)
{
    const long long nw = gw ? (long long)Co * C * KK : 0, total = nw + (gb ? Co : 0);
    const size_t K = (size_t)KK * cp;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        if (i < nw) {
            const int k = (int)(i % KK);
            const int c = (int)((i / KK) % C);
            const int co = (int)(i / ((long long)KK * C));
            float acc = 0.f;
            for (int s = 0; s < splits; ++s) acc += slab[((size_t)s * co_pad + co) * K + (size_t)k * cp + c];
            gw[((size_t)co * Ctot + c0 + c) * KK + k] = acc;
        } else {
            const int co = (int)(i - nw);
            float acc = 0.f;
            for (int s = 0; s < splits; ++s) acc += bslab[(size_t)s * co_pad + co];
            gb[co] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
struct DcnBwdWs {
    long long in_off, om_off, go_off, wt_off, gcol_off, col_off, gin_off, slab_off, bslab_off, total;
    int cp, co_pad, om_cs, ho, wo, K, splits, chunk;
};

// `c` = channels of ONE deformable group.  The layout does not depend on which gradients are wanted.
static DcnBwdWs dcn_bwd_ws(int n, int c, int h, int w, int co, int kh, int kw, int stride, int pad, int dil)
{
    DcnBwdWs s;
    s.cp = (int)rupll(c, 64);          // the sampling kernel runs whole waves of 64 channels
    s.co_pad = (int)rupll(co, 64);     // channel stride of grad_out NHWC = K of the gcol GEMM = row count of a slab
    s.ho = (h + 2 * pad - (dil * (kh - 1) + 1)) / stride + 1;
    s.wo = (w + 2 * pad - (dil * (kw - 1) + 1)) / stride + 1;
    s.om_cs = (int)rupll(3 * kh * kw, 4);
    s.K = kh * kw * s.cp;
    const long long P = (long long)n * (s.ho > 0 ? s.ho : 0) * (s.wo > 0 ? s.wo : 0);
    // pixel splits of the weight-gradient GEMM: about 2048 waves in all, at most 4096 and at least 64 pixels per split
    const long long tiles = (long long)(s.K / 64) * (s.co_pad / (s.co_pad % 128 ? 64 : 128));
    long long sp = (2048 + tiles - 1) / tiles;
    if (sp < (P + 4095) / 4096) sp = (P + 4095) / 4096;
    if (sp > (P + 63) / 64) sp = (P + 63) / 64;
    if (sp < 1) sp = 1;
    s.chunk = (int)rupll((P + sp - 1) / sp > 0 ? (P + sp - 1) / sp : 1, 2);
    s.splits = P > 0 ? (int)((P + s.chunk - 1) / s.chunk) : 1;
    long long o = 0;
    s.in_off = o;    o += rupll((long long)n * h * w * s.cp * 4, 256);
    s.om_off = o;    o += rupll(P * s.om_cs * 4, 256);
    s.go_off = o;    o += rupll(P * s.co_pad * 4, 256);
    s.wt_off = o;    o += rupll((long long)s.K * s.co_pad * 4, 256);
    s.gcol_off = o;  o += rupll(P * s.K * 4, 256);
    s.col_off = o;   o += rupll(P * s.K * 4, 256);
    s.gin_off = o;   o += rupll((long long)n * h * w * s.cp * 4, 256);
    s.slab_off = o;  o += rupll((long long)s.splits * s.co_pad * s.K * 4, 256);
    s.bslab_off = o; o += rupll((long long)s.splits * s.co_pad * 4, 256);
    s.total = o;
    return s;
}

extern "C" long long m3d_dcn_v2_backward_workspace_bytes(int batch, int channels, int height, int width, int channels_out,
                                                         int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                                         int deformable_group)
{
    if (deformable_group < 1 || channels < 1 || channels % deformable_group) return -1;
    if (batch < 1 || height < 1 || width < 1 || channels_out < 1 || kernel_h < 1 || kernel_w < 1 || stride < 1 || pad < 0 || dilation < 1)
        return -1;
    return dcn_bwd_ws(batch, channels / deformable_group, height, width, channels_out, kernel_h, kernel_w, stride, pad, dilation).total;
}

extern "C" int m3d_dcn_v2_backward(const float *input, const float *weight, const float *offset, const float *mask,
                                   const float *grad_output, float *grad_input, float *grad_offset, float *grad_mask,
                                   float *grad_weight, float *grad_bias, int batch, int channels, int height, int width,
                                   int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                   int dilation_h, int dilation_w, int deformable_group, void *workspace, long long workspace_bytes,
                                   m3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    M3D_REQUIRE(input && weight && offset && mask && grad_output && workspace, "dcn_v2_backward: null pointer");
    M3D_REQUIRE(batch > 0 && channels > 0 && height > 0 && width > 0 && channels_out > 0 && kernel_h > 0 && kernel_w > 0 &&
                    stride_h > 0 && pad_h >= 0 && dilation_h > 0,
                "dcn_v2_backward: bad shape");
    M3D_REQUIRE(deformable_group >= 1 && channels % deformable_group == 0,
                "dcn_v2_backward: deformable_group (%d) must divide the input channels (%d)", deformable_group, channels);
    M3D_REQUIRE(stride_h == stride_w && pad_h == pad_w && dilation_h == dilation_w,
                "dcn_v2_backward: anisotropic stride/pad/dilation not supported");
    M3D_REQUIRE(((uintptr_t)workspace & 255) == 0, "dcn_v2_backward: workspace must be 256-byte aligned");
    const int G = deformable_group, cg = channels / G, kk = kernel_h * kernel_w;
    const DcnBwdWs s = dcn_bwd_ws(batch, cg, height, width, channels_out, kernel_h, kernel_w, stride_h, pad_h, dilation_h);
    if (workspace_bytes < s.total) {
        m3d_set_error("dcn_v2_backward: workspace %lld < %lld bytes (m3d_dcn_v2_backward_workspace_bytes)", workspace_bytes, s.total);
        return M3D_E_WORKSPACE;
    }
    M3D_REQUIRE(s.ho > 0 && s.wo > 0, "dcn_v2_backward: empty output");
    const long long P = (long long)batch * s.ho * s.wo, HoWo = (long long)s.ho * s.wo;
    M3D_REQUIRE(P < (1ll << 29) && (long long)batch * height * width * s.cp < (1ll << 31), "dcn_v2_backward: tensor too large");
    if (!grad_input && !grad_offset && !grad_mask && !grad_weight && !grad_bias) return M3D_OK;
    char *ws = (char *)workspace;
    float *in_nhwc = (float *)(ws + s.in_off), *om = (float *)(ws + s.om_off), *go = (float *)(ws + s.go_off);
    float *wt = (float *)(ws + s.wt_off), *gcol = (float *)(ws + s.gcol_off), *col = (float *)(ws + s.col_off);
    float *gin = (float *)(ws + s.gin_off), *slab = (float *)(ws + s.slab_off), *bslab = (float *)(ws + s.bslab_off);
    const bool need_gcol = grad_input || grad_offset || grad_mask, need_col = grad_weight != nullptr;
    const bool need_sample = need_gcol || need_col;
    int rc;
    if (s.co_pad != channels_out) M3D_HIP(hipMemsetAsync(go, 0, (size_t)P * s.co_pad * 4, stream));
    if ((rc = m3d_nchw_to_nhwc_slice(grad_output, channels_out, 0, go, batch, channels_out, s.ho, s.wo, s.co_pad, stream))) return rc;
    for (int g = 0; g < G; ++g) {
        if (need_sample) {
            if (s.cp != cg) M3D_HIP(hipMemsetAsync(in_nhwc, 0, (size_t)batch * height * width * s.cp * 4, stream));
            if ((rc = m3d_nchw_to_nhwc_slice(input, channels, g * cg, in_nhwc, batch, cg, height, width, s.cp, stream))) return rc;
            if ((rc = m3d_nchw_to_nhwc_slice(offset, 2 * kk * G, g * 2 * kk, om, batch, 2 * kk, s.ho, s.wo, s.om_cs, stream))) return rc;
            if ((rc = m3d_nchw_to_nhwc_slice(mask, kk * G, g * kk, om + 2 * kk, batch, kk, s.ho, s.wo, s.om_cs, stream))) return rc;
        }
        if (need_gcol) {
            const long long total = (long long)s.K * s.co_pad;
            hipLaunchKernelGGL(dcn_bwd_pack_wt_kernel, dim3(imin(cdiv(total, 256), 4096)), dim3(256), 0, stream, weight, wt,
                               channels_out, s.co_pad, cg, s.cp, kk, channels, g * cg);
            M3D_LAUNCH_CHECK();
            m3d_conv_desc d;
            memset(&d, 0, sizeof(d));
            d.in = go; d.in_cs = s.co_pad; d.N = batch; d.H = s.ho; d.W = s.wo; d.Cin = s.co_pad;
            d.wgt = wt; d.Cout = s.K; d.Cout_pad = s.K;
            d.kh = 1; d.kw = 1; d.stride = 1; d.pad = 0; d.dil = 1;
            d.Ho = s.ho; d.Wo = s.wo; d.out = gcol; d.out_cs = s.K;
            d.sigmoid_from = -1;
            if ((rc = m3d_conv2d_forward(&d, stream))) return rc;
        }
        if (grad_input) M3D_HIP(hipMemsetAsync(gin, 0, (size_t)batch * height * width * s.cp * 4, stream));
        if (need_sample) {
            DcnBwdSampleArgs a;
            a.in = in_nhwc; a.om = om; a.gcol = need_gcol ? gcol : nullptr; a.col = need_col ? col : nullptr;
            a.gin = grad_input ? gin : nullptr;
            a.goff = grad_offset ? grad_offset + (size_t)g * 2 * kk * HoWo : nullptr;
            a.gmask = grad_mask ? grad_mask + (size_t)g * kk * HoWo : nullptr;
            a.goff_img = (long long)2 * kk * G * HoWo; a.gmask_img = (long long)kk * G * HoWo;
            a.P = (int)P; a.H = height; a.W = width; a.Ho = s.ho; a.Wo = s.wo; a.cp = s.cp; a.kh = kernel_h; a.kw = kernel_w;
            a.stride = stride_h; a.pad = pad_h; a.dil = dilation_h; a.om_cs = s.om_cs;
            hipLaunchKernelGGL(dcn_bwd_sample_kernel, dim3(cdiv(P, 4)), dim3(256), 0, stream, a);
            M3D_LAUNCH_CHECK();
        }
        if (grad_input) {
            hipLaunchKernelGGL(dcn_bwd_nhwc_to_nchw_slice_kernel, dim3(cdiv((long long)height * width, 32), cdiv(cg, 32), batch), dim3(256),
                               0, stream, gin, s.cp, grad_input, cg, height * width, channels, g * cg);
            M3D_LAUNCH_CHECK();
        }
        const bool want_bias = grad_bias && g == 0;
        if (need_col || want_bias) {
            const int ta = s.co_pad % 128 ? 2 : 4;
            const dim3 grid(need_col ? s.K / 64 : 1, s.co_pad / (32 * ta), s.splits);
#define M3D_WGRAD(TA_, DW_)                                                                                                   \
    hipLaunchKernelGGL((dcn_bwd_wgrad_kernel<TA_, DW_>), grid, dim3(64), 0, stream, go, s.co_pad, col, s.K, slab, bslab, s.co_pad, \
                       (int)P, s.chunk)
            if (ta == 4 && need_col) M3D_WGRAD(4, true);
            else if (ta == 4) M3D_WGRAD(4, false);
            else if (need_col) M3D_WGRAD(2, true);
            else M3D_WGRAD(2, false);
#undef M3D_WGRAD
            M3D_LAUNCH_CHECK();
            const long long total = (need_col ? (long long)channels_out * cg * kk : 0) + (want_bias ? channels_out : 0);
            hipLaunchKernelGGL(dcn_bwd_reduce_kernel, dim3(imin(cdiv(total, 256), 4096)), dim3(256), 0, stream, slab, bslab,
                               need_col ? grad_weight : nullptr, want_bias ? grad_bias : nullptr, s.splits, channels_out, s.co_pad, cg,
                               s.cp, kk, channels, g * cg);
            M3D_LAUNCH_CHECK();
        }
    }
    return M3D_OK;
}
