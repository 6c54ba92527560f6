// The DCNv2 operator on NCHW tensors, forward and backward, fp32 and bf16: the drop-ins for dcn_v2_cuda_forward
// (model/DCNv2/src/dcn_v2_cuda.c:10-102) and dcn_v2_cuda_backward (dcn_v2_cuda.c:104-241, kernels
// model/DCNv2/src/cuda/dcn_v2_im2col_cuda.cu:49-116,182-312), and the same operator on bf16 tensors: what a training loop under
// torch.autocast(dtype=bfloat16) reaches.  The fp32 and the bf16 backward are ONE driver, ONE workspace planner and ONE copy of
// the sampling, slab-reduce, weight-pack and slice-transpose kernels, instantiated on the element traits DcnF32 / DcnBf16; the two
// weight-gradient kernels and the two forward drivers share no logic and stay per type (see there).
//
// The mathematics of the backward is the analytic derivative of the forward as THIS library defines it, piecewise rule included:
// a sample at (h_im, w_im) contributes iff h_im > -1, w_im > -1, h_im < H, w_im < W, each of its four corners iff it lies inside
// the image, hl = floor(h_im), lh = h_im - hl; the sampling state comes from dcn_corners (common.h) in fp32 -- the same code the
// forward kernels of both types run, no lane masks in SGPRs.
//
// Forward, fp32: the reference loops over images on the host and round-trips a `columns` scratch through HBM; here the whole batch
// is one fused gather+GEMM launch per deformable group.  NCHW<->NHWC conversion and weight packing happen in the caller-provided
// workspace (the engine path keeps everything NHWC and skips them).
//
// Forward, bf16, per deformable group: NCHW bf16 -> NHWC bf16 (channels padded with zeros to what m3d_conv_bf16_forward needs: a
// power of two for kernels larger than 1x1, a multiple of 8 otherwise), weights packed [Cout_pad][Kpad], offsets / masks packed
// fp32 NHWC [3*kk], the implicit-GEMM deformable convolution on v_mfma_f32_32x32x16_bf16 writes fp32 NHWC (one buffer per group,
// bias in the first); one kernel adds the group buffers in group order, rounds once and writes bf16 NCHW.  The LDS-patch variant is
// not enabled: its rounding depends on the offset data.
//
// Backward, per deformable group (channel slice g of the input, offset / mask slice g, weights not grouped), everything NHWC inside:
//   1. gcol[p][k*C + c] = sum_co grad_out[p][co] * W[co][c][k]: a 1x1 convolution Co -> kk*C of grad_out on m3d_conv2d_forward
//      (bf16: m3d_conv_bf16_forward, fp32 NHWC output) with a pack of the transposed weight matrix (no new GEMM);
//   2. dcn_sample_kernel: one wave per output pixel, lane = channel.  Per tap it recomputes the corner state, reads gcol and
//      the four corner rows, and produces grad_mask[p][k] = sum_c gcol * val, grad_offset[p][2k], [2k+1] = mask * sum_c gcol *
//      d val / d(h, w) (butterfly reduction over the lanes: fixed order), col[p][k*C + c] = mask * val (the forward's A operand,
//      kept for step 3) and adds gcol * mask * w_q into the four corner rows of an fp32 NHWC staging buffer of grad_input with float
//      atomics: each atomic wave-instruction is 64 lanes x one channel = 256 contiguous bytes of one NHWC pixel row; one fp32
//      NHWC -> NCHW transpose (bf16: convert-transpose) finishes grad_input;
//   3. the weight-gradient GEMM: grad_weight[co][k*C + c] = sum_p grad_out[p][co] * col[p][k*C + c], dcn_bwd_wgrad_kernel on
//      v_mfma_f32_32x32x2_f32 or dcn16_wgrad_kernel on v_mfma_f32_32x32x16_bf16.  The reduction runs over pixels and the output is
//      tiny, so the pixel range is split over workgroups; every split writes a raw fp32 partial slab (grad_bias = pixel sums of
//      grad_out rides in the same launch), dcn_reduce_kernel adds the slabs in split order and scatters to the [Co][C][kh][kw]
//      layout.
// `col` is written once by the sampling kernel and read back by the weight-gradient GEMM (not gathered again in the operand
// load): the sampling kernel has every value in registers anyway (grad_mask needs val), and the GEMM stays a plain two-operand
// stream without sampling code in its loop.
//
// Types of the bf16 operator: input / weight / grad_output bf16, bias fp32, offset / mask fp32 or bf16 (widened: exact) and used as
// fp32.  Rounding points: the modulated sample mask * val -> bf16 once (the MFMA operand of the forward and of the weight
// gradient), products exact, accumulation fp32, bias added in fp32, output -> bf16 once; in the backward gcol stays fp32,
// grad_input is accumulated in fp32 with plain float atomics and rounded to bf16 once at the end, grad_weight is rounded to bf16
// once after the split-order reduction; grad_offset / grad_mask / grad_bias are fp32.  dilation must be 1 (the bf16 convolution
// descriptor has none).
//
// Determinism: grad_offset, grad_mask, grad_weight, grad_bias are bitwise reproducible (fixed reduction orders).  grad_input is
// accumulated with float atomics, as the reference does (dcn_v2_im2col_cuda.cu:234): its last bits depend on arrival order.
// m3d_dcn_v2_backward_det / _det_bf16 are the same driver and the same sampling code with a compile-time switch (DET) for the one
// step that differs, and make grad_input a function of the inputs alone -- the same bits on every launch, and for an image alone
// or inside any batch.  Contract and mechanism: each contribution gcol * mask * w_q, the fp32 value of the float form, is scaled by
// 2^s_n (exact), rounded to the nearest integer and added into a 64-bit integer staging buffer (integer addition is associative);
// the finish converts to fp32 (round to nearest), scales by 2^-s_n (exact) and, for bf16, rounds once more.  s_n = 62 - E -
// ceil(log2(Ho*Wo*kh*kw)) with 2^E > 2 A_n W_g M_n, from the order-independent maxima A_n = max |grad_out[n]|, W_g = max over
// (channel, tap) of sum_co |W|, M_n = max |mask[n, group]| (three small reduction kernels, read by the sampling kernel from the
// workspace: the host never sees s_n); DESIGN.md has the argument that no input can overflow the sum.  Resolution: 2^-s_n, 45 bits
// below 2^E on a 48x160 map with a 3x3 kernel.  Non-finite rule (the difference from the float form): a NaN / infinity in grad_out[n],
// the weights or the masks of image n (or a bound of 2^126 and more) makes the whole grad_input of that image and group NaN; a zero
// bound gives zeros; non-finite offsets are dcn_corners' business in both forms.  Measured cost (MI355X, bs 8,
// profiles/dcn_backward_det_bench.jsonl): the full call takes 1.39x to 1.56x the float form in fp32, 1.66x to 2.04x in bf16; the
// 64-bit atomics move twice the bytes at the byte rate of the fp32 ones.  With torch.use_deterministic_algorithms set the host
// layer takes this form (ops.set_dcn_deterministic), and every HIP operator of the training step is then bitwise reproducible.
// Every non-NULL gradient is OVERWRITTEN (the reference accumulates into grad_weight / grad_bias and adds into a zeroed
// grad_input); a NULL gradient pointer = not wanted, and the work only it needs is skipped.
#include <limits.h>
#include <string.h>

#include "common.h"

#include "bf16_tile.h"

typedef unsigned short u16;
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));

static inline long long rup(long long a, long long b) { return (a + b - 1) / b * b; }

__device__ __forceinline__ float bf16_bits_to_f32(u16 v) { return __uint_as_float((unsigned)v << 16); }
__device__ __forceinline__ u16 f32_to_bf16_bits(float v) { return (u16)(pack_bf16(v, 0.f) & 0xFFFFu); }   // round to nearest even

// ------------------------------------------------------------------------------------------------------------------------
// Element traits: what the shared kernels, the backward's workspace planner and its driver need to know about the type of
// input / weight / grad_output / col / grad_input / grad_weight.  store() is the one rounding of a stored value.
struct DcnF32 {
    typedef float T;
    static constexpr bool is_bf16 = false;
    static constexpr int size = 4;
    static constexpr int split_granule = 2;                 // pixels one v_mfma_f32_32x32x2_f32 consumes
    static constexpr int wgrad_rows(int co_pad) { return co_pad % 128 ? 64 : 128; }   // rows (co) of a weight-gradient tile
    static constexpr long long max_in_elems = 1ll << 31, max_go_elems = LLONG_MAX;    // NHWC input / grad_out elements
    static constexpr const char *bwd_name = "dcn_v2_backward", *bwd_query = "m3d_dcn_v2_backward_workspace_bytes";
    static constexpr const char *det_name = "dcn_v2_backward_det", *det_query = "m3d_dcn_v2_backward_det_workspace_bytes";
    static __device__ __forceinline__ float load(float v) { return v; }
    static __device__ __forceinline__ float store(float v) { return v; }
};
struct DcnBf16 {
    typedef u16 T;
    static constexpr bool is_bf16 = true;
    static constexpr int size = 2;
    static constexpr int split_granule = 32;                // pixels of one LDS tile of dcn16_wgrad_kernel
    static constexpr int wgrad_rows(int) { return 64; }
    static constexpr long long max_in_elems = 1ll << 30, max_go_elems = 1ll << 30;
    static constexpr const char *bwd_name = "dcn_v2_backward_bf16", *bwd_query = "m3d_dcn_v2_backward_workspace_bytes_bf16";
    static constexpr const char *det_name = "dcn_v2_backward_det_bf16", *det_query = "m3d_dcn_v2_backward_det_workspace_bytes_bf16";
    static __device__ __forceinline__ float load(u16 v) { return bf16_bits_to_f32(v); }
    static __device__ __forceinline__ u16 store(float v) { return f32_to_bf16_bits(v); }
};

// ------------------------------------------------------------------------------------------------------------------------
// The argument rules of the four entry points.  `ptrs_ok`: every pointer the entry requires is non-NULL; `shape_ok`: its shape
// rule (dcn_shape_ok; the fp32 forward has none and passes true).
static bool dcn_shape_ok(bool bf16, int n, int c, int h, int w, int co, int kh, int kw, int stride, int pad, int dil)
{
    return n > 0 && c > 0 && h > 0 && w > 0 && co > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0 && (bf16 ? kh * kw <= 9 : dil > 0);
}

static int dcn_check_args(const char *name, bool bf16, bool ptrs_ok, bool shape_ok, int channels, int deformable_group, int stride_h,
                          int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, const void *workspace)
{
    M3D_REQUIRE(ptrs_ok, "%s: null pointer", name);
    M3D_REQUIRE(shape_ok, "%s: bad shape", name);
    M3D_REQUIRE(deformable_group >= 1 && channels % deformable_group == 0, "%s: deformable_group (%d) must divide the input channels (%d)",
                name, deformable_group, channels);
    M3D_REQUIRE(stride_h == stride_w && pad_h == pad_w && dilation_h == dilation_w, "%s: anisotropic stride/pad/dilation not supported",
                name);
    M3D_REQUIRE(!bf16 || dilation_h == 1, "%s: the bf16 path supports dilation 1 only (got %d); use float32 tensors for a dilated layer",
                name, dilation_h);
    M3D_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", name);
    return M3D_OK;
}

static int dcn_check_workspace(const char *name, const char *query, long long have, long long need)
{
    if (have >= need) return M3D_OK;
    m3d_set_error("%s: workspace %lld < %lld bytes (%s)", name, have, need, query);
    return M3D_E_WORKSPACE;
}

// what the workspace queries of the backward (both types) and of the bf16 forward accept
static bool dcn_query_ok(bool bf16, int n, int c, int h, int w, int co, int kh, int kw, int stride, int pad, int dil, int G)
{
    return G >= 1 && c >= 1 && c % G == 0 && dcn_shape_ok(bf16, n, c, h, w, co, kh, kw, stride, pad, dil) && (!bf16 || dil == 1);
}

// ------------------------------------------------------------------------------------------------------------------------
// channel slice [c0, c0 + C) of a bf16 NCHW tensor with Ctot channels -> bf16 NHWC [N*HW][cs]; channels [C, cs) are written as zeros
__global__ void dcn16_nchw_to_nhwc_kernel(const u16 *__restrict__ in, u16 *__restrict__ out, int C, int HW, int Ctot, int c0s, int cs)
{
    __shared__ u16 t[32][33];
    const int n = blockIdx.z, c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, p = p0 + tx;
        t[r][tx] = (c < C && p < HW) ? in[((size_t)n * Ctot + c0s + c) * HW + p] : (u16)0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + r, c = c0 + tx;
        if (c < cs && p < HW) out[((size_t)n * HW + p) * cs + c] = t[tx][r];
    }
}

// the sum, in buffer order, of `nsum` fp32 NHWC buffers [N*HW][in_cs] (`sum_stride` floats apart) -> channel slice [c0s, c0s + C)
// of an NCHW tensor with Ctot channels, through a 32x32 LDS tile: one rounding to the stored type
template <class E>
__global__ void dcn_nhwc_f32_to_nchw_kernel(const float *__restrict__ in, int in_cs, int nsum, long long sum_stride,
                                            typename E::T *__restrict__ out, int C, int HW, int Ctot, int c0s)
{
    __shared__ float t[32][33];
    const int n = blockIdx.z, c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + r, c = c0 + tx;
        float v = 0.f;
        if (c < C && p < HW) {
            const size_t i = ((size_t)n * HW + p) * in_cs + c;
            v = in[i];
            for (int s = 1; s < nsum; ++s) v += in[i + (size_t)s * sum_stride];
        }
        t[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, p = p0 + tx;
        if (c < C && p < HW) out[((size_t)n * Ctot + c0s + c) * HW + p] = E::store(t[tx][r]);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// The deterministic grad_input (m3d_dcn_v2_backward_det*): 64-bit fixed point with one binary exponent per image.
//
// sexp[n] = s_n: a contribution v (fp32) enters the sum as rint(v * 2^s_n), the finished element is fp32(sum) * 2^-s_n.  One value of
// sexp[n] is no exponent: DCN_SEXP_NAN = the bound of image n is not finite, its grad_input is NaN, nothing is added.
#define DCN_SEXP_NAN INT_MIN

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }
__device__ __forceinline__ float dcn_widen(float v) { return v; }
__device__ __forceinline__ float dcn_widen(u16 v) { return bf16_bits_to_f32(v); }

__device__ __forceinline__ unsigned wave_max_u32(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off));
    return v;
}

// out[n] = max over rows r < rows, channels [c0, c0 + cn) of |src[(n*rows + r)*cs + c]| as the BIT PATTERN of the absolute value:
// unsigned order is the order of the magnitudes, an infinity lies above every finite value and a NaN above the infinity, so the
// maximum both finds the largest magnitude and keeps a NaN.  A maximum does not depend on the order it is taken in (the atomic
// is an integer maximum).  out[] zeroed by the caller.
template <class T>
__global__ __launch_bounds__(256) void dcn_absmax_kernel(const T *__restrict__ src, int rows, int cs, int c0, int cn,
                                                         unsigned *__restrict__ out)
{
    const int n = blockIdx.y;
    const long long total = (long long)rows * cn;
    const T *img = src + (size_t)n * rows * cs + c0;
    unsigned m = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cn;
        m = max(m, abs_bits(dcn_widen(img[r * cs + (i - r * cn)])));
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0) atomicMax(out + n, m);
}

// out[0] = max over the rows (tap, channel) of the transposed weight pack [rows][cs] of sum_co |p[row][co]| (bit pattern, as above);
// one wave per row, fixed summation order
template <class T>
__global__ __launch_bounds__(256) void dcn_wsum_max_kernel(const T *__restrict__ p, int rows, int cs, unsigned *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float s = 0.f;
    for (int c = lane; c < cs; c += 64) s += fabsf(dcn_widen(p[(size_t)row * cs + c]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) atomicMax(out, abs_bits(s));
}

// sexp[n] from A_n = amax[n] (grad_out), M_n = mmax[n] (masks of this group), W_g = wmax[0]; log2T = ceil(log2(Ho*Wo*kh*kw)).
// Bound of one contribution: |gcol * mask * w_q| <= A W M in exact arithmetic; the GEMM, the weight sums and the two products round,
// each by a relative 2^-24 per term, which one spare bit covers: with 2^e > A W M every contribution is below 2^(e + 1) = 2^E.
// The product is formed in double (no overflow, no underflow); E > 127 counts as not finite (fp32 gcol may have overflowed).
__global__ void dcn_sexp_kernel(const unsigned *__restrict__ amax, const unsigned *__restrict__ mmax, const unsigned *__restrict__ wmax,
                                int *__restrict__ sexp, int N, int log2T)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const unsigned a = amax[n], m = mmax[n], w = wmax[0];
    int s;
    if (a >= 0x7F800000u || m >= 0x7F800000u || w >= 0x7F800000u) {
        s = DCN_SEXP_NAN;
    } else {
        const double b = (double)__uint_as_float(a) * (double)__uint_as_float(m) * (double)__uint_as_float(w);
        if (b == 0.0) {
            s = 0;                                               // every contribution is zero
        } else {
            const int E = ilogb(b) + 2;
            s = E > 127 ? DCN_SEXP_NAN : 62 - E - log2T;
        }
    }
    sexp[n] = s;
}

// 64-bit sums [N*HW][in_cs] -> channel slice [c0s, c0s + C) of an NCHW tensor with Ctot channels: fp32(sum) * 2^-sexp[n] (the
// conversion rounds to nearest, the scaling is exact), one more rounding to the stored type for bf16; NaN where sexp[n] says so
template <class E>
__global__ void dcn_nhwc_i64_to_nchw_kernel(const long long *__restrict__ in, int in_cs, const int *__restrict__ sexp,
                                            typename E::T *__restrict__ out, int C, int HW, int Ctot, int c0s)
{
    __shared__ float t[32][33];
    const int n = blockIdx.z, c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int s = sexp[n];
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + r, c = c0 + tx;
        float v = 0.f;
        if (c < C && p < HW)
            v = s == DCN_SEXP_NAN ? __uint_as_float(0x7FC00000u) : ldexpf(__ll2float_rn(in[((size_t)n * HW + p) * in_cs + c]), -s);
        t[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, p = p0 + tx;
        if (c < C && p < HW) out[((size_t)n * Ctot + c0s + c) * HW + p] = E::store(t[tx][r]);
    }
}

// offset channels [g*2kk, (g+1)*2kk) and mask channels [g*kk, (g+1)*kk) of NCHW tensors (fp32 or bf16) -> fp32 NHWC [P][om_cs]:
// 2k = dh, 2k + 1 = dw, 2kk + k = mask, the padding channels zero
__global__ void dcn16_pack_om_kernel(const void *__restrict__ off, int off_bf16, const void *__restrict__ mask, int mask_bf16,
                                     float *__restrict__ om, int N, int HoWo, int kk, int G, int g, int om_cs)
{
    const long long total = (long long)N * om_cs * HoWo;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int pix = (int)(i % HoWo);
        const int ch = (int)((i / HoWo) % om_cs);
        const int n = (int)(i / ((long long)HoWo * om_cs));
        float v = 0.f;
        if (ch < 2 * kk) {
            const size_t s = ((size_t)n * 2 * kk * G + (size_t)g * 2 * kk + ch) * HoWo + pix;
            v = off_bf16 ? bf16_bits_to_f32(((const u16 *)off)[s]) : ((const float *)off)[s];
        } else if (ch < 3 * kk) {
            const size_t s = ((size_t)n * kk * G + (size_t)g * kk + (ch - 2 * kk)) * HoWo + pix;
            v = mask_bf16 ? bf16_bits_to_f32(((const u16 *)mask)[s]) : ((const float *)mask)[s];
        }
        om[((size_t)n * HoWo + pix) * om_cs + ch] = v;
    }
}

// [Co, Ctot, kh, kw] bf16 (channel slice [c0, c0 + C)) -> the forward's [co_pad][Kpad] with K index k*Cp + c (zero padded)
__global__ void dcn16_pack_w_kernel(const u16 *__restrict__ w, u16 *__restrict__ p, int Co, int co_pad, int C, int Cp, int KK, int Kpad,
                                    int Ctot, int c0)
{
    const long long total = (long long)co_pad * Kpad;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int kc = (int)(i % Kpad), co = (int)(i / Kpad);
        const int k = kc / Cp, c = kc - k * Cp;
        p[i] = (co < Co && k < KK && c < C) ? w[((size_t)co * Ctot + c0 + c) * KK + k] : (u16)0;
    }
}

// [Co, Ctot, kh, kw] (channel slice [c0, c0 + C)) -> the packed weights of the 1x1 convolution that yields gcol:
// p[(k*Cp + c)][co] with row length cs (rows of padded channels and columns >= Co are zero)
template <class E>
__global__ void dcn_pack_wt_kernel(const typename E::T *__restrict__ w, typename E::T *__restrict__ p, int Co, int cs, int C, int Cp,
                                   int KK, int Ctot, int c0)
{
    typedef typename E::T T;
    const long long total = (long long)KK * Cp * cs;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int co = (int)(i % cs);
        const int c = (int)((i / cs) % Cp);
        const int k = (int)(i / ((long long)cs * Cp));
        p[i] = (co < Co && c < C) ? w[((long long)co * Ctot + c0 + c) * KK + k] : (T)0;
    }
}

// ================================================================================================== forward, fp32
struct DcnWs {
    long long in_off, om_off, w_off, out_off, out2_off, total;
    int cp, co_pad, om_cs, out_cs, ho, wo;
};

// `c` = channels of ONE deformable group (the whole input when deformable_group == 1); groups > 1 add a second output
// buffer: group g accumulates onto group g-1's result through the residual input of the conv epilogue (ping-pong).
static DcnWs dcn_ws(int n, int c, int h, int w, int co, int kh, int kw, int stride, int pad, int dil, int groups)
{
    DcnWs s;
    s.cp = (int)rup(c, 32);   // deformable tiles use BK = 32
    s.co_pad = (int)rup(co, 64);
    s.ho = (h + 2 * pad - (dil * (kh - 1) + 1)) / stride + 1;
    s.wo = (w + 2 * pad - (dil * (kw - 1) + 1)) / stride + 1;
    s.om_cs = (int)rup(3 * kh * kw, 4);
    s.out_cs = (int)rup(co, 4);
    long long o = 0;
    s.in_off = o;  o += rup((long long)n * h * w * s.cp * 4, 256);
    s.om_off = o;  o += rup((long long)n * s.ho * s.wo * s.om_cs * 4, 256);
    s.w_off = o;   o += rup((long long)s.co_pad * kh * kw * s.cp * 4, 256);
    s.out_off = o; o += rup((long long)n * s.ho * s.wo * s.out_cs * 4, 256);
    s.out2_off = o;
    if (groups > 1) o += rup((long long)n * s.ho * s.wo * s.out_cs * 4, 256);
    s.total = o;
    return s;
}

extern "C" long long m3d_dcn_v2_workspace_bytes(int batch, int channels, int height, int width, int channels_out,
                                                int kernel_h, int kernel_w, int stride, int pad, int dilation)
{
    return dcn_ws(batch, channels, height, width, channels_out, kernel_h, kernel_w, stride, pad, dilation, 1).total;
}

extern "C" long long m3d_dcn_v2_workspace_bytes_grouped(int batch, int channels, int height, int width, int channels_out,
                                                        int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                                        int deformable_group)
{
    if (deformable_group < 1 || channels % deformable_group) return -1;
    return dcn_ws(batch, channels / deformable_group, height, width, channels_out, kernel_h, kernel_w, stride, pad, dilation,
                  deformable_group).total;
}

extern "C" int m3d_dcn_v2_forward(const float *input, const float *weight, const float *bias, const float *offset,
                                  const float *mask, float *output, int batch, int channels, int height, int width,
                                  int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h,
                                  int pad_w, int dilation_h, int dilation_w, int deformable_group, void *workspace,
                                  long long workspace_bytes, m3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    int rc;
    if ((rc = dcn_check_args("dcn_v2_forward", false, input && weight && bias && offset && mask && output && workspace, true, channels,
                             deformable_group, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, workspace)))
        return rc;
    const int G = deformable_group, cg = channels / G;
    const DcnWs s = dcn_ws(batch, cg, height, width, channels_out, kernel_h, kernel_w, stride_h, pad_h, dilation_h, G);
    if ((rc = dcn_check_workspace("dcn_v2_forward", G > 1 ? "m3d_dcn_v2_workspace_bytes_grouped" : "m3d_dcn_v2_workspace_bytes",
                                  workspace_bytes, s.total)))
        return rc;
    M3D_REQUIRE(s.ho > 0 && s.wo > 0, "dcn_v2_forward: empty output");
    char *ws = (char *)workspace;
    float *in_nhwc = (float *)(ws + s.in_off), *om = (float *)(ws + s.om_off);
    float *wp = (float *)(ws + s.w_off);
    float *outs[2] = {(float *)(ws + s.out_off), (float *)(ws + s.out2_off)};
    const int kk = kernel_h * kernel_w;
    // Deformable group g (dcn_v2_im2col_cuda.cu:139-156): input channels [g*cg, (g+1)*cg) are sampled at the positions of
    // offset channels [g*2kk, (g+1)*2kk) with mask channels [g*kk, (g+1)*kk); the weights are not grouped, so the output
    // is the sum over g of a deformable conv of that channel slice with weight[:, g*cg:(g+1)*cg] -- one fused gather + GEMM
    // launch per group, accumulated through the epilogue's residual input, bias added once.
    for (int g = 0; g < G; ++g) {
        if (s.cp != cg) M3D_HIP(hipMemsetAsync(in_nhwc, 0, (size_t)batch * height * width * s.cp * 4, stream));
        if ((rc = m3d_nchw_to_nhwc_slice(input, channels, g * cg, in_nhwc, batch, cg, height, width, s.cp, stream))) return rc;
        if ((rc = m3d_nchw_to_nhwc_slice(offset, 2 * kk * G, g * 2 * kk, om, batch, 2 * kk, s.ho, s.wo, s.om_cs, stream))) return rc;
        if ((rc = m3d_nchw_to_nhwc_slice(mask, kk * G, g * kk, om + 2 * kk, batch, kk, s.ho, s.wo, s.om_cs, stream))) return rc;
        if ((rc = m3d_pack_conv_weight_slice(weight, channels, g * cg, wp, channels_out, s.co_pad, cg, s.cp, kernel_h, kernel_w,
                                             stream)))
            return rc;
        m3d_conv_desc d;
        memset(&d, 0, sizeof(d));
        d.in = in_nhwc; d.in_cs = s.cp; d.N = batch; d.H = height; d.W = width; d.Cin = s.cp;
        d.wgt = wp; d.Cout = channels_out; d.Cout_pad = s.co_pad;
        d.kh = kernel_h; d.kw = kernel_w; d.stride = stride_h; d.pad = pad_h; d.dil = dilation_h;
        d.Ho = s.ho; d.Wo = s.wo; d.out = outs[g & 1]; d.out_cs = s.out_cs;
        d.shift = g == 0 ? bias : nullptr;   // bias GEMM-with-ones of dcn_v2_cuda.c:72-78 folded into the epilogue
        if (g > 0) { d.res = outs[(g - 1) & 1]; d.res_cs = s.out_cs; d.res_mode = 0; }
        d.sigmoid_from = -1;
        d.dcn_offmask = om; d.dcn_om_cs = s.om_cs;
        if ((rc = m3d_conv2d_forward(&d, stream))) return rc;
    }
    return m3d_nhwc_to_nchw(outs[(G - 1) & 1], s.out_cs, output, batch, channels_out, s.ho, s.wo, stream);
}

// ================================================================================================== forward, bf16
// (its own driver: the groups are summed from per-group fp32 buffers at the end, not through the epilogue's residual input)
struct Dcn16FwdWs {
    long long in_off, om_off, w_off, out_off, out_stride, total;
    int cp, co_pad, kpad, om_cs, out_cs, ho, wo;
};

// `c` = channels of ONE deformable group
static Dcn16FwdWs dcn16_fwd_ws(int n, int c, int h, int w, int co, int kh, int kw, int stride, int pad, int G)
{
    Dcn16FwdWs s;
    if (kh * kw == 1) s.cp = (int)rup(c, 8);
    else { s.cp = 8; while (s.cp < c) s.cp *= 2; }          // a kernel larger than 1x1 needs a power-of-two Cin
    s.co_pad = (int)rup(co, 32);
    s.kpad = (int)rup((long long)kh * kw * s.cp, 64);
    s.ho = (h + 2 * pad - kh) / stride + 1;
    s.wo = (w + 2 * pad - kw) / stride + 1;
    s.om_cs = (int)rup(3 * kh * kw, 4);
    s.out_cs = (int)rup(co, 4);
    const long long P = (long long)n * (s.ho > 0 ? s.ho : 0) * (s.wo > 0 ? s.wo : 0);
    long long o = 0;
    s.in_off = o;  o += rup((long long)n * h * w * s.cp * 2, 256);
    s.om_off = o;  o += rup(P * s.om_cs * 4, 256);
    s.w_off = o;   o += rup((long long)s.co_pad * s.kpad * 2, 256);
    s.out_stride = rup(P * s.out_cs * 4, 256) / 4;         // floats between the group buffers
    s.out_off = o; o += s.out_stride * 4 * G;
    s.total = o;
    return s;
}

extern "C" long long m3d_dcn_v2_workspace_bytes_bf16(int batch, int channels, int height, int width, int channels_out, int kernel_h,
                                                     int kernel_w, int stride, int pad, int dilation, int deformable_group)
{
    if (!dcn_query_ok(true, batch, channels, height, width, channels_out, kernel_h, kernel_w, stride, pad, dilation, deformable_group))
        return -1;
    return dcn16_fwd_ws(batch, channels / deformable_group, height, width, channels_out, kernel_h, kernel_w, stride, pad, deformable_group).total;
}

extern "C" int m3d_dcn_v2_forward_bf16(const void *input, const void *weight, const float *bias, const void *offset, int offset_is_bf16,
                                       const void *mask, int mask_is_bf16, void *output, int batch, int channels, int height, int width,
                                       int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                       int dilation_h, int dilation_w, int deformable_group, void *workspace, long long workspace_bytes,
                                       m3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    int rc;
    if ((rc = dcn_check_args("dcn_v2_forward_bf16", true, input && weight && bias && offset && mask && output && workspace,
                             dcn_shape_ok(true, batch, channels, height, width, channels_out, kernel_h, kernel_w, stride_h, pad_h, dilation_h),
                             channels, deformable_group, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, workspace)))
        return rc;
    const int G = deformable_group, cg = channels / G, kk = kernel_h * kernel_w;
    const Dcn16FwdWs s = dcn16_fwd_ws(batch, cg, height, width, channels_out, kernel_h, kernel_w, stride_h, pad_h, G);
    if ((rc = dcn_check_workspace("dcn_v2_forward_bf16", "m3d_dcn_v2_workspace_bytes_bf16", workspace_bytes, s.total))) return rc;
    M3D_REQUIRE(s.ho > 0 && s.wo > 0, "dcn_v2_forward_bf16: empty output");
    const int HW = height * width, HoWo = s.ho * s.wo;
    const long long P = (long long)batch * HoWo;
    M3D_REQUIRE(P < (1ll << 29) && (long long)batch * HW * s.cp < (1ll << 30), "dcn_v2_forward_bf16: tensor too large");
    char *ws = (char *)workspace;
    u16 *in_nhwc = (u16 *)(ws + s.in_off), *wp = (u16 *)(ws + s.w_off);
    float *om = (float *)(ws + s.om_off), *outs = (float *)(ws + s.out_off);
    for (int g = 0; g < G; ++g) {
        hipLaunchKernelGGL(dcn16_nchw_to_nhwc_kernel, dim3(cdiv(HW, 32), cdiv(s.cp, 32), batch), dim3(256), 0, stream, (const u16 *)input,
                           in_nhwc, cg, HW, channels, g * cg, s.cp);
        M3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(dcn16_pack_om_kernel, dim3(imin(cdiv(P * s.om_cs, 256), 4096)), dim3(256), 0, stream, offset, offset_is_bf16, mask,
                           mask_is_bf16, om, batch, HoWo, kk, G, g, s.om_cs);
        M3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(dcn16_pack_w_kernel, dim3(imin(cdiv((long long)s.co_pad * s.kpad, 256), 4096)), dim3(256), 0, stream,
                           (const u16 *)weight, wp, channels_out, s.co_pad, cg, s.cp, kk, s.kpad, channels, g * cg);
        M3D_LAUNCH_CHECK();
        m3d_conv_bf16_desc d;
        memset(&d, 0, sizeof(d));
        d.in = in_nhwc; d.in_cs = s.cp; d.N = batch; d.H = height; d.W = width; d.Cin = s.cp;
        d.wgt = wp; d.Cout = channels_out; d.Cout_pad = s.co_pad; d.Kpad = s.kpad;
        d.kh = kernel_h; d.kw = kernel_w; d.stride = stride_h; d.pad = pad_h;
        d.Ho = s.ho; d.Wo = s.wo; d.out = outs + (size_t)g * s.out_stride; d.out_cs = s.out_cs; d.out_mode = 1;
        d.shift = g == 0 ? bias : nullptr;
        d.sigmoid_from = -1;
        d.dcn_offmask = om; d.dcn_om_cs = s.om_cs;
        d.groups = 1;
        if ((rc = m3d_conv_bf16_forward(&d, stream))) return rc;
    }
    hipLaunchKernelGGL(dcn_nhwc_f32_to_nchw_kernel<DcnBf16>, dim3(cdiv(HoWo, 32), cdiv(channels_out, 32), batch), dim3(256), 0, stream, outs,
                       s.out_cs, G, s.out_stride, (u16 *)output, channels_out, HoWo, channels_out, 0);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

// ================================================================================================== backward: the sampling kernel
template <class E>
struct DcnSampleArgs {
    const typename E::T *in;   // [N*H*W][cp], channels >= C zero
    const float *om;           // [P][om_cs]: 2k = dh, 2k+1 = dw, 2kk + k = mask
    const float *gcol;         // fp32 [P][kk*cp] or NULL (then only col is produced)
    typename E::T *col;        // [P][kk*cp] or NULL
    float *gin;                // fp32 [N*H*W][cp], zeroed, or NULL; the deterministic form: long long [N*H*W][cp], zeroed
    float *goff, *gmask;       // fp32 NCHW, already moved to this group's first channel, or NULL
    long long goff_img, gmask_img;   // floats between images of goff / gmask
    int P, H, W, Ho, Wo, cp, kh, kw, stride, pad, dil, om_cs;
    const int *sexp;           // the deterministic form: [N], the fixed-point exponent of each image (DCN_SEXP_NAN: add nothing)
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
// (readfirstlane + scalar branch), not through a lane mask.  Everything after the load of a corner value and before the store
// of col is fp32 whatever the element type.
// DET (a compile-time choice: the float form carries no trace of it): the contribution gm * w_q, the same fp32 value, is scaled by
// 2^sexp[n] (exact), rounded to the nearest integer and added with a 64-bit integer atomic -- integer addition is associative, so
// the sum does not depend on arrival order.  One atomic wave-instruction is 64 lanes x 8 bytes = 512 contiguous bytes.
template <class E, bool DET>
__global__ __launch_bounds__(256) void dcn_sample_kernel(DcnSampleArgs<E> a)
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
    const typename E::T *inb = a.in + img;
    int sn = 0;
    if constexpr (DET) sn = a.gin ? __builtin_amdgcn_readfirstlane(a.sexp[n]) : 0;
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
            for (int q = 0; q < 4; ++q) v[q] = and_not(E::load(inb[row[q] + c]), drop[q]);
            const float val = w[0] * v[0] + w[1] * v[1] + w[2] * v[2] + w[3] * v[3];
            const size_t ci = (size_t)p * K + (size_t)k * a.cp + c;
            if (a.col) a.col[ci] = E::store(mk * val);
            if (a.gcol) {
                const float g = a.gcol[ci];
                sm += g * val;
                sh += g * (dwh[0] * v[0] + dwh[1] * v[1] + dwh[2] * v[2] + dwh[3] * v[3]);
                sw += g * (dww[0] * v[0] + dww[1] * v[1] + dww[2] * v[2] + dww[3] * v[3]);
                if (a.gin) {
                    const float gm = g * mk;
                    if constexpr (DET) {
                        unsigned long long *gb = (unsigned long long *)a.gin + img + c;
                        if (sn != DCN_SEXP_NAN) {
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                if (keep[q]) atomicAdd(gb + row[q], (unsigned long long)__float2ll_rn(ldexpf(gm * w[q], sn)));
                        }
                    } else {
                        float *gb = a.gin + img + c;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (keep[q]) atomicAdd(gb + row[q], gm * w[q]);
                    }
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

// ================================================================================================== backward: the weight gradient
// The two weight-gradient kernels share no logic (fp32 operands come straight from global memory, two pixels per MFMA; bf16
// operands need a transposing read through LDS, 16 pixels per MFMA) and stay separate.
//
// fp32.  grad_weight partials: D[co][kc] = sum over the pixels of one split of go[p][co] * col[p][kc].  One wave per workgroup
// owns a (32 * TA) x 64 tile of D; one v_mfma_f32_32x32x2_f32 consumes two pixels (A = go^T: row co = lane % 32, k = lane / 32;
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

// bf16.  The same partials on v_mfma_f32_32x32x16_bf16.  The reduction index is the pixel and both operands are pixel-major, so
// the eight consecutive K elements of a lane are strided in memory.  One wave per workgroup owns a 64 x 64 tile of D.  A step takes
// 32 pixels: their 64-channel row segments of go and col (128 bytes each) go to LDS as they lie, [pixel][channel] with a row stride
// of 192 bytes, and both MFMA operands (A = go^T: row co = lane % 32; B = col: column kc = lane % 32; k = pixel 8 * (lane / 32) + e)
// come back through ds_read_b64_tr_b16: per group of 16 lanes a block of 4 pixels x 16 channels, lane 4q + r of the group supplies
// the address of pixel q, channels 4r .. 4r + 3, lane i receives channel i of the 4 pixels.  With the 192-byte stride the 8 row
// segments a 32-lane half reads (4 pixels x 2 channel blocks of 32 bytes) fall on disjoint banks.  Every lane takes part in every
// transposed read with an in-tile address (the tile is always complete: pixels past the end of the split are staged as zeros), EXEC
// is all ones there, and the static tile is 16-byte aligned.
// The pixel sums of go (grad_bias) ride along in the workgroups of the first column block.  DW == false: bias sums only.
#define DCN16_RS 96          // LDS row stride in bf16 elements
__device__ __forceinline__ bf16x8 dcn16_tr_frag(const u16 *tile_base)
{
    typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
    const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)tile_base);
    const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)(tile_base + 4 * DCN16_RS));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <bool DW>
__global__ __launch_bounds__(64) void dcn16_wgrad_kernel(const u16 *__restrict__ go, int go_cs, const u16 *__restrict__ col, int K,
                                                         float *__restrict__ slab, float *__restrict__ bslab, int co_pad, int P, int chunk)
{
    __shared__ __attribute__((aligned(16))) u16 tile[2][32 * DCN16_RS];
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    const int kc0 = blockIdx.x * 64, co0 = blockIdx.y * 64, s = blockIdx.z;
    const int p_beg = s * chunk, p_end = min(P, p_beg + chunk);
    // transposed-read address of this lane inside a 16-pixel x 32-channel fragment (elements)
    const int grp = lane >> 4, li = lane & 15;
    const int tr_off = (8 * (grp >> 1) + (li >> 2)) * DCN16_RS + 16 * (grp & 1) + 4 * (li & 3);
    f32x16 acc[2][2];
    float bsum[2] = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
    const bool want_bias = blockIdx.x == 0;
    for (int pp = p_beg; pp < p_end; pp += 32) {
        u32x4 ra[4], rb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int id = j * 64 + lane, row = id >> 3, ch = id & 7;
            const int p = pp + row;
            const bool ok = p < p_end;                   // past the end of the split: the operand is zero (row p_beg is read)
            const size_t pc = (size_t)(ok ? p : p_beg);
            const u32x4 zero = {0u, 0u, 0u, 0u};
            const u32x4 g = *reinterpret_cast<const u32x4 *>(go + pc * go_cs + co0 + ch * 8);
            ra[j] = ok ? g : zero;
            if constexpr (DW) {
                const u32x4 c = *reinterpret_cast<const u32x4 *>(col + pc * K + kc0 + ch * 8);
                rb[j] = ok ? c : zero;
            } else {
                rb[j] = zero;
            }
        }
        __syncthreads();                                 // the reads of the previous step are done
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int id = j * 64 + lane, row = id >> 3, ch = id & 7;
            *reinterpret_cast<u32x4 *>(&tile[0][row * DCN16_RS + ch * 8]) = ra[j];
            if constexpr (DW) *reinterpret_cast<u32x4 *>(&tile[1][row * DCN16_RS + ch * 8]) = rb[j];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) fa[t] = dcn16_tr_frag(&tile[0][ks * 16 * DCN16_RS + 32 * t + tr_off]);
            if constexpr (DW) {
#pragma unroll
                for (int u = 0; u < 2; ++u) fb[u] = dcn16_tr_frag(&tile[1][ks * 16 * DCN16_RS + 32 * u + tr_off]);
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int u = 0; u < 2; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[t], fb[u], acc[t][u], 0, 0, 0);
            }
            if (want_bias) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int e = 0; e < 8; ++e) bsum[t] += (float)fa[t][e];
            }
        }
    }
    if constexpr (DW) {
        // D layout of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
                    slab[((size_t)s * co_pad + co) * K + kc0 + 32 * u + l31] = acc[t][u][r];
                }
    }
    if (want_bias) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float b = bsum[t] + __shfl_xor(bsum[t], 32);
            if (half == 0) bslab[(size_t)s * co_pad + co0 + 32 * t + l31] = b;
        }
    }
}

// slabs added in split order; grad_weight element (co, c0 + c, k) <- column k*cp + c, rounded once to the stored type;
// grad_bias[co] <- the bias slabs, fp32
template <class E>
__global__ void dcn_reduce_kernel(const float *__restrict__ slab, const float *__restrict__ bslab, typename E::T *__restrict__ gw,
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
            gw[((size_t)co * Ctot + c0 + c) * KK + k] = E::store(acc);
        } else {
            const int co = (int)(i - nw);
            float acc = 0.f;
            for (int s = 0; s < splits; ++s) acc += bslab[(size_t)s * co_pad + co];
            gb[co] = acc;
        }
    }
}

// ================================================================================================== backward: workspace
struct DcnBwdWs {
    long long in_off, om_off, go_off, wt_off, gcol_off, col_off, gin_off, slab_off, bslab_off, stat_off, total;
    int cp, co_pad, om_cs, ho, wo, K, splits, chunk;
};

// `c` = channels of ONE deformable group.  The layout does not depend on which gradients are wanted.  in / go / wt / col hold
// elements of the operator's type; om, gcol, the grad_input staging buffer and the slabs are fp32.  `det`: the staging buffer holds
// 64-bit sums and a last region holds the statistics of the exponent: amax[n], mmax[n], wmax[1] (unsigned), sexp[n] (int).
template <class E>
static DcnBwdWs dcn_bwd_ws(int n, int c, int h, int w, int co, int kh, int kw, int stride, int pad, int dil, bool det)
{
    DcnBwdWs s;
    s.cp = (int)rup(c, 64);          // the sampling kernel runs whole waves of 64 channels
    s.co_pad = (int)rup(co, 64);     // channel stride of grad_out NHWC = K of the gcol GEMM = row count of a slab
    s.ho = (h + 2 * pad - (dil * (kh - 1) + 1)) / stride + 1;
    s.wo = (w + 2 * pad - (dil * (kw - 1) + 1)) / stride + 1;
    s.om_cs = (int)rup(3 * kh * kw, 4);
    s.K = kh * kw * s.cp;
    const long long P = (long long)n * (s.ho > 0 ? s.ho : 0) * (s.wo > 0 ? s.wo : 0);
    // pixel splits of the weight-gradient GEMM: about 2048 waves in all, at most 4096 and at least 64 pixels per split
    const long long tiles = (long long)(s.K / 64) * (s.co_pad / E::wgrad_rows(s.co_pad));
    long long sp = (2048 + tiles - 1) / tiles;
    if (sp < (P + 4095) / 4096) sp = (P + 4095) / 4096;
    if (sp > (P + 63) / 64) sp = (P + 63) / 64;
    if (sp < 1) sp = 1;
    s.chunk = (int)rup((P + sp - 1) / sp > 0 ? (P + sp - 1) / sp : 1, E::split_granule);
    s.splits = P > 0 ? (int)((P + s.chunk - 1) / s.chunk) : 1;
    long long o = 0;
    s.in_off = o;    o += rup((long long)n * h * w * s.cp * E::size, 256);
    s.om_off = o;    o += rup(P * s.om_cs * 4, 256);
    s.go_off = o;    o += rup(P * s.co_pad * E::size, 256);
    s.wt_off = o;    o += rup((long long)s.K * s.co_pad * E::size, 256);
    s.gcol_off = o;  o += rup(P * s.K * 4, 256);
    s.col_off = o;   o += rup(P * s.K * E::size, 256);
    s.gin_off = o;   o += rup((long long)n * h * w * s.cp * (det ? 8 : 4), 256);
    s.slab_off = o;  o += rup((long long)s.splits * s.co_pad * s.K * 4, 256);
    s.bslab_off = o; o += rup((long long)s.splits * s.co_pad * 4, 256);
    s.stat_off = o;
    if (det) o += rup(((long long)3 * n + 1) * 4, 256);
    s.total = o;
    return s;
}

template <class E>
static long long dcn_bwd_ws_bytes(int n, int c, int h, int w, int co, int kh, int kw, int stride, int pad, int dil, int G, bool det)
{
    if (!dcn_query_ok(E::is_bf16, n, c, h, w, co, kh, kw, stride, pad, dil, G)) return -1;
    return dcn_bwd_ws<E>(n, c / G, h, w, co, kh, kw, stride, pad, dil, det).total;
}

extern "C" long long m3d_dcn_v2_backward_det_workspace_bytes(int batch, int channels, int height, int width, int channels_out,
                                                             int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                                             int deformable_group)
{
    return dcn_bwd_ws_bytes<DcnF32>(batch, channels, height, width, channels_out, kernel_h, kernel_w, stride, pad, dilation, deformable_group,
                                    true);
}

extern "C" long long m3d_dcn_v2_backward_det_workspace_bytes_bf16(int batch, int channels, int height, int width, int channels_out,
                                                                  int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                                                  int deformable_group)
{
    return dcn_bwd_ws_bytes<DcnBf16>(batch, channels, height, width, channels_out, kernel_h, kernel_w, stride, pad, dilation, deformable_group,
                                     true);
}

extern "C" long long m3d_dcn_v2_backward_workspace_bytes(int batch, int channels, int height, int width, int channels_out,
                                                         int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                                         int deformable_group)
{
    return dcn_bwd_ws_bytes<DcnF32>(batch, channels, height, width, channels_out, kernel_h, kernel_w, stride, pad, dilation, deformable_group,
                                    false);
}

extern "C" long long m3d_dcn_v2_backward_workspace_bytes_bf16(int batch, int channels, int height, int width, int channels_out,
                                                              int kernel_h, int kernel_w, int stride, int pad, int dilation,
                                                              int deformable_group)
{
    return dcn_bwd_ws_bytes<DcnBf16>(batch, channels, height, width, channels_out, kernel_h, kernel_w, stride, pad, dilation, deformable_group,
                                     false);
}

// ================================================================================================== backward: per-type steps
// The four places where the two types take different routes (overloads on the traits tag); everything else is dcn_backward.
//
// (1) NCHW operands -> NHWC in the workspace.  A channel slice [c0, c0 + C) of an activation (grad_output, input) with the
// channels [C, cs) zero ...
static int dcn_pack_act(DcnF32, const float *src, int Ctot, int c0, float *dst, int N, int C, int H, int W, int cs, hipStream_t stream)
{
    if (cs != C) M3D_HIP(hipMemsetAsync(dst, 0, (size_t)N * H * W * cs * 4, stream));
    return m3d_nchw_to_nhwc_slice(src, Ctot, c0, dst, N, C, H, W, cs, stream);
}

static int dcn_pack_act(DcnBf16, const u16 *src, int Ctot, int c0, u16 *dst, int N, int C, int H, int W, int cs, hipStream_t stream)
{
    hipLaunchKernelGGL(dcn16_nchw_to_nhwc_kernel, dim3(cdiv((long long)H * W, 32), cdiv(cs, 32), N), dim3(256), 0, stream, src, dst, C, H * W,
                       Ctot, c0, cs);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

// ... and the offsets and masks of group g as fp32 [P][om_cs] (fp32: always float tensors; bf16: either type, per flag)
struct DcnOmSrc {
    const void *offset, *mask;
    int offset_is_bf16, mask_is_bf16;
};

static int dcn_pack_om(DcnF32, const DcnOmSrc &o, float *om, int N, int Ho, int Wo, int kk, int G, int g, int om_cs, hipStream_t stream)
{
    int rc;
    if ((rc = m3d_nchw_to_nhwc_slice((const float *)o.offset, 2 * kk * G, g * 2 * kk, om, N, 2 * kk, Ho, Wo, om_cs, stream))) return rc;
    return m3d_nchw_to_nhwc_slice((const float *)o.mask, kk * G, g * kk, om + 2 * kk, N, kk, Ho, Wo, om_cs, stream);
}

static int dcn_pack_om(DcnBf16, const DcnOmSrc &o, float *om, int N, int Ho, int Wo, int kk, int G, int g, int om_cs, hipStream_t stream)
{
    hipLaunchKernelGGL(dcn16_pack_om_kernel, dim3(imin(cdiv((long long)N * Ho * Wo * om_cs, 256), 4096)), dim3(256), 0, stream, o.offset,
                       o.offset_is_bf16, o.mask, o.mask_is_bf16, om, N, Ho * Wo, kk, G, g, om_cs);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

// (2) gcol = the 1x1 convolution Co -> kk*cp of grad_out with the transposed weight pack, fp32 NHWC output
static int dcn_gcol_gemm(DcnF32, const float *go, const float *wt, float *gcol, int N, const DcnBwdWs &s, hipStream_t stream)
{
    m3d_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.in = go; d.in_cs = s.co_pad; d.N = N; d.H = s.ho; d.W = s.wo; d.Cin = s.co_pad;
    d.wgt = wt; d.Cout = s.K; d.Cout_pad = s.K;
    d.kh = 1; d.kw = 1; d.stride = 1; d.pad = 0; d.dil = 1;
    d.Ho = s.ho; d.Wo = s.wo; d.out = gcol; d.out_cs = s.K;
    d.sigmoid_from = -1;
    return m3d_conv2d_forward(&d, stream);
}

static int dcn_gcol_gemm(DcnBf16, const u16 *go, const u16 *wt, float *gcol, int N, const DcnBwdWs &s, hipStream_t stream)
{
    m3d_conv_bf16_desc d;
    memset(&d, 0, sizeof(d));
    d.in = go; d.in_cs = s.co_pad; d.N = N; d.H = s.ho; d.W = s.wo; d.Cin = s.co_pad;
    d.wgt = wt; d.Cout = s.K; d.Cout_pad = s.K; d.Kpad = s.co_pad;
    d.kh = 1; d.kw = 1; d.stride = 1; d.pad = 0;
    d.Ho = s.ho; d.Wo = s.wo; d.out = gcol; d.out_cs = s.K; d.out_mode = 1;
    d.sigmoid_from = -1;
    d.groups = 1;
    return m3d_conv_bf16_forward(&d, stream);
}

// (3) the weight-gradient launch on `grid` = (column blocks, co / wgrad_rows, splits); dw == false: bias sums only
static void dcn_wgrad_launch(DcnF32, dim3 grid, bool dw, const float *go, const float *col, float *slab, float *bslab, const DcnBwdWs &s,
                             int P, hipStream_t stream)
{
    const int ta = DcnF32::wgrad_rows(s.co_pad) / 32;
#define M3D_WGRAD(TA_, DW_)                                                                                                   \
    hipLaunchKernelGGL((dcn_bwd_wgrad_kernel<TA_, DW_>), grid, dim3(64), 0, stream, go, s.co_pad, col, s.K, slab, bslab, s.co_pad, \
                       P, s.chunk)
    if (ta == 4 && dw) M3D_WGRAD(4, true);
    else if (ta == 4) M3D_WGRAD(4, false);
    else if (dw) M3D_WGRAD(2, true);
    else M3D_WGRAD(2, false);
#undef M3D_WGRAD
}

static void dcn_wgrad_launch(DcnBf16, dim3 grid, bool dw, const u16 *go, const u16 *col, float *slab, float *bslab, const DcnBwdWs &s,
                             int P, hipStream_t stream)
{
    if (dw) hipLaunchKernelGGL((dcn16_wgrad_kernel<true>), grid, dim3(64), 0, stream, go, s.co_pad, col, s.K, slab, bslab, s.co_pad, P, s.chunk);
    else hipLaunchKernelGGL((dcn16_wgrad_kernel<false>), grid, dim3(64), 0, stream, go, s.co_pad, col, s.K, slab, bslab, s.co_pad, P, s.chunk);
}
// (4) the size limits: E::max_in_elems / E::max_go_elems

// ================================================================================================== backward: the driver
template <class E, bool DET>
static int dcn_backward(const typename E::T *input, const typename E::T *weight, const DcnOmSrc &om_src, const typename E::T *grad_output,
                        typename E::T *grad_input, float *grad_offset, float *grad_mask, typename E::T *grad_weight, float *grad_bias,
                        int batch, int channels, int height, int width, int channels_out, int kernel_h, int kernel_w, int stride_h,
                        int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, int deformable_group, void *workspace,
                        long long workspace_bytes, hipStream_t stream)
{
    typedef typename E::T T;
    const char *name = DET ? E::det_name : E::bwd_name;
    int rc;
    if ((rc = dcn_check_args(name, E::is_bf16, input && weight && om_src.offset && om_src.mask && grad_output && workspace,
                             dcn_shape_ok(E::is_bf16, batch, channels, height, width, channels_out, kernel_h, kernel_w, stride_h, pad_h,
                                          dilation_h),
                             channels, deformable_group, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, workspace)))
        return rc;
    const int G = deformable_group, cg = channels / G, kk = kernel_h * kernel_w;
    const DcnBwdWs s = dcn_bwd_ws<E>(batch, cg, height, width, channels_out, kernel_h, kernel_w, stride_h, pad_h, dilation_h, DET);
    if ((rc = dcn_check_workspace(name, DET ? E::det_query : E::bwd_query, workspace_bytes, s.total))) return rc;
    M3D_REQUIRE(s.ho > 0 && s.wo > 0, "%s: empty output", name);
    const long long P = (long long)batch * s.ho * s.wo, HoWo = (long long)s.ho * s.wo;
    const long long in_elems = (long long)batch * height * width * s.cp;
    M3D_REQUIRE(P < (1ll << 29) && in_elems < E::max_in_elems && P * s.co_pad < E::max_go_elems, "%s: tensor too large", name);
    if (!grad_input && !grad_offset && !grad_mask && !grad_weight && !grad_bias) return M3D_OK;
    const int HW = height * width;
    char *ws = (char *)workspace;
    T *in_nhwc = (T *)(ws + s.in_off), *go = (T *)(ws + s.go_off), *wt = (T *)(ws + s.wt_off), *col = (T *)(ws + s.col_off);
    float *om = (float *)(ws + s.om_off), *gcol = (float *)(ws + s.gcol_off), *gin = (float *)(ws + s.gin_off);
    float *slab = (float *)(ws + s.slab_off), *bslab = (float *)(ws + s.bslab_off);
    const bool need_gcol = grad_input || grad_offset || grad_mask, need_col = grad_weight != nullptr;
    const bool need_sample = need_gcol || need_col;
    if ((rc = dcn_pack_act(E(), grad_output, channels_out, 0, go, batch, channels_out, s.ho, s.wo, s.co_pad, stream))) return rc;
    // the deterministic form: the statistics of the fixed-point exponent (dcn_sexp_kernel), all on the device
    unsigned *amax = (unsigned *)(ws + s.stat_off), *mmax = amax + batch, *wmax = mmax + batch;
    int *sexp = (int *)(wmax + 1);
    const bool det_gin = DET && grad_input;
    int log2T = 0;
    while ((1ll << log2T) < HoWo * kk) ++log2T;
    if (det_gin) {
        M3D_HIP(hipMemsetAsync(amax, 0, ((size_t)2 * batch + 1) * 4, stream));
        hipLaunchKernelGGL(dcn_absmax_kernel<T>, dim3(imin(cdiv(HoWo * s.co_pad, 256), 256), batch), dim3(256), 0, stream, (const T *)go,
                           (int)HoWo, s.co_pad, 0, s.co_pad, amax);
        M3D_LAUNCH_CHECK();
    }
    for (int g = 0; g < G; ++g) {
        if (need_sample) {
            if ((rc = dcn_pack_act(E(), input, channels, g * cg, in_nhwc, batch, cg, height, width, s.cp, stream))) return rc;
            if ((rc = dcn_pack_om(E(), om_src, om, batch, s.ho, s.wo, kk, G, g, s.om_cs, stream))) return rc;
        }
        if (need_gcol) {
            const long long total = (long long)s.K * s.co_pad;
            hipLaunchKernelGGL(dcn_pack_wt_kernel<E>, dim3(imin(cdiv(total, 256), 4096)), dim3(256), 0, stream, weight, wt, channels_out,
                               s.co_pad, cg, s.cp, kk, channels, g * cg);
            M3D_LAUNCH_CHECK();
            if ((rc = dcn_gcol_gemm(E(), go, wt, gcol, batch, s, stream))) return rc;
        }
        if (det_gin) {
            if (g > 0) M3D_HIP(hipMemsetAsync(mmax, 0, ((size_t)batch + 1) * 4, stream));
            hipLaunchKernelGGL(dcn_absmax_kernel<float>, dim3(imin(cdiv(HoWo * kk, 256), 256), batch), dim3(256), 0, stream, (const float *)om,
                               (int)HoWo, s.om_cs, 2 * kk, kk, mmax);
            M3D_LAUNCH_CHECK();
            hipLaunchKernelGGL(dcn_wsum_max_kernel<T>, dim3(cdiv(s.K, 4)), dim3(256), 0, stream, (const T *)wt, s.K, s.co_pad, wmax);
            M3D_LAUNCH_CHECK();
            hipLaunchKernelGGL(dcn_sexp_kernel, dim3(cdiv(batch, 64)), dim3(64), 0, stream, amax, mmax, wmax, sexp, batch, log2T);
            M3D_LAUNCH_CHECK();
        }
        if (grad_input) M3D_HIP(hipMemsetAsync(gin, 0, (size_t)in_elems * (DET ? 8 : 4), stream));
        if (need_sample) {
            DcnSampleArgs<E> a;
            a.in = in_nhwc; a.om = om; a.gcol = need_gcol ? gcol : nullptr; a.col = need_col ? col : nullptr;
            a.gin = grad_input ? gin : nullptr; a.sexp = det_gin ? sexp : nullptr;
            a.goff = grad_offset ? grad_offset + (size_t)g * 2 * kk * HoWo : nullptr;
            a.gmask = grad_mask ? grad_mask + (size_t)g * kk * HoWo : nullptr;
            a.goff_img = (long long)2 * kk * G * HoWo; a.gmask_img = (long long)kk * G * HoWo;
            a.P = (int)P; a.H = height; a.W = width; a.Ho = s.ho; a.Wo = s.wo; a.cp = s.cp; a.kh = kernel_h; a.kw = kernel_w;
            a.stride = stride_h; a.pad = pad_h; a.dil = dilation_h; a.om_cs = s.om_cs;
            hipLaunchKernelGGL((dcn_sample_kernel<E, DET>), dim3(cdiv(P, 4)), dim3(256), 0, stream, a);
            M3D_LAUNCH_CHECK();
        }
        if (det_gin) {
            hipLaunchKernelGGL(dcn_nhwc_i64_to_nchw_kernel<E>, dim3(cdiv(HW, 32), cdiv(cg, 32), batch), dim3(256), 0, stream,
                               (const long long *)gin, s.cp, sexp, grad_input, cg, HW, channels, g * cg);
            M3D_LAUNCH_CHECK();
        } else if (grad_input) {
            hipLaunchKernelGGL(dcn_nhwc_f32_to_nchw_kernel<E>, dim3(cdiv(HW, 32), cdiv(cg, 32), batch), dim3(256), 0, stream, gin, s.cp, 1, 0ll,
                               grad_input, cg, HW, channels, g * cg);
            M3D_LAUNCH_CHECK();
        }
        const bool want_bias = grad_bias && g == 0;
        if (need_col || want_bias) {
            const dim3 grid(need_col ? s.K / 64 : 1, s.co_pad / E::wgrad_rows(s.co_pad), s.splits);
            dcn_wgrad_launch(E(), grid, need_col, go, col, slab, bslab, s, (int)P, stream);
            M3D_LAUNCH_CHECK();
            const long long total = (need_col ? (long long)channels_out * cg * kk : 0) + (want_bias ? channels_out : 0);
            hipLaunchKernelGGL(dcn_reduce_kernel<E>, dim3(imin(cdiv(total, 256), 4096)), dim3(256), 0, stream, slab, bslab,
                               need_col ? grad_weight : nullptr, want_bias ? grad_bias : nullptr, s.splits, channels_out, s.co_pad, cg, s.cp,
                               kk, channels, g * cg);
            M3D_LAUNCH_CHECK();
        }
    }
    return M3D_OK;
}

extern "C" int m3d_dcn_v2_backward(const float *input, const float *weight, const float *offset, const float *mask,
                                   const float *grad_output, float *grad_input, float *grad_offset, float *grad_mask,
                                   float *grad_weight, float *grad_bias, int batch, int channels, int height, int width,
                                   int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                   int dilation_h, int dilation_w, int deformable_group, void *workspace, long long workspace_bytes,
                                   m3d_stream_t stream_)
{
    return dcn_backward<DcnF32, false>(input, weight, DcnOmSrc{offset, mask, 0, 0}, grad_output, grad_input, grad_offset, grad_mask, grad_weight,
                                grad_bias, batch, channels, height, width, channels_out, kernel_h, kernel_w, stride_h, stride_w, pad_h,
                                pad_w, dilation_h, dilation_w, deformable_group, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int m3d_dcn_v2_backward_bf16(const void *input, const void *weight, const void *offset, int offset_is_bf16, const void *mask,
                                        int mask_is_bf16, const void *grad_output, void *grad_input, float *grad_offset, float *grad_mask,
                                        void *grad_weight, float *grad_bias, int batch, int channels, int height, int width,
                                        int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                        int dilation_h, int dilation_w, int deformable_group, void *workspace, long long workspace_bytes,
                                        m3d_stream_t stream_)
{
    return dcn_backward<DcnBf16, false>((const u16 *)input, (const u16 *)weight, DcnOmSrc{offset, mask, offset_is_bf16, mask_is_bf16},
                                 (const u16 *)grad_output, (u16 *)grad_input, grad_offset, grad_mask, (u16 *)grad_weight, grad_bias, batch,
                                 channels, height, width, channels_out, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                                 dilation_w, deformable_group, workspace, workspace_bytes, (hipStream_t)stream_);
}

// The same two calls with a bitwise-reproducible grad_input (64-bit fixed-point sums, see dcn_sexp_kernel); the other four gradients
// take the path of the calls above and have their bits.
extern "C" int m3d_dcn_v2_backward_det(const float *input, const float *weight, const float *offset, const float *mask,
                                       const float *grad_output, float *grad_input, float *grad_offset, float *grad_mask,
                                       float *grad_weight, float *grad_bias, int batch, int channels, int height, int width,
                                       int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                       int dilation_h, int dilation_w, int deformable_group, void *workspace, long long workspace_bytes,
                                       m3d_stream_t stream_)
{
    return dcn_backward<DcnF32, true>(input, weight, DcnOmSrc{offset, mask, 0, 0}, grad_output, grad_input, grad_offset, grad_mask,
                                      grad_weight, grad_bias, batch, channels, height, width, channels_out, kernel_h, kernel_w, stride_h,
                                      stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group, workspace, workspace_bytes,
                                      (hipStream_t)stream_);
}

extern "C" int m3d_dcn_v2_backward_det_bf16(const void *input, const void *weight, const void *offset, int offset_is_bf16,
                                            const void *mask, int mask_is_bf16, const void *grad_output, void *grad_input,
                                            float *grad_offset, float *grad_mask, void *grad_weight, float *grad_bias, int batch,
                                            int channels, int height, int width, int channels_out, int kernel_h, int kernel_w,
                                            int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w,
                                            int deformable_group, void *workspace, long long workspace_bytes, m3d_stream_t stream_)
{
    return dcn_backward<DcnBf16, true>((const u16 *)input, (const u16 *)weight, DcnOmSrc{offset, mask, offset_is_bf16, mask_is_bf16},
                                       (const u16 *)grad_output, (u16 *)grad_input, grad_offset, grad_mask, (u16 *)grad_weight, grad_bias,
                                       batch, channels, height, width, channels_out, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                       dilation_h, dilation_w, deformable_group, workspace, workspace_bytes, (hipStream_t)stream_);
}
