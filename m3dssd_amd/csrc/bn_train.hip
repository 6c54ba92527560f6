// BatchNorm2d with batch statistics + optional residual add + LeakyReLU / ReLU / no activation, for TRAINING: forward and backward,
// fp32 NCHW (the chain host/train.py otherwise hands to torch after every convolution: model/pose_dla_dcn.py:107-121,261-269,379-389,
// 482-485, M3d_inference_align.py:66-210).
//
//   forward   mean = sum(x) / N,  var = max(sum(x^2) / N - mean^2, 0)  (N = B*H*W, biased),  invstd = 1 / sqrt(var + eps)
//             z = (x - mean) * invstd * gamma + beta (+ residual),   y = z > 0 ? z : slope * z
//             running_mean = (1 - m) * running_mean + m * mean,   running_var = (1 - m) * running_var + m * var * N / (N - 1)
//   backward  dz = grad_y * (y > 0 ? 1 : slope)  (the mask comes from the saved OUTPUT),  dres = dz,  dbeta = sum(dz),
//             dgamma = sum(dz * xhat) with xhat = (x - mean) * invstd,  dx = gamma * invstd * (dz - dbeta / N - xhat * dgamma / N)
//
// A channel's N values are cut into CHUNKS of BN_CHUNK consecutive positions n = b * HW + p (the last one may be shorter); one
// workgroup per (channel, chunk), so C = 16 with N ~ 10^6 gives thousands of workgroups and C = 512 with N = 8 gives 512 small ones.
// Each direction is TWO launches:
//   *_stats_kernel   per (channel, chunk) the two sums in float64 (every thread adds its elements in a fixed order, the 256 thread
//                    sums are combined by a fixed tree in LDS) -> workspace [C][chunks][2].  No atomics.
//   *_apply_kernel   every workgroup adds the partials of ITS channel (thread t the chunks t, t + 256, ... in that order, then the
//                    same tree: all workgroups of a channel derive the same bits), then applies to its chunk.  The workgroup of
//                    chunk 0 writes the per-channel results (save_mean / save_invstd / running statistics; grad_gamma / grad_beta).
// Every word of the workspace that is read was written by the stats launch of the same call: nothing depends on what it held.
// float32 values are rounded once from the float64 statistics; the forward and the backward evaluate xhat from the same float32
// save_mean / save_invstd.
//
// Access: 16-byte loads and stores when HW % 4 == 0 and every tensor is 16-byte aligned (a group of 4 positions then lies inside one
// (image, channel) slab), else one element per lane (with odd HW the slabs do not start on 16-byte boundaries).  Each thread issues
// all loads of its chunk share before the first use.  The launchers keep no state: nothing here is per device or per process.
#include <math.h>
#include <stdint.h>

#include "common.h"

#define BN_NT 256
#define BN_CHUNK 4096

struct BnGeom { int C, HW, N, chunks; };

template <bool VEC> struct BnTr;
template <> struct BnTr<true> { typedef f32x4 T; enum { W = 4, IT = BN_CHUNK / (BN_NT * 4) }; };
template <> struct BnTr<false> { typedef float T; enum { W = 1, IT = BN_CHUNK / BN_NT }; };

__device__ __forceinline__ float bn_get(float v, int) { return v; }
__device__ __forceinline__ float bn_get(f32x4 v, int j) { return v[j]; }
__device__ __forceinline__ void bn_set(float &v, int, float s) { v = s; }
__device__ __forceinline__ void bn_set(f32x4 &v, int j, float s) { v[j] = s; }
__device__ __forceinline__ void bn_store(float *p, float v) { *p = v; }
__device__ __forceinline__ void bn_store(float *p, f32x4 v) { global_store_u32x4_nop(p, __builtin_bit_cast(u32x4, v)); }

// element offsets of this thread's share of chunk k of channel c; ok[i] clear: past the end of the channel
template <bool VEC>
__device__ __forceinline__ void bn_offsets(const BnGeom &g, int c, int k, size_t (&off)[BnTr<VEC>::IT], bool (&ok)[BnTr<VEC>::IT])
{
    constexpr int W = BnTr<VEC>::W, IT = BnTr<VEC>::IT;
    const int n0 = k * BN_CHUNK;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int n = n0 + (i * BN_NT + (int)threadIdx.x) * W;        // (HW % 4 == 0 on the 16-byte path: n + 3 < N, same slab)
        ok[i] = n < g.N;
        const int b = ok[i] ? n / g.HW : 0, p = ok[i] ? n - b * g.HW : 0;
        off[i] = ((size_t)b * g.C + c) * g.HW + p;
    }
}

// sum of the BN_NT pairs by a fixed tree; every thread gets the totals
__device__ __forceinline__ void bn_block_sum(double &a, double &b, double *s_a, double *s_b)
{
    const int tid = threadIdx.x;
    s_a[tid] = a;
    s_b[tid] = b;
    __syncthreads();
    for (int s = BN_NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            s_a[tid] = s_a[tid] + s_a[tid + s];
            s_b[tid] = s_b[tid] + s_b[tid + s];
        }
        __syncthreads();
    }
    a = s_a[0];
    b = s_b[0];
}

// the partials of channel c in a fixed order -> totals in every thread
__device__ __forceinline__ void bn_channel_sums(const double *part, const BnGeom &g, int c, double &a, double &b, double *s_a, double *s_b)
{
    a = 0.0;
    b = 0.0;
    const double *pc = part + (size_t)c * g.chunks * 2;
    for (int j = threadIdx.x; j < g.chunks; j += BN_NT) {
        a = a + pc[2 * j];
        b = b + pc[2 * j + 1];
    }
    bn_block_sum(a, b, s_a, s_b);
}

template <bool VEC>
__global__ __launch_bounds__(BN_NT) void bn_fwd_stats_kernel(const float *x, BnGeom g, double *part)
{
    typedef typename BnTr<VEC>::T T;
    constexpr int W = BnTr<VEC>::W, IT = BnTr<VEC>::IT;
    __shared__ double s_a[BN_NT], s_b[BN_NT];
    const int c = blockIdx.x / g.chunks, k = blockIdx.x - c * g.chunks;
    size_t off[IT];
    bool ok[IT];
    bn_offsets<VEC>(g, c, k, off, ok);
    T v[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i)
        if (ok[i]) v[i] = *reinterpret_cast<const T *>(x + off[i]);
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int i = 0; i < IT; ++i)
        if (ok[i]) {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const double d = (double)bn_get(v[i], j);
                s = s + d;
                q = q + d * d;
            }
        }
    bn_block_sum(s, q, s_a, s_b);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = s;
        part[2 * (size_t)blockIdx.x + 1] = q;
    }
}

struct BnFwdArgs {
    const float *x, *res, *gamma, *beta;
    float *running_mean, *running_var, *y, *save_mean, *save_invstd;
    const double *part;
    double eps, momentum;
    float slope;
    BnGeom g;
};

template <bool VEC>
__global__ __launch_bounds__(BN_NT) void bn_fwd_apply_kernel(BnFwdArgs a)
{
    typedef typename BnTr<VEC>::T T;
    constexpr int W = BnTr<VEC>::W, IT = BnTr<VEC>::IT;
    __shared__ double s_a[BN_NT], s_b[BN_NT];
    const BnGeom g = a.g;
    const int c = blockIdx.x / g.chunks, k = blockIdx.x - c * g.chunks;
    size_t off[IT];
    bool ok[IT];
    bn_offsets<VEC>(g, c, k, off, ok);
    T xv[IT], rv[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i)
        if (ok[i]) {
            xv[i] = *reinterpret_cast<const T *>(a.x + off[i]);
            if (a.res) rv[i] = *reinterpret_cast<const T *>(a.res + off[i]);
        }
    double s, q;
    bn_channel_sums(a.part, g, c, s, q, s_a, s_b);
    const double mean = s / (double)g.N;
    const double var = fmax(q / (double)g.N - mean * mean, 0.0);
    const float mean_f = (float)mean, invstd_f = (float)(1.0 / sqrt(var + a.eps));
    if (k == 0 && threadIdx.x == 0) {
        a.save_mean[c] = mean_f;
        a.save_invstd[c] = invstd_f;
        if (a.running_mean) a.running_mean[c] = (float)((1.0 - a.momentum) * (double)a.running_mean[c] + a.momentum * mean);
        if (a.running_var)
            a.running_var[c] = (float)((1.0 - a.momentum) * (double)a.running_var[c] +
                                       a.momentum * (var * ((double)g.N / (double)(g.N - 1))));
    }
    const float gamma = a.gamma[c], beta = a.beta[c], slope = a.slope;
#pragma unroll
    for (int i = 0; i < IT; ++i)
        if (ok[i]) {
            T out;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                float z = (bn_get(xv[i], j) - mean_f) * invstd_f * gamma + beta;
                if (a.res) z = z + bn_get(rv[i], j);
                bn_set(out, j, z > 0.f ? z : slope * z);
            }
            bn_store(a.y + off[i], out);
        }
}

struct BnBwdArgs {
    const float *gy, *x, *y, *gamma, *save_mean, *save_invstd;
    float *gx, *gres, *ggamma, *gbeta;
    double *part;
    float slope;
    int need_sums;
    BnGeom g;
};

template <bool VEC>
__global__ __launch_bounds__(BN_NT) void bn_bwd_stats_kernel(BnBwdArgs a)
{
    typedef typename BnTr<VEC>::T T;
    constexpr int W = BnTr<VEC>::W, IT = BnTr<VEC>::IT;
    __shared__ double s_a[BN_NT], s_b[BN_NT];
    const BnGeom g = a.g;
    const int c = blockIdx.x / g.chunks, k = blockIdx.x - c * g.chunks;
    size_t off[IT];
    bool ok[IT];
    bn_offsets<VEC>(g, c, k, off, ok);
    T gv[IT], xv[IT], yv[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i)
        if (ok[i]) {
            gv[i] = *reinterpret_cast<const T *>(a.gy + off[i]);
            xv[i] = *reinterpret_cast<const T *>(a.x + off[i]);
            yv[i] = *reinterpret_cast<const T *>(a.y + off[i]);
        }
    const float mean = a.save_mean[c], invstd = a.save_invstd[c], slope = a.slope;
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int i = 0; i < IT; ++i)
        if (ok[i]) {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const float dz = bn_get(gv[i], j) * (bn_get(yv[i], j) > 0.f ? 1.f : slope);
                const float xhat = (bn_get(xv[i], j) - mean) * invstd;
                s = s + (double)dz;
                q = q + (double)dz * (double)xhat;
            }
        }
    bn_block_sum(s, q, s_a, s_b);
    if (threadIdx.x == 0) {
        a.part[2 * (size_t)blockIdx.x] = s;
        a.part[2 * (size_t)blockIdx.x + 1] = q;
    }
}

template <bool VEC>
__global__ __launch_bounds__(BN_NT) void bn_bwd_apply_kernel(BnBwdArgs a)
{
    typedef typename BnTr<VEC>::T T;
    constexpr int W = BnTr<VEC>::W, IT = BnTr<VEC>::IT;
    __shared__ double s_a[BN_NT], s_b[BN_NT];
    const BnGeom g = a.g;
    const int c = blockIdx.x / g.chunks, k = blockIdx.x - c * g.chunks;
    const bool elems = a.gx || a.gres;
    if (!elems && k != 0) return;                       // only the per-channel sums are wanted: chunk 0 writes them
    size_t off[IT];
    bool ok[IT];
    bn_offsets<VEC>(g, c, k, off, ok);
    T gv[IT], xv[IT], yv[IT];
    if (elems) {
#pragma unroll
        for (int i = 0; i < IT; ++i)
            if (ok[i]) {
                gv[i] = *reinterpret_cast<const T *>(a.gy + off[i]);
                yv[i] = *reinterpret_cast<const T *>(a.y + off[i]);
                if (a.gx) xv[i] = *reinterpret_cast<const T *>(a.x + off[i]);
            }
    }
    double s = 0.0, q = 0.0;
    if (a.need_sums) bn_channel_sums(a.part, g, c, s, q, s_a, s_b);
    if (k == 0 && threadIdx.x == 0) {
        if (a.gbeta) a.gbeta[c] = (float)s;
        if (a.ggamma) a.ggamma[c] = (float)q;
    }
    if (!elems) return;
    const float mean = a.save_mean[c], invstd = a.save_invstd[c], slope = a.slope;
    const float scale = a.gamma[c] * invstd, mb = (float)(s / (double)g.N), mg = (float)(q / (double)g.N);
#pragma unroll
    for (int i = 0; i < IT; ++i)
        if (ok[i]) {
            T dzv, dxv;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const float dz = bn_get(gv[i], j) * (bn_get(yv[i], j) > 0.f ? 1.f : slope);
                bn_set(dzv, j, dz);
                if (a.gx) {
                    const float xhat = (bn_get(xv[i], j) - mean) * invstd;
                    bn_set(dxv, j, scale * (dz - mb - xhat * mg));
                }
            }
            if (a.gres) bn_store(a.gres + off[i], dzv);
            if (a.gx) bn_store(a.gx + off[i], dxv);
        }
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
// chunks per channel, 0 for a shape outside the supported range (a size < 1, fewer than 2 values per channel, a count past 2^31)
static int bn_chunks(int B, int C, int H, int W)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
    const long long hw = (long long)H * W, n = hw * B;
    if (n < 2 || n > 0x7fffffffLL - 2 * BN_CHUNK) return 0;
    const long long chunks = (n + BN_CHUNK - 1) / BN_CHUNK;
    if (chunks * C > 0x7fffffffLL) return 0;
    return (int)chunks;
}

extern "C" int m3d_bn_act_train_chunks(int B, int C, int H, int W) { const int k = bn_chunks(B, C, H, W); return k ? k : -1; }

extern "C" long long m3d_bn_act_train_workspace_bytes(int B, int C, int H, int W)
{
    const int k = bn_chunks(B, C, H, W);
    return k ? (long long)C * k * 2 * (long long)sizeof(double) : -1;
}

static int bn_check(const char *who, int B, int C, int H, int W, float slope, const void *workspace, long long workspace_bytes, BnGeom &g)
{
    M3D_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: bad shape [%d, %d, %d, %d]", who, B, C, H, W);
    M3D_REQUIRE((long long)B * H * W >= 2, "%s: batch statistics need more than 1 value per channel (B*H*W = %lld)", who,
                (long long)B * H * W);
    const int chunks = bn_chunks(B, C, H, W);
    M3D_REQUIRE(chunks > 0, "%s: shape [%d, %d, %d, %d] is too large", who, B, C, H, W);
    M3D_REQUIRE(slope >= 0.f && slope <= 1.f, "%s: slope %g outside [0, 1]", who, (double)slope);
    M3D_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "%s: the workspace must be a 16-byte aligned device pointer", who);
    const long long need = m3d_bn_act_train_workspace_bytes(B, C, H, W);
    M3D_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes; [%d, %d, %d, %d] needs %lld", who, workspace_bytes, B, C, H, W, need);
    g.C = C;
    g.HW = H * W;
    g.N = B * H * W;
    g.chunks = chunks;
    return M3D_OK;
}

extern "C" int m3d_bn_act_train_forward(const float *x, const float *residual, const float *gamma, const float *beta, float *running_mean,
                                        float *running_var, float *y, float *save_mean, float *save_invstd, int B, int C, int H, int W,
                                        double eps, double momentum, float slope, void *workspace, long long workspace_bytes,
                                        m3d_stream_t stream)
{
    const char *who = "bn_act_train_forward";
    M3D_REQUIRE(x && gamma && beta && y && save_mean && save_invstd, "%s: null pointer", who);
    BnGeom g;
    const int rc = bn_check(who, B, C, H, W, slope, workspace, workspace_bytes, g);
    if (rc != M3D_OK) return rc;
    M3D_REQUIRE(isfinite(eps) && eps >= 0.0 && isfinite(momentum), "%s: eps %g / momentum %g", who, eps, momentum);
    const uintptr_t all = (uintptr_t)x | (uintptr_t)residual | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)running_mean |
                          (uintptr_t)running_var | (uintptr_t)y | (uintptr_t)save_mean | (uintptr_t)save_invstd;
    M3D_REQUIRE((all & 3) == 0, "%s: the tensors must be 4-byte aligned", who);
    const bool vec = g.HW % 4 == 0 && (((uintptr_t)x | (uintptr_t)residual | (uintptr_t)y) & 15) == 0;
    BnFwdArgs a = {x, residual, gamma, beta, running_mean, running_var, y, save_mean, save_invstd, (const double *)workspace,
                   eps, momentum, slope, g};
    const dim3 grid((unsigned)(C * g.chunks)), block(BN_NT);
    if (vec) {
        hipLaunchKernelGGL(bn_fwd_stats_kernel<true>, grid, block, 0, (hipStream_t)stream, x, g, (double *)workspace);
        M3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(bn_fwd_apply_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(bn_fwd_stats_kernel<false>, grid, block, 0, (hipStream_t)stream, x, g, (double *)workspace);
        M3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(bn_fwd_apply_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    }
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

extern "C" int m3d_bn_act_train_backward(const float *grad_y, const float *x, const float *y, const float *gamma, const float *save_mean,
                                         const float *save_invstd, float *grad_x, float *grad_residual, float *grad_gamma,
                                         float *grad_beta, int B, int C, int H, int W, float slope, void *workspace,
                                         long long workspace_bytes, m3d_stream_t stream)
{
    const char *who = "bn_act_train_backward";
    M3D_REQUIRE(grad_y && x && y && gamma && save_mean && save_invstd, "%s: null pointer", who);
    BnGeom g;
    const int rc = bn_check(who, B, C, H, W, slope, workspace, workspace_bytes, g);
    if (rc != M3D_OK) return rc;
    const uintptr_t all = (uintptr_t)grad_y | (uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)save_mean |
                          (uintptr_t)save_invstd | (uintptr_t)grad_x | (uintptr_t)grad_residual | (uintptr_t)grad_gamma |
                          (uintptr_t)grad_beta;
    M3D_REQUIRE((all & 3) == 0, "%s: the tensors must be 4-byte aligned", who);
    if (!grad_x && !grad_residual && !grad_gamma && !grad_beta) return M3D_OK;
    const bool vec = g.HW % 4 == 0 &&
                     (((uintptr_t)grad_y | (uintptr_t)x | (uintptr_t)y | (uintptr_t)grad_x | (uintptr_t)grad_residual) & 15) == 0;
    const int need_sums = grad_x || grad_gamma || grad_beta;         // grad_residual alone is grad_y times the mask
    BnBwdArgs a = {grad_y, x, y, gamma, save_mean, save_invstd, grad_x, grad_residual, grad_gamma, grad_beta, (double *)workspace,
                   slope, need_sums, g};
    const dim3 grid((unsigned)(C * g.chunks)), block(BN_NT);
    if (need_sums) {
        if (vec) hipLaunchKernelGGL(bn_bwd_stats_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(bn_bwd_stats_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
        M3D_LAUNCH_CHECK();
    }
    if (vec) hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}
