// Deformable position-sensitive RoI pooling, forward and backward, fp32: the drop-ins for dcn_v2_psroi_pooling_cuda_forward /
// _backward (model/DCNv2/src/dcn_v2_cuda.c, kernels model/DCNv2/src/cuda/dcn_v2_psroi_pooling_cuda.cu), the operator behind
// DCNv2PoolingFunction / DCNv2Pooling / DCNPooling.  include/m3dssd_hip.h states the definition; this file follows it literally.
//
// Layout.  The sampling state of (region, bin, class) -- region geometry, learned offset, the S x S sample coordinates, which of
// them count -- is the same for every output channel of that class, so it is wave-uniform: one wave takes one (region, bin, class,
// block of 64 output channels), lane = output channel.  Output channel c of bin (gh, gw) reads input channel (c*G + gh)*G + gw:
// in the NCHW input a lane's corner reads would lie H*W*G*G floats apart.  psroi_pack_kernel therefore transposes the first
// D*G*G channels of `data` once per call into the workspace as [N*H*W][G*G][D] (pixel-major, then group cell, then output
// channel): a corner read of a wave is one contiguous row segment of up to 256 bytes, for every G.  The backward adds grad_data
// into an fp32 staging buffer of the same layout with float atomics (each atomic wave-instruction = contiguous channels of one
// pixel row) and psroi_unpack_kernel transposes it back, writing zeros into the channels past D*G*G.
//
// grad_trans is reduced without atomics: lanes by a butterfly, then psroi_trans_reduce_kernel adds the per-wave partials of the
// bins of a part cell in (ph, pw, channel block) order.  It is bitwise reproducible; grad_data (float atomics) is not.
//
// Every coordinate operation is rounded once, in the documented order: contraction is off for this whole file, so that a
// float32 restatement (tests/psroi_ref.py) reproduces every counted / not counted decision.
#include <limits.h>

#include "common.h"

#pragma clang fp contract(off)

static inline long long rup256(long long a) { return (a + 255) / 256 * 256; }

struct PsroiArgs {
    const float *data;              // workspace [N*H*W][CS], CS = G*G*D (backward: NULL unless grad_trans is wanted)
    const float *rois, *trans;      // [n][5]; [>= n][2K][part][part] or NULL (no_trans)
    float *out, *count;             // forward: [n][D][P][P]; count may be NULL
    const float *gout;              // backward: [n][D][P][P]
    float *gin;                     // backward: staging [N*H*W][CS], zeroed, or NULL
    float *partial;                 // backward: [items][2] (x, y) or NULL
    int N, H, W, n, D, G, P, part, S, K, cec, nch, CS, items;
    float scale, trans_std;
};

// part cell of bin index q: floorf((float)q / P * part_size), the reference's float32 expression (it differs from
// (q * part) / P for a few (q, P)); the clamp keeps a degenerate size inside the tensor
__device__ __forceinline__ int psroi_part(int q, int P, int part)
{
    const int v = (int)floorf((float)q / (float)P * (float)part);
    return min(max(v, 0), part - 1);
}

__device__ __forceinline__ bool psroi_finite(float v) { return v - v == 0.f; }

struct PsroiBin {
    float wstart, hstart, sub_w, sub_h, roi_w, roi_h;
    int b, cell, qh, qw;            // image, group cell gh*G + gw, part cell
    bool ok;                        // region usable: batch index an integer in [0, N), corners finite
};

// geometry of bin (ph, pw) of region i for class `cls`: every value is the same in all lanes
__device__ __forceinline__ PsroiBin psroi_bin(const PsroiArgs &a, int i, int cls, int ph, int pw)
{
    PsroiBin s;
    const float *r = a.rois + (size_t)i * 5;
    const float bf = r[0], x1 = r[1], y1 = r[2], x2 = r[3], y2 = r[4];
    s.ok = bf >= 0.f && bf < (float)a.N && bf == floorf(bf) && psroi_finite(x1) && psroi_finite(y1) && psroi_finite(x2) &&
           psroi_finite(y2);
    s.b = s.ok ? (int)bf : 0;
    const float rs_w = roundf(x1) * a.scale - 0.5f, rs_h = roundf(y1) * a.scale - 0.5f;
    const float re_w = (roundf(x2) + 1.f) * a.scale - 0.5f, re_h = (roundf(y2) + 1.f) * a.scale - 0.5f;
    s.roi_w = fmaxf(re_w - rs_w, 0.1f);
    s.roi_h = fmaxf(re_h - rs_h, 0.1f);
    const float bin_w = s.roi_w / (float)a.P, bin_h = s.roi_h / (float)a.P;
    s.sub_w = bin_w / (float)a.S;
    s.sub_h = bin_h / (float)a.S;
    s.qh = psroi_part(ph, a.P, a.part);
    s.qw = psroi_part(pw, a.P, a.part);
    const int gw = min(max((int)floorf((float)pw * (float)a.G / (float)a.P), 0), a.G - 1);
    const int gh = min(max((int)floorf((float)ph * (float)a.G / (float)a.P), 0), a.G - 1);
    s.cell = gh * a.G + gw;
    float tx = 0.f, ty = 0.f;
    if (a.trans && s.ok) {
        const float *t = a.trans + (((size_t)i * 2 * a.K + 2 * cls) * a.part + s.qh) * a.part + s.qw;
        tx = t[0] * a.trans_std;
        ty = t[(size_t)a.part * a.part] * a.trans_std;
    }
    s.wstart = ((float)pw * bin_w + rs_w) + tx * s.roi_w;
    s.hstart = ((float)ph * bin_h + rs_h) + ty * s.roi_h;
    return s;
}

// One sample: counted iff -0.5 <= w <= W - 0.5 and -0.5 <= h <= H - 0.5 (false for NaN and inf); then clamped to the map and
// resolved into floor / ceil corners (pixel offsets y*W + x inside the image plane) and the weights of the ceil side.
struct PsroiSample {
    int o11, o12, o21, o22;         // (y1, x1), (y2, x1), (y1, x2), (y2, x2): y1 / x1 = floor, y2 / x2 = ceil
    float dx, dy;
};

__device__ __forceinline__ bool psroi_sample(const PsroiBin &s, int ih, int iw, int H, int W, PsroiSample &q)
{
    float w = s.wstart + (float)iw * s.sub_w, h = s.hstart + (float)ih * s.sub_h;
    if (!(w >= -0.5f && w <= (float)W - 0.5f && h >= -0.5f && h <= (float)H - 0.5f)) return false;
    w = fminf(fmaxf(w, 0.f), (float)W - 1.f);
    h = fminf(fmaxf(h, 0.f), (float)H - 1.f);
    const float xf = floorf(w), yf = floorf(h);
    const int x1 = (int)xf, x2 = (int)ceilf(w), y1 = (int)yf, y2 = (int)ceilf(h);     // all in [0, W-1] / [0, H-1]
    q.dx = w - xf;
    q.dy = h - yf;
    q.o11 = y1 * W + x1; q.o12 = y2 * W + x1; q.o21 = y1 * W + x2; q.o22 = y2 * W + x2;
    return true;
}

// the number of counted samples of a bin: the one definition the forward and the backward share
__device__ __forceinline__ int psroi_count(const PsroiBin &s, int S, int H, int W)
{
    if (!s.ok) return 0;
    int cnt = 0;
    PsroiSample q;
    for (int ih = 0; ih < S; ++ih)
        for (int iw = 0; iw < S; ++iw) cnt += psroi_sample(s, ih, iw, H, W, q) ? 1 : 0;
    return cnt;
}

// work item -> (region, ph, pw, class, channel block); the order of `partial` and of psroi_trans_reduce_kernel
__device__ __forceinline__ void psroi_item(const PsroiArgs &a, int wid, int &i, int &ph, int &pw, int &cls, int &chunk)
{
    chunk = wid % a.nch;
    int t = wid / a.nch;
    cls = t % a.K;  t /= a.K;
    pw = t % a.P;   t /= a.P;
    ph = t % a.P;
    i = t / a.P;
}

__device__ __forceinline__ float psroi_wave_sum(float v)    // butterfly over the 64 lanes: the same order in every run
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ------------------------------------------------------------------------------------------------------------------------
// channels [0, D*G2) of NCHW `in` (C channels) -> out[(n*HW + p)*CS + cell*D + c], source channel c*G2 + cell; 32 x 32 LDS tile
// over (output channel, pixel) of one group cell: reads and writes are both 128-byte row segments
__global__ void psroi_pack_kernel(const float *__restrict__ in, float *__restrict__ out, int C, int HW, int D, int G2, int dt)
{
    __shared__ float t[32][33];
    const int n = blockIdx.z, cell = blockIdx.y / dt, c0 = (blockIdx.y % dt) * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const size_t CS = (size_t)G2 * D;
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, p = p0 + tx;
        t[r][tx] = (c < D && p < HW) ? in[((size_t)n * C + (size_t)c * G2 + cell) * HW + p] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + r, c = c0 + tx;
        if (c < D && p < HW) out[((size_t)n * HW + p) * CS + (size_t)cell * D + c] = t[tx][r];
    }
}

// the inverse: staging [N*HW][CS] -> NCHW grad_data; the blocks past G2 * dt write zeros into channels [D*G2, C)
__global__ void psroi_unpack_kernel(const float *__restrict__ in, float *__restrict__ out, int C, int HW, int D, int G2, int dt)
{
    __shared__ float t[32][33];
    const int n = blockIdx.z, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if ((int)blockIdx.y >= G2 * dt) {
        const int ch0 = D * G2 + ((int)blockIdx.y - G2 * dt) * 32;
        for (int r = ty; r < 32; r += 8) {
            const int ch = ch0 + r, p = p0 + tx;
            if (ch < C && p < HW) out[((size_t)n * C + ch) * HW + p] = 0.f;
        }
        return;
    }
    const int cell = blockIdx.y / dt, c0 = (blockIdx.y % dt) * 32;
    const size_t CS = (size_t)G2 * D;
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + r, c = c0 + tx;
        t[r][tx] = (c < D && p < HW) ? in[((size_t)n * HW + p) * CS + (size_t)cell * D + c] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, p = p0 + tx;
        if (c < D && p < HW) out[((size_t)n * C + (size_t)c * G2 + cell) * HW + p] = t[tx][r];
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// forward: one wave per work item, lane = output channel of the class
__global__ __launch_bounds__(256) void psroi_forward_kernel(PsroiArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= a.items) return;
    int i, ph, pw, cls, chunk;
    psroi_item(a, wid, i, ph, pw, cls, chunk);
    const int cc = chunk * 64 + lane;                   // channel inside the class
    const bool active = cc < a.cec;
    const int c = cls * a.cec + (active ? cc : 0);      // < D
    const PsroiBin s = psroi_bin(a, i, cls, ph, pw);
    const int cnt = psroi_count(s, a.S, a.H, a.W);
    float sum = 0.f;
    if (cnt > 0 && active) {
        const float *base = a.data + (size_t)s.b * a.H * a.W * a.CS + (size_t)s.cell * a.D + c;
        PsroiSample q;
        for (int ih = 0; ih < a.S; ++ih)
            for (int iw = 0; iw < a.S; ++iw) {
                if (!psroi_sample(s, ih, iw, a.H, a.W, q)) continue;
                const float v11 = base[(size_t)q.o11 * a.CS], v12 = base[(size_t)q.o12 * a.CS];
                const float v21 = base[(size_t)q.o21 * a.CS], v22 = base[(size_t)q.o22 * a.CS];
                const float ux = 1.f - q.dx, uy = 1.f - q.dy;
                sum += ux * uy * v11 + ux * q.dy * v12 + q.dx * uy * v21 + q.dx * q.dy * v22;
            }
    }
    if (active) {
        const size_t o = (((size_t)i * a.D + c) * a.P + ph) * a.P + pw;
        a.out[o] = cnt > 0 ? sum / (float)cnt : 0.f;
        if (a.count) a.count[o] = (float)cnt;
    }
}

// backward: the same work items.  grad_data: every counted sample adds grad_out / count times its corner weight to its corners
// (a corner of weight 0 -- the ceil side at an integer or clamped coordinate -- is skipped: a wave-uniform decision).
// grad_trans: per lane the sum over the samples of grad_out / count * slope, the lanes by a butterfly, times trans_std * roi size.
__global__ __launch_bounds__(256) void psroi_backward_kernel(PsroiArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= a.items) return;
    int i, ph, pw, cls, chunk;
    psroi_item(a, wid, i, ph, pw, cls, chunk);
    const int cc = chunk * 64 + lane;
    const bool active = cc < a.cec;
    const int c = cls * a.cec + (active ? cc : 0);
    const PsroiBin s = psroi_bin(a, i, cls, ph, pw);
    const int cnt = psroi_count(s, a.S, a.H, a.W);
    float sx = 0.f, sy = 0.f;
    if (cnt > 0) {
        const float g = active ? a.gout[(((size_t)i * a.D + c) * a.P + ph) * a.P + pw] / (float)cnt : 0.f;
        const size_t off = (size_t)s.b * a.H * a.W * a.CS + (size_t)s.cell * a.D + c;
        PsroiSample q;
        for (int ih = 0; ih < a.S; ++ih)
            for (int iw = 0; iw < a.S; ++iw) {
                if (!psroi_sample(s, ih, iw, a.H, a.W, q)) continue;
                const float ux = 1.f - q.dx, uy = 1.f - q.dy;
                if (a.gin && active) {
                    float *gb = a.gin + off;
                    const float w11 = ux * uy, w12 = ux * q.dy, w21 = q.dx * uy, w22 = q.dx * q.dy;
                    if (w11 != 0.f) atomicAdd(gb + (size_t)q.o11 * a.CS, g * w11);
                    if (w12 != 0.f) atomicAdd(gb + (size_t)q.o12 * a.CS, g * w12);
                    if (w21 != 0.f) atomicAdd(gb + (size_t)q.o21 * a.CS, g * w21);
                    if (w22 != 0.f) atomicAdd(gb + (size_t)q.o22 * a.CS, g * w22);
                }
                if (a.partial && active) {
                    const float *base = a.data + off;
                    const float v11 = base[(size_t)q.o11 * a.CS], v12 = base[(size_t)q.o12 * a.CS];
                    const float v21 = base[(size_t)q.o21 * a.CS], v22 = base[(size_t)q.o22 * a.CS];
                    sx += g * (uy * (v21 - v11) + q.dy * (v22 - v12));
                    sy += g * (ux * (v12 - v11) + q.dx * (v22 - v21));
                }
            }
    }
    if (a.partial) {
        sx = psroi_wave_sum(sx);
        sy = psroi_wave_sum(sy);
        if (lane == 0) {
            // (a bin without counted samples has no gradient, whatever its region's size: that size may be inf)
            a.partial[(size_t)wid * 2] = cnt > 0 ? a.trans_std * s.roi_w * sx : 0.f;
            a.partial[(size_t)wid * 2 + 1] = cnt > 0 ? a.trans_std * s.roi_h * sy : 0.f;
        }
    }
}

// grad_trans[i][2*cls + xy][qh][qw] = the partials of the bins whose part cell is (qh, qw), added in (ph, pw, channel block)
// order; rows i >= n are zero
__global__ void psroi_trans_reduce_kernel(const float *__restrict__ partial, float *__restrict__ gt, long long total, int n, int P,
                                          int part, int K, int nch)
{
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int qw = (int)(e % part);
        const int qh = (int)((e / part) % part);
        const int ch = (int)((e / ((long long)part * part)) % (2 * K));
        const long long i = e / ((long long)part * part * 2 * K);
        float acc = 0.f;
        if (i < n) {
            const int cls = ch >> 1, xy = ch & 1;
            for (int ph = 0; ph < P; ++ph) {
                if (psroi_part(ph, P, part) != qh) continue;
                for (int pw = 0; pw < P; ++pw) {
                    if (psroi_part(pw, P, part) != qw) continue;
                    const size_t w0 = ((((size_t)i * P + ph) * P + pw) * K + cls) * nch;
                    for (int k = 0; k < nch; ++k) acc += partial[(w0 + k) * 2 + xy];
                }
            }
        }
        gt[e] = acc;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
struct PsroiWs {
    long long data_off, gin_off, partial_off, total;
    int K, cec, nch, CS, items;
};

static bool psroi_sizes_ok(int batch, int channels, int height, int width, int num_rois, int num_classes, int output_dim,
                           int group_size, int pooled_size)
{
    if (batch < 1 || channels < 1 || height < 1 || width < 1 || num_rois < 0 || num_classes < 1 || output_dim < 1 || group_size < 1 ||
        pooled_size < 1)
        return false;
    if (batch > 65535 || group_size > 256 || pooled_size > 4096) return false;
    if (output_dim % num_classes) return false;
    const long long g2 = (long long)group_size * group_size, cs = g2 * output_dim;
    if (cs > channels) return false;
    const long long hw = (long long)height * width;
    if (hw >= (1ll << 31) || (long long)batch * hw * cs >= (1ll << 40)) return false;
    const long long cec = output_dim / num_classes, nch = (cec + 63) / 64;
    if ((long long)num_rois * pooled_size * pooled_size * num_classes * nch >= (1ll << 30)) return false;
    if (g2 * ((output_dim + 31) / 32) + (channels + 31) / 32 > 65535) return false;
    return true;
}

static PsroiWs psroi_ws(int batch, int height, int width, int num_rois, int K, int D, int G, int P, bool backward)
{
    PsroiWs s;
    s.K = K;
    s.cec = D / K;
    s.nch = (s.cec + 63) / 64;
    s.CS = G * G * D;
    s.items = num_rois * P * P * K * s.nch;
    const long long plane = rup256((long long)batch * height * width * s.CS * 4);
    long long o = 0;
    s.data_off = o;    o += plane;
    s.gin_off = o;     if (backward) o += plane;
    s.partial_off = o; if (backward) o += rup256((long long)s.items * 2 * 4);
    s.total = o;
    return s;
}

extern "C" long long m3d_dcn_v2_psroi_pooling_workspace_bytes(int batch, int channels, int height, int width, int num_rois,
                                                              int num_classes, int output_dim, int group_size, int pooled_size,
                                                              int backward)
{
    if (!psroi_sizes_ok(batch, channels, height, width, num_rois, num_classes, output_dim, group_size, pooled_size)) return -1;
    return psroi_ws(batch, height, width, num_rois, num_classes, output_dim, group_size, pooled_size, backward != 0).total;
}

// the argument rules both entry points share; *K = the class count in use
static int psroi_check(const char *name, bool ptrs_ok, int batch, int channels, int height, int width, int num_rois, int trans_rows,
                       int num_classes, int no_trans, float spatial_scale, int output_dim, int group_size, int pooled_size, int part_size,
                       int sample_per_part, float trans_std, const void *workspace, int *K)
{
    M3D_REQUIRE(ptrs_ok, "%s: null pointer", name);
    M3D_REQUIRE(pooled_size >= 1 && sample_per_part >= 1 && group_size >= 1 && part_size >= 1,
                "%s: pooled_size (%d), sample_per_part (%d), group_size (%d) and part_size (%d) must be at least 1", name, pooled_size,
                sample_per_part, group_size, part_size);
    *K = no_trans ? 1 : num_classes;
    M3D_REQUIRE(*K >= 1 && output_dim >= 1 && output_dim % *K == 0, "%s: output_dim (%d) must be a multiple of the class count (%d)", name,
                output_dim, *K);
    M3D_REQUIRE((long long)output_dim * group_size * group_size <= channels,
                "%s: the data has %d channels, output_dim * group_size^2 = %lld are needed", name, channels,
                (long long)output_dim * group_size * group_size);
    M3D_REQUIRE(no_trans || trans_rows >= num_rois, "%s: trans has %d rows for %d regions", name, trans_rows, num_rois);
    M3D_REQUIRE(trans_std >= 0.f && trans_std <= 1.f, "%s: trans_std must lie in [0, 1]", name);
    M3D_REQUIRE(spatial_scale == spatial_scale, "%s: spatial_scale is NaN", name);
    M3D_REQUIRE(sample_per_part <= 1024 && part_size <= 4096, "%s: sample_per_part or part_size too large", name);
    M3D_REQUIRE(no_trans || (trans_rows >= 0 && (long long)trans_rows * 2 * *K * part_size * part_size < (1ll << 31)),
                "%s: trans has %d rows of 2 * %d * %d * %d elements; fewer than 2^31 elements are supported", name, trans_rows, *K, part_size,
                part_size);
    M3D_REQUIRE(psroi_sizes_ok(batch, channels, height, width, num_rois, *K, output_dim, group_size, pooled_size),
                "%s: bad shape or tensor too large", name);
    M3D_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", name);
    return M3D_OK;
}

static int psroi_check_workspace(const char *name, const void *workspace, long long have, long long need)
{
    if (have >= need && (workspace || need == 0)) return M3D_OK;
    m3d_set_error("%s: workspace %lld < %lld bytes (m3d_dcn_v2_psroi_pooling_workspace_bytes)", name, workspace ? have : 0ll, need);
    return M3D_E_WORKSPACE;
}

static PsroiArgs psroi_args(const PsroiWs &s, const float *rois, const float *trans, int batch, int height, int width, int num_rois,
                            int no_trans, float spatial_scale, int output_dim, int group_size, int pooled_size, int part_size,
                            int sample_per_part, float trans_std)
{
    PsroiArgs a = {};
    a.rois = rois;
    a.trans = no_trans ? nullptr : trans;
    a.N = batch; a.H = height; a.W = width; a.n = num_rois; a.D = output_dim; a.G = group_size; a.P = pooled_size;
    a.part = part_size; a.S = sample_per_part; a.K = s.K; a.cec = s.cec; a.nch = s.nch; a.CS = s.CS; a.items = s.items;
    a.scale = spatial_scale; a.trans_std = trans_std;
    return a;
}

static int psroi_pack(const float *data, float *dst, int batch, int channels, int height, int width, int D, int G, hipStream_t stream)
{
    const int HW = height * width, dt = cdiv(D, 32);
    hipLaunchKernelGGL(psroi_pack_kernel, dim3(cdiv(HW, 32), G * G * dt, batch), dim3(256), 0, stream, data, dst, channels, HW, D, G * G, dt);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

extern "C" int m3d_dcn_v2_psroi_pooling_forward(const float *data, const float *rois, const float *trans, float *out, float *top_count,
                                                int batch, int channels, int height, int width, int num_rois, int trans_rows,
                                                int num_classes, int no_trans, float spatial_scale, int output_dim, int group_size,
                                                int pooled_size, int part_size, int sample_per_part, float trans_std, void *workspace,
                                                long long workspace_bytes, m3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *name = "dcn_v2_psroi_pooling_forward";
    int rc, K;
    if ((rc = psroi_check(name, data && (num_rois == 0 || (rois && out)) && (no_trans || num_rois == 0 || trans), batch, channels, height,
                          width, num_rois, trans_rows, num_classes, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                          sample_per_part, trans_std, workspace, &K)))
        return rc;
    if (num_rois == 0) return M3D_OK;
    const PsroiWs s = psroi_ws(batch, height, width, num_rois, K, output_dim, group_size, pooled_size, false);
    if ((rc = psroi_check_workspace(name, workspace, workspace_bytes, s.total))) return rc;
    float *dn = (float *)((char *)workspace + s.data_off);
    if ((rc = psroi_pack(data, dn, batch, channels, height, width, output_dim, group_size, stream))) return rc;
    PsroiArgs a = psroi_args(s, rois, trans, batch, height, width, num_rois, no_trans, spatial_scale, output_dim, group_size, pooled_size,
                             part_size, sample_per_part, trans_std);
    a.data = dn; a.out = out; a.count = top_count;
    hipLaunchKernelGGL(psroi_forward_kernel, dim3(cdiv(s.items, 4)), dim3(256), 0, stream, a);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

extern "C" int m3d_dcn_v2_psroi_pooling_backward(const float *grad_out, const float *data, const float *rois, const float *trans,
                                                 float *grad_data, float *grad_trans, int batch, int channels, int height, int width,
                                                 int num_rois, int trans_rows, int num_classes, int no_trans, float spatial_scale,
                                                 int output_dim, int group_size, int pooled_size, int part_size, int sample_per_part,
                                                 float trans_std, void *workspace, long long workspace_bytes, m3d_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *name = "dcn_v2_psroi_pooling_backward";
    int rc, K;
    if ((rc = psroi_check(name, data && (num_rois == 0 || (rois && grad_out)) && (no_trans || num_rois == 0 || trans), batch, channels,
                          height, width, num_rois, trans_rows, num_classes, no_trans, spatial_scale, output_dim, group_size, pooled_size,
                          part_size, sample_per_part, trans_std, workspace, &K)))
        return rc;
    if (no_trans) grad_trans = nullptr;                  // there is no trans tensor: nothing to write
    if (!grad_data && !grad_trans) return M3D_OK;
    const long long trans_elems = no_trans ? 0 : (long long)trans_rows * 2 * K * part_size * part_size;
    if (num_rois == 0) {                                 // no region: zero gradients, no launch
        if (grad_data) M3D_HIP(hipMemsetAsync(grad_data, 0, (size_t)batch * channels * height * width * 4, stream));
        if (grad_trans && trans_elems) M3D_HIP(hipMemsetAsync(grad_trans, 0, (size_t)trans_elems * 4, stream));
        return M3D_OK;
    }
    const PsroiWs s = psroi_ws(batch, height, width, num_rois, K, output_dim, group_size, pooled_size, true);
    if ((rc = psroi_check_workspace(name, workspace, workspace_bytes, s.total))) return rc;
    char *ws = (char *)workspace;
    float *dn = (float *)(ws + s.data_off), *gin = (float *)(ws + s.gin_off), *partial = (float *)(ws + s.partial_off);
    const int HW = height * width, G2 = group_size * group_size, dt = cdiv(output_dim, 32);
    if (grad_trans && (rc = psroi_pack(data, dn, batch, channels, height, width, output_dim, group_size, stream))) return rc;
    if (grad_data) M3D_HIP(hipMemsetAsync(gin, 0, (size_t)batch * HW * s.CS * 4, stream));
    PsroiArgs a = psroi_args(s, rois, trans, batch, height, width, num_rois, no_trans, spatial_scale, output_dim, group_size, pooled_size,
                             part_size, sample_per_part, trans_std);
    a.data = grad_trans ? dn : nullptr; a.gout = grad_out; a.gin = grad_data ? gin : nullptr; a.partial = grad_trans ? partial : nullptr;
    hipLaunchKernelGGL(psroi_backward_kernel, dim3(cdiv(s.items, 4)), dim3(256), 0, stream, a);
    M3D_LAUNCH_CHECK();
    if (grad_data) {
        hipLaunchKernelGGL(psroi_unpack_kernel, dim3(cdiv(HW, 32), G2 * dt + cdiv(channels - G2 * output_dim, 32), batch), dim3(256), 0,
                           stream, gin, grad_data, channels, HW, output_dim, G2, dt);
        M3D_LAUNCH_CHECK();
    }
    if (grad_trans) {
        hipLaunchKernelGGL(psroi_trans_reduce_kernel, dim3(imin(cdiv(trans_elems, 256), 4096)), dim3(256), 0, stream, partial, grad_trans,
                           trans_elems, num_rois, pooled_size, part_size, K, s.nch);
        M3D_LAUNCH_CHECK();
    }
    return M3D_OK;
}
