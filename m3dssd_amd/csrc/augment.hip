// Training augmentation on the device: the image path of the reference's lib.augmentations.Augmentation (photometric distortion,
// RandomMirror, RandomTransform, Normalize; augmentations.py:164-234,236-469) followed by the BGR->RGB swap and the HWC->CHW
// permute of lib/dataloader.py:943-950, for a batch of uint8 BGR frames, in one launch.
//
// The random decisions are made on the host (m3dssd_amd/host/augment.py: draw_params); what arrives here per image is the source
// size, ONE inverse 2x3 matrix in float64 with the mirror folded in (x_src = (w - 1) - u) and the photometric parameters.  Per
// output pixel: (u, v) = Minv . (x, y, 1) in float64 with separate multiplies and adds (the bits numpy produces), four bilinear
// taps at the exact coordinate, the photometric step per tap (the reference distorts the whole source before it warps, so the
// constant border stays 0 and normalises to (0 - mean) / std), the blend in float32, then /255, -mean, /stds as u8_normalise of
// backbone_kernels.hip does it.  No atomics: the output is a pure function of the inputs.
//
// Two documented differences from OpenCV: warpAffine quantises the source coordinate to 1/32 pixel and reads
// the weights from a table, this kernel interpolates at the exact coordinate; and the HSV formulas are OpenCV's float forms as
// documented, not checked against a cv2 binary (tests/augment_ref.py is the contract).
#include <float.h>
#include <math.h>

#include "common.h"

// every expression in this file is evaluated as written: no fma contraction (floor(), the fractions and the float32 arithmetic
// are compared with numpy's)
#pragma clang fp contract(off)

#define AUG_MAX_IMGS 16     // images per launch: their parameters travel as kernel arguments (80 bytes each)
#define AUG_PX 4            // consecutive x per thread: one 16-byte store per plane
#define AUG_BX 64
#define AUG_BY 4

struct AugImg {
    double m[6];                        // Minv, row major 2x3
    float delta, alpha, sat, hue;
    int h, w, mode, pad_;               // mode: 0 none, 1 contrast first, 2 contrast last
};
struct AugArgs {
    AugImg img[AUG_MAX_IMGS];
    float mean[3], stds[3];             // indexed by BGR position, as the reference applies them
};

// PhotometricDistort on one float BGR value (augmentations.py:236-321,375-430), cv2.cvtColor's float BGR<->HSV in between.
__host__ __device__ __forceinline__ void aug_photometric(float (&px)[3], const AugImg &p)
{
    float b = px[0] + p.delta, g = px[1] + p.delta, r = px[2] + p.delta;
    if (p.mode == 1) { b *= p.alpha; g *= p.alpha; r *= p.alpha; }
    // BGR -> HSV
    const float v = fmaxf(fmaxf(b, g), r), vmin = fminf(fminf(b, g), r);
    const float diff = v - vmin;
    float s = diff / (fabsf(v) + FLT_EPSILON);
    const float k = 60.0f / (diff + FLT_EPSILON);
    float h;
    if (v == r) h = (g - b) * k;
    else if (v == g) h = (b - r) * k + 120.0f;
    else h = (r - g) * k + 240.0f;
    if (h < 0.0f) h += 360.0f;
    // RandomSaturation, RandomHue
    s *= p.sat;
    h += p.hue;
    if (h > 360.0f) h -= 360.0f;
    if (h < 0.0f) h += 360.0f;
    // HSV -> BGR
    if (s == 0.0f) {
        b = g = r = v;
    } else {
        float hh = h / 60.0f;
        if (hh < 0.0f) hh += 6.0f;
        else if (hh >= 6.0f) hh -= 6.0f;
        float fs = floorf(hh);
        hh -= fs;
        if (!(fs >= 0.0f && fs < 6.0f)) { fs = 0.0f; hh = 0.0f; }
        const int sector = (int)fs;
        const float t1 = v * (1.0f - s), t2 = v * (1.0f - s * hh), t3 = v * (1.0f - s * (1.0f - hh));
        // sector -> (b, g, r): 0 (t1 t3 v) 1 (t1 v t2) 2 (t3 v t1) 3 (v t2 t1) 4 (v t1 t3) 5 (t2 t1 v)
        b = sector == 0 || sector == 1 ? t1 : sector == 2 ? t3 : sector == 5 ? t2 : v;
        g = sector == 0 ? t3 : sector == 1 || sector == 2 ? v : sector == 3 ? t2 : t1;
        r = sector == 0 || sector == 5 ? v : sector == 1 ? t2 : sector == 4 ? t3 : t1;
    }
    if (p.mode == 2) { b *= p.alpha; g *= p.alpha; r *= p.alpha; }
    px[0] = b; px[1] = g; px[2] = r;
}

// acc += wgt * tap(y, x); a tap outside the image or with weight 0 is not read and adds nothing
__host__ __device__ __forceinline__ void aug_tap(const unsigned char *__restrict__ frame, int wmax, const AugImg &p, int y, int x, float wgt,
                                        float (&acc)[3])
{
    if (wgt == 0.0f || (unsigned)x >= (unsigned)p.w || (unsigned)y >= (unsigned)p.h) return;
    const unsigned char *q = frame + ((size_t)y * wmax + x) * 3;
    float px[3] = {(float)q[0], (float)q[1], (float)q[2]};
    if (p.mode != 0) aug_photometric(px, p);
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + wgt * px[c];
}

// one output pixel: the three normalised values by BGR position (host-callable: the arithmetic has no device-only part)
__host__ __device__ __forceinline__ void aug_pixel(const unsigned char *__restrict__ frame, int wmax, const AugImg &p, const float *mean,
                                                   const float *stds, int x, int y, float (&res)[3])
{
    const double xd = (double)x, yd = (double)y;
    const double u = p.m[0] * xd + p.m[1] * yd + p.m[2];
    const double v = p.m[3] * xd + p.m[4] * yd + p.m[5];
    const double fu = floor(u), fv = floor(v);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    // a pixel with a tap inside has fu in [-1, w - 1] and fv in [-1, h - 1]; everything else (NaN included) is border
    if (fu >= -1.0 && fu <= (double)(p.w - 1) && fv >= -1.0 && fv <= (double)(p.h - 1)) {
        const int sx = (int)fu, sy = (int)fv;
        const float fx = (float)(u - fu), fy = (float)(v - fv);
        const float gx = 1.0f - fx, gy = 1.0f - fy;
        aug_tap(frame, wmax, p, sy, sx, gx * gy, acc);
        aug_tap(frame, wmax, p, sy, sx + 1, fx * gy, acc);
        aug_tap(frame, wmax, p, sy + 1, sx, gx * fy, acc);
        aug_tap(frame, wmax, p, sy + 1, sx + 1, fx * fy, acc);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {           // Normalize (augmentations.py:44-57): IEEE division, numpy's order
        float t = acc[c] / 255.0f;
        t = t - mean[c];
        res[c] = t / stds[c];
    }
}

__global__ __launch_bounds__(AUG_BX *AUG_BY) void augment_u8_kernel(const unsigned char *__restrict__ frames, float *__restrict__ out,
                                                                     int hmax, int wmax, int H, int W, int vec_store, AugArgs a)
{
    const int n = blockIdx.z;
    const int y = blockIdx.y * AUG_BY + threadIdx.y;
    const int x0 = (blockIdx.x * AUG_BX + threadIdx.x) * AUG_PX;
    if (y >= H || x0 >= W) return;
    const AugImg &p = a.img[n];
    const unsigned char *frame = frames + (size_t)n * hmax * wmax * 3;
    float res[3][AUG_PX];
#pragma unroll
    for (int i = 0; i < AUG_PX; ++i) {
        float r3[3];
        aug_pixel(frame, wmax, p, a.mean, a.stds, x0 + i, y, r3);
#pragma unroll
        for (int c = 0; c < 3; ++c) res[c][i] = r3[c];
    }
    const size_t plane = (size_t)H * W;
    float *o = out + (size_t)n * 3 * plane + (size_t)y * W + x0;
    if (vec_store) {                        // W % 4 == 0 and a 16-byte aligned base: every row start and every x0 is aligned
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            u32x4 d;
#pragma unroll
            for (int i = 0; i < AUG_PX; ++i) d[i] = __float_as_uint(res[c][i]);
            global_store_u32x4_nop(o + (size_t)(2 - c) * plane, d);       // BGR position c -> RGB plane 2 - c
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < AUG_PX; ++i)
                if (x0 + i < W) o[(size_t)(2 - c) * plane + i] = res[c][i];
    }
}

extern "C" int m3d_augment_u8(const unsigned char *frames_bgr, int N, int hmax, int wmax, const double *params, int param_stride,
                              const float *mean3, const float *stds3, float *out_nchw, int H, int W, m3d_stream_t stream)
{
    M3D_REQUIRE(frames_bgr && params && mean3 && stds3 && out_nchw, "augment_u8: null pointer");
    M3D_REQUIRE(N >= 1 && hmax >= 1 && wmax >= 1 && H >= 1 && W >= 1 && param_stride >= M3D_AUGMENT_PARAMS,
                "augment_u8: bad sizes (N %d, buffer %dx%d, out %dx%d, param_stride %d)", N, hmax, wmax, H, W, param_stride);
    M3D_REQUIRE((long long)hmax * wmax * 3 < (1ll << 31) && (long long)H * W < (1ll << 31) && H <= 65535 * AUG_BY,
                "augment_u8: frame too large");
    for (int c = 0; c < 3; ++c) M3D_REQUIRE(isfinite(mean3[c]) && isfinite(stds3[c]) && stds3[c] != 0.f, "augment_u8: bad mean / std");
    // every image is validated before the first launch
    for (int n = 0; n < N; ++n) {
        const double *q = params + (size_t)n * param_stride;
        for (int k = 0; k < M3D_AUGMENT_PARAMS; ++k) M3D_REQUIRE(isfinite(q[k]), "augment_u8: image %d: parameter %d is not finite", n, k);
        M3D_REQUIRE(q[0] >= 1 && q[1] >= 1 && q[0] <= hmax && q[1] <= wmax && q[0] == floor(q[0]) && q[1] == floor(q[1]),
                    "augment_u8: image %d: size %gx%g does not fit the buffer %dx%d", n, q[0], q[1], hmax, wmax);
        M3D_REQUIRE(q[2] == 0 || q[2] == 1 || q[2] == 2, "augment_u8: image %d: photometric mode %g (0 none, 1 contrast first, 2 last)", n, q[2]);
        M3D_REQUIRE(fabs(q[6]) <= 360.0, "augment_u8: image %d: hue shift %g outside [-360, 360]", n, q[6]);
        const double det = q[8] * q[12] - q[9] * q[11];
        M3D_REQUIRE(isfinite(det) && det != 0.0, "augment_u8: image %d: singular matrix", n);
    }
    const int vec_store = (W % AUG_PX) == 0 && ((size_t)out_nchw & 15) == 0;
    for (int n0 = 0; n0 < N; n0 += AUG_MAX_IMGS) {
        const int nb = imin(AUG_MAX_IMGS, N - n0);
        AugArgs a = {};
        for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.stds[c] = stds3[c]; }
        for (int i = 0; i < nb; ++i) {
            const double *q = params + (size_t)(n0 + i) * param_stride;
            AugImg &g = a.img[i];
            g.h = (int)q[0]; g.w = (int)q[1]; g.mode = (int)q[2];
            g.delta = (float)q[3]; g.alpha = (float)q[4]; g.sat = (float)q[5]; g.hue = (float)q[6];
            for (int k = 0; k < 6; ++k) g.m[k] = q[8 + k];
        }
        hipLaunchKernelGGL(augment_u8_kernel, dim3(cdiv(cdiv(W, AUG_PX), AUG_BX), cdiv(H, AUG_BY), nb), dim3(AUG_BX, AUG_BY), 0,
                           (hipStream_t)stream, frames_bgr + (size_t)n0 * hmax * wmax * 3, out_nchw + (size_t)n0 * 3 * H * W, hmax,
                           wmax, H, W, vec_store, a);
        M3D_LAUNCH_CHECK();
    }
    return M3D_OK;
}
