// RPN_3D_loss on the device (lib/loss/rpn_3d.py:14-657 with compute_targets, lib/rpn_util.py:430-532): target assignment,
// hard-negative sampling and the fused loss + gradients.  The reference runs this stage in host numpy, one image at a time, after
// copying `prob` to the host; here nothing crosses to the host between launches.
//
// Row r of an image is anchor (a, h, w) with r = (a*H + h)*W + w; its roi is float32(w*stride + anchors[a][0..3]) evaluated in
// float64 first (locate_anchors(...).float()).  Everything a LABEL depends on follows the reference's arithmetic operation by
// operation, with contraction off for the whole file:
//   overlap  = inter / ((area_a + area_b) - inter), inter = max(min(x2) - max(x1), 0) * max(min(y2) - max(y1), 0), float64, where
//              area_a = (x2 - x1) * (y2 - y1) of the roi is a FLOAT32 product (the rois reach compute_targets as a float32 array)
//              and area_b of the ground truth is float64;
//   ignore   = inter / area_a (iou_ign: `area_b * 0 - inter * 0`).
// On seeded inputs several anchors share a ground truth's best overlap bit for bit (np.argmax takes the lowest row), so the
// per-gt arg-max over all workgroups is done exactly: launch 1 takes the maximum of the overlap's bit pattern (an unsigned
// 64-bit vector atomic max: order-independent), launch 2 takes the minimum row among the anchors whose overlap equals it (an
// unsigned 32-bit vector atomic min), launch 3 recomputes the same bits once more and assigns.  Integer max / min / add only:
// the result does not depend on arrival order.
//
// m3d_rpn_target_stats (compute_bbox_stats, lib/rpn_util.py:732-889: the means and stds of the raw transforms over a dataset) runs
// launches 1-3 with the roi kept in FLOAT64 -- that function hands locate_anchors' float64 array over without the loss' cast --
// so the roi arithmetic is generic over its scalar type (RpnRoiT<T>); T = float is the loss path, bit for bit what it was.
//
// Launches (m3d_rpn_targets: 1-3, m3d_rpn_loss: 4-6; m3d_rpn_precompute_targets: 1-3 without cls / prob; m3d_rpn_loss_smp: the
// ingest launch, then 4-6; m3d_rpn_target_stats: 1, 2, 3S, S):
//   3S rpn_stats_kernel      launch 3's decisions on float64 rois; writes no labels and no targets: per workgroup n_fg and the
//                            float64 sums of (t32 - center) and its square over the fg rows, t32 the float32-rounded transform
//   S rpn_stats_finish_kernel per image: adds its workgroups' partials in a fixed order -> out[b][23]
//   1 rpn_gt_max_kernel     per anchor x valid gt: overlap -> max of its bits over 1 024 anchors on chip, one atomic max per gt
//   2 rpn_gt_row_kernel     per anchor x valid gt: overlap == max -> atomic min of the row per gt
//   3 rpn_assign_kernel     per anchor: row max / arg-max, ignore overlap, label, gt index, the 11 normalised regression targets,
//                           the score prob[label] the sampling sorts by, and the fg / bg counts + arg-max accuracy counts
//   I rpn_ingest_kernel     (RPN_3D_loss_smp, lib/loss/rpn_3d.py:659-1360: targets arrive pre-computed) per anchor: the label as the
//                           data loader collates it (int64) or as launch 3 writes it (int16) -> checked int16 label, the score
//                           prob[label], the packed targets and the same per-image counts launch 3 leaves, + a bad-label count
//   4 rpn_select_kernel     per (image, fg | bg): the k lowest (score, row) keys by radix select (8-bit digits over the sortable
//                           score bits, then over the row among the scores equal to the threshold) -> a threshold key
//   5 rpn_loss_kernel       per anchor (at most 2 048 workgroups stride over the rows): sampled iff key <= threshold; weighted
//                           cross-entropy, smooth-L1, -log IoU, the stats and the three gradients (zero where not sampled) in
//                           float64, partial sums per workgroup
//   6 rpn_finish_kernel     adds the partials in a fixed order, divides by the batch-wide counts, writes loss and stat block
// Sums are float64 in fixed orders (a thread's rows in order, lane butterfly, waves in order, workgroups strided then a tree):
// loss, stats and gradients are bitwise reproducible from run to run.
#include <math.h>
#include <string.h>

#include "common.h"

#pragma clang fp contract(off)

#define RPN_TPB 256
#define RPN_SEL_TPB 1024
#define RPN_NQ 16              // partial sums per workgroup of launch 5
#define RPN_LOSS_MAX_WG 2048    // launch 5 strides over the rows with at most this many workgroups (256 CUs x 8)
#define RPN_IGN_LABEL 3000     // IGN_FLAG of the reference

struct RpnConf {
    double mean[11], stdv[11];
    double fg_thresh, ign_thresh, bg_lo, bg_hi, best_thresh;
    double box_samples, fg_fraction, focal, lam_cls, lam_iou, lam_2d, lam_3d, stride;
};

struct RpnWs {
    unsigned long long *gtmax;   // [B][M3D_RPN_MAX_GT] bits of the best overlap per valid gt
    unsigned *bestrow;           // [B][M3D_RPN_MAX_GT] lowest row with that overlap
    int *counts;                 // [B][8]: 0 fg, 1 bg, 2 fg arg-max correct, 3 bg arg-max correct, 4 labels outside the allowed set (ingest)
    unsigned *sel;               // [B][2][8]: 0 mode (0 none, 1 all, 2 threshold), 1 score key, 2 row, 3 selected, 4 selected with score 1
    double *partials;            // [workgroups of launch 5][RPN_NQ]
    long long total;
};

static RpnWs rpn_ws_layout(void *base, int B, long long R)
{
    RpnWs w;
    char *p = (char *)base;
    long long o = 0;
    w.gtmax = (unsigned long long *)(p + o); o += (long long)B * M3D_RPN_MAX_GT * 8;
    w.bestrow = (unsigned *)(p + o); o += (long long)B * M3D_RPN_MAX_GT * 4;
    w.counts = (int *)(p + o); o += (long long)B * 8 * 4;
    w.sel = (unsigned *)(p + o); o += (long long)B * 2 * 8 * 4;
    o = (o + 255) / 256 * 256;
    w.partials = (double *)(p + o); o += (long long)imin(cdiv((long long)B * R, RPN_TPB), RPN_LOSS_MAX_WG) * RPN_NQ * 8;
    w.total = o;
    return w;
}

// assign_only (m3d_rpn_target_stats): only the thresholds and the stride are read; means, stds and the loss settings are not
// checked (the caller is about to compute the means and stds).
static int rpn_conf_from(const double *c, int n, RpnConf *o, const char *who, bool assign_only = false)
{
    M3D_REQUIRE(c && n == M3D_RPN_CONF_COUNT, "%s: conf must hold M3D_RPN_CONF_COUNT = %d doubles (got %d)", who, M3D_RPN_CONF_COUNT, n);
    for (int i = 0; i < 11; ++i) { o->mean[i] = c[M3D_RPN_CONF_MEANS + i]; o->stdv[i] = c[M3D_RPN_CONF_STDS + i]; }
    o->fg_thresh = c[M3D_RPN_CONF_FG_THRESH]; o->ign_thresh = c[M3D_RPN_CONF_IGN_THRESH];
    o->bg_lo = c[M3D_RPN_CONF_BG_LO]; o->bg_hi = c[M3D_RPN_CONF_BG_HI]; o->best_thresh = c[M3D_RPN_CONF_BEST_THRESH];
    o->box_samples = c[M3D_RPN_CONF_BOX_SAMPLES]; o->fg_fraction = c[M3D_RPN_CONF_FG_FRACTION]; o->focal = c[M3D_RPN_CONF_FOCAL];
    o->lam_cls = c[M3D_RPN_CONF_LAMBDA_CLS]; o->lam_iou = c[M3D_RPN_CONF_LAMBDA_IOU];
    o->lam_2d = c[M3D_RPN_CONF_LAMBDA_2D]; o->lam_3d = c[M3D_RPN_CONF_LAMBDA_3D]; o->stride = c[M3D_RPN_CONF_STRIDE];
    M3D_REQUIRE(o->stride > 0, "%s: feat_stride must be positive", who);
    if (assign_only) return M3D_OK;
    for (int i = 0; i < 11; ++i) M3D_REQUIRE(o->stdv[i] != 0.0 && isfinite(o->stdv[i]) && isfinite(o->mean[i]), "%s: bbox_means / bbox_stds must be finite, stds non-zero", who);
    M3D_REQUIRE(o->box_samples > 0, "%s: box_samples must be positive or inf", who);
    M3D_REQUIRE(isinf(o->box_samples) || (o->fg_fraction >= 0 && o->fg_fraction <= 1),
                "%s: a finite box_samples needs fg_fraction in [0, 1] (the reference multiplies by it)", who);
    M3D_REQUIRE(isnan(o->fg_fraction) || (o->fg_fraction >= 0 && o->fg_fraction < 1), "%s: fg_fraction must be in [0, 1) or NaN for None", who);
    M3D_REQUIRE(o->focal >= 0, "%s: focal_loss must be >= 0", who);
    return M3D_OK;
}

// ---- shared geometry ---------------------------------------------------------------------------------------------------
// T is the scalar type the roi reaches compute_targets in: float for the loss (locate_anchors(...).float()), double for the
// dataset statistics (compute_bbox_stats hands the float64 rois of locate_anchors over as they are).  T = float is the
// arithmetic this file always had; both instantiations evaluate the same expressions in the same order.
template <typename T>
struct RpnRoiT {
    T x1, y1, x2, y2;
    int a;
};
typedef RpnRoiT<float> RpnRoi;

template <typename T>
__device__ __forceinline__ RpnRoiT<T> rpn_roi(const double *__restrict__ anchors, int r, int H, int W, double stride)
{
    RpnRoiT<T> o;
    const int hw = H * W;
    o.a = r / hw;
    const int rem = r - o.a * hw;
    const int h = rem / W, w = rem - h * W;
    const double sx = (double)w * stride, sy = (double)h * stride;
    const double *an = anchors + o.a * 9;
    o.x1 = (T)(sx + an[0]);
    o.y1 = (T)(sy + an[1]);
    o.x2 = (T)(sx + an[2]);
    o.y2 = (T)(sy + an[3]);
    return o;
}

template <typename T>
__device__ __forceinline__ double rpn_inter(const RpnRoiT<T> &q, const double *g)
{
    const double iw = fmax(fmin((double)q.x2, g[2]) - fmax((double)q.x1, g[0]), 0.0);
    const double ih = fmax(fmin((double)q.y2, g[3]) - fmax((double)q.y1, g[1]), 0.0);
    return iw * ih;
}
// g: x1 y1 x2 y2 area
template <typename T>
__device__ __forceinline__ double rpn_iou(const RpnRoiT<T> &q, double area_a, const double *g)
{
    const double inter = rpn_inter(q, g);
    const double uni = (area_a + g[4]) - inter;
    return inter / uni;
}
template <typename T>
__device__ __forceinline__ double rpn_roi_area(const RpnRoiT<T> &q)
{
    const T w = q.x2 - q.x1, h = q.y2 - q.y1;
    const T a = w * h;
    return (double)a;
}

// the gt table of one image -> LDS: sg[g][0..4] = x1 y1 x2 y2 area for the valid rows, then the ignore rows
__device__ __forceinline__ void rpn_load_gts(const double *__restrict__ gt, int Gmax, int b, double (*sg)[5], int &n_val, int &n_ign)
{
    const double *t = gt + (size_t)b * (Gmax + 1) * M3D_RPN_GT_COLS;
    int nv = (int)t[0], ni = (int)t[1];
    nv = max(0, min(nv, Gmax));
    ni = max(0, min(ni, Gmax - nv));
    for (int i = threadIdx.x; i < (nv + ni) * 5; i += blockDim.x) {
        const int g = i / 5, c = i - g * 5;
        const double *row = t + (size_t)(g + 1) * M3D_RPN_GT_COLS;
        sg[g][c] = c < 4 ? row[c] : (row[2] - row[0]) * (row[3] - row[1]);
    }
    n_val = nv;
    n_ign = ni;
    __syncthreads();
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- launch 1 ----------------------------------------------------------------------------------------------------------
#define RPN_MAX_ROWS 4          // rows per thread of launch 1: 1024 anchors share one atomic per gt
template <typename T>
__global__ __launch_bounds__(RPN_TPB) void rpn_gt_max_kernel(const double *__restrict__ anchors, const double *__restrict__ gt, int Gmax,
                                                             int R, int H, int W, double stride, unsigned long long *__restrict__ gtmax)
{
    __shared__ double sg[M3D_RPN_MAX_GT][5];
    __shared__ unsigned long long sm[RPN_TPB / 64];
    const int b = blockIdx.y;
    int nv, ni;
    rpn_load_gts(gt, Gmax, b, sg, nv, ni);
    if (nv == 0) return;
    RpnRoiT<T> q[RPN_MAX_ROWS];
    double area[RPN_MAX_ROWS];
    bool live[RPN_MAX_ROWS];
#pragma unroll
    for (int u = 0; u < RPN_MAX_ROWS; ++u) {
        const int r = (blockIdx.x * RPN_MAX_ROWS + u) * RPN_TPB + threadIdx.x;
        live[u] = r < R;
        q[u] = rpn_roi<T>(anchors, live[u] ? r : 0, H, W, stride);
        area[u] = rpn_roi_area(q[u]);
    }
    for (int g = 0; g < nv; ++g) {
        unsigned long long bits = 0ull;
#pragma unroll
        for (int u = 0; u < RPN_MAX_ROWS; ++u) {
            const double v = rpn_iou(q[u], area[u], sg[g]);
            const unsigned long long bu = (live[u] && v > 0.0) ? (unsigned long long)__double_as_longlong(v) : 0ull;   // NaN / 0: 0
            bits = bu > bits ? bu : bits;
        }
        bits = wave_max_u64(bits);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = bits;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long m = sm[0];
            for (int w = 1; w < RPN_TPB / 64; ++w) m = sm[w] > m ? sm[w] : m;
            if (m > gtmax[b * M3D_RPN_MAX_GT + g]) atomicMax(&gtmax[b * M3D_RPN_MAX_GT + g], m);
        }
        __syncthreads();
    }
}

// ---- launch 2 ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(RPN_TPB) void rpn_gt_row_kernel(const double *__restrict__ anchors, const double *__restrict__ gt, int Gmax,
                                                             int R, int H, int W, double stride,
                                                             const unsigned long long *__restrict__ gtmax, unsigned *__restrict__ bestrow)
{
    __shared__ double sg[M3D_RPN_MAX_GT][5];
    const int b = blockIdx.y;
    int nv, ni;
    rpn_load_gts(gt, Gmax, b, sg, nv, ni);
    if (nv == 0) return;
    const int r = blockIdx.x * RPN_TPB + threadIdx.x;
    const bool live = r < R;
    const RpnRoiT<T> q = rpn_roi<T>(anchors, live ? r : 0, H, W, stride);
    const double area = rpn_roi_area(q);
    for (int g = 0; g < nv; ++g) {
        const double v = rpn_iou(q, area, sg[g]);
        const unsigned long long bits = (v > 0.0) ? (unsigned long long)__double_as_longlong(v) : 0ull;
        const bool eq = live && bits == gtmax[b * M3D_RPN_MAX_GT + g];
        const unsigned long long m = __ballot(eq);
        // rows grow with the lane: the first matching lane holds the wave's lowest row
        if (m != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1 && (unsigned)r < bestrow[b * M3D_RPN_MAX_GT + g])
            atomicMin(&bestrow[b * M3D_RPN_MAX_GT + g], (unsigned)r);
    }
}

// ---- launch 3 ----------------------------------------------------------------------------------------------------------
struct RpnAssignArgs {
    const double *anchors, *gt;
    const float *cls, *prob;
    const unsigned long long *gtmax;
    const unsigned *bestrow;
    short *labels, *gt_index;
    float *targets, *scores;
    int *counts;
    int Gmax, R, H, W, C;
    float *tar_2d, *tar_3d;      // PRE only: the targets as [B, R, 4] and [B, R, 7] (the data loader's layout) instead of `targets`
    int *any_val;                // PRE only: [B], 1 where the image has a valid gt
};

__device__ __forceinline__ float rpn_norm(double t, double mean, double stdv)
{
    // float32 array -= means; /= stds: each step evaluated in float64 and stored as float32
    const float t32 = (float)t;
    const float s = (float)((double)t32 - mean);
    return (float)((double)s / stdv);
}

struct RpnRow {
    int label, gidx;
    bool is_fg, is_bg;
};

// One row of an image with a valid gt (nv > 0): the label decision and the raw (not normalised) transforms t[0..10], 0 where the
// row is not fg.  Shared by every form of launch 3; T as in RpnRoiT.
template <typename T>
__device__ __forceinline__ RpnRow rpn_assign_row(const double *__restrict__ anchors, const double *__restrict__ gt,
                                                 const unsigned long long *__restrict__ gtmax, const unsigned *__restrict__ bestrow,
                                                 int Gmax, int H, int W, int b, int r, bool live, int nv, int ni,
                                                 const double (*sg)[5], const RpnConf &cf, double *t)
{
    RpnRow o;
    o.label = 0;
    o.gidx = -1;
    const RpnRoiT<T> q = rpn_roi<T>(anchors, live ? r : 0, H, W, cf.stride);
    const double area = rpn_roi_area(q);
    double ols_max = -1.0;
    int arg = 0;
    bool best = false;
    for (int g = 0; g < nv; ++g) {
        const double v = rpn_iou(q, area, sg[g]);
        if (v > ols_max) { ols_max = v; arg = g; }
        const unsigned long long mx = gtmax[b * M3D_RPN_MAX_GT + g];
        best = best || (bestrow[b * M3D_RPN_MAX_GT + g] == (unsigned)r && __longlong_as_double((long long)mx) >= cf.best_thresh);
    }
    double ign_max = 0.0;      // np.zeros when the image has no ignore region
    for (int g = nv; g < nv + ni; ++g) {
        const double v = rpn_inter(q, sg[g]) / area;
        if (v > ign_max) ign_max = v;
    }
    o.is_fg = (ols_max >= cf.fg_thresh) || best;
    const bool is_ign = ign_max >= cf.ign_thresh;
    o.is_bg = (ols_max >= cf.bg_lo) && (ols_max < cf.bg_hi) && !is_ign && !o.is_fg;
    const double *grow = gt + ((size_t)b * (Gmax + 1) + 1 + arg) * M3D_RPN_GT_COLS;
#pragma unroll
    for (int i = 0; i < 11; ++i) t[i] = 0.0;
    if (o.is_fg) {
        o.gidx = arg;
        o.label = (int)grow[4];
        // bbox_transform / bbox_transform_3d: the roi side in T (the dtype of the roi array), the gt side in float64
        const T ex_w = q.x2 - q.x1 + (T)1.0, ex_h = q.y2 - q.y1 + (T)1.0;
        const T ex_cx = q.x1 + (T)0.5 * (ex_w - (T)1.0), ex_cy = q.y1 + (T)0.5 * (ex_h - (T)1.0);
        const double gw = grow[2] - grow[0] + 1.0, gh = grow[3] - grow[1] + 1.0;
        const double gcx = grow[0] + 0.5 * (gw - 1.0), gcy = grow[1] + 0.5 * (gh - 1.0);
        t[0] = (gcx - (double)ex_cx) / (double)ex_w;
        t[1] = (gcy - (double)ex_cy) / (double)ex_h;
        t[2] = log(gw / (double)ex_w);
        t[3] = log(gh / (double)ex_h);
        const double *an = anchors + q.a * 9;
        t[4] = (grow[5] - (double)ex_cx) / (double)ex_w;
        t[5] = (grow[6] - (double)ex_cy) / (double)ex_h;
        t[6] = grow[7] - an[4];
        t[7] = log(grow[8] / an[5]);
        t[8] = log(grow[9] / an[6]);
        t[9] = log(grow[10] / an[7]);
        t[10] = grow[11] - an[8];
    } else if (!o.is_bg) {
        o.label = RPN_IGN_LABEL;
    }
    return o;
}

// PRE (m3d_rpn_precompute_targets): no cls / prob, so no score, no accuracy count; labels, gt index and target bits as without
template <bool PRE>
__global__ __launch_bounds__(RPN_TPB) void rpn_assign_kernel(RpnAssignArgs A, RpnConf cf)
{
    __shared__ double sg[M3D_RPN_MAX_GT][5];
    __shared__ int sc[4];
    const int b = blockIdx.y;
    int nv, ni;
    if (threadIdx.x < 4) sc[threadIdx.x] = 0;
    rpn_load_gts(A.gt, A.Gmax, b, sg, nv, ni);
    const int r = blockIdx.x * RPN_TPB + threadIdx.x;
    const bool live = r < A.R;
    const size_t row = (size_t)b * A.R + (live ? r : 0);
    int label = 0, gidx = -1;
    bool is_fg = false, is_bg = false;
    float tar[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) tar[i] = 0.f;
    if (nv > 0) {
        double t[11];
        const RpnRow o = rpn_assign_row<float>(A.anchors, A.gt, A.gtmax, A.bestrow, A.Gmax, A.H, A.W, b, r, live, nv, ni, sg, cf, t);
        label = o.label; gidx = o.gidx; is_fg = o.is_fg; is_bg = o.is_bg;
#pragma unroll
        for (int i = 0; i < 11; ++i) tar[i] = rpn_norm(t[i], cf.mean[i], cf.stdv[i]);
    } else {
        is_bg = true;      // an image without a valid gt keeps label 0 everywhere (and is never sampled)
    }
    if (PRE) {
        if (blockIdx.x == 0 && threadIdx.x == 0) A.any_val[b] = nv > 0 ? 1 : 0;
        if (live) {
            A.labels[row] = (short)label;
            A.gt_index[row] = (short)gidx;
            float *o2 = A.tar_2d + row * 4, *o3 = A.tar_3d + row * 7;
#pragma unroll
            for (int i = 0; i < 4; ++i) o2[i] = tar[i];
#pragma unroll
            for (int i = 0; i < 7; ++i) o3[i] = tar[4 + i];
        }
        return;
    }
    int pred = 0;
    float score = 0.f;
    if (live) {
        const float *c = A.cls + row * A.C;
        float mx = c[0];
        for (int k = 1; k < A.C; ++k)
            if (c[k] > mx) { mx = c[k]; pred = k; }
        if (nv > 0 && label < A.C) score = A.prob[row * A.C + label];
        A.labels[row] = (short)label;
        A.gt_index[row] = (short)gidx;
        A.scores[row] = score;
        float *o = A.targets + row * 11;
#pragma unroll
        for (int i = 0; i < 11; ++i) o[i] = tar[i];
    }
    const bool cfg = live && is_fg, cbg = live && is_bg;
    const unsigned long long m0 = __ballot(cfg), m1 = __ballot(cbg), m2 = __ballot(cfg && pred == label), m3 = __ballot(cbg && pred == 0);
    if ((threadIdx.x & 63) == 0) {
        if (m0) atomicAdd(&sc[0], __popcll(m0));
        if (m1) atomicAdd(&sc[1], __popcll(m1));
        if (m2) atomicAdd(&sc[2], __popcll(m2));
        if (m3) atomicAdd(&sc[3], __popcll(m3));
    }
    __syncthreads();
    if (threadIdx.x < 4 && sc[threadIdx.x]) atomicAdd(&A.counts[b * 8 + threadIdx.x], sc[threadIdx.x]);
}

// ---- launch 3, reducing form + its finish launch (m3d_rpn_target_stats) ----------------------------------------------------
// compute_bbox_stats (lib/rpn_util.py:732-889) needs, per image, the count of the fg rows and the sums of their raw transforms
// -- not the rows.  Same decisions as launch 3 on float64 rois; the transform is rounded to float32 (the reference's
// `transforms` array), then (t32 - center) and its square are taken and added in float64: a thread's one row, the lane butterfly,
// the waves in order -> one partial block per workgroup; the finish launch adds an image's blocks strided, then a tree.  No
// atomics: an image's sums depend on nothing but its own table, R and the launch shape that R fixes.
#define RPN_NS M3D_RPN_TARGET_STATS_COLS          // n_fg, 11 sums, 11 sums of squares
struct RpnStatsArgs {
    const double *anchors, *gt, *center;
    const unsigned long long *gtmax;
    const unsigned *bestrow;
    double *partials;          // [B][gridDim.x][RPN_NS]
    int Gmax, R, H, W;
};

__global__ __launch_bounds__(RPN_TPB) void rpn_stats_kernel(RpnStatsArgs A, RpnConf cf)
{
    __shared__ double sg[M3D_RPN_MAX_GT][5];
    __shared__ double sw[RPN_TPB / 64][RPN_NS];
    const int b = blockIdx.y;
    int nv, ni;
    rpn_load_gts(A.gt, A.Gmax, b, sg, nv, ni);
    const int r = blockIdx.x * RPN_TPB + threadIdx.x;
    const bool live = r < A.R;
    bool is_fg = false;
    double q[RPN_NS];
#pragma unroll
    for (int k = 0; k < RPN_NS; ++k) q[k] = 0.0;
    if (nv > 0) {
        double t[11];
        const RpnRow o = rpn_assign_row<double>(A.anchors, A.gt, A.gtmax, A.bestrow, A.Gmax, A.H, A.W, b, r, live, nv, ni, sg, cf, t);
        is_fg = live && o.is_fg;
        if (is_fg) {
            q[0] = 1.0;
#pragma unroll
            for (int i = 0; i < 11; ++i) {
                const float t32 = (float)t[i];
                const double d = (double)t32 - A.center[i];
                q[1 + i] = d;
                q[12 + i] = d * d;
            }
        }
    }
    const bool any = __ballot(is_fg) != 0ull;          // most waves hold no fg row: their sums are 0 without the butterfly
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < RPN_NS; ++k) {
        const double v = any ? wave_sum_f64(q[k]) : 0.0;
        if ((threadIdx.x & 63) == 0) sw[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < RPN_NS) {
        double v = sw[0][threadIdx.x];
        for (int w = 1; w < RPN_TPB / 64; ++w) v += sw[w][threadIdx.x];
        A.partials[((size_t)b * gridDim.x + blockIdx.x) * RPN_NS + threadIdx.x] = v;
    }
}

#define RPN_SFIN_L 32          // thread (l, k): quantity k of the workgroups l, l + 32, ...; then a tree over l
__global__ __launch_bounds__(RPN_SFIN_L * 32) void rpn_stats_finish_kernel(const double *__restrict__ partials, int nwg, double *__restrict__ out)
{
    __shared__ double red[RPN_SFIN_L][RPN_NS];
    const int k = threadIdx.x & 31, l = threadIdx.x >> 5, b = blockIdx.x;
    const bool on = k < RPN_NS;
    if (on) {
        const double *p = partials + (size_t)b * nwg * RPN_NS;
        double v = 0.0;
        for (int j = l; j < nwg; j += RPN_SFIN_L) v += p[(size_t)j * RPN_NS + k];
        red[l][k] = v;
    }
    __syncthreads();
    for (int s = RPN_SFIN_L / 2; s > 0; s >>= 1) {
        if (on && l < s) red[l][k] += red[l + s][k];
        __syncthreads();
    }
    if (on && l == 0) out[(size_t)b * RPN_NS + k] = red[0][k];
}

// ---- ingest (RPN_3D_loss_smp) ---------------------------------------------------------------------------------------------
struct RpnIngestArgs {
    const void *labels_in;       // [B, R] int64 (the data loader's collated labels) or int16 (launch 3's)
    const float *tar_2d, *tar_3d, *cls, *prob;
    const int *any_val;
    short *labels;
    float *targets, *scores;
    int *counts;
    int R, C;
};

template <typename T> struct RpnLabelPair;
template <> struct RpnLabelPair<long long> { typedef longlong2 type; };     // one 16-byte load
template <> struct RpnLabelPair<short> { typedef short2 type; };            // one 4-byte load

// Two consecutive rows per thread.  A label outside {0, 1 .. C-1, 3000} is counted and treated as ignored.  The score follows
// launch 3: prob[label] where the image has a valid gt and the row is not ignored, else 0.  The counts are launch 3's (every
// image, with or without a valid gt, enters the accuracy stats), integer atomics only.
template <typename T, bool VEC>
__global__ __launch_bounds__(RPN_TPB) void rpn_ingest_kernel(RpnIngestArgs A)
{
    __shared__ int sc[5];
    const int b = blockIdx.y;
    if (threadIdx.x < 5) sc[threadIdx.x] = 0;
    __syncthreads();
    const int r0 = (blockIdx.x * RPN_TPB + threadIdx.x) * 2;
    const T *lin = (const T *)A.labels_in + (size_t)b * A.R;
    const bool has_gt = A.any_val[b] != 0;
    const bool live[2] = {r0 < A.R, r0 + 1 < A.R};
    long long lv[2] = {0, 0};
    if (VEC) {
        if (live[1]) {
            const typename RpnLabelPair<T>::type p = *reinterpret_cast<const typename RpnLabelPair<T>::type *>(lin + r0);
            lv[0] = (long long)p.x;
            lv[1] = (long long)p.y;
        }
    } else {
        if (live[0]) lv[0] = (long long)lin[r0];
        if (live[1]) lv[1] = (long long)lin[r0 + 1];
    }
    bool f_fg[2], f_bg[2], f_okfg[2], f_okbg[2], f_bad[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const bool ok = lv[u] == 0 || (lv[u] > 0 && lv[u] < (long long)A.C) || lv[u] == RPN_IGN_LABEL;
        const int label = ok ? (int)lv[u] : RPN_IGN_LABEL;
        const bool is_fg = label > 0 && label != RPN_IGN_LABEL, is_bg = label == 0;
        int pred = 0;
        if (live[u]) {
            const size_t row = (size_t)b * A.R + r0 + u;
            const float *c = A.cls + row * A.C;
            float mx = c[0];
            for (int k = 1; k < A.C; ++k)
                if (c[k] > mx) { mx = c[k]; pred = k; }
            float score = 0.f;
            if (has_gt && label < A.C) score = A.prob[row * A.C + label];
            A.labels[row] = (short)label;
            A.scores[row] = score;
        }
        f_fg[u] = live[u] && is_fg;
        f_bg[u] = live[u] && is_bg;
        f_okfg[u] = f_fg[u] && pred == label;
        f_okbg[u] = f_bg[u] && pred == 0;
        f_bad[u] = live[u] && !ok;
    }
    // the packed targets of this workgroup's rows: consecutive threads write consecutive floats
    {
        const int base = blockIdx.x * RPN_TPB * 2, nrows = min(RPN_TPB * 2, A.R - base);
        const size_t row0 = (size_t)b * A.R + base;
        const float *i2 = A.tar_2d + row0 * 4, *i3 = A.tar_3d + row0 * 7;
        float *o = A.targets + row0 * 11;
        for (int e = threadIdx.x; e < nrows * 11; e += RPN_TPB) {
            const int rr = e / 11, c = e - rr * 11;
            o[e] = c < 4 ? i2[rr * 4 + c] : i3[rr * 7 + (c - 4)];
        }
    }
    int n[5];
    n[0] = __popcll(__ballot(f_fg[0])) + __popcll(__ballot(f_fg[1]));
    n[1] = __popcll(__ballot(f_bg[0])) + __popcll(__ballot(f_bg[1]));
    n[2] = __popcll(__ballot(f_okfg[0])) + __popcll(__ballot(f_okfg[1]));
    n[3] = __popcll(__ballot(f_okbg[0])) + __popcll(__ballot(f_okbg[1]));
    n[4] = __popcll(__ballot(f_bad[0])) + __popcll(__ballot(f_bad[1]));
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (n[k]) atomicAdd(&sc[k], n[k]);
    }
    __syncthreads();
    if (threadIdx.x < 5 && sc[threadIdx.x]) atomicAdd(&A.counts[b * 8 + threadIdx.x], sc[threadIdx.x]);
}

// ---- launch 4 ----------------------------------------------------------------------------------------------------------
// kind 0: fg (0 < label < IGN), kind 1: bg (label == 0)
__device__ __forceinline__ bool rpn_kind_match(int label, int kind) { return kind == 0 ? (label > 0 && label != RPN_IGN_LABEL) : label == 0; }

__device__ __forceinline__ void rpn_hist_add(unsigned *hist, bool cand, unsigned digit)
{
    // a wave whose candidates all fall into one bin (the sign / exponent digits of probabilities) adds once
    const unsigned long long m = __ballot(cand);
    if (m == 0ull) return;
    const int first = __ffsll((long long)m) - 1;
    const unsigned d0 = (unsigned)__shfl((int)digit, first, 64);
    const unsigned long long same = __ballot(cand && digit == d0);
    if (same == m) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[d0], (unsigned)__popcll(m));
    } else if (cand) {
        atomicAdd(&hist[digit], 1u);
    }
}

// one pass of the radix select: histogram of digit `shift` over the candidates, then the bin holding rank k (1-based).
// Returns the digit; k becomes the rank inside the bin, n_bin the bin's population.  VEC: four rows per thread and iteration
// from one 8-byte and one 16-byte load (R % 4 == 0 and aligned bases): the loop is bound by load latency, not by bytes.
template <bool VEC, typename KeyFn>
__device__ __forceinline__ unsigned rpn_select_pass(unsigned *hist, unsigned *bc, const short *__restrict__ lb, const float *__restrict__ sc,
                                                    int R, int shift, unsigned &k, unsigned &n_bin, KeyFn key)
{
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    if (VEC) {
        for (int r0 = 0; r0 < R; r0 += blockDim.x * 4) {
            const int r = r0 + threadIdx.x * 4;
            const bool in = r < R;
            short l4[4] = {0, 0, 0, 0};
            float s4[4] = {0.f, 0.f, 0.f, 0.f};
            if (in) {
                const uint2 lv = *reinterpret_cast<const uint2 *>(lb + r);
                const float4 sv = *reinterpret_cast<const float4 *>(sc + r);
                l4[0] = (short)(lv.x & 0xffffu); l4[1] = (short)(lv.x >> 16); l4[2] = (short)(lv.y & 0xffffu); l4[3] = (short)(lv.y >> 16);
                s4[0] = sv.x; s4[1] = sv.y; s4[2] = sv.z; s4[3] = sv.w;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                unsigned kv = 0;
                const bool cand = in && key(l4[u], s4[u], r + u, kv);
                rpn_hist_add(hist, cand, (kv >> shift) & 255u);
            }
        }
    } else {
        for (int r0 = 0; r0 < R; r0 += blockDim.x) {
            const int r = r0 + threadIdx.x;
            unsigned kv = 0;
            const bool cand = r < R && key(lb[r], sc[r], r, kv);
            rpn_hist_add(hist, cand, (kv >> shift) & 255u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned cum = 0, d = 0;
        for (; d < 255; ++d) {
            if (cum + hist[d] >= k) break;
            cum += hist[d];
        }
        bc[0] = d; bc[1] = k - cum; bc[2] = hist[d];
    }
    __syncthreads();
    const unsigned d = bc[0];
    k = bc[1];
    n_bin = bc[2];
    __syncthreads();
    return d;
}

template <bool VEC>
__global__ __launch_bounds__(RPN_SEL_TPB) void rpn_select_kernel(const short *__restrict__ labels, const float *__restrict__ scores,
                                                                 const double *__restrict__ gt, int Gmax, const int *__restrict__ any_val,
                                                                 const int *__restrict__ counts, unsigned *__restrict__ sel, int R,
                                                                 RpnConf cf)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned bc[4];
    const int kind = blockIdx.x, b = blockIdx.y;
    const short *lb = labels + (size_t)b * R;
    const float *sc = scores + (size_t)b * R;
    unsigned *out = sel + (b * 2 + kind) * 8;
    // whether the image has a valid gt: from its table, or (pre-computed targets: no table) from the loader's any_val
    const int nv = gt ? (int)gt[(size_t)b * (Gmax + 1) * M3D_RPN_GT_COLS] : any_val[b];
    const int n_fg = counts[b * 8 + 0], n_bg = counts[b * 8 + 1];
    long long fg_num, bg_num;
    if (isinf(cf.box_samples)) {
        fg_num = n_fg;
        bg_num = n_bg;
    } else {
        const double want = (double)R * cf.box_samples;
        fg_num = min((long long)rint(want * cf.fg_fraction), (long long)n_fg);         // Python round(): half to even, like rint
        bg_num = min((long long)rint(want - (double)fg_num), (long long)n_bg);
    }
    if (nv <= 0) fg_num = bg_num = 0;
    const unsigned avail = (unsigned)(kind == 0 ? n_fg : n_bg);
    unsigned k = (unsigned)max(0ll, kind == 0 ? fg_num : bg_num);
    unsigned mode, tkey = 0, trow = 0xffffffffu;
    if (k == 0) {
        mode = 0;
    } else if (k >= avail) {
        mode = 1;
        k = avail;
    } else {
        mode = 2;
        unsigned prefix = 0, n_bin = 0, krem = k;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
            const unsigned d = rpn_select_pass<VEC>(hist, bc, lb, sc, R, shift, krem, n_bin, [&](int label, float score, int r, unsigned &kv) {
                kv = f32_sortable(score);
                return rpn_kind_match(label, kind) && (kv & himask) == prefix;
            });
            prefix |= d << shift;
        }
        tkey = prefix;
        if (krem < n_bin) {        // the threshold score is shared: the lowest rows among its holders
            unsigned rp = 0;
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
                const unsigned d = rpn_select_pass<VEC>(hist, bc, lb, sc, R, shift, krem, n_bin, [&](int label, float score, int r, unsigned &kv) {
                    kv = (unsigned)r;
                    return rpn_kind_match(label, kind) && f32_sortable(score) == tkey && (kv & himask) == rp;
                });
                rp |= d << shift;
            }
            trow = rp;
        }
    }
    // sampled anchors whose score is exactly 1: (1 - score)^focal is 0, the reference drops them from the mean's count
    unsigned n_one = 0;
    if (cf.focal > 0 && mode != 0) {
        if (threadIdx.x == 0) bc[3] = 0;
        __syncthreads();
        const unsigned one = f32_sortable(1.0f);
        for (int r0 = 0; r0 < R; r0 += blockDim.x) {
            const int r = r0 + threadIdx.x;
            bool hit = false;
            if (r < R && rpn_kind_match(lb[r], kind)) {
                const unsigned kv = f32_sortable(sc[r]);
                const bool in = mode == 1 || kv < tkey || (kv == tkey && (unsigned)r <= trow);
                hit = in && kv == one;
            }
            const unsigned long long m = __ballot(hit);
            if (m && (threadIdx.x & 63) == 0) atomicAdd(&bc[3], (unsigned)__popcll(m));
        }
        __syncthreads();
        n_one = bc[3];
    }
    if (threadIdx.x == 0) {
        out[0] = mode; out[1] = tkey; out[2] = trow; out[3] = k; out[4] = n_one; out[5] = out[6] = out[7] = 0;
    }
}

// ---- launch 5 ----------------------------------------------------------------------------------------------------------
struct RpnLossArgs {
    const double *anchors;
    const float *cls, *bbox_2d, *bbox_3d;
    const short *labels;
    const float *targets, *scores;
    const unsigned *sel;
    unsigned char *sampled;
    float *g_cls, *g_2d, *g_3d;
    double *partials;
    int B, R, H, W, C;
};

struct RpnTotals {
    double fg_num, bg_num, n_active, fg_weight;
};

__device__ __forceinline__ RpnTotals rpn_totals(const unsigned *sel, int B, const RpnConf &cf)
{
    long long fg = 0, bg = 0, fg1 = 0, bg1 = 0;
    for (int b = 0; b < B; ++b) {
        fg += sel[(b * 2 + 0) * 8 + 3]; fg1 += sel[(b * 2 + 0) * 8 + 4];
        bg += sel[(b * 2 + 1) * 8 + 3]; bg1 += sel[(b * 2 + 1) * 8 + 4];
    }
    RpnTotals t;
    t.fg_num = (double)fg;
    t.bg_num = (double)bg;
    t.fg_weight = 1.0;
    if (!isnan(cf.fg_fraction) && fg > 0) t.fg_weight = (cf.fg_fraction / (1.0 - cf.fg_fraction)) * ((double)bg / (double)fg);
    t.n_active = (double)(bg - bg1) + (t.fg_weight > 0.0 ? (double)(fg - fg1) : 0.0);
    return t;
}

__device__ __forceinline__ double smooth_l1(double d, double &g)
{
    const double a = fabs(d);
    if (a < 1.0) { g = d; return 0.5 * d * d; }
    g = d > 0 ? 1.0 : -1.0;
    return a - 0.5;
}

// d min(a, b) / da and d max(a, b) / da the way autograd splits a tie
__device__ __forceinline__ double dmin_da(double a, double b) { return a < b ? 1.0 : (a == b ? 0.5 : 0.0); }
__device__ __forceinline__ double dmax_da(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }

__global__ __launch_bounds__(RPN_TPB) void rpn_loss_kernel(RpnLossArgs A, RpnConf cf)
{
    __shared__ RpnTotals st;
    __shared__ double sw[RPN_TPB / 64][RPN_NQ];
    if (threadIdx.x == 0) st = rpn_totals(A.sel, A.B, cf);
    __syncthreads();
    const RpnTotals T = st;
    const long long total = (long long)A.B * A.R;
    double acc[RPN_NQ];          // this thread's rows, in row order
#pragma unroll
    for (int k = 0; k < RPN_NQ; ++k) acc[k] = 0.0;
    for (long long i = (long long)blockIdx.x * RPN_TPB + threadIdx.x; i < total; i += (long long)gridDim.x * RPN_TPB) {
    const bool live = true;
    double q[RPN_NQ];
#pragma unroll
    for (int k = 0; k < RPN_NQ; ++k) q[k] = 0.0;
    int smp = 0;          // 0 not sampled, 1 fg, 2 bg
    int label = 0;
    int b = 0, r = 0;
    float score = 0.f;
    if (live) {
        b = (int)(i / A.R);
        r = (int)(i - (long long)b * A.R);
        label = A.labels[i];
        if (label != RPN_IGN_LABEL && label >= 0 && label < A.C) {
            const int kind = label > 0 ? 0 : 1;
            const unsigned *s = A.sel + (b * 2 + kind) * 8;
            const unsigned mode = s[0];
            score = A.scores[i];
            const unsigned kv = f32_sortable(score);
            if (mode == 1 || (mode == 2 && (kv < s[1] || (kv == s[1] && (unsigned)r <= s[2])))) smp = kind + 1;
        }
    }
    const int C = A.C;
    if (smp) {
        // ---- classification: weight * (logsumexp - logit[label]), clamped to [0, 2000] with zero gradient where clamped
        double w = smp == 1 ? T.fg_weight : 1.0;
        if (cf.focal > 0) w *= pow(1.0 - (double)score, cf.focal);
        const float *c = A.cls + i * C;
        float *gc = A.g_cls + i * C;
        if (cf.lam_cls != 0.0 && w > 0.0 && T.n_active > 0.0) {
            double mx = c[0];
            for (int k = 1; k < C; ++k) mx = fmax(mx, (double)c[k]);
            double se = 0.0;
            for (int k = 0; k < C; ++k) se += exp((double)c[k] - mx);
            const double lse = mx + log(se);
            const double v = w * (lse - (double)c[label]);
            const bool clamped = v > 2000.0;
            q[0] = clamped ? 2000.0 : v;
            const double gs = clamped ? 0.0 : cf.lam_cls * w / T.n_active;
            for (int k = 0; k < C; ++k) gc[k] = (float)(gs * (exp((double)c[k] - lse) - (k == label ? 1.0 : 0.0)));
        } else {
            for (int k = 0; k < C; ++k) gc[k] = 0.f;
        }
    } else if (live) {
        float *gc = A.g_cls + i * C;
        for (int k = 0; k < C; ++k) gc[k] = 0.f;
    }
    if (smp == 1) {
        const float *tr = A.targets + i * 11;
        const float *p2 = A.bbox_2d + i * 4, *p3 = A.bbox_3d + i * 7;
        const double inv_fg = 1.0 / T.fg_num;
        double g2[4] = {0.0, 0.0, 0.0, 0.0};
        if (cf.lam_2d != 0.0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double g;
                q[1 + k] = smooth_l1((double)p2[k] - (double)tr[k], g);
                g2[k] = cf.lam_2d * inv_fg * g;
            }
        }
        float *o3 = A.g_3d + i * 7;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            double g = 0.0;
            if (cf.lam_3d != 0.0) q[5 + k] = smooth_l1((double)p3[k] - (double)tr[4 + k], g);
            o3[k] = (float)(cf.lam_3d * inv_fg * g);
        }
        // ---- z / ry in absolute units (the anchor's own z / ry cancels in exact arithmetic; kept as the reference has it)
        RpnRoi roi = rpn_roi<float>(A.anchors, r, A.H, A.W, cf.stride);
        const double *an = A.anchors + roi.a * 9;
        const double zt = an[4] + ((double)tr[6] * cf.stdv[6] + cf.mean[6]), zp = an[4] + ((double)p3[2] * cf.stdv[6] + cf.mean[6]);
        const double rt = an[8] + ((double)tr[10] * cf.stdv[10] + cf.mean[10]), rp = an[8] + ((double)p3[6] * cf.stdv[10] + cf.mean[10]);
        q[12] = fabs(zt - zp);
        q[13] = fabs(rt - rp);
        // ---- IoU of the decoded predicted box with the box decoded from the normalised target (bbox_transform_inv, iou 'list')
        const double rw = (double)roi.x2 - (double)roi.x1 + 1.0, rh = (double)roi.y2 - (double)roi.y1 + 1.0;
        const double cx = (double)roi.x1 + 0.5 * rw, cy = (double)roi.y1 + 0.5 * rh;
        double pb[4], tb[4], pw, ph;
        {
            const double dx = (double)p2[0] * cf.stdv[0] + cf.mean[0], dy = (double)p2[1] * cf.stdv[1] + cf.mean[1];
            const double dw = (double)p2[2] * cf.stdv[2] + cf.mean[2], dh = (double)p2[3] * cf.stdv[3] + cf.mean[3];
            const double pcx = dx * rw + cx, pcy = dy * rh + cy;
            pw = exp(dw) * rw; ph = exp(dh) * rh;
            pb[0] = pcx - 0.5 * pw; pb[1] = pcy - 0.5 * ph; pb[2] = pcx + 0.5 * pw; pb[3] = pcy + 0.5 * ph;
        }
        {
            const double dx = (double)tr[0] * cf.stdv[0] + cf.mean[0], dy = (double)tr[1] * cf.stdv[1] + cf.mean[1];
            const double dw = (double)tr[2] * cf.stdv[2] + cf.mean[2], dh = (double)tr[3] * cf.stdv[3] + cf.mean[3];
            const double tcx = dx * rw + cx, tcy = dy * rh + cy;
            const double tw = exp(dw) * rw, th = exp(dh) * rh;
            tb[0] = tcx - 0.5 * tw; tb[1] = tcy - 0.5 * th; tb[2] = tcx + 0.5 * tw; tb[3] = tcy + 0.5 * th;
        }
        const double iw_raw = fmin(pb[2], tb[2]) - fmax(pb[0], tb[0]), ih_raw = fmin(pb[3], tb[3]) - fmax(pb[1], tb[1]);
        const double iw = fmax(iw_raw, 0.0), ih = fmax(ih_raw, 0.0);
        const double inter = iw * ih;
        const double pwd = pb[2] - pb[0], phd = pb[3] - pb[1];
        const double area_p = pwd * phd, area_t = (tb[2] - tb[0]) * (tb[3] - tb[1]);
        const double den = (area_p + area_t - inter) + 1e-8;
        const double iou = inter / den;
        q[14] = iou;
        if (cf.lam_iou != 0.0) {
            q[15] = -log(iou);            // +inf for disjoint boxes, as in the reference
            if (inter > 0.0) {
                // dL/d(inter) and dL/d(area_p) of L = -log(inter / (area_p + area_t - inter + eps)) * lambda / n_fg
                const double s = cf.lam_iou * inv_fg;
                const double dl_diou = -s / iou;
                const double diou_dinter = 1.0 / den + inter / (den * den), diou_darea = -inter / (den * den);
                const double gi = dl_diou * diou_dinter, ga = dl_diou * diou_darea;
                const double giw = iw_raw >= 0.0 ? gi * ih : 0.0, gih = ih_raw >= 0.0 ? gi * iw : 0.0;
                const double gx1 = -giw * dmax_da(pb[0], tb[0]) - ga * phd, gx2 = giw * dmin_da(pb[2], tb[2]) + ga * phd;
                const double gy1 = -gih * dmax_da(pb[1], tb[1]) - ga * pwd, gy2 = gih * dmin_da(pb[3], tb[3]) + ga * pwd;
                const double gcx = gx1 + gx2, gcy = gy1 + gy2, gpw = 0.5 * (gx2 - gx1), gph = 0.5 * (gy2 - gy1);
                g2[0] += cf.stdv[0] * rw * gcx;
                g2[1] += cf.stdv[1] * rh * gcy;
                g2[2] += cf.stdv[2] * pw * gpw;
                g2[3] += cf.stdv[3] * ph * gph;
            }
        }
        float *o2 = A.g_2d + i * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) o2[k] = (float)g2[k];
    } else if (live) {
        float *o2 = A.g_2d + i * 4, *o3 = A.g_3d + i * 7;
#pragma unroll
        for (int k = 0; k < 4; ++k) o2[k] = 0.f;
#pragma unroll
        for (int k = 0; k < 7; ++k) o3[k] = 0.f;
    }
    if (live) A.sampled[i] = (unsigned char)smp;
    if (smp) {
#pragma unroll
        for (int k = 0; k < RPN_NQ; ++k) acc[k] += q[k];
    }
    }
    // ---- partial sums: lanes (butterfly), then the waves in order
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < RPN_NQ; ++k) {
        const double v = wave_sum_f64(acc[k]);
        if ((threadIdx.x & 63) == 0) sw[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < RPN_NQ) {
        double v = sw[0][threadIdx.x];
        for (int w = 1; w < RPN_TPB / 64; ++w) v += sw[w][threadIdx.x];
        A.partials[(size_t)blockIdx.x * RPN_NQ + threadIdx.x] = v;
    }
}

// ---- launch 6 ----------------------------------------------------------------------------------------------------------
#define RPN_FIN_TPB 1024
__global__ __launch_bounds__(RPN_FIN_TPB) void rpn_finish_kernel(const double *__restrict__ partials, int nblk, const unsigned *__restrict__ sel,
                                                                 const int *__restrict__ counts, int B, RpnConf cf, float *__restrict__ loss_out,
                                                                 double *__restrict__ stats, int smp)
{
    // thread (l, k) adds the partials of quantity k of the workgroups l, l + 64, ...; then a tree over l: fixed order
    __shared__ double red[RPN_FIN_TPB / RPN_NQ][RPN_NQ];
    const int k0 = threadIdx.x % RPN_NQ, l = threadIdx.x / RPN_NQ;
    double v = 0.0;
    for (int j = l; j < nblk; j += RPN_FIN_TPB / RPN_NQ) v += partials[(size_t)j * RPN_NQ + k0];
    red[l][k0] = v;
    __syncthreads();
    for (int s = RPN_FIN_TPB / RPN_NQ / 2; s > 0; s >>= 1) {
        if (l < s) red[l][k0] += red[l + s][k0];
        __syncthreads();
    }
    const double *tot = red[0];
    if (threadIdx.x != 0) return;
    const RpnTotals T = rpn_totals(sel, B, cf);
    long long n_fg = 0, n_bg = 0, ok_fg = 0, ok_bg = 0;
    for (int b = 0; b < B; ++b) {
        n_fg += counts[b * 8 + 0]; n_bg += counts[b * 8 + 1]; ok_fg += counts[b * 8 + 2]; ok_bg += counts[b * 8 + 3];
    }
    double s[M3D_RPN_STAT_COUNT];
    for (int k = 0; k < M3D_RPN_STAT_COUNT; ++k) s[k] = 0.0;
    double loss = 0.0;
    const bool has_cls = cf.lam_cls != 0.0 && T.n_active > 0.0, has_box = T.fg_num > 0.0;
    if (has_cls) { s[M3D_RPN_STAT_CLS] = cf.lam_cls * (tot[0] / T.n_active); loss += s[M3D_RPN_STAT_CLS]; }
    if (has_box) {
        if (cf.lam_2d != 0.0) {
            s[M3D_RPN_STAT_BBOX_2D] = cf.lam_2d * (tot[1] / T.fg_num + tot[2] / T.fg_num + tot[3] / T.fg_num + tot[4] / T.fg_num);
            loss += s[M3D_RPN_STAT_BBOX_2D];
        }
        if (cf.lam_3d != 0.0) {
            s[M3D_RPN_STAT_BBOX_3D] = cf.lam_3d * ((tot[5] / T.fg_num + tot[6] / T.fg_num + tot[7] / T.fg_num) +
                                                   (tot[8] / T.fg_num + tot[9] / T.fg_num + tot[10] / T.fg_num + tot[11] / T.fg_num));
            loss += s[M3D_RPN_STAT_BBOX_3D];
        }
        s[M3D_RPN_STAT_Z] = tot[12] / T.fg_num;
        s[M3D_RPN_STAT_RY] = tot[13] / T.fg_num;
        s[M3D_RPN_STAT_IOU_ACC] = tot[14] / T.fg_num;
        if (cf.lam_iou != 0.0) { s[M3D_RPN_STAT_IOU_LOSS] = cf.lam_iou * (tot[15] / T.fg_num); loss += s[M3D_RPN_STAT_IOU_LOSS]; }
    }
    s[M3D_RPN_STAT_LOSS] = loss;
    s[M3D_RPN_STAT_ACC_FG] = n_fg > 0 ? (double)ok_fg / (double)n_fg : 0.0;
    s[M3D_RPN_STAT_ACC_BG] = n_bg > 0 ? (double)ok_bg / (double)n_bg : 0.0;
    s[M3D_RPN_STAT_N_FG] = (double)n_fg;
    s[M3D_RPN_STAT_N_BG] = (double)n_bg;
    s[M3D_RPN_STAT_FG_NUM] = T.fg_num;
    s[M3D_RPN_STAT_BG_NUM] = T.bg_num;
    s[M3D_RPN_STAT_N_ACTIVE] = T.n_active;
    s[M3D_RPN_STAT_FG_WEIGHT] = T.fg_weight;
    for (int k = 0; k < M3D_RPN_STAT_COUNT; ++k) stats[k] = s[k];
    if (smp) {
        long long bad = 0;
        for (int b = 0; b < B; ++b) bad += counts[b * 8 + 4];
        stats[M3D_RPN_SMP_STAT_BAD_LABELS] = (double)bad;
    }
    loss_out[0] = (float)loss;
}

// ---- entry points ------------------------------------------------------------------------------------------------------
static int rpn_check_shape(const char *who, int A, int H, int W, int B, int C, int Gmax, long long *R)
{
    M3D_REQUIRE(A > 0 && H > 0 && W > 0 && B > 0, "%s: anchors (%d), feat_size (%d x %d) and batch (%d) must be positive", who, A, H, W, B);
    M3D_REQUIRE(B <= 4096, "%s: at most 4096 images per call (got %d)", who, B);
    M3D_REQUIRE(C >= 2 && C <= 64, "%s: 2..64 classes including background (got %d)", who, C);
    *R = (long long)A * H * W;
    M3D_REQUIRE(*R * B * 11 < (1ll << 31), "%s: %d x %lld anchor rows exceed the 32-bit index range of this build", who, B, *R);
    M3D_REQUIRE(Gmax >= 0, "%s: negative gt table size", who);
    M3D_REQUIRE(Gmax <= M3D_RPN_MAX_GT,
                "%s: %d ground truths (valid + ignore) in one image exceed the kernel's cap M3D_RPN_MAX_GT = %d; nothing is truncated", who,
                Gmax, M3D_RPN_MAX_GT);
    return M3D_OK;
}

extern "C" long long m3d_rpn_loss_workspace_bytes(int B, long long R)
{
    if (B <= 0 || R <= 0) return -1;
    return rpn_ws_layout(nullptr, B, R).total;
}

extern "C" int m3d_rpn_targets(const double *anchors, int A, int H, int W, const double *conf, int n_conf, const double *gt_table, int B,
                               int Gmax, const float *cls, const float *prob, int C, short *labels, short *gt_index, float *targets,
                               float *scores, void *workspace, long long workspace_bytes, m3d_stream_t stream)
{
    long long R;
    RpnConf cf;
    int st = rpn_check_shape("rpn_targets", A, H, W, B, C, Gmax, &R);
    if (st) return st;
    if ((st = rpn_conf_from(conf, n_conf, &cf, "rpn_targets"))) return st;
    M3D_REQUIRE(anchors && gt_table && cls && prob && labels && gt_index && targets && scores && workspace, "rpn_targets: NULL pointer");
    const RpnWs ws = rpn_ws_layout(workspace, B, R);
    if (workspace_bytes < ws.total) {
        m3d_set_error("rpn_targets: workspace %lld < %lld bytes (m3d_rpn_loss_workspace_bytes)", workspace_bytes, ws.total);
        return M3D_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    M3D_HIP(hipMemsetAsync(ws.gtmax, 0, (size_t)B * M3D_RPN_MAX_GT * 8, s));
    M3D_HIP(hipMemsetAsync(ws.bestrow, 0xff, (size_t)B * M3D_RPN_MAX_GT * 4, s));
    M3D_HIP(hipMemsetAsync(ws.counts, 0, (size_t)B * 8 * 4, s));
    const dim3 grid(cdiv(R, RPN_TPB), B);
    hipLaunchKernelGGL(rpn_gt_max_kernel<float>, dim3(cdiv(R, RPN_TPB * RPN_MAX_ROWS), B), dim3(RPN_TPB), 0, s, anchors, gt_table, Gmax, (int)R, H, W, cf.stride, ws.gtmax);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(rpn_gt_row_kernel<float>, grid, dim3(RPN_TPB), 0, s, anchors, gt_table, Gmax, (int)R, H, W, cf.stride, ws.gtmax, ws.bestrow);
    M3D_LAUNCH_CHECK();
    RpnAssignArgs a;
    a.anchors = anchors; a.gt = gt_table; a.cls = cls; a.prob = prob; a.gtmax = ws.gtmax; a.bestrow = ws.bestrow;
    a.labels = labels; a.gt_index = gt_index; a.targets = targets; a.scores = scores; a.counts = ws.counts;
    a.Gmax = Gmax; a.R = (int)R; a.H = H; a.W = W; a.C = C; a.tar_2d = a.tar_3d = nullptr; a.any_val = nullptr;
    hipLaunchKernelGGL(rpn_assign_kernel<false>, grid, dim3(RPN_TPB), 0, s, a, cf);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

// launches 4-6 behind m3d_rpn_loss (gt_table) and m3d_rpn_loss_smp (any_val, one more stat slot)
static int rpn_launch_loss(const char *who, const double *anchors, int H, int W, const RpnConf &cf, const double *gt_table, int Gmax,
                           const int *any_val, int B, long long R, const float *cls, const float *bbox_2d, const float *bbox_3d, int C,
                           const short *labels, const float *targets, const float *scores, unsigned char *sampled, float *grad_cls,
                           float *grad_bbox_2d, float *grad_bbox_3d, float *loss, double *stats, const RpnWs &ws, hipStream_t s)
{
    if (!isinf(cf.box_samples)) {
        // with a rounded count of 0 the reference keeps EVERY candidate instead of none (its `num > 0 and ...` guards)
        const double want = (double)R * cf.box_samples, fg_cap = rint(want * cf.fg_fraction);
        M3D_REQUIRE(fg_cap >= 1 && rint(want - fg_cap) >= 1, "%s: box_samples %g x fg_fraction %g of %lld anchors rounds to no fg or no bg sample",
                    who, cf.box_samples, cf.fg_fraction, R);
    }
    if (R % 4 == 0 && (uintptr_t)labels % 8 == 0 && (uintptr_t)scores % 16 == 0)
        hipLaunchKernelGGL(rpn_select_kernel<true>, dim3(2, B), dim3(RPN_SEL_TPB), 0, s, labels, scores, gt_table, Gmax, any_val, ws.counts, ws.sel, (int)R, cf);
    else
        hipLaunchKernelGGL(rpn_select_kernel<false>, dim3(2, B), dim3(RPN_SEL_TPB), 0, s, labels, scores, gt_table, Gmax, any_val, ws.counts, ws.sel, (int)R, cf);
    M3D_LAUNCH_CHECK();
    RpnLossArgs a;
    a.anchors = anchors; a.cls = cls; a.bbox_2d = bbox_2d; a.bbox_3d = bbox_3d; a.labels = labels; a.targets = targets; a.scores = scores;
    a.sel = ws.sel; a.sampled = sampled; a.g_cls = grad_cls; a.g_2d = grad_bbox_2d; a.g_3d = grad_bbox_3d; a.partials = ws.partials;
    a.B = B; a.R = (int)R; a.H = H; a.W = W; a.C = C;
    const int nblk = imin(cdiv((long long)B * R, RPN_TPB), RPN_LOSS_MAX_WG);
    hipLaunchKernelGGL(rpn_loss_kernel, dim3(nblk), dim3(RPN_TPB), 0, s, a, cf);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(rpn_finish_kernel, dim3(1), dim3(RPN_FIN_TPB), 0, s, ws.partials, nblk, ws.sel, ws.counts, B, cf, loss, stats, gt_table ? 0 : 1);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

extern "C" int m3d_rpn_loss(const double *anchors, int A, int H, int W, const double *conf, int n_conf, const double *gt_table, int B,
                            int Gmax, const float *cls, const float *bbox_2d, const float *bbox_3d, int C, const short *labels,
                            const float *targets, const float *scores, unsigned char *sampled, float *grad_cls, float *grad_bbox_2d,
                            float *grad_bbox_3d, float *loss, double *stats, void *workspace, long long workspace_bytes,
                            m3d_stream_t stream)
{
    long long R;
    RpnConf cf;
    int st = rpn_check_shape("rpn_loss", A, H, W, B, C, Gmax, &R);
    if (st) return st;
    if ((st = rpn_conf_from(conf, n_conf, &cf, "rpn_loss"))) return st;
    M3D_REQUIRE(anchors && gt_table && cls && bbox_2d && bbox_3d && labels && targets && scores && sampled && grad_cls && grad_bbox_2d &&
                    grad_bbox_3d && loss && stats && workspace,
                "rpn_loss: NULL pointer");
    const RpnWs ws = rpn_ws_layout(workspace, B, R);
    if (workspace_bytes < ws.total) {
        m3d_set_error("rpn_loss: workspace %lld < %lld bytes (m3d_rpn_loss_workspace_bytes)", workspace_bytes, ws.total);
        return M3D_E_WORKSPACE;
    }
    return rpn_launch_loss("rpn_loss", anchors, H, W, cf, gt_table, Gmax, nullptr, B, R, cls, bbox_2d, bbox_3d, C, labels, targets, scores,
                           sampled, grad_cls, grad_bbox_2d, grad_bbox_3d, loss, stats, ws, (hipStream_t)stream);
}

extern "C" int m3d_rpn_precompute_targets(const double *anchors, int A, int H, int W, const double *conf, int n_conf,
                                          const double *gt_table, int B, int Gmax, short *labels, short *gt_index, float *bbox_2d_tar,
                                          float *bbox_3d_tar, int *any_val, void *workspace, long long workspace_bytes,
                                          m3d_stream_t stream)
{
    long long R;
    RpnConf cf;
    int st = rpn_check_shape("rpn_precompute_targets", A, H, W, B, 2, Gmax, &R);
    if (st) return st;
    if ((st = rpn_conf_from(conf, n_conf, &cf, "rpn_precompute_targets"))) return st;
    M3D_REQUIRE(anchors && gt_table && labels && gt_index && bbox_2d_tar && bbox_3d_tar && any_val && workspace,
                "rpn_precompute_targets: NULL pointer");
    const RpnWs ws = rpn_ws_layout(workspace, B, R);
    if (workspace_bytes < ws.total) {
        m3d_set_error("rpn_precompute_targets: workspace %lld < %lld bytes (m3d_rpn_loss_workspace_bytes)", workspace_bytes, ws.total);
        return M3D_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    M3D_HIP(hipMemsetAsync(ws.gtmax, 0, (size_t)B * M3D_RPN_MAX_GT * 8, s));
    M3D_HIP(hipMemsetAsync(ws.bestrow, 0xff, (size_t)B * M3D_RPN_MAX_GT * 4, s));
    const dim3 grid(cdiv(R, RPN_TPB), B);
    hipLaunchKernelGGL(rpn_gt_max_kernel<float>, dim3(cdiv(R, RPN_TPB * RPN_MAX_ROWS), B), dim3(RPN_TPB), 0, s, anchors, gt_table, Gmax, (int)R, H, W, cf.stride, ws.gtmax);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(rpn_gt_row_kernel<float>, grid, dim3(RPN_TPB), 0, s, anchors, gt_table, Gmax, (int)R, H, W, cf.stride, ws.gtmax, ws.bestrow);
    M3D_LAUNCH_CHECK();
    RpnAssignArgs a;
    a.anchors = anchors; a.gt = gt_table; a.cls = nullptr; a.prob = nullptr; a.gtmax = ws.gtmax; a.bestrow = ws.bestrow;
    a.labels = labels; a.gt_index = gt_index; a.targets = nullptr; a.scores = nullptr; a.counts = nullptr;
    a.Gmax = Gmax; a.R = (int)R; a.H = H; a.W = W; a.C = 0; a.tar_2d = bbox_2d_tar; a.tar_3d = bbox_3d_tar; a.any_val = any_val;
    hipLaunchKernelGGL(rpn_assign_kernel<true>, grid, dim3(RPN_TPB), 0, s, a, cf);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

extern "C" int m3d_rpn_loss_smp(const double *anchors, int A, int H, int W, const double *conf, int n_conf, int B, const void *labels_in,
                                int label_bytes, const float *bbox_2d_tar, const float *bbox_3d_tar, const int *any_val, const float *cls,
                                const float *prob, const float *bbox_2d, const float *bbox_3d, int C, short *labels, float *targets,
                                float *scores, unsigned char *sampled, float *grad_cls, float *grad_bbox_2d, float *grad_bbox_3d,
                                float *loss, double *stats, void *workspace, long long workspace_bytes, m3d_stream_t stream)
{
    long long R;
    RpnConf cf;
    int st = rpn_check_shape("rpn_loss_smp", A, H, W, B, C, 0, &R);
    if (st) return st;
    if ((st = rpn_conf_from(conf, n_conf, &cf, "rpn_loss_smp"))) return st;
    M3D_REQUIRE(label_bytes == 8 || label_bytes == 2, "rpn_loss_smp: labels are int64 (label_bytes 8) or int16 (2), got %d", label_bytes);
    M3D_REQUIRE(anchors && labels_in && bbox_2d_tar && bbox_3d_tar && any_val && cls && prob && bbox_2d && bbox_3d && labels && targets &&
                    scores && sampled && grad_cls && grad_bbox_2d && grad_bbox_3d && loss && stats && workspace,
                "rpn_loss_smp: NULL pointer");
    M3D_REQUIRE((uintptr_t)labels_in % label_bytes == 0, "rpn_loss_smp: labels are not aligned to their own size");
    M3D_REQUIRE(labels_in != (const void *)labels, "rpn_loss_smp: the int16 label output must not alias the label input");
    const RpnWs ws = rpn_ws_layout(workspace, B, R);
    if (workspace_bytes < ws.total) {
        m3d_set_error("rpn_loss_smp: workspace %lld < %lld bytes (m3d_rpn_loss_workspace_bytes)", workspace_bytes, ws.total);
        return M3D_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    M3D_HIP(hipMemsetAsync(ws.counts, 0, (size_t)B * 8 * 4, s));
    RpnIngestArgs g;
    g.labels_in = labels_in; g.tar_2d = bbox_2d_tar; g.tar_3d = bbox_3d_tar; g.any_val = any_val; g.cls = cls; g.prob = prob;
    g.labels = labels; g.targets = targets; g.scores = scores; g.counts = ws.counts; g.R = (int)R; g.C = C;
    // two labels per load: every image's first row is then aligned iff R is even
    const bool vec = R % 2 == 0 && (uintptr_t)labels_in % (2 * label_bytes) == 0;
    const dim3 grid(cdiv(R, RPN_TPB * 2), B);
    if (label_bytes == 8) {
        if (vec) hipLaunchKernelGGL((rpn_ingest_kernel<long long, true>), grid, dim3(RPN_TPB), 0, s, g);
        else hipLaunchKernelGGL((rpn_ingest_kernel<long long, false>), grid, dim3(RPN_TPB), 0, s, g);
    } else {
        if (vec) hipLaunchKernelGGL((rpn_ingest_kernel<short, true>), grid, dim3(RPN_TPB), 0, s, g);
        else hipLaunchKernelGGL((rpn_ingest_kernel<short, false>), grid, dim3(RPN_TPB), 0, s, g);
    }
    M3D_LAUNCH_CHECK();
    return rpn_launch_loss("rpn_loss_smp", anchors, H, W, cf, nullptr, 0, any_val, B, R, cls, bbox_2d, bbox_3d, C, labels, targets, scores,
                           sampled, grad_cls, grad_bbox_2d, grad_bbox_3d, loss, stats, ws, s);
}

// ---- dataset statistics (compute_bbox_stats, lib/rpn_util.py:732-889) ----------------------------------------------------------
struct RpnStatsWs {
    unsigned long long *gtmax;   // [B][M3D_RPN_MAX_GT]
    unsigned *bestrow;           // [B][M3D_RPN_MAX_GT]
    double *partials;            // [B][cdiv(R, RPN_TPB)][RPN_NS]
    long long total;
};

static RpnStatsWs rpn_stats_ws_layout(void *base, int B, long long R)
{
    RpnStatsWs w;
    char *p = (char *)base;
    long long o = 0;
    w.gtmax = (unsigned long long *)(p + o); o += (long long)B * M3D_RPN_MAX_GT * 8;
    w.bestrow = (unsigned *)(p + o); o += (long long)B * M3D_RPN_MAX_GT * 4;
    o = (o + 255) / 256 * 256;
    w.partials = (double *)(p + o); o += (long long)B * cdiv(R, RPN_TPB) * RPN_NS * 8;
    w.total = o;
    return w;
}

extern "C" long long m3d_rpn_target_stats_workspace_bytes(int B, long long R)
{
    if (B <= 0 || R <= 0) return -1;
    return rpn_stats_ws_layout(nullptr, B, R).total;
}

extern "C" int m3d_rpn_target_stats(const double *anchors, int A, int H, int W, const double *conf, int n_conf, const double *gt_table,
                                    int B, int Gmax, const double *center, double *out, void *workspace, long long workspace_bytes,
                                    m3d_stream_t stream)
{
    long long R;
    RpnConf cf;
    int st = rpn_check_shape("rpn_target_stats", A, H, W, B, 2, Gmax, &R);
    if (st) return st;
    if ((st = rpn_conf_from(conf, n_conf, &cf, "rpn_target_stats", true))) return st;
    M3D_REQUIRE(anchors && gt_table && center && out && workspace, "rpn_target_stats: NULL pointer");
    const RpnStatsWs ws = rpn_stats_ws_layout(workspace, B, R);
    if (workspace_bytes < ws.total) {
        m3d_set_error("rpn_target_stats: workspace %lld < %lld bytes (m3d_rpn_target_stats_workspace_bytes)", workspace_bytes, ws.total);
        return M3D_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    M3D_HIP(hipMemsetAsync(ws.gtmax, 0, (size_t)B * M3D_RPN_MAX_GT * 8, s));
    M3D_HIP(hipMemsetAsync(ws.bestrow, 0xff, (size_t)B * M3D_RPN_MAX_GT * 4, s));
    const int nwg = cdiv(R, RPN_TPB);
    const dim3 grid(nwg, B);
    hipLaunchKernelGGL(rpn_gt_max_kernel<double>, dim3(cdiv(R, RPN_TPB * RPN_MAX_ROWS), B), dim3(RPN_TPB), 0, s, anchors, gt_table, Gmax, (int)R, H, W, cf.stride, ws.gtmax);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(rpn_gt_row_kernel<double>, grid, dim3(RPN_TPB), 0, s, anchors, gt_table, Gmax, (int)R, H, W, cf.stride, ws.gtmax, ws.bestrow);
    M3D_LAUNCH_CHECK();
    RpnStatsArgs a;
    a.anchors = anchors; a.gt = gt_table; a.center = center; a.gtmax = ws.gtmax; a.bestrow = ws.bestrow; a.partials = ws.partials;
    a.Gmax = Gmax; a.R = (int)R; a.H = H; a.W = W;
    hipLaunchKernelGGL(rpn_stats_kernel, grid, dim3(RPN_TPB), 0, s, a, cf);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(rpn_stats_finish_kernel, dim3(B), dim3(RPN_SFIN_L * 32), 0, s, ws.partials, nwg, out);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}
