// Post-forward detection stage on the device (lib/rpn_util.py:1442-1555 in the reference):
//   decode of the network outputs for the top-N-pre rows, the descending score sort that picks them, and the selection of
//   the kept rows after NMS into fixed-size blocks.
//
//  * topk_decode_kernel: ONE workgroup per image does the reference's `argsort()[::-1][:nms_topN_pre]` (rpn_util.py:1510-1544)
//    as an MSD radix SELECT over the 64-bit total order  key = (sortable score bits << 32) | (0xFFFFFFFF - row)
//    -- descending score, ascending row among equal scores -- followed by a bitonic sort of the k selected keys in LDS and
//    the decode of exactly those k rows.  Level 0 histograms the top 11 score bits of all R rows (LDS atomics on integers:
//    deterministic), rows above the threshold bin are selected, rows inside it become the candidates of the next digit
//    (ping-pong buffers in the workspace; typically a few hundred rows); the walk ends as soon as the candidates left are
//    exactly the rows still needed.  No float atomics, no data-dependent launch count: graph-capturable.
//  * topk_mw_*: the same selection for ONE frame, where one workgroup per image leaves the chip idle: the level-0 pass over all R
//    keys is spread over `wgs` workgroups per image (zero -> per-slice LDS histogram added into a global one -> every workgroup
//    finds the threshold bin itself and appends its slice's keys to a global selected / candidate list), and the finishing
//    launch is topk_decode_kernel<true>: the lower digits, the sort and the decode of the single-workgroup kernel, unchanged.
//    The 64-bit keys are unique and the finish sorts them, so the output does not depend on the order of the appends.
//  * select_post_kernel: keep lists of the NMS -> [B][post + 1][14] blocks (zero padded; row `post` carries the count), the
//    wire format of the multi-GPU all-gather.
#include "common.h"

#define TOPK_NT 1024
#define TOPK_MAXK 16384                  // keys of the final sort in LDS: 8 bytes each, next power of two of k (dynamic allocation)

// Decode (lib/rpn_util.py:1442-1521 + bbox_transform_inv :1137-1186), scale_factor = 1.
// Row layout out: x1,y1,x2,y2,score,cls,x3d,y3d,z3d,w3d,h3d,l3d,ry3d,anchor  (rpn_util.py:1550)
// In two parts: what the NMS and the post-NMS cut read (the 2-D box, score and class) with the projected centre and the anchor,
// and the five columns that nobody reads before a row is among the nms_topN_post kept ones (m3d_fill_post_3d).
// 2-D / centre part: columns 0..7 and 13.  vc = the x3d, y3d outputs.
__device__ __forceinline__ void decode_values_2d(int row, const float *__restrict__ v2 /*[4]*/, const float *__restrict__ vc /*[2]*/,
                                                 float p1, float p2, float p3, const float *__restrict__ rois,
                                                 const float *__restrict__ means, const float *__restrict__ stds,
                                                 float *__restrict__ q)
{
    const float *ro = rois + (size_t)row * 5;
    const float x1 = ro[0], y1 = ro[1], x2 = ro[2], y2 = ro[3];
    const int tr = (int)ro[4];
    const float widths = x2 - x1 + 1.0f, heights = y2 - y1 + 1.0f;
    const float ctr_x = x1 + 0.5f * widths, ctr_y = y1 + 0.5f * heights;
    float d3[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) d3[k] = vc[k] * stds[4 + k] + means[4 + k];
    const float dx = v2[0] * stds[0] + means[0];
    const float dy = v2[1] * stds[1] + means[1];
    const float dw = v2[2] * stds[2] + means[2];
    const float dh = v2[3] * stds[3] + means[3];
    const float pcx = dx * widths + ctr_x, pcy = dy * heights + ctr_y;
    const float pw = expf(dw) * widths, ph = expf(dh) * heights;
    q[0] = pcx - 0.5f * pw;
    q[1] = pcy - 0.5f * ph;
    q[2] = pcx + 0.5f * pw;
    q[3] = pcy + 0.5f * ph;
    float sc = p1;
    int cl = 1;
    if (p2 > sc) { sc = p2; cl = 2; }
    if (p3 > sc) { sc = p3; cl = 3; }
    q[4] = sc;
    q[5] = (float)cl;
    q[6] = d3[0] * widths + ctr_x;
    q[7] = d3[1] * heights + ctr_y;
    q[13] = (float)tr;
}

// deferred part: columns 8..12 (z3d, w3d, h3d, l3d, ry3d) of a row whose anchor is tr.  vd = the z3d .. rY3d outputs.
__device__ __forceinline__ void decode_values_3d(int tr, const float *__restrict__ vd /*[5]*/, const float *__restrict__ anchors,
                                                 const float *__restrict__ means, const float *__restrict__ stds,
                                                 float *__restrict__ q)
{
    const float *an = anchors + tr * 9;
    float d3[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) d3[k] = vd[k] * stds[6 + k] + means[6 + k];
    q[8] = an[4] + d3[0];
    q[9] = expf(d3[1]) * an[5];
    q[10] = expf(d3[2]) * an[6];
    q[11] = expf(d3[3]) * an[7];
    q[12] = an[8] + d3[4];
}

__device__ __forceinline__ void decode_values(int row, const float *__restrict__ v2 /*[4]*/, const float *__restrict__ v3 /*[7]*/,
                                              float p1, float p2, float p3, const float *__restrict__ rois,
                                              const float *__restrict__ anchors, const float *__restrict__ means,
                                              const float *__restrict__ stds, float *__restrict__ q)
{
    decode_values_2d(row, v2, v3, p1, p2, p3, rois, means, stds, q);
    decode_values_3d((int)rois[(size_t)row * 5 + 4], v3 + 2, anchors, means, stds, q);
}

// rows of the bundled tensors prob [B][R][4], bbox_2d [B][R][4], bbox_3d [B][R][7]; o = img * R + row
__device__ __forceinline__ void decode_row(int row, size_t o, const float *__restrict__ prob, const float *__restrict__ b2,
                                           const float *__restrict__ b3, const float *__restrict__ rois,
                                           const float *__restrict__ anchors, const float *__restrict__ means,
                                           const float *__restrict__ stds, float *__restrict__ q)
{
    float v2[4], v3[7];
#pragma unroll
    for (int k = 0; k < 4; ++k) v2[k] = b2[o * 4 + k];
#pragma unroll
    for (int k = 0; k < 7; ++k) v3[k] = b3[o * 7 + k];
    decode_values(row, v2, v3, prob[o * 4 + 1], prob[o * 4 + 2], prob[o * 4 + 3], rois, anchors, means, stds, q);
}

// the same row read from the planar staging the heads write (cls [B][4A][HW], box [B][11][A*HW]): the class probabilities are
// recomputed from the four logits with the arithmetic of bundle_outputs (class_softmax4, common.h) -- the same bits.
// defer3d: box planes 6..10 are not read and columns 8..12 are +0 (m3d_topk_decode_planar_2d)
__device__ __forceinline__ void decode_row_planar(int row, int img, int A, int HW, const float *__restrict__ cls_pl,
                                                  const float *__restrict__ box_pl, const float *__restrict__ rois,
                                                  const float *__restrict__ anchors, const float *__restrict__ means,
                                                  const float *__restrict__ stds, bool defer3d, float *__restrict__ q)
{
    const int R = A * HW;
    const int an = row / HW, p = row - an * HW;
    const float *cb = cls_pl + (size_t)img * 4 * R;
    f32x4 l;
#pragma unroll
    for (int c = 0; c < 4; ++c) l[c] = cb[(size_t)(c * A + an) * HW + p];
    const f32x4 pr = class_softmax4(l);
    const float *bb = box_pl + (size_t)img * 11 * R + row;
    float v2[4], v3[7];
#pragma unroll
    for (int k = 0; k < 4; ++k) v2[k] = bb[(size_t)k * R];
    if (defer3d) {
#pragma unroll
        for (int k = 0; k < 2; ++k) v3[k] = bb[(size_t)(4 + k) * R];
        decode_values_2d(row, v2, v3, pr[1], pr[2], pr[3], rois, means, stds, q);
#pragma unroll
        for (int c = 8; c < 13; ++c) q[c] = 0.0f;
        return;
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) v3[k] = bb[(size_t)(4 + k) * R];
    decode_values(row, v2, v3, pr[1], pr[2], pr[3], rois, anchors, means, stds, q);
}

__global__ void decode_rows_kernel(const long long *__restrict__ rows, const float *__restrict__ prob,
                                   const float *__restrict__ b2, const float *__restrict__ b3,
                                   const float *__restrict__ rois, const float *__restrict__ anchors,
                                   const float *__restrict__ means, const float *__restrict__ stds,
                                   float *__restrict__ out, int R, int n_rows)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int row = (int)rows[(size_t)b * n_rows + i];
    decode_row(row, (size_t)b * R + row, prob, b2, b3, rois, anchors, means, stds, out + ((size_t)b * n_rows + i) * 14);
}

extern "C" int m3d_decode_rows(const long long *rows, const float *prob, const float *bbox_2d, const float *bbox_3d,
                               const float *rois, const float *anchors, const float *means, const float *stds,
                               float *aboxes, int B, int R, int n_rows, m3d_stream_t stream)
{
    M3D_REQUIRE(rows && prob && bbox_2d && bbox_3d && rois && anchors && means && stds && aboxes && n_rows > 0,
                "decode_rows: bad arguments");
    hipLaunchKernelGGL(decode_rows_kernel, dim3(cdiv(n_rows, 256), B), dim3(256), 0, (hipStream_t)stream, rows, prob,
                       bbox_2d, bbox_3d, rois, anchors, means, stds, aboxes, R, n_rows);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
struct TopkArgs {
    const unsigned int *score_bits;   // [B][R] monotone (sortable) bits of the row score
    const float *prob, *b2, *b3, *rois, *anchors, *means, *stds;
    float *aboxes;                    // [B][k][14]
    int *rows_out;                    // [B][k] selected rows, score-descending (optional)
    unsigned long long *cand;         // workspace [B][2][R]
    const float *scale;               // [B] or null: test-time scale factor of each image (lib/rpn_util.py:1504-1506)
    int R, k;
    int A, HW;                        // planar form (A > 0): prob = cls planar [B][4A][HW], b2 = box planar [B][11][A*HW], b3 unused
    int defer3d;                      // planar form: box planes 6..10 are not read, columns 8..12 are written as +0
    // multi-workgroup form (topk_mw_*): what the level-0 launches leave for the finishing one, behind `cand` in the workspace
    unsigned long long *mw_sel;       // [B][k] keys above the threshold bin (fewer than k by the definition of the bin)
    unsigned *mw_hist;                // [B][2048] histogram of the top 11 score bits
    unsigned *mw_cnt;                 // [B][2] keys in mw_sel, keys in cand[b][0]
};

// Exclusive prefix sum of one value per thread over the 1024-thread workgroup (16 waves): wave shuffles + one LDS hop.
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned *wave_tot /*[16] LDS*/, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int w = 0; w < wave; ++w) base += wave_tot[w];
    __syncthreads();
    return base + inc - v;
}

// the 64-bit total order: descending score, ascending row among equal scores
__device__ __forceinline__ unsigned long long topk_key(unsigned s, int row)
{
    return ((unsigned long long)s << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)row);
}

// A slice of one image's keys, in units of 16-byte groups of four keys (vec: R % 4 == 0, the image's R * 4 bytes are then 16-byte
// aligned) or of single keys.  Image b's keys are cut into `wgs` such slices; slices past the end are empty.
struct TopkSlice { int lo, hi; bool vec; };

__device__ __forceinline__ TopkSlice topk_slice(int R, int wg, int wgs)
{
    TopkSlice s;
    s.vec = (R & 3) == 0;
    const int n = s.vec ? (R >> 2) : R;
    const int per = (n + wgs - 1) / wgs;
    s.lo = min(n, wg * per);
    s.hi = min(n, s.lo + per);
    return s;
}

// f(score bits, row) for every key of the slice, strided over the workgroup: the only place that knows about the 16-byte loads
template <typename F>
__device__ __forceinline__ void topk_for_keys(const unsigned int *sc, TopkSlice sl, int tid, F f)
{
    if (sl.vec) {
        const u32x4 *sc4 = reinterpret_cast<const u32x4 *>(sc);
        for (int i = sl.lo + tid; i < sl.hi; i += TOPK_NT) {
            const u32x4 v = sc4[i];
            f(v[0], 4 * i); f(v[1], 4 * i + 1); f(v[2], 4 * i + 2); f(v[3], 4 * i + 3);
        }
    } else {
        for (int i = sl.lo + tid; i < sl.hi; i += TOPK_NT) f(sc[i], i);
    }
}

// threshold bin of a 2048-bin histogram in LDS: the highest bin b with  count(digit > b) < need <= count(digit >= b)
// -> *s_bin = b, *s_above = count(digit > b)  (both in LDS, valid for every thread on return)
__device__ __forceinline__ void topk_find_bin(const unsigned *hist, unsigned need, unsigned *wave_tot, int tid, unsigned *s_bin,
                                              unsigned *s_above)
{
    const int j0 = 2047 - 2 * tid, j1 = j0 - 1;                // two bins per thread, walking down from the top bin
    const unsigned h0 = hist[j0], h1 = hist[j1];
    const unsigned ex = block_excl_scan(h0 + h1, wave_tot, tid);
    if (ex < need && need <= ex + h0) { *s_bin = (unsigned)j0; *s_above = ex; }
    else if (ex + h0 < need && need <= ex + h0 + h1) { *s_bin = (unsigned)j1; *s_above = ex + h0; }
    __syncthreads();
}

// MW: level 0 was done by topk_mw_hist_kernel / topk_mw_scatter_kernel (selected keys in a.mw_sel, candidates in cand[img][0])
template <bool MW>
__global__ __launch_bounds__(TOPK_NT) void topk_decode_kernel(TopkArgs a)
{
    __shared__ unsigned hist[2048];
    extern __shared__ __attribute__((aligned(16))) unsigned long long sel[];      // P = next power of two >= k keys
    __shared__ unsigned wave_tot[16];
    __shared__ unsigned s_bin, s_above, s_nsel, s_ncand;
    const int img = blockIdx.x, tid = threadIdx.x;
    const int R = a.R, k = a.k;
    [[maybe_unused]] const unsigned int *sc = a.score_bits + (size_t)img * R;
    unsigned long long *candA = a.cand + (size_t)img * 2 * R, *candB = candA + R;

    unsigned need = (unsigned)k;
    if (tid == 0) { s_nsel = 0; s_ncand = 0; }
    for (int i = tid; i < 2048; i += TOPK_NT) hist[i] = 0;
    __syncthreads();
    // ---- level 0: top 11 bits of the score over all R rows -----------------------------------------------------------
    unsigned ncand;
    if constexpr (!MW) {
        const TopkSlice all = topk_slice(R, 0, 1);                 // the whole image
        topk_for_keys(sc, all, tid, [&](unsigned s, int) { atomicAdd(&hist[s >> 21], 1u); });
        __syncthreads();
        topk_find_bin(hist, need, wave_tot, tid, &s_bin, &s_above);
        const unsigned bin = s_bin;
        topk_for_keys(sc, all, tid, [&](unsigned s, int row) {
            const unsigned d = s >> 21;
            if (d >= bin) {
                const unsigned long long key = topk_key(s, row);
                if (d > bin) sel[atomicAdd(&s_nsel, 1u)] = key;
                else candA[atomicAdd(&s_ncand, 1u)] = key;
            }
        });
        __threadfence_block();
        __syncthreads();
        need -= s_above;
        ncand = s_ncand;
        __syncthreads();                                           // everyone has read the counters before they are reset
    } else {
        const unsigned nsel = min(a.mw_cnt[2 * img], (unsigned)k);
        const unsigned long long *gsel = a.mw_sel + (size_t)img * k;
        for (unsigned i = tid; i < nsel; i += TOPK_NT) sel[i] = gsel[i];
        if (tid == 0) s_nsel = nsel;
        need -= nsel;                                          // = count(digit > threshold bin)
        ncand = min(a.mw_cnt[2 * img + 1], (unsigned)R);
        __syncthreads();
    }
    // ---- lower digits over the candidate list (global ping-pong; the workgroup is its only reader / writer) ---------
    // key bits 52..42, 41..32, then the row part: bits 31..22 are all ones for R < 2^22, so 21..11 and 10..0
    const int shifts[4] = {42, 32, 11, 0};
    const unsigned masks[4] = {0x7FFu, 0x3FFu, 0x7FFu, 0x7FFu};
    for (int lv = 0; lv < 4 && ncand != need; ++lv) {
        const int sh = shifts[lv];
        const unsigned mk = masks[lv];
        for (int i = tid; i < 2048; i += TOPK_NT) hist[i] = 0;
        if (tid == 0) s_ncand = 0;
        __syncthreads();
        for (unsigned i = tid; i < ncand; i += TOPK_NT) atomicAdd(&hist[(unsigned)(candA[i] >> sh) & mk], 1u);
        __syncthreads();
        topk_find_bin(hist, need, wave_tot, tid, &s_bin, &s_above);
        const unsigned bin = s_bin;
        for (unsigned i = tid; i < ncand; i += TOPK_NT) {
            const unsigned long long key = candA[i];
            const unsigned d = (unsigned)(key >> sh) & mk;
            if (d > bin) sel[atomicAdd(&s_nsel, 1u)] = key;
            else if (d == bin) candB[atomicAdd(&s_ncand, 1u)] = key;
        }
        __threadfence_block();
        __syncthreads();
        need -= s_above;
        ncand = s_ncand;
        unsigned long long *t = candA; candA = candB; candB = t;
        __syncthreads();
    }
    // the candidates left are exactly the rows still needed (keys are unique, so the walk always ends here)
    {
        const unsigned base = s_nsel;
        for (unsigned i = tid; i < need; i += TOPK_NT) sel[base + i] = candA[i];
    }
    // ---- bitonic sort of the k keys, descending (padding keys 0 sort last) -------------------------------------------
    int P = 1;
    while (P < k) P <<= 1;
    for (int i = k + tid; i < P; i += TOPK_NT) sel[i] = 0ULL;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += TOPK_NT) {
                const int lo = 2 * t - (t & (stride - 1));     // index with bit `stride` clear
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const unsigned long long x = sel[lo], y = sel[hi];
                if ((x < y) == desc) { sel[lo] = y; sel[hi] = x; }
            }
            __syncthreads();
        }
    }
    // ---- decode exactly the k selected rows --------------------------------------------------------------------------
    for (int i = tid; i < k; i += TOPK_NT) {
        const int row = (int)(0xFFFFFFFFu - (unsigned)sel[i]);
        if (a.rows_out) a.rows_out[(size_t)img * k + i] = row;
        float *q = a.aboxes + ((size_t)img * k + i) * 14;
        if (a.A > 0) decode_row_planar(row, img, a.A, a.HW, a.prob, a.b2, a.rois, a.anchors, a.means, a.stds, a.defer3d != 0, q);
        else decode_row(row, (size_t)img * R + row, a.prob, a.b2, a.b3, a.rois, a.anchors, a.means, a.stds, q);
        if (a.scale) {
            // `coords_2d[:, 0:4] /= scale_factor; coords_3d[:, 0:2] /= scale_factor` BEFORE the sort and the NMS, as the reference
            // does it (lib/rpn_util.py:1504-1506): the +1 convention of the NMS areas is not scale invariant, so an IoU next to
            // nms_thres can fall on the other side when the division comes after the NMS.  float32 divisions like torch's.
            const float sf = a.scale[img];
#pragma unroll
            for (int c = 0; c < 4; ++c) q[c] = __fdiv_rn(q[c], sf);
            q[6] = __fdiv_rn(q[6], sf);
            q[7] = __fdiv_rn(q[7], sf);
        }
    }
}

template <bool MW>
static int topk_launch(const TopkArgs &a, int B, hipStream_t stream)
{
    int P = 1;
    while (P < a.k) P <<= 1;
    const int lds = P * (int)sizeof(unsigned long long);             // <= 128 KB (+ 8 KB of static LDS)
    if (lds > 32768) {
        static m3d_lds_state raised;                                   // (per kernel form)
        int dev = 0;
        M3D_HIP(hipGetDevice(&dev));
        M3D_REQUIRE(m3d_raise_dyn_lds(&topk_decode_kernel<MW>, TOPK_MAXK * (int)sizeof(unsigned long long), raised) == M3D_OK,
                    "topk_decode: device %d cannot reserve %d bytes of LDS for k = %d", dev, lds, a.k);
    }
    hipLaunchKernelGGL(topk_decode_kernel<MW>, dim3(B), dim3(TOPK_NT), lds, stream, a);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

extern "C" long long m3d_topk_decode_workspace_bytes(int B, int R)
{
    return (long long)B * 2 * R * (long long)sizeof(unsigned long long);
}

static long long topk_mw_align(long long v) { return (v + 15) & ~15LL; }

extern "C" long long m3d_topk_decode_mw_workspace_bytes(int B, int R, int k)
{
    if (B < 1 || R < 1 || k < 1) return -1;
    // cand [B][2][R] keys (the layout of m3d_topk_decode_workspace_bytes), selected keys [B][k], histogram [B][2048], counters [B][2]
    return m3d_topk_decode_workspace_bytes(B, R) + (long long)B * k * (long long)sizeof(unsigned long long)
           + (long long)B * 2048 * (long long)sizeof(unsigned) + topk_mw_align((long long)B * 2 * (long long)sizeof(unsigned));
}

// The argument checks, the workspace check and the TopkArgs of every m3d_topk_decode* entry point (`name`: the one in the messages).
//   bundled (planar = false): prob / b2 / b3 = prob, bbox_2d, bbox_3d [B][R][*], n0 = R, n1 unused
//   planar:                   prob / b2 = cls planar, box planar, b3 unused, (n0, n1) = (A, HW)
//   mw: the workspace rule and the mw_* pointers of the multi-workgroup form
static int topk_args(TopkArgs &a, bool planar, bool mw, const char *name, const unsigned int *score_bits, const float *prob,
                     const float *b2, const float *b3, const float *rois, const float *anchors, const float *means,
                     const float *stds, const float *scale, float *aboxes, int *rows_out, void *workspace, long long workspace_bytes,
                     int B, int n0, int n1, int k)
{
    a = TopkArgs{};
    M3D_REQUIRE(score_bits && prob && b2 && (planar || b3) && rois && anchors && means && stds && aboxes && workspace,
                "%s: null pointer", name);
    if (!planar) n1 = 1;
    M3D_REQUIRE(B >= 1 && n0 >= 1 && n1 >= 1 && (long long)n0 * n1 < (1 << 22), "%s: %s (%lld) must be in [1, 2^22)", name,
                planar ? "A * HW" : "R", (long long)n0 * n1);
    const int R = n0 * n1;
    M3D_REQUIRE(k >= 1 && k <= R && k <= TOPK_MAXK, "%s: k (%d) must be in [1, min(R, %d)]", name, k, TOPK_MAXK);
    const long long need = mw ? m3d_topk_decode_mw_workspace_bytes(B, R, k) : m3d_topk_decode_workspace_bytes(B, R);
    if (workspace_bytes < need) {
        m3d_set_error("%s: workspace of %lld bytes, %lld needed", name, workspace_bytes, need);
        return M3D_E_WORKSPACE;
    }
    a.score_bits = score_bits; a.prob = prob; a.b2 = b2; a.b3 = b3; a.rois = rois; a.anchors = anchors;
    a.means = means; a.stds = stds; a.aboxes = aboxes; a.rows_out = rows_out; a.cand = (unsigned long long *)workspace;
    a.scale = scale; a.R = R; a.k = k;
    if (planar) { a.A = n0; a.HW = n1; }
    if (mw) {
        a.mw_sel = a.cand + (size_t)B * 2 * R;
        a.mw_hist = reinterpret_cast<unsigned *>(a.mw_sel + (size_t)B * k);
        a.mw_cnt = a.mw_hist + (size_t)B * 2048;
    }
    return M3D_OK;
}

extern "C" int m3d_topk_decode(const unsigned int *score_bits, const float *prob, const float *bbox_2d, const float *bbox_3d,
                               const float *rois, const float *anchors, const float *means, const float *stds, float *aboxes,
                               int *rows_out, void *workspace, long long workspace_bytes, int B, int R, int k,
                               m3d_stream_t stream)
{
    return m3d_topk_decode_scaled(score_bits, prob, bbox_2d, bbox_3d, rois, anchors, means, stds, nullptr, aboxes, rows_out, workspace,
                                  workspace_bytes, B, R, k, stream);
}

extern "C" int m3d_topk_decode_scaled(const unsigned int *score_bits, const float *prob, const float *bbox_2d, const float *bbox_3d,
                                      const float *rois, const float *anchors, const float *means, const float *stds,
                                      const float *scale, float *aboxes, int *rows_out, void *workspace, long long workspace_bytes,
                                      int B, int R, int k, m3d_stream_t stream)
{
    TopkArgs a;
    const int rc = topk_args(a, false, false, "topk_decode", score_bits, prob, bbox_2d, bbox_3d, rois, anchors, means, stds, scale,
                             aboxes, rows_out, workspace, workspace_bytes, B, R, 0, k);
    return rc != M3D_OK ? rc : topk_launch<false>(a, B, (hipStream_t)stream);
}

extern "C" int m3d_topk_decode_planar(const unsigned int *score_bits, const float *cls_planar, const float *box_planar,
                                      const float *rois, const float *anchors, const float *means, const float *stds,
                                      const float *scale, float *aboxes, int *rows_out, void *workspace, long long workspace_bytes,
                                      int B, int A, int HW, int k, m3d_stream_t stream)
{
    TopkArgs a;
    const int rc = topk_args(a, true, false, "topk_decode_planar", score_bits, cls_planar, box_planar, nullptr, rois, anchors, means,
                             stds, scale, aboxes, rows_out, workspace, workspace_bytes, B, A, HW, k);
    return rc != M3D_OK ? rc : topk_launch<false>(a, B, (hipStream_t)stream);
}

extern "C" int m3d_topk_decode_planar_2d(const unsigned int *score_bits, const float *cls_planar, const float *box_planar,
                                         const float *rois, const float *anchors, const float *means, const float *stds,
                                         const float *scale, float *aboxes, int *rows_out, void *workspace,
                                         long long workspace_bytes, int B, int A, int HW, int k, m3d_stream_t stream)
{
    M3D_REQUIRE(rows_out, "topk_decode_planar_2d: rows_out is required (m3d_fill_post_3d finds the staging rows through it)");
    TopkArgs a;
    const int rc = topk_args(a, true, false, "topk_decode_planar_2d", score_bits, cls_planar, box_planar, nullptr, rois, anchors,
                             means, stds, scale, aboxes, rows_out, workspace, workspace_bytes, B, A, HW, k);
    a.defer3d = 1;
    return rc != M3D_OK ? rc : topk_launch<false>(a, B, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Multi-workgroup level 0 (one frame on a 256-CU chip: one workgroup per image reads all R keys twice from a single CU).
// Image b's keys are cut into `wgs` slices (topk_slice).
//   zero    : global histogram and the two list counters of every image (nothing carries over from an earlier call)
//   hist    : per-slice LDS histogram of the top 11 score bits, non-zero bins added into the image's global histogram
//   scatter : every workgroup finds the threshold bin from the global histogram, counts its slice's keys above / inside the
//             bin, reserves room in the global lists with ONE atomicAdd per list, and writes the keys there
//   finish  : topk_decode_kernel<true>
// Integer atomics only.  The launch list is fixed: graph-capturable.
#define TOPK_MW_MAX_WGS 256               // per image: one slice per CU
// library's choice for wgs_per_image = 0: one slice per four CUs, 1 080 16-byte groups per slice at R = 276 480.  To be replaced by the
// best of the sweep of tools/latency_frame.py's kernel leg (B = 1, R = 276 480, k = 3000; profiles/latency_frame.jsonl): NOT MEASURED yet.
#define TOPK_MW_DEFAULT_WGS 64

__global__ __launch_bounds__(TOPK_NT) void topk_mw_zero_kernel(TopkArgs a)
{
    const int img = blockIdx.x;
    for (int i = threadIdx.x; i < 2048; i += TOPK_NT) a.mw_hist[(size_t)img * 2048 + i] = 0;
    if (threadIdx.x < 2) a.mw_cnt[2 * img + threadIdx.x] = 0;
}

__global__ __launch_bounds__(TOPK_NT) void topk_mw_hist_kernel(TopkArgs a)
{
    __shared__ unsigned hist[2048];
    const int img = blockIdx.y, tid = threadIdx.x;
    const TopkSlice sl = topk_slice(a.R, blockIdx.x, gridDim.x);
    if (sl.lo >= sl.hi) return;                            // (uniform over the workgroup)
    const unsigned int *sc = a.score_bits + (size_t)img * a.R;
    for (int i = tid; i < 2048; i += TOPK_NT) hist[i] = 0;
    __syncthreads();
    topk_for_keys(sc, sl, tid, [&](unsigned s, int) { atomicAdd(&hist[s >> 21], 1u); });
    __syncthreads();
    unsigned *gh = a.mw_hist + (size_t)img * 2048;
    for (int i = tid; i < 2048; i += TOPK_NT) {
        const unsigned h = hist[i];
        if (h) atomicAdd(&gh[i], h);
    }
}

__global__ __launch_bounds__(TOPK_NT) void topk_mw_scatter_kernel(TopkArgs a)
{
    __shared__ unsigned hist[2048];
    __shared__ unsigned wave_tot[16];
    __shared__ unsigned s_bin, s_above, s_csel, s_ccand, s_bsel, s_bcand, s_isel, s_icand;
    const int img = blockIdx.y, tid = threadIdx.x;
    const int R = a.R, k = a.k;
    const TopkSlice sl = topk_slice(R, blockIdx.x, gridDim.x);
    if (sl.lo >= sl.hi) return;
    const unsigned int *sc = a.score_bits + (size_t)img * R;
    const unsigned *gh = a.mw_hist + (size_t)img * 2048;
    for (int i = tid; i < 2048; i += TOPK_NT) hist[i] = gh[i];
    if (tid == 0) { s_csel = 0; s_ccand = 0; s_isel = 0; s_icand = 0; }
    __syncthreads();
    topk_find_bin(hist, (unsigned)k, wave_tot, tid, &s_bin, &s_above);      // (the finishing launch counts the keys above the bin itself)
    const unsigned bin = s_bin;
    // how many keys of the slice go to either list
    unsigned csel = 0, ccand = 0;
    topk_for_keys(sc, sl, tid, [&](unsigned s, int) {
        const unsigned d = s >> 21;
        csel += d > bin;
        ccand += d == bin;
    });
    if (csel) atomicAdd(&s_csel, csel);
    if (ccand) atomicAdd(&s_ccand, ccand);
    __syncthreads();
    if (s_csel == 0 && s_ccand == 0) return;               // (uniform)
    if (tid == 0) {
        s_bsel = s_csel ? atomicAdd(&a.mw_cnt[2 * img], s_csel) : 0;
        s_bcand = s_ccand ? atomicAdd(&a.mw_cnt[2 * img + 1], s_ccand) : 0;
    }
    __syncthreads();
    const unsigned bsel = s_bsel, bcand = s_bcand;
    unsigned long long *gsel = a.mw_sel + (size_t)img * k;
    unsigned long long *cand = a.cand + (size_t)img * 2 * R;
    topk_for_keys(sc, sl, tid, [&](unsigned s, int row) {
        const unsigned d = s >> 21;
        if (d >= bin) {
            const unsigned long long key = topk_key(s, row);
            if (d > bin) {
                const unsigned at = bsel + atomicAdd(&s_isel, 1u);
                if (at < (unsigned)k) gsel[at] = key;      // (count(digit > bin) < k: the bound never binds)
            } else {
                const unsigned at = bcand + atomicAdd(&s_icand, 1u);
                if (at < (unsigned)R) cand[at] = key;
            }
        }
    });
}

extern "C" int m3d_topk_decode_planar_mw(const unsigned int *score_bits, const float *cls_planar, const float *box_planar,
                                         const float *rois, const float *anchors, const float *means, const float *stds,
                                         const float *scale, float *aboxes, int *rows_out, void *workspace,
                                         long long workspace_bytes, int B, int A, int HW, int k, int wgs_per_image,
                                         m3d_stream_t stream)
{
    M3D_REQUIRE(wgs_per_image >= 0 && wgs_per_image <= TOPK_MW_MAX_WGS,
                "topk_decode_planar_mw: wgs_per_image (%d) must be in [0, %d] (0 = library's choice)", wgs_per_image, TOPK_MW_MAX_WGS);
    TopkArgs a;
    const int rc = topk_args(a, true, true, "topk_decode_planar_mw", score_bits, cls_planar, box_planar, nullptr, rois, anchors, means,
                             stds, scale, aboxes, rows_out, workspace, workspace_bytes, B, A, HW, k);
    if (rc != M3D_OK) return rc;
    int wgs = wgs_per_image;
    if (wgs == 0) {                                        // no more slices than there are workgroup-sized pieces of the image
        const int units = (a.R & 3) ? a.R : (a.R >> 2);
        wgs = max(1, min(TOPK_MW_DEFAULT_WGS, cdiv(units, TOPK_NT)));
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(topk_mw_zero_kernel, dim3(B), dim3(TOPK_NT), 0, st, a);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(topk_mw_hist_kernel, dim3(wgs, B), dim3(TOPK_NT), 0, st, a);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(topk_mw_scatter_kernel, dim3(wgs, B), dim3(TOPK_NT), 0, st, a);
    M3D_LAUNCH_CHECK();
    return topk_launch<true>(a, B, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// Needed pixels (m3d_need_rows): the detection stage decodes the k highest-scoring rows of an image and nothing else, and row
// a * HW + pix belongs to pixel pix, so a box head whose output feeds only the decode is needed at the pixels that hold one of
// those rows.  T_b = the exact k-th largest 32-bit key of image b by a three-digit radix select (11 + 11 + 10 bits; the top 11
// bits alone put every score in [0.5, 1) into four bins), need[b][pix] = any of the pixel's A keys >= T_b (ties at T_b only
// enlarge the set), rows = the needed pixels b * HW + pix in ascending order, *n_rows their number.
//   zero    : the three global histograms of every image
//   hist<l> : every workgroup finds the bins of the digits above l from the global histograms, then histograms digit l of its
//             slice's keys that carry that prefix (LDS atomics, non-zero bins added to the global histogram)
//   mark    : T_b from the three histograms; one workgroup per 256 pixels sets need[] and counts its pixels
//   compact : the slice's place in the list = the counts of the slices in front of it; ordered scan inside the slice
// Integer atomics only, fixed grids, every count stays on the device: graph-capturable.
#define NEED_PX 256                      // pixels per workgroup of the mark / compact launches

struct NeedArgs {
    const unsigned int *score_bits;   // [B][A*HW]
    unsigned *hist;                   // [B][3][2048]
    unsigned *cnt;                    // [B][nsl] needed pixels of every 256-pixel slice
    unsigned *thresh;                 // [B]
    unsigned char *need;              // [B][HW]
    int *rows, *n_rows;
    int R, A, HW, k, nsl, B;
};

// the digits above level LV of the k-th largest key: -> prefix (the key bits above digit LV), *need = its rank inside that prefix
template <int LV>
__device__ __forceinline__ unsigned need_prefix(const NeedArgs &a, int img, unsigned *hist, unsigned *wave_tot, unsigned *s_bin,
                                                unsigned *s_above, int tid, unsigned *need)
{
    unsigned prefix = 0;
#pragma unroll
    for (int l = 0; l < LV; ++l) {
        const unsigned *gh = a.hist + ((size_t)img * 3 + l) * 2048;
        for (int i = tid; i < 2048; i += TOPK_NT) hist[i] = gh[i];
        __syncthreads();
        topk_find_bin(hist, *need, wave_tot, tid, s_bin, s_above);
        prefix = (prefix << (l == 2 ? 10 : 11)) | *s_bin;
        *need -= *s_above;
    }
    return prefix;
}

__global__ __launch_bounds__(TOPK_NT) void need_zero_kernel(NeedArgs a)
{
    for (int i = threadIdx.x; i < 3 * 2048; i += TOPK_NT) a.hist[(size_t)blockIdx.x * 3 * 2048 + i] = 0;
}

template <int LV>
__global__ __launch_bounds__(TOPK_NT) void need_hist_kernel(NeedArgs a)
{
    __shared__ unsigned hist[2048];
    __shared__ unsigned wave_tot[16];
    __shared__ unsigned s_bin, s_above;
    const int img = blockIdx.y, tid = threadIdx.x;
    const TopkSlice sl = topk_slice(a.R, blockIdx.x, gridDim.x);
    if (sl.lo >= sl.hi) return;                            // (uniform over the workgroup)
    unsigned need = (unsigned)a.k;
    const unsigned prefix = need_prefix<LV>(a, img, hist, wave_tot, &s_bin, &s_above, tid, &need);
    __syncthreads();
    for (int i = tid; i < 2048; i += TOPK_NT) hist[i] = 0;
    __syncthreads();
    constexpr int sh = LV == 0 ? 21 : LV == 1 ? 10 : 0;
    constexpr unsigned mk = LV == 2 ? 0x3FFu : 0x7FFu;
    constexpr int psh = LV == 1 ? 21 : 10;                 // (LV > 0) the bits above this digit
    topk_for_keys(a.score_bits + (size_t)img * a.R, sl, tid, [&](unsigned s, int) {
        if (LV == 0 || (s >> psh) == prefix) atomicAdd(&hist[(s >> sh) & mk], 1u);
    });
    __syncthreads();
    unsigned *gh = a.hist + ((size_t)img * 3 + LV) * 2048;
    for (int i = tid; i < 2048; i += TOPK_NT) {
        const unsigned h = hist[i];
        if (h) atomicAdd(&gh[i], h);
    }
}

__global__ __launch_bounds__(TOPK_NT) void need_mark_kernel(NeedArgs a)
{
    __shared__ unsigned hist[2048];
    __shared__ unsigned wave_tot[16];
    __shared__ unsigned s_bin, s_above, s_cnt;
    __shared__ unsigned s_need[NEED_PX];
    const int img = blockIdx.y, tid = threadIdx.x;
    if (tid < NEED_PX) s_need[tid] = 0;
    if (tid == 0) s_cnt = 0;
    unsigned need = (unsigned)a.k;
    const unsigned T = need_prefix<3>(a, img, hist, wave_tot, &s_bin, &s_above, tid, &need);
    const int pl = tid & (NEED_PX - 1), ag = tid / NEED_PX;            // four threads per pixel, each takes every fourth anchor
    const int p = blockIdx.x * NEED_PX + pl;
    if (p < a.HW) {
        const unsigned int *sc = a.score_bits + (size_t)img * a.R + p;
        bool f = false;
        for (int an = ag; an < a.A; an += TOPK_NT / NEED_PX) f |= sc[(size_t)an * a.HW] >= T;
        if (f) s_need[pl] = 1;
    }
    __syncthreads();
    if (tid < NEED_PX) {                                               // (whole waves)
        const bool f = p < a.HW && s_need[tid];
        if (p < a.HW) a.need[(size_t)img * a.HW + p] = f ? 1 : 0;
        const unsigned c = (unsigned)__popcll(__ballot(f));
        if ((tid & 63) == 0 && c) atomicAdd(&s_cnt, c);
    }
    __syncthreads();
    if (tid == 0) {
        a.cnt[(size_t)img * a.nsl + blockIdx.x] = s_cnt;
        if (blockIdx.x == 0) a.thresh[img] = T;
    }
}

__global__ __launch_bounds__(NEED_PX) void need_compact_kernel(NeedArgs a)
{
    __shared__ unsigned wave_tot[16];
    __shared__ unsigned s_part[NEED_PX / 64][2];
    const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int me = img * a.nsl + blockIdx.x, total = a.B * a.nsl;
    unsigned before = 0, all = 0;
    for (int i = tid; i < total; i += NEED_PX) {
        const unsigned v = a.cnt[i];
        all += v;
        if (i < me) before += v;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        before += __shfl_xor(before, d, 64);
        all += __shfl_xor(all, d, 64);
    }
    if (lane == 0) { s_part[wave][0] = before; s_part[wave][1] = all; }
    __syncthreads();
    before = 0; all = 0;
#pragma unroll
    for (int w = 0; w < NEED_PX / 64; ++w) { before += s_part[w][0]; all += s_part[w][1]; }
    const int p = blockIdx.x * NEED_PX + tid;
    const unsigned f = (p < a.HW && a.need[(size_t)img * a.HW + p]) ? 1u : 0u;
    const unsigned ex = block_excl_scan(f, wave_tot, tid);
    if (f) a.rows[before + ex] = img * a.HW + p;
    if (me == 0 && tid == 0) *a.n_rows = (int)all;
}

extern "C" long long m3d_need_rows_workspace_bytes(int B, int HW)
{
    if (B < 1 || HW < 1) return -1;
    return (long long)B * 3 * 2048 * (long long)sizeof(unsigned) + (long long)B * cdiv(HW, NEED_PX) * (long long)sizeof(unsigned);
}

extern "C" int m3d_need_rows(const unsigned int *score_bits, int B, int A, int HW, int k, unsigned int *thresh,
                             unsigned char *need, int *rows, int *n_rows, void *workspace, long long workspace_bytes,
                             m3d_stream_t stream)
{
    M3D_REQUIRE(score_bits && thresh && need && rows && n_rows && workspace, "need_rows: null pointer");
    M3D_REQUIRE(B >= 1 && A >= 1 && HW >= 1 && (long long)A * HW < (1ll << 31) && (long long)B * HW < (1ll << 31) &&
                    cdiv(HW, NEED_PX) <= 65535 && B <= 65535,
                "need_rows: bad B / A / HW (%d, %d, %d)", B, A, HW);
    M3D_REQUIRE(k >= 1, "need_rows: k (%d) must be positive", k);
    M3D_REQUIRE(((uintptr_t)score_bits & 15) == 0, "need_rows: score_bits must be 16-byte aligned");
    const long long nb = m3d_need_rows_workspace_bytes(B, HW);
    if (workspace_bytes < nb) {
        m3d_set_error("need_rows: workspace of %lld bytes, %lld needed", workspace_bytes, nb);
        return M3D_E_WORKSPACE;
    }
    NeedArgs a;
    a.score_bits = score_bits;
    a.hist = (unsigned *)workspace;
    a.cnt = a.hist + (size_t)B * 3 * 2048;
    a.thresh = thresh; a.need = need; a.rows = rows; a.n_rows = n_rows;
    a.R = A * HW; a.A = A; a.HW = HW; a.B = B;
    a.k = k < a.R ? k : a.R;                               // k >= A * HW: the threshold is the smallest key, every pixel is needed
    a.nsl = cdiv(HW, NEED_PX);
    const int units = (a.R & 3) ? a.R : (a.R >> 2);
    const int wgs = max(1, min(TOPK_MW_DEFAULT_WGS, cdiv(units, TOPK_NT)));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(need_zero_kernel, dim3(B), dim3(TOPK_NT), 0, st, a);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(need_hist_kernel<0>, dim3(wgs, B), dim3(TOPK_NT), 0, st, a);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(need_hist_kernel<1>, dim3(wgs, B), dim3(TOPK_NT), 0, st, a);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(need_hist_kernel<2>, dim3(wgs, B), dim3(TOPK_NT), 0, st, a);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(need_mark_kernel, dim3(a.nsl, B), dim3(TOPK_NT), 0, st, a);
    M3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(need_compact_kernel, dim3(a.nsl, B), dim3(NEED_PX), 0, st, a);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Kept rows -> fixed-size blocks.  block [B][post + 1][14]: rows [0, min(num, post)) = aboxes[keep[j]], the rest zero;
// row `post` = (count, 0, ...).  counts [B] gets the same count as int32.
__global__ void select_post_kernel(const float *__restrict__ aboxes, const int *__restrict__ keep, const int *__restrict__ num,
                                   int n, int post, float *__restrict__ block, int *__restrict__ counts)
{
    const int b = blockIdx.x;
    const int cnt = min(num[b], post);
    for (int e = threadIdx.x; e < (post + 1) * 14; e += blockDim.x) {
        const int j = e / 14, c = e - j * 14;
        float v = 0.f;
        if (j < cnt) v = aboxes[((size_t)b * n + keep[(size_t)b * n + j]) * 14 + c];
        else if (j == post && c == 0) v = (float)cnt;
        block[(size_t)b * (post + 1) * 14 + e] = v;
    }
    if (threadIdx.x == 0 && counts) counts[b] = cnt;
}

extern "C" int m3d_select_post(const float *aboxes, const int *keep, const int *num_keep, int B, int n, int post, float *block,
                               int *counts, m3d_stream_t stream)
{
    M3D_REQUIRE(aboxes && keep && num_keep && block && B >= 1 && n >= 1 && post >= 1, "select_post: bad arguments");
    hipLaunchKernelGGL(select_post_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, aboxes, keep, num_keep, n, post, block,
                       counts);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The 3-D size, depth and angle of a row (columns 8..12) are read by nobody unless the row is among the `post` rows per image
// that select_post_kernel copies: the heads behind them run at the pixels of those rows only.
//  * post_rows_kernel: ONE workgroup.  Entry (b, j < min(num_keep[b], post)) is pixel b * HW + rows_out[b][keep[b][j]] % HW; the
//    B * post entries (absent ones = INT_MAX) are sorted ascending in LDS (bitonic), every value that differs from its
//    predecessor is kept, and an ordered scan places it: the list contract of m3d_need_rows (distinct, ascending, n_rows on the
//    device, nothing written past it).  Nothing carries over between calls.
//  * fill_post_3d_kernel: columns 8..12 of the selected rows from box planes 6..10, with decode_values_3d (the bits of the
//    full decode).
#define POST_ROWS_MAX 4096               // B * post entries of the sort (bs 64 x nms_topN_post 40 = 2560)
#define POST_ROWS_NT 1024

__global__ __launch_bounds__(POST_ROWS_NT) void post_rows_kernel(const int *__restrict__ rows_out, const int *__restrict__ keep,
                                                                 const int *__restrict__ num, int B, int n, int post, int HW,
                                                                 int *__restrict__ rows, int *__restrict__ n_rows)
{
    __shared__ int s[POST_ROWS_MAX];
    __shared__ unsigned wave_tot[16];
    const int tid = threadIdx.x;
    const int total = B * post;
    int P = 1;
    while (P < total) P <<= 1;                                         // <= POST_ROWS_MAX (checked by the launcher)
    for (int e = tid; e < P; e += POST_ROWS_NT) {
        int v = 0x7FFFFFFF;
        if (e < total) {
            const int b = e / post, j = e - b * post;
            if (j < min(num[b], post)) {
                const int kp = keep[(size_t)b * n + j];
                if (kp >= 0 && kp < n) {
                    const int row = rows_out[(size_t)b * n + kp];
                    if (row >= 0) v = b * HW + row % HW;
                }
            }
        }
        s[e] = v;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += POST_ROWS_NT) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool asc = ((lo & size) == 0);
                const int x = s[lo], y = s[hi];
                if ((x > y) == asc) { s[lo] = y; s[hi] = x; }
            }
            __syncthreads();
        }
    }
    // thread t owns the four sorted entries [4t, 4t + 4): P <= 4 * POST_ROWS_NT
    int v[4];
    unsigned f[4], c = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = 4 * tid + i;
        v[i] = e < P ? s[e] : 0x7FFFFFFF;
        f[i] = (v[i] != 0x7FFFFFFF && (e == 0 || s[e - 1] != v[i])) ? 1u : 0u;
        c += f[i];
    }
    unsigned at = block_excl_scan(c, wave_tot, tid);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (f[i]) rows[at++] = v[i];
    if (tid == POST_ROWS_NT - 1) *n_rows = (int)at;                    // (the last thread's end = the total)
}

extern "C" int m3d_post_rows(const int *rows_out, const int *keep, const int *num_keep, int B, int n, int post, int HW, int *rows,
                             int *n_rows, m3d_stream_t stream)
{
    M3D_REQUIRE(rows_out && keep && num_keep && rows && n_rows, "post_rows: null pointer");
    M3D_REQUIRE(B >= 1 && n >= 1 && post >= 1 && HW >= 1 && (long long)B * HW < (1ll << 31), "post_rows: bad B / n / post / HW (%d, %d, %d, %d)",
                B, n, post, HW);
    M3D_REQUIRE((long long)B * post <= POST_ROWS_MAX, "post_rows: B * post (%lld) must be at most %d", (long long)B * post,
                POST_ROWS_MAX);
    hipLaunchKernelGGL(post_rows_kernel, dim3(1), dim3(POST_ROWS_NT), 0, (hipStream_t)stream, rows_out, keep, num_keep, B, n, post,
                       HW, rows, n_rows);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

__global__ void fill_post_3d_kernel(const float *__restrict__ box_pl, const float *__restrict__ rois,
                                    const float *__restrict__ anchors, const float *__restrict__ means,
                                    const float *__restrict__ stds, const int *__restrict__ rows_out, const int *__restrict__ keep,
                                    const int *__restrict__ counts, int R, int n, int post, float *__restrict__ block)
{
    const int b = blockIdx.x;
    const int cnt = min(counts[b], post);
    for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
        const int kp = keep[(size_t)b * n + j];
        if (kp < 0 || kp >= n) continue;
        const int row = rows_out[(size_t)b * n + kp];
        if (row < 0 || row >= R) continue;
        const float *bb = box_pl + (size_t)b * 11 * R + row;
        float vd[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) vd[k] = bb[(size_t)(6 + k) * R];
        decode_values_3d((int)rois[(size_t)row * 5 + 4], vd, anchors, means, stds, block + ((size_t)b * (post + 1) + j) * 14);
    }
}

extern "C" int m3d_fill_post_3d(const float *box_planar, const float *rois, const float *anchors, const float *means,
                                const float *stds, const int *rows_out, const int *keep, const int *counts, int B, int A, int HW,
                                int n, int post, float *block, m3d_stream_t stream)
{
    M3D_REQUIRE(box_planar && rois && anchors && means && stds && rows_out && keep && counts && block, "fill_post_3d: null pointer");
    M3D_REQUIRE(B >= 1 && A >= 1 && HW >= 1 && n >= 1 && post >= 1 && (long long)A * HW < (1 << 22),
                "fill_post_3d: bad B / A / HW / n / post (%d, %d, %d, %d, %d)", B, A, HW, n, post);
    hipLaunchKernelGGL(fill_post_3d_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, box_planar, rois, anchors, means, stds,
                       rows_out, keep, counts, A * HW, n, post, block);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}
