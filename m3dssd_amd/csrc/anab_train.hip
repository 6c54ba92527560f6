// The ANAB attention core for training (model/module/attention.py:136-147, 207-211): the forward through the inference launches
// and a hand-written backward.  Per image, fp32, N = H*W pixels, 337 keys (the AdaptiveAvgPool2d bins of sizes 1/4/8/16):
//     khat[b] = mean_{p in win_b} g[p][scale(b)] k[p]        vhat likewise from v
//     S = q khat^T,  P = softmax_keys(S),  O = P vhat
// Backward (dO = grad_out):  dvhat = P^T dO,  dP = dO vhat^T,  D = rowsum(dO * O) = rowsum(P * dP),  dS = P * (dP - D),
//     dq = dS khat,  dkhat = dS^T q;   with w_b(p) = [p in win_b] / area_b:
//     dk[p] = sum_b w_b(p) g[p][scale(b)] dkhat[b],  dv likewise,  dg[p][s] = sum_{b of scale s} w_b(p) (k[p].dkhat[b] + v[p].dvhat[b])
//
// The backward in launches (everything on one stream, nothing atomic, every sum in a fixed order):
//   1. the pooling of the forward again (khat, vhat^T into the zeroed workspace), vhat^T transposed to vhat [key][Cv];
//   2. anab_bwd_pix_kernel, PIXEL-major, the shape of csrc/anab_attend.hip: a workgroup = 128 pixels, a lane = one pixel that holds
//      its q and dO rows in registers, the keys walked in tiles of 32 through LDS.  Both S and dP are MFMA tiles with rows = keys
//      and columns = pixels, so the softmax statistics are in-lane.  Pass 1: running maximum, sum and sum(e * dP) -> (m, 1/l, D)
//      per pixel into the workspace.  Pass 2 (only when dq is wanted): the tiles again, dS in registers IS the B operand of
//      dq^T += khat_tile^T . dS (the P.V trick of the forward);
//   3. anab_bwd_key_kernel, KEY-major: the same body with pixels and keys swapped.  A lane = one key that holds its khat (and
//      vhat) row, a workgroup = 128 keys x a chunk of up to 512 pixels walked in tiles of 32; S^T and dP^T have rows = pixels and
//      columns = keys, P / dS come from the per-pixel statistics of step 2, and they are the B operands of
//      dkhat^T += q_tile^T . dS (ROLE 0) and dvhat^T += dO_tile^T . P (ROLE 1, 128 value channels per workgroup).  Each chunk
//      writes its partial [352][C];
//   4. anab_bwd_reduce_kernel adds the chunk partials in chunk order and divides by the bin area;
//   5. anab_bwd_gather_kernel, one wave per pixel: every bin that contains the pixel (index range from y, H and the scale: one
//      bin where the windows nest, two where they overlap, more where H < scale) -> dk, dv, dg.
// The logits, P, dP and dS never reach memory.  What bounds it: steps 2 and 3 compute S four times (both passes of the pixel-major
// kernel, both roles of the key-major one) and dP three times, beside dq, dkhat and dvhat once each: about 31 GMAC at B = 8,
// 48x160, Ck = 168, Cv = 128 against 6.1 for the forward, on the 256 FLOP/cycle/CU fp32 MFMA, with the tiles staged without
// overlap (load -> barrier -> multiply).
#include <stdlib.h>

#include "anab_bins.h"

#define AT_TROW (32 * 4 + 16)            // bytes per row of a transposed tile in LDS (32 tile rows + 16 pad)
#define AT_CHUNK_TILES 16                // pixel tiles of 32 per key-major workgroup

struct AnabBwdArgs {
    const float *q, *go, *khat, *vhat;   // khat [B][352][CAP], vhat [B][352][Cv]: zero outside [337][Ck] / past key 337
    float *stats;                        // [B*HW][4] = m, 1/l, D, 0
    float *gq;
    float *partK, *partV;                // [B][nch][352][CAP], [B][nch][352][Cv]
    int q_cs, go_cs, gq_cs, HW, nch, Cv, need_dq;
};

// 32 rows x C floats from global (row stride `stride` floats, 16-byte aligned pieces) into LDS: row-major (row stride C * 4 + 16
// bytes) and / or transposed ([C][AT_TROW]).  All 256 threads of the workgroup.
template <int C, bool ROWMAJOR, bool TRANS>
__device__ __forceinline__ void at_stage(const float *src, const size_t stride, unsigned char *R, unsigned char *T, const int tid)
{
    constexpr int P4 = C / 4, NP = 32 * P4;
#pragma unroll
    for (int p = 0; p < (NP + 255) / 256; ++p) {
        const int i = tid + 256 * p;
        if (i < NP) {
            const int row = i / P4, c4 = i - row * P4;
            const f32x4 x = *reinterpret_cast<const f32x4 *>(src + (size_t)row * stride + c4 * 4);
            if (ROWMAJOR) *reinterpret_cast<f32x4 *>(R + row * (C * 4 + 16) + c4 * 16) = x;
            if (TRANS) {
#pragma unroll
                for (int e = 0; e < 4; ++e) *reinterpret_cast<float *>(T + (c4 * 4 + e) * AT_TROW + row * 4) = x[e];
            }
        }
    }
}

// D[row][lane] = sum_c A[row][c] * b[lane][c]: A = the 32 rows of a row-major LDS tile, b = the lane's own row, held as
// bf[g] = b[8 g + 4 h + {0..3}] (h = lane half).  Register r of the result is row 8 (r / 4) + 4 h + r % 4, the column is lane & 31.
template <int C, int ROWBYTES>
__device__ __forceinline__ f32x16 at_rows_mm(const unsigned char *As, const f32x4 (&bf)[C / 8], const int l31, const int lh)
{
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const unsigned char *ab = As + l31 * ROWBYTES + lh * 16;
#pragma unroll
    for (int g = 0; g < C / 8; ++g) {
        const f32x4 af = *reinterpret_cast<const f32x4 *>(ab + g * 32);
#pragma unroll
        for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], bf[g][j], s, 0, 0, 0);
    }
    return s;
}

// acc[j][.][lane] += sum_t T[32 j + .][t] * w[t][lane]: T = a transposed LDS tile (rows = output channels, 32 tile rows each),
// w = the lane's register tile in the layout at_rows_mm returns -- exactly the two k of each MFMA step, no exchange.
template <int NJ>
__device__ __forceinline__ void at_acc_mm(const unsigned char *Ts, const float (&w)[16], f32x16 (&acc)[NJ], const int l31, const int lh)
{
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const unsigned char *tb = Ts + (32 * j + l31) * AT_TROW + lh * 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 tf = *reinterpret_cast<const f32x4 *>(tb + i * 32);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(tf[jj], w[4 * i + jj], acc[j], 0, 0, 0);
        }
    }
}

// ---- step 2: pixel-major ------------------------------------------------------------------------------------------------------------
template <int CA, int CB>              // key / query channels (multiple of 8), value channels
__global__ __launch_bounds__(256) void anab_bwd_pix_kernel(const AnabBwdArgs a)
{
    constexpr int CAP = (CA + 31) / 32 * 32;
    constexpr int KROW = CAP * 4 + 16, VROW = CB * 4 + 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[32 * KROW + CAP * AT_TROW + 32 * VROW];
    unsigned char *Ks = lds, *KsT = lds + 32 * KROW, *Vs = KsT + CAP * AT_TROW;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.x / (a.HW / 128);
    const size_t mq = (size_t)blockIdx.x * 128 + wave * 32 + l31;        // this lane's pixel (linear over the batch)

    f32x4 qf[CA / 8], gf[CB / 8];
    {
        const float *qp = a.q + mq * a.q_cs + 4 * lh, *gp = a.go + mq * a.go_cs + 4 * lh;
#pragma unroll
        for (int t = 0; t < CA / 8; ++t) qf[t] = *reinterpret_cast<const f32x4 *>(qp + 8 * t);
#pragma unroll
        for (int t = 0; t < CB / 8; ++t) gf[t] = *reinterpret_cast<const f32x4 *>(gp + 8 * t);
    }
    const float *kimg = a.khat + (size_t)img * AT_KPAD * CAP, *vimg = a.vhat + (size_t)img * AT_KPAD * CB;
    constexpr int T = AT_KPAD / 32;

    // ---- pass 1: m, l, sum(e * dP) -----------------------------------------------------------------------------------------------
    float m = -INFINITY, l = 0.f, dacc = 0.f;
    for (int t = 0; t < T; ++t) {
        __syncthreads();
        at_stage<CAP, true, false>(kimg + (size_t)32 * t * CAP, CAP, Ks, nullptr, tid);
        at_stage<CB, true, false>(vimg + (size_t)32 * t * CB, CB, Vs, nullptr, tid);
        __syncthreads();
        f32x16 s = at_rows_mm<CA, KROW>(Ks, qf, l31, lh);
        const f32x16 dp = at_rows_mm<CB, VROW>(Vs, gf, l31, lh);
        if (32 * t + 32 > AT_KEYS) {                              // (uniform) keys past the end count as -inf
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 32 * t + 8 * (r >> 2) + 4 * lh + (r & 3) < AT_KEYS ? s[r] : -INFINITY;
        }
        float mt = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, s[r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mn = fmaxf(m, mt);
        const float alpha = expf(m - mn);                          // 0 for the first tile
        float ls = 0.f, ds = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = expf(s[r] - mn);
            ls += e;
            ds = fmaf(e, dp[r], ds);                               // (vhat rows past the keys are zero: e = 0, dp = 0)
        }
        l = l * alpha + ls;
        dacc = dacc * alpha + ds;
        m = mn;
    }
    l += __shfl_xor(l, 32, 64);
    dacc += __shfl_xor(dacc, 32, 64);
    const float inv = 1.0f / l, D = dacc * inv;
    if (lh == 0) {
        float *sp = a.stats + mq * 4;
        sp[0] = m; sp[1] = inv; sp[2] = D; sp[3] = 0.f;
    }
    if (!a.need_dq) return;                                        // (uniform)

    // ---- pass 2: dq^T += khat_tile^T . dS ---------------------------------------------------------------------------------------
    f32x16 acc[CAP / 32];
#pragma unroll
    for (int j = 0; j < CAP / 32; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    for (int t = 0; t < T; ++t) {
        __syncthreads();
        at_stage<CAP, true, true>(kimg + (size_t)32 * t * CAP, CAP, Ks, KsT, tid);
        at_stage<CB, true, false>(vimg + (size_t)32 * t * CB, CB, Vs, nullptr, tid);
        __syncthreads();
        const f32x16 s = at_rows_mm<CA, KROW>(Ks, qf, l31, lh);
        const f32x16 dp = at_rows_mm<CB, VROW>(Vs, gf, l31, lh);
        float w[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool valid = 32 * t + 8 * (r >> 2) + 4 * lh + (r & 3) < AT_KEYS;
            const float p = valid ? expf(s[r] - m) * inv : 0.f;
            w[r] = p * (dp[r] - D);
        }
        at_acc_mm<CAP / 32>(KsT, w, acc, l31, lh);
    }
    float *op = a.gq + mq * a.gq_cs;
#pragma unroll
    for (int j = 0; j < CAP / 32; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 32 * j + 8 * i + 4 * lh;                 // channels past Ck are not ours
            if (c < CA) {
#pragma unroll
                for (int e = 0; e < 4; ++e) op[c + e] = acc[j][4 * i + e];
            }
        }
}

// ---- step 3: key-major --------------------------------------------------------------------------------------------------------------
// grid = (3 key blocks of 128 [x Cv / 128 value slices for ROLE 1], pixel chunks, images).  ROLE 0: dkhat, ROLE 1: dvhat.
template <int CA, int CB, int ROLE>
__global__ __launch_bounds__(256) void anab_bwd_key_kernel(const AnabBwdArgs a)
{
    constexpr int CAP = (CA + 31) / 32 * 32;
    constexpr int QROW = CA * 4 + 16, GROW = CB * 4 + 16;
    constexpr int NJ = ROLE == 0 ? CAP / 32 : 4;
    // ROLE 0: Qs, QsT [CAP], Gs (all value channels, row-major).  ROLE 1: Qs, GsT [128] (this workgroup's value channels)
    constexpr int LDS_BYTES = 32 * QROW + (ROLE == 0 ? CAP * AT_TROW + 32 * GROW : 128 * AT_TROW) + 32 * 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    unsigned char *Qs = lds, *Ts = lds + 32 * QROW;               // Ts: QsT (ROLE 0) or GsT (ROLE 1)
    unsigned char *Gs = Ts + CAP * AT_TROW;                        // (ROLE 0 only)
    unsigned char *St = lds + LDS_BYTES - 32 * 16;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kb = ROLE == 0 ? (int)blockIdx.x : (int)blockIdx.x % 3;
    const int cv0 = ROLE == 0 ? 0 : ((int)blockIdx.x / 3) * 128;
    const int ch = blockIdx.y, img = blockIdx.z;
    const bool active = kb * 128 + wave * 32 < AT_KPAD;           // (wave-uniform) the last block has three waves of keys
    const int key = kb * 128 + wave * 32 + l31;
    const int keyc = min(key, AT_KPAD - 1);

    f32x4 kf[CA / 8], vf[ROLE == 0 ? CB / 8 : 1];
    {
        const float *kp = a.khat + ((size_t)img * AT_KPAD + keyc) * CAP + 4 * lh;
#pragma unroll
        for (int t = 0; t < CA / 8; ++t) kf[t] = *reinterpret_cast<const f32x4 *>(kp + 8 * t);
        if constexpr (ROLE == 0) {
            const float *vp = a.vhat + ((size_t)img * AT_KPAD + keyc) * CB + 4 * lh;
#pragma unroll
            for (int t = 0; t < CB / 8; ++t) vf[t] = *reinterpret_cast<const f32x4 *>(vp + 8 * t);
        }
    }
    if (ROLE == 0 && CAP > CA)                                     // rows of q^T past Ck: never staged, their products never stored
        for (int i = tid; i < (CAP - CA) * (AT_TROW / 4); i += 256) reinterpret_cast<float *>(Ts + CA * AT_TROW)[i] = 0.f;

    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int pt0 = ch * AT_CHUNK_TILES, pt1 = min(pt0 + AT_CHUNK_TILES, a.HW / 32);
    for (int pt = pt0; pt < pt1; ++pt) {
        const size_t p0 = (size_t)img * a.HW + (size_t)pt * 32;
        __syncthreads();
        if constexpr (ROLE == 0) {
            at_stage<CA, true, true>(a.q + p0 * a.q_cs, a.q_cs, Qs, Ts, tid);
            at_stage<CB, true, false>(a.go + p0 * a.go_cs, a.go_cs, Gs, nullptr, tid);
        } else {
            at_stage<CA, true, false>(a.q + p0 * a.q_cs, a.q_cs, Qs, nullptr, tid);
            at_stage<128, false, true>(a.go + p0 * a.go_cs + cv0, a.go_cs, nullptr, Ts, tid);
        }
        if (tid < 32) *reinterpret_cast<f32x4 *>(St + tid * 16) = *reinterpret_cast<const f32x4 *>(a.stats + (p0 + tid) * 4);
        __syncthreads();
        if (active) {
            const f32x16 s = at_rows_mm<CA, QROW>(Qs, kf, l31, lh);      // rows = pixels of the tile, column = this lane's key
            float w[16];
            if constexpr (ROLE == 0) {
                const f32x16 dp = at_rows_mm<CB, GROW>(Gs, vf, l31, lh);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const f32x4 st = *reinterpret_cast<const f32x4 *>(St + (8 * (r >> 2) + 4 * lh + (r & 3)) * 16);
                    w[r] = expf(s[r] - st[0]) * st[1] * (dp[r] - st[2]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const f32x4 st = *reinterpret_cast<const f32x4 *>(St + (8 * (r >> 2) + 4 * lh + (r & 3)) * 16);
                    w[r] = expf(s[r] - st[0]) * st[1];
                }
            }
            at_acc_mm<NJ>(Ts, w, acc, l31, lh);
        }
    }
    if (!active || key >= AT_KEYS) return;                         // (a padding key's column holds whatever its zero row gave)
    const size_t prow = ((size_t)img * a.nch + ch) * AT_KPAD + key;
    float *op = ROLE == 0 ? a.partK + prow * CAP : a.partV + prow * a.Cv + cv0;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 32 * j + 8 * i + 4 * lh;
            if (ROLE == 1 || c < CA) {
#pragma unroll
                for (int e = 0; e < 4; ++e) op[c + e] = acc[j][4 * i + e];
            }
        }
}

// ---- the small kernels --------------------------------------------------------------------------------------------------------------
// The work items of m3d_anab_pool_partial for an H x W map, built on the device (what Engine._anab_items builds on the host): windows
// split into chunks of ceil(H / 16) rows x ceil(W / 4) columns.  One workgroup of 384 threads, thread = bin.
__global__ void anab_items_kernel(int *__restrict__ items, int *__restrict__ bin_scale, int *__restrict__ bin_slots,
                                  float *__restrict__ bin_inv, int H, int W)
{
    __shared__ int cnt[AT_KEYS];
    const int bin = threadIdx.x;
    const int rchunk = max(1, (H + 15) / 16), cchunk = max(1, (W + 3) / 4);
    int si = 0, sz = 1, bi = 0, bj = 0, h0 = 0, h1 = 0, w0 = 0, w1 = 0, nr = 0, nc = 0;
    if (bin < AT_KEYS) {
        at_bin_pos(bin, si, sz, bi, bj);
        h0 = at_win_lo(bi, H, sz); h1 = at_win_hi(bi, H, sz);
        w0 = at_win_lo(bj, W, sz); w1 = at_win_hi(bj, W, sz);
        nr = (h1 - h0 + rchunk - 1) / rchunk;
        nc = (w1 - w0 + cchunk - 1) / cchunk;
        cnt[bin] = nr * nc;
    }
    __syncthreads();
    if (bin >= AT_KEYS) return;
    int first = 0;
    for (int b = 0; b < bin; ++b) first += cnt[b];
    bin_scale[bin] = si;
    bin_slots[bin] = nr * nc;
    bin_inv[bin] = 1.0f / (float)((h1 - h0) * (w1 - w0));
    for (int r = 0; r < nr; ++r)
        for (int c = 0; c < nc; ++c) {
            int *it = items + (size_t)(first + r * nc + c) * 6;
            it[0] = bin;
            it[1] = h0 + r * rchunk; it[2] = min(h0 + (r + 1) * rchunk, h1);
            it[3] = w0 + c * cchunk; it[4] = min(w0 + (c + 1) * cchunk, w1);
            it[5] = r * nc + c;
        }
}

// vhat [B][352][Cv] from vhat^T [B][Cv][352]; rows past the keys zero
__global__ void anab_vhat_rows_kernel(const float *__restrict__ vhatT, float *__restrict__ vhat, int Cv, long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int cv = (int)(i % Cv);
    const long long bk = i / Cv;
    const int key = (int)(bk % AT_KPAD);
    const long long b = bk / AT_KPAD;
    vhat[i] = key < AT_KEYS ? vhatT[(b * Cv + cv) * AT_KPAD + key] : 0.f;
}

struct AnabGatherArgs {
    const float *k, *v, *g, *dkv;
    float *gk, *gv, *gg;
    int k_cs, v_cs, g_cs, gk_cs, gv_cs, gg_cs, H, W, Ck, Cv, do_k, do_v;
    long long pixels;
};

// One wave per pixel; lane = channel (strided by 64) of K|V.  For each scale the bins [i_lo, i_hi] x [j_lo, j_hi] that contain the
// pixel: i_lo = floor(y s / H), i_hi = ceil((y + 1) s / H) - 1 (every i with floor(i H / s) <= y < ceil((i + 1) H / s)).
__global__ __launch_bounds__(256) void anab_bwd_gather_kernel(const AnabGatherArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.pixels) return;                                     // (wave-uniform)
    const int HW = a.H * a.W;
    const long long b = p / HW;
    const int pix = (int)(p - b * HW), y = pix / a.W, x = pix - y * a.W;
    const int C = a.Ck + a.Cv;
    const float *dimg = a.dkv + (size_t)b * AT_KEYS * C;
    float gate[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) gate[s] = a.g[(size_t)p * a.g_cs + s];
    float dgs[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < C; c += 64) {
        const bool isk = c < a.Ck;
        if (isk ? !a.do_k : !a.do_v) continue;
        const float xv = a.gg ? (isk ? a.k[(size_t)p * a.k_cs + c] : a.v[(size_t)p * a.v_cs + (c - a.Ck)]) : 0.f;
        float o = 0.f;
        int base = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int sz = s == 0 ? 1 : (s == 1 ? 4 : (s == 2 ? 8 : 16));
            const int i0 = (y * sz) / a.H, i1 = ((y + 1) * sz + a.H - 1) / a.H - 1;
            const int j0 = (x * sz) / a.W, j1 = ((x + 1) * sz + a.W - 1) / a.W - 1;
            float t = 0.f;
            for (int i = i0; i <= i1; ++i)
                for (int j = j0; j <= j1; ++j) t += dimg[(size_t)(base + i * sz + j) * C + c];
            o = fmaf(gate[s], t, o);
            dgs[s] = fmaf(xv, t, dgs[s]);
            base += sz * sz;
        }
        if (isk) { if (a.gk) a.gk[(size_t)p * a.gk_cs + c] = o; }
        else if (a.gv) a.gv[(size_t)p * a.gv_cs + (c - a.Ck)] = o;
    }
    if (!a.gg) return;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float t = dgs[s];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
        if (lane == s) a.gg[(size_t)p * a.gg_cs + s] = t;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static bool at_supported(int B, int H, int W, int Ck, int Cv)
{
    if (B < 1 || H < 1 || W < 1) return false;
    const long long HW = (long long)H * W;
    if (HW % 128 != 0 || (long long)B * HW >= 0x7FFFFFFFLL / 4 || H > 32768 || W > 32768) return false;
    return (Cv == 128 && (Ck == 64 || Ck == 128 || Ck == 168)) || (Cv == 256 && Ck == 168);
}

struct AtLayout {                        // offsets in floats into the 256-byte aligned workspace
    int nested, n_items, max_slots, nch, CAP;
    long long khat, vhatT, scratch, items, bin_scale, bin_slots, bin_inv, fwd_end;
    long long vhat, stats, partK, partV, dkv, bwd_end;
};

static long long at_up(long long x) { return (x + 63) / 64 * 64; }

static AtLayout at_layout(int B, int H, int W, int Ck, int Cv)
{
    AtLayout L;
    const long long HW = (long long)H * W;
    L.CAP = (Ck + 31) / 32 * 32;
    L.nested = H % 16 == 0 && W % 16 == 0;
    L.n_items = 0;
    L.max_slots = 1;
    const int rchunk = std::max(1, (H + 15) / 16), cchunk = std::max(1, (W + 3) / 4);
    const int sizes[4] = {1, 4, 8, 16};
    for (int si = 0; si < 4; ++si)
        for (int i = 0; i < sizes[si]; ++i)
            for (int j = 0; j < sizes[si]; ++j) {
                const int hh = at_win_hi(i, H, sizes[si]) - at_win_lo(i, H, sizes[si]);
                const int ww = at_win_hi(j, W, sizes[si]) - at_win_lo(j, W, sizes[si]);
                const int n = ((hh + rchunk - 1) / rchunk) * ((ww + cchunk - 1) / cchunk);
                L.n_items += n;
                L.max_slots = std::max(L.max_slots, n);
            }
    const int Cmax = std::max(Ck, Cv);
    long long o = 0;
    L.khat = o; o += at_up((long long)B * AT_KPAD * L.CAP);
    L.vhatT = o; o += at_up((long long)B * Cv * AT_KPAD);
    L.scratch = o;
    o += at_up(L.nested ? (long long)B * 256 * 4 * Cmax : (long long)B * AT_KEYS * L.max_slots * Cmax);
    L.items = o; o += at_up((long long)L.n_items * 6);
    L.bin_scale = o; o += at_up(AT_KEYS);
    L.bin_slots = o; o += at_up(AT_KEYS);
    L.bin_inv = o; o += at_up(AT_KEYS);
    L.fwd_end = o;
    L.nch = (int)((HW / 32 + AT_CHUNK_TILES - 1) / AT_CHUNK_TILES);
    L.vhat = o; o += at_up((long long)B * AT_KPAD * Cv);
    L.stats = o; o += at_up((long long)B * HW * 4);
    L.partK = o; o += at_up((long long)B * L.nch * AT_KPAD * L.CAP);
    L.partV = o; o += at_up((long long)B * L.nch * AT_KPAD * Cv);
    L.dkv = o; o += at_up((long long)B * AT_KEYS * (Ck + Cv));
    L.bwd_end = o;
    return L;
}

extern "C" long long m3d_anab_attention_workspace_bytes(int B, int H, int W, int Ck, int Cv, int backward)
{
    if (!at_supported(B, H, W, Ck, Cv)) return -1;
    const AtLayout L = at_layout(B, H, W, Ck, Cv);
    return (backward ? L.bwd_end : L.fwd_end) * 4;
}

static int at_check(const char *name, int B, int H, int W, int Ck, int Cv, const void *workspace, long long workspace_bytes, int backward)
{
    M3D_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: B, H, W must be positive", name);
    M3D_REQUIRE(((long long)H * W) % 128 == 0, "%s: H*W must be a multiple of 128 (HW %% 128 == 0; got %dx%d)", name, H, W);
    M3D_REQUIRE((Cv == 128 && (Ck == 64 || Ck == 128 || Ck == 168)) || (Cv == 256 && Ck == 168),
                "%s: built for (Ck, Cv) in {(64, 128), (128, 128), (168, 128), (168, 256)} (got %d, %d)", name, Ck, Cv);
    M3D_REQUIRE(at_supported(B, H, W, Ck, Cv), "%s: too many pixels", name);
    M3D_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", name);
    const long long need = m3d_anab_attention_workspace_bytes(B, H, W, Ck, Cv, backward);
    if (workspace_bytes < need) {
        m3d_set_error("%s: workspace %lld < %lld bytes (m3d_anab_attention_workspace_bytes)", name, workspace_bytes, need);
        return M3D_E_WORKSPACE;
    }
    return M3D_OK;
}

// khat [B][352][CAP] (zero outside [337][Ck]) and vhat^T [B][Cv][352] into the workspace through the engine's pooling launches: K
// and V are separate views here, so each is pooled on its own (a channel's sums do not depend on the other channels: the same bits)
static int at_pool(const AtLayout &L, float *ws, const float *k, int k_cs, const float *v, int v_cs, const float *g, int g_cs, int B,
                   int H, int W, int Ck, int Cv, bool zero_khat, m3d_stream_t stream)
{
    const hipStream_t st = (hipStream_t)stream;
    float *khat = ws + L.khat, *vhatT = ws + L.vhatT, *scratch = ws + L.scratch;
    if (zero_khat) M3D_HIP(hipMemsetAsync(khat, 0, (size_t)B * AT_KPAD * L.CAP * 4, st));
    if (L.nested) {
        int rc = m3d_anab_pool_nested(k, k_cs, g, g_cs, B, H, W, Ck, 0, scratch, khat, AT_KPAD, L.CAP, vhatT, 0, stream);
        if (rc != M3D_OK) return rc;
        return m3d_anab_pool_nested(v, v_cs, g, g_cs, B, H, W, 0, Cv, scratch, khat, AT_KPAD, L.CAP, vhatT, 0, stream);
    }
    int *items = reinterpret_cast<int *>(ws + L.items), *bscale = reinterpret_cast<int *>(ws + L.bin_scale);
    int *bslots = reinterpret_cast<int *>(ws + L.bin_slots);
    float *binv = ws + L.bin_inv;
    hipLaunchKernelGGL(anab_items_kernel, dim3(1), dim3(384), 0, st, items, bscale, bslots, binv, H, W);
    M3D_LAUNCH_CHECK();
    int rc = m3d_anab_pool_partial(k, k_cs, g, g_cs, items, L.n_items, bscale, AT_KEYS, scratch, L.max_slots, B, H, W, Ck, stream);
    if (rc != M3D_OK) return rc;
    rc = m3d_anab_pool_finish(scratch, bslots, binv, AT_KEYS, L.max_slots, Ck, 0, khat, AT_KPAD, L.CAP, vhatT, B, 0, stream);
    if (rc != M3D_OK) return rc;
    rc = m3d_anab_pool_partial(v, v_cs, g, g_cs, items, L.n_items, bscale, AT_KEYS, scratch, L.max_slots, B, H, W, Cv, stream);
    if (rc != M3D_OK) return rc;
    return m3d_anab_pool_finish(scratch, bslots, binv, AT_KEYS, L.max_slots, 0, Cv, khat, AT_KPAD, L.CAP, vhatT, B, 0, stream);
}

extern "C" int m3d_anab_attention_forward(const float *q, const float *k, const float *v, const float *g, float *out, int B, int H, int W,
                                          int Ck, int Cv, int q_cs, int k_cs, int v_cs, int g_cs, int out_cs, void *workspace,
                                          long long workspace_bytes, m3d_stream_t stream)
{
    M3D_REQUIRE(q && k && v && g && out, "anab_attention_forward: null pointer");
    int rc = at_check("anab_attention_forward", B, H, W, Ck, Cv, workspace, workspace_bytes, 0);
    if (rc != M3D_OK) return rc;
    M3D_REQUIRE(k_cs >= Ck && v_cs >= Cv && g_cs >= 4 && out_cs >= Cv, "anab_attention_forward: a row stride is below its channel count");
    const AtLayout L = at_layout(B, H, W, Ck, Cv);
    float *ws = static_cast<float *>(workspace);
    rc = at_pool(L, ws, k, k_cs, v, v_cs, g, g_cs, B, H, W, Ck, Cv, false, stream);
    if (rc != M3D_OK) return rc;
    return m3d_anab_attend_f32(q, q_cs, ws + L.khat, L.CAP, ws + L.vhatT, B, H * W, Ck, AT_KEYS, AT_KPAD, Cv, nullptr, 0, 0, nullptr,
                               nullptr, 0, out, out_cs, stream);
}

template <int CA, int CB>
static void at_launch_main(const AnabBwdArgs &a, int B, bool do_k, bool do_v, hipStream_t st)
{
    hipLaunchKernelGGL((anab_bwd_pix_kernel<CA, CB>), dim3(B * (a.HW / 128)), dim3(256), 0, st, a);
    if (do_k) hipLaunchKernelGGL((anab_bwd_key_kernel<CA, CB, 0>), dim3(3, a.nch, B), dim3(256), 0, st, a);
    if (do_v) hipLaunchKernelGGL((anab_bwd_key_kernel<CA, CB, 1>), dim3(3 * (CB / 128), a.nch, B), dim3(256), 0, st, a);
}

extern "C" int m3d_anab_attention_backward(const float *q, const float *k, const float *v, const float *g, const float *grad_out,
                                           float *grad_q, float *grad_k, float *grad_v, float *grad_g, int B, int H, int W, int Ck,
                                           int Cv, int q_cs, int k_cs, int v_cs, int g_cs, int go_cs, int gq_cs, int gk_cs, int gv_cs,
                                           int gg_cs, void *workspace, long long workspace_bytes, m3d_stream_t stream)
{
    M3D_REQUIRE(q && k && v && g && grad_out, "anab_attention_backward: null pointer");
    int rc = at_check("anab_attention_backward", B, H, W, Ck, Cv, workspace, workspace_bytes, 1);
    if (rc != M3D_OK) return rc;
    M3D_REQUIRE(q_cs >= Ck && k_cs >= Ck && v_cs >= Cv && g_cs >= 4 && go_cs >= Cv, "anab_attention_backward: a row stride is below its channel count");
    M3D_REQUIRE((!grad_q || gq_cs >= Ck) && (!grad_k || gk_cs >= Ck) && (!grad_v || gv_cs >= Cv) && (!grad_g || gg_cs >= 4),
                "anab_attention_backward: a gradient's row stride is below its channel count");
    M3D_REQUIRE(q_cs % 4 == 0 && go_cs % 4 == 0 && (((uintptr_t)q | (uintptr_t)grad_out) & 15) == 0,
                "anab_attention_backward: q and grad_out must be 16-byte aligned views with row strides that are multiples of 4 floats");
    if (!grad_q && !grad_k && !grad_v && !grad_g) return M3D_OK;
    const hipStream_t st = (hipStream_t)stream;
    const AtLayout L = at_layout(B, H, W, Ck, Cv);
    float *ws = static_cast<float *>(workspace);
    const int HW = H * W;
    rc = at_pool(L, ws, k, k_cs, v, v_cs, g, g_cs, B, H, W, Ck, Cv, true, stream);
    if (rc != M3D_OK) return rc;
    {
        const long long total = (long long)B * AT_KPAD * Cv;
        hipLaunchKernelGGL(anab_vhat_rows_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, ws + L.vhatT, ws + L.vhat, Cv, total);
        M3D_LAUNCH_CHECK();
    }
    // dkhat feeds grad_k and grad_g, dvhat feeds grad_v and grad_g; the statistics of the pixel-major kernel feed both
    const bool do_k = grad_k || grad_g, do_v = grad_v || grad_g;
    AnabBwdArgs a;
    a.q = q; a.go = grad_out; a.khat = ws + L.khat; a.vhat = ws + L.vhat; a.stats = ws + L.stats; a.gq = grad_q;
    a.partK = ws + L.partK; a.partV = ws + L.partV;
    a.q_cs = q_cs; a.go_cs = go_cs; a.gq_cs = gq_cs; a.HW = HW; a.nch = L.nch; a.Cv = Cv; a.need_dq = grad_q ? 1 : 0;
    if (Cv == 256) at_launch_main<168, 256>(a, B, do_k, do_v, st);
    else if (Ck == 168) at_launch_main<168, 128>(a, B, do_k, do_v, st);
    else if (Ck == 128) at_launch_main<128, 128>(a, B, do_k, do_v, st);
    else at_launch_main<64, 128>(a, B, do_k, do_v, st);
    M3D_LAUNCH_CHECK();
    if (!do_k && !do_v) return M3D_OK;
    {
        const long long total = (long long)B * AT_KEYS * (Ck + Cv);
        hipLaunchKernelGGL(anab_bwd_reduce_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, a.partK, a.partV, ws + L.dkv, L.nch, L.CAP, Ck,
                           Cv, H, W, do_k ? 1 : 0, do_v ? 1 : 0, total);
        M3D_LAUNCH_CHECK();
    }
    AnabGatherArgs ga;
    ga.k = k; ga.v = v; ga.g = g; ga.dkv = ws + L.dkv; ga.gk = grad_k; ga.gv = grad_v; ga.gg = grad_g;
    ga.k_cs = k_cs; ga.v_cs = v_cs; ga.g_cs = g_cs; ga.gk_cs = gk_cs; ga.gv_cs = gv_cs; ga.gg_cs = gg_cs;
    ga.H = H; ga.W = W; ga.Ck = Ck; ga.Cv = Cv; ga.do_k = do_k ? 1 : 0; ga.do_v = do_v ? 1 : 0;
    ga.pixels = (long long)B * HW;
    hipLaunchKernelGGL(anab_bwd_gather_kernel, dim3(cdiv(ga.pixels, 4)), dim3(256), 0, st, ga);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}
