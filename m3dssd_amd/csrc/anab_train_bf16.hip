// The ANAB attention core for training with bf16 tensors (the second compute type of csrc/anab_train.hip, for
// torch.autocast(bfloat16)): the same mathematics, bin rule and launch structure, every product on v_mfma_f32_32x32x16_bf16.
//     khat[b] = mean_{p in win_b} g[p][scale(b)] k[p],  vhat likewise,  S = q khat^T,  P = softmax_keys(S),  O = P vhat
//     dvhat = P^T dO,  dP = dO vhat^T,  D = rowsum(P * dP),  dS = P * (dP - D),  dq = dS khat,  dkhat = dS^T q,  then the gather.
// Rounding points (the contract of include/m3dssd_hip.h): pooling sums, softmax statistics and every accumulator are fp32; khat /
// vhat are rounded once to bf16 (the MFMA operands); S and dP are never rounded; P is rounded once as the operand of P.vhat (the
// unnormalised exponential, 1/l applied to the fp32 accumulator) and of P^T.dO (normalised); dS is rounded once as the operand of dq
// and dkhat; dkhat / dvhat, their chunk sums and the gather stay fp32; every output is rounded once.  1/l is an IEEE division.
//
// Launches (one stream, nothing atomic, every sum in a fixed order):
//   1. anab16_pool_kernel: one workgroup per (bin, image, 128-channel slab), 16 waves that each walk every 16th pixel of the window
//      in window order, partial sums added in wave order -> khat [352][CAP], khat^T [CAP][352], vhat [352][Cv], vhat^T [Cv][352],
//      bf16, in the zeroed workspace.  Serves nested and overlapping windows alike;
//   2. forward: anab16_fwd_kernel, pixel-major (a lane = one pixel that holds its q row as MFMA B fragments), keys in tiles of 32
//      through LDS, one pass with a running maximum.  S has rows = keys and columns = pixels, so exp(S - m) in registers IS the B
//      operand of O^T += vhat_tile^T . P (the k order of an accumulator used as an operand: keys 16u + 8(j >> 2) + 4h + (j & 3), and
//      the A fragment of vhat^T is fetched in that order);
//   3. backward: anab16_pix_kernel (statistics m, 1/l, D; then dq^T += khat_tile^T . dS), anab16_key_kernel (the same body with
//      pixels and keys swapped: dkhat^T += q_tile^T . dS, dvhat^T += dO_tile^T . P, per chunk of 512 pixels), anab_bwd_reduce_kernel
//      (chunk partials in chunk order, / area), anab16_gather_kernel (one wave per pixel, every bin that contains it).
#include <stdlib.h>

#include "anab_bins.h"
#include "bf16_tile.h"

#define AB_TROW (32 * 2 + 16)            // bytes per row of a transposed tile in LDS (32 tile rows + 16 pad)
#define AB_CHUNK_TILES 16                // pixel tiles of 32 per key-major workgroup
#define AB_POOL_WAVES 16

typedef unsigned short bf16_t;

__device__ __forceinline__ float ab_f(bf16_t x) { return __uint_as_float((unsigned)x << 16); }
__device__ __forceinline__ bf16_t ab_r(float x) { return (bf16_t)(pack_bf16(x, 0.f) & 0xFFFFu); }

struct Anab16Args {
    const bf16_t *q, *go;
    const bf16_t *khat, *khatT, *vhat, *vhatT;   // [B][352][CAP], [B][CAP][352], [B][352][Cv], [B][Cv][352]: zero outside [337][C]
    float *stats;                        // [B*HW][4] = m, 1/l, D, 0
    bf16_t *gq, *out;
    float *partK, *partV;                // [B][nch][352][CAP], [B][nch][352][Cv]
    int q_cs, go_cs, gq_cs, out_cs, HW, nch, Cv, need_dq;
};

// 32 rows x C bf16 (channels [CV, C) as zeros, never read) from global (row stride `stride` elements, 16-byte aligned pieces) into
// LDS: row-major (row stride C * 2 + 16 bytes) and / or transposed ([C][AB_TROW]).  All 256 threads of the workgroup.
template <int C, int CV, bool ROWMAJOR, bool TRANS>
__device__ __forceinline__ void ab_stage(const bf16_t *src, const size_t stride, unsigned char *R, unsigned char *T, const int tid)
{
    constexpr int P8 = C / 8, NP = 32 * P8;
#pragma unroll
    for (int p = 0; p < (NP + 255) / 256; ++p) {
        const int i = tid + 256 * p;
        if (i < NP) {
            const int row = i / P8, c8 = i - row * P8;
            u32x4 x = {0u, 0u, 0u, 0u};
            if (c8 * 8 < CV) x = *reinterpret_cast<const u32x4 *>(src + (size_t)row * stride + c8 * 8);
            if (ROWMAJOR) *reinterpret_cast<u32x4 *>(R + row * (C * 2 + 16) + c8 * 16) = x;
            if (TRANS) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    *reinterpret_cast<bf16_t *>(T + (c8 * 8 + e) * AB_TROW + row * 2) = (bf16_t)(x[e >> 1] >> (16 * (e & 1)));
            }
        }
    }
}

// NR rows of a [.][352] workspace matrix, columns 32 t .. 32 t + 31 -> the transposed LDS tile [NR][AB_TROW]
template <int NR>
__device__ __forceinline__ void ab_stage_cols(const bf16_t *src, unsigned char *T, const int tid)
{
#pragma unroll
    for (int p = 0; p < (NR * 4 + 255) / 256; ++p) {
        const int i = tid + 256 * p;
        if (i < NR * 4) {
            const int row = i >> 2, pc = i & 3;
            *reinterpret_cast<u32x4 *>(T + row * AB_TROW + pc * 16) = *reinterpret_cast<const u32x4 *>(src + (size_t)row * AT_KPAD + pc * 8);
        }
    }
}

// The lane's own row as B fragments: bf[g] = row[16 g + 8 h + (0..7)], zero from channel C on
template <int C>
__device__ __forceinline__ void ab_own_row(const bf16_t *row, bf16x8 (&bf)[(C + 15) / 16], const int lh)
{
#pragma unroll
    for (int g = 0; g < (C + 15) / 16; ++g) {
        u32x4 x = {0u, 0u, 0u, 0u};
        if (16 * g + 8 < C || lh == 0) x = *reinterpret_cast<const u32x4 *>(row + 16 * g + 8 * lh);
        bf[g] = __builtin_bit_cast(bf16x8, x);
    }
}

// D[row][lane] = sum_c A[row][c] * b[lane][c]: A = the 32 rows of a row-major LDS tile, b = the lane's own row (ab_own_row).
// Register r of the result is row 8 (r / 4) + 4 h + r % 4, the column is lane & 31.
template <int NG, int ROWBYTES>
__device__ __forceinline__ f32x16 ab_rows_mm(const unsigned char *As, const bf16x8 (&bf)[NG], const int l31, const int lh)
{
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const unsigned char *ab = As + l31 * ROWBYTES + lh * 16;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const bf16x8 af = *reinterpret_cast<const bf16x8 *>(ab + g * 32);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf[g], s, 0, 0, 0);
    }
    return s;
}

// acc[j][.][lane] += sum_t T[32 j + .][t] * bf16(w[t][lane]): T = a transposed LDS tile (rows = output channels, 32 tile rows each),
// w = the lane's register tile in the layout ab_rows_mm returns.  Registers 8u .. 8u + 7 are the B fragment of k-step u; its
// element j of lane half h is tile row 16u + 8 (j >> 2) + 4h + (j & 3), and the A fragment is read from T in that same order.
template <int NJ>
__device__ __forceinline__ void ab_acc_mm(const unsigned char *Ts, const float (&w)[16], f32x16 (&acc)[NJ], const int l31, const int lh)
{
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        u32x4 pb;
#pragma unroll
        for (int i = 0; i < 4; ++i) pb[i] = pack_bf16(w[8 * u + 2 * i], w[8 * u + 2 * i + 1]);
        const bf16x8 pf = __builtin_bit_cast(bf16x8, pb);
        const unsigned char *tb = Ts + l31 * AB_TROW + (16 * u + 4 * lh) * 2;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const u32x2 lo = *reinterpret_cast<const u32x2 *>(tb + j * 32 * AB_TROW);
            const u32x2 hi = *reinterpret_cast<const u32x2 *>(tb + j * 32 * AB_TROW + 16);
            const u32x4 tw = {lo[0], lo[1], hi[0], hi[1]};
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, tw), pf, acc[j], 0, 0, 0);
        }
    }
}

// 4 consecutive channels of one row, rounded once
__device__ __forceinline__ void ab_store4(bf16_t *p, const float a, const float b, const float c, const float d, const bool al8)
{
    if (al8) {
        const u32x2 w = {pack_bf16(a, b), pack_bf16(c, d)};
        *reinterpret_cast<u32x2 *>(p) = w;
    } else {
        p[0] = ab_r(a); p[1] = ab_r(b); p[2] = ab_r(c); p[3] = ab_r(d);
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// grid = (pixel tiles of 128 over the batch, Cv / 128 value slices)
template <int CA>
__global__ __launch_bounds__(256) void anab16_fwd_kernel(const Anab16Args a)
{
    constexpr int CAP = (CA + 31) / 32 * 32, NG = (CA + 15) / 16;
    constexpr int KROW = CAP * 2 + 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[32 * KROW + 128 * AB_TROW];
    unsigned char *Ks = lds, *VsT = lds + 32 * KROW;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.x / (a.HW / 128), cv0 = blockIdx.y * 128;
    const size_t mq = (size_t)blockIdx.x * 128 + wave * 32 + l31;        // this lane's pixel (linear over the batch)

    bf16x8 qf[NG];
    ab_own_row<CA>(a.q + mq * a.q_cs, qf, lh);
    const bf16_t *kimg = a.khat + (size_t)img * AT_KPAD * CAP, *vimg = a.vhatT + ((size_t)img * a.Cv + cv0) * AT_KPAD;

    f32x16 o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[j][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int t = 0; t < AT_KPAD / 32; ++t) {
        __syncthreads();
        ab_stage<CAP, CAP, true, false>(kimg + (size_t)32 * t * CAP, CAP, Ks, nullptr, tid);
        ab_stage_cols<128>(vimg + 32 * t, VsT, tid);
        __syncthreads();
        f32x16 s = ab_rows_mm<NG, KROW>(Ks, qf, l31, lh);
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
        float e[16], ls = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            e[r] = expf(s[r] - mn);
            ls += e[r];
        }
        l = l * alpha + ls;
        m = mn;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] *= alpha;
        ab_acc_mm<4>(VsT, e, o, l31, lh);
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    bf16_t *op = a.out + mq * a.out_cs + cv0;
    const bool al8 = (((uintptr_t)a.out & 7) | (a.out_cs & 3)) == 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            ab_store4(op + 32 * j + 8 * i + 4 * lh, o[j][4 * i] * inv, o[j][4 * i + 1] * inv, o[j][4 * i + 2] * inv, o[j][4 * i + 3] * inv, al8);
}

// ---- backward, pixel-major: statistics and dq -----------------------------------------------------------------------------------------
template <int CA, int CB>
__global__ __launch_bounds__(256) void anab16_pix_kernel(const Anab16Args a)
{
    constexpr int CAP = (CA + 31) / 32 * 32, NG = (CA + 15) / 16;
    constexpr int KROW = CAP * 2 + 16, VROW = CB * 2 + 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[32 * KROW + CAP * AB_TROW + 32 * VROW];
    unsigned char *Ks = lds, *KsT = lds + 32 * KROW, *Vs = KsT + CAP * AB_TROW;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.x / (a.HW / 128);
    const size_t mq = (size_t)blockIdx.x * 128 + wave * 32 + l31;

    bf16x8 qf[NG], gf[CB / 16];
    ab_own_row<CA>(a.q + mq * a.q_cs, qf, lh);
    ab_own_row<CB>(a.go + mq * a.go_cs, gf, lh);
    const bf16_t *kimg = a.khat + (size_t)img * AT_KPAD * CAP, *vimg = a.vhat + (size_t)img * AT_KPAD * CB;
    const bf16_t *ktimg = a.khatT + (size_t)img * CAP * AT_KPAD;
    constexpr int T = AT_KPAD / 32;

    // ---- pass 1: m, l, sum(e * dP) -----------------------------------------------------------------------------------------------
    float m = -INFINITY, l = 0.f, dacc = 0.f;
    for (int t = 0; t < T; ++t) {
        __syncthreads();
        ab_stage<CAP, CAP, true, false>(kimg + (size_t)32 * t * CAP, CAP, Ks, nullptr, tid);
        ab_stage<CB, CB, true, false>(vimg + (size_t)32 * t * CB, CB, Vs, nullptr, tid);
        __syncthreads();
        f32x16 s = ab_rows_mm<NG, KROW>(Ks, qf, l31, lh);
        const f32x16 dp = ab_rows_mm<CB / 16, VROW>(Vs, gf, l31, lh);
        if (32 * t + 32 > AT_KEYS) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 32 * t + 8 * (r >> 2) + 4 * lh + (r & 3) < AT_KEYS ? s[r] : -INFINITY;
        }
        float mt = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, s[r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mn = fmaxf(m, mt);
        const float alpha = expf(m - mn);
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
        ab_stage<CAP, CAP, true, false>(kimg + (size_t)32 * t * CAP, CAP, Ks, nullptr, tid);
        ab_stage_cols<CAP>(ktimg + 32 * t, KsT, tid);
        ab_stage<CB, CB, true, false>(vimg + (size_t)32 * t * CB, CB, Vs, nullptr, tid);
        __syncthreads();
        const f32x16 s = ab_rows_mm<NG, KROW>(Ks, qf, l31, lh);
        const f32x16 dp = ab_rows_mm<CB / 16, VROW>(Vs, gf, l31, lh);
        float w[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool valid = 32 * t + 8 * (r >> 2) + 4 * lh + (r & 3) < AT_KEYS;
            const float p = valid ? expf(s[r] - m) * inv : 0.f;
            w[r] = p * (dp[r] - D);
        }
        ab_acc_mm<CAP / 32>(KsT, w, acc, l31, lh);
    }
    bf16_t *op = a.gq + mq * a.gq_cs;
    const bool al8 = (((uintptr_t)a.gq & 7) | (a.gq_cs & 3)) == 0;
#pragma unroll
    for (int j = 0; j < CAP / 32; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 32 * j + 8 * i + 4 * lh;                 // channels past Ck are not ours
            if (c < CA) ab_store4(op + c, acc[j][4 * i], acc[j][4 * i + 1], acc[j][4 * i + 2], acc[j][4 * i + 3], al8);
        }
}

// ---- backward, key-major --------------------------------------------------------------------------------------------------------------
// grid = (3 key blocks of 128 [x Cv / 128 value slices for ROLE 1], pixel chunks, images).  ROLE 0: dkhat, ROLE 1: dvhat.
template <int CA, int CB, int ROLE>
__global__ __launch_bounds__(256) void anab16_key_kernel(const Anab16Args a)
{
    constexpr int CAP = (CA + 31) / 32 * 32, NG = (CA + 15) / 16, CA16 = NG * 16;
    constexpr int QROW = CA16 * 2 + 16, GROW = CB * 2 + 16;
    constexpr int NJ = ROLE == 0 ? CAP / 32 : 4;
    // ROLE 0: Qs, QsT [CAP], Gs (all value channels, row-major).  ROLE 1: Qs, GsT [128] (this workgroup's value channels)
    constexpr int LDS_BYTES = 32 * QROW + (ROLE == 0 ? CAP * AB_TROW + 32 * GROW : 128 * AB_TROW) + 32 * 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    unsigned char *Qs = lds, *Ts = lds + 32 * QROW;               // Ts: QsT (ROLE 0) or GsT (ROLE 1)
    unsigned char *Gs = Ts + CAP * AB_TROW;                        // (ROLE 0 only)
    unsigned char *St = lds + LDS_BYTES - 32 * 16;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kb = ROLE == 0 ? (int)blockIdx.x : (int)blockIdx.x % 3;
    const int cv0 = ROLE == 0 ? 0 : ((int)blockIdx.x / 3) * 128;
    const int ch = blockIdx.y, img = blockIdx.z;
    const bool active = kb * 128 + wave * 32 < AT_KPAD;           // (wave-uniform) the last block has three waves of keys
    const int key = kb * 128 + wave * 32 + l31;
    const int keyc = min(key, AT_KPAD - 1);

    bf16x8 kf[NG], vf[ROLE == 0 ? CB / 16 : 1];
    ab_own_row<CA>(a.khat + ((size_t)img * AT_KPAD + keyc) * CAP, kf, lh);
    if constexpr (ROLE == 0) ab_own_row<CB>(a.vhat + ((size_t)img * AT_KPAD + keyc) * CB, vf, lh);
    if (ROLE == 0 && CAP > CA)                                     // rows of q^T past Ck: never staged, their products never stored
        for (int i = tid; i < (CAP - CA) * (AB_TROW / 4); i += 256) reinterpret_cast<unsigned *>(Ts + CA * AB_TROW)[i] = 0u;

    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int pt0 = ch * AB_CHUNK_TILES, pt1 = min(pt0 + AB_CHUNK_TILES, a.HW / 32);
    for (int pt = pt0; pt < pt1; ++pt) {
        const size_t p0 = (size_t)img * a.HW + (size_t)pt * 32;
        __syncthreads();
        if constexpr (ROLE == 0) {
            ab_stage<CA16, CA, true, true>(a.q + p0 * a.q_cs, a.q_cs, Qs, Ts, tid);
            ab_stage<CB, CB, true, false>(a.go + p0 * a.go_cs, a.go_cs, Gs, nullptr, tid);
        } else {
            ab_stage<CA16, CA, true, false>(a.q + p0 * a.q_cs, a.q_cs, Qs, nullptr, tid);
            ab_stage<128, 128, false, true>(a.go + p0 * a.go_cs + cv0, a.go_cs, nullptr, Ts, tid);
        }
        if (tid < 32) *reinterpret_cast<f32x4 *>(St + tid * 16) = *reinterpret_cast<const f32x4 *>(a.stats + (p0 + tid) * 4);
        __syncthreads();
        if (active) {
            const f32x16 s = ab_rows_mm<NG, QROW>(Qs, kf, l31, lh);      // rows = pixels of the tile, column = this lane's key
            float w[16];
            if constexpr (ROLE == 0) {
                const f32x16 dp = ab_rows_mm<CB / 16, GROW>(Gs, vf, l31, lh);
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
            ab_acc_mm<NJ>(Ts, w, acc, l31, lh);
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
struct Anab16PoolArgs {
    const bf16_t *k, *v, *g;
    bf16_t *khat, *khatT, *vhat, *vhatT;
    int k_cs, v_cs, g_cs, H, W, Ck, Cv, CAP, nsk;                 // nsk: 128-channel slabs of K (the slabs of V follow)
};

// grid = (337 bins, images, slabs of 128 channels of K then V); 16 waves, lane = a channel pair.  Wave w sums pixels w, w + 16, ...
// of the window (row-major inside the window), the sixteen partial sums are added in wave order: fixed, whatever the launch.
__global__ __launch_bounds__(64 * AB_POOL_WAVES) void anab16_pool_kernel(const Anab16PoolArgs a)
{
    __shared__ float red[AB_POOL_WAVES][128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bin = blockIdx.x, img = blockIdx.y;
    const bool isk = (int)blockIdx.z < a.nsk;
    const int c0 = (isk ? (int)blockIdx.z : (int)blockIdx.z - a.nsk) * 128;
    const int C = isk ? a.Ck : a.Cv, cs = isk ? a.k_cs : a.v_cs;
    const bf16_t *src = isk ? a.k : a.v;
    int si, sz, bi, bj;
    at_bin_pos(bin, si, sz, bi, bj);
    const int h0 = at_win_lo(bi, a.H, sz), h1 = at_win_hi(bi, a.H, sz), w0 = at_win_lo(bj, a.W, sz), w1 = at_win_hi(bj, a.W, sz);
    const int ww = w1 - w0, n = (h1 - h0) * ww;
    const int c = c0 + 2 * lane;
    const bool mine = c < C;                                       // (C is even)
    float s0 = 0.f, s1 = 0.f;
    for (int i0 = wave; i0 < n; i0 += 4 * AB_POOL_WAVES) {        // four pixels' loads in flight, added in pixel order
        float gt[4];
        unsigned xw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + AB_POOL_WAVES * u;
            gt[u] = 0.f;
            xw[u] = 0u;
            if (i < n) {                                           // (wave-uniform)
                const int dy = i / ww, dx = i - dy * ww;
                const size_t p = (size_t)img * a.H * a.W + (size_t)(h0 + dy) * a.W + (w0 + dx);
                gt[u] = ab_f(a.g[p * a.g_cs + si]);
                if (mine) xw[u] = *reinterpret_cast<const unsigned *>(src + p * cs + c);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const f32x2 x = unpack_bf16(xw[u]);
            s0 = fmaf(gt[u], x[0], s0);
            s1 = fmaf(gt[u], x[1], s1);
        }
    }
    red[wave][2 * lane] = s0;
    red[wave][2 * lane + 1] = s1;
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= 128 || c0 + t >= C) return;
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < AB_POOL_WAVES; ++w) acc += red[w][t];
    const bf16_t r = ab_r(acc * (1.0f / (float)n));
    const int cc = c0 + t;
    if (isk) {
        a.khat[((size_t)img * AT_KPAD + bin) * a.CAP + cc] = r;
        a.khatT[((size_t)img * a.CAP + cc) * AT_KPAD + bin] = r;
    } else {
        a.vhat[((size_t)img * AT_KPAD + bin) * a.Cv + cc] = r;
        a.vhatT[((size_t)img * a.Cv + cc) * AT_KPAD + bin] = r;
    }
}

struct Anab16GatherArgs {
    const bf16_t *k, *v, *g;
    const float *dkv;
    bf16_t *gk, *gv, *gg;
    int k_cs, v_cs, g_cs, gk_cs, gv_cs, gg_cs, H, W, Ck, Cv, do_k, do_v;
    long long pixels;
};

// One wave per pixel; lane = channel (strided by 64) of K|V.  For each scale the bins [i_lo, i_hi] x [j_lo, j_hi] that contain the
// pixel: i_lo = floor(y s / H), i_hi = ceil((y + 1) s / H) - 1 (every i with floor(i H / s) <= y < ceil((i + 1) H / s)).
__global__ __launch_bounds__(256) void anab16_gather_kernel(const Anab16GatherArgs a)
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
    for (int s = 0; s < 4; ++s) gate[s] = ab_f(a.g[(size_t)p * a.g_cs + s]);
    float dgs[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < C; c += 64) {
        const bool isk = c < a.Ck;
        if (isk ? !a.do_k : !a.do_v) continue;
        const float xv = a.gg ? ab_f(isk ? a.k[(size_t)p * a.k_cs + c] : a.v[(size_t)p * a.v_cs + (c - a.Ck)]) : 0.f;
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
        if (isk) { if (a.gk) a.gk[(size_t)p * a.gk_cs + c] = ab_r(o); }
        else if (a.gv) a.gv[(size_t)p * a.gv_cs + (c - a.Ck)] = ab_r(o);
    }
    if (!a.gg) return;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float t = dgs[s];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
        if (lane == s) a.gg[(size_t)p * a.gg_cs + s] = ab_r(t);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static bool ab_supported(int B, int H, int W, int Ck, int Cv)
{
    if (B < 1 || H < 1 || W < 1) return false;
    const long long HW = (long long)H * W;
    if (HW % 128 != 0 || (long long)B * HW >= 0x7FFFFFFFLL / 4 || H > 32768 || W > 32768) return false;
    return (Cv == 128 && (Ck == 64 || Ck == 128 || Ck == 168)) || (Cv == 256 && Ck == 168);
}

struct AbLayout {                        // offsets in bytes into the 256-byte aligned workspace
    int nch, CAP;
    long long khat, khatT, vhat, vhatT, fwd_end, stats, partK, partV, dkv, bwd_end;
};

static long long ab_up(long long x) { return (x + 255) / 256 * 256; }

static AbLayout ab_layout(int B, int H, int W, int Ck, int Cv)
{
    AbLayout L;
    const long long HW = (long long)H * W;
    L.CAP = (Ck + 31) / 32 * 32;
    L.nch = (int)((HW / 32 + AB_CHUNK_TILES - 1) / AB_CHUNK_TILES);
    long long o = 0;
    L.khat = o; o += ab_up((long long)B * AT_KPAD * L.CAP * 2);
    L.khatT = o; o += ab_up((long long)B * AT_KPAD * L.CAP * 2);
    L.vhat = o; o += ab_up((long long)B * AT_KPAD * Cv * 2);
    L.vhatT = o; o += ab_up((long long)B * AT_KPAD * Cv * 2);
    L.fwd_end = o;
    L.stats = o; o += ab_up((long long)B * HW * 4 * 4);
    L.partK = o; o += ab_up((long long)B * L.nch * AT_KPAD * L.CAP * 4);
    L.partV = o; o += ab_up((long long)B * L.nch * AT_KPAD * Cv * 4);
    L.dkv = o; o += ab_up((long long)B * AT_KEYS * (Ck + Cv) * 4);
    L.bwd_end = o;
    return L;
}

extern "C" long long m3d_anab_attention_workspace_bytes_bf16(int B, int H, int W, int Ck, int Cv, int backward)
{
    if (!ab_supported(B, H, W, Ck, Cv)) return -1;
    const AbLayout L = ab_layout(B, H, W, Ck, Cv);
    return backward ? L.bwd_end : L.fwd_end;
}

static int ab_check(const char *name, int B, int H, int W, int Ck, int Cv, const void *workspace, long long workspace_bytes, int backward)
{
    M3D_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: B, H, W must be positive", name);
    M3D_REQUIRE(((long long)H * W) % 128 == 0, "%s: H*W must be a multiple of 128 (HW %% 128 == 0; got %dx%d)", name, H, W);
    M3D_REQUIRE((Cv == 128 && (Ck == 64 || Ck == 128 || Ck == 168)) || (Cv == 256 && Ck == 168),
                "%s: built for (Ck, Cv) in {(64, 128), (128, 128), (168, 128), (168, 256)} (got %d, %d)", name, Ck, Cv);
    M3D_REQUIRE(ab_supported(B, H, W, Ck, Cv), "%s: too many pixels", name);
    M3D_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", name);
    const long long need = m3d_anab_attention_workspace_bytes_bf16(B, H, W, Ck, Cv, backward);
    M3D_REQUIRE(workspace_bytes >= need, "%s: workspace %lld < %lld bytes (m3d_anab_attention_workspace_bytes_bf16)", name,
                workspace_bytes, need);
    return M3D_OK;
}

// q / grad_out: 16-byte loads; k / v: 4-byte loads of channel pairs
static bool ab_rows16(const void *p, int cs) { return ((uintptr_t)p & 15) == 0 && cs % 8 == 0; }
static bool ab_rows4(const void *p, int cs) { return ((uintptr_t)p & 3) == 0 && cs % 2 == 0; }

// khat, khat^T, vhat, vhat^T (bf16, zero padded) into the first four blocks of the workspace
static int ab_pool(const AbLayout &L, unsigned char *ws, const void *k, int k_cs, const void *v, int v_cs, const void *g, int g_cs, int B,
                   int H, int W, int Ck, int Cv, hipStream_t st)
{
    M3D_HIP(hipMemsetAsync(ws, 0, (size_t)L.fwd_end, st));
    Anab16PoolArgs pa;
    pa.k = (const bf16_t *)k; pa.v = (const bf16_t *)v; pa.g = (const bf16_t *)g;
    pa.khat = (bf16_t *)(ws + L.khat); pa.khatT = (bf16_t *)(ws + L.khatT);
    pa.vhat = (bf16_t *)(ws + L.vhat); pa.vhatT = (bf16_t *)(ws + L.vhatT);
    pa.k_cs = k_cs; pa.v_cs = v_cs; pa.g_cs = g_cs; pa.H = H; pa.W = W; pa.Ck = Ck; pa.Cv = Cv; pa.CAP = L.CAP;
    pa.nsk = (Ck + 127) / 128;
    hipLaunchKernelGGL(anab16_pool_kernel, dim3(AT_KEYS, B, pa.nsk + Cv / 128), dim3(64 * AB_POOL_WAVES), 0, st, pa);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

extern "C" int m3d_anab_attention_forward_bf16(const void *q, const void *k, const void *v, const void *g, void *out, int B, int H, int W,
                                               int Ck, int Cv, int q_cs, int k_cs, int v_cs, int g_cs, int out_cs, void *workspace,
                                               long long workspace_bytes, m3d_stream_t stream)
{
    const char *name = "anab_attention_forward_bf16";
    M3D_REQUIRE(q && k && v && g && out, "%s: null pointer", name);
    int rc = ab_check(name, B, H, W, Ck, Cv, workspace, workspace_bytes, 0);
    if (rc != M3D_OK) return rc;
    M3D_REQUIRE(q_cs >= Ck && k_cs >= Ck && v_cs >= Cv && g_cs >= 4 && out_cs >= Cv, "%s: a row stride is below its channel count", name);
    M3D_REQUIRE(ab_rows16(q, q_cs), "%s: q must be a 16-byte aligned view with a row stride that is a multiple of 8 elements", name);
    M3D_REQUIRE(ab_rows4(k, k_cs) && ab_rows4(v, v_cs) && ab_rows4(g, g_cs),
                "%s: k, v and g must be 4-byte aligned views with even row strides", name);
    const hipStream_t st = (hipStream_t)stream;
    const AbLayout L = ab_layout(B, H, W, Ck, Cv);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    rc = ab_pool(L, ws, k, k_cs, v, v_cs, g, g_cs, B, H, W, Ck, Cv, st);
    if (rc != M3D_OK) return rc;
    Anab16Args a = {};
    a.q = (const bf16_t *)q; a.khat = (const bf16_t *)(ws + L.khat); a.vhatT = (const bf16_t *)(ws + L.vhatT);
    a.out = (bf16_t *)out; a.q_cs = q_cs; a.out_cs = out_cs; a.HW = H * W; a.Cv = Cv;
    const dim3 grid(B * (a.HW / 128), Cv / 128);
    if (Ck == 168) hipLaunchKernelGGL((anab16_fwd_kernel<168>), grid, dim3(256), 0, st, a);
    else if (Ck == 128) hipLaunchKernelGGL((anab16_fwd_kernel<128>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((anab16_fwd_kernel<64>), grid, dim3(256), 0, st, a);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

template <int CA, int CB>
static void ab_launch_main(const Anab16Args &a, int B, bool do_k, bool do_v, hipStream_t st)
{
    hipLaunchKernelGGL((anab16_pix_kernel<CA, CB>), dim3(B * (a.HW / 128)), dim3(256), 0, st, a);
    if (do_k) hipLaunchKernelGGL((anab16_key_kernel<CA, CB, 0>), dim3(3, a.nch, B), dim3(256), 0, st, a);
    if (do_v) hipLaunchKernelGGL((anab16_key_kernel<CA, CB, 1>), dim3(3 * (CB / 128), a.nch, B), dim3(256), 0, st, a);
}

extern "C" int m3d_anab_attention_backward_bf16(const void *q, const void *k, const void *v, const void *g, const void *grad_out,
                                                void *grad_q, void *grad_k, void *grad_v, void *grad_g, int B, int H, int W, int Ck,
                                                int Cv, int q_cs, int k_cs, int v_cs, int g_cs, int go_cs, int gq_cs, int gk_cs,
                                                int gv_cs, int gg_cs, void *workspace, long long workspace_bytes, m3d_stream_t stream)
{
    const char *name = "anab_attention_backward_bf16";
    M3D_REQUIRE(q && k && v && g && grad_out, "%s: null pointer", name);
    int rc = ab_check(name, B, H, W, Ck, Cv, workspace, workspace_bytes, 1);
    if (rc != M3D_OK) return rc;
    M3D_REQUIRE(q_cs >= Ck && k_cs >= Ck && v_cs >= Cv && g_cs >= 4 && go_cs >= Cv, "%s: a row stride is below its channel count", name);
    M3D_REQUIRE((!grad_q || gq_cs >= Ck) && (!grad_k || gk_cs >= Ck) && (!grad_v || gv_cs >= Cv) && (!grad_g || gg_cs >= 4),
                "%s: a gradient's row stride is below its channel count", name);
    M3D_REQUIRE(ab_rows16(q, q_cs) && ab_rows16(grad_out, go_cs),
                "%s: q and grad_out must be 16-byte aligned views with row strides that are multiples of 8 elements", name);
    M3D_REQUIRE(ab_rows4(k, k_cs) && ab_rows4(v, v_cs) && ab_rows4(g, g_cs),
                "%s: k, v and g must be 4-byte aligned views with even row strides", name);
    if (!grad_q && !grad_k && !grad_v && !grad_g) return M3D_OK;
    const hipStream_t st = (hipStream_t)stream;
    const AbLayout L = ab_layout(B, H, W, Ck, Cv);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const int HW = H * W;
    rc = ab_pool(L, ws, k, k_cs, v, v_cs, g, g_cs, B, H, W, Ck, Cv, st);
    if (rc != M3D_OK) return rc;
    // dkhat feeds grad_k and grad_g, dvhat feeds grad_v and grad_g; the statistics of the pixel-major kernel feed both
    const bool do_k = grad_k || grad_g, do_v = grad_v || grad_g;
    Anab16Args a = {};
    a.q = (const bf16_t *)q; a.go = (const bf16_t *)grad_out;
    a.khat = (const bf16_t *)(ws + L.khat); a.khatT = (const bf16_t *)(ws + L.khatT); a.vhat = (const bf16_t *)(ws + L.vhat);
    a.stats = (float *)(ws + L.stats); a.gq = (bf16_t *)grad_q;
    a.partK = (float *)(ws + L.partK); a.partV = (float *)(ws + L.partV);
    a.q_cs = q_cs; a.go_cs = go_cs; a.gq_cs = gq_cs; a.HW = HW; a.nch = L.nch; a.Cv = Cv; a.need_dq = grad_q ? 1 : 0;
    if (Cv == 256) ab_launch_main<168, 256>(a, B, do_k, do_v, st);
    else if (Ck == 168) ab_launch_main<168, 128>(a, B, do_k, do_v, st);
    else if (Ck == 128) ab_launch_main<128, 128>(a, B, do_k, do_v, st);
    else ab_launch_main<64, 128>(a, B, do_k, do_v, st);
    M3D_LAUNCH_CHECK();
    if (!do_k && !do_v) return M3D_OK;
    float *dkv = (float *)(ws + L.dkv);
    {
        const long long total = (long long)B * AT_KEYS * (Ck + Cv);
        hipLaunchKernelGGL(anab_bwd_reduce_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, a.partK, a.partV, dkv, L.nch, L.CAP, Ck, Cv, H,
                           W, do_k ? 1 : 0, do_v ? 1 : 0, total);
        M3D_LAUNCH_CHECK();
    }
    Anab16GatherArgs ga;
    ga.k = (const bf16_t *)k; ga.v = (const bf16_t *)v; ga.g = (const bf16_t *)g; ga.dkv = dkv;
    ga.gk = (bf16_t *)grad_k; ga.gv = (bf16_t *)grad_v; ga.gg = (bf16_t *)grad_g;
    ga.k_cs = k_cs; ga.v_cs = v_cs; ga.g_cs = g_cs; ga.gk_cs = gk_cs; ga.gv_cs = gv_cs; ga.gg_cs = gg_cs;
    ga.H = H; ga.W = W; ga.Ck = Ck; ga.Cv = Cv; ga.do_k = do_k ? 1 : 0; ga.do_v = do_v ? 1 : 0;
    ga.pixels = (long long)B * HW;
    hipLaunchKernelGGL(anab16_gather_kernel, dim3(cdiv(ga.pixels, 4)), dim3(256), 0, st, ga);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}
