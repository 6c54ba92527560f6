// The ANAB attention core for training (model/module/attention.py:136-147, 207-211) in both compute types: fp32, and bf16 tensors for
// torch.autocast(bfloat16).  Per image, N = H*W pixels, 337 keys (the AdaptiveAvgPool2d bins of sizes 1/4/8/16, scale-major):
//     khat[b] = mean_{p in win_b} g[p][scale(b)] k[p]        vhat likewise from v
//     S = q khat^T,  P = softmax_keys(S),  O = P vhat
// Backward (dO = grad_out):  dvhat = P^T dO,  dP = dO vhat^T,  D = rowsum(dO * O) = rowsum(P * dP),  dS = P * (dP - D),
//     dq = dS khat,  dkhat = dS^T q;   with w_b(p) = [p in win_b] / area_b:
//     dk[p] = sum_b w_b(p) g[p][scale(b)] dkhat[b],  dv likewise,  dg[p][s] = sum_{b of scale s} w_b(p) (k[p].dkhat[b] + v[p].dvhat[b])
//
// The backward in launches (everything on one stream, nothing atomic, every sum in a fixed order):
//   1. the pooling of the forward again: khat [key][CAP] and vhat [key][Cv] into the zeroed workspace (per type, see below);
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
// The logits, P, dP and dS never reach memory.  What bounds the fp32 operator: steps 2 and 3 compute S four times (both passes of
// the pixel-major kernel, both roles of the key-major one) and dP three times, beside dq, dkhat and dvhat once each: about 31 GMAC
// at B = 8, 48x160, Ck = 168, Cv = 128 against 6.1 for the forward, on the 256 FLOP/cycle/CU fp32 MFMA, with the tiles staged
// without overlap (load -> barrier -> multiply).
//
// bf16: every product on v_mfma_f32_32x32x16_bf16.  Rounding points (the contract of include/m3dssd_hip.h): pooling sums, softmax
// statistics and every accumulator are fp32; khat / vhat are rounded once to bf16 (the MFMA operands); S and dP are never rounded;
// P is rounded once as the operand of P.vhat (the unnormalised exponential, 1/l applied to the fp32 accumulator) and of P^T.dO
// (normalised); dS is rounded once as the operand of dq and dkhat; dkhat / dvhat, their chunk sums and the gather stay fp32; every
// output is rounded once.  1/l is an IEEE division.
//
// Shared, once, on the element traits AnabF32 / AnabBf16: the pixel-major, key-major, gather and reduce kernels with their argument
// structs, the shape rule, the argument check, the (Ck, Cv) dispatch and the backward driver.
// Per type: the tile helpers inside the traits (another MFMA, another fragment), the forward (fp32 goes through the engine's pooling
// and attention launches, bf16 has a pooling and a forward kernel of its own), the workspace planners (floats against bytes, other
// blocks) and the alignment rules.
#include <stdlib.h>

#include "common.h"
#include "bf16_tile.h"

#define AT_KEYS 337
#define AT_KPAD 352                      // keys padded to the tile of 32
#define AT_CHUNK_TILES 16                // pixel tiles of 32 per key-major workgroup
#define AB_POOL_WAVES 16

typedef unsigned short bf16_t;

__device__ __forceinline__ float ab_f(bf16_t x) { return __uint_as_float((unsigned)x << 16); }
__device__ __forceinline__ bf16_t ab_r(float x) { return (bf16_t)(pack_bf16(x, 0.f) & 0xFFFFu); }

// ---- the bins: key order and windows of the pyramid ----------------------------------------------------------------------------------
// bin -> its scale index, grid size and position (scale-major: 1 + 16 + 64 + 256)
__device__ __forceinline__ void at_bin_pos(const int bin, int &si, int &sz, int &bi, int &bj)
{
    int local;
    if (bin < 1) { si = 0; sz = 1; local = bin; }
    else if (bin < 17) { si = 1; sz = 4; local = bin - 1; }
    else if (bin < 81) { si = 2; sz = 8; local = bin - 17; }
    else { si = 3; sz = 16; local = bin - 81; }
    bi = local / sz;
    bj = local - bi * sz;
}
__host__ __device__ __forceinline__ int at_win_lo(int i, int n, int s) { return (i * n) / s; }
__host__ __device__ __forceinline__ int at_win_hi(int i, int n, int s) { return ((i + 1) * n + s - 1) / s; }

template <class E>
struct AnabBwdArgs {
    typedef typename E::T T;
    const T *q, *go, *khat, *vhat;       // khat [B][352][CAP], vhat [B][352][Cv]: zero outside [337][Ck] / past key 337
    float *stats;                        // [B*HW][4] = m, 1/l, D, 0
    T *gq;
    float *partK, *partV;                // [B][nch][352][CAP], [B][nch][352][Cv]
    int q_cs, go_cs, gq_cs, HW, nch, Cv, need_dq;
    const T *khatT;                      // [B][CAP][352], what stage_k_tiles reads beside khat: bf16 only, NULL for fp32
};

// ---- the element traits: what the shared kernels and the shared driver need to know about a compute type ----------------------------
// Device side, the tile helpers.  A staged tile is 32 rows; row-major it has a row pitch of C * sizeof(T) + 16 bytes, transposed it
// is [C][TROW].  A lane's own row is held as Frag[frags(C)], KSTEP channels per fragment over the two lane halves.
// Host side, what differs between the two C ABIs: the size query and what a short workspace returns, the alignment rule of the
// backward, and the front of the backward (plan the workspace, pool) that fills the kernels' arguments.
struct AnabF32 {
    typedef float T;
    typedef f32x4 Frag;
    static constexpr int KSTEP = 8;                    // bf[g] = row[8 g + 4 h + {0..3}] (h = lane half)
    static constexpr int TROW = 32 * 4 + 16;           // bytes per row of a transposed tile in LDS (32 tile rows + 16 pad)

    static __device__ __forceinline__ float load(const float x) { return x; }
    static __device__ __forceinline__ float store(const float x) { return x; }
    static __device__ __forceinline__ bool store4_aligned(const float *, const int) { return true; }
    static __device__ __forceinline__ void store4(float *p, const float a, const float b, const float c, const float d, const bool)
    {
        p[0] = a; p[1] = b; p[2] = c; p[3] = d;
    }

    // 32 rows x C floats from global (row stride `stride` floats, 16-byte aligned pieces) into LDS: row-major (row stride C * 4 + 16
    // bytes) and / or transposed ([C][TROW]).  All 256 threads of the workgroup.  (Every supported C is whole: CV == C.)
    template <int C, int CV, bool ROWMAJOR, bool TRANS>
    static __device__ __forceinline__ void stage(const float *src, const size_t stride, unsigned char *R, unsigned char *T, const int tid)
    {
        static_assert(C == CV, "fp32 rows are staged whole");
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
                    for (int e = 0; e < 4; ++e) *reinterpret_cast<float *>(T + (c4 * 4 + e) * TROW + row * 4) = x[e];
                }
            }
        }
    }

    // a key tile of khat (32 rows of [352][CAP]), row-major and transposed: one load, transposed while staging
    template <int CAP>
    static __device__ __forceinline__ void stage_k_tiles(const float *khat, const float *, unsigned char *Ks, unsigned char *KsT,
                                                         const int tid)
    {
        stage<CAP, CAP, true, true>(khat, CAP, Ks, KsT, tid);
    }

    template <int C>
    static __device__ __forceinline__ void own_row(const float *row, f32x4 (&bf)[C / 8], const int lh)
    {
        const float *p = row + 4 * lh;
#pragma unroll
        for (int t = 0; t < C / 8; ++t) bf[t] = *reinterpret_cast<const f32x4 *>(p + 8 * t);
    }

    // D[row][lane] = sum_c A[row][c] * b[lane][c]: A = the 32 rows of a row-major LDS tile, b = the lane's own row (own_row).
    // Register r of the result is row 8 (r / 4) + 4 h + r % 4, the column is lane & 31.
    template <int NG, int ROWBYTES>
    static __device__ __forceinline__ f32x16 rows_mm(const unsigned char *As, const f32x4 (&bf)[NG], const int l31, const int lh)
    {
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        const unsigned char *ab = As + l31 * ROWBYTES + lh * 16;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const f32x4 af = *reinterpret_cast<const f32x4 *>(ab + g * 32);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], bf[g][j], s, 0, 0, 0);
        }
        return s;
    }

    // acc[j][.][lane] += sum_t T[32 j + .][t] * w[t][lane]: T = a transposed LDS tile (rows = output channels, 32 tile rows each),
    // w = the lane's register tile in the layout rows_mm returns -- exactly the two k of each MFMA step, no exchange.
    template <int NJ>
    static __device__ __forceinline__ void acc_mm(const unsigned char *Ts, const float (&w)[16], f32x16 (&acc)[NJ], const int l31,
                                                  const int lh)
    {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const unsigned char *tb = Ts + (32 * j + l31) * TROW + lh * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 tf = *reinterpret_cast<const f32x4 *>(tb + i * 32);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(tf[jj], w[4 * i + jj], acc[j], 0, 0, 0);
            }
        }
    }

    static constexpr const char *bwd_name = "anab_attention_backward", *query_name = "m3d_anab_attention_workspace_bytes";
    static constexpr int short_workspace = M3D_E_WORKSPACE;
    static long long workspace_bytes(int B, int H, int W, int Ck, int Cv, int backward)
    {
        return m3d_anab_attention_workspace_bytes(B, H, W, Ck, Cv, backward);
    }
    static int check_backward_views(const float *q, int q_cs, const float *k, int k_cs, const float *v, int v_cs, const float *g, int g_cs,
                                    const float *grad_out, int go_cs);
    static int begin_backward(AnabBwdArgs<AnabF32> &a, float *&dkv, void *workspace, const float *k, int k_cs, const float *v, int v_cs,
                              const float *g, int g_cs, int B, int H, int W, int Ck, int Cv, m3d_stream_t stream);
};

struct AnabBf16 {
    typedef bf16_t T;
    typedef bf16x8 Frag;
    static constexpr int KSTEP = 16;                   // bf[g] = row[16 g + 8 h + (0..7)]
    static constexpr int TROW = 32 * 2 + 16;

    static __device__ __forceinline__ float load(const bf16_t x) { return ab_f(x); }
    static __device__ __forceinline__ bf16_t store(const float x) { return ab_r(x); }
    static __device__ __forceinline__ bool store4_aligned(const bf16_t *base, const int cs) { return (((uintptr_t)base & 7) | (cs & 3)) == 0; }
    // 4 consecutive channels of one row, rounded once
    static __device__ __forceinline__ void store4(bf16_t *p, const float a, const float b, const float c, const float d, const bool al8)
    {
        if (al8) {
            const u32x2 w = {pack_bf16(a, b), pack_bf16(c, d)};
            *reinterpret_cast<u32x2 *>(p) = w;
        } else {
            p[0] = ab_r(a); p[1] = ab_r(b); p[2] = ab_r(c); p[3] = ab_r(d);
        }
    }

    // 32 rows x C bf16 (channels [CV, C) as zeros, never read) from global (row stride `stride` elements, 16-byte aligned pieces) into
    // LDS: row-major (row stride C * 2 + 16 bytes) and / or transposed ([C][TROW]).  All 256 threads of the workgroup.
    template <int C, int CV, bool ROWMAJOR, bool TRANS>
    static __device__ __forceinline__ void stage(const bf16_t *src, const size_t stride, unsigned char *R, unsigned char *T, const int tid)
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
                        *reinterpret_cast<bf16_t *>(T + (c8 * 8 + e) * TROW + row * 2) = (bf16_t)(x[e >> 1] >> (16 * (e & 1)));
                }
            }
        }
    }

    // NR rows of a [.][352] workspace matrix, columns 32 t .. 32 t + 31 -> the transposed LDS tile [NR][TROW]
    template <int NR>
    static __device__ __forceinline__ void stage_cols(const bf16_t *src, unsigned char *T, const int tid)
    {
#pragma unroll
        for (int p = 0; p < (NR * 4 + 255) / 256; ++p) {
            const int i = tid + 256 * p;
            if (i < NR * 4) {
                const int row = i >> 2, pc = i & 3;
                *reinterpret_cast<u32x4 *>(T + row * TROW + pc * 16) = *reinterpret_cast<const u32x4 *>(src + (size_t)row * AT_KPAD + pc * 8);
            }
        }
    }

    // a key tile of khat (32 rows of [352][CAP]), row-major and transposed: khat, and the same 32 columns of the khat^T block
    // [CAP][352] of the workspace
    template <int CAP>
    static __device__ __forceinline__ void stage_k_tiles(const bf16_t *khat, const bf16_t *khatT, unsigned char *Ks, unsigned char *KsT,
                                                         const int tid)
    {
        stage<CAP, CAP, true, false>(khat, CAP, Ks, nullptr, tid);
        stage_cols<CAP>(khatT, KsT, tid);
    }

    // The lane's own row as B fragments, zero from channel C on
    template <int C>
    static __device__ __forceinline__ void own_row(const bf16_t *row, bf16x8 (&bf)[(C + 15) / 16], const int lh)
    {
#pragma unroll
        for (int g = 0; g < (C + 15) / 16; ++g) {
            u32x4 x = {0u, 0u, 0u, 0u};
            if (16 * g + 8 < C || lh == 0) x = *reinterpret_cast<const u32x4 *>(row + 16 * g + 8 * lh);
            bf[g] = __builtin_bit_cast(bf16x8, x);
        }
    }

    // D[row][lane] = sum_c A[row][c] * b[lane][c]: A = the 32 rows of a row-major LDS tile, b = the lane's own row (own_row).
    // Register r of the result is row 8 (r / 4) + 4 h + r % 4, the column is lane & 31.
    template <int NG, int ROWBYTES>
    static __device__ __forceinline__ f32x16 rows_mm(const unsigned char *As, const bf16x8 (&bf)[NG], const int l31, const int lh)
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

    // acc[j][.][lane] += sum_t T[32 j + .][t] * bf16(w[t][lane]): T = a transposed LDS tile (rows = output channels, 32 tile rows
    // each), w = the lane's register tile in the layout rows_mm returns.  Registers 8u .. 8u + 7 are the B fragment of k-step u; its
    // element j of lane half h is tile row 16u + 8 (j >> 2) + 4h + (j & 3), and the A fragment is read from T in that same order.
    template <int NJ>
    static __device__ __forceinline__ void acc_mm(const unsigned char *Ts, const float (&w)[16], f32x16 (&acc)[NJ], const int l31,
                                                  const int lh)
    {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            u32x4 pb;
#pragma unroll
            for (int i = 0; i < 4; ++i) pb[i] = pack_bf16(w[8 * u + 2 * i], w[8 * u + 2 * i + 1]);
            const bf16x8 pf = __builtin_bit_cast(bf16x8, pb);
            const unsigned char *tb = Ts + l31 * TROW + (16 * u + 4 * lh) * 2;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const u32x2 lo = *reinterpret_cast<const u32x2 *>(tb + j * 32 * TROW);
                const u32x2 hi = *reinterpret_cast<const u32x2 *>(tb + j * 32 * TROW + 16);
                const u32x4 tw = {lo[0], lo[1], hi[0], hi[1]};
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, tw), pf, acc[j], 0, 0, 0);
            }
        }
    }

    static constexpr const char *bwd_name = "anab_attention_backward_bf16", *query_name = "m3d_anab_attention_workspace_bytes_bf16";
    static constexpr int short_workspace = M3D_E_ARG;
    static long long workspace_bytes(int B, int H, int W, int Ck, int Cv, int backward)
    {
        return m3d_anab_attention_workspace_bytes_bf16(B, H, W, Ck, Cv, backward);
    }
    static int check_backward_views(const bf16_t *q, int q_cs, const bf16_t *k, int k_cs, const bf16_t *v, int v_cs, const bf16_t *g,
                                    int g_cs, const bf16_t *grad_out, int go_cs);
    static int begin_backward(AnabBwdArgs<AnabBf16> &a, float *&dkv, void *workspace, const bf16_t *k, int k_cs, const bf16_t *v, int v_cs,
                              const bf16_t *g, int g_cs, int B, int H, int W, int Ck, int Cv, m3d_stream_t stream);
};

// ---- step 2: pixel-major ------------------------------------------------------------------------------------------------------------
template <class E, int CA, int CB>     // key / query channels (multiple of 8), value channels
__global__ __launch_bounds__(256) void anab_bwd_pix_kernel(const AnabBwdArgs<E> a)
{
    typedef typename E::T T;
    constexpr int CAP = (CA + 31) / 32 * 32, NGA = (CA + E::KSTEP - 1) / E::KSTEP, NGB = CB / E::KSTEP;
    constexpr int KROW = CAP * sizeof(T) + 16, VROW = CB * sizeof(T) + 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[32 * KROW + CAP * E::TROW + 32 * VROW];
    unsigned char *Ks = lds, *KsT = lds + 32 * KROW, *Vs = KsT + CAP * E::TROW;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.x / (a.HW / 128);
    const size_t mq = (size_t)blockIdx.x * 128 + wave * 32 + l31;        // this lane's pixel (linear over the batch)

    typename E::Frag qf[NGA], gf[NGB];
    E::template own_row<CA>(a.q + mq * a.q_cs, qf, lh);
    E::template own_row<CB>(a.go + mq * a.go_cs, gf, lh);
    const T *kimg = a.khat + (size_t)img * AT_KPAD * CAP, *vimg = a.vhat + (size_t)img * AT_KPAD * CB;
    const T *ktimg = a.khatT + (size_t)img * CAP * AT_KPAD;
    constexpr int NT = AT_KPAD / 32;

    // ---- pass 1: m, l, sum(e * dP) -----------------------------------------------------------------------------------------------
    float m = -INFINITY, l = 0.f, dacc = 0.f;
    for (int t = 0; t < NT; ++t) {
        __syncthreads();
        E::template stage<CAP, CAP, true, false>(kimg + (size_t)32 * t * CAP, CAP, Ks, nullptr, tid);
        E::template stage<CB, CB, true, false>(vimg + (size_t)32 * t * CB, CB, Vs, nullptr, tid);
        __syncthreads();
        f32x16 s = E::template rows_mm<NGA, KROW>(Ks, qf, l31, lh);
        const f32x16 dp = E::template rows_mm<NGB, VROW>(Vs, gf, l31, lh);
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
    for (int t = 0; t < NT; ++t) {
        __syncthreads();
        E::template stage_k_tiles<CAP>(kimg + (size_t)32 * t * CAP, ktimg + 32 * t, Ks, KsT, tid);
        E::template stage<CB, CB, true, false>(vimg + (size_t)32 * t * CB, CB, Vs, nullptr, tid);
        __syncthreads();
        const f32x16 s = E::template rows_mm<NGA, KROW>(Ks, qf, l31, lh);
        const f32x16 dp = E::template rows_mm<NGB, VROW>(Vs, gf, l31, lh);
        float w[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool valid = 32 * t + 8 * (r >> 2) + 4 * lh + (r & 3) < AT_KEYS;
            const float p = valid ? expf(s[r] - m) * inv : 0.f;
            w[r] = p * (dp[r] - D);
        }
        E::template acc_mm<CAP / 32>(KsT, w, acc, l31, lh);
    }
    T *op = a.gq + mq * a.gq_cs;
    const bool al = E::store4_aligned(a.gq, a.gq_cs);
#pragma unroll
    for (int j = 0; j < CAP / 32; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 32 * j + 8 * i + 4 * lh;                 // channels past Ck are not ours
            if (c < CA) E::store4(op + c, acc[j][4 * i], acc[j][4 * i + 1], acc[j][4 * i + 2], acc[j][4 * i + 3], al);
        }
}

// ---- step 3: key-major --------------------------------------------------------------------------------------------------------------
// grid = (3 key blocks of 128 [x Cv / 128 value slices for ROLE 1], pixel chunks, images).  ROLE 0: dkhat, ROLE 1: dvhat.
template <class E, int CA, int CB, int ROLE>
__global__ __launch_bounds__(256) void anab_bwd_key_kernel(const AnabBwdArgs<E> a)
{
    typedef typename E::T T;
    constexpr int CAP = (CA + 31) / 32 * 32, NGA = (CA + E::KSTEP - 1) / E::KSTEP, NGB = CB / E::KSTEP;
    constexpr int CAK = NGA * E::KSTEP;                            // a staged q row, padded to the k-step (fp32: CA)
    constexpr int QROW = CAK * sizeof(T) + 16, GROW = CB * sizeof(T) + 16;
    constexpr int NJ = ROLE == 0 ? CAP / 32 : 4;
    // ROLE 0: Qs, QsT [CAP], Gs (all value channels, row-major).  ROLE 1: Qs, GsT [128] (this workgroup's value channels)
    constexpr int LDS_BYTES = 32 * QROW + (ROLE == 0 ? CAP * E::TROW + 32 * GROW : 128 * E::TROW) + 32 * 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    unsigned char *Qs = lds, *Ts = lds + 32 * QROW;               // Ts: QsT (ROLE 0) or GsT (ROLE 1)
    unsigned char *Gs = Ts + CAP * E::TROW;                        // (ROLE 0 only)
    unsigned char *St = lds + LDS_BYTES - 32 * 16;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kb = ROLE == 0 ? (int)blockIdx.x : (int)blockIdx.x % 3;
    const int cv0 = ROLE == 0 ? 0 : ((int)blockIdx.x / 3) * 128;
    const int ch = blockIdx.y, img = blockIdx.z;
    const bool active = kb * 128 + wave * 32 < AT_KPAD;           // (wave-uniform) the last block has three waves of keys
    const int key = kb * 128 + wave * 32 + l31;
    const int keyc = min(key, AT_KPAD - 1);

    typename E::Frag kf[NGA], vf[ROLE == 0 ? NGB : 1];
    E::template own_row<CA>(a.khat + ((size_t)img * AT_KPAD + keyc) * CAP, kf, lh);
    if constexpr (ROLE == 0) E::template own_row<CB>(a.vhat + ((size_t)img * AT_KPAD + keyc) * CB, vf, lh);
    if (ROLE == 0 && CAP > CA)                                     // rows of q^T past Ck: never staged, their products never stored
        for (int i = tid; i < (CAP - CA) * (E::TROW / 4); i += 256) reinterpret_cast<unsigned *>(Ts + CA * E::TROW)[i] = 0u;

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
            E::template stage<CAK, CA, true, true>(a.q + p0 * a.q_cs, a.q_cs, Qs, Ts, tid);
            E::template stage<CB, CB, true, false>(a.go + p0 * a.go_cs, a.go_cs, Gs, nullptr, tid);
        } else {
            E::template stage<CAK, CA, true, false>(a.q + p0 * a.q_cs, a.q_cs, Qs, nullptr, tid);
            E::template stage<128, 128, false, true>(a.go + p0 * a.go_cs + cv0, a.go_cs, nullptr, Ts, tid);
        }
        if (tid < 32) *reinterpret_cast<f32x4 *>(St + tid * 16) = *reinterpret_cast<const f32x4 *>(a.stats + (p0 + tid) * 4);
        __syncthreads();
        if (active) {
            const f32x16 s = E::template rows_mm<NGA, QROW>(Qs, kf, l31, lh);   // rows = pixels of the tile, column = this lane's key
            float w[16];
            if constexpr (ROLE == 0) {
                const f32x16 dp = E::template rows_mm<NGB, GROW>(Gs, vf, l31, lh);
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
            E::template acc_mm<NJ>(Ts, w, acc, l31, lh);
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

// ---- steps 4 and 5: reduce and gather -----------------------------------------------------------------------------------------------
// dkv [B][337][Ck + Cv] = (1 / area_bin) * sum over the pixel chunks, in chunk order, of the key-major kernel's
// partials [B][nch][352][CAP] and [B][nch][352][Cv]
__global__ void anab_bwd_reduce_kernel(const float *__restrict__ partK, const float *__restrict__ partV, float *__restrict__ dkv, int nch,
                                       int CAP, int Ck, int Cv, int H, int W, int do_k, int do_v, long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int C = Ck + Cv;
    const int c = (int)(i % C);
    const long long bb = i / C;
    const int bin = (int)(bb % AT_KEYS);
    const long long b = bb / AT_KEYS;
    const bool isk = c < Ck;
    if (isk ? !do_k : !do_v) return;
    float acc = 0.f;
    for (int ch = 0; ch < nch; ++ch) {
        const size_t row = ((size_t)b * nch + ch) * AT_KPAD + bin;
        acc += isk ? partK[row * CAP + c] : partV[row * Cv + (c - Ck)];
    }
    int si, sz, bi, bj;
    at_bin_pos(bin, si, sz, bi, bj);
    const int area = (at_win_hi(bi, H, sz) - at_win_lo(bi, H, sz)) * (at_win_hi(bj, W, sz) - at_win_lo(bj, W, sz));
    dkv[i] = acc * (1.0f / (float)area);
}

template <class E>
struct AnabGatherArgs {
    typedef typename E::T T;
    const T *k, *v, *g;
    const float *dkv;
    T *gk, *gv, *gg;
    int k_cs, v_cs, g_cs, gk_cs, gv_cs, gg_cs, H, W, Ck, Cv, do_k, do_v;
    long long pixels;
};

// One wave per pixel; lane = channel (strided by 64) of K|V.  For each scale the bins [i_lo, i_hi] x [j_lo, j_hi] that contain the
// pixel: i_lo = floor(y s / H), i_hi = ceil((y + 1) s / H) - 1 (every i with floor(i H / s) <= y < ceil((i + 1) H / s)).
template <class E>
__global__ __launch_bounds__(256) void anab_bwd_gather_kernel(const AnabGatherArgs<E> a)
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
    for (int s = 0; s < 4; ++s) gate[s] = E::load(a.g[(size_t)p * a.g_cs + s]);
    float dgs[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < C; c += 64) {
        const bool isk = c < a.Ck;
        if (isk ? !a.do_k : !a.do_v) continue;
        const float xv = a.gg ? E::load(isk ? a.k[(size_t)p * a.k_cs + c] : a.v[(size_t)p * a.v_cs + (c - a.Ck)]) : 0.f;
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
        if (isk) { if (a.gk) a.gk[(size_t)p * a.gk_cs + c] = E::store(o); }
        else if (a.gv) a.gv[(size_t)p * a.gv_cs + (c - a.Ck)] = E::store(o);
    }
    if (!a.gg) return;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float t = dgs[s];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
        if (lane == s) a.gg[(size_t)p * a.gg_cs + s] = E::store(t);
    }
}

// ---- host, shared -------------------------------------------------------------------------------------------------------------------
static bool anab_supported(int B, int H, int W, int Ck, int Cv)
{
    if (B < 1 || H < 1 || W < 1) return false;
    const long long HW = (long long)H * W;
    if (HW % 128 != 0 || (long long)B * HW >= 0x7FFFFFFFLL / 4 || H > 32768 || W > 32768) return false;
    return (Cv == 128 && (Ck == 64 || Ck == 128 || Ck == 168)) || (Cv == 256 && Ck == 168);
}

template <class E>
static int anab_check(const char *name, int B, int H, int W, int Ck, int Cv, const void *workspace, long long workspace_bytes, int backward)
{
    M3D_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: B, H, W must be positive", name);
    M3D_REQUIRE(((long long)H * W) % 128 == 0, "%s: H*W must be a multiple of 128 (HW %% 128 == 0; got %dx%d)", name, H, W);
    M3D_REQUIRE((Cv == 128 && (Ck == 64 || Ck == 128 || Ck == 168)) || (Cv == 256 && Ck == 168),
                "%s: built for (Ck, Cv) in {(64, 128), (128, 128), (168, 128), (168, 256)} (got %d, %d)", name, Ck, Cv);
    M3D_REQUIRE(anab_supported(B, H, W, Ck, Cv), "%s: too many pixels", name);
    M3D_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", name);
    const long long need = E::workspace_bytes(B, H, W, Ck, Cv, backward);
    if (workspace_bytes < need) {                                  // (M3D_E_WORKSPACE for fp32, M3D_E_ARG for bf16: include/m3dssd_hip.h)
        m3d_set_error("%s: workspace %lld < %lld bytes (%s)", name, workspace_bytes, need, E::query_name);
        return E::short_workspace;
    }
    return M3D_OK;
}

template <class E, int CA, int CB>
static void anab_launch_main(const AnabBwdArgs<E> &a, int B, bool do_k, bool do_v, hipStream_t st)
{
    hipLaunchKernelGGL((anab_bwd_pix_kernel<E, CA, CB>), dim3(B * (a.HW / 128)), dim3(256), 0, st, a);
    if (do_k) hipLaunchKernelGGL((anab_bwd_key_kernel<E, CA, CB, 0>), dim3(3, a.nch, B), dim3(256), 0, st, a);
    if (do_v) hipLaunchKernelGGL((anab_bwd_key_kernel<E, CA, CB, 1>), dim3(3 * (CB / 128), a.nch, B), dim3(256), 0, st, a);
}

template <class E>
static int anab_backward(const typename E::T *q, const typename E::T *k, const typename E::T *v, const typename E::T *g,
                         const typename E::T *grad_out, typename E::T *grad_q, typename E::T *grad_k, typename E::T *grad_v,
                         typename E::T *grad_g, int B, int H, int W, int Ck, int Cv, int q_cs, int k_cs, int v_cs, int g_cs, int go_cs,
                         int gq_cs, int gk_cs, int gv_cs, int gg_cs, void *workspace, long long workspace_bytes, m3d_stream_t stream)
{
    const char *name = E::bwd_name;
    M3D_REQUIRE(q && k && v && g && grad_out, "%s: null pointer", name);
    int rc = anab_check<E>(name, B, H, W, Ck, Cv, workspace, workspace_bytes, 1);
    if (rc != M3D_OK) return rc;
    M3D_REQUIRE(q_cs >= Ck && k_cs >= Ck && v_cs >= Cv && g_cs >= 4 && go_cs >= Cv, "%s: a row stride is below its channel count", name);
    M3D_REQUIRE((!grad_q || gq_cs >= Ck) && (!grad_k || gk_cs >= Ck) && (!grad_v || gv_cs >= Cv) && (!grad_g || gg_cs >= 4),
                "%s: a gradient's row stride is below its channel count", name);
    if ((rc = E::check_backward_views(q, q_cs, k, k_cs, v, v_cs, g, g_cs, grad_out, go_cs)) != M3D_OK) return rc;
    if (!grad_q && !grad_k && !grad_v && !grad_g) return M3D_OK;
    const hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    AnabBwdArgs<E> a = {};
    float *dkv = nullptr;
    if ((rc = E::begin_backward(a, dkv, workspace, k, k_cs, v, v_cs, g, g_cs, B, H, W, Ck, Cv, stream)) != M3D_OK) return rc;
    // dkhat feeds grad_k and grad_g, dvhat feeds grad_v and grad_g; the statistics of the pixel-major kernel feed both
    const bool do_k = grad_k || grad_g, do_v = grad_v || grad_g;
    a.q = q; a.go = grad_out; a.gq = grad_q;
    a.q_cs = q_cs; a.go_cs = go_cs; a.gq_cs = gq_cs; a.HW = HW; a.Cv = Cv; a.need_dq = grad_q ? 1 : 0;
    if (Cv == 256) anab_launch_main<E, 168, 256>(a, B, do_k, do_v, st);
    else if (Ck == 168) anab_launch_main<E, 168, 128>(a, B, do_k, do_v, st);
    else if (Ck == 128) anab_launch_main<E, 128, 128>(a, B, do_k, do_v, st);
    else anab_launch_main<E, 64, 128>(a, B, do_k, do_v, st);
    M3D_LAUNCH_CHECK();
    if (!do_k && !do_v) return M3D_OK;
    {
        const long long total = (long long)B * AT_KEYS * (Ck + Cv);
        hipLaunchKernelGGL(anab_bwd_reduce_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, a.partK, a.partV, dkv, a.nch,
                           (Ck + 31) / 32 * 32, Ck, Cv, H, W, do_k ? 1 : 0, do_v ? 1 : 0, total);
        M3D_LAUNCH_CHECK();
    }
    AnabGatherArgs<E> ga;
    ga.k = k; ga.v = v; ga.g = g; ga.dkv = dkv; ga.gk = grad_k; ga.gv = grad_v; ga.gg = grad_g;
    ga.k_cs = k_cs; ga.v_cs = v_cs; ga.g_cs = g_cs; ga.gk_cs = gk_cs; ga.gv_cs = gv_cs; ga.gg_cs = gg_cs;
    ga.H = H; ga.W = W; ga.Ck = Ck; ga.Cv = Cv; ga.do_k = do_k ? 1 : 0; ga.do_v = do_v ? 1 : 0;
    ga.pixels = (long long)B * HW;
    hipLaunchKernelGGL(anab_bwd_gather_kernel<E>, dim3(cdiv(ga.pixels, 4)), dim3(256), 0, st, ga);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

// ---- fp32 only: the forward goes through the engine's pooling and attention launches (csrc/anab_attend.hip), which the bf16 operator
// does not use; its workspace is counted in floats and holds their scratch, work items and bin tables ------------------------------------
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
    if (!anab_supported(B, H, W, Ck, Cv)) return -1;
    const AtLayout L = at_layout(B, H, W, Ck, Cv);
    return (backward ? L.bwd_end : L.fwd_end) * 4;
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
    int rc = anab_check<AnabF32>("anab_attention_forward", B, H, W, Ck, Cv, workspace, workspace_bytes, 0);
    if (rc != M3D_OK) return rc;
    M3D_REQUIRE(k_cs >= Ck && v_cs >= Cv && g_cs >= 4 && out_cs >= Cv, "anab_attention_forward: a row stride is below its channel count");
    const AtLayout L = at_layout(B, H, W, Ck, Cv);
    float *ws = static_cast<float *>(workspace);
    rc = at_pool(L, ws, k, k_cs, v, v_cs, g, g_cs, B, H, W, Ck, Cv, false, stream);
    if (rc != M3D_OK) return rc;
    return m3d_anab_attend_f32(q, q_cs, ws + L.khat, L.CAP, ws + L.vhatT, B, H * W, Ck, AT_KEYS, AT_KPAD, Cv, nullptr, 0, 0, nullptr,
                               nullptr, 0, out, out_cs, stream);
}

int AnabF32::check_backward_views(const float *q, int q_cs, const float *, int, const float *, int, const float *, int,
                                  const float *grad_out, int go_cs)
{
    M3D_REQUIRE(q_cs % 4 == 0 && go_cs % 4 == 0 && (((uintptr_t)q | (uintptr_t)grad_out) & 15) == 0,
                "anab_attention_backward: q and grad_out must be 16-byte aligned views with row strides that are multiples of 4 floats");
    return M3D_OK;
}

// the pooling of the forward again (only khat zeroed first), then vhat^T transposed to vhat [key][Cv]
int AnabF32::begin_backward(AnabBwdArgs<AnabF32> &a, float *&dkv, void *workspace, const float *k, int k_cs, const float *v, int v_cs,
                            const float *g, int g_cs, int B, int H, int W, int Ck, int Cv, m3d_stream_t stream)
{
    const AtLayout L = at_layout(B, H, W, Ck, Cv);
    float *ws = static_cast<float *>(workspace);
    const int rc = at_pool(L, ws, k, k_cs, v, v_cs, g, g_cs, B, H, W, Ck, Cv, true, stream);
    if (rc != M3D_OK) return rc;
    const long long total = (long long)B * AT_KPAD * Cv;
    hipLaunchKernelGGL(anab_vhat_rows_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, ws + L.vhatT, ws + L.vhat, Cv,
                       total);
    M3D_LAUNCH_CHECK();
    a.khat = ws + L.khat; a.vhat = ws + L.vhat; a.stats = ws + L.stats; a.partK = ws + L.partK; a.partV = ws + L.partV; a.nch = L.nch;
    dkv = ws + L.dkv;
    return M3D_OK;
}

extern "C" int m3d_anab_attention_backward(const float *q, const float *k, const float *v, const float *g, const float *grad_out,
                                           float *grad_q, float *grad_k, float *grad_v, float *grad_g, int B, int H, int W, int Ck,
                                           int Cv, int q_cs, int k_cs, int v_cs, int g_cs, int go_cs, int gq_cs, int gk_cs, int gv_cs,
                                           int gg_cs, void *workspace, long long workspace_bytes, m3d_stream_t stream)
{
    return anab_backward<AnabF32>(q, k, v, g, grad_out, grad_q, grad_k, grad_v, grad_g, B, H, W, Ck, Cv, q_cs, k_cs, v_cs, g_cs, go_cs,
                                  gq_cs, gk_cs, gv_cs, gg_cs, workspace, workspace_bytes, stream);
}

// ---- bf16 only: a pooling kernel that writes khat, vhat and both transposes in bf16 (the fp32 pooling launches write fp32) and a
// one-pass forward kernel; the workspace is counted in bytes and starts with those four blocks ------------------------------------------
struct Anab16FwdArgs {
    const bf16_t *q, *khat, *vhatT;      // khat [B][352][CAP], vhat^T [B][Cv][352]
    bf16_t *out;
    int q_cs, out_cs, HW, Cv;
};

// grid = (pixel tiles of 128 over the batch, Cv / 128 value slices).  Pixel-major (a lane = one pixel that holds its q row as MFMA B
// fragments), keys in tiles of 32 through LDS, one pass with a running maximum.  S has rows = keys and columns = pixels, so
// exp(S - m) in registers IS the B operand of O^T += vhat_tile^T . P.
template <int CA>
__global__ __launch_bounds__(256) void anab16_fwd_kernel(const Anab16FwdArgs a)
{
    typedef AnabBf16 E;
    constexpr int CAP = (CA + 31) / 32 * 32, NG = (CA + 15) / 16;
    constexpr int KROW = CAP * 2 + 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[32 * KROW + 128 * E::TROW];
    unsigned char *Ks = lds, *VsT = lds + 32 * KROW;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.x / (a.HW / 128), cv0 = blockIdx.y * 128;
    const size_t mq = (size_t)blockIdx.x * 128 + wave * 32 + l31;        // this lane's pixel (linear over the batch)

    bf16x8 qf[NG];
    E::own_row<CA>(a.q + mq * a.q_cs, qf, lh);
    const bf16_t *kimg = a.khat + (size_t)img * AT_KPAD * CAP, *vimg = a.vhatT + ((size_t)img * a.Cv + cv0) * AT_KPAD;

    f32x16 o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[j][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int t = 0; t < AT_KPAD / 32; ++t) {
        __syncthreads();
        E::stage<CAP, CAP, true, false>(kimg + (size_t)32 * t * CAP, CAP, Ks, nullptr, tid);
        E::stage_cols<128>(vimg + 32 * t, VsT, tid);
        __syncthreads();
        f32x16 s = E::rows_mm<NG, KROW>(Ks, qf, l31, lh);
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
        E::acc_mm<4>(VsT, e, o, l31, lh);
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    bf16_t *op = a.out + mq * a.out_cs + cv0;
    const bool al8 = E::store4_aligned(a.out, a.out_cs);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            E::store4(op + 32 * j + 8 * i + 4 * lh, o[j][4 * i] * inv, o[j][4 * i + 1] * inv, o[j][4 * i + 2] * inv, o[j][4 * i + 3] * inv, al8);
}

struct Anab16PoolArgs {
    const bf16_t *k, *v, *g;
    bf16_t *khat, *khatT, *vhat, *vhatT;
    int k_cs, v_cs, g_cs, H, W, Ck, Cv, CAP, nsk;                 // nsk: 128-channel slabs of K (the slabs of V follow)
};

// grid = (337 bins, images, slabs of 128 channels of K then V); 16 waves, lane = a channel pair.  Wave w sums pixels w, w + 16, ...
// of the window (row-major inside the window), the sixteen partial sums are added in wave order: fixed, whatever the launch.
// Serves nested and overlapping windows alike.
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
    L.nch = (int)((HW / 32 + AT_CHUNK_TILES - 1) / AT_CHUNK_TILES);
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
    if (!anab_supported(B, H, W, Ck, Cv)) return -1;
    const AbLayout L = ab_layout(B, H, W, Ck, Cv);
    return backward ? L.bwd_end : L.fwd_end;
}

// q / grad_out: 16-byte loads; k / v: 4-byte loads of channel pairs
static bool ab_rows16(const void *p, int cs) { return ((uintptr_t)p & 15) == 0 && cs % 8 == 0; }
static bool ab_rows4(const void *p, int cs) { return ((uintptr_t)p & 3) == 0 && cs % 2 == 0; }

// khat, khat^T, vhat, vhat^T (bf16, zero padded) into the first four blocks of the workspace, all four zeroed first
static int ab_pool(const AbLayout &L, unsigned char *ws, const bf16_t *k, int k_cs, const bf16_t *v, int v_cs, const bf16_t *g, int g_cs,
                   int B, int H, int W, int Ck, int Cv, hipStream_t st)
{
    M3D_HIP(hipMemsetAsync(ws, 0, (size_t)L.fwd_end, st));
    Anab16PoolArgs pa;
    pa.k = k; pa.v = v; pa.g = g;
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
    int rc = anab_check<AnabBf16>(name, B, H, W, Ck, Cv, workspace, workspace_bytes, 0);
    if (rc != M3D_OK) return rc;
    M3D_REQUIRE(q_cs >= Ck && k_cs >= Ck && v_cs >= Cv && g_cs >= 4 && out_cs >= Cv, "%s: a row stride is below its channel count", name);
    M3D_REQUIRE(ab_rows16(q, q_cs), "%s: q must be a 16-byte aligned view with a row stride that is a multiple of 8 elements", name);
    M3D_REQUIRE(ab_rows4(k, k_cs) && ab_rows4(v, v_cs) && ab_rows4(g, g_cs),
                "%s: k, v and g must be 4-byte aligned views with even row strides", name);
    const hipStream_t st = (hipStream_t)stream;
    const AbLayout L = ab_layout(B, H, W, Ck, Cv);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    rc = ab_pool(L, ws, (const bf16_t *)k, k_cs, (const bf16_t *)v, v_cs, (const bf16_t *)g, g_cs, B, H, W, Ck, Cv, st);
    if (rc != M3D_OK) return rc;
    Anab16FwdArgs a;
    a.q = (const bf16_t *)q; a.khat = (const bf16_t *)(ws + L.khat); a.vhatT = (const bf16_t *)(ws + L.vhatT);
    a.out = (bf16_t *)out; a.q_cs = q_cs; a.out_cs = out_cs; a.HW = H * W; a.Cv = Cv;
    const dim3 grid(B * (a.HW / 128), Cv / 128);
    if (Ck == 168) hipLaunchKernelGGL((anab16_fwd_kernel<168>), grid, dim3(256), 0, st, a);
    else if (Ck == 128) hipLaunchKernelGGL((anab16_fwd_kernel<128>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((anab16_fwd_kernel<64>), grid, dim3(256), 0, st, a);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

int AnabBf16::check_backward_views(const bf16_t *q, int q_cs, const bf16_t *k, int k_cs, const bf16_t *v, int v_cs, const bf16_t *g,
                                   int g_cs, const bf16_t *grad_out, int go_cs)
{
    M3D_REQUIRE(ab_rows16(q, q_cs) && ab_rows16(grad_out, go_cs),
                "%s: q and grad_out must be 16-byte aligned views with row strides that are multiples of 8 elements", bwd_name);
    M3D_REQUIRE(ab_rows4(k, k_cs) && ab_rows4(v, v_cs) && ab_rows4(g, g_cs),
                "%s: k, v and g must be 4-byte aligned views with even row strides", bwd_name);
    return M3D_OK;
}

int AnabBf16::begin_backward(AnabBwdArgs<AnabBf16> &a, float *&dkv, void *workspace, const bf16_t *k, int k_cs, const bf16_t *v, int v_cs,
                             const bf16_t *g, int g_cs, int B, int H, int W, int Ck, int Cv, m3d_stream_t stream)
{
    const AbLayout L = ab_layout(B, H, W, Ck, Cv);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const int rc = ab_pool(L, ws, k, k_cs, v, v_cs, g, g_cs, B, H, W, Ck, Cv, (hipStream_t)stream);
    if (rc != M3D_OK) return rc;
    a.khat = (const bf16_t *)(ws + L.khat); a.khatT = (const bf16_t *)(ws + L.khatT); a.vhat = (const bf16_t *)(ws + L.vhat);
    a.stats = (float *)(ws + L.stats); a.partK = (float *)(ws + L.partK); a.partV = (float *)(ws + L.partV); a.nch = L.nch;
    dkv = (float *)(ws + L.dkv);
    return M3D_OK;
}

extern "C" int m3d_anab_attention_backward_bf16(const void *q, const void *k, const void *v, const void *g, const void *grad_out,
                                                void *grad_q, void *grad_k, void *grad_v, void *grad_g, int B, int H, int W, int Ck,
                                                int Cv, int q_cs, int k_cs, int v_cs, int g_cs, int go_cs, int gq_cs, int gk_cs,
                                                int gv_cs, int gg_cs, void *workspace, long long workspace_bytes, m3d_stream_t stream)
{
    typedef bf16_t T;
    return anab_backward<AnabBf16>((const T *)q, (const T *)k, (const T *)v, (const T *)g, (const T *)grad_out, (T *)grad_q, (T *)grad_k,
                                   (T *)grad_v, (T *)grad_g, B, H, W, Ck, Cv, q_cs, k_cs, v_cs, g_cs, go_cs, gq_cs, gk_cs, gv_cs, gg_cs,
                                   workspace, workspace_bytes, stream);
}
