// Shared by csrc/anab_train.hip and csrc/anab_train_bf16.hip: the key order and windows of the ANAB pyramid (the AdaptiveAvgPool2d bins
// of sizes 1 / 4 / 8 / 16, scale-major) and the fixed-order sum of the key-major kernels' chunk partials.
#pragma once
#include "common.h"

#define AT_KEYS 337
#define AT_KPAD 352                      // keys padded to the tile of 32

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

// dkv [B][337][Ck + Cv] = (1 / area_bin) * sum over the pixel chunks, in chunk order, of the key-major kernel's
// partials [B][nch][352][CAP] and [B][nch][352][Cv]
static __global__ void anab_bwd_reduce_kernel(const float *__restrict__ partK, const float *__restrict__ partV, float *__restrict__ dkv,
                                              int nch, int CAP, int Ck, int Cv, int H, int W, int do_k, int do_v, long long total)
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
