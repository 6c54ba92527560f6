// The optimizer step on the device: SGD (momentum, weight decay), Adam and Adamax -- the three solvers lib/core.py:76-99 can
// build -- over a whole parameter set in one streaming pass, preceded by one pass over the gradients that takes the decision the
// reference's loop takes on the host (scripts/train_rpn_3d.py:208-218: step only `if total_loss > 0`).
//
// The parameter set is a TENSOR TABLE resident on the device (built by m3dssd_amd/host/optim.py once per set of pointers):
// `OptEntry` per tensor, and a CHUNK LIST of (entry, chunk index inside the tensor).  A chunk is M3D_OPTIM_CHUNK consecutive
// elements (the last one of a tensor may be shorter); one workgroup handles one chunk, grid-striding over the list.  The list is a
// function of the table alone, so nothing a kernel computes depends on the launch geometry.
//
//   m3d_optim_prepare   optim_gradsq_kernel: per chunk the sum of g*g in float64 and the count of non-finite g.  Every thread adds
//                       its elements in a fixed order, the 256 thread sums are combined by a fixed tree in LDS.  No atomics.
//                       optim_finish_kernel (one workgroup): thread i adds the partials of the chunks [i*per, (i+1)*per) in chunk
//                       order, the same tree combines the 256 sums; thread 0 then decides `do_step` (loss > 0 when a loss is
//                       given -- false for NaN --, and no non-finite gradient when skip_nonfinite), and, when the step is taken,
//                       advances t and the running products beta1^t, beta2^t (float64, one multiplication each, no pow) and
//                       derives the float32 scalars of the step from them (float64 arithmetic, rounded once).
//   m3d_optim_step      optim_step_kernel<KIND>: returns at once when do_step is clear; else p, the state and (zero_grads) g in place.
//
// The arithmetic is FIXED (tests/optim_ref.py is the contract, float32, one correctly rounded operation per line, the order of
// torch's single-tensor implementations):
//   all     g += wd*p                                   (skipped for wd == 0)
//   SGD     buf = g on the first taken step, else buf = momentum*buf + g;   p += (-lr)*buf        (momentum 0: p += (-lr)*g)
//   Adam    m += (1-beta1)*(g-m);  v = beta2*v + (1-beta2)*(g*g);  denom = sqrt(v)/sqrt(bc2) + eps;  p += (-(lr/bc1))*(m/denom)
//   Adamax  m += (1-beta1)*(g-m);  u = max(beta2*u, |g|+eps) (a NaN operand gives NaN, as torch.maximum);  p += (-(lr/bc1))*(m/u)
// Denormal inputs and NaN payloads are outside the contract.
#include <math.h>
#include <stdint.h>

#include "common.h"

// every expression in this file is evaluated as written: no fma contraction.  `/` and sqrtf are hipcc's correctly rounded forms
// (its default, -fhip-fp32-correctly-rounded-divide-sqrt); the __f*_rn intrinsics are NOT used: in this toolchain they are plain
// operators inside a header (contractable there) and __fsqrt_rn is the native, not correctly rounded, square root.
#pragma clang fp contract(off)

#define OPT_NT 256
#define OPT_VEC 4
#define OPT_ITERS (M3D_OPTIM_CHUNK / (OPT_NT * OPT_VEC))
static_assert(M3D_OPTIM_CHUNK % (OPT_NT * OPT_VEC) == 0, "a chunk is a whole number of 16-byte accesses per thread");

struct OptEntry {               // M3D_OPTIM_ENTRY_BYTES; s0: momentum_buffer / exp_avg, s1: exp_avg_sq / exp_inf (null: unused)
    float *p, *g, *s0, *s1;
    long long numel;
    int group, pad_;
};
static_assert(sizeof(OptEntry) == M3D_OPTIM_ENTRY_BYTES, "table entry layout");
struct OptChunk { int entry, index; };          // elements [index * M3D_OPTIM_CHUNK, ...) of table[entry]
struct OptState {               // the head of the state block (M3D_OPTIM_STATE_* are its byte offsets); the partials follow it
    double grad_sq_sum;
    long long grad_nonfinite;
    int do_step, pad_;
    long long t;
    double prod1[M3D_OPTIM_MAX_GROUPS], prod2[M3D_OPTIM_MAX_GROUPS];
    float bc1[M3D_OPTIM_MAX_GROUPS], bc2_sqrt[M3D_OPTIM_MAX_GROUPS], step_size[M3D_OPTIM_MAX_GROUPS];
};
static_assert(offsetof(OptState, grad_sq_sum) == M3D_OPTIM_STATE_GRAD_SQ_SUM && offsetof(OptState, grad_nonfinite) == M3D_OPTIM_STATE_NONFINITE &&
              offsetof(OptState, do_step) == M3D_OPTIM_STATE_DO_STEP && offsetof(OptState, t) == M3D_OPTIM_STATE_T &&
              offsetof(OptState, prod1) == M3D_OPTIM_STATE_PROD1 && offsetof(OptState, prod2) == M3D_OPTIM_STATE_PROD2 &&
              offsetof(OptState, bc1) == M3D_OPTIM_STATE_BC1 && offsetof(OptState, bc2_sqrt) == M3D_OPTIM_STATE_BC2_SQRT &&
              offsetof(OptState, step_size) == M3D_OPTIM_STATE_STEP_SIZE && sizeof(OptState) == M3D_OPTIM_STATE_HEAD_BYTES,
              "state block layout");

struct OptPrepArgs {            // what the finish needs of the groups, in float64 as the host holds it
    double lr[M3D_OPTIM_MAX_GROUPS], beta1[M3D_OPTIM_MAX_GROUPS], beta2[M3D_OPTIM_MAX_GROUPS];
    int n_groups, kind;
};
struct OptGroup { float neg_lr, momentum, wd, omb1, beta2, omb2, eps; };          // the float64 settings rounded once, on the host
struct OptStepArgs { OptGroup g[M3D_OPTIM_MAX_GROUPS]; };

__device__ __forceinline__ double *opt_part_sq(void *state) { return (double *)((char *)state + M3D_OPTIM_STATE_HEAD_BYTES); }
__device__ __forceinline__ unsigned *opt_part_nf(void *state, int n_chunks) { return (unsigned *)(opt_part_sq(state) + n_chunks); }

// sum of the OPT_NT values (fixed tree: the result does not depend on which wave runs first); the total is returned to thread 0
__device__ __forceinline__ void opt_block_sum(double &sq, unsigned &nf, double *s_sq, unsigned *s_nf)
{
    const int tid = threadIdx.x;
    s_sq[tid] = sq;
    s_nf[tid] = nf;
    __syncthreads();
    for (int s = OPT_NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            s_sq[tid] = s_sq[tid] + s_sq[tid + s];
            s_nf[tid] = s_nf[tid] + s_nf[tid + s];
        }
        __syncthreads();
    }
    sq = s_sq[0];
    nf = s_nf[0];
    __syncthreads();            // the arrays are written again by the next chunk
}

__device__ __forceinline__ void opt_acc(float x, double &sq, unsigned &nf)
{
    const double d = (double)x;
    sq = sq + d * d;
    nf += (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

__global__ __launch_bounds__(OPT_NT) void optim_gradsq_kernel(const OptEntry *table, const OptChunk *chunks, int n_chunks, void *state)
{
    __shared__ double s_sq[OPT_NT];
    __shared__ unsigned s_nf[OPT_NT];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptEntry e = table[ck.entry];
        const long long off = (long long)ck.index * M3D_OPTIM_CHUNK;
        const int n = (int)min((long long)M3D_OPTIM_CHUNK, e.numel - off);
        const float *g = e.g + off;
        const bool vec = ((uintptr_t)g & 15) == 0;
        double sq = 0.0;
        unsigned nf = 0;
#pragma unroll
        for (int k = 0; k < OPT_ITERS; ++k) {
            const int i = (k * OPT_NT + tid) * OPT_VEC;
            if (vec && i + OPT_VEC <= n) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(g + i);
#pragma unroll
                for (int j = 0; j < OPT_VEC; ++j) opt_acc(v[j], sq, nf);
            } else {
                for (int j = 0; j < OPT_VEC; ++j)
                    if (i + j < n) opt_acc(g[i + j], sq, nf);
            }
        }
        opt_block_sum(sq, nf, s_sq, s_nf);
        if (tid == 0) {
            opt_part_sq(state)[c] = sq;
            opt_part_nf(state, n_chunks)[c] = nf;
        }
    }
}

__global__ __launch_bounds__(OPT_NT) void optim_finish_kernel(int n_chunks, const float *loss, int skip_nonfinite, void *state, OptPrepArgs a)
{
    __shared__ double s_sq[OPT_NT];
    __shared__ unsigned s_nf[OPT_NT];
    __shared__ unsigned long long s_cnt[OPT_NT];
    const int tid = threadIdx.x;
    const int per = (n_chunks + OPT_NT - 1) / OPT_NT;
    const double *psq = opt_part_sq(state);
    const unsigned *pnf = opt_part_nf(state, n_chunks);
    double sq = 0.0;
    unsigned long long cnt = 0;
    for (int c = tid * per; c < min(n_chunks, (tid + 1) * per); ++c) {
        sq = sq + psq[c];
        cnt += pnf[c];
    }
    // the counts do not fit 32 bits for more than 2^32 elements: they are combined as 64-bit integers (order irrelevant)
    s_cnt[tid] = cnt;
    unsigned dummy = 0;
    opt_block_sum(sq, dummy, s_sq, s_nf);
    if (tid != 0) return;
    for (int i = 1; i < OPT_NT; ++i) cnt += s_cnt[i];
    OptState *st = (OptState *)state;
    st->grad_sq_sum = sq;
    st->grad_nonfinite = (long long)cnt;
    int go = 1;
    if (loss) go = *loss > 0.0f;                         // false for NaN, as the reference's host comparison
    if (skip_nonfinite) go = go && cnt == 0;
    st->do_step = go;
    if (!go) return;                                     // t, the products and the derived scalars keep their bits
    st->t = st->t + 1;
    if (a.kind == 0) return;
    for (int g = 0; g < a.n_groups; ++g) {
        const double p1 = st->prod1[g] * a.beta1[g], p2 = st->prod2[g] * a.beta2[g];
        st->prod1[g] = p1;
        st->prod2[g] = p2;
        const double bc1 = 1.0 - p1, bc2 = 1.0 - p2;
        st->bc1[g] = (float)bc1;
        st->bc2_sqrt[g] = (float)sqrt(bc2);
        st->step_size[g] = (float)(a.lr[g] / bc1);
    }
}

// torch.maximum / numpy.maximum: a NaN operand gives NaN (fmaxf would return the other operand)
__device__ __forceinline__ float opt_max_nan(float a, float b) { return a != a ? a : b != b ? b : fmaxf(a, b); }

struct OptScalars { float neg_lr, momentum, wd, omb1, beta2, omb2, eps, bc2_sqrt, neg_step; bool first; };

// one element; s0 / s1 are read and written only where the solver has them
template <int KIND, bool HAS_BUF>
__device__ __forceinline__ void opt_update(float &p, float g, float &s0, float &s1, const OptScalars &c)
{
    if (c.wd != 0.0f) g = g + c.wd * p;
    if (KIND == 0) {
        if (HAS_BUF) {
            s0 = c.first ? g : c.momentum * s0 + g;
            g = s0;
        }
        p = p + c.neg_lr * g;
    } else {
        s0 = s0 + c.omb1 * (g - s0);
        if (KIND == 1) {
            s1 = c.beta2 * s1 + c.omb2 * (g * g);
            const float denom = sqrtf(s1) / c.bc2_sqrt + c.eps;
            p = p + c.neg_step * (s0 / denom);
        } else {
            s1 = opt_max_nan(c.beta2 * s1, fabsf(g) + c.eps);
            p = p + c.neg_step * (s0 / s1);
        }
    }
}

__device__ __forceinline__ void opt_store4(float *q, f32x4 v) { global_store_u32x4_nop(q, __builtin_bit_cast(u32x4, v)); }

template <int KIND, bool HAS_BUF>
__device__ __forceinline__ void opt_chunk(const OptEntry &e, long long off, int n, const OptScalars &c, int zero_grads)
{
    constexpr bool S0 = KIND != 0 || HAS_BUF, S1 = KIND != 0;
    const int tid = threadIdx.x;
    float *p = e.p + off, *g = e.g + off, *s0 = S0 ? e.s0 + off : nullptr, *s1 = S1 ? e.s1 + off : nullptr;
    // 16-byte accesses where every pointer of the tensor allows them (a chunk offset is a multiple of 16 bytes)
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1) & 15) == 0;
#pragma unroll
    for (int k = 0; k < OPT_ITERS; ++k) {
        const int i = (k * OPT_NT + tid) * OPT_VEC;
        if (i >= n) break;
        if (vec && i + OPT_VEC <= n) {
            f32x4 vp = *reinterpret_cast<const f32x4 *>(p + i);
            const f32x4 vg = *reinterpret_cast<const f32x4 *>(g + i);
            f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
            if (S0) v0 = *reinterpret_cast<const f32x4 *>(s0 + i);
            if (S1) v1 = *reinterpret_cast<const f32x4 *>(s1 + i);
#pragma unroll
            for (int j = 0; j < OPT_VEC; ++j) {
                float a = vp[j], b0 = v0[j], b1 = v1[j];
                opt_update<KIND, HAS_BUF>(a, vg[j], b0, b1, c);
                vp[j] = a; v0[j] = b0; v1[j] = b1;
            }
            opt_store4(p + i, vp);
            if (S0) opt_store4(s0 + i, v0);
            if (S1) opt_store4(s1 + i, v1);
            if (zero_grads) opt_store4(g + i, f32x4{0.f, 0.f, 0.f, 0.f});
        } else {
            for (int j = 0; j < OPT_VEC && i + j < n; ++j) {
                float a = p[i + j], b0 = S0 ? s0[i + j] : 0.f, b1 = S1 ? s1[i + j] : 0.f;
                opt_update<KIND, HAS_BUF>(a, g[i + j], b0, b1, c);
                p[i + j] = a;
                if (S0) s0[i + j] = b0;
                if (S1) s1[i + j] = b1;
                if (zero_grads) g[i + j] = 0.f;
            }
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(OPT_NT) void optim_step_kernel(const OptEntry *table, const OptChunk *chunks, int n_chunks, int zero_grads,
                                                            const void *state, OptStepArgs a)
{
    const OptState *st = (const OptState *)state;
    if (!st->do_step) return;                   // not a byte of parameters, state or gradients is written
    const bool first = st->t == 1;              // the finish has counted this step already
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptEntry e = table[ck.entry];
        const long long off = (long long)ck.index * M3D_OPTIM_CHUNK;
        const int n = (int)min((long long)M3D_OPTIM_CHUNK, e.numel - off);
        const OptGroup &h = a.g[e.group];
        OptScalars s;
        s.neg_lr = h.neg_lr; s.momentum = h.momentum; s.wd = h.wd; s.omb1 = h.omb1; s.beta2 = h.beta2; s.omb2 = h.omb2; s.eps = h.eps;
        s.bc2_sqrt = KIND == 1 ? st->bc2_sqrt[e.group] : 1.f;
        s.neg_step = KIND != 0 ? -st->step_size[e.group] : 0.f;
        s.first = first;
        if (KIND == 0 && e.s0 == nullptr) opt_chunk<KIND, false>(e, off, n, s, zero_grads);     // momentum 0: no buffer
        else opt_chunk<KIND, true>(e, off, n, s, zero_grads);
    }
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" long long m3d_optim_state_bytes(int n_chunks)
{
    if (n_chunks < 0) return -1;
    // head, float64 partial per chunk, 32-bit count per chunk, rounded up to 16 bytes
    return ((long long)M3D_OPTIM_STATE_HEAD_BYTES + (long long)n_chunks * 12 + 15) / 16 * 16;
}

static int opt_check(const char *who, const void *table, int n_entries, const void *chunks, int n_chunks, int kind, const double *hyper,
                     int n_groups, const void *state, long long state_bytes)
{
    M3D_REQUIRE(table && chunks && hyper && state, "%s: null pointer", who);
    M3D_REQUIRE(n_entries >= 0 && n_chunks >= 0, "%s: bad sizes (%d entries, %d chunks)", who, n_entries, n_chunks);
    M3D_REQUIRE(n_entries > 0 || n_chunks == 0, "%s: %d chunks of an empty table", who, n_chunks);
    M3D_REQUIRE(kind >= 0 && kind <= 2, "%s: kind %d (0 SGD, 1 Adam, 2 Adamax)", who, kind);
    M3D_REQUIRE(n_groups >= 1 && n_groups <= M3D_OPTIM_MAX_GROUPS, "%s: %d parameter groups (1 .. %d)", who, n_groups, M3D_OPTIM_MAX_GROUPS);
    M3D_REQUIRE((((uintptr_t)table | (uintptr_t)chunks) & 7) == 0 && ((uintptr_t)state & 15) == 0,
                "%s: the table and the chunk list must be 8-byte, the state block 16-byte aligned", who);
    M3D_REQUIRE(state_bytes >= m3d_optim_state_bytes(n_chunks), "%s: state block of %lld bytes; %d chunks need %lld", who, state_bytes,
                n_chunks, m3d_optim_state_bytes(n_chunks));
    for (int g = 0; g < n_groups; ++g) {
        const double *h = hyper + (size_t)g * M3D_OPTIM_HYPER_COLS;
        for (int k = 0; k < M3D_OPTIM_HYPER_COLS; ++k) M3D_REQUIRE(isfinite(h[k]), "%s: group %d: setting %d is not finite", who, g, k);
        M3D_REQUIRE(h[1] >= 0 && h[2] >= 0 && h[5] >= 0, "%s: group %d: negative momentum, weight_decay or eps", who, g);
        if (kind != 0) M3D_REQUIRE(h[3] >= 0 && h[3] < 1 && h[4] >= 0 && h[4] < 1, "%s: group %d: betas (%g, %g) outside [0, 1)", who, g, h[3], h[4]);
    }
    return M3D_OK;
}

static int opt_grid(int n_chunks) { return imin(n_chunks, m3d_cu_count() * 8); }

extern "C" int m3d_optim_prepare(const void *table, int n_entries, const void *chunks, int n_chunks, int kind, const double *hyper,
                                 int n_groups, const float *loss, int skip_nonfinite, void *state, long long state_bytes,
                                 m3d_stream_t stream)
{
    const int rc = opt_check("optim_prepare", table, n_entries, chunks, n_chunks, kind, hyper, n_groups, state, state_bytes);
    if (rc != M3D_OK) return rc;
    M3D_REQUIRE(((uintptr_t)loss & 3) == 0, "optim_prepare: the loss pointer must be 4-byte aligned");
    OptPrepArgs a = {};
    a.n_groups = n_groups;
    a.kind = kind;
    for (int g = 0; g < n_groups; ++g) {
        const double *h = hyper + (size_t)g * M3D_OPTIM_HYPER_COLS;
        a.lr[g] = h[0]; a.beta1[g] = h[3]; a.beta2[g] = h[4];
    }
    if (n_chunks > 0) {
        hipLaunchKernelGGL(optim_gradsq_kernel, dim3(opt_grid(n_chunks)), dim3(OPT_NT), 0, (hipStream_t)stream, (const OptEntry *)table,
                           (const OptChunk *)chunks, n_chunks, state);
        M3D_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(OPT_NT), 0, (hipStream_t)stream, n_chunks, loss, skip_nonfinite, state, a);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}

extern "C" int m3d_optim_step(const void *table, int n_entries, const void *chunks, int n_chunks, int kind, const double *hyper,
                              int n_groups, int zero_grads, void *state, long long state_bytes, m3d_stream_t stream)
{
    const int rc = opt_check("optim_step", table, n_entries, chunks, n_chunks, kind, hyper, n_groups, state, state_bytes);
    if (rc != M3D_OK) return rc;
    if (n_chunks == 0) return M3D_OK;
    OptStepArgs a = {};
    for (int g = 0; g < n_groups; ++g) {
        const double *h = hyper + (size_t)g * M3D_OPTIM_HYPER_COLS;
        OptGroup &o = a.g[g];
        o.neg_lr = (float)-h[0]; o.momentum = (float)h[1]; o.wd = (float)h[2];
        o.omb1 = (float)(1.0 - h[3]); o.beta2 = (float)h[4]; o.omb2 = (float)(1.0 - h[4]); o.eps = (float)h[5];
    }
    const dim3 grid(opt_grid(n_chunks)), block(OPT_NT);
    const OptEntry *t = (const OptEntry *)table;
    const OptChunk *c = (const OptChunk *)chunks;
    if (kind == 0) hipLaunchKernelGGL(optim_step_kernel<0>, grid, block, 0, (hipStream_t)stream, t, c, n_chunks, zero_grads, (const void *)state, a);
    else if (kind == 1) hipLaunchKernelGGL(optim_step_kernel<1>, grid, block, 0, (hipStream_t)stream, t, c, n_chunks, zero_grads, (const void *)state, a);
    else hipLaunchKernelGGL(optim_step_kernel<2>, grid, block, 0, (hipStream_t)stream, t, c, n_chunks, zero_grads, (const void *)state, a);
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}
