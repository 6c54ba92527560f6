// libm3dssd_hip.so: error reporting, launcher state, events, source hashes, ABI version and the clock probe.
#include <stdlib.h>

#include "common.h"

static thread_local char g_err[512] = "";

void m3d_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *m3d_last_error(void) { return g_err; }

// ---- launcher state (common.h) ---------------------------------------------------------------------------------------------------
int m3d_env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

int m3d_raise_dyn_lds_(const void *kernel, int bytes, m3d_lds_state &state, const char *what, const char *file, int line)
{
    int dev = 0;
    M3D_HIP(hipGetDevice(&dev));
    const int err = *state.get(dev, [&]() {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) (void)hipGetLastError();
        return std::optional<int>((int)e);
    });
    if (err != (int)hipSuccess) {
        m3d_set_error("hipFuncSetAttribute(%s, hipFuncAttributeMaxDynamicSharedMemorySize, %d) failed: %s (%s:%d)", what, bytes,
                      hipGetErrorString((hipError_t)err), file, line);
        return M3D_E_HIP;
    }
    return M3D_OK;
}

int m3d_cu_count()
{
    static PerDevice<int> count;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;                  // no current device: no slot, the fallback
    return *count.get(dev, [&]() {
        int ncu = 0;
        if (dev < 0 || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) {
            (void)hipGetLastError();
            ncu = 256;
        }
        return std::optional<int>(ncu);
    });
}

int m3d_scratch_bytes_(const void *const *kernels, int n)
{
    long long sum = 0;
    for (int i = 0; i < n; ++i) {
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, kernels[i]) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
        sum += (long long)fa.localSizeBytes;
    }
    return (int)sum;
}
extern "C" int m3d_abi_version(void) { return M3D_ABI_VERSION; }
// "name:sha256[:16];..." of every source this library was built from (build/src_hash.h, written by the Makefile): lets a
// measurement taken with one build (profiles/*_hbm_traffic.json) be told apart from the build that is loaded now.
#include "build/src_hash.h"
extern "C" const char *m3d_source_hashes(void) { return M3D_SRC_HASHES; }

// ------------------------------------------------------------------------------------------
extern "C" int m3d_event_create(void **ev)
{
    hipEvent_t e;
    M3D_HIP(hipEventCreate(&e));
    *ev = (void *)e;
    return M3D_OK;
}
extern "C" int m3d_event_record(void *ev, m3d_stream_t stream)
{
    M3D_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return M3D_OK;
}
extern "C" int m3d_event_elapsed_ms(void *start, void *stop, float *ms)
{
    M3D_HIP(hipEventSynchronize((hipEvent_t)stop));
    M3D_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return M3D_OK;
}
extern "C" int m3d_event_destroy(void *ev)
{
    M3D_HIP(hipEventDestroy((hipEvent_t)ev));
    return M3D_OK;
}

// ------------------------------------------------------------------------------------------
// Shader clock the chip actually holds over a window (bench.py: `sclk_under_step_ghz`): ONE wave samples s_memtime (one tick per
// shader cycle) and s_memrealtime (constant 100 MHz) when it starts, sleeps until `ticks` of the 100 MHz clock have passed and
// samples both again; run on a side stream while the step replays on the main one, d(memtime) / d(realtime) x 100 MHz is the
// clock the MFMA peak of that window has to be priced at (the 157.3 TFLOP/s behind `roofline.frac` assume 2.4 GHz; under the fp32
// kernels the part holds 2.0-2.1 at ~1.2 kW: DESIGN.md).  out = {memtime0, realtime0, memtime1, realtime1}.
__global__ void clock_probe_kernel(long long *out, long long ticks)
{
    if (threadIdx.x != 0) return;
    const long long c0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
    long long r1 = r0;
    while (r1 - r0 < ticks) {
        __builtin_amdgcn_s_sleep(127);
        r1 = __builtin_amdgcn_s_memrealtime();
    }
    out[0] = c0; out[1] = r0; out[2] = __builtin_readcyclecounter(); out[3] = r1;
}

extern "C" int m3d_clock_probe(long long *out4_dev, double seconds, m3d_stream_t stream)
{
    M3D_REQUIRE(out4_dev && seconds > 0 && seconds <= 1.0, "clock_probe: bad arguments (window <= 1 s)");
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out4_dev, (long long)(seconds * 1e8));
    M3D_LAUNCH_CHECK();
    return M3D_OK;
}
