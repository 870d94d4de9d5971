// Stale-state probe (test infrastructure, tests/stale.py): kernels that put a known pattern into the WHOLE LDS of every CU, so that a product
// kernel launched next on the same stream meets poisoned on-chip memory instead of a fresh process's zeros or its own earlier data.
// LDS is not cleared between dispatches: a kernel that reads a cell it did not write on some path reads what these kernels left.
//
// Plain C ABI, every entry point takes the caller's stream.  The kernels touch nothing but their own dynamic LDS allocation and the caller's
// output arrays (one record per workgroup, bounds = the grid); the hold is a counted loop of s_sleep, bounded by its trip count -- no
// workgroup waits for another one.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int BLOCK = 256;
constexpr int LDS_CU = 160 * 1024;            // the LDS of a gfx950 CU
constexpr int LDS_FLOOR = 64 * 1024;          // granted to every kernel without asking: the fallback if the attribute is refused

extern __shared__ uint32_t lds[];

// XCC_ID[3:0] above HW_ID's SE / SH / CU fields (bits 15:8): one value per physical CU of the device
__device__ __forceinline__ uint32_t cu_id()
{
    const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20 /* HW_REG_XCC_ID */) & 0xF;
    const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4 /* HW_REG_HW_ID */);
    return (xcc << 8) | ((hw >> 8) & 0xFF);
}

__device__ __forceinline__ void hold(int sleeps)
{
    for (int i = 0; i < sleeps; ++i) __builtin_amdgcn_s_sleep(127);          // 127 x 64 clocks each; the trip count is the bound
}

__global__ __launch_bounds__(BLOCK) void poison_kernel(uint32_t pattern, int words, int sleeps, uint32_t *ids)
{
    volatile uint32_t *s = lds;
    for (int i = threadIdx.x; i < words; i += BLOCK) s[i] = pattern;
    __syncthreads();
    hold(sleeps);
    if (threadIdx.x == 0) ids[blockIdx.x] = cu_id();
}

// reads, never writes: per workgroup {CU id, words that still hold the pattern}; out arrives zeroed
__global__ __launch_bounds__(BLOCK) void canary_kernel(uint32_t pattern, int words, int sleeps, uint32_t *out)
{
    const volatile uint32_t *s = lds;
    uint32_t n = 0;
    for (int i = threadIdx.x; i < words; i += BLOCK) n += s[i] == pattern;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    hold(sleeps);
    if (threadIdx.x == 0) out[2 * blockIdx.x] = cu_id();
    if (threadIdx.x % 64 == 0) atomicAdd(&out[2 * blockIdx.x + 1], n);          // (the caller zeroed out)
}

// The toy op: 64 values through LDS plus ONE extra cell, s[64].  y[i] = x[i] + s[64] * 0 for i < 63 (a zero mask: NaN * 0 is NaN, but
// finite * 0 is 0) and y[63] = x[63] + fmaxf(s[64], 0) (fmaxf launders a NaN into 0, but a finite value passes): the two ways a stale cell
// reaches or misses a result, each seen by one pattern only.  The good kernel writes s[64] = 0 first, the bad one does not: on zeroed LDS
// both give y = x.
template <bool GOOD>
__global__ __launch_bounds__(64) void demo_kernel(const float *x, float *y)
{
    float *s = (float *)lds;
    const int i = threadIdx.x;
    s[i] = x[i];
    if (GOOD && i == 0) s[64] = 0.0f;
    __syncthreads();
    const float stale = ((volatile float *)s)[64];
    y[i] = i < 63 ? s[i] + stale * 0.0f : s[i] + fmaxf(stale, 0.0f);
}

int g_lds[64];          // per device: the dynamic size granted to the three full-LDS kernels (0 = not asked yet)

int lds_bytes()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (g_lds[dev]) return g_lds[dev];
    int got = LDS_FLOOR;
    for (int want = LDS_CU; want > LDS_FLOOR; want -= 16 * 1024) {          // the largest size all of them are granted
        if (hipFuncSetAttribute((const void *)poison_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess &&
            hipFuncSetAttribute((const void *)canary_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess) {
            got = want;
            break;
        }
        (void)hipGetLastError();
    }
    return g_lds[dev] = got;
}

int cu_count()
{
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    return n;
}

}  // namespace

extern "C" {

// the LDS bytes a poison workgroup fills and a canary workgroup reads
int stale_lds_bytes(void) { return lds_bytes(); }

// grid = multiple x CU count workgroups, each holding sleeps x s_sleep(127) (127 x 64 clocks); the values tests/stale.py settled on
int g_multiple = 4, g_sleeps = 8;
int stale_configure(int multiple, int sleeps)
{
    if (multiple < 1 || multiple > 64 || sleeps < 0 || sleeps > 4096) return -1;
    g_multiple = multiple, g_sleeps = sleeps;
    return 0;
}
int stale_grid(void) { const int cus = cu_count(); return cus <= 0 ? -1 : cus * g_multiple; }

// every workgroup fills its CU's LDS with `pattern`, then holds; ids_out: stale_grid() uint32 (device), the CU id of every workgroup.
// Returns the grid, or -hipError.
int stale_poison(uint32_t pattern, void *stream, uint32_t *ids_out)
{
    const int cus = cu_count(), bytes = lds_bytes(), multiple = g_multiple, sleeps = g_sleeps;
    if (cus <= 0 || !ids_out) return -1;
    hipLaunchKernelGGL(poison_kernel, dim3(cus * multiple), dim3(BLOCK), bytes, (hipStream_t)stream, pattern, bytes / 4, sleeps, ids_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? cus * multiple : -(int)e;
}

// counts_out: 2 x stale_grid() uint32 (device), zeroed by the caller: {CU id, words still holding `pattern`} per workgroup
int stale_canary(uint32_t pattern, void *stream, uint32_t *counts_out)
{
    const int cus = cu_count(), bytes = lds_bytes(), multiple = g_multiple, sleeps = g_sleeps;
    if (cus <= 0 || !counts_out) return -1;
    hipLaunchKernelGGL(canary_kernel, dim3(cus * multiple), dim3(BLOCK), bytes, (hipStream_t)stream, pattern, bytes / 4, sleeps, counts_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? cus * multiple : -(int)e;
}

// x, y: 64 floats (device); one workgroup of 64 lanes, on whichever CU the dispatcher picks -- the poison reached all of them
int stale_demo_good(const float *x, float *y, void *stream)
{
    hipLaunchKernelGGL(demo_kernel<true>, dim3(1), dim3(64), 65 * 4, (hipStream_t)stream, x, y);
    return -(int)hipGetLastError();
}

int stale_demo_bad(const float *x, float *y, void *stream)
{
    hipLaunchKernelGGL(demo_kernel<false>, dim3(1), dim3(64), 65 * 4, (hipStream_t)stream, x, y);
    return -(int)hipGetLastError();
}

}  // extern "C"
