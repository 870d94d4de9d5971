// frame_scene.hip -- what a scene-cut detector needs from a frame, computed on the device (include/bsvd_hip.h: bsvd_scene_grid,
// bsvd_scene_diff).  Two helper kernels on the caller's stream, outside the captured graphs; a translation unit of its own, so the code
// objects of the other frame I/O files stay what they were.
//   grid : the sum of L = qR + 2 qG + qB over every full 16 x 16 block of the picture, q = clamp(rint(255 v), 0, 255).  One wave per block:
//          lane l reads one float4 per plane, columns 4 (l & 3) .. + 3 of row l >> 2 -- four lanes a row, sixteen rows -- and the wave sums
//          its 64 partial sums with five-and-one xor shuffles.  The four waves of a workgroup take four blocks side by side, so a row of
//          the workgroup is one 256-byte run.  Lane 0 stores the block's sum.
//   diff : sad[t] = sum over the blocks of |grid[t] - grid[t-1]|: per-thread uint64 partial sums, a wave shuffle, LDS across the waves, one
//          64-bit atomic add per workgroup into the (zeroed) sum.
// Integers throughout: neither result depends on the launch shape or on the order of the adds.
#include "bsvd_internal.h"

namespace bsvd {

enum { SCENE_BLOCK = 16, SCENE_WAVES = 4, SCENE_DIFF_THREADS = 256, SCENE_DIFF_MAX_WGS = 64 };

// NaN -> 0 (fmaxf returns the other operand), -inf -> 0, +inf -> 255; rintf rounds halves to even
__device__ __forceinline__ int scene_q(float v)
{
    return (int)fminf(fmaxf(rintf(v * 255.f), 0.f), 255.f);
}

__device__ __forceinline__ int scene_q4(const float *p, int vec)
{
    if (vec) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        return (scene_q(v.x) + scene_q(v.y)) + (scene_q(v.z) + scene_q(v.w));
    }
    return (scene_q(p[0]) + scene_q(p[1])) + (scene_q(p[2]) + scene_q(p[3]));
}

__global__ __launch_bounds__(SCENE_WAVES * 64) void scene_grid_kernel(const float *__restrict__ x, int32_t *__restrict__ grid, int GW, int blocks, int Wp,
                                                                      int64_t plane, int64_t fstride, int vec)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * SCENE_WAVES + (threadIdx.x >> 6);          // wave-uniform
    if (b >= blocks) return;
    const int by = b / GW, bx = b - by * GW;
    const float *p = x + (int64_t)blockIdx.y * fstride + (int64_t)(by * SCENE_BLOCK + (lane >> 2)) * Wp + bx * SCENE_BLOCK + 4 * (lane & 3);
    int s = scene_q4(p, vec) + 2 * scene_q4(p + plane, vec) + scene_q4(p + 2 * plane, vec);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) grid[(int64_t)blockIdx.y * blocks + b] = s;
}

__global__ __launch_bounds__(SCENE_DIFF_THREADS) void scene_diff_kernel(const int32_t *__restrict__ grid, const int32_t *__restrict__ prev_grid, int blocks,
                                                                        unsigned long long *__restrict__ sad)
{
    __shared__ unsigned long long part[SCENE_DIFF_THREADS / 64];
    const int t = blockIdx.y;
    const int32_t *cur = grid + (int64_t)t * blocks;
    const int32_t *old = t ? cur - blocks : prev_grid;
    if (!old) return;                                                      // frame 0 without a predecessor: its sum stays 0 (uniform over the workgroup)
    unsigned long long s = 0;
    for (int i = blockIdx.x * SCENE_DIFF_THREADS + threadIdx.x; i < blocks; i += gridDim.x * SCENE_DIFF_THREADS) {
        const int d = cur[i] - old[i];
        s += (unsigned)(d < 0 ? -d : d);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
#pragma unroll
        for (int w = 0; w < SCENE_DIFF_THREADS / 64; ++w) all += part[w];
        if (all) atomicAdd(sad + t, all);
    }
}

}  // namespace bsvd

using namespace bsvd;

extern "C" {

int bsvd_scene_grid(const float *x, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp, int64_t frame_stride, int32_t *grid, void *stream)
{
    const char *fn = "bsvd_scene_grid";
    if (!x) { set_error("%s: x is NULL", fn); return -3; }
    if ((uintptr_t)x & 3) { set_error("%s: x must be 4-byte aligned", fn); return -3; }
    if (frames <= 0 || frames > 65535) { set_error("%s: frames = %d must be in 1 .. 65535", fn, frames); return -3; }
    if (H < 0) { set_error("%s: H = %d must not be negative", fn, H); return -3; }
    if (W < 0) { set_error("%s: W = %d must not be negative", fn, W); return -3; }
    if (Hp <= 0 || Hp < H) { set_error("%s: Hp = %d must be positive and at least H = %d", fn, Hp, H); return -3; }
    if (Wp <= 0 || Wp < W) { set_error("%s: Wp = %d must be positive and at least W = %d", fn, Wp, W); return -3; }
    const int64_t plane = (int64_t)Hp * Wp;
    if (frame_stride < 3 * plane) {
        set_error("%s: frame_stride = %lld floats is below the 3 planes of %d x %d it spans (%lld)", fn, (long long)frame_stride, Hp, Wp, (long long)(3 * plane));
        return -3;
    }
    const int GH = H / SCENE_BLOCK, GW = W / SCENE_BLOCK;
    const int64_t blocks = (int64_t)GH * GW;
    if (blocks == 0) return 0;                                             // no full block: nothing to write, nothing launched
    if (blocks > 0x3fffffff) { set_error("%s: %lld blocks per frame: more than 2^30", fn, (long long)blocks); return -3; }
    if (!grid) { set_error("%s: grid is NULL", fn); return -3; }
    if ((uintptr_t)grid & 3) { set_error("%s: grid must be 4-byte aligned", fn); return -3; }
    const int vec = aligned16(x) && !(Wp & 3) && !(frame_stride & 3);
    const unsigned gx = (unsigned)((blocks + SCENE_WAVES - 1) / SCENE_WAVES);
    hipLaunchKernelGGL(scene_grid_kernel, dim3(gx, (unsigned)frames), dim3(SCENE_WAVES * 64), 0, (hipStream_t)stream, x, grid, GW, (int)blocks, (int)Wp, plane,
                       frame_stride, vec);
    return (int)hipGetLastError();
}

int bsvd_scene_diff(const int32_t *grid, const int32_t *prev_grid, int32_t frames, int32_t blocks, uint64_t *sad, void *stream)
{
    const char *fn = "bsvd_scene_diff";
    if (frames <= 0 || frames > 65535) { set_error("%s: frames = %d must be in 1 .. 65535", fn, frames); return -3; }
    if (blocks < 0 || blocks > 0x3fffffff) { set_error("%s: blocks = %d must be in 0 .. 2^30", fn, blocks); return -3; }
    if (!sad) { set_error("%s: sad is NULL", fn); return -3; }
    if ((uintptr_t)sad & 7) { set_error("%s: sad must be 8-byte aligned", fn); return -3; }
    if (blocks && !grid) { set_error("%s: grid is NULL", fn); return -3; }
    if (((uintptr_t)grid | (uintptr_t)prev_grid) & 3) { set_error("%s: grid and prev_grid must be 4-byte aligned", fn); return -3; }
    hipError_t e = hipMemsetAsync(sad, 0, (size_t)frames * sizeof(uint64_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (blocks == 0 || (frames == 1 && !prev_grid)) return 0;              // every sum is 0: no kernel
    unsigned gx = grid_for(blocks, SCENE_DIFF_THREADS);
    if (gx > SCENE_DIFF_MAX_WGS) gx = SCENE_DIFF_MAX_WGS;
    hipLaunchKernelGGL(scene_diff_kernel, dim3(gx, (unsigned)frames), dim3(SCENE_DIFF_THREADS), 0, (hipStream_t)stream, grid, prev_grid, (int)blocks,
                       (unsigned long long *)sad);
    return (int)hipGetLastError();
}

}  // extern "C"
