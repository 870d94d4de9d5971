// frame_nlf.hip -- the noise-level function of a frame, estimated on the device, and the per-pixel noise map made from it
// (include/bsvd_hip.h: bsvd_nlf_workspace_bytes, bsvd_estimate_nlf, bsvd_fill_nlf_plane): sigma as a function of local intensity, for
// sources whose noise depends on the signal level, where frame_sigma.hip has one number per frame.  A translation unit of its own: the code
// objects of the other files stay what they were.  Three helper kernels on the caller's stream, outside the captured graphs; the item
// bodies are in frame_nlf_items.h.
//   histogram : one bandwidth pass over the three colour planes.  A workgroup keeps a private [16][1024] histogram in LDS (64 KB, integer
//               LDS atomics: two 512-thread workgroups per CU) and merges it into the frame's global counts at its end: contiguous uint32
//               atomic adds, empty entries skipped.
//   finish    : one workgroup of sixteen waves per frame, wave l on level l: integer prefix sums, the median's bin, one double division
//               (nlf_from_median); the pooled median by wave 0; the nearest-valid fill by sixteen lanes.
//   map       : the frame's sixteen curve values from device memory into LDS, three planes through the box stencil, one plane written with
//               float4 stores.
// Built with -ffp-contract=off (sources.sh): the map's interpolation is a multiply and an add that round separately.
#include "bsvd_internal.h"
#include "frame_nlf_items.h"

#ifndef BSVD_NLF_ROUNDS
#define BSVD_NLF_ROUNDS 1            // wave-aggregation rounds of the LDS add; profiles/noise_curve.txt has what 0 .. 3 measured
#endif

namespace bsvd {

enum { NLF_BLOCK = 512, NLF_MAX_WGS = 512, NLF_MAP_BLOCK = 256 };

// The LDS add of one sample per lane, keyed by (level << 10) | bin.  The worst case for LDS atomics is a clean flat frame: every lane of
// every wave on one key.  So the wave aggregates first, as LdsAdd of frame_sigma.hip does: the lanes that hold the key of the wave's first
// remaining lane are counted with one ballot and added by that lane alone, for ROUNDS rounds; whoever remains adds its own 1.
template <int ROUNDS>
struct NlfLdsAdd {
    unsigned *h;
    __device__ __forceinline__ void operator()(int key, bool counted) const
    {
        const int lane = threadIdx.x & 63;
        unsigned long long rest = __ballot(counted);
#pragma unroll
        for (int round = 0; round < ROUNDS; ++round) {
            if (!rest) break;                                        // wave-uniform
            const int leader = __ffsll((long long)rest) - 1;
            const int lk = __shfl(key, leader);
            const bool mine = counted && key == lk;
            const unsigned long long same = __ballot(mine);
            if (lane == leader) atomicAdd(&h[lk], (unsigned)__popcll(same));
            if (mine) counted = false;
            rest &= ~same;
        }
        if (counted) atomicAdd(&h[key], 1u);
    }
};

__global__ __launch_bounds__(NLF_BLOCK) void nlf_hist_kernel(const float *__restrict__ x, uint32_t *__restrict__ hist, SigmaGeom g, int items)
{
    __shared__ unsigned lds[NLF_HIST];
    for (int i = threadIdx.x; i < NLF_HIST; i += NLF_BLOCK) lds[i] = 0;
    __syncthreads();
    const float *fr = x + (int64_t)blockIdx.y * g.fstride;
    NlfLdsAdd<BSVD_NLF_ROUNDS> add{lds};
    for (int i = blockIdx.x * NLF_BLOCK + threadIdx.x; i < items; i += gridDim.x * NLF_BLOCK) nlf_hist_item(fr, g, i, add);
    __syncthreads();
    uint32_t *out = hist + (int64_t)blockIdx.y * NLF_HIST;
    for (int i = threadIdx.x; i < NLF_HIST; i += NLF_BLOCK) {
        const unsigned v = lds[i];
        if (v) atomicAdd(out + i, v);
    }
}

// One wave on one histogram of 1024 counts: lane t owns bins 16 t .. 16 t + 15 (v), part[t] their sum.  Exactly one lane finds the median's
// bin in its run (lane 0 where the histogram is empty) and writes *value; that lane also writes *N_out.
__device__ __forceinline__ void nlf_wave_median(const uint32_t (&v)[16], const unsigned long long *part, int lane, float gain, float lo, float hi,
                                                float *value, unsigned long long *N_out)
{
    unsigned long long N = 0, before = 0, own = 0;
#pragma unroll 4
    for (int j = 0; j < 64; ++j) {
        const unsigned long long p = part[j];
        N += p;
        if (j < lane) before += p;
        if (j == lane) own = p;
    }
    if (N == 0) {
        if (lane == 0) { *value = nlf_from_median(0, 0, 0, 0, gain, lo, hi); *N_out = 0; }
        return;
    }
    if (2 * before < N && 2 * (before + own) >= N) {
        unsigned long long cum = before;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            cum += v[j];
            if (2 * cum >= N) { *value = nlf_from_median(N, lane * 16 + j, cum - v[j], v[j], gain, lo, hi); *N_out = N; break; }
        }
    }
}

__global__ __launch_bounds__(1024) void nlf_finish_kernel(const uint32_t *__restrict__ hist, float *__restrict__ curve, float gain, float lo, float hi, int min_count)
{
    __shared__ unsigned long long part[NLF_LEVELS + 1][64];
    __shared__ unsigned long long count[NLF_LEVELS + 1];
    __shared__ unsigned pooled[NLF_BINS];
    __shared__ float own[NLF_LEVELS + 1];
    const uint32_t *h = hist + (int64_t)blockIdx.x * NLF_HIST;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned p = 0;                                                  // below 2^32: the entry point bounds the samples of a frame
    for (int l = 0; l < NLF_LEVELS; ++l) p += h[l * NLF_BINS + threadIdx.x];
    pooled[threadIdx.x] = p;
    uint32_t v[16];
    unsigned long long sum = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) { v[j] = h[wave * NLF_BINS + lane * 16 + j]; sum += v[j]; }
    part[wave][lane] = sum;
    __syncthreads();
    nlf_wave_median(v, part[wave], lane, gain, lo, hi, &own[wave], &count[wave]);
    if (wave == 0) {
        sum = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) { v[j] = pooled[lane * 16 + j]; sum += v[j]; }
        part[NLF_LEVELS][lane] = sum;
    }
    __syncthreads();
    if (wave == 0) nlf_wave_median(v, part[NLF_LEVELS], lane, gain, lo, hi, &own[NLF_LEVELS], &count[NLF_LEVELS]);
    __syncthreads();
    if (threadIdx.x < NLF_LEVELS) {
        unsigned valid = 0;
        for (int l = 0; l < NLF_LEVELS; ++l)
            if (count[l] >= (unsigned long long)min_count) valid |= 1u << l;
        curve[(int64_t)blockIdx.x * NLF_LEVELS + threadIdx.x] = nlf_level_value(threadIdx.x, own, valid, own[NLF_LEVELS]);
    }
}

__global__ __launch_bounds__(NLF_MAP_BLOCK) void nlf_map_kernel(float *__restrict__ x, const float *__restrict__ curve, NlfMapGeom g, int64_t items)
{
    __shared__ float c[NLF_LEVELS];
    if (threadIdx.x < NLF_LEVELS) c[threadIdx.x] = curve[(int64_t)blockIdx.y * NLF_LEVELS + threadIdx.x];
    __syncthreads();
    float *fr = x + (int64_t)blockIdx.y * g.fstride;
    for (int64_t i = blockIdx.x * (int64_t)NLF_MAP_BLOCK + threadIdx.x; i < items; i += (int64_t)gridDim.x * NLF_MAP_BLOCK)
        nlf_map_item(fr, g, c, i);
}

// ---------------------------------------------------------------------------------------------
// host side: validation (no device needed), launches
static bool nlf_finite(float v) { return v - v == 0.f; }

static int nlf_planes_check(const char *fn, const void *x, int32_t frames, int32_t Hp, int32_t Wp, int64_t frame_stride, int planes)
{
    if (!x) { set_error("%s: x is NULL", fn); return -3; }
    if ((uintptr_t)x & 3) { set_error("%s: x must be 4-byte aligned", fn); return -3; }
    if (frames <= 0 || frames > 65535) { set_error("%s: frames = %d must be in 1 .. 65535", fn, frames); return -3; }
    if (Hp <= 0) { set_error("%s: Hp = %d must be positive", fn, Hp); return -3; }
    if (Wp <= 0) { set_error("%s: Wp = %d must be positive", fn, Wp); return -3; }
    const int64_t need = (int64_t)planes * Hp * Wp;
    if (frame_stride < need) {
        set_error("%s: frame_stride = %lld floats is below the %d planes of %d x %d it spans (%lld)", fn, (long long)frame_stride, planes, Hp, Wp, (long long)need);
        return -3;
    }
    return 0;
}

}  // namespace bsvd

using namespace bsvd;

extern "C" {

int64_t bsvd_nlf_workspace_bytes(int32_t frames)
{
    if (frames <= 0) { set_error("bsvd_nlf_workspace_bytes: frames = %d must be positive", frames); return -1; }
    return (int64_t)frames * NLF_HIST * (int64_t)sizeof(uint32_t);
}

int bsvd_estimate_nlf(const float *x, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp, int64_t frame_stride,
                      float gain, float lo, float hi, int32_t min_count, void *workspace, float *curve_out, void *stream)
{
    const char *fn = "bsvd_estimate_nlf";
    if (!workspace) { set_error("%s: workspace is NULL", fn); return -3; }
    if (!curve_out) { set_error("%s: curve_out is NULL", fn); return -3; }
    if (((uintptr_t)workspace | (uintptr_t)curve_out) & 3) { set_error("%s: workspace and curve_out must be 4-byte aligned", fn); return -3; }
    if (H < 3) { set_error("%s: H = %d must be at least 3 (the estimate samples interior pixels)", fn, H); return -3; }
    if (W < 3) { set_error("%s: W = %d must be at least 3 (the estimate samples interior pixels)", fn, W); return -3; }
    if (Hp < H) { set_error("%s: Hp = %d is below H = %d", fn, Hp, H); return -3; }
    if (Wp < W) { set_error("%s: Wp = %d is below W = %d", fn, Wp, W); return -3; }
    const int rc = nlf_planes_check(fn, x, frames, Hp, Wp, frame_stride, 3);
    if (rc) return rc;
    if (3.0 * (double)(H - 2) * (double)(W - 2) >= 4294967296.0) {
        set_error("%s: 3 x (H - 2) x (W - 2) = 3 x %d x %d: 2^32 samples or more per frame (the counts are uint32)", fn, H - 2, W - 2);
        return -3;
    }
    if (!nlf_finite(gain) || !(gain > 0.f)) { set_error("%s: gain = %g must be positive and finite", fn, (double)gain); return -3; }
    if (!nlf_finite(lo) || !nlf_finite(hi) || lo < 0.f || lo > hi) { set_error("%s: clamp [lo, hi] = [%g, %g]: 0 <= lo <= hi, both finite", fn, (double)lo, (double)hi); return -3; }
    if (min_count < 1) { set_error("%s: min_count = %d must be at least 1", fn, min_count); return -3; }
    SigmaGeom g;
    g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp; g.ch = 3; g.fstride = frame_stride;
    g.vec = aligned16(x) && !(Wp & 3) && !(frame_stride & 3);
    const int64_t items = sigma_items(g);
    if (items > 0x3fffffff) { set_error("%s: %lld items per frame: more than 2^30", fn, (long long)items); return -3; }

    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)frames * NLF_HIST * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    int64_t gx = (items + NLF_BLOCK - 1) / NLF_BLOCK;
    const int64_t cap = NLF_MAX_WGS / frames > 0 ? NLF_MAX_WGS / frames : 1;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(nlf_hist_kernel, dim3((unsigned)gx, (unsigned)frames), dim3(NLF_BLOCK), 0, (hipStream_t)stream, x, (uint32_t *)workspace, g, (int)items);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(nlf_finish_kernel, dim3((unsigned)frames), dim3(1024), 0, (hipStream_t)stream, (const uint32_t *)workspace, curve_out, gain, lo, hi, (int)min_count);
    return (int)hipGetLastError();
}

int bsvd_finish_nlf(const void *workspace, int32_t frames, float gain, float lo, float hi, int32_t min_count, float *curve_out, void *stream)
{
    const char *fn = "bsvd_finish_nlf";
    if (!workspace) { set_error("%s: workspace is NULL", fn); return -3; }
    if (!curve_out) { set_error("%s: curve_out is NULL", fn); return -3; }
    if (((uintptr_t)workspace | (uintptr_t)curve_out) & 3) { set_error("%s: workspace and curve_out must be 4-byte aligned", fn); return -3; }
    if (frames <= 0 || frames > 65535) { set_error("%s: frames = %d must be in 1 .. 65535", fn, frames); return -3; }
    if (!nlf_finite(gain) || !(gain > 0.f)) { set_error("%s: gain = %g must be positive and finite", fn, (double)gain); return -3; }
    if (!nlf_finite(lo) || !nlf_finite(hi) || lo < 0.f || lo > hi) { set_error("%s: clamp [lo, hi] = [%g, %g]: 0 <= lo <= hi, both finite", fn, (double)lo, (double)hi); return -3; }
    if (min_count < 1) { set_error("%s: min_count = %d must be at least 1", fn, min_count); return -3; }
    hipLaunchKernelGGL(nlf_finish_kernel, dim3((unsigned)frames), dim3(1024), 0, (hipStream_t)stream, (const uint32_t *)workspace, curve_out, gain, lo, hi, (int)min_count);
    return (int)hipGetLastError();
}

int bsvd_fill_nlf_plane(float *x, int32_t frames, int32_t channels, int32_t Hp, int32_t Wp, int64_t frame_stride, const float *curve_dev, void *stream)
{
    const char *fn = "bsvd_fill_nlf_plane";
    if (!curve_dev) { set_error("%s: curve_dev is NULL", fn); return -3; }
    if ((uintptr_t)curve_dev & 3) { set_error("%s: curve_dev must be 4-byte aligned", fn); return -3; }
    if (channels < 3) { set_error("%s: channels = %d must be at least 3 (the map reads three colour planes)", fn, channels); return -3; }
    const int rc = nlf_planes_check(fn, x, frames, Hp, Wp, frame_stride, channels + 1);
    if (rc) return rc;
    NlfMapGeom g;
    g.Hp = Hp; g.Wp = Wp; g.out_plane = channels; g.fstride = frame_stride;
    g.vec = aligned16(x) && !(Wp & 3) && !(frame_stride & 3);
    const int64_t items = nlf_map_items(g);
    unsigned gx = grid_for(items, NLF_MAP_BLOCK);
    const unsigned cap = 4096u / (unsigned)frames > 0 ? 4096u / (unsigned)frames : 1u;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(nlf_map_kernel, dim3(gx, (unsigned)frames), dim3(NLF_MAP_BLOCK), 0, (hipStream_t)stream, x, curve_dev, g, items);
    return (int)hipGetLastError();
}

}  // extern "C"
