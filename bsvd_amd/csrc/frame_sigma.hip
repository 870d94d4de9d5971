// frame_sigma.hip -- the noise level of a frame, estimated on the device (include/bsvd_hip.h: bsvd_sigma_workspace_bytes,
// bsvd_estimate_sigma, bsvd_fill_sigma_plane): what stands in for the constant sigma map of temp_denoise (validation_seq_infer.py:19-21)
// where the caller has frames and no sigma.  A translation unit of its own: the code objects of the other frame I/O files stay what they
// were.  Three helper kernels on the caller's stream, outside the captured graphs; the item bodies are in frame_sigma_items.h.
//   histogram : one bandwidth pass over the first `channels` planes.  A workgroup keeps a private histogram in LDS (16 KB, integer LDS
//               atomics) and merges it into the frame's 4096 global counts at its end: contiguous uint32 atomic adds, lane l of a wave
//               on bin base + l, one 256-byte run per wave instruction, empty bins skipped.
//   finish    : one workgroup per frame; integer prefix sums, the median's bin, one double division (sigma_from_median).
//   fill      : sigma_t from device memory into plane `channels` of frame t, float4 stores.
// Built with -ffp-contract=off (sources.sh): the definition has no multiply-add to contract, and the flag keeps it that way.
#include "bsvd_internal.h"
#include "frame_sigma_items.h"

namespace bsvd {

enum { SIGMA_BLOCK = 512, SIGMA_MAX_WGS = 512 };

// The LDS add of one sample per lane.  The worst case for LDS atomics is a clean flat frame: every lane of every wave on bin 0.  So the
// wave aggregates first: the lanes that hold the bin of the wave's first remaining lane are counted with one ballot and added by that lane
// alone.  Two such rounds, then whoever remains adds its own 1 -- on a noisy frame a wave holds some 50 different bins, and emptying it
// round by round would cost more than the atomics it saves.
struct LdsAdd {
    unsigned *h;
    __device__ __forceinline__ void operator()(int q, bool counted) const
    {
        const int lane = threadIdx.x & 63;
        unsigned long long rest = __ballot(counted);
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            if (!rest) break;                                        // wave-uniform
            const int leader = __ffsll((long long)rest) - 1;
            const int lq = __shfl(q, leader);
            const bool mine = counted && q == lq;
            const unsigned long long same = __ballot(mine);
            if (lane == leader) atomicAdd(&h[lq], (unsigned)__popcll(same));
            if (mine) counted = false;
            rest &= ~same;
        }
        if (counted) atomicAdd(&h[q], 1u);
    }
};

__global__ __launch_bounds__(SIGMA_BLOCK) void sigma_hist_kernel(const float *__restrict__ x, uint32_t *__restrict__ hist, SigmaGeom g, int items)
{
    __shared__ unsigned lds[SIGMA_BINS];
    for (int i = threadIdx.x; i < SIGMA_BINS; i += SIGMA_BLOCK) lds[i] = 0;
    __syncthreads();
    const float *fr = x + (int64_t)blockIdx.y * g.fstride;
    LdsAdd add{lds};
    for (int i = blockIdx.x * SIGMA_BLOCK + threadIdx.x; i < items; i += gridDim.x * SIGMA_BLOCK) sigma_hist_item(fr, g, i, add);
    __syncthreads();
    uint32_t *out = hist + (int64_t)blockIdx.y * SIGMA_BINS;
    for (int i = threadIdx.x; i < SIGMA_BINS; i += SIGMA_BLOCK) {
        const unsigned v = lds[i];
        if (v) atomicAdd(out + i, v);
    }
}

// lane t owns bins 16 t .. 16 t + 15; exactly one lane finds the median's bin in its run and writes the frame's sigma
__global__ __launch_bounds__(256) void sigma_finish_kernel(const uint32_t *__restrict__ hist, float *__restrict__ sigma, float gain, float lo, float hi)
{
    __shared__ unsigned long long part[256];
    const uint32_t *h = hist + (int64_t)blockIdx.x * SIGMA_BINS + threadIdx.x * 16;
    uint32_t v[16];
    unsigned long long own = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) { v[j] = h[j]; own += v[j]; }
    part[threadIdx.x] = own;
    __syncthreads();
    unsigned long long N = 0, before = 0;
    for (int j = 0; j < 256; ++j) {
        const unsigned long long p = part[j];
        N += p;
        if (j < (int)threadIdx.x) before += p;
    }
    if (N == 0) {
        if (threadIdx.x == 0) sigma[blockIdx.x] = sigma_from_median(0, 0, 0, 0, gain, lo, hi);
        return;
    }
    if (2 * before < N && 2 * (before + own) >= N) {
        unsigned long long cum = before;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            cum += v[j];
            if (2 * cum >= N) { sigma[blockIdx.x] = sigma_from_median(N, threadIdx.x * 16 + j, cum - v[j], v[j], gain, lo, hi); break; }
        }
    }
}

__global__ __launch_bounds__(256) void sigma_fill_kernel(float *__restrict__ x, const float *__restrict__ sigma, int64_t plane_off, int64_t n, int64_t fstride, int64_t items, int vec)
{
    float *plane = x + (int64_t)blockIdx.y * fstride + plane_off;
    const float v = sigma[blockIdx.y];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x)
        sigma_fill_item(plane, n, i, v, vec);
}

// ---------------------------------------------------------------------------------------------
// host side: validation (no device needed), launches
static bool finite_f(float v) { return v - v == 0.f; }

static int planes_check(const char *fn, const void *x, int32_t frames, int32_t channels, int32_t Hp, int32_t Wp, int64_t frame_stride, int planes)
{
    if (!x) { set_error("%s: x is NULL", fn); return -3; }
    if ((uintptr_t)x & 3) { set_error("%s: x must be 4-byte aligned", fn); return -3; }
    if (frames <= 0 || frames > 65535) { set_error("%s: frames = %d must be in 1 .. 65535", fn, frames); return -3; }
    if (channels <= 0) { set_error("%s: channels = %d must be positive", fn, channels); return -3; }
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

int64_t bsvd_sigma_workspace_bytes(int32_t frames)
{
    if (frames <= 0) { set_error("bsvd_sigma_workspace_bytes: frames = %d must be positive", frames); return -1; }
    return (int64_t)frames * SIGMA_BINS * (int64_t)sizeof(uint32_t);
}

int bsvd_estimate_sigma(const float *x, int32_t frames, int32_t channels, int32_t H, int32_t W, int32_t Hp, int32_t Wp, int64_t frame_stride,
                        float gain, float lo, float hi, void *workspace, float *sigma_out, void *stream)
{
    const char *fn = "bsvd_estimate_sigma";
    if (!workspace) { set_error("%s: workspace is NULL", fn); return -3; }
    if (!sigma_out) { set_error("%s: sigma_out is NULL", fn); return -3; }
    if (((uintptr_t)workspace | (uintptr_t)sigma_out) & 3) { set_error("%s: workspace and sigma_out must be 4-byte aligned", fn); return -3; }
    if (H < 3) { set_error("%s: H = %d must be at least 3 (the estimate samples interior pixels)", fn, H); return -3; }
    if (W < 3) { set_error("%s: W = %d must be at least 3 (the estimate samples interior pixels)", fn, W); return -3; }
    if (Hp < H) { set_error("%s: Hp = %d is below H = %d", fn, Hp, H); return -3; }
    if (Wp < W) { set_error("%s: Wp = %d is below W = %d", fn, Wp, W); return -3; }
    const int rc = planes_check(fn, x, frames, channels, Hp, Wp, frame_stride, channels);
    if (rc) return rc;
    if ((double)channels * (double)(H - 2) * (double)(W - 2) >= 4294967296.0) {
        set_error("%s: channels x (H - 2) x (W - 2) = %d x %d x %d: 2^32 samples or more per frame (the counts are uint32)", fn, channels, H - 2, W - 2);
        return -3;
    }
    if (!finite_f(gain) || !(gain > 0.f)) { set_error("%s: gain = %g must be positive and finite", fn, (double)gain); return -3; }
    if (!finite_f(lo) || !finite_f(hi) || lo < 0.f || lo > hi) { set_error("%s: clamp [lo, hi] = [%g, %g]: 0 <= lo <= hi, both finite", fn, (double)lo, (double)hi); return -3; }
    SigmaGeom g;
    g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp; g.ch = channels; g.fstride = frame_stride;
    g.vec = aligned16(x) && !(Wp & 3) && !(frame_stride & 3);
    const int64_t items = sigma_items(g);
    if (items > 0x3fffffff) { set_error("%s: %lld items per frame: more than 2^30", fn, (long long)items); return -3; }

    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)frames * SIGMA_BINS * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    int64_t gx = (items + SIGMA_BLOCK - 1) / SIGMA_BLOCK;
    const int64_t cap = SIGMA_MAX_WGS / frames > 0 ? SIGMA_MAX_WGS / frames : 1;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(sigma_hist_kernel, dim3((unsigned)gx, (unsigned)frames), dim3(SIGMA_BLOCK), 0, (hipStream_t)stream, x, (uint32_t *)workspace, g, (int)items);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sigma_finish_kernel, dim3((unsigned)frames), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)workspace, sigma_out, gain, lo, hi);
    return (int)hipGetLastError();
}

int bsvd_fill_sigma_plane(float *x, int32_t frames, int32_t channels, int32_t Hp, int32_t Wp, int64_t frame_stride, const float *sigma_dev, void *stream)
{
    const char *fn = "bsvd_fill_sigma_plane";
    if (!sigma_dev) { set_error("%s: sigma_dev is NULL", fn); return -3; }
    if ((uintptr_t)sigma_dev & 3) { set_error("%s: sigma_dev must be 4-byte aligned", fn); return -3; }
    const int rc = planes_check(fn, x, frames, channels, Hp, Wp, frame_stride, channels + 1);
    if (rc) return rc;
    const int64_t n = (int64_t)Hp * Wp;
    const int vec = aligned16(x) && !(n & 3) && !(frame_stride & 3);
    const int64_t items = (n + 3) / 4;
    unsigned gx = grid_for(items, 256);
    const unsigned cap = 4096u / (unsigned)frames > 0 ? 4096u / (unsigned)frames : 1u;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(sigma_fill_kernel, dim3(gx, (unsigned)frames), dim3(256), 0, (hipStream_t)stream, x, sigma_dev, (int64_t)channels * n, n, frame_stride, items, vec);
    return (int)hipGetLastError();
}

}  // extern "C"
