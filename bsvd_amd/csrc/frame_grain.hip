// frame_grain.hip -- the film-grain model on the device (include/bsvd_hip.h: bsvd_grain_stats_bytes, bsvd_grain_stats, bsvd_grain_apply):
// the statistics of the noise the network removed (its strength against the result's brightness, its spatial autocovariance), from which
// the host fits a model, and the synthesis of clean grain from such a model onto the result.  A translation unit of its own: the code
// objects of the other files stay what they were.  Two helper kernels on the caller's stream, outside the captured graphs; the per-pixel
// bodies are in frame_grain_items.h.
//   stats : a workgroup of four waves takes tiles of GRAIN_TH x 64 pixels.  It stages the tile's three q planes in LDS as int16 with a halo
//           of 3 rows below and 6 columns on each side (what the lags reach; outside the picture: zeros, nothing is read there), adding
//           the level moments of the pixels the tile owns on the way: the wave aggregates them by level first (a flat frame has every lane
//           on one level), as NlfLdsAdd of frame_nlf.hip does.  Then lag by lag: a lane holds the anchors of one column (GRAIN_TH / 4 rows)
//           in registers, multiplies them with the staged neighbour, the wave adds the partial sums and one lane adds the total to the
//           workgroup's int64 accumulators in LDS.  The 256 accumulators go to the frame's workspace once, at the workgroup's end.
//           Bound of the int32 partial sums: a wave adds 64 lanes x GRAIN_TH / 4 products of two |q| <= 2047: at GRAIN_TH = 32 that is
//           512 x 2047^2 = 2 145 387 008 <= 2^31 - 1 (by 2 096 639: GRAIN_TH may not grow).  One accumulator per lag per lane instead
//           (138 int32 and their 64-bit flushes) does not fit the register budget next to the anchors.
//   apply : a grid-stride loop around grain_apply_item; the sixteen levels of the three std curves in LDS (the level index differs per
//           lane), the templates (196 KB) read through the caches: neighbouring lanes read neighbouring floats of one template row.
// Built with -ffp-contract=off (sources.sh): products and sums round separately except where the header says fmaf.
#include "bsvd_internal.h"
#include "frame_grain_items.h"

#ifndef BSVD_GRAIN_TILE_ROWS
#define BSVD_GRAIN_TILE_ROWS 32      // rows of a statistics tile: 16 or 32; profiles/film_grain.txt has what both measured
#endif
#ifndef BSVD_GRAIN_ROUNDS
#define BSVD_GRAIN_ROUNDS 2          // wave-aggregation rounds of the level moments before the lanes that remain add their own
#endif

namespace bsvd {

enum { GRAIN_TH = BSVD_GRAIN_TILE_ROWS, GRAIN_TW = 64, GRAIN_WG = 256, GRAIN_SR = GRAIN_TH + GRAIN_LAG_ROWS, GRAIN_SC = GRAIN_TW + 2 * GRAIN_LAG_COLS,
       GRAIN_MAX_WGS = 512, GRAIN_ANCHORS = GRAIN_TH / 4 };
static_assert(GRAIN_TH % 4 == 0 && 64LL * GRAIN_ANCHORS * GRAIN_QMAX * GRAIN_QMAX <= 2147483647LL, "a wave's partial sum of products must fit int32");
static_assert(GRAIN_A_AT + 3 * GRAIN_LAGS <= GRAIN_STATS && GRAIN_STATS == GRAIN_WG, "the statistics of a frame are 256 int64");

struct GrainStatsGeom { int H, W, Wp, tiles_x, tiles; int64_t x_fs, y_fs, plane; float w[3]; };

__device__ __forceinline__ int grain_wave_sum(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ void grain_acc_add(unsigned long long *at, long long v) { atomicAdd(at, (unsigned long long)v); }

// the level moments of one pixel per lane (owned: it is the tile's and it is counted): every lane of the wave reaches this together
__device__ __forceinline__ void grain_moments_add(unsigned long long *acc, int l, bool owned, const int *q)
{
    const int lane = threadIdx.x & 63;
    unsigned long long rest = __ballot(owned);
#pragma unroll
    for (int round = 0; round < BSVD_GRAIN_ROUNDS; ++round) {
        if (!rest) break;                                            // wave-uniform
        const int leader = __ffsll((long long)rest) - 1;
        const int ll = __shfl(l, leader);
        const bool mine = owned && l == ll;
        const unsigned long long same = __ballot(mine);
        int s1[3], s2[3];                                            // 64 x 2047^2 < 2^29
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s1[k] = grain_wave_sum(mine ? q[k] : 0);
            s2[k] = grain_wave_sum(mine ? q[k] * q[k] : 0);
        }
        if (lane == leader) {
            grain_acc_add(&acc[GRAIN_N_AT + ll], __popcll(same));
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                grain_acc_add(&acc[GRAIN_S1_AT + k * GRAIN_LEVELS + ll], s1[k]);
                grain_acc_add(&acc[GRAIN_S2_AT + k * GRAIN_LEVELS + ll], s2[k]);
            }
        }
        if (mine) owned = false;
        rest &= ~same;
    }
    if (owned) {
        grain_acc_add(&acc[GRAIN_N_AT + l], 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            grain_acc_add(&acc[GRAIN_S1_AT + k * GRAIN_LEVELS + l], q[k]);
            grain_acc_add(&acc[GRAIN_S2_AT + k * GRAIN_LEVELS + l], q[k] * q[k]);
        }
    }
}

__global__ __launch_bounds__(GRAIN_WG) void grain_stats_kernel(const float *__restrict__ x, const float *__restrict__ y, unsigned long long *__restrict__ ws,
                                                               GrainStatsGeom g)
{
    __shared__ short q[3][GRAIN_SR][GRAIN_SC];
    __shared__ unsigned long long acc[GRAIN_STATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    acc[tid] = 0;                                                    // GRAIN_STATS == GRAIN_WG
    const float *xf = x + (int64_t)blockIdx.y * g.x_fs, *yf = y + (int64_t)blockIdx.y * g.y_fs;
    for (int tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {
        __syncthreads();                                             // acc is zero / the tile before has been read
        const int r0 = (tile / g.tiles_x) * GRAIN_TH, c0 = (tile % g.tiles_x) * GRAIN_TW;
        for (int i0 = 0; i0 < GRAIN_SR * GRAIN_SC; i0 += GRAIN_WG) { // the same trips in every lane: the moments are a wave's business
            const int i = i0 + tid, rr = i / GRAIN_SC, cc = i - rr * GRAIN_SC;
            const int pr = r0 + rr, pc = c0 - GRAIN_LAG_COLS + cc;
            const bool staged = i < GRAIN_SR * GRAIN_SC;
            int l = 0, qq[3] = {0, 0, 0};
            bool counted = false;
            if (staged && pr < g.H && pc >= 0 && pc < g.W) {         // the picture, and nothing else, is read
                const int64_t at = (int64_t)pr * g.Wp + pc;
                const float x3[3] = {xf[at], xf[at + g.plane], xf[at + 2 * g.plane]};
                const float y3[3] = {yf[at], yf[at + g.plane], yf[at + 2 * g.plane]};
                counted = grain_pixel_q(x3, y3, g.w, &l, qq);
            }
            if (staged) {
#pragma unroll
                for (int k = 0; k < 3; ++k) q[k][rr][cc] = (short)qq[k];
            }
            grain_moments_add(acc, l, counted && rr < GRAIN_TH && cc >= GRAIN_LAG_COLS && cc < GRAIN_LAG_COLS + GRAIN_TW, qq);
        }
        __syncthreads();
        // anchors: column c0 + lane, rows r0 + wave + 4 j; the rule 0 <= r <= H - 4, 6 <= c <= W - 7 is the same for every lag
        const int ac = c0 + lane;
        const bool col_ok = ac >= GRAIN_LAG_COLS && ac <= g.W - 1 - GRAIN_LAG_COLS;
        for (int k = 0; k < 3; ++k) {
            int a[GRAIN_ANCHORS];
#pragma unroll
            for (int j = 0; j < GRAIN_ANCHORS; ++j) {
                const int ar = wave + 4 * j;
                a[j] = col_ok && r0 + ar <= g.H - 1 - GRAIN_LAG_ROWS ? (int)q[k][ar][lane + GRAIN_LAG_COLS] : 0;
            }
#pragma unroll
            for (int lag = 0; lag < GRAIN_LAGS; ++lag) {
                int dy, dx;
                grain_lag(lag, &dy, &dx);
                int s = 0;
#pragma unroll
                for (int j = 0; j < GRAIN_ANCHORS; ++j) s += a[j] * (int)q[k][wave + 4 * j + dy][lane + GRAIN_LAG_COLS + dx];
                s = grain_wave_sum(s);
                if (lane == 0 && s) grain_acc_add(&acc[GRAIN_A_AT + k * GRAIN_LAGS + lag], s);
            }
        }
    }
    __syncthreads();
    const unsigned long long v = acc[tid];
    if (v) atomicAdd(ws + (int64_t)blockIdx.y * GRAIN_STATS + tid, v);
}

__global__ __launch_bounds__(256) void grain_apply_kernel(float *__restrict__ y, const float *__restrict__ tmpl, GrainApplyGeom g, int64_t items)
{
    __shared__ float sd[3][GRAIN_LEVELS];
#pragma unroll
    for (int j = 0; j < 3 * GRAIN_LEVELS; ++j)                       // constant indices into the argument: no copy of it in scratch
        if ((int)threadIdx.x == j) sd[j / GRAIN_LEVELS][j % GRAIN_LEVELS] = g.std[j / GRAIN_LEVELS][j % GRAIN_LEVELS];
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x)
        grain_apply_item(y, tmpl, g, sd, i);
}

// ---------------------------------------------------------------------------------------------
// host side: validation (no device needed), launches
static bool grain_finite(float v) { return v - v == 0.f; }

static int grain_planes_check(const char *fn, const char *name, const void *p, int32_t Hp, int32_t Wp, int64_t frame_stride)
{
    if (!p) { set_error("%s: %s is NULL", fn, name); return -3; }
    if ((uintptr_t)p & 3) { set_error("%s: %s must be 4-byte aligned", fn, name); return -3; }
    const int64_t need = 3 * (int64_t)Hp * Wp;
    if (frame_stride < need) {
        set_error("%s: %s_frame_stride = %lld floats is below the 3 planes of %d x %d it spans (%lld)", fn, name, (long long)frame_stride, Hp, Wp, (long long)need);
        return -3;
    }
    return 0;
}

}  // namespace bsvd

using namespace bsvd;

extern "C" {

int64_t bsvd_grain_stats_bytes(int32_t frames)
{
    if (frames <= 0) { set_error("bsvd_grain_stats_bytes: frames = %d must be positive", frames); return -1; }
    return (int64_t)frames * GRAIN_STATS * (int64_t)sizeof(int64_t);
}

int bsvd_grain_stats(const float *x, int64_t x_frame_stride, const float *y, int64_t y_frame_stride, int32_t frames, int32_t H, int32_t W,
                     int32_t Hp, int32_t Wp, const float luma_w[3], void *workspace, void *stream)
{
    const char *fn = "bsvd_grain_stats";
    if (!luma_w) { set_error("%s: luma_w is NULL", fn); return -3; }
    if (!workspace) { set_error("%s: workspace is NULL", fn); return -3; }
    if ((uintptr_t)workspace & 7) { set_error("%s: workspace must be 8-byte aligned", fn); return -3; }
    if (frames <= 0 || frames > 65535) { set_error("%s: frames = %d must be in 1 .. 65535", fn, frames); return -3; }
    if (H < 1 + GRAIN_LAG_ROWS) { set_error("%s: H = %d must be at least 4 (an anchor and the 3 rows below it)", fn, H); return -3; }
    if (W < 1 + 2 * GRAIN_LAG_COLS) { set_error("%s: W = %d must be at least 13 (an anchor and 6 columns on each side)", fn, W); return -3; }
    if (Hp < H) { set_error("%s: Hp = %d is below H = %d", fn, Hp, H); return -3; }
    if (Wp < W) { set_error("%s: Wp = %d is below W = %d", fn, Wp, W); return -3; }
    int rc = grain_planes_check(fn, "x", x, Hp, Wp, x_frame_stride);
    if (!rc) rc = grain_planes_check(fn, "y", y, Hp, Wp, y_frame_stride);
    if (rc) return rc;
    for (int c = 0; c < 3; ++c)
        if (!grain_finite(luma_w[c])) { set_error("%s: luma_w[%d] = %g must be finite", fn, c, (double)luma_w[c]); return -3; }
    GrainStatsGeom g;
    g.H = H; g.W = W; g.Wp = Wp;
    g.tiles_x = (W + GRAIN_TW - 1) / GRAIN_TW;
    const int64_t tiles = (int64_t)g.tiles_x * ((H + GRAIN_TH - 1) / GRAIN_TH);
    if (tiles > 0x3fffffff) { set_error("%s: %lld tiles per frame: more than 2^30", fn, (long long)tiles); return -3; }
    g.tiles = (int)tiles;
    g.x_fs = x_frame_stride; g.y_fs = y_frame_stride; g.plane = (int64_t)Hp * Wp;
    for (int c = 0; c < 3; ++c) g.w[c] = luma_w[c];

    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)frames * GRAIN_STATS * sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    int64_t gx = tiles;
    const int64_t cap = GRAIN_MAX_WGS / frames > 0 ? GRAIN_MAX_WGS / frames : 1;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(grain_stats_kernel, dim3((unsigned)gx, (unsigned)frames), dim3(GRAIN_WG), 0, (hipStream_t)stream, x, y, (unsigned long long *)workspace, g);
    return (int)hipGetLastError();
}

int bsvd_grain_apply(float *y, int64_t y_frame_stride, int32_t frames, int32_t Hp, int32_t Wp, const float *templates, const float *std,
                     float amount, const float luma_w[3], float inv_wg, uint32_t seed, int64_t frame0, void *stream)
{
    const char *fn = "bsvd_grain_apply";
    if (!templates) { set_error("%s: templates is NULL", fn); return -3; }
    if ((uintptr_t)templates & 3) { set_error("%s: templates must be 4-byte aligned", fn); return -3; }
    if (!std) { set_error("%s: std is NULL", fn); return -3; }
    if (!luma_w) { set_error("%s: luma_w is NULL", fn); return -3; }
    if (frames <= 0 || frames > 65535) { set_error("%s: frames = %d must be in 1 .. 65535", fn, frames); return -3; }
    if (Hp <= 0) { set_error("%s: Hp = %d must be positive", fn, Hp); return -3; }
    if (Wp <= 0) { set_error("%s: Wp = %d must be positive", fn, Wp); return -3; }
    const int rc = grain_planes_check(fn, "y", y, Hp, Wp, y_frame_stride);
    if (rc) return rc;
    if (!grain_finite(amount) || amount < 0.f) { set_error("%s: amount = %g must be finite and not negative", fn, (double)amount); return -3; }
    for (int c = 0; c < 3; ++c)
        if (!grain_finite(luma_w[c])) { set_error("%s: luma_w[%d] = %g must be finite", fn, c, (double)luma_w[c]); return -3; }
    if (!grain_finite(inv_wg)) { set_error("%s: inv_wg = %g must be finite", fn, (double)inv_wg); return -3; }
    if (frame0 < 0) { set_error("%s: frame0 = %lld must not be negative", fn, (long long)frame0); return -3; }
    bool any = false;
    for (int j = 0; j < 3 * GRAIN_LEVELS; ++j) {
        if (!grain_finite(std[j]) || std[j] < 0.f) { set_error("%s: std[%d][%d] = %g must be finite and not negative", fn, j / GRAIN_LEVELS, j % GRAIN_LEVELS, (double)std[j]); return -3; }
        any = any || std[j] != 0.f;
    }
    if (amount == 0.f || !any) return 0;                             // nothing to add: nothing is launched and y keeps its bytes
    GrainApplyGeom g;
    g.Hp = Hp; g.Wp = Wp; g.fstride = y_frame_stride; g.plane = (int64_t)Hp * Wp;
    g.vec = (Wp & 3) == 0 && aligned16(y) && (y_frame_stride & 3) == 0;
    g.per_frame = g.vec ? g.plane / 4 : g.plane;
    g.amount = amount; g.inv_wg = inv_wg; g.seed = seed; g.frame0 = frame0;
    for (int c = 0; c < 3; ++c) g.w[c] = luma_w[c];
    for (int j = 0; j < 3 * GRAIN_LEVELS; ++j) g.std[j / GRAIN_LEVELS][j % GRAIN_LEVELS] = std[j];
    const int64_t items = g.per_frame * frames;
    return launch_sweep(grain_apply_kernel, items, stream, y, (const float *)templates, g, items);
}

}  // extern "C"
