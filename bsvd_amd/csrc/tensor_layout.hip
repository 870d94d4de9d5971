// tensor_layout.hip -- the bandwidth-bound layout helpers of the ABI (include/bsvd_hip.h): NCHW <-> NHWC at the clip's entry and exit, uint8
// frame I/O, halo slices for frame-window sharding, and the transformed-domain tensors of the Winograd form (bsvd_to_v and its sizes).
#include <math.h>
#include "bsvd_internal.h"
#include "frame_items.h"      // the item bodies of the pad / crop uint8 kernels
#include "wino_forms.h"

namespace bsvd {

// ---------------------------------------------------------------------------------------------
// clip entry / exit
__global__ void nchw_to_nhwc_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int HW, int Cpad, int64_t total_pix)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total_pix; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / HW, pix = i - f * HW;
        const float *s = src + f * (int64_t)C * HW + pix;
        float *d = dst + i * Cpad;
        for (int c = 0; c < Cpad; ++c) d[c] = c < C ? s[(int64_t)c * HW] : 0.f;
    }
}

__global__ void nhwc_to_nchw_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int HW, int Cpad, int64_t total_pix, int do_clamp, float lo, float hi)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total_pix; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / HW, pix = i - f * HW;
        const float *s = src + i * Cpad;
        float *d = dst + f * (int64_t)C * HW + pix;
        for (int c = 0; c < C; ++c) {
            float v = s[c];
            if (do_clamp) v = fminf(fmaxf(v, lo), hi);
            d[(int64_t)c * HW] = v;
        }
    }
}

// channels [c0, c0 + n) of an NHWC frame <-> a compact [pixels][n] slice (unpack: slice -> frame)
__global__ void halo_copy_kernel(float *__restrict__ frame, float *__restrict__ slice, int64_t total, int C, int c0, int n, int unpack)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i / n;
        float *f = frame + pix * C + c0 + (int)(i - pix * n);
        if (unpack) *f = slice[i];
        else slice[i] = *f;
    }
}

// split16 half-chunk slice (fold == 8): channels [c0, c0+8) of a split16 frame are two 16-byte pieces of one chunk
// (hi at chunk*16 + half*4 floats, lo 8 floats further); the compact slice stores them as [hi x8 | lo x8] per pixel
__global__ void halo_pack_split8_kernel(const float *__restrict__ frame, float *__restrict__ dst, int64_t HW, int C, int c0, int unpack)
{
    const int off = (c0 >> 4) * 16 + ((c0 >> 3) & 1) * 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 2 * HW; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i >> 1;
        const int part = (int)(i & 1);                       // 0 = hi, 1 = lo
        float *f = const_cast<float *>(frame) + pix * C + off + part * 8;
        float *d = dst + pix * 8 + part * 4;
        if (unpack) *reinterpret_cast<float4 *>(f) = *reinterpret_cast<const float4 *>(d);
        else *reinterpret_cast<float4 *>(d) = *reinterpret_cast<const float4 *>(f);
    }
}

// uint8 frame I/O: HWC or planar uint8 -> planar fp32 in [0,1] (+ constant trailing channels, e.g. the
// sigma map) and back with the reference's clamp + round-half-even (tensor2img, img_util.py:66,87-90)
__global__ void u8_to_planar_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, int C, int Cout, int HW, int hwc, float const_val, int64_t total)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i % HW;
        const int64_t fc = i / HW;
        const int c = (int)(fc % Cout);
        const int64_t f = fc / Cout;
        float v = const_val;
        if (c < C) v = (float)src[hwc ? (f * HW + pix) * C + c : (f * C + c) * HW + pix] / 255.0f;
        dst[i] = v;
    }
}

__global__ void planar_to_u8_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, int C, int HW, int hwc, int reverse_ch, int64_t total)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i % HW;
        const int64_t fc = i / HW;
        const int c = (int)(fc % C);
        const int64_t f = fc / C;
        const float v = fminf(fmaxf(src[i], 0.f), 1.f) * 255.0f;
        const int co = reverse_ch ? C - 1 - c : c;
        dst[hwc ? (f * HW + pix) * C + co : (f * C + co) * HW + pix] = (uint8_t)rintf(v);
    }
}

// bsvd_to_v: one thread per (frame, row, group, 8-channel block): the A = M + 2 pixels of the group (zero outside the image), BT per channel in
// fp32 (the kernels' WinoForm<M>::input), every transformed value split into an fp16 pair with the kernels' saturating conversions
template <int M>
__global__ void to_v_kernel(const float *__restrict__ x, int64_t x_fs, int x_f32, float *__restrict__ v, int64_t v_fs, int frames, int H, int W, int C, int wg)
{
    constexpr int A = M + 2;
    using F = WinoForm<M>;
    fp16_saturate_on();
    const int c8n = C >> 3;
    const int64_t total = (int64_t)frames * H * wg * c8n;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % c8n);
        int64_t r = i / c8n;
        const int g = (int)(r % wg); r /= wg;
        const int row = (int)(r % H);
        const int f = (int)(r / H);
        const int chunk = c8 >> 1, half = c8 & 1;
        float d[A][8];
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const int px = M * g - 1 + a;
            const bool ok = px >= 0 && px < W;
            const float *src = x + f * x_fs + ((int64_t)row * W + (ok ? px : 0)) * C;
            if (x_f32) {
#pragma unroll
                for (int k = 0; k < 8; ++k) d[a][k] = ok ? src[c8 * 8 + k] : 0.f;
            } else {
                const _Float16 *hp = reinterpret_cast<const _Float16 *>(src + chunk * 16) + half * 8;
#pragma unroll
                for (int k = 0; k < 8; ++k) d[a][k] = ok ? (float)hp[k] + (float)hp[16 + k] : 0.f;
            }
        }
        _Float16 hi[A][8], lo[A][8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float din[A], vout[A];
#pragma unroll
            for (int a = 0; a < A; ++a) din[a] = d[a][k];
            F::input(din, vout);
#pragma unroll
            for (int a = 0; a < A; ++a) {
                hi[a][k] = (_Float16)vout[a];
                lo[a][k] = (_Float16)__builtin_fmaf((float)hi[a][k], -1.0f, vout[a]);
            }
        }
        // block (row, tile g / 8, chunk): [position][quarter][8 groups] x 16 B, then the edge line [side][quarter] x 16 B
        constexpr int BLK = v_block_floats(M);
        float *dst = v + f * v_fs + ((int64_t)(row * (wg >> 3) + (g >> 3)) * (C >> 4) + chunk) * BLK;
        const int gl = g & 7;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            *reinterpret_cast<float4 *>(dst + ((a * 4 + half) * 8 + gl) * 4) = *reinterpret_cast<const float4 *>(hi[a]);
            *reinterpret_cast<float4 *>(dst + ((a * 4 + 2 + half) * 8 + gl) * 4) = *reinterpret_cast<const float4 *>(lo[a]);
        }
        if (gl == 0) {
            *reinterpret_cast<float4 *>(dst + A * 128 + half * 4) = *reinterpret_cast<const float4 *>(hi[0]);
            *reinterpret_cast<float4 *>(dst + A * 128 + (2 + half) * 4) = *reinterpret_cast<const float4 *>(lo[0]);
        }
        if (gl == 7) {
            *reinterpret_cast<float4 *>(dst + A * 128 + (4 + half) * 4) = *reinterpret_cast<const float4 *>(hi[A - 1]);
            *reinterpret_cast<float4 *>(dst + A * 128 + (6 + half) * 4) = *reinterpret_cast<const float4 *>(lo[A - 1]);
        }
    }
}

// u8_to_planar_kernel / planar_to_u8_kernel with reflect pad / crop (bsvd_u8_to_planar_pad / bsvd_planar_to_u8_crop) in the YUV kernels' shape: an item is 4 columns of a
// picture row, one float4 per plane on the fp32 side, one group of bytes on the uint8 side (frame_items.h)
__global__ __launch_bounds__(256) void u8_to_planar_pad_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, U8Geom g, int64_t items)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) u8_to_planar_pad_item(src, dst, g, i);
}

__global__ __launch_bounds__(256) void planar_to_u8_crop_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, U8Geom g, int64_t items)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) planar_to_u8_crop_item(src, dst, g, i);
}

// bsvd_halo_pack / bsvd_halo_unpack: one check, one copy in either direction
static int halo_copy(const void *frame, const void *slice, int32_t HW, int32_t C, int32_t c0, int32_t n, int32_t dtype, int unpack, void *stream)
{
    const char *verb = unpack ? "unpack" : "pack";
    if (dtype != BSVD_F32 && dtype != BSVD_F16X3) { set_error("bsvd_halo_%s: dtype %d not supported", verb, dtype); return -2; }
    if (!frame || !slice || HW <= 0 || C <= 0 || c0 < 0 || n <= 0 || c0 + n > C) { set_error("bsvd_halo_%s: bad arguments", verb); return -3; }
    float *f = const_cast<float *>((const float *)frame), *s = const_cast<float *>((const float *)slice);
    if (dtype == BSVD_F32) return launch_sweep(halo_copy_kernel, (int64_t)HW * n, stream, f, s, (int64_t)HW * n, C, c0, n, unpack);
    // half-chunk slice of a split16 frame (whole chunks are plain float ranges: use BSVD_F32)
    if (n != 8 || (c0 & 7) || (C & 15)) { set_error("bsvd_halo_%s: BSVD_F16X3 %ss one 8-channel half chunk (n == 8, c0 %% 8 == 0)", verb, verb); return -3; }
    return launch_sweep(halo_pack_split8_kernel, 2 * (int64_t)HW, stream, (const float *)f, s, (int64_t)HW, C, c0, unpack);
}

// the checks of bsvd_u8_to_planar_pad / bsvd_planar_to_u8_crop: picture H x W, tensor Hp x Wp -> items (negative: refused)
static int64_t u8_pad_check(const char *fn, const void *src, const void *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t Hp, int32_t Wp)
{
    if (!src) { set_error("%s: src is NULL", fn); return -3; }
    if (!dst) { set_error("%s: dst is NULL", fn); return -3; }
    if (frames <= 0) { set_error("%s: frames = %d must be positive", fn, frames); return -3; }
    if (C <= 0) { set_error("%s: C = %d must be positive", fn, C); return -3; }
    if (H <= 0) { set_error("%s: H = %d must be positive", fn, H); return -3; }
    if (W <= 0) { set_error("%s: W = %d must be positive", fn, W); return -3; }
    if (Hp < H) { set_error("%s: Hp = %d is below H = %d", fn, Hp, H); return -3; }
    if (Wp < W) { set_error("%s: Wp = %d is below W = %d", fn, Wp, W); return -3; }
    if (Hp - H >= H) { set_error("%s: Hp = %d pads H = %d by a whole dimension or more (reflect is defined up to 2 H - 1)", fn, Hp, H); return -3; }
    if (Wp - W >= W) { set_error("%s: Wp = %d pads W = %d by a whole dimension or more (reflect is defined up to 2 W - 1)", fn, Wp, W); return -3; }
    const int64_t per_frame = (int64_t)H * items_per_row(W);
    if (per_frame > 0x7fffffff) { set_error("%s: H x W = %d x %d: more than 2^31 items per frame", fn, H, W); return -3; }
    return per_frame * frames;
}

}  // namespace bsvd

using namespace bsvd;

extern "C" {

int bsvd_nchw_to_nhwc(const float *src, void *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t C_pad, int32_t dtype, void *stream)
{
    if (dtype != BSVD_F32) { set_error("bsvd_nchw_to_nhwc: dtype %d not supported", dtype); return -2; }
    if (!src || !dst || frames <= 0 || C <= 0 || H <= 0 || W <= 0 || C_pad < C) { set_error("bsvd_nchw_to_nhwc: bad arguments"); return -3; }
    const int64_t total = (int64_t)frames * H * W;
    return launch_sweep(nchw_to_nhwc_kernel, total, stream, src, (float *)dst, C, H * W, C_pad, total);
}

int bsvd_nhwc_to_nchw(const void *src, float *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t C_pad, int32_t dtype, int32_t do_clamp, float lo, float hi, void *stream)
{
    if (dtype != BSVD_F32) { set_error("bsvd_nhwc_to_nchw: dtype %d not supported", dtype); return -2; }
    if (!src || !dst || frames <= 0 || C <= 0 || H <= 0 || W <= 0 || C_pad < C) { set_error("bsvd_nhwc_to_nchw: bad arguments"); return -3; }
    const int64_t total = (int64_t)frames * H * W;
    return launch_sweep(nhwc_to_nchw_kernel, total, stream, (const float *)src, dst, C, H * W, C_pad, total, do_clamp, lo, hi);
}

int bsvd_u8_to_planar(const uint8_t *src, float *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t src_hwc, int32_t const_channels, float const_val, void *stream)
{
    if (!src || !dst || frames <= 0 || C <= 0 || H <= 0 || W <= 0 || const_channels < 0) { set_error("bsvd_u8_to_planar: bad arguments"); return -3; }
    const int64_t total = (int64_t)frames * (C + const_channels) * H * W;
    return launch_sweep(u8_to_planar_kernel, total, stream, src, dst, C, C + const_channels, H * W, src_hwc ? 1 : 0, const_val, total);
}

int bsvd_planar_to_u8(const float *src, uint8_t *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t dst_hwc, int32_t reverse_channels, void *stream)
{
    if (!src || !dst || frames <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("bsvd_planar_to_u8: bad arguments"); return -3; }
    const int64_t total = (int64_t)frames * C * H * W;
    return launch_sweep(planar_to_u8_kernel, total, stream, src, dst, C, H * W, dst_hwc ? 1 : 0, reverse_channels ? 1 : 0, total);
}

int bsvd_u8_to_planar_pad(const uint8_t *src, float *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t Hp, int32_t Wp, int32_t src_hwc,
                          int32_t const_channels, float const_val, void *stream)
{
    const int64_t items = u8_pad_check("bsvd_u8_to_planar_pad", src, dst, frames, C, H, W, Hp, Wp);
    if (items < 0) return (int)items;
    if (const_channels < 0) { set_error("bsvd_u8_to_planar_pad: const_channels = %d must not be negative", const_channels); return -3; }
    const U8Geom g = {C, const_channels, H, W, Hp, Wp, src_hwc ? 1 : 0, 0, (Wp & 3) == 0 && aligned16(dst), const_val};
    return launch_sweep(u8_to_planar_pad_kernel, items, stream, src, dst, g, items);
}

int bsvd_planar_to_u8_crop(const float *src, uint8_t *dst, int32_t frames, int32_t C, int32_t Hp, int32_t Wp, int32_t H, int32_t W, int32_t dst_hwc,
                           int32_t reverse_channels, void *stream)
{
    const int64_t items = u8_pad_check("bsvd_planar_to_u8_crop", src, dst, frames, C, H, W, Hp, Wp);
    if (items < 0) return (int)items;
    const U8Geom g = {C, 0, H, W, Hp, Wp, dst_hwc ? 1 : 0, reverse_channels ? 1 : 0, (Wp & 3) == 0 && aligned16(src), 0.f};
    return launch_sweep(planar_to_u8_crop_kernel, items, stream, src, dst, g, items);
}

int bsvd_halo_pack(const void *frame, void *dst, int32_t HW, int32_t C, int32_t c0, int32_t n, int32_t dtype, void *stream) { return halo_copy(frame, dst, HW, C, c0, n, dtype, 0, stream); }
int bsvd_halo_unpack(const void *src, void *frame, int32_t HW, int32_t C, int32_t c0, int32_t n, int32_t dtype, void *stream) { return halo_copy(frame, src, HW, C, c0, n, dtype, 1, stream); }

int32_t bsvd_v_groups(int32_t W, int32_t m) { return wino_m_ok(m) && W > 0 ? v_groups(W, m) : -1; }

int64_t bsvd_v_frame_elems(int32_t H, int32_t W, int32_t C, int32_t m)
{
    if (!wino_m_ok(m) || H <= 0 || W <= 0 || C <= 0 || (C & 15)) { set_error("bsvd_v_frame_elems: m = 2 | 4 | 6, C %% 16 == 0"); return -1; }
    return v_plane_elems(H, W, C, m) + v_edge_elems(H, W, C, m);
}

int bsvd_to_v(const void *x, int64_t x_fs, int32_t x_f32, void *v, int64_t v_fs, int32_t frames, int32_t H, int32_t W, int32_t C, int32_t m, void *stream)
{
    if (!x || !v || frames <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 15)) { set_error("bsvd_to_v: bad arguments (C %% 16 == 0)"); return -3; }
    if (!wino_m_ok(m)) { set_error("bsvd_to_v: m = %d (2, 4 or 6)", m); return -2; }
    if (!aligned16(x) || !aligned16(v) || (v_fs & 3)) { set_error("bsvd_to_v: 16-byte aligned tensors"); return -3; }
    if (v_fs < bsvd_v_frame_elems(H, W, C, m)) { set_error("bsvd_to_v: v_frame_stride < bsvd_v_frame_elems"); return -3; }
    const int wg = v_groups(W, m);
    // pad groups and the edge record: zeros -- of the frames themselves, never of what the caller keeps between them (v_fs > the frame)
    hipError_t e = hipMemset2DAsync(v, (size_t)v_fs * 4, 0, (size_t)bsvd_v_frame_elems(H, W, C, m) * 4, (size_t)frames, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    return launch_sweep(m == 2 ? to_v_kernel<2> : m == 4 ? to_v_kernel<4> : to_v_kernel<6>, (int64_t)frames * H * wg * (C >> 3), stream,
                        (const float *)x, x_fs, x_f32, (float *)v, v_fs, frames, H, W, C, wg);
}

}  // extern "C"
