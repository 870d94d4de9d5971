// frame_rgb_items.h -- the item bodies of the RGB surface entry points (include/bsvd_hip.h: bsvd_rgb_to_planar, bsvd_planar_to_rgb), plain
// __host__ __device__ functions on the item arithmetic of frame_items.h, like the YUV bodies of frame_surface_items.h: the kernels of
// frame_rgb.hip are grid-stride loops around them.
//
// A surface format is three compile-time facts: the layout (packed pixels; packed 2:10:10:10 words; planes), the bytes of a sample (1, 2;
// 4 for the word) and the number of SLOTS -- samples of a pixel, fields of a word, planes.  Which component sits in which slot, the
// sample's mask and the scale are kernel arguments: one instantiation serves rgb24 and bgr24, rgba, bgra, argb, abgr and the four fillers,
// all of gbrp10le / 12le / 16le.  A runtime component position would index registers; it indexes planes instead: slot j of a pixel belongs
// to component chan[j], and chan[j] only ever selects the fp32 PLANE (or the alpha side plane) the slot's four values go to or come from.
//
// Work over lanes is that of the uint8 pad / crop kernels: an ITEM is 4 columns of one picture row, consecutive lanes take consecutive
// items, a lane moves one float4 per plane on the fp32 side and the item's 4 pixels -- 12, 16, 24 or 32 bytes of a packed row, 16 of an
// x2 row, 4 or 8 per plane -- as ONE load or store on the surface side.  A surface promises no more than its sample's alignment (a packed
// 3-byte row starts anywhere), hence the memcpy: gfx950 takes a wide global access at any address.  The part item that W % 4 leaves at
// the end of a row moves pixel by pixel, and so does the fp32 side when Wp % 4 != 0 or the tensor is not 16-byte aligned: the same
// arithmetic on the same codes, the same bits.
#pragma once
#include <type_traits>
#include "frame_items.h"
#include "frame_finish_items.h"

namespace bsvd {

template <int LAY_, int SB_, int SLOTS_> struct RgbFmt {
    static constexpr int LAY = LAY_, SB = SB_, SLOTS = SLOTS_;
    using S = typename std::conditional<SB_ == 1, uint8_t, typename std::conditional<SB_ == 2, uint16_t, uint32_t>::type>::type;   // the container
    using A = typename std::conditional<SB_ == 1, uint8_t, uint16_t>::type;                                                     // of the alpha side plane
};

// chan[j]: the component (0 R, 1 G, 2 B, 3 the fourth sample) of slot j.  off / pitch in bytes, resolved by the host (no zeros left).
struct RgbGeom { int H, W, Hp, Wp, cc, vec; float const_val; int chan[4]; unsigned mask; int64_t fstride, off[4], pitch[4]; };
struct RgbDecode { float sub, div; };                      // v = ((float)code - sub) / div
struct RgbEncode { float mul, add, lo, hi; unsigned fill; };   // code = clamp(rintf(clamp01(v) * mul + add), lo, hi); fill: the fourth sample without alpha_in

template <class T, int N> BSVD_HD void load_group(const uint8_t *p, T *v) { __builtin_memcpy(v, __builtin_assume_aligned(p, sizeof(T)), N * sizeof(T)); }
template <class T, int N> BSVD_HD void store_group(uint8_t *p, const T *v) { __builtin_memcpy(__builtin_assume_aligned(p, sizeof(T)), v, N * sizeof(T)); }

// the codes of the item's n <= 4 pixels, by slot, not yet masked to `bits` (x2 fields are: nothing of a field is ignored)
template <class F>
BSVD_HD void load_codes(const uint8_t *fr, const RgbGeom &g, const PadItem &it, unsigned code[F::SLOTS][4])
{
    using S = typename F::S;
    constexpr int K = F::SLOTS;
    if constexpr (F::LAY == BSVD_RGB_PLANAR) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const uint8_t *p = fr + g.off[j] + (int64_t)it.row * g.pitch[j] + (int64_t)it.x0 * F::SB;
            S v[4] = {};
            if (it.n == 4) load_group<S, 4>(p, v);
            else {
#pragma unroll
                for (int q = 0; q < 3; ++q) if (q < it.n) load_group<S, 1>(p + q * F::SB, v + q);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) code[j][q] = v[q];
        }
    } else if constexpr (F::LAY == BSVD_RGB_PACKED) {
        const uint8_t *p = fr + g.off[0] + (int64_t)it.row * g.pitch[0] + (int64_t)it.x0 * (K * F::SB);
        S v[4 * K] = {};
        if (it.n == 4) load_group<S, 4 * K>(p, v);
        else {
#pragma unroll
            for (int q = 0; q < 3; ++q) if (q < it.n) load_group<S, K>(p + q * K * F::SB, v + q * K);
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) code[j][q] = v[q * K + j];
    } else {
        const uint8_t *p = fr + g.off[0] + (int64_t)it.row * g.pitch[0] + (int64_t)it.x0 * 4;
        uint32_t w[4] = {};
        if (it.n == 4) load_group<uint32_t, 4>(p, w);
        else {
#pragma unroll
            for (int q = 0; q < 3; ++q) if (q < it.n) load_group<uint32_t, 1>(p + q * 4, w + q);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) code[j][q] = w[q] >> (10 * j);
    }
}

// ... and back: codes already legal, below 2^bits
template <class F>
BSVD_HD void store_codes(uint8_t *fr, const RgbGeom &g, const PadItem &it, const unsigned code[F::SLOTS][4])
{
    using S = typename F::S;
    constexpr int K = F::SLOTS;
    if constexpr (F::LAY == BSVD_RGB_PLANAR) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            uint8_t *p = fr + g.off[j] + (int64_t)it.row * g.pitch[j] + (int64_t)it.x0 * F::SB;
            const S v[4] = {(S)code[j][0], (S)code[j][1], (S)code[j][2], (S)code[j][3]};
            if (it.n == 4) store_group<S, 4>(p, v);
            else {
#pragma unroll
                for (int q = 0; q < 3; ++q) if (q < it.n) store_group<S, 1>(p + q * F::SB, v + q);
            }
        }
    } else if constexpr (F::LAY == BSVD_RGB_PACKED) {
        uint8_t *p = fr + g.off[0] + (int64_t)it.row * g.pitch[0] + (int64_t)it.x0 * (K * F::SB);
        S v[4 * K];
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q * K + j] = (S)code[j][q];
        if (it.n == 4) store_group<S, 4 * K>(p, v);
        else {
#pragma unroll
            for (int q = 0; q < 3; ++q) if (q < it.n) store_group<S, K>(p + q * K * F::SB, v + q * K);
        }
    } else {
        uint8_t *p = fr + g.off[0] + (int64_t)it.row * g.pitch[0] + (int64_t)it.x0 * 4;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = 0xc0000000u | code[0][q] | (code[1][q] << 10) | (code[2][q] << 20);
        if (it.n == 4) store_group<uint32_t, 4>(p, w);
        else {
#pragma unroll
            for (int q = 0; q < 3; ++q) if (q < it.n) store_group<uint32_t, 1>(p + q * 4, w + q);
        }
    }
}

BSVD_HD void rgb_put(float *plane, const Images &im, const PadItem &it, const float *v, const RgbGeom &g)
{
    put_own(plane + (int64_t)it.row * g.Wp + it.x0, it.n, v, g.vec);
    if (im.any()) put_images(plane, im, it.row, it.x0, it.n, v, g.W, g.Wp, g.vec);
}

// ---------------------------------------------------------------------------------------------
// decode: surface -> [frames][3 + cc][Hp][Wp], mirror images of the pad region included (frame_items.h); alpha: the side plane or NULL
template <class F>
BSVD_HD void rgb_to_planar_item(const uint8_t *src, float *dst, void *alpha, const RgbGeom &g, const RgbDecode &k, int64_t i)
{
    using A = typename F::A;
    const PadItem it = pad_item_of(i, g.H, g.W, 1);
    const int64_t plane = (int64_t)g.Hp * g.Wp;
    const Images im = images_of(it.row, it.x0, it.n, g.H, g.W, g.Hp, g.Wp);
    float *d = dst + it.f * (3 + g.cc) * plane;
    unsigned code[F::SLOTS][4];
    load_codes<F>(src + it.f * g.fstride, g, it, code);
#pragma unroll
    for (int j = 0; j < F::SLOTS; ++j) {
        const int c = g.chan[j];
        if (c < 3) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = ((float)(code[j][q] & g.mask) - k.sub) / k.div;
            rgb_put(d + c * plane, im, it, v, g);
        } else if (alpha) {
            if constexpr (F::SLOTS == 4) {
                uint8_t *o = (uint8_t *)alpha + ((it.f * g.H + it.row) * (int64_t)g.W + it.x0) * (int64_t)sizeof(A);
                const A a[4] = {(A)(code[j][0] & g.mask), (A)(code[j][1] & g.mask), (A)(code[j][2] & g.mask), (A)(code[j][3] & g.mask)};
                if (it.n == 4) store_group<A, 4>(o, a);
                else {
#pragma unroll
                    for (int q = 0; q < 3; ++q) if (q < it.n) store_group<A, 1>(o + q * sizeof(A), a + q);
                }
            }
        }
    }
    const float kc[4] = {g.const_val, g.const_val, g.const_val, g.const_val};
    for (int c = 3; c < 3 + g.cc; ++c) rgb_put(d + c * plane, im, it, kc, g);
}

BSVD_HD unsigned rgb_code(float v, const RgbEncode &k) { return (unsigned)fminf(fmaxf(rintf(clamp01(v) * k.mul + k.add), k.lo), k.hi); }

// ... with the dither value d (frame_finish_items.h) joining the scaled value right before rintf: clamp(rintf(t + d), lo, hi)
BSVD_HD unsigned rgb_code_d(float v, const RgbEncode &k, float d) { return (unsigned)fminf(fmaxf(rintf(clamp01(v) * k.mul + k.add + d), k.lo), k.hi); }

// encode: [frames][3][Hp][Wp] -> surface; only picture rows and columns are read.  alpha: the side plane, or NULL (the fourth sample is k.fill).
// Dither touches R, G and B on the picture's grid, never the fourth sample; with di.mode == BSVD_DITHER_NONE the codes are rgb_code's.
template <class F>
BSVD_HD void planar_to_rgb_item(const float *src, uint8_t *dst, const void *alpha, const RgbGeom &g, const RgbEncode &k, const Dither &di, int64_t i)
{
    using A = typename F::A;
    const PadItem it = pad_item_of(i, g.H, g.W, 1);
    const int64_t plane = (int64_t)g.Hp * g.Wp;
    const float *s = src + it.f * 3 * plane + (int64_t)it.row * g.Wp + it.x0;
    unsigned code[F::SLOTS][4] = {};
#pragma unroll
    for (int j = 0; j < F::SLOTS; ++j) {
        const int c = g.chan[j];
        if (c < 3) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (g.vec && it.n == 4) {
                const float4 x = *reinterpret_cast<const float4 *>(s + c * plane);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (q < it.n) v[q] = s[c * plane + q];
            }
            if (di.mode != BSVD_DITHER_NONE) {
                float d[4] = {0.f, 0.f, 0.f, 0.f};
                dither_add<4>(di, it.f, c, it.row, it.x0, d);
#pragma unroll
                for (int q = 0; q < 4; ++q) code[j][q] = rgb_code_d(v[q], k, d[q]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) code[j][q] = rgb_code(v[q], k);
            }
        } else if constexpr (F::SLOTS == 4) {
            A a[4] = {(A)k.fill, (A)k.fill, (A)k.fill, (A)k.fill};
            if (alpha) {
                const uint8_t *p = (const uint8_t *)alpha + ((it.f * g.H + it.row) * (int64_t)g.W + it.x0) * (int64_t)sizeof(A);
                if (it.n == 4) load_group<A, 4>(p, a);
                else {
#pragma unroll
                    for (int q = 0; q < 3; ++q) if (q < it.n) load_group<A, 1>(p + q * sizeof(A), a + q);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) code[j][q] = a[q] & g.mask;
        }
    }
    store_codes<F>(dst + it.f * g.fstride, g, it, code);
}

// dither off: the body as its callers of before the finish stage name it
template <class F>
BSVD_HD void planar_to_rgb_item(const float *src, uint8_t *dst, const void *alpha, const RgbGeom &g, const RgbEncode &k, int64_t i)
{
    planar_to_rgb_item<F>(src, dst, alpha, g, k, Dither{BSVD_DITHER_NONE, 0u, 0}, i);
}

}  // namespace bsvd
