// frame_finish_items.h -- the output finish (include/bsvd_hip.h: bsvd_blend_planar and the `_d` encoders), as plain __host__ __device__
// functions like the other frame headers: the blend's item body (frame_finish.hip is a grid-stride loop around it) and the dither value d
// that the item bodies of frame_surface_items.h / frame_rgb_items.h add to a scaled value right before their clamp and rintf.
// tools/debug/finish_bounds.hip runs all of them over exact-size heap buffers under AddressSanitizer; tests/finish_model.py states the
// same arithmetic in numpy, operation by operation.
//
// ---- the blend, per pixel, fp32, no contraction (sources.sh), y = the network's output, x = its input, both planes R, G, B ----
//   m_c   = s_c * y_c + om * x_c                  two products, one sum; om = (float)(1 - s_chroma), computed once on the host
//   l     = fmaf(w_B, x_B - y_B, fmaf(w_G, x_G - y_G, w_R * (x_R - y_R)))        the luma of the removed noise: R first, then G, then B
//   out_c = m_c + dl * l                          one product, one sum; dl = s_chroma - s_luma, one fp32 subtraction on the host
// The form is chosen for its ends (finite x and y):
//   s_luma = s_chroma = 1: om = 0 and dl = 0, so out_c = (y_c + 0) + 0 = y_c, bit for bit;
//   s_luma = s_chroma = 0: s_c = 0, om = 1, dl = 0, so out_c = (0 + x_c) + 0 = x_c, bit for bit;
//   s_luma == s_chroma:    dl * l is an exact zero, out_c = m_c, the plain two-product lerp.
// (One bit pattern is outside that: a value that is -0 comes out as +0, because -0 + +0 = +0.)  y + (1 - s)(x - y) has none of these ends.
//
// ---- the dither value d, in units of one code, in the OPEN interval (-0.5, 0.5) ----
// A sample is named by its component (0, 1, 2: Y, Cb, Cr of a YUV surface; R, G, B of an RGB one), the row and column of ITS OWN grid (the
// picture's for luma, 4:4:4 and RGB; the chroma grid for subsampled chroma) and its frame.  Alpha and filler samples have no d.
//   ORDERED  d = ((float)B[(row + r_c) & 7][(col + q_c) & 7] + 0.5f) * (1 / 64) - 0.5f, B the 8 x 8 Bayer matrix (0 .. 63; bayer8 below
//            computes B[y][x] from the bits of x ^ y and y), (r_c, q_c) = (0, 0), (2, 5), (5, 2) for components 0, 1, 2 so that the three do
//            not step together.  Every operation is exact in fp32; |d| <= 0.5 - 1/128.  The same for every frame.
//   RANDOM   d = ((float)((int32_t)(h >> 8) - 8388608) + 0.5f) * 2^-24, which is ((h >> 8) + 0.5) 2^-24 - 0.5 with every step exact in fp32
//            (the literal form rounds 16777215.5 up to 2^24 and d to the closed end 0.5), then limited to +-DITHER_RANDOM_MAX = 0.5 - 2^-7,
//            the largest |d| of ORDERED: t + d is ONE fp32 addition, rounded at t's precision, and fp32 is 2^-8 apart at the highest codes
//            (2^15 .. 2^16).  The limit leaves two such spacings below the tie: one for the rounding of the sum, one for a t that a
//            decode / encode round trip left one spacing off its code -- a whole code stays put at every served bit depth.
//            h = fmix32(kf ^ p), fmix32 the 32-bit finaliser of MurmurHash3 (Appleby): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13;
//            h *= 0xc2b2ae35; h ^= h >> 16.
//            kf: the 64-bit number n = (uint64)(frame0 + f) * 4 + component (frame0 + f: the frame's STREAM index; wraps mod 2^64) reduced as
//                kf = fmix32(seed ^ fmix32((uint32)n ^ fmix32((uint32)(n >> 32))))
//            p:  the 64-bit position row * 2^32 + col reduced as p = (uint32)col + (uint32)row * 0x9e3779b1 (mod 2^32).
// Both are rectangular (uniform) on purpose: a whole code t gives rint(t + d) = t, so half-to-even meets no tie it did not have before.
#pragma once
#include "frame_items.h"

namespace bsvd {

// what the encoders' kernels get: BsvdDither, checked, without its reserved field
struct Dither { int mode; uint32_t seed; int64_t frame0; };

constexpr float DITHER_RANDOM_MAX = 0.4921875f;   // 0.5 - 2^-7

// host: the caller's BsvdDither -> Dither; NULL is "off" (the entry points that take none).  -3 with the field named in bsvd_last_error().
void set_error(const char *fmt, ...);
static inline int dither_check(const char *fn, const BsvdDither *d, Dither *out)
{
    out->mode = BSVD_DITHER_NONE; out->seed = 0; out->frame0 = 0;
    if (!d) return 0;
    if (d->mode < BSVD_DITHER_NONE || d->mode > BSVD_DITHER_RANDOM) { set_error("%s: dither->mode = %d (BSVD_DITHER_NONE .. BSVD_DITHER_RANDOM)", fn, d->mode); return -3; }
    if (d->frame0 < 0) { set_error("%s: dither->frame0 = %lld must not be negative", fn, (long long)d->frame0); return -3; }
    if (d->reserved != 0) { set_error("%s: dither->reserved = %lld must be 0", fn, (long long)d->reserved); return -3; }
    out->mode = d->mode; out->seed = d->seed; out->frame0 = d->frame0;
    return 0;
}

BSVD_HD uint32_t fmix32(uint32_t h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// B[y][x] of the 8 x 8 Bayer matrix, x, y in 0 .. 7: the bits of x ^ y and y interleaved, lowest bits on top
BSVD_HD unsigned bayer8(unsigned x, unsigned y)
{
    const unsigned c = x ^ y;
    return ((c & 1) << 5) | ((y & 1) << 4) | ((c & 2) << 2) | ((y & 2) << 1) | ((c & 4) >> 1) | ((y & 4) >> 2);
}

BSVD_HD float dither_ordered(int comp, int row, int col)
{
    const unsigned r = (unsigned)row + (comp == 0 ? 0u : comp == 1 ? 2u : 5u), q = (unsigned)col + (comp == 0 ? 0u : comp == 1 ? 5u : 2u);
    return ((float)bayer8(q & 7, r & 7) + 0.5f) * 0.015625f - 0.5f;
}

// the (seed, frame, component) part of the hash key: once per item and component
BSVD_HD uint32_t dither_frame_key(uint32_t seed, int64_t frame, int comp)
{
    const uint64_t n = (uint64_t)frame * 4u + (uint64_t)comp;
    return fmix32(seed ^ fmix32((uint32_t)n ^ fmix32((uint32_t)(n >> 32))));
}

BSVD_HD float dither_random(uint32_t kf, int row, int col)
{
    const uint32_t h = fmix32(kf ^ ((uint32_t)col + (uint32_t)row * 0x9e3779b1u));
    const float d = ((float)((int32_t)(h >> 8) - 8388608) + 0.5f) * 5.9604644775390625e-08f;
    return fminf(fmaxf(d, -DITHER_RANDOM_MAX), DITHER_RANDOM_MAX);
}

// The d of N consecutive samples of one row of one component's grid, added in place to their scaled values.  di.mode != NONE (the
// callers branch on it once per item: the branch is wave-uniform, and with dither off no value is touched).
template <int N>
BSVD_HD void dither_add(const Dither &di, int64_t f, int comp, int row, int col0, float *t)
{
    if (di.mode == BSVD_DITHER_ORDERED) {
#pragma unroll
        for (int q = 0; q < N; ++q) t[q] += dither_ordered(comp, row, col0 + q);
    } else {
        const uint32_t kf = dither_frame_key(di.seed, di.frame0 + f, comp);
#pragma unroll
        for (int q = 0; q < N; ++q) t[q] += dither_random(kf, row, col0 + q);
    }
}

// ---------------------------------------------------------------------------------------------
// the blend.  An item is 4 consecutive elements of a plane (vec: Wp % 4 == 0, both pointers 16-byte aligned, both frame strides multiples
// of 4: one float4 per plane and tensor) or one element; the planes are contiguous Hp x Wp, so an item never leaves its plane.
struct BlendGeom { int64_t y_fs, x_fs, plane, per_frame; int vec; float s_c, om, dl, w[3]; };

BSVD_HD void blend_pixel(const BlendGeom &g, float *y3, const float *x3)
{
    const float l = fmaf(g.w[2], x3[2] - y3[2], fmaf(g.w[1], x3[1] - y3[1], g.w[0] * (x3[0] - y3[0])));
    const float t = g.dl * l;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float m = g.s_c * y3[c] + g.om * x3[c];
        y3[c] = m + t;
    }
}

BSVD_HD void blend_planar_item(float *y, const float *x, const BlendGeom &g, int64_t i)
{
    const int64_t f = i / g.per_frame, e = (i - f * g.per_frame) * (g.vec ? 4 : 1);
    float *yp = y + f * g.y_fs + e;
    const float *xp = x + f * g.x_fs + e;
    if (g.vec) {
        float4 yv[3], xv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            yv[c] = *reinterpret_cast<const float4 *>(yp + c * g.plane);
            xv[c] = *reinterpret_cast<const float4 *>(xp + c * g.plane);
        }
        float a[4][3], b[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[0][c] = yv[c].x; a[1][c] = yv[c].y; a[2][c] = yv[c].z; a[3][c] = yv[c].w;
            b[0][c] = xv[c].x; b[1][c] = xv[c].y; b[2][c] = xv[c].z; b[3][c] = xv[c].w;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) blend_pixel(g, a[q], b[q]);
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4 *>(yp + c * g.plane) = make_float4(a[0][c], a[1][c], a[2][c], a[3][c]);
    } else {
        float a[3] = {yp[0], yp[g.plane], yp[2 * g.plane]};
        const float b[3] = {xp[0], xp[g.plane], xp[2 * g.plane]};
        blend_pixel(g, a, b);
        yp[0] = a[0]; yp[g.plane] = a[1]; yp[2 * g.plane] = a[2];
    }
}

}  // namespace bsvd
