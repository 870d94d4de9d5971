// frame_items.h -- the frame I/O kernels' work on ONE item, as plain __host__ __device__ functions: the item bodies of the uint8 pad / crop
// entry points (include/bsvd_hip.h: bsvd_u8_to_planar_pad, bsvd_planar_to_u8_crop), and what they share with the YUV bodies of
// frame_surface_items.h and with frame_sigma_items.h: the item -> address arithmetic, the mirror images of the pad region and the
// constants of the colour conversion.  The kernels are grid-stride loops around these bodies; a host program can run the same bodies over
// exact-size heap buffers under AddressSanitizer (tools/debug/frame_pad_bounds.hip, tools/debug/yuv_surface_bounds.hip), which sees the
// reads a GPU run cannot show: the tail of a part item, pitch padding, the bytes behind the last row of the last frame.
//
// Pad rule (one for all entry points): the picture is H x W, the network's tensor Hp x Wp with Hp >= H, Wp >= W, pad on the right and bottom only,
// padded element (r, c) = converted picture element (refl_H(r), refl_W(c)), refl_N(i) = i below N, else 2 (N - 1) - i (torch's 'reflect').
// On the way in, the lane that owns a picture element writes it AND its mirror images (at most one row image, one column image and the
// corner they span): every destination element has exactly one writer, and a pad element holds the bits of its source by construction.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "bsvd_hip.h"

#define BSVD_HD __host__ __device__ __forceinline__

namespace bsvd {

// decode: codes -> (Y - y_off) * y_mul, (C - c_off) * c_mul -> R = y + r_cr cr, G = y - g_cr cr - g_cb cb, B = y + b_cb cb.  NOT clamped.
struct YuvDecode { float y_off, y_mul, c_off, c_mul, r_cr, g_cr, g_cb, b_cb; };

// encode: clamp RGB to [0,1] -> Y' = kr R + kg G + kb B, B - Y', R - Y' -> chroma filter on the differences (it is linear; cb_mul / cr_mul
// carry the 1 / (2 (1 - K)) of Cb / Cr with the code scale) -> scale + offset -> clamp to the legal codes -> rintf
struct YuvEncode { float kr, kg, kb, y_mul, y_off, cb_mul, cr_mul, c_off, y_lo, y_hi, c_lo, c_hi; };

BSVD_HD float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// ---------------------------------------------------------------------------------------------
// item -> address / count arithmetic of the pad / crop kernels

// where index i of a dimension of N picture elements, padded to Np, appears a second time: 2 (N - 1) - i if that lies in [N, Np), else -1
BSVD_HD int mirror_of(int i, int N, int Np)
{
    const int m = 2 * (N - 1) - i;
    return m >= N && m < Np ? m : -1;
}

// an item of `rows_per_item` picture rows x 4 columns: frame, first row, first column and the number of picture columns it holds -- 4, or
// the rest of the row in its last item (1..3; 2 for a 4:2:0 surface, whose W is even).  Items of one frame fit 32 bits (checked by the host).
struct PadItem { int64_t f; int row, x0, n; };
BSVD_HD int items_per_row(int W) { return (W + 3) >> 2; }
BSVD_HD PadItem pad_item_of(int64_t i, int item_rows, int W, int rows_per_item)
{
    const int wq = items_per_row(W);
    const int64_t per_frame = (int64_t)item_rows * wq;
    PadItem it;
    it.f = i / per_frame;
    const int r = (int)(i - it.f * per_frame);
    const int j = r / wq;
    it.row = j * rows_per_item;
    it.x0 = (r - j * wq) * 4;
    it.n = W - it.x0 < 4 ? W - it.x0 : 4;
    return it;
}

// Where an item's n <= 4 values of picture row `row`, columns x0 .. x0 + n - 1, go in a plane Wp wide.  Every item stores them at their own
// place (one float4 for a whole item when the rows allow it).  The few items near the right and bottom edge also own IMAGES: `cols` says
// that some of the columns has one, `mrow` is the row's image or -1.  any() is false for all but those items, so the common path is the plain store and one untaken branch.
struct Images {
    int mrow, cols;
    BSVD_HD bool any() const { return mrow >= 0 || cols; }
};
BSVD_HD Images images_of(int row, int x0, int n, int H, int W, int Hp, int Wp)
{
    Images im;
    im.mrow = mirror_of(row, H, Hp);
    const int lo = x0 > 2 * (W - 1) - Wp + 1 ? x0 : 2 * (W - 1) - Wp + 1, hi = x0 + n - 1 < W - 2 ? x0 + n - 1 : W - 2;
    im.cols = lo <= hi;                                               // columns (2 (W - 1) - Wp, W - 2] have an image in [W, Wp)
    return im;
}
BSVD_HD void put_own(float *at, int n, const float *v, int vec)
{
    if (n == 4 && vec) *reinterpret_cast<float4 *>(at) = make_float4(v[0], v[1], v[2], v[3]);
    else for (int q = 0; q < n; ++q) at[q] = v[q];
}
BSVD_HD void put_col_images(float *row, int x0, int n, const float *v, int W, int Wp)
{
    for (int q = 0; q < n; ++q) {
        const int m = mirror_of(x0 + q, W, Wp);
        if (m >= 0) row[m] = v[q];
    }
}
// plane: the element (0, 0) of the destination plane
BSVD_HD void put_images(float *plane, const Images &im, int row, int x0, int n, const float *v, int W, int Wp, int vec)
{
    if (im.cols) put_col_images(plane + (int64_t)row * Wp, x0, n, v, W, Wp);
    if (im.mrow >= 0) {
        put_own(plane + (int64_t)im.mrow * Wp + x0, n, v, vec);
        if (im.cols) put_col_images(plane + (int64_t)im.mrow * Wp, x0, n, v, W, Wp);
    }
}

// ---------------------------------------------------------------------------------------------
// uint8 <-> planar fp32 with pad / crop.  An item is 4 columns of one picture row, all channels: the 4 C bytes of 4 HWC pixels (one 12-byte
// group for C == 3) or 4 bytes per plane on the uint8 side, one float4 per plane on the fp32 side (vec: Wp % 4 == 0 and a 16-byte aligned
// tensor; otherwise, and in the last item of a row that W % 4 leaves short, scalars).
struct U8Geom { int C, cc, H, W, Hp, Wp, hwc, rev, vec; float const_val; };

BSVD_HD void u8_put(float *plane, const Images &im, const PadItem &it, const float *v, const U8Geom &g)
{
    put_own(plane + (int64_t)it.row * g.Wp + it.x0, it.n, v, g.vec);
    if (im.any()) put_images(plane, im, it.row, it.x0, it.n, v, g.W, g.Wp, g.vec);
}

BSVD_HD void u8_to_planar_pad_item(const uint8_t *src, float *dst, const U8Geom &g, int64_t i)
{
    const PadItem it = pad_item_of(i, g.H, g.W, 1);
    const int64_t plane = (int64_t)g.Hp * g.Wp, pic = (int64_t)g.H * g.W;
    const Images im = images_of(it.row, it.x0, it.n, g.H, g.W, g.Hp, g.Wp);
    float *d = dst + it.f * (g.C + g.cc) * plane;
    const int64_t pix = (int64_t)it.row * g.W + it.x0;
    if (g.hwc && g.C == 3 && it.n == 4) {
        uint8_t b[12];
        __builtin_memcpy(b, src + (it.f * pic + pix) * 3, 12);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v[4] = {(float)b[c] / 255.0f, (float)b[3 + c] / 255.0f, (float)b[6 + c] / 255.0f, (float)b[9 + c] / 255.0f};
            u8_put(d + c * plane, im, it, v, g);
        }
    } else {
        for (int c = 0; c < g.C; ++c) {
            uint8_t b[4] = {0, 0, 0, 0};
            if (g.hwc) {
                const uint8_t *s = src + (it.f * pic + pix) * g.C + c;
                for (int q = 0; q < it.n; ++q) b[q] = s[(int64_t)q * g.C];
            } else {
                const uint8_t *s = src + (it.f * g.C + c) * pic + pix;
                if (it.n == 4) __builtin_memcpy(b, s, 4);
                else for (int q = 0; q < it.n; ++q) b[q] = s[q];
            }
            const float v[4] = {(float)b[0] / 255.0f, (float)b[1] / 255.0f, (float)b[2] / 255.0f, (float)b[3] / 255.0f};
            u8_put(d + c * plane, im, it, v, g);
        }
    }
    const float k[4] = {g.const_val, g.const_val, g.const_val, g.const_val};
    for (int c = g.C; c < g.C + g.cc; ++c) u8_put(d + c * plane, im, it, k, g);
}

// the code of planar_to_u8_kernel: clamp to [0,1], x255, round half to even
BSVD_HD uint8_t u8_code(float v) { return (uint8_t)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

BSVD_HD void planar_to_u8_crop_item(const float *src, uint8_t *dst, const U8Geom &g, int64_t i)
{
    const PadItem it = pad_item_of(i, g.H, g.W, 1);
    const int64_t plane = (int64_t)g.Hp * g.Wp, pic = (int64_t)g.H * g.W;
    const float *s = src + it.f * g.C * plane + (int64_t)it.row * g.Wp + it.x0;
    const int64_t pix = (int64_t)it.row * g.W + it.x0;
    if (g.hwc && g.C == 3 && it.n == 4) {
        uint8_t b[12];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[4];
            if (g.vec) {
                const float4 x = *reinterpret_cast<const float4 *>(s + c * plane);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else {
                for (int q = 0; q < 4; ++q) v[q] = s[c * plane + q];
            }
            const int co = g.rev ? 2 - c : c;
#pragma unroll
            for (int q = 0; q < 4; ++q) b[3 * q + co] = u8_code(v[q]);
        }
        __builtin_memcpy(dst + (it.f * pic + pix) * 3, b, 12);
    } else {
        for (int c = 0; c < g.C; ++c) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (g.vec && it.n == 4) {
                const float4 x = *reinterpret_cast<const float4 *>(s + c * plane);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else {
                for (int q = 0; q < it.n; ++q) v[q] = s[c * plane + q];
            }
            const uint8_t b[4] = {u8_code(v[0]), u8_code(v[1]), u8_code(v[2]), u8_code(v[3])};
            const int co = g.rev ? g.C - 1 - c : c;
            if (g.hwc) {
                uint8_t *o = dst + (it.f * pic + pix) * g.C + co;
                for (int q = 0; q < it.n; ++q) o[(int64_t)q * g.C] = b[q];
            } else {
                uint8_t *o = dst + (it.f * g.C + co) * pic + pix;
                if (it.n == 4) __builtin_memcpy(o, b, 4);
                else for (int q = 0; q < it.n; ++q) o[q] = b[q];
            }
        }
    }
}

}  // namespace bsvd
