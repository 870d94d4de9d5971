// frame_items.h -- the frame I/O kernels' work on ONE item, as plain __host__ __device__ functions: the sample groups of frame_yuv.hip
// (load_codes / store_codes) and the item bodies of the pad / crop entry points (include/bsvd_hip.h: bsvd_u8_to_planar_pad,
// bsvd_planar_to_u8_crop, bsvd_yuv420_to_planar_pad, bsvd_planar_to_yuv420_crop).  The kernels are grid-stride loops around these bodies;
// a host program can run the same bodies over exact-size heap buffers under AddressSanitizer (tools/debug/frame_pad_bounds.hip), which
// sees the reads a GPU run cannot show: the tail of a half item, pitch padding, the bytes behind the last row of the last frame.
//
// Pad rule (one for all four): the picture is H x W, the network's tensor Hp x Wp with Hp >= H, Wp >= W, pad on the right and bottom only,
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

template <int PIX> struct Pix;
template <> struct Pix<BSVD_PIX_NV12> { using S = uint8_t;  static constexpr int SHIFT = 0; };
template <> struct Pix<BSVD_PIX_P010> { using S = uint16_t; static constexpr int SHIFT = 6; };   // 10-bit code in the high bits of the word

// N consecutive samples of a surface row.  A surface promises no more than its sample's own alignment (pitch and base are the caller's),
// hence the memcpy: one load / store of the group's width, legal at any sample-aligned address.
template <int PIX, int N>
BSVD_HD void load_codes(const uint8_t *p, float *out)
{
    typename Pix<PIX>::S v[N];
    __builtin_memcpy(v, __builtin_assume_aligned(p, sizeof(v[0])), sizeof(v));
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = (float)(v[k] >> Pix<PIX>::SHIFT);
}

// scaled values -> legal codes (clamp, round half to even like planar_to_u8_kernel) -> N samples in one store
template <int PIX, int N = 4>
BSVD_HD void store_codes(uint8_t *p, const float *val, float lo, float hi)
{
    typename Pix<PIX>::S v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (typename Pix<PIX>::S)((unsigned)rintf(fminf(fmaxf(val[k], lo), hi)) << Pix<PIX>::SHIFT);
    __builtin_memcpy(__builtin_assume_aligned(p, sizeof(v[0])), v, sizeof(v));
}

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

// ---------------------------------------------------------------------------------------------
// YUV 4:2:0 <-> planar fp32 with pad / crop.  The item of frame_yuv.hip, 4 columns x 2 rows with the one chroma row under them; W % 4 == 2
// leaves a HALF item at the right edge (2 luma samples per row, one CbCr pair), H / 2 may be odd.  Hp is even and Wp a multiple of 4, so
// every picture item owns float4-aligned positions of the planes.
struct YuvPadGeom { int H, W, Hp, Wp, cc; int64_t pitch, fstride; float const_val; };

// N = 4: a whole item; N = 2: the half item.  Straight-line in either: every load of the item is issued before the first is needed.
template <int PIX, int LINEAR, int N>
BSVD_HD void yuv420_to_planar_pad_body(const uint8_t *src, float *dst, const YuvPadGeom &g, const YuvDecode &k, const PadItem &it)
{
    constexpr int SB = (int)sizeof(typename Pix<PIX>::S);
    const int hh = g.H >> 1, j = it.row >> 1;
    const int64_t plane = (int64_t)g.Hp * g.Wp;
    const uint8_t *py = src + it.f * g.fstride + (int64_t)it.row * g.pitch + it.x0 * SB;
    const uint8_t *pc = src + it.f * g.fstride + (int64_t)g.H * g.pitch + it.x0 * SB;    // + row * pitch: the item's CbCr pairs of a chroma row
    float Y[2][4] = {}, cb[2][4], cr[2][4];
    load_codes<PIX, N>(py, Y[0]);
    load_codes<PIX, N>(py + g.pitch, Y[1]);
    if (!LINEAR) {
        float c[4];                                              // Cb0 Cr0 Cb1 Cr1
        load_codes<PIX, N>(pc + (int64_t)j * g.pitch, c);
        if (N == 2) { c[2] = c[0]; c[3] = c[1]; }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            cb[r][0] = cb[r][1] = c[0]; cb[r][2] = cb[r][3] = c[2];
            cr[r][0] = cr[r][1] = c[1]; cr[r][2] = cr[r][3] = c[3];
        }
    } else {
        // chroma sample (i, j) sits at luma (2i, 2j + 0.5): rows j - 1, j, j + 1 and the pair right of the item's, clamped at the PICTURE's edges
        const int rows[3] = {j > 0 ? j - 1 : 0, j, j + 1 < hh ? j + 1 : hh - 1};
        const int xn = (it.x0 + 4 < g.W ? it.x0 + 4 : g.W - 2) - it.x0;
        float a[3][6];                                           // Cb0 Cr0 Cb1 Cr1 Cb2 Cr2 of each row
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const uint8_t *p = pc + (int64_t)rows[r] * g.pitch;
            load_codes<PIX, N>(p, a[r]);
            if (N == 4) {
                load_codes<PIX, 2>(p + xn * SB, a[r] + 4);
            } else {                                             // the half item's one pair is the row's last: its right neighbour is itself
                a[r][2] = a[r][4] = a[r][0];
                a[r][3] = a[r][5] = a[r][1];
            }
        }
        // vertical first, then horizontal; dyadic weights on <= 10-bit integers: exact in fp32
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            float v[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) v[q] = r == 0 ? 0.25f * a[0][q] + 0.75f * a[1][q] : 0.75f * a[1][q] + 0.25f * a[2][q];
            cb[r][0] = v[0]; cb[r][1] = 0.5f * (v[0] + v[2]); cb[r][2] = v[2]; cb[r][3] = 0.5f * (v[2] + v[4]);
            cr[r][0] = v[1]; cr[r][1] = 0.5f * (v[1] + v[3]); cr[r][2] = v[3]; cr[r][3] = 0.5f * (v[3] + v[5]);
        }
    }
    float *d = dst + it.f * (3 + g.cc) * plane;
    const float kc[4] = {g.const_val, g.const_val, g.const_val, g.const_val};
    float rgb[2][3][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float y = (Y[r][q] - k.y_off) * k.y_mul;
            const float u = (cb[r][q] - k.c_off) * k.c_mul, v = (cr[r][q] - k.c_off) * k.c_mul;
            rgb[r][0][q] = fmaf(k.r_cr, v, y);
            rgb[r][1][q] = fmaf(-k.g_cb, u, fmaf(-k.g_cr, v, y));
            rgb[r][2][q] = fmaf(k.b_cb, u, y);
        }
        float *own = d + (int64_t)(it.row + r) * g.Wp + it.x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) put_own(own + c * plane, N, rgb[r][c], 1);
        for (int c = 0; c < g.cc; ++c) put_own(own + (3 + c) * plane, N, kc, 1);
    }
    // the images: only items at the right and bottom edge own any
    const Images im0 = images_of(it.row, it.x0, N, g.H, g.W, g.Hp, g.Wp), im1 = images_of(it.row + 1, it.x0, N, g.H, g.W, g.Hp, g.Wp);
    if (im0.any() || im1.any()) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const Images &im = r ? im1 : im0;
#pragma unroll
            for (int c = 0; c < 3; ++c) put_images(d + c * plane, im, it.row + r, it.x0, N, rgb[r][c], g.W, g.Wp, 1);
            for (int c = 0; c < g.cc; ++c) put_images(d + (3 + c) * plane, im, it.row + r, it.x0, N, kc, g.W, g.Wp, 1);
        }
    }
}

template <int PIX, int LINEAR>
BSVD_HD void yuv420_to_planar_pad_item(const uint8_t *src, float *dst, const YuvPadGeom &g, const YuvDecode &k, int64_t i)
{
    const PadItem it = pad_item_of(i, g.H >> 1, g.W, 2);
    if (it.n == 4) yuv420_to_planar_pad_body<PIX, LINEAR, 4>(src, dst, g, k, it);
    else yuv420_to_planar_pad_body<PIX, LINEAR, 2>(src, dst, g, k, it);
}

// src is the network's [frames][3][Hp][Wp]; only its picture rows and columns reach a sample.  A half item's float4 still lies inside its
// row of src (Wp is a multiple of 4 above W); the two pad values it carries end in no stored code.
template <int PIX, int LINEAR>
BSVD_HD void planar_to_yuv420_crop_item(const float *src, uint8_t *dst, const YuvPadGeom &g, const YuvEncode &k, int64_t i)
{
    constexpr int SB = (int)sizeof(typename Pix<PIX>::S);
    const PadItem it = pad_item_of(i, g.H >> 1, g.W, 2);
    const int64_t plane = (int64_t)g.Hp * g.Wp;
    const float *s = src + it.f * 3 * plane + (int64_t)it.row * g.Wp + it.x0;
    float yv[2][4], db[5] = {}, dr[5] = {};   // db / dr: mean over the two rows of B - Y', R - Y' at columns x0 - 1 (edge-clamped) .. x0 + 3
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float *row = s + (int64_t)r * g.Wp;
        const float4 R = *reinterpret_cast<const float4 *>(row);
        const float4 G = *reinterpret_cast<const float4 *>(row + plane);
        const float4 B = *reinterpret_cast<const float4 *>(row + 2 * plane);
        const float pr[4] = {R.x, R.y, R.z, R.w}, pg[4] = {G.x, G.y, G.z, G.w}, pb[4] = {B.x, B.y, B.z, B.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float cr_ = clamp01(pr[q]), cg = clamp01(pg[q]), cb_ = clamp01(pb[q]);
            const float y = fmaf(k.kb, cb_, fmaf(k.kg, cg, k.kr * cr_));
            yv[r][q] = fmaf(y, k.y_mul, k.y_off);
            db[q + 1] += 0.5f * (cb_ - y);
            dr[q + 1] += 0.5f * (cr_ - y);
        }
        if (LINEAR && it.x0 > 0) {                               // the column left of the item: tap 2i - 1 of its first chroma sample
            const float cr_ = clamp01(row[-1]), cg = clamp01(row[plane - 1]), cb_ = clamp01(row[2 * plane - 1]);
            const float y = fmaf(k.kb, cb_, fmaf(k.kg, cg, k.kr * cr_));
            db[0] += 0.5f * (cb_ - y);
            dr[0] += 0.5f * (cr_ - y);
        }
    }
    if (LINEAR && it.x0 == 0) { db[0] = db[1]; dr[0] = dr[1]; }   // ... clamped at the frame's left edge
    float c[4];                                                  // Cb0 Cr0 Cb1 Cr1
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        float mb, mr;
        if (LINEAR) {                                            // [1 2 1] / 4 over columns 2i - 1, 2i, 2i + 1: picture columns, all three
            mb = 0.25f * (db[2 * p] + db[2 * p + 2]) + 0.5f * db[2 * p + 1];
            mr = 0.25f * (dr[2 * p] + dr[2 * p + 2]) + 0.5f * dr[2 * p + 1];
        } else {                                                 // mean of the 2 x 2 block
            mb = 0.5f * (db[2 * p + 1] + db[2 * p + 2]);
            mr = 0.5f * (dr[2 * p + 1] + dr[2 * p + 2]);
        }
        c[2 * p] = fmaf(mb, k.cb_mul, k.c_off);
        c[2 * p + 1] = fmaf(mr, k.cr_mul, k.c_off);
    }
    uint8_t *py = dst + it.f * g.fstride + (int64_t)it.row * g.pitch + it.x0 * SB;
    uint8_t *pc = dst + it.f * g.fstride + (int64_t)(g.H + (it.row >> 1)) * g.pitch + it.x0 * SB;
    if (it.n == 4) {
        store_codes<PIX, 4>(py, yv[0], k.y_lo, k.y_hi);
        store_codes<PIX, 4>(py + g.pitch, yv[1], k.y_lo, k.y_hi);
        store_codes<PIX, 4>(pc, c, k.c_lo, k.c_hi);
    } else {
        store_codes<PIX, 2>(py, yv[0], k.y_lo, k.y_hi);
        store_codes<PIX, 2>(py + g.pitch, yv[1], k.y_lo, k.y_hi);
        store_codes<PIX, 2>(pc, c, k.c_lo, k.c_hi);
    }
}

}  // namespace bsvd
