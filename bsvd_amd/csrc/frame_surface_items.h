// frame_surface_items.h -- the item bodies of the YUV entry points (include/bsvd_hip.h: bsvd_yuv420_to_planar, bsvd_planar_to_yuv420,
// bsvd_yuv_to_planar, bsvd_planar_to_yuv and their _pad / _crop forms), as plain __host__ __device__ functions like those of
// frame_items.h: the kernels of frame_yuv.hip are grid-stride loops around them, and tools/debug/yuv_surface_bounds.hip runs the same
// bodies over exact-size heap buffers under AddressSanitizer.
//
// A surface format is three compile-time facts: the subsampling (4:2:0, 4:2:2, 4:4:4), the layout (three planes; Y + interleaved CbCr;
// packed Cb Y0 Cr Y1; packed Y0 Cb Y1 Cr) and the sample rule (8 bit; 10 bit in the high bits of a 16-bit word; 10 bit in the low bits).
// Both kernels are bandwidth-bound and the fp32 side carries 8 to 16 times the bytes of the YUV side, so the fp32 side decides the layout
// of work over lanes: an ITEM is 4 columns of one picture row (4:2:2, 4:4:4) or of a row
// pair with the one chroma row under it (4:2:0), consecutive lanes take consecutive items of a row, a lane moves one float4 per plane row.
// On the surface side the item's samples are one group per plane and row -- 4 Y, 2 (or 4) Cb, 2 (or 4) Cr, or the 8 bytes of two packed
// pixel pairs -- each read or written once, as a whole, by this lane alone.  A row that W % 4 leaves short ends in a part item of 2 columns
// (W is even with subsampled chroma) or of 1..3 (4:4:4), which moves as groups of 2 and 1.
#pragma once
#include "frame_items.h"
#include "frame_finish_items.h"

namespace bsvd {

enum { SMP_U8 = 0, SMP_HIGH10 = 1, SMP_LOW10 = 2 };
template <int SMP> struct Smp;
template <> struct Smp<SMP_U8>     { using S = uint8_t;  static constexpr int SHIFT = 0; static constexpr unsigned MASK = 0xffu; };
template <> struct Smp<SMP_HIGH10> { using S = uint16_t; static constexpr int SHIFT = 6; static constexpr unsigned MASK = 0x3ffu; };   // P010 rule
template <> struct Smp<SMP_LOW10>  { using S = uint16_t; static constexpr int SHIFT = 0; static constexpr unsigned MASK = 0x3ffu; };   // yuv4xxp10le rule: high 6 bits ignored in, zero out

template <int SUB_, int LAY_, int SMP_> struct SurfFmt {
    static constexpr int SUB = SUB_, LAY = LAY_, SMP = SMP_;
    static constexpr int ROWS = SUB_ == BSVD_SUB_420 ? 2 : 1;                                      // picture rows of an item
    static constexpr bool PACKED = LAY_ == BSVD_LAYOUT_UYVY || LAY_ == BSVD_LAYOUT_YUYV;
    using S = typename Smp<SMP_>::S;
    static constexpr int SB = (int)sizeof(S);
};

// planes: 0 = Y (or the packed plane), 1 = Cb or CbCr, 2 = Cr.  off / pitch in bytes, resolved by the host (no zeros left).
struct SurfGeom { int H, W, Hp, Wp, cc; float const_val; int64_t fstride, off[3], pitch[3]; };

// N consecutive samples of a row, with the sample rule of the format.  A surface promises no more than its sample's own alignment (pitch
// and base are the caller's), hence the memcpy: one load / store of the group's width, legal at any sample-aligned address.
template <int SMP, int N>
BSVD_HD void load_smp(const uint8_t *p, float *out)
{
    typename Smp<SMP>::S v[N];
    __builtin_memcpy(v, __builtin_assume_aligned(p, sizeof(v[0])), sizeof(v));
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = (float)(((unsigned)v[k] >> Smp<SMP>::SHIFT) & Smp<SMP>::MASK);
}
BSVD_HD unsigned legal_code(float v, float lo, float hi) { return (unsigned)rintf(fminf(fmaxf(v, lo), hi)); }
template <int SMP, int N>
BSVD_HD void store_smp(uint8_t *p, const float *val, float lo, float hi)
{
    typename Smp<SMP>::S v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (typename Smp<SMP>::S)(legal_code(val[k], lo, hi) << Smp<SMP>::SHIFT);
    __builtin_memcpy(__builtin_assume_aligned(p, sizeof(v[0])), v, sizeof(v));
}

// N luma samples of picture row `row` from column x0 (packed: N even, x0 even -- whole pixel pairs)
template <class F, int N>
BSVD_HD void load_luma(const uint8_t *fr, const SurfGeom &g, int row, int x0, float *Y)
{
    if constexpr (F::PACKED) {
        float b[2 * N];
        load_smp<F::SMP, 2 * N>(fr + g.off[0] + (int64_t)row * g.pitch[0] + x0 * 2, b);
#pragma unroll
        for (int q = 0; q < N; ++q) Y[q] = b[2 * q + (F::LAY == BSVD_LAYOUT_UYVY ? 1 : 0)];
    } else {
        load_smp<F::SMP, N>(fr + g.off[0] + (int64_t)row * g.pitch[0] + x0 * F::SB, Y);
    }
}

// NC chroma samples (Cb and Cr) of chroma row `crow` from chroma column ci
template <class F, int NC>
BSVD_HD void load_chroma(const uint8_t *fr, const SurfGeom &g, int crow, int ci, float *cb, float *cr)
{
    if constexpr (F::PACKED) {                                   // Cb Y Cr Y | Y Cb Y Cr: one 4-byte group per chroma sample
        float b[4 * NC];
        load_smp<F::SMP, 4 * NC>(fr + g.off[0] + (int64_t)crow * g.pitch[0] + ci * 4, b);
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            cb[q] = b[4 * q + (F::LAY == BSVD_LAYOUT_UYVY ? 0 : 1)];
            cr[q] = b[4 * q + (F::LAY == BSVD_LAYOUT_UYVY ? 2 : 3)];
        }
    } else if constexpr (F::LAY == BSVD_LAYOUT_SEMIPLANAR) {
        float b[2 * NC];
        load_smp<F::SMP, 2 * NC>(fr + g.off[1] + (int64_t)crow * g.pitch[1] + ci * 2 * F::SB, b);
#pragma unroll
        for (int q = 0; q < NC; ++q) { cb[q] = b[2 * q]; cr[q] = b[2 * q + 1]; }
    } else {
        load_smp<F::SMP, NC>(fr + g.off[1] + (int64_t)crow * g.pitch[1] + ci * F::SB, cb);
        load_smp<F::SMP, NC>(fr + g.off[2] + (int64_t)crow * g.pitch[2] + ci * F::SB, cr);
    }
}

// the stores of the planar and semi-planar layouts: N luma values / NC chroma pairs, scaled but neither clamped nor rounded yet
template <class F, int N>
BSVD_HD void store_luma(uint8_t *fr, const SurfGeom &g, const YuvEncode &k, int row, int x0, const float *yv)
{
    store_smp<F::SMP, N>(fr + g.off[0] + (int64_t)row * g.pitch[0] + x0 * F::SB, yv, k.y_lo, k.y_hi);
}
template <class F, int NC>
BSVD_HD void store_chroma(uint8_t *fr, const SurfGeom &g, const YuvEncode &k, int crow, int ci, const float *cb, const float *cr)
{
    if constexpr (F::LAY == BSVD_LAYOUT_SEMIPLANAR) {
        float b[2 * NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) { b[2 * q] = cb[q]; b[2 * q + 1] = cr[q]; }
        store_smp<F::SMP, 2 * NC>(fr + g.off[1] + (int64_t)crow * g.pitch[1] + ci * 2 * F::SB, b, k.c_lo, k.c_hi);
    } else {
        store_smp<F::SMP, NC>(fr + g.off[1] + (int64_t)crow * g.pitch[1] + ci * F::SB, cb, k.c_lo, k.c_hi);
        store_smp<F::SMP, NC>(fr + g.off[2] + (int64_t)crow * g.pitch[2] + ci * F::SB, cr, k.c_lo, k.c_hi);
    }
}
// ... and of the packed ones: N / 2 pixel pairs, 2 N bytes, one store
template <class F, int N>
BSVD_HD void store_packed(uint8_t *fr, const SurfGeom &g, const YuvEncode &k, int row, int x0, const float *yv, const float *cb, const float *cr)
{
    uint8_t b[2 * N];
    constexpr int YO = F::LAY == BSVD_LAYOUT_UYVY ? 1 : 0, CO = 1 - YO;
#pragma unroll
    for (int q = 0; q < N; ++q) b[2 * q + YO] = (uint8_t)legal_code(yv[q], k.y_lo, k.y_hi);
#pragma unroll
    for (int p = 0; p < N / 2; ++p) {
        b[4 * p + CO] = (uint8_t)legal_code(cb[p], k.c_lo, k.c_hi);
        b[4 * p + CO + 2] = (uint8_t)legal_code(cr[p], k.c_lo, k.c_hi);
    }
    __builtin_memcpy(fr + g.off[0] + (int64_t)row * g.pitch[0] + x0 * 2, b, sizeof(b));
}

// ---------------------------------------------------------------------------------------------
// decode.  N picture columns from (it.row, x0): 4 = a whole item, 2 / 1 = the groups of a part item (1 with 4:4:4 only).  Chroma filters
// clamp at the PICTURE's edges; the mirror images of the pad region are copies of the converted values (frame_items.h, put_images).
// 4:2:0: vertical filter, then horizontal.  4:2:2: the horizontal half.  4:4:4: none.
template <class F, int LINEAR, int N>
BSVD_HD void yuv_to_planar_body(const uint8_t *src, float *dst, const SurfGeom &g, const YuvDecode &k, int64_t f, int row, int x0)
{
    constexpr int R = F::ROWS;
    const int64_t plane = (int64_t)g.Hp * g.Wp;
    const uint8_t *fr = src + f * g.fstride;
    float Y[R][4] = {}, cb[R][4] = {}, cr[R][4] = {};
#pragma unroll
    for (int r = 0; r < R; ++r) load_luma<F, N>(fr, g, row + r, x0, Y[r]);
    if constexpr (F::SUB == BSVD_SUB_444) {
        load_chroma<F, N>(fr, g, row, x0, cb[0], cr[0]);
    } else {
        constexpr int NC = N / 2;
        const int ci = x0 >> 1, cw = g.W >> 1;
        const int crow = F::SUB == BSVD_SUB_420 ? row >> 1 : row;
        if (!LINEAR) {
            float b[NC], c[NC];
            load_chroma<F, NC>(fr, g, crow, ci, b, c);
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int p = 0; p < NC; ++p) {
                    cb[r][2 * p] = cb[r][2 * p + 1] = b[p];
                    cr[r][2 * p] = cr[r][2 * p + 1] = c[p];
                }
        } else {
            // the item's NC samples and the one right of them, clamped at the picture's edge (a part item's last sample is the row's last)
            const int cn = ci + NC < cw ? ci + NC : cw - 1;
            float vb[R][NC + 1], vr[R][NC + 1];
            if constexpr (F::SUB == BSVD_SUB_420) {
                // chroma sample (i, j) sits at luma (2i, 2j + 0.5): rows j - 1, j, j + 1, clamped; vertical first, then horizontal; dyadic
                // weights on <= 10-bit integers: exact in fp32
                const int hh = g.H >> 1;
                const int rows[3] = {crow > 0 ? crow - 1 : 0, crow, crow + 1 < hh ? crow + 1 : hh - 1};
                float ab[3][NC + 1], ar[3][NC + 1];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    load_chroma<F, NC>(fr, g, rows[r], ci, ab[r], ar[r]);
                    load_chroma<F, 1>(fr, g, rows[r], cn, ab[r] + NC, ar[r] + NC);
                }
#pragma unroll
                for (int q = 0; q <= NC; ++q) {
                    vb[0][q] = 0.25f * ab[0][q] + 0.75f * ab[1][q]; vb[1][q] = 0.75f * ab[1][q] + 0.25f * ab[2][q];
                    vr[0][q] = 0.25f * ar[0][q] + 0.75f * ar[1][q]; vr[1][q] = 0.75f * ar[1][q] + 0.25f * ar[2][q];
                }
            } else {
                load_chroma<F, NC>(fr, g, crow, ci, vb[0], vr[0]);
                load_chroma<F, 1>(fr, g, crow, cn, vb[0] + NC, vr[0] + NC);
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int p = 0; p < NC; ++p) {
                    cb[r][2 * p] = vb[r][p]; cb[r][2 * p + 1] = 0.5f * (vb[r][p] + vb[r][p + 1]);
                    cr[r][2 * p] = vr[r][p]; cr[r][2 * p + 1] = 0.5f * (vr[r][p] + vr[r][p + 1]);
                }
        }
    }
    float *d = dst + f * (3 + g.cc) * plane;
    const float kc[4] = {g.const_val, g.const_val, g.const_val, g.const_val};
    float rgb[R][3][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float y = (Y[r][q] - k.y_off) * k.y_mul;
            const float u = (cb[r][q] - k.c_off) * k.c_mul, v = (cr[r][q] - k.c_off) * k.c_mul;
            rgb[r][0][q] = fmaf(k.r_cr, v, y);
            rgb[r][1][q] = fmaf(-k.g_cb, u, fmaf(-k.g_cr, v, y));
            rgb[r][2][q] = fmaf(k.b_cb, u, y);
        }
        float *own = d + (int64_t)(row + r) * g.Wp + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) put_own(own + c * plane, N, rgb[r][c], 1);
        for (int c = 0; c < g.cc; ++c) put_own(own + (3 + c) * plane, N, kc, 1);
    }
    // the images: only items at the right and bottom edge own any
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const Images im = images_of(row + r, x0, N, g.H, g.W, g.Hp, g.Wp);
        if (im.any()) {
#pragma unroll
            for (int c = 0; c < 3; ++c) put_images(d + c * plane, im, row + r, x0, N, rgb[r][c], g.W, g.Wp, 1);
            for (int c = 0; c < g.cc; ++c) put_images(d + (3 + c) * plane, im, row + r, x0, N, kc, g.W, g.Wp, 1);
        }
    }
}

template <class F> BSVD_HD int surf_item_rows(int H) { return F::ROWS == 2 ? H >> 1 : H; }

template <class F, int LINEAR>
BSVD_HD void yuv_to_planar_item(const uint8_t *src, float *dst, const SurfGeom &g, const YuvDecode &k, int64_t i)
{
    const PadItem it = pad_item_of(i, surf_item_rows<F>(g.H), g.W, F::ROWS);
    if (it.n == 4) { yuv_to_planar_body<F, LINEAR, 4>(src, dst, g, k, it.f, it.row, it.x0); return; }
    if (it.n >= 2) yuv_to_planar_body<F, LINEAR, 2>(src, dst, g, k, it.f, it.row, it.x0);
    if constexpr (F::SUB == BSVD_SUB_444) {
        if (it.n & 1) yuv_to_planar_body<F, LINEAR, 1>(src, dst, g, k, it.f, it.row, it.x0 + (it.n & 2));
    }
}

// ---------------------------------------------------------------------------------------------
// encode.  src is the network's [frames][3][Hp][Wp]; only its picture rows and columns reach a sample.  A part item's float4 still lies
// inside its row of src (Wp is a multiple of 4 at or above W); the pad values it carries end in no stored code.  4:2:0: chroma from the
// mean over the item's two rows.  4:2:2: the same without that mean.  4:4:4: Cb and Cr of every pixel.
// Dither (frame_finish_items.h): d joins a scaled value right before the store's clamp and rintf -- rint(clamp(t + d, lo, hi)) --, luma and
// 4:4:4 chroma on the picture's grid, subsampled chroma on the chroma grid; with di.mode == BSVD_DITHER_NONE no value is touched.
template <class F, int LINEAR>
BSVD_HD void planar_to_yuv_item(const float *src, uint8_t *dst, const SurfGeom &g, const YuvEncode &k, const Dither &di, int64_t i)
{
    constexpr int R = F::ROWS;
    constexpr float WGT = R == 2 ? 0.5f : 1.0f;
    const PadItem it = pad_item_of(i, surf_item_rows<F>(g.H), g.W, R);
    const int64_t plane = (int64_t)g.Hp * g.Wp;
    const float *s = src + it.f * 3 * plane + (int64_t)it.row * g.Wp + it.x0;
    float yv[R][4], db[5] = {}, dr[5] = {};   // db / dr: (mean over the item's rows of) B - Y', R - Y' at columns x0 - 1 (edge-clamped) .. x0 + 3
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float *row = s + (int64_t)r * g.Wp;
        const float4 Rv = *reinterpret_cast<const float4 *>(row);
        const float4 Gv = *reinterpret_cast<const float4 *>(row + plane);
        const float4 Bv = *reinterpret_cast<const float4 *>(row + 2 * plane);
        const float pr[4] = {Rv.x, Rv.y, Rv.z, Rv.w}, pg[4] = {Gv.x, Gv.y, Gv.z, Gv.w}, pb[4] = {Bv.x, Bv.y, Bv.z, Bv.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float cr_ = clamp01(pr[q]), cg = clamp01(pg[q]), cb_ = clamp01(pb[q]);
            const float y = fmaf(k.kb, cb_, fmaf(k.kg, cg, k.kr * cr_));
            yv[r][q] = fmaf(y, k.y_mul, k.y_off);
            db[q + 1] += WGT * (cb_ - y);
            dr[q + 1] += WGT * (cr_ - y);
        }
        if (LINEAR && F::SUB != BSVD_SUB_444 && it.x0 > 0) {     // the column left of the item: tap 2i - 1 of its first chroma sample
            const float cr_ = clamp01(row[-1]), cg = clamp01(row[plane - 1]), cb_ = clamp01(row[2 * plane - 1]);
            const float y = fmaf(k.kb, cb_, fmaf(k.kg, cg, k.kr * cr_));
            db[0] += WGT * (cb_ - y);
            dr[0] += WGT * (cr_ - y);
        }
    }
    uint8_t *fr = dst + it.f * g.fstride;
    if (di.mode != BSVD_DITHER_NONE) {
#pragma unroll
        for (int r = 0; r < R; ++r) dither_add<4>(di, it.f, 0, it.row + r, it.x0, yv[r]);
    }
    if constexpr (F::SUB == BSVD_SUB_444) {
        float cb[4], cr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { cb[q] = fmaf(db[q + 1], k.cb_mul, k.c_off); cr[q] = fmaf(dr[q + 1], k.cr_mul, k.c_off); }
        if (di.mode != BSVD_DITHER_NONE) {
            dither_add<4>(di, it.f, 1, it.row, it.x0, cb);
            dither_add<4>(di, it.f, 2, it.row, it.x0, cr);
        }
        if (it.n == 4) {
            store_luma<F, 4>(fr, g, k, it.row, it.x0, yv[0]);
            store_chroma<F, 4>(fr, g, k, it.row, it.x0, cb, cr);
        } else {
            const int h = it.n & 2;
            if (h) { store_luma<F, 2>(fr, g, k, it.row, it.x0, yv[0]); store_chroma<F, 2>(fr, g, k, it.row, it.x0, cb, cr); }
            if (it.n & 1) { store_luma<F, 1>(fr, g, k, it.row, it.x0 + h, yv[0] + h); store_chroma<F, 1>(fr, g, k, it.row, it.x0 + h, cb + h, cr + h); }
        }
    } else {
        if (LINEAR && it.x0 == 0) { db[0] = db[1]; dr[0] = dr[1]; }   // ... clamped at the picture's left edge
        float cb[2], cr[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float mb, mr;
            if (LINEAR) {                                            // [1 2 1] / 4 over columns 2i - 1, 2i, 2i + 1: picture columns, all three
                mb = 0.25f * (db[2 * p] + db[2 * p + 2]) + 0.5f * db[2 * p + 1];
                mr = 0.25f * (dr[2 * p] + dr[2 * p + 2]) + 0.5f * dr[2 * p + 1];
            } else {                                                 // mean of the two columns (of the 2 x 2 block with 4:2:0)
                mb = 0.5f * (db[2 * p + 1] + db[2 * p + 2]);
                mr = 0.5f * (dr[2 * p + 1] + dr[2 * p + 2]);
            }
            cb[p] = fmaf(mb, k.cb_mul, k.c_off);
            cr[p] = fmaf(mr, k.cr_mul, k.c_off);
        }
        const int ci = it.x0 >> 1, crow = F::SUB == BSVD_SUB_420 ? it.row >> 1 : it.row;
        if (di.mode != BSVD_DITHER_NONE) {
            dither_add<2>(di, it.f, 1, crow, ci, cb);
            dither_add<2>(di, it.f, 2, crow, ci, cr);
        }
        if constexpr (F::PACKED) {
            if (it.n == 4) store_packed<F, 4>(fr, g, k, it.row, it.x0, yv[0], cb, cr);
            else store_packed<F, 2>(fr, g, k, it.row, it.x0, yv[0], cb, cr);
        } else if (it.n == 4) {
#pragma unroll
            for (int r = 0; r < R; ++r) store_luma<F, 4>(fr, g, k, it.row + r, it.x0, yv[r]);
            store_chroma<F, 2>(fr, g, k, crow, ci, cb, cr);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) store_luma<F, 2>(fr, g, k, it.row + r, it.x0, yv[r]);
            store_chroma<F, 1>(fr, g, k, crow, ci, cb, cr);
        }
    }
}

// dither off: the body as its callers of before the finish stage name it
template <class F, int LINEAR>
BSVD_HD void planar_to_yuv_item(const float *src, uint8_t *dst, const SurfGeom &g, const YuvEncode &k, int64_t i)
{
    planar_to_yuv_item<F, LINEAR>(src, dst, g, k, Dither{BSVD_DITHER_NONE, 0u, 0}, i);
}

}  // namespace bsvd
