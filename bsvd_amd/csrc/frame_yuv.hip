// frame_yuv.hip -- YUV 4:2:0 frame I/O on the device (include/bsvd_hip.h, bsvd_yuv420_to_planar / bsvd_planar_to_yuv420): NV12 and P010
// surfaces, as decoders, capture cards and encoders hand them over, <-> the planar fp32 tensors of the network.  The YUV counterpart of
// u8_to_planar_kernel / planar_to_u8_kernel (tensor_layout.hip): helper kernels on the caller's stream, outside the captured graphs.
//
// Both kernels are bandwidth-bound and the fp32 side carries 8 to 16 times the bytes of the YUV side, so the fp32 side decides the layout
// of work over lanes: one ITEM is 4 columns x 2 rows of one frame, consecutive lanes take consecutive items of a row pair -- a lane moves one
// float4 per plane row, a wave whole contiguous runs of a plane row -- and the one chroma row under the two luma rows serves both.  On
// the YUV side an item is one group of 4 Y samples per row and the 2 CbCr pairs under them (4 + 4 + 4 bytes with NV12, 8 + 8 + 8 with
// P010), each read or written once, as a whole, by this lane alone.
#include "bsvd_internal.h"
#include "frame_items.h"      // Pix, load_codes / store_codes, YuvDecode / YuvEncode; the item bodies of the pad / crop kernels

namespace bsvd {

// item index -> frame, chroma row j (luma rows 2j, 2j + 1), first column x0.  Items of one frame fit 32 bits (checked by the host).
struct Item { int64_t f; int j, x0; };
__device__ __forceinline__ Item item_of(int64_t i, int64_t per_frame, int wq)
{
    Item it;
    it.f = i / per_frame;
    const int r = (int)(i - it.f * per_frame);
    it.j = r / wq;
    it.x0 = (r - it.j * wq) * 4;
    return it;
}

// ---------------------------------------------------------------------------------------------
template <int PIX, int LINEAR>
__global__ __launch_bounds__(256) void yuv420_to_planar_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, int H, int W, int64_t pitch,
                                                               int64_t fstride, int cc, float const_val, YuvDecode k, int64_t items)
{
    constexpr int SB = (int)sizeof(typename Pix<PIX>::S);
    const int wq = W >> 2, hh = H >> 1;
    const int64_t per_frame = (int64_t)wq * hh, plane = (int64_t)H * W;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const Item it = item_of(i, per_frame, wq);
        const uint8_t *py = src + it.f * fstride + (int64_t)(2 * it.j) * pitch + it.x0 * SB;
        const uint8_t *pc = src + it.f * fstride + (int64_t)H * pitch + it.x0 * SB;      // + row * pitch: the item's two CbCr pairs of a chroma row
        float Y[2][4], cb[2][4], cr[2][4];
        load_codes<PIX, 4>(py, Y[0]);
        load_codes<PIX, 4>(py + pitch, Y[1]);
        if (!LINEAR) {
            float c[4];                                              // Cb0 Cr0 Cb1 Cr1
            load_codes<PIX, 4>(pc + (int64_t)it.j * pitch, c);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                cb[r][0] = cb[r][1] = c[0]; cb[r][2] = cb[r][3] = c[2];
                cr[r][0] = cr[r][1] = c[1]; cr[r][2] = cr[r][3] = c[3];
            }
        } else {
            // chroma sample (i, j) sits at luma (2i, 2j + 0.5): rows j - 1, j, j + 1 and the pair right of the item's two, clamped at the edges
            const int rows[3] = {it.j > 0 ? it.j - 1 : 0, it.j, it.j + 1 < hh ? it.j + 1 : hh - 1};
            const int xn = (it.x0 + 4 < W ? it.x0 + 4 : W - 2) - it.x0;
            float a[3][6];                                           // Cb0 Cr0 Cb1 Cr1 Cb2 Cr2 of each row
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                load_codes<PIX, 4>(pc + (int64_t)rows[r] * pitch, a[r]);
                load_codes<PIX, 2>(pc + (int64_t)rows[r] * pitch + xn * SB, a[r] + 4);
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
        float *d = dst + it.f * (3 + cc) * plane + (int64_t)(2 * it.j) * W + it.x0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            float4 R, G, B;
            float *pr = &R.x, *pg = &G.x, *pb = &B.x;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float y = (Y[r][q] - k.y_off) * k.y_mul;
                const float u = (cb[r][q] - k.c_off) * k.c_mul, v = (cr[r][q] - k.c_off) * k.c_mul;
                pr[q] = fmaf(k.r_cr, v, y);
                pg[q] = fmaf(-k.g_cb, u, fmaf(-k.g_cr, v, y));
                pb[q] = fmaf(k.b_cb, u, y);
            }
            float *row = d + (int64_t)r * W;
            *reinterpret_cast<float4 *>(row) = R;
            *reinterpret_cast<float4 *>(row + plane) = G;
            *reinterpret_cast<float4 *>(row + 2 * plane) = B;
            for (int c = 0; c < cc; ++c) *reinterpret_cast<float4 *>(row + (3 + c) * plane) = make_float4(const_val, const_val, const_val, const_val);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// encode (YuvEncode, frame_items.h)
template <int PIX, int LINEAR>
__global__ __launch_bounds__(256) void planar_to_yuv420_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, int H, int W, int64_t pitch,
                                                               int64_t fstride, YuvEncode k, int64_t items)
{
    constexpr int SB = (int)sizeof(typename Pix<PIX>::S);
    const int wq = W >> 2, hh = H >> 1;
    const int64_t per_frame = (int64_t)wq * hh, plane = (int64_t)H * W;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const Item it = item_of(i, per_frame, wq);
        const float *s = src + it.f * 3 * plane + (int64_t)(2 * it.j) * W + it.x0;
        float yv[2][4], db[5] = {}, dr[5] = {};   // db / dr: mean over the two rows of B - Y', R - Y' at columns x0 - 1 (edge-clamped) .. x0 + 3
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const float *row = s + (int64_t)r * W;
            const float4 R = *reinterpret_cast<const float4 *>(row);
            const float4 G = *reinterpret_cast<const float4 *>(row + plane);
            const float4 B = *reinterpret_cast<const float4 *>(row + 2 * plane);
            const float *pr = &R.x, *pg = &G.x, *pb = &B.x;
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
            if (LINEAR) {                                            // [1 2 1] / 4 over columns 2i - 1, 2i, 2i + 1
                mb = 0.25f * (db[2 * p] + db[2 * p + 2]) + 0.5f * db[2 * p + 1];
                mr = 0.25f * (dr[2 * p] + dr[2 * p + 2]) + 0.5f * dr[2 * p + 1];
            } else {                                                 // mean of the 2 x 2 block
                mb = 0.5f * (db[2 * p + 1] + db[2 * p + 2]);
                mr = 0.5f * (dr[2 * p + 1] + dr[2 * p + 2]);
            }
            c[2 * p] = fmaf(mb, k.cb_mul, k.c_off);
            c[2 * p + 1] = fmaf(mr, k.cr_mul, k.c_off);
        }
        uint8_t *py = dst + it.f * fstride + (int64_t)(2 * it.j) * pitch + it.x0 * SB;
        store_codes<PIX>(py, yv[0], k.y_lo, k.y_hi);
        store_codes<PIX>(py + pitch, yv[1], k.y_lo, k.y_hi);
        store_codes<PIX>(dst + it.f * fstride + (int64_t)(H + it.j) * pitch + it.x0 * SB, c, k.c_lo, k.c_hi);
    }
}

// ---------------------------------------------------------------------------------------------
// pad / crop (bsvd_yuv420_to_planar_pad / bsvd_planar_to_yuv420_crop): the same work shape over the PICTURE's items; the bodies, with the
// half item of W % 4 == 2 and the mirror images of the pad region, are in frame_items.h
template <int PIX, int LINEAR>
__global__ __launch_bounds__(256) void yuv420_to_planar_pad_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, YuvPadGeom g, YuvDecode k, int64_t items)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x)
        yuv420_to_planar_pad_item<PIX, LINEAR>(src, dst, g, k, i);
}

template <int PIX, int LINEAR>
__global__ __launch_bounds__(256) void planar_to_yuv420_crop_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, YuvPadGeom g, YuvEncode k, int64_t items)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x)
        planar_to_yuv420_crop_item<PIX, LINEAR>(src, dst, g, k, i);
}

// ---------------------------------------------------------------------------------------------
// host side: validation (no device needed), constants in double, dispatch
static const double kMatrix[3][2] = {{0.299, 0.114}, {0.2126, 0.0722}, {0.2627, 0.0593}};   // (Kr, Kb): BT.601, BT.709, BT.2020 ncl

struct YuvGeom { int64_t pitch, fstride, items; };

static inline int sample_bytes(int pix_fmt) { return pix_fmt == BSVD_PIX_P010 ? 2 : 1; }

// H x W is the surface's picture.  pad == 0: the plain entry points, H and W multiples of 4.  pad != 0: the pad / crop entry points, H and W
// even, the planar tensor Hp x Wp.
static int yuv_check(const char *fn, const void *yuv, const char *yuv_name, const float *planar, const char *planar_name, int32_t frames, int32_t H,
                     int32_t W, const BsvdYuvDesc *d, YuvGeom *g, int pad = 0, int32_t Hp = 0, int32_t Wp = 0)
{
    if (!yuv) { set_error("%s: %s is NULL", fn, yuv_name); return -3; }
    if (!planar) { set_error("%s: %s is NULL", fn, planar_name); return -3; }
    if (!d) { set_error("%s: desc is NULL", fn); return -3; }
    if (frames <= 0) { set_error("%s: frames = %d must be positive", fn, frames); return -3; }
    if (!pad) {
        if (H <= 0 || (H & 3)) { set_error("%s: H = %d must be a positive multiple of 4", fn, H); return -3; }
        if (W <= 0 || (W & 3)) { set_error("%s: W = %d must be a positive multiple of 4", fn, W); return -3; }
    } else {
        if (H <= 0 || (H & 1)) { set_error("%s: H = %d must be positive and even (4:2:0)", fn, H); return -3; }
        if (W <= 0 || (W & 1)) { set_error("%s: W = %d must be positive and even (4:2:0)", fn, W); return -3; }
        if (Hp < H) { set_error("%s: Hp = %d is below H = %d", fn, Hp, H); return -3; }
        if (Wp < W) { set_error("%s: Wp = %d is below W = %d", fn, Wp, W); return -3; }
        if (Hp - H >= H) { set_error("%s: Hp = %d pads H = %d by a whole dimension or more (reflect is defined up to 2 H - 1)", fn, Hp, H); return -3; }
        if (Wp - W >= W) { set_error("%s: Wp = %d pads W = %d by a whole dimension or more (reflect is defined up to 2 W - 1)", fn, Wp, W); return -3; }
        if (Hp & 1) { set_error("%s: Hp = %d must be even", fn, Hp); return -3; }
        if (Wp & 3) { set_error("%s: Wp = %d must be a multiple of 4 (rows move as float4)", fn, Wp); return -3; }
    }
    if (d->pix_fmt != BSVD_PIX_NV12 && d->pix_fmt != BSVD_PIX_P010) { set_error("%s: desc->pix_fmt = %d (BSVD_PIX_NV12, BSVD_PIX_P010)", fn, d->pix_fmt); return -3; }
    if (d->matrix < BSVD_MATRIX_BT601 || d->matrix > BSVD_MATRIX_BT2020) { set_error("%s: desc->matrix = %d (BSVD_MATRIX_BT601 .. BT2020)", fn, d->matrix); return -3; }
    if (d->full_range != 0 && d->full_range != 1) { set_error("%s: desc->full_range = %d (0 or 1)", fn, d->full_range); return -3; }
    if (d->chroma != BSVD_CHROMA_NEAREST && d->chroma != BSVD_CHROMA_LINEAR) { set_error("%s: desc->chroma = %d (BSVD_CHROMA_NEAREST, BSVD_CHROMA_LINEAR)", fn, d->chroma); return -3; }
    if (d->reserved != 0) { set_error("%s: desc->reserved = %d must be 0", fn, d->reserved); return -3; }
    const int sb = sample_bytes(d->pix_fmt);
    const int64_t tight = (int64_t)W * sb;
    g->pitch = d->row_pitch ? d->row_pitch : tight;
    if (g->pitch < tight) { set_error("%s: desc->row_pitch = %d bytes is below W = %d samples (%lld bytes)", fn, d->row_pitch, W, (long long)tight); return -3; }
    const int64_t frame = g->pitch * H / 2 * 3;
    g->fstride = d->frame_stride ? d->frame_stride : frame;
    if (g->fstride < frame) { set_error("%s: desc->frame_stride = %lld bytes is below one frame (%lld bytes)", fn, (long long)d->frame_stride, (long long)frame); return -3; }
    if (sb == 2) {
        if (g->pitch & 1) { set_error("%s: desc->row_pitch = %d must be a multiple of 2 with BSVD_PIX_P010", fn, d->row_pitch); return -3; }
        if (g->fstride & 1) { set_error("%s: desc->frame_stride = %lld must be a multiple of 2 with BSVD_PIX_P010", fn, (long long)d->frame_stride); return -3; }
        if ((uintptr_t)yuv & 1) { set_error("%s: %s must be 2-byte aligned with BSVD_PIX_P010", fn, yuv_name); return -3; }
    }
    if ((uintptr_t)planar & 15) { set_error("%s: %s must be 16-byte aligned (rows move as float4)", fn, planar_name); return -3; }
    const int64_t per_frame = (int64_t)(H / 2) * (pad ? items_per_row(W) : W / 4);
    if (per_frame > 0x7fffffff) { set_error("%s: H x W = %d x %d: more than 2^31 items per frame", fn, H, W); return -3; }
    g->items = per_frame * frames;
    return 0;
}

static YuvDecode decode_constants(const BsvdYuvDesc *desc)
{
    const int bits = desc->pix_fmt == BSVD_PIX_P010 ? 10 : 8;
    const double s = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
    const double kr = kMatrix[desc->matrix][0], kb = kMatrix[desc->matrix][1], kg = 1.0 - kr - kb;
    YuvDecode k;
    k.y_off = desc->full_range ? 0.f : (float)(16 * s);
    k.y_mul = (float)(1.0 / (desc->full_range ? top : 219 * s));
    k.c_off = desc->full_range ? (float)(1 << (bits - 1)) : (float)(128 * s);
    k.c_mul = (float)(1.0 / (desc->full_range ? top : 224 * s));
    k.r_cr = (float)(2 * (1 - kr));
    k.g_cr = (float)(2 * kr * (1 - kr) / kg);
    k.g_cb = (float)(2 * kb * (1 - kb) / kg);
    k.b_cb = (float)(2 * (1 - kb));
    return k;
}

static YuvEncode encode_constants(const BsvdYuvDesc *desc)
{
    const int bits = desc->pix_fmt == BSVD_PIX_P010 ? 10 : 8;
    const double s = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
    const double kr = kMatrix[desc->matrix][0], kb = kMatrix[desc->matrix][1], kg = 1.0 - kr - kb;
    const double cs = desc->full_range ? top : 224 * s;
    YuvEncode k;
    k.kr = (float)kr; k.kg = (float)kg; k.kb = (float)kb;
    k.y_mul = (float)(desc->full_range ? top : 219 * s);
    k.y_off = desc->full_range ? 0.f : (float)(16 * s);
    k.cb_mul = (float)(cs / (2 * (1 - kb)));
    k.cr_mul = (float)(cs / (2 * (1 - kr)));
    k.c_off = desc->full_range ? (float)(1 << (bits - 1)) : (float)(128 * s);
    k.y_lo = k.c_lo = desc->full_range ? 0.f : (float)(16 * s);
    k.y_hi = desc->full_range ? (float)top : (float)(235 * s);
    k.c_hi = desc->full_range ? (float)top : (float)(240 * s);
    return k;
}

static int64_t yuv_bytes(int32_t H, int32_t W, int32_t pix_fmt, int32_t row_pitch, int mask)
{
    if (H <= 0 || W <= 0 || (H & mask) || (W & mask) || (pix_fmt != BSVD_PIX_NV12 && pix_fmt != BSVD_PIX_P010) || row_pitch < 0) return -1;
    const int sb = sample_bytes(pix_fmt);
    const int64_t pitch = row_pitch ? row_pitch : (int64_t)W * sb;
    if (pitch < (int64_t)W * sb || (pitch & (sb - 1))) return -1;
    return pitch * H / 2 * 3;
}

}  // namespace bsvd

using namespace bsvd;

extern "C" {

int64_t bsvd_yuv420_frame_bytes(int32_t H, int32_t W, int32_t pix_fmt, int32_t row_pitch) { return yuv_bytes(H, W, pix_fmt, row_pitch, 3); }
int64_t bsvd_yuv420_picture_bytes(int32_t H, int32_t W, int32_t pix_fmt, int32_t row_pitch) { return yuv_bytes(H, W, pix_fmt, row_pitch, 1); }

int bsvd_yuv420_to_planar(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, const BsvdYuvDesc *desc, int32_t const_channels,
                          float const_value, void *stream)
{
    YuvGeom g;
    const int rc = yuv_check("bsvd_yuv420_to_planar", src, "src", dst, "dst", frames, H, W, desc, &g);
    if (rc) return rc;
    if (const_channels < 0) { set_error("bsvd_yuv420_to_planar: const_channels = %d must not be negative", const_channels); return -3; }
    const YuvDecode k = decode_constants(desc);
    const int sel = desc->pix_fmt * 2 + desc->chroma;
    static decltype(&yuv420_to_planar_kernel<BSVD_PIX_NV12, 0>) const kernels[4] = {yuv420_to_planar_kernel<BSVD_PIX_NV12, 0>, yuv420_to_planar_kernel<BSVD_PIX_NV12, 1>,
        yuv420_to_planar_kernel<BSVD_PIX_P010, 0>, yuv420_to_planar_kernel<BSVD_PIX_P010, 1>};
    return launch_sweep(kernels[sel], g.items, stream, (const uint8_t *)src, dst, H, W, g.pitch, g.fstride, const_channels, const_value, k, g.items);
}

int bsvd_planar_to_yuv420(const float *src, void *dst, int32_t frames, int32_t H, int32_t W, const BsvdYuvDesc *desc, void *stream)
{
    YuvGeom g;
    const int rc = yuv_check("bsvd_planar_to_yuv420", dst, "dst", src, "src", frames, H, W, desc, &g);
    if (rc) return rc;
    const YuvEncode k = encode_constants(desc);
    const int sel = desc->pix_fmt * 2 + desc->chroma;
    static decltype(&planar_to_yuv420_kernel<BSVD_PIX_NV12, 0>) const kernels[4] = {planar_to_yuv420_kernel<BSVD_PIX_NV12, 0>, planar_to_yuv420_kernel<BSVD_PIX_NV12, 1>,
        planar_to_yuv420_kernel<BSVD_PIX_P010, 0>, planar_to_yuv420_kernel<BSVD_PIX_P010, 1>};
    return launch_sweep(kernels[sel], g.items, stream, src, (uint8_t *)dst, H, W, g.pitch, g.fstride, k, g.items);
}

int bsvd_yuv420_to_planar_pad(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp, const BsvdYuvDesc *desc,
                              int32_t const_channels, float const_value, void *stream)
{
    YuvGeom g;
    const int rc = yuv_check("bsvd_yuv420_to_planar_pad", src, "src", dst, "dst", frames, H, W, desc, &g, 1, Hp, Wp);
    if (rc) return rc;
    if (const_channels < 0) { set_error("bsvd_yuv420_to_planar_pad: const_channels = %d must not be negative", const_channels); return -3; }
    const YuvPadGeom pg = {H, W, Hp, Wp, const_channels, g.pitch, g.fstride, const_value};
    const int sel = desc->pix_fmt * 2 + desc->chroma;
    static decltype(&yuv420_to_planar_pad_kernel<BSVD_PIX_NV12, 0>) const kernels[4] = {yuv420_to_planar_pad_kernel<BSVD_PIX_NV12, 0>, yuv420_to_planar_pad_kernel<BSVD_PIX_NV12, 1>,
        yuv420_to_planar_pad_kernel<BSVD_PIX_P010, 0>, yuv420_to_planar_pad_kernel<BSVD_PIX_P010, 1>};
    return launch_sweep(kernels[sel], g.items, stream, (const uint8_t *)src, dst, pg, decode_constants(desc), g.items);
}

int bsvd_planar_to_yuv420_crop(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W, const BsvdYuvDesc *desc,
                               void *stream)
{
    YuvGeom g;
    const int rc = yuv_check("bsvd_planar_to_yuv420_crop", dst, "dst", src, "src", frames, H, W, desc, &g, 1, Hp, Wp);
    if (rc) return rc;
    const YuvPadGeom pg = {H, W, Hp, Wp, 0, g.pitch, g.fstride, 0.f};
    const int sel = desc->pix_fmt * 2 + desc->chroma;
    static decltype(&planar_to_yuv420_crop_kernel<BSVD_PIX_NV12, 0>) const kernels[4] = {planar_to_yuv420_crop_kernel<BSVD_PIX_NV12, 0>, planar_to_yuv420_crop_kernel<BSVD_PIX_NV12, 1>,
        planar_to_yuv420_crop_kernel<BSVD_PIX_P010, 0>, planar_to_yuv420_crop_kernel<BSVD_PIX_P010, 1>};
    return launch_sweep(kernels[sel], g.items, stream, src, (uint8_t *)dst, pg, encode_constants(desc), g.items);
}

}  // extern "C"
